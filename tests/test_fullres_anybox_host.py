"""CPU: the any-size box feature's numpy restatement (tests/fullres_anybox_emulation.py) held to independent statements, and the
host side of its entries (csrc/gcfr_fullres_anybox.hip, postprocess.ingest_anybox_device / fullres_anybox_composites_device, the
inference.relight_*_in_photograph_anybox entries): every refusal is made before any launch, so it is exercised without a GPU.

  anchor    on boxes with both axes at least the network's, the ingest and the composites are tests/fullres_box_emulation.py's, bit
            for bit
  magnify   the ingest of a box smaller than the network is torch's bilinear interpolation in f64 over 255 within one f32 rounding
  minify    the carry of a plane onto a box smaller than the network is the f64 mean of the repeated-and-regrouped plane within
            per-axis budgets that add
  identity  rendered == x_lo under a full mask returns the photograph in every byte that neither `floor` nor the clamp touches
  outside   the box, and under a zero mask, nothing reaches the output -- not a NaN in `rendered` either"""
import ctypes

import numpy as np
import pytest
import torch

import fullres_anybox_emulation as anybox
import fullres_box_emulation as box

H5, W7 = 5, 7
# (bh, bw) over (5, 7): smaller on both axes, 1 x 1, one axis at the boundary, and lerp mixed with area both ways
SMALL_5x7 = [(1, 1), (4, 3), (3, 6), (2, 2), (5, 6), (4, 7)]
MIXED_5x7 = [(3, 9), (20, 2), (11, 6), (4, 28)]
LARGE_5x7 = [(5, 7), (6, 7), (13, 9), (17, 23), (40, 55), (11, 56)]


def _bits(a):
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


def resample_f64(a, n_out):
    """the independent statement of one axis (the last), in f64: towards MORE samples torch's linear interpolation at half-pixel
    centres; towards FEWER every value repeated n_out times, regrouped into n_out groups of n_in, and the mean taken"""
    import torch.nn.functional as Fn
    a = np.asarray(a, dtype=np.float64)
    n_in = a.shape[-1]
    if n_out >= n_in:
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(1, -1, n_in))
        return Fn.interpolate(t, size=n_out, mode="linear", align_corners=False).numpy().reshape(a.shape[:-1] + (n_out,))
    return np.repeat(a, n_out, axis=-1).reshape(a.shape[:-1] + (n_out, n_in)).mean(axis=-1)


def resample2_f64(a, rows, cols):
    """(..., r, c) -> (..., rows, cols) by `resample_f64` on each axis, columns first"""
    hz = resample_f64(a, cols)
    return np.swapaxes(resample_f64(np.swapaxes(hz, -1, -2), rows), -1, -2)


def test_on_boxes_no_smaller_than_the_network_the_restatement_is_the_box_restatement_bit_for_bit():
    rng = np.random.default_rng(1)
    for (h, w), sizes in (((H5, W7), LARGE_5x7), ((3, 5), [(3, 5), (4, 6), (7, 19), (10, 5), (24, 40)]), ((4, 8), [(5, 9), (15, 33), (4, 8)])):
        for bh, bw in sizes:
            Hp, Wp = bh + 4, bw + 5
            photo = rng.integers(0, 256, (2, Hp, Wp, 3), dtype=np.uint8)
            boxes = np.array([(3, 2, bw, bh), (5, 4, bw, bh)])
            x = anybox.ingest(photo, boxes, h, w)
            np.testing.assert_array_equal(_bits(x), _bits(box.ingest(photo, boxes, h, w)))
            a = rng.standard_normal((2, 3, h, w)).astype(np.float32)
            np.testing.assert_array_equal(_bits(anybox.carry(a, bh, bw)), _bits(box.up(a, bh, bw)))
            x_lo = (x * (0.1 + 1.9 * rng.random((2, h, w, 3), dtype=np.float32))).astype(np.float32)
            rendered = (0.5 + 1.5 * rng.standard_normal((2, 3, 3, h, w))).astype(np.float32)
            mask = rng.choice(np.array([0, 64, 128, 255], np.uint8), (2, h, w))
            for paste in (True, False):
                np.testing.assert_array_equal(anybox.composites(photo, boxes, x_lo, rendered, mask, paste=paste),
                                              box.composites(photo, boxes, x_lo, rendered, mask, paste=paste))
    # boxes of different sizes in one pasted call
    photo = rng.integers(0, 256, (3, 50, 64, 3), dtype=np.uint8)
    boxes = np.array([(0, 0, 7, 5), (3, 9, 23, 17), (8, 10, 56, 40)])
    x = anybox.ingest(photo, boxes, H5, W7)
    np.testing.assert_array_equal(_bits(x), _bits(box.ingest(photo, boxes, H5, W7)))
    rendered = (0.5 + 1.5 * rng.standard_normal((3, 2, 3, H5, W7))).astype(np.float32)
    mask = rng.choice(np.array([0, 64, 128, 255], np.uint8), (1, H5, W7))
    np.testing.assert_array_equal(anybox.composites(photo, boxes, x, rendered, mask), box.composites(photo, boxes, x, rendered, mask))


def test_the_magnifying_ingest_is_torchs_bilinear_in_f64_within_one_rounding():
    """The bound.  S and 255 Dy Dx are exact integers, so the restated value is the exact rational S / (255 Dy Dx) in [0, 1] after
    one f64 division (relative 2^-53) and ONE rounding to f32: at most half an ulp of a value in [1/2, 1], 2^-25.  The reference
    (torch's interpolation in f64, divided by 255) forms its source coordinate and two products in f64: below 2^-40 for the sizes
    here, which is added.  A constant photograph leaves no rounding at all: S = c Dy Dx exactly, and (float)(c / 255.0) is what
    every other ingest of this library returns."""
    bound = 2.0 ** -25 + 2.0 ** -40
    rng = np.random.default_rng(2)
    worst = 0.0
    cases = (((H5, W7), SMALL_5x7 + MIXED_5x7), ((23, 17), [(3, 3), (22, 16), (9, 11), (3, 40), (50, 5), (13, 17)]), ((64, 48), [(37, 29), (8, 6)]))
    for (h, w), sizes in cases:
        for bh, bw in sizes:
            crop = rng.integers(0, 256, (bh, bw, 3), dtype=np.uint8)
            got = anybox.ingest_crop(crop, h, w)
            assert got.shape == (h, w, 3) and got.dtype == np.float32
            want = np.moveaxis(resample2_f64(np.moveaxis(crop.astype(np.float64), 2, 0), h, w), 0, 2) / 255.0
            err = float(np.abs(got.astype(np.float64) - want).max())
            print("(%d,%d) -> (%d,%d): max |ingest - f64| %.3g = %.3f x 2^-25" % (bh, bw, h, w, err, err * 2.0 ** 25))
            worst = max(worst, err)
            assert err <= bound
            for c in (0, 1, 37, 128, 255):
                const = anybox.ingest_crop(np.full((bh, bw, 3), c, np.uint8), h, w)
                assert (_bits(const) == _bits(np.array([c / 255.0], np.float32))[0]).all(), (c, bh, bw)
    print("worst %.3g, bound %.3g" % (worst, bound))
    # through the whole-photograph entry of the restatement, at an origin
    photo = rng.integers(0, 256, (1, 9, 11, 3), dtype=np.uint8)
    np.testing.assert_array_equal(_bits(anybox.ingest(photo, (4, 3, 3, 4), H5, W7)[0]), _bits(anybox.ingest_crop(photo[0, 3:7, 4:7], H5, W7)))


def test_the_minifying_carry_is_the_mean_of_the_repeated_plane():
    """The bound, with u = 2^-24 and planes in [0, 1).  An AREA axis: the weights are exact integers that sum to n and every product
    (double)wt (double)v is exact; the at most nine f64 additions and the division each round by 2^-53 of a value below n, under
    2^-40 in all; the one rounding of the quotient (in [0, 1)) to f32 is at most u / 2, budgeted as u.  A LERP axis: 2 u
    (tests/test_fullres_box_host.py derives it).  The horizontal results reach the vertical operator through non-negative weights
    that sum to one, a convex combination of their errors, and the vertical operator adds its own budget: the budgets of the two
    axes add.  The f64 reference rounds far below 2^-40."""
    u = 2.0 ** -24
    budget = lambda nb, n: 2.0 * u if nb >= n else u + 2.0 ** -40
    rng = np.random.default_rng(3)
    worst = 0.0
    cases = (((H5, W7), SMALL_5x7 + MIXED_5x7), ((23, 17), [(3, 3), (22, 16), (9, 11), (3, 40), (50, 5), (23, 16)]), ((4, 8), [(1, 1), (3, 4), (2, 20)]))
    for (h, w), sizes in cases:
        a = rng.random((2, 3, h, w), dtype=np.float32)
        for bh, bw in sizes:
            got = anybox.carry(a, bh, bw)
            assert got.shape == (2, 3, bh, bw) and got.dtype == np.float32
            err = float(np.abs(got.astype(np.float64) - resample2_f64(a, bh, bw)).max())
            bound = budget(bh, h) + budget(bw, w)
            print("(%d,%d) -> (%d,%d): max |carry - f64| %.3g = %.2f x 2^-24, bound %.2f x 2^-24" % (h, w, bh, bw, err, err / u, bound / u))
            worst = max(worst, err / bound)
            assert err <= bound
            # a constant plane is carried exactly, also one that is not a dyadic number
            assert (anybox.carry(np.full((h, w), np.float32(0.1)), bh, bw) == np.float32(0.1)).all()
    print("worst: %.2f of its bound" % worst)


def _smooth_photograph(rng, Hp, Wp):
    y, x = np.mgrid[0:Hp, 0:Wp]
    base = 120.0 + 30.0 * np.sin(y / 9.0)[..., None] + 25.0 * np.cos(x[..., None] / 7.0 + np.arange(3))
    return np.clip(np.rint(base + rng.integers(-6, 7, (Hp, Wp, 3))), 0, 255).astype(np.uint8)[None]


def test_identity_rendered_equal_to_x_lo_returns_the_photograph():
    rng = np.random.default_rng(5)
    total = qualifying = 0
    for bh, bw in SMALL_5x7 + MIXED_5x7 + [(20, 2), (3, 9)]:
        Hp, Wp = bh + 4, bw + 5
        photo = _smooth_photograph(rng, Hp, Wp)
        b = (3, 2, bw, bh)
        crop = photo[0, 2:2 + bh, 3:3 + bw]
        x_lo = anybox.ingest(photo, b, H5, W7)
        rendered = np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2)))[:, None]
        mask = np.full((1, H5, W7), 255, np.uint8)
        _, m, _, xl = anybox.box_terms(crop, x_lo[0], rendered[0], mask[0])
        assert (m == np.float32(1.0)).all()
        with np.errstate(divide="ignore"):
            quotient = crop.astype(np.float32) / np.fmax(xl, np.float32(1.0))
        ok = (xl >= np.float32(1.0)) & (quotient > np.float32(0.25)) & (quotient < np.float32(4.0))
        got = anybox.composites(photo, b, x_lo, rendered, mask, paste=False)
        assert got.shape == (1, 1, bh, bw, 3) and got.dtype == np.uint8
        total += ok.size
        qualifying += int(ok.sum())
        np.testing.assert_array_equal(got[0, 0][ok], crop[ok])
        pasted = anybox.composites(photo, b, x_lo, rendered, mask)[0, 0]
        np.testing.assert_array_equal(pasted[2:2 + bh, 3:3 + bw], got[0, 0])
        outside = np.ones((Hp, Wp), bool)
        outside[2:2 + bh, 3:3 + bw] = False
        np.testing.assert_array_equal(pasted[outside], photo[0][outside])
    print("identity: %d of %d bytes qualify (%.1f %%)" % (qualifying, total, 100.0 * qualifying / total))
    assert qualifying >= 0.95 * total                                              # a condition on the input, not a tolerance


def test_outside_the_box_and_under_a_zero_mask_nothing_reaches_the_output():
    rng = np.random.default_rng(6)
    h, w, Hp, Wp = 5, 7, 17, 22
    for bh, bw in ((3, 4), (3, 13), (10, 4)):
        photo = rng.integers(0, 256, (2, Hp, Wp, 3), dtype=np.uint8)
        boxes = np.array([(4, 3, bw, bh), (9, 7, bw, bh)])
        x_lo = anybox.ingest(photo, boxes, h, w)
        rendered = np.full((2, 2, 3, h, w), np.nan, np.float32)
        mask = np.zeros((1, h, w), np.uint8)
        mask[0, 1, 2] = 255
        got = anybox.composites(photo, boxes, x_lo, rendered, mask)
        m = anybox.carry(mask[0].astype(np.float32) / np.float32(255.0), bh, bw)
        assert 0 < (m > 0).sum() < m.size
        for b, (x0, y0, _, _) in enumerate(boxes):
            relit = np.zeros((Hp, Wp), bool)
            relit[y0:y0 + bh, x0:x0 + bw] = m > 0
            assert (got[b][:, relit] == 0).all()                                   # NaN -> 0 inside the box and the mask
            np.testing.assert_array_equal(got[b][:, ~relit], np.broadcast_to(photo[b][~relit], got[b][:, ~relit].shape))
        alone = anybox.composites(photo, boxes, x_lo, rendered, mask, paste=False)
        for b, (x0, y0, _, _) in enumerate(boxes):
            np.testing.assert_array_equal(alone[b], got[b][:, y0:y0 + bh, x0:x0 + bw])
        # an all-zero mask: the photograph, whatever `rendered` holds
        zero = np.zeros((1, h, w), np.uint8)
        np.testing.assert_array_equal(anybox.composites(photo, boxes, x_lo, rendered, zero), np.stack([photo, photo], axis=1))


# ------------------------------------------------------------------------------------------------
# the entries' host side
# ------------------------------------------------------------------------------------------------
def _host_boxes(rows):
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 4))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_the_c_entries_refuse_before_any_launch():
    """junk device pointers throughout: every call below must return before it launches"""
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = lambda v: ctypes.c_void_p(v)
    # a (17, 23) network: a 5 x 4 box is allowed (8 x 5 >= 23, 8 x 4 >= 17), a 2-wide or 2-high one is not
    ok = dict(photo=p(1 << 20), x_lo=p(128), rendered=p(256), mask=p(512), mask_batch=1, B=2, L=3, Hp=30, Wp=40, h=17, w=23, paste=1,
              floor=1.0, clamp=4.0, out=p(1 << 30), boxes=[(3, 2, 5, 4), (20, 15, 5, 4)])

    def comp(**kw):
        a = dict(ok, **kw)
        keep, bp = (None, None) if a["boxes"] is None else _host_boxes(a["boxes"])
        return L.gcfr_fullres_composites_anybox_u8(a["photo"], a["x_lo"], a["rendered"], a["mask"], a["mask_batch"], a["B"], a["L"],
                                                   a["Hp"], a["Wp"], bp, a["h"], a["w"], a["paste"], a["floor"], a["clamp"], a["out"], None)

    def ing(**kw):
        a = dict(ok, **kw)
        keep, bp = (None, None) if a["boxes"] is None else _host_boxes(a["boxes"])
        return L.gcfr_ingest_anybox_u8(a["photo"], a["B"], a["Hp"], a["Wp"], bp, a["h"], a["w"], a["x_lo"], None)

    for name in ("photo", "x_lo", "rendered", "mask", "out", "boxes"):
        assert comp(**{name: None}) == -1, name
    for name in ("photo", "x_lo", "boxes"):
        assert ing(**{name: None}) == -1, name
    second = lambda *b: [(3, 2, 5, 4), b]
    bad_boxes = [second(-1, 15, 5, 4), second(20, -1, 5, 4), second(36, 15, 5, 4), second(20, 27, 5, 4),               # outside
                 second(20, 15, 2, 4), second(20, 15, 5, 2), second(20, 15, 2, 30 - 15), second(20, 15, 40 - 20, 2),   # 8 nb < n
                 second(20, 15, 0, 4), second(20, 15, 5, 0), second(20, 15, 0, 0), second(20, 15, -5, 4),             # nb < 1
                 second(0, 0, 41, 4), second(0, 0, 5, 31), second(2 ** 31 - 4, 0, 5, 4)]
    for b in bad_boxes:
        for paste in (0, 1):
            assert comp(boxes=b, paste=paste) == -1, b
        assert ing(boxes=b) == -1, b
    # the FIRST face's box is checked like every other
    assert comp(boxes=[(38, 2, 5, 4), (20, 15, 5, 4)]) == -1 and ing(boxes=[(3, 2, 5, 2), (20, 15, 5, 4)]) == -1
    # 2 bh h, 2 bw w in 31 bits: on a lerp axis and on an area axis (8 nb >= n holds in all four)
    tall = dict(B=1, Hp=1 << 15, Wp=1, h=1 << 15, w=1, boxes=[(0, 0, 1, 1 << 15)])
    wide = dict(B=1, Hp=1, Wp=1 << 15, h=1, w=1 << 15, boxes=[(0, 0, 1 << 15, 1)])
    short = dict(B=1, Hp=1 << 14, Wp=1, h=1 << 16, w=1, boxes=[(0, 0, 1, 1 << 14)])
    narrow = dict(B=1, Hp=1, Wp=1 << 14, h=1, w=1 << 16, boxes=[(0, 0, 1 << 14, 1)])
    for d in (tall, wide, short, narrow):
        assert comp(**d) == -1 and ing(**d) == -1
    # Hp Wp, and the chunk count, in 31 bits
    huge = dict(B=1, Hp=1 << 16, Wp=1 << 16, boxes=[(0, 0, 5, 4)])
    assert comp(**huge) == -1 and ing(**huge) == -1
    many = dict(B=1 << 12, Hp=1 << 15, Wp=1 << 15, boxes=[(0, 0, 5, 4)] * (1 << 12))
    assert comp(**many) == -1 and ing(**many) == -1
    assert comp(B=0) == -1 and comp(h=0) == -1 and comp(w=0) == -1 and comp(Hp=0) == -1 and comp(Wp=-1) == -1
    assert ing(B=0) == -1 and ing(h=0) == -1 and ing(w=-1) == -1 and ing(Hp=0) == -1 and ing(Wp=0) == -1
    # paste, and boxes of different sizes without it
    assert comp(paste=2) == -1 and comp(paste=-1) == -1
    assert comp(paste=0, boxes=[(3, 2, 5, 4), (20, 15, 6, 4)]) == -1 and comp(paste=0, boxes=[(3, 2, 5, 4), (20, 15, 5, 5)]) == -1
    # what gcfr_fullres_composites_u8 refuses
    assert comp(L=0) == -1 and comp(L=4097) == -1 and comp(L=-1) == -1
    assert comp(mask_batch=0) == -1 and comp(mask_batch=3) == -1
    assert comp(clamp=0.99) == -1 and comp(clamp=float("nan")) == -1
    assert comp(floor=0.0) == -1 and comp(floor=-1.0) == -1 and comp(floor=float("nan")) == -1
    # an out that overlaps the photographs (2 x 30 x 40 x 3 = 7200 bytes from 1 << 20; out is 3 x 7200 bytes pasted and
    # 2 x 3 x 4 x 5 x 3 = 360 not)
    for out in ((1 << 20), (1 << 20) + 7199, (1 << 20) - 1, (1 << 20) - 3 * 7200 + 1):
        assert comp(out=p(out)) == -1, out
    for out in ((1 << 20), (1 << 20) + 7199, (1 << 20) - 360 + 1):
        assert comp(out=p(out), paste=0) == -1, out
    assert ing(x_lo=p(1 << 20)) == -1                                             # x_lo_out == photo


def test_the_python_entries_refuse_malformed_operands_without_a_gpu():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    B, L, h, w, Hp, Wp = 2, 3, 17, 23, 30, 40
    photo = torch.zeros((B, Hp, Wp, 3), dtype=torch.uint8)
    x_lo = torch.zeros((B, h, w, 3))
    rendered = torch.zeros((B, L, 3, h, w))
    mask = torch.zeros((h, w), dtype=torch.uint8)
    boxes = [(3, 2, 5, 4), (20, 15, 5, 4)]
    bad_boxes = [[(3, 2, 5, 4)], [(3, 2, 5, 4)] * 3, (3, 2, 5), [(3.0, 2.0, 5.0, 4.0)] * 2, np.zeros((B, 4), np.float32),
                 torch.tensor(boxes, dtype=torch.float32), np.array(boxes, dtype=bool), "box", None,
                 (-1, 2, 5, 4), (3, -1, 5, 4), (36, 2, 5, 4), (3, 27, 5, 4), (3, 2, 2, 4), (3, 2, 5, 2), (3, 2, 0, 4), (3, 2, 5, 0),
                 (3, 2, -5, 4), (0, 0, 41, 4), (0, 0, 5, 31)]
    bad = [dict(boxes=b) for b in bad_boxes] + [
        dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(photo_u8=photo.numpy()), dict(photo_u8=photo[..., :2]),
        dict(x_lo=x_lo[:1]), dict(x_lo=x_lo.double()), dict(x_lo=x_lo.permute(0, 3, 1, 2)), dict(x_lo=x_lo[0]),
        dict(rendered=rendered[:, :, :2]), dict(rendered=rendered[:1]), dict(rendered=rendered[0, 0]), dict(rendered=rendered.to(torch.int32)),
        dict(rendered=torch.zeros((B, 0, 3, h, w))), dict(rendered=torch.zeros((B, Hp, Wp, 3))),
        dict(mask_u8=mask.float()), dict(mask_u8=torch.zeros((4, 5), dtype=torch.uint8)), dict(mask_u8=torch.zeros((3, h, w), dtype=torch.uint8)),
        dict(detail_clamp=0.5), dict(detail_clamp=float("nan")), dict(floor=0.0), dict(floor=-2.0),
        dict(paste=2), dict(paste="yes"), dict(paste=None),
        dict(paste=False, boxes=[(3, 2, 5, 4), (20, 15, 6, 4)]),
        dict(out=torch.zeros((B, L, Hp, Wp, 3))), dict(out=torch.zeros((B, Hp, Wp, 3), dtype=torch.uint8)),
        dict(out=torch.zeros((B, L, 4, 5, 3), dtype=torch.uint8)), dict(paste=False, out=torch.zeros((B, L, Hp, Wp, 3), dtype=torch.uint8)),
    ]
    for kw in bad:
        a = dict(photo_u8=photo, boxes=boxes, x_lo=x_lo, rendered=rendered, mask_u8=mask)
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.fullres_anybox_composites_device(**a)
    with pytest.raises(TypeError):                                                 # no guided carrying over small boxes
        pp.fullres_anybox_composites_device(photo, boxes, x_lo, rendered, mask, upsample="guided")
    # 2 bh h in 31 bits, through Python
    with pytest.raises(GcfrError, match="31 bits"):
        pp.ingest_anybox_device(torch.zeros((1, 1 << 14, 1, 3), dtype=torch.uint8), (0, 0, 1, 1 << 14), (1 << 16, 1))
    # well-formed host tensors, boxes as a list, an array, a CPU tensor or one box for every face: there is no CPU path
    for b in (boxes, np.array(boxes), np.array(boxes, dtype=np.uint16), torch.tensor(boxes), (3, 2, 5, 4), (3, 2, 30, 4), (0, 0, 40, 30)):
        for paste in (True, False):
            with pytest.raises(GcfrError, match="no CPU path"):
                pp.fullres_anybox_composites_device(photo, b, x_lo, rendered, mask, paste=paste)
        with pytest.raises(GcfrError, match="no CPU path"):
            pp.ingest_anybox_device(photo, b, (h, w))
    with pytest.raises(GcfrError, match="no CPU path"):
        pp.ingest_anybox_device(photo, (0, 0, 3, 3), 23)                           # an int: a square network
    for kw in [dict(boxes=b) for b in bad_boxes] + [dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(size=0), dict(size=(5,)),
                                                    dict(size=(5.0, 7.0)), dict(size=(5, 7, 3)), dict(size=None), dict(size=(33, 23)),
                                                    dict(size=(17, 41))]:
        a = dict(photo_u8=photo, boxes=boxes, size=(h, w))
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.ingest_anybox_device(**a)
    # the existing entries keep refusing what the new ones take
    with pytest.raises(GcfrError, match="smaller than the network"):
        pp.ingest_box_device(photo, boxes, (h, w))


def test_the_inference_entries_exist_and_refuse_malformed_operands():
    import inspect
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd._lib import GcfrError
    names = ("relight_lights_in_photograph_anybox", "relight_lights_in_photograph_anybox_device", "relight_rig_in_photograph_anybox",
             "relight_rig_in_photograph_anybox_device")
    for name in names:
        sig = inspect.signature(getattr(inf, name))
        assert "upsample" not in sig.parameters and sig.parameters["paste"].default is True
    mask = np.zeros((17, 23), np.uint8)
    with pytest.raises(GcfrError, match="uint8"):
        inf.relight_lights_in_photograph_anybox_device(None, np.zeros((1, 30, 40, 3), np.float32), (3, 2, 5, 4), mask, None, device="cpu")
    photos = np.zeros((1, 30, 40, 3), np.uint8)
    for b in ((3, 2, 2, 4), (3, 2, 5, 2), (3, 2, 0, 4), (38, 2, 5, 4), (3.0, 2.0, 5.0, 4.0), [(3, 2, 5, 4)] * 2):
        with pytest.raises(GcfrError):
            inf.relight_lights_in_photograph_anybox_device(None, photos, b, mask, None, device="cpu")
        with pytest.raises(GcfrError):
            inf.relight_rig_in_photograph_anybox_device(None, photos, b, mask, None, None, device="cpu")
        with pytest.raises(GcfrError):
            inf.relight_lights_in_photograph_anybox(None, photos, b, mask, None, device="cpu")
        with pytest.raises(GcfrError):
            inf.relight_rig_in_photograph_anybox(None, photos, b, mask, None, None, device="cpu")
    with pytest.raises(GcfrError, match="mask_u8"):
        inf.relight_lights_in_photograph_anybox_device(None, photos, (3, 2, 5, 4), np.zeros((2, 17, 23), np.uint8), None, device="cpu")
    for b in ((3, 2, 5, 4), (3, 2, 30, 4), (3, 2, 5, 20)):                         # small and mixed boxes pass every check
        with pytest.raises(GcfrError, match="no CPU path"):
            inf.relight_lights_in_photograph_anybox_device(None, photos, b, mask, None, device="cpu")
