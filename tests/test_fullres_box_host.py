"""CPU: the box feature's numpy restatement (tests/fullres_box_emulation.py) held to independent statements, and the host side of
the two entries (csrc/gcfr_fullres_box.hip, postprocess.ingest_box_device / fullres_box_composites_device, the
inference.relight_*_in_photograph entries): every refusal is made before any launch, so it is exercised without a GPU.

  anchor    with the box the whole photograph and s in {1, 2, 4, 8} the ingest, the taps and Up are tests/fullres_emulation.py's, bit
            for bit: the box statement is a strict generalisation of the power-of-two one
  ingest    the repeat-and-sum integer equals the statement's overlap-weight sum on boxes of non-integer ratio; a constant
            photograph c ingests to np.float32(c / 255.0) exactly
  Up        a constant field is returned exactly; within 4 x 2^-24 of torch's bilinear interpolation in f64 (derived below)
  identity  rendered == x_lo with no pixel clamped returns the photograph in every byte
  outside   the box, and under a zero mask, nothing reaches the output -- not a NaN in `rendered` either"""
import ctypes

import numpy as np
import pytest
import torch

import fullres_box_emulation as box
import fullres_emulation as emu

# (bh, bw) over (h, w) = (5, 7): ratio 1, one row more, non-integer both ways, just under and just over 8 (39 / 5, 50 / 7; 40 / 5,
# 55 / 7), and an anisotropic one (11 / 5 = 2.2 by 56 / 7 = 8)
H5, W7 = 5, 7
BOXES_5x7 = [(5, 7), (6, 7), (13, 9), (17, 23), (39, 50), (40, 55), (11, 56)]


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_a_whole_photograph_power_of_two_box_is_the_fullres_statement_bit_for_bit(s):
    rng = np.random.default_rng(s)
    for h, w in [(5, 7), (3, 5), (4, 8), (1, 1), (20, 28)]:
        photo = rng.integers(0, 256, (2, s * h, s * w, 3), dtype=np.uint8)
        whole = (0, 0, s * w, s * h)
        np.testing.assert_array_equal(box.ingest(photo, whole, h, w).view(np.uint32), emu.ingest(photo, s).view(np.uint32))
        for n in (h, w):
            i0, i1, t = box.taps(s * n, n)
            j0, j1, u = emu.taps(s * n, s, n)
            np.testing.assert_array_equal(i0, j0)
            np.testing.assert_array_equal(i1, j1)
            assert t.dtype == u.dtype == np.float32
            np.testing.assert_array_equal(t.view(np.uint32), u.view(np.uint32))
        a = rng.standard_normal((2, 3, h, w)).astype(np.float32)
        np.testing.assert_array_equal(box.up(a, s * h, s * w).view(np.uint32), emu.up(a, s).view(np.uint32))
        # and the composite, pasted or not
        x_lo = (emu.ingest(photo, s) * (0.1 + 1.9 * rng.random((2, h, w, 3), dtype=np.float32))).astype(np.float32)
        rendered = (0.5 + 1.5 * rng.standard_normal((2, 3, 3, h, w))).astype(np.float32)
        mask = rng.choice(np.array([0, 64, 128, 255], np.uint8), (2, h, w))
        want = emu.composites(photo, x_lo, rendered, mask, s)
        np.testing.assert_array_equal(box.composites(photo, whole, x_lo, rendered, mask), want)
        np.testing.assert_array_equal(box.composites(photo, whole, x_lo, rendered, mask, paste=False), want)


def test_the_repeat_and_sum_ingest_is_the_overlap_weight_sum():
    rng = np.random.default_rng(2)
    for (h, w), sizes in (((H5, W7), BOXES_5x7), ((3, 5), [(3, 5), (4, 6), (7, 19), (10, 5)]), ((4, 8), [(5, 9), (15, 33)])):
        for bh, bw in sizes:
            crop = rng.integers(0, 256, (bh, bw, 3), dtype=np.uint8)
            S = box.area_sum(crop, h, w)
            assert S.dtype == np.int64 and S.shape == (h, w, 3)
            np.testing.assert_array_equal(S, box.overlap_sum(crop, h, w))
            # the weights of one axis: each low-resolution cell weighs n_box, each box pixel n_lo, none outside [0, n_lo]
            for n_box, n_lo in ((bh, h), (bw, w)):
                wgt = box.overlap(n_box, n_lo)
                assert (wgt.sum(axis=1) == n_box).all() and (wgt.sum(axis=0) == n_lo).all() and wgt.min() >= 0 and wgt.max() <= n_lo
            assert int(S.sum()) == h * w * int(crop.astype(np.int64).sum())


def test_a_constant_photograph_ingests_and_comes_back_exactly():
    for c in (0, 1, 37, 128, 254, 255):
        for bh, bw in BOXES_5x7:
            photo = np.full((1, bh + 3, bw + 2, 3), c, np.uint8)
            x = box.ingest(photo, (1, 2, bw, bh), H5, W7)
            assert x.dtype == np.float32 and (x.view(np.uint32) == np.float32(c / 255.0).view(np.uint32)).all(), (c, bh, bw)
    # Up returns a constant field exactly, also one that is not a dyadic number
    f = np.full((2, H5, W7), np.float32(0.1))
    for bh, bw in BOXES_5x7:
        assert (box.up(f, bh, bw) == np.float32(0.1)).all()


def test_up_is_torchs_bilinear_in_f64():
    """The bound, with u = 2^-24 and planes in [0, 1).  The taps are exact integers and t = rem / (2 n) < 1 is rounded once: |dt| <=
    u / 2.  One lerp a0 + t (a1 - a0) of operands in [0, 1): the difference (|.| < 1) rounds by at most u / 2 and is then scaled
    by t <= 1; the error of t scales |a1 - a0| < 1: u / 2; the product (|.| < 1) rounds by u / 2; the sum (in [0, 1]) rounds by
    u / 2: at most 2 u per lerp.  The two horizontal lerps reach the vertical one as a convex combination of their errors, 2 u,
    and the vertical lerp adds its own 2 u: 4 u = 4 x 2^-24 = 2.4e-7, plus second-order terms and the f64 reference's own rounding,
    both below 2^-40.  (Measured: about 1.7 u.)"""
    import torch.nn.functional as Fn
    bound = 4.0 * 2.0 ** -24 + 2.0 ** -40
    rng = np.random.default_rng(3)
    worst = 0.0
    for (h, w), sizes in (((H5, W7), BOXES_5x7), ((3, 5), [(3, 5), (7, 19), (10, 5), (64, 77)]), ((20, 28), [(20, 28), (53, 97)])):
        a = rng.random((2, 3, h, w), dtype=np.float32)
        for bh, bw in sizes:
            want = Fn.interpolate(torch.from_numpy(a).to(torch.float64), size=(bh, bw), mode="bilinear", align_corners=False).numpy()
            got = box.up(a, bh, bw)
            assert got.shape == (2, 3, bh, bw) and got.dtype == np.float32
            err = float(np.abs(got.astype(np.float64) - want).max())
            print("(%d,%d) -> (%d,%d): max |Up - interpolate_f64| %.3g = %.2f x 2^-24" % (h, w, bh, bw, err, err * 2.0 ** 24))
            worst = max(worst, err)
            assert err <= bound
    print("worst %.3g, bound %.3g" % (worst, bound))


def _levels(rng, level, MB, h, w):
    m = np.full((MB, h, w), level, np.uint8)
    m[rng.random((MB, h, w)) < 0.2] = 0
    return m


def test_identity_rendered_equal_to_x_lo_returns_the_photograph():
    rng = np.random.default_rng(5)
    total = differing = 0
    for level in (255, 64, 1):
        for bh, bw in BOXES_5x7:
            Hp, Wp = bh + 4, bw + 5
            photo = rng.integers(64, 193, (1, Hp, Wp, 3), dtype=np.uint8)
            b = (3, 2, bw, bh)
            x_lo = box.ingest(photo, b, H5, W7)
            rendered = np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2)))[:, None]
            mask = _levels(rng, level, 1, H5, W7)
            _, _, d = box.box_values(photo[0, 2:2 + bh, 3:3 + bw], x_lo[0], rendered[0], mask[0])
            assert d.min() > 0.25 and d.max() < 4.0                                # no pixel is clamped
            got = box.composites(photo, b, x_lo, rendered, mask, paste=False)
            assert got.shape == (1, 1, bh, bw, 3) and got.dtype == np.uint8
            total += got.size
            differing += int((got[0, 0] != photo[0, 2:2 + bh, 3:3 + bw]).sum())
            np.testing.assert_array_equal(box.composites(photo, b, x_lo, rendered, mask)[:, 0], photo)
    print("identity: %d of %d bytes differ" % (differing, total))
    assert total == 48159 and differing == 0


def test_outside_the_box_and_under_a_zero_mask_nothing_reaches_the_output():
    rng = np.random.default_rng(6)
    h, w, bh, bw, Hp, Wp = 3, 5, 10, 13, 17, 22
    photo = rng.integers(0, 256, (2, Hp, Wp, 3), dtype=np.uint8)
    boxes = np.array([(4, 3, bw, bh), (9, 7, bw, bh)])
    x_lo = box.ingest(photo, boxes, h, w)
    rendered = np.full((2, 2, 3, h, w), np.nan, np.float32)
    mask = np.zeros((1, h, w), np.uint8)
    mask[0, 1, 2] = 255
    got = box.composites(photo, boxes, x_lo, rendered, mask)
    m = box.up(mask[0].astype(np.float32) / np.float32(255.0), bh, bw)
    assert 0 < (m > 0).sum() < m.size
    for b, (x0, y0, _, _) in enumerate(boxes):
        relit = np.zeros((Hp, Wp), bool)
        relit[y0:y0 + bh, x0:x0 + bw] = m > 0
        assert (got[b][:, relit] == 0).all()                                       # NaN -> 0 inside the box and the mask
        np.testing.assert_array_equal(got[b][:, ~relit], np.broadcast_to(photo[b][~relit], got[b][:, ~relit].shape))
    # the box alone is the pasted photograph's box region
    alone = box.composites(photo, boxes, x_lo, rendered, mask, paste=False)
    for b, (x0, y0, _, _) in enumerate(boxes):
        np.testing.assert_array_equal(alone[b], got[b][:, y0:y0 + bh, x0:x0 + bw])


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
    ok = dict(photo=p(1 << 20), x_lo=p(128), rendered=p(256), mask=p(512), mask_batch=1, B=2, L=3, Hp=30, Wp=40, h=5, w=7, paste=1,
              floor=1.0, clamp=4.0, out=p(1 << 30), boxes=[(3, 2, 17, 11), (20, 15, 17, 11)])

    def comp(**kw):
        a = dict(ok, **kw)
        keep, bp = (None, None) if a["boxes"] is None else _host_boxes(a["boxes"])
        return L.gcfr_fullres_composites_box_u8(a["photo"], a["x_lo"], a["rendered"], a["mask"], a["mask_batch"], a["B"], a["L"], a["Hp"],
                                                a["Wp"], bp, a["h"], a["w"], a["paste"], a["floor"], a["clamp"], a["out"], None)

    def ing(**kw):
        a = dict(ok, **kw)
        keep, bp = (None, None) if a["boxes"] is None else _host_boxes(a["boxes"])
        return L.gcfr_ingest_box_u8(a["photo"], a["B"], a["Hp"], a["Wp"], bp, a["h"], a["w"], a["x_lo"], None)

    for name in ("photo", "x_lo", "rendered", "mask", "out", "boxes"):
        assert comp(**{name: None}) == -1, name
    for name in ("photo", "x_lo", "boxes"):
        assert ing(**{name: None}) == -1, name
    second = lambda *b: [(3, 2, 17, 11), b]
    bad_boxes = [second(-1, 15, 17, 11), second(20, -1, 17, 11), second(24, 15, 17, 11), second(20, 20, 17, 11),     # outside
                 second(20, 15, 6, 11), second(20, 15, 17, 4), second(20, 15, 0, 0), second(20, 15, -17, 11),       # smaller than (h, w)
                 second(0, 0, 41, 11), second(0, 0, 17, 31), second(2 ** 31 - 8, 0, 17, 11)]
    for b in bad_boxes:
        for paste in (0, 1):
            assert comp(boxes=b, paste=paste) == -1, b
        assert ing(boxes=b) == -1, b
    # the FIRST face's box is checked like every other
    assert comp(boxes=[(30, 2, 17, 11), (20, 15, 17, 11)]) == -1 and ing(boxes=[(3, 2, 17, 4), (20, 15, 17, 11)]) == -1
    # 2 bh h, 2 bw w in 31 bits
    tall = dict(B=1, Hp=1 << 15, Wp=1, h=1 << 15, w=1, boxes=[(0, 0, 1, 1 << 15)])
    wide = dict(B=1, Hp=1, Wp=1 << 15, h=1, w=1 << 15, boxes=[(0, 0, 1 << 15, 1)])
    assert comp(**tall) == -1 and ing(**tall) == -1 and comp(**wide) == -1 and ing(**wide) == -1
    # Hp Wp, and the chunk count, in 31 bits
    huge = dict(B=1, Hp=1 << 16, Wp=1 << 16, boxes=[(0, 0, 7, 5)])
    assert comp(**huge) == -1 and ing(**huge) == -1
    many = dict(B=1 << 12, Hp=1 << 15, Wp=1 << 15, boxes=[(0, 0, 7, 5)] * (1 << 12))
    assert comp(**many) == -1 and ing(**many) == -1
    assert comp(B=0) == -1 and comp(h=0) == -1 and comp(w=0) == -1 and comp(Hp=0) == -1 and comp(Wp=-1) == -1
    assert ing(B=0) == -1 and ing(h=0) == -1 and ing(w=-1) == -1 and ing(Hp=0) == -1 and ing(Wp=0) == -1
    # paste, and boxes of different sizes without it
    assert comp(paste=2) == -1 and comp(paste=-1) == -1
    assert comp(paste=0, boxes=[(3, 2, 17, 11), (20, 15, 18, 11)]) == -1 and comp(paste=0, boxes=[(3, 2, 17, 11), (20, 15, 17, 12)]) == -1
    # what gcfr_fullres_composites_u8 refuses
    assert comp(L=0) == -1 and comp(L=4097) == -1 and comp(L=-1) == -1
    assert comp(mask_batch=0) == -1 and comp(mask_batch=3) == -1
    assert comp(clamp=0.99) == -1 and comp(clamp=float("nan")) == -1
    assert comp(floor=0.0) == -1 and comp(floor=-1.0) == -1 and comp(floor=float("nan")) == -1
    # an out that overlaps the photographs (2 x 30 x 40 x 3 = 7200 bytes from 1 << 20; out is 3 x 7200 bytes pasted and
    # 2 x 3 x 11 x 17 x 3 = 3366 not)
    for out in ((1 << 20), (1 << 20) + 7199, (1 << 20) - 1, (1 << 20) - 3 * 7200 + 1):
        assert comp(out=p(out)) == -1, out
    for out in ((1 << 20), (1 << 20) + 7199, (1 << 20) - 3366 + 1):
        assert comp(out=p(out), paste=0) == -1, out
    assert ing(x_lo=p(1 << 20)) == -1                                             # x_lo_out == photo


def test_the_python_entries_refuse_malformed_operands_without_a_gpu():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    B, L, h, w, Hp, Wp = 2, 3, 5, 7, 30, 40
    photo = torch.zeros((B, Hp, Wp, 3), dtype=torch.uint8)
    x_lo = torch.zeros((B, h, w, 3))
    rendered = torch.zeros((B, L, 3, h, w))
    mask = torch.zeros((h, w), dtype=torch.uint8)
    boxes = [(3, 2, 17, 11), (20, 15, 17, 11)]
    bad_boxes = [[(3, 2, 17, 11)], [(3, 2, 17, 11)] * 3, (3, 2, 17), [(3.0, 2.0, 17.0, 11.0)] * 2, np.zeros((B, 4), np.float32),
                 torch.tensor(boxes, dtype=torch.float32), np.array(boxes, dtype=bool), "box", None,
                 (-1, 2, 17, 11), (3, -1, 17, 11), (24, 2, 17, 11), (3, 20, 17, 11), (3, 2, 6, 11), (3, 2, 17, 4), (0, 0, 41, 11)]
    bad = [dict(boxes=b) for b in bad_boxes] + [
        dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(photo_u8=photo.numpy()), dict(photo_u8=photo[..., :2]),
        dict(x_lo=x_lo[:1]), dict(x_lo=x_lo.double()), dict(x_lo=x_lo.permute(0, 3, 1, 2)), dict(x_lo=x_lo[0]),
        dict(rendered=rendered[:, :, :2]), dict(rendered=rendered[:1]), dict(rendered=rendered[0, 0]), dict(rendered=rendered.to(torch.int32)),
        dict(rendered=torch.zeros((B, 0, 3, h, w))), dict(rendered=torch.zeros((B, Hp, Wp, 3))),
        dict(mask_u8=mask.float()), dict(mask_u8=torch.zeros((11, 17), dtype=torch.uint8)), dict(mask_u8=torch.zeros((3, h, w), dtype=torch.uint8)),
        dict(detail_clamp=0.5), dict(detail_clamp=float("nan")), dict(floor=0.0), dict(floor=-2.0),
        dict(paste=2), dict(paste="yes"), dict(paste=None),
        dict(paste=False, boxes=[(3, 2, 17, 11), (20, 15, 18, 11)]),
        dict(out=torch.zeros((B, L, Hp, Wp, 3))), dict(out=torch.zeros((B, Hp, Wp, 3), dtype=torch.uint8)),
        dict(out=torch.zeros((B, L, 11, 17, 3), dtype=torch.uint8)), dict(paste=False, out=torch.zeros((B, L, Hp, Wp, 3), dtype=torch.uint8)),
    ]
    for kw in bad:
        a = dict(photo_u8=photo, boxes=boxes, x_lo=x_lo, rendered=rendered, mask_u8=mask)
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.fullres_box_composites_device(**a)
    # well-formed host tensors, boxes as a list, an array, a CPU tensor or one box for every face: there is no CPU path
    for b in (boxes, np.array(boxes), np.array(boxes, dtype=np.uint16), torch.tensor(boxes), (3, 2, 17, 11)):
        for paste in (True, False):
            with pytest.raises(GcfrError, match="no CPU path"):
                pp.fullres_box_composites_device(photo, b, x_lo, rendered, mask, paste=paste)
        with pytest.raises(GcfrError, match="no CPU path"):
            pp.ingest_box_device(photo, b, (h, w))
    with pytest.raises(GcfrError, match="no CPU path"):
        pp.ingest_box_device(photo, (0, 0, 11, 11), 11)                            # an int: a square network
    for kw in [dict(boxes=b) for b in bad_boxes] + [dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(size=0), dict(size=(5,)),
                                                    dict(size=(5.0, 7.0)), dict(size=(5, 7, 3)), dict(size=None), dict(size=(18, 7))]:
        a = dict(photo_u8=photo, boxes=boxes, size=(h, w))
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.ingest_box_device(**a)


def test_the_inference_entries_exist_and_refuse_malformed_operands():
    import inspect
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd._lib import GcfrError
    names = ("relight_lights_in_photograph", "relight_lights_in_photograph_device", "relight_rig_in_photograph", "relight_rig_in_photograph_device")
    for name in names:
        sig = inspect.signature(getattr(inf, name))
        assert "upsample" not in sig.parameters and sig.parameters["paste"].default is True
    mask = np.zeros((5, 7), np.uint8)
    with pytest.raises(GcfrError, match="uint8"):
        inf.relight_lights_in_photograph_device(None, np.zeros((1, 30, 40, 3), np.float32), (3, 2, 17, 11), mask, None, device="cpu")
    photos = np.zeros((1, 30, 40, 3), np.uint8)
    for b in ((3, 2, 6, 11), (30, 2, 17, 11), (3.0, 2.0, 17.0, 11.0), [(3, 2, 17, 11)] * 2):
        with pytest.raises(GcfrError):
            inf.relight_lights_in_photograph_device(None, photos, b, mask, None, device="cpu")
        with pytest.raises(GcfrError):
            inf.relight_rig_in_photograph_device(None, photos, b, mask, None, None, device="cpu")
    with pytest.raises(GcfrError, match="mask_u8"):
        inf.relight_lights_in_photograph_device(None, photos, (3, 2, 17, 11), np.zeros((2, 5, 7), np.uint8), None, device="cpu")
    with pytest.raises(GcfrError, match="no CPU path"):
        inf.relight_lights_in_photograph_device(None, photos, (3, 2, 17, 11), mask, None, device="cpu")
