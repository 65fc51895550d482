"""CPU: the guided box composite's numpy restatement (tests/fullres_box_guided_emulation.py) held to independent statements, and the
host side of the entries (csrc/gcfr_fullres_box_guided.hip, postprocess.fullres_box_composites_device(upsample="guided"), the
inference.relight_*_in_photograph_guided entries): every refusal is made before any launch, so it is exercised without a GPU.

  anchor      with the box the whole photograph and s in {1, 2, 4, 8} the bytes are tests/fullres_guided_emulation.py's: the box
              statement is a strict generalisation of the power-of-two one
  integers    per axis the four integer weights are >= 0 and sum to 8 b
  den         range_sigma = inf: |den - 4| <= 72 x 2^-24 (derived at the test)
  f64         an f64 evaluation of the same formulas from half-pixel positions in floating point agrees with v within 5e-4 grey
              levels, and the 16 wn sum to 1 within 4e-7: tests/test_fullres_guided_host.py's bounds and its reasoning; the one
              operation this statement adds per weight (the rounding of k / (4 b), then of sy sx) is of the same 2^-24 relative size
              as the ~40 that reasoning already counts
  identity    rendered == x_lo returns the photograph wherever the quotient is not clamped
  step edge   across an edge inside a low-resolution pixel, on boxes of non-integer ratio, the guided composite follows the
              piecewise gain and does not leak through a one-sided mask; the bilinear box restatement on the same input does both
  NaNs        stay where the statement says, over the four-tap footprint"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import fullres_box_emulation as bil
import fullres_box_guided_emulation as emu
import fullres_guided_emulation as guided
from test_fullres_guided_host import SHAPES

F = np.float32
LEVELS = np.array([0, 64, 128, 255], np.uint8)
# (h, w, bh, bw): from one low-resolution pixel under a 3 x 5 box to (12,16) under 100 x 90; ratio 1, non-integer ratios on both
# sides of 2 and of 4, just under and over 8, anisotropic ones
BOXED = [(1, 1, 3, 5), (2, 3, 2, 3), (3, 5, 7, 19), (5, 7, 13, 9), (5, 7, 39, 50), (5, 7, 40, 55), (5, 7, 11, 56), (4, 8, 15, 33),
         (6, 8, 23, 30), (12, 16, 100, 90)]


def _inputs(seed, B, L, h, w, bh, bw, MB, margin=(0, 0, 0, 0)):
    """photographs whose box is all of them but `margin` (left, top, right, bottom)"""
    rng = np.random.default_rng(seed)
    ml, mt, mr, mb = margin
    photo = rng.integers(0, 256, (B, mt + bh + mb, ml + bw + mr, 3), dtype=np.uint8)
    boxes = np.array([(ml, mt, bw, bh)] * B)
    x_lo = (emu.ingest(photo, boxes, h, w) * (0.5 + rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (1.2 * rng.random((B, L, 3, h, w))).astype(np.float32)
    mask = LEVELS[rng.integers(0, 4, (MB, h, w))]
    return photo, boxes, x_lo, rendered, mask


@pytest.mark.parametrize("s,h,w", SHAPES)
def test_a_whole_photograph_power_of_two_box_is_the_guided_statement_byte_for_byte(s, h, w):
    rng = np.random.default_rng(7 * s + h)
    B, L = 2, 2
    photo = rng.integers(0, 256, (B, s * h, s * w, 3), dtype=np.uint8)
    x_lo = (guided.ingest(photo, s) * (0.5 + rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (1.2 * rng.random((B, L, 3, h, w))).astype(np.float32)
    whole = (0, 0, s * w, s * h)
    for n in (h, w):                                                               # the taps and the weights, bit for bit
        ia, wa = emu.spatial(s * n, n)
        ib, wb = guided.spatial(s * n, s, n)
        np.testing.assert_array_equal(ia, ib)
        np.testing.assert_array_equal(wa.view(np.uint32), wb.view(np.uint32))
    for sigma, MB in ((20.0, 1), (3.0, B), (np.inf, 1)):
        mask = LEVELS[rng.integers(0, 4, (MB, h, w))]
        want = guided.composites(photo, x_lo, rendered, mask, s, range_sigma=sigma)
        for paste in (True, False):
            np.testing.assert_array_equal(emu.composites(photo, whole, x_lo, rendered, mask, paste=paste, range_sigma=sigma), want)
        assert h * w == 1 or (want != photo[:, None]).any()                        # (one low-resolution pixel may draw a zero mask)


@pytest.mark.parametrize("h,w,bh,bw", BOXED)
def test_the_integer_weights_are_non_negative_and_sum_to_eight_b(h, w, bh, bw):
    for n_box, n_lo in ((bh, h), (bw, w)):
        idx, wint = emu.taps(n_box, n_lo)
        assert idx.shape == wint.shape == (n_box, 4)
        assert (wint >= 0).all() and (wint.sum(axis=1) == 8 * n_box).all()
        assert idx.min() >= 0 and idx.max() <= n_lo - 1 and (np.diff(idx, axis=1) >= 0).all()
        _, wf = emu.spatial(n_box, n_lo)
        assert wf.dtype == np.float32 and (np.abs(wf.astype(np.float64) * (4 * n_box) - wint) <= 2.0 ** -24 * wint).all()


@pytest.mark.parametrize("h,w,bh,bw", BOXED)
def test_the_tent_alone_sums_to_four_within_72_roundings(h, w, bh, bw):
    """range_sigma = inf: inv = 0, d2 inv = 0 and k = 1 exactly, so wt = fl(sy sx).  With u = 2^-24: every sy[j], sx[i] is its exact
    quotient k / (4 b) <= 1 rounded once, and the exact quotients of an axis sum to 2, so the rounded ones sum to 2 (1 + a) with
    |a| <= u.  The exact products of the rounded weights then sum to 4 (1 + a)(1 + a') -- within 8 u of 4 -- and rounding each
    product moves the sum by at most 4 u more: 12 u before the first addition.  Each of the 15 additions rounds a partial sum of
    at most 4 (+ 12 u): half an ulp below 4 is 2 u, at 4 it is 4 u; 15 x 4 u = 60 u.  |den - 4| <= 72 u = 4.3e-6, plus second-order
    terms below 2^-40."""
    rng = np.random.default_rng(bh + bw)
    crop = rng.integers(0, 256, (bh, bw, 3), dtype=np.uint8)
    x_lo = rng.random((h, w, 3), dtype=np.float32)
    _, den = emu.weights(crop, x_lo, np.inf)
    err = float(np.abs(den.astype(np.float64) - 4.0).max())
    print("(%d,%d) under %d x %d: max |den - 4| %.3g = %.1f x 2^-24" % (h, w, bh, bw, err, err * 2.0 ** 24))
    assert err <= 72.0 * 2.0 ** -24 + 2.0 ** -40
    if bh % h == 0 and bw % w == 0 and (bh // h) in (1, 2, 4, 8) and (bw // w) in (1, 2, 4, 8):
        assert err == 0.0                                                          # every weight is exact there


def _taps_f64(n_box, n_lo):
    """the same taps from half-pixel positions in floating point: indices (n_box,4) and f64 weights that sum to 2"""
    f = np.maximum((np.arange(n_box) + 0.5) * n_lo / n_box - 0.5, 0.0)
    y0 = np.floor(f)
    t = f - y0
    idx = np.clip(y0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_lo - 1)
    return idx, np.stack([(1 - t) / 2, (2 - t) / 2, (1 + t) / 2, t / 2], axis=1)


def _values_f64(crop, x_lo, rendered, mask, detail_clamp, floor, range_sigma):
    """one face in f64: v (L,bh,bw,3) and wn (bh,bw,4,4)"""
    bh, bw, _ = crop.shape
    h, w, _ = x_lo.shape
    iy, wy = _taps_f64(bh, h)
    ix, wx = _taps_f64(bw, w)
    g16 = lambda a: a.astype(np.float64)[..., iy[:, None, :, None], ix[None, :, None, :]]       # (..., bh, bw, 4, 4)
    p = crop.astype(np.float64)
    xt = np.stack([g16(x_lo[..., c]) for c in range(3)], axis=-1)                   # (bh,bw,4,4,3)
    d2 = ((p[:, :, None, None, :] - 255.0 * xt) ** 2).sum(axis=-1)
    wt = wy[:, None, :, None] * wx[None, :, None, :] / (1.0 + d2 / (float(range_sigma) ** 2))
    wn = wt / wt.sum(axis=(-1, -2), keepdims=True)
    xl = 255.0 * (wn[..., None] * xt).sum(axis=(2, 3))
    d = np.clip(p / np.maximum(xl, floor), 1.0 / detail_clamp, detail_clamp)
    m = (wn * g16(mask / 255.0)).sum(axis=(-1, -2))
    r = np.transpose(255.0 * (wn[None, None] * g16(rendered)).sum(axis=(-1, -2)), (0, 2, 3, 1))      # (L,bh,bw,3)
    return p[None] + m[None, :, :, None] * (r * d[None] - p[None]), wn


@pytest.mark.parametrize("h,w,bh,bw", BOXED)
def test_the_statement_agrees_with_its_f64_evaluation_and_its_weights_sum_to_one(h, w, bh, bw):
    B, L = 2, 2
    worst, worst_sum, top = 0.0, 0.0, 0.0
    for sigma, MB in ((20.0, 1), (8.0, B)):
        photo, boxes, x_lo, rendered, mask = _inputs(10 * bh + bw + int(sigma), B, L, h, w, bh, bw, MB)
        for b in range(B):
            mk = mask[b if MB > 1 else 0]
            v, _, _ = emu.box_values(photo[b], x_lo[b], rendered[b], mk, range_sigma=sigma)
            want, _ = _values_f64(photo[b], x_lo[b], rendered[b], mk, 4.0, 1.0, sigma)
            wn, _ = emu.weights(photo[b], x_lo[b], sigma)
            worst = max(worst, float(np.abs(v.astype(np.float64) - want).max()))
            worst_sum = max(worst_sum, float(np.abs(wn.astype(np.float64).sum(axis=(-1, -2)) - 1.0).max()))
            top = max(top, float(np.abs(want).max()))
    print("(%d,%d) under %d x %d: max |v - v_f64| %.3g at |v| up to %.0f; max |sum wn - 1| %.3g" % (h, w, bh, bw, worst, top, worst_sum))
    assert worst <= 5e-4
    assert worst_sum <= 4e-7


@pytest.mark.parametrize("h,w,bh,bw", BOXED)
def test_identity_rendered_equal_to_x_lo_returns_the_photograph(h, w, bh, bw):
    rng = np.random.default_rng(bh + 3 * bw)
    for B, MB in ((1, 1), (2, 2)):
        photo = rng.integers(64, 225, (B, bh + 3, bw + 5, 3), dtype=np.uint8)
        boxes = np.array([(2, 1, bw, bh), (5, 3, bw, bh)][:B])
        x_lo = emu.ingest(photo, boxes, h, w)
        rendered = np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2)))[:, None]
        mask = LEVELS[rng.integers(0, 4, (MB, h, w))]
        for b, (x0, y0, _, _) in enumerate(boxes):
            _, raw, _, xl, _ = emu.box_parts(photo[b, y0:y0 + bh, x0:x0 + bw], x_lo[b], mask[b if MB > 1 else 0])
            assert ((raw > 0.25) & (raw < 4.0) & (xl >= 1.0)).all()                  # no pixel is clamped
        got = emu.composites(photo, boxes, x_lo, rendered, mask)
        assert got.shape == (B, 1, bh + 3, bw + 5, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got[:, 0], photo)
        alone = emu.composites(photo, boxes, x_lo, rendered, mask, paste=False)
        for b, (x0, y0, _, _) in enumerate(boxes):
            np.testing.assert_array_equal(alone[b, 0], photo[b, y0:y0 + bh, x0:x0 + bw])


# ------------------------------------------------------------------------------------------------
# the step edge, on boxes of non-integer ratio over (h, w) = (12, 16)
# ------------------------------------------------------------------------------------------------
EDGE_BOXES = [(41, 56), (41, 33), (100, 90)]
EDGE_AT = [8.5, 8.75]                                                              # in low-resolution columns


def step_edge(bh, bw, at, seed=0):
    """tests/test_fullres_guided_host.py's scene on a bh x bw photograph that is its own box: (180,140,120) left of column
    e = round(at bw / 16) and (30,25,20) from e on, plus integer noise in [-6, 6]; x_lo its box ingest; rendered = x_lo times 0.5
    on the low-res columns whose centre lies left of e and times 1 elsewhere.  -> photo, box, x_lo, rendered, e, the low-res
    columns with gain 0.5, the ideal output (float)"""
    h, w = 12, 16
    e = int(round(at * bw / w))
    rng = np.random.default_rng(seed)
    base = np.where((np.arange(bw) < e)[None, :, None], np.array([180, 140, 120]), np.array([30, 25, 20]))
    photo = (base + rng.integers(-6, 7, (bh, bw, 3))).astype(np.uint8)[None]
    box = (0, 0, bw, bh)
    x_lo = emu.ingest(photo, box, h, w)
    half = (np.arange(w) + 0.5) * bw < e * w
    gain = np.where(half, F(0.5), F(1.0)).astype(np.float32)
    rendered = np.ascontiguousarray(np.transpose(x_lo * gain[None, None, :, None], (0, 3, 1, 2)))[:, None]
    ideal = photo[0].astype(np.float64) * np.where(np.arange(bw) < e, 0.5, 1.0)[None, :, None]
    return photo, box, x_lo, rendered, e, half, ideal


@pytest.mark.parametrize("bh,bw", EDGE_BOXES)
def test_step_edge_the_guided_composite_follows_the_piecewise_gain(bh, bw):
    """condition (i), under a full mask, in the band of two low-resolution pixels either side of the edge"""
    h, w = 12, 16
    full = np.full((1, h, w), 255, np.uint8)
    ry, rx = -(-2 * bh // h), -(-2 * bw // w)
    for at in EDGE_AT:
        photo, box, x_lo, rendered, e, _, ideal = step_edge(bh, bw, at)
        rows, cols = slice(ry, bh - ry), slice(e - rx, e + rx)
        band = lambda out: float(np.abs(out[0, 0].astype(np.float64) - ideal)[rows, cols].mean())
        g = band(emu.composites(photo, box, x_lo, rendered, full))
        b = band(bil.composites(photo, box, x_lo, rendered, full))
        print("%d x %d edge at %.2f (column %d): mean |out - ideal| in the band: guided %.3f, bilinear %.3f (ratio %.1f)" % (bh, bw, at, e, g, b, b / g))
        assert g <= 1.0
        assert 3.0 * g <= b


@pytest.mark.parametrize("bh,bw", EDGE_BOXES)
def test_step_edge_nothing_leaks_through_a_one_sided_mask(bh, bw):
    """condition (ii), under a mask that is 255 on the gain-0.5 columns and 0 elsewhere"""
    worst_bilinear = 0
    for at in EDGE_AT:
        photo, box, x_lo, rendered, e, half, _ = step_edge(bh, bw, at)
        mask = np.broadcast_to(np.where(half, 255, 0).astype(np.uint8)[None, None, :], (1, 12, 16)).copy()
        moved = lambda out: int(np.abs(out[0, 0].astype(np.int64) - photo[0].astype(np.int64))[:, e:].max())
        g = moved(emu.composites(photo, box, x_lo, rendered, mask))
        b = moved(bil.composites(photo, box, x_lo, rendered, mask))
        print("%d x %d edge at %.2f: largest move right of the edge: guided %d, bilinear %d" % (bh, bw, at, g, b))
        assert g <= 1
        worst_bilinear = max(worst_bilinear, b)
    assert worst_bilinear >= 3


def test_nans_stay_where_the_statement_says():
    h, w, bh, bw = 6, 8, 23, 30
    photo, boxes, x_lo, rendered, mask = _inputs(5, 1, 2, h, w, bh, bw, 1, margin=(3, 2, 4, 1))
    mask[:] = 255
    clean = emu.composites(photo, boxes, x_lo, rendered, mask)
    rows, cols = emu.tap_footprint(bh, h, 2) + 2, emu.tap_footprint(bw, w, 3) + 3
    assert rows.size >= 4 * (bh // h) and cols.size >= 4 * (bw // w)               # four taps wide, not the bilinear two
    # in `rendered` alone: byte 0 in that light and channel over the tap footprint, nothing else moves
    ren = rendered.copy()
    ren[0, 1, 2, 2, 3] = np.nan
    got = emu.composites(photo, boxes, x_lo, ren, mask)
    want = clean.copy()
    want[0, 1, rows[:, None], cols[None, :], 2] = 0
    np.testing.assert_array_equal(got, want)
    # in x_lo: the weights, hence m, are NaN there, and the photograph's bytes are kept in every light
    x = x_lo.copy()
    x[0, 2, 3, 1] = np.nan
    got = emu.composites(photo, boxes, x, rendered, mask)
    want = clean.copy()
    R, C = np.ix_(rows, cols)
    want[0][:, R, C, :] = photo[0][R, C][None]
    np.testing.assert_array_equal(got, want)
    assert (clean[0][:, R, C, :] != photo[0][R, C][None]).any()
    # outside the box nothing moves, whatever `rendered` holds
    got = emu.composites(photo, boxes, x_lo, np.full_like(rendered, np.nan), mask)
    outside = np.ones(photo.shape[1:3], bool)
    outside[2:2 + bh, 3:3 + bw] = False
    np.testing.assert_array_equal(got[0][:, outside], np.broadcast_to(photo[0][outside], got[0][:, outside].shape))
    assert (got[0][:, ~outside] == 0).all()


# ------------------------------------------------------------------------------------------------
# the entries' host side
# ------------------------------------------------------------------------------------------------
def _host_boxes(rows):
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 4))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_the_c_entry_refuses_before_any_launch():
    """junk device pointers throughout: every call below must return before it launches"""
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = lambda v: ctypes.c_void_p(v)
    ok = dict(photo=p(1 << 20), x_lo=p(128), rendered=p(256), mask=p(512), mask_batch=1, B=2, L=3, Hp=30, Wp=40, h=5, w=7, paste=1,
              floor=1.0, clamp=4.0, sigma=20.0, out=p(1 << 30), boxes=[(3, 2, 17, 11), (20, 15, 17, 11)])

    def comp(**kw):
        a = dict(ok, **kw)
        keep, bp = (None, None) if a["boxes"] is None else _host_boxes(a["boxes"])
        return L.gcfr_fullres_composites_box_guided_u8(a["photo"], a["x_lo"], a["rendered"], a["mask"], a["mask_batch"], a["B"], a["L"],
                                                       a["Hp"], a["Wp"], bp, a["h"], a["w"], a["paste"], a["floor"], a["clamp"],
                                                       a["sigma"], a["out"], None)

    for sigma in (0.0, -1.0, -float("inf"), float("nan")):
        for paste in (0, 1):
            assert comp(sigma=sigma, paste=paste) == -1, sigma
    # gcfr_fullres_composites_box_u8's refusals, through this symbol
    for name in ("photo", "x_lo", "rendered", "mask", "out", "boxes"):
        assert comp(**{name: None}) == -1, name
    second = lambda *b: [(3, 2, 17, 11), b]
    bad_boxes = [second(-1, 15, 17, 11), second(20, -1, 17, 11), second(24, 15, 17, 11), second(20, 20, 17, 11),     # outside
                 second(20, 15, 6, 11), second(20, 15, 17, 4), second(20, 15, 0, 0), second(20, 15, -17, 11),       # smaller than (h, w)
                 second(0, 0, 41, 11), second(0, 0, 17, 31), second(2 ** 31 - 8, 0, 17, 11)]
    for b in bad_boxes:
        for paste in (0, 1):
            assert comp(boxes=b, paste=paste) == -1, b
    assert comp(boxes=[(30, 2, 17, 11), (20, 15, 17, 11)]) == -1                    # the FIRST face's box is checked like every other
    # 2 bh h, 2 bw w in 31 bits
    assert comp(B=1, Hp=1 << 15, Wp=1, h=1 << 15, w=1, boxes=[(0, 0, 1, 1 << 15)]) == -1
    assert comp(B=1, Hp=1, Wp=1 << 15, h=1, w=1 << 15, boxes=[(0, 0, 1 << 15, 1)]) == -1
    # Hp Wp, and the chunk count, in 31 bits
    assert comp(B=1, Hp=1 << 16, Wp=1 << 16, boxes=[(0, 0, 7, 5)]) == -1
    assert comp(B=1 << 12, Hp=1 << 15, Wp=1 << 15, boxes=[(0, 0, 7, 5)] * (1 << 12)) == -1
    assert comp(B=0) == -1 and comp(h=0) == -1 and comp(w=0) == -1 and comp(Hp=0) == -1 and comp(Wp=-1) == -1
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


def _reached(*a, **k):
    raise AssertionError("a refused call reached the library")


def test_the_python_entry_refuses_before_anything_is_loaded_or_launched(monkeypatch):
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import postprocess as pp
    monkeypatch.setattr(_lib, "launch", _reached)
    monkeypatch.setattr(_lib, "load", _reached)
    B, L, h, w, Hp, Wp = 2, 3, 5, 7, 30, 40
    photo = torch.zeros((B, Hp, Wp, 3), dtype=torch.uint8)
    x_lo = torch.zeros((B, h, w, 3))
    rendered = torch.zeros((B, L, 3, h, w))
    mask = torch.zeros((h, w), dtype=torch.uint8)
    boxes = [(3, 2, 17, 11), (20, 15, 17, 11)]
    g = dict(upsample="guided")
    bad = [
        dict(upsample="bicubic"), dict(upsample="Guided"), dict(upsample=""), dict(upsample=None), dict(upsample=1),
        dict(g, range_sigma=0.0), dict(g, range_sigma=-3.0), dict(g, range_sigma=float("nan")), dict(g, range_sigma="20"),
        dict(g, range_sigma=None), dict(g, range_sigma=True),
        dict(range_sigma=0.0), dict(range_sigma="20"), dict(upsample="bilinear", range_sigma=True),      # with the default upsample as well
        # the operands' checks are the bilinear box entry's
        dict(g, boxes=[(3, 2, 17, 11)]), dict(g, boxes=(3, 2, 17)), dict(g, boxes=np.zeros((B, 4), np.float32)), dict(g, boxes=None),
        dict(g, boxes=(-1, 2, 17, 11)), dict(g, boxes=(24, 2, 17, 11)), dict(g, boxes=(3, 2, 6, 11)), dict(g, boxes=(0, 0, 41, 11)),
        dict(g, photo_u8=photo.float()), dict(g, photo_u8=photo[0]), dict(g, x_lo=x_lo[:1]), dict(g, x_lo=x_lo.double()),
        dict(g, rendered=rendered[:, :, :2]), dict(g, rendered=rendered.to(torch.int32)), dict(g, mask_u8=mask.float()),
        dict(g, mask_u8=torch.zeros((11, 17), dtype=torch.uint8)), dict(g, detail_clamp=0.5), dict(g, floor=0.0),
        dict(g, paste=2), dict(g, paste=None), dict(g, paste=False, boxes=[(3, 2, 17, 11), (20, 15, 18, 11)]),
        dict(g, out=torch.zeros((B, L, Hp, Wp, 3))), dict(g, out=torch.zeros((B, L, 11, 17, 3), dtype=torch.uint8)),
    ]
    for kw in bad:
        a = dict(photo_u8=photo, boxes=boxes, x_lo=x_lo, rendered=rendered, mask_u8=mask)
        a.update(kw)
        with pytest.raises(_lib.GcfrError) as e:
            pp.fullres_box_composites_device(**a)
        assert "no CPU path" not in str(e.value), (kw, str(e.value))
    # the two keywords' messages are fullres_composites_device's
    for kw in (dict(upsample="bicubic"), dict(g, range_sigma=-3.0)):
        with pytest.raises(_lib.GcfrError) as e1:
            pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, **kw)
        with pytest.raises(_lib.GcfrError) as e2:
            pp.fullres_composites_device(photo[:, :10, :14], x_lo, rendered, mask, 2, **kw)
        assert str(e1.value).split(": ", 1)[1] == str(e2.value).split(": ", 1)[1]
    # well-formed host tensors: there is no CPU path, with either upsample and with an infinite range_sigma
    for kw in (g, dict(g, range_sigma=float("inf")), dict(g, range_sigma=8), dict(g, paste=False), dict(upsample="bilinear", range_sigma=5.0)):
        with pytest.raises(_lib.GcfrError, match="no CPU path"):
            pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, **kw)


def test_the_inference_entries_exist_and_refuse_malformed_operands():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    par = inspect.signature(pp.fullres_box_composites_device).parameters
    assert par["upsample"].default == "bilinear" and par["range_sigma"].default == 20.0
    names = ("relight_lights_in_photograph_guided", "relight_lights_in_photograph_guided_device", "relight_rig_in_photograph_guided",
             "relight_rig_in_photograph_guided_device")
    for name in names:
        par = inspect.signature(getattr(inf, name)).parameters
        assert par["paste"].default is True and par["range_sigma"].default == 20.0 and "upsample" not in par, name
        plain = inspect.signature(getattr(inf, name.replace("_guided", ""))).parameters
        assert list(par) == list(plain) + ["range_sigma"], name
    mask = np.zeros((5, 7), np.uint8)
    lights_fn, rig_fn = inf.relight_lights_in_photograph_guided_device, inf.relight_rig_in_photograph_guided_device
    with pytest.raises(GcfrError, match="uint8"):
        lights_fn(None, np.zeros((1, 30, 40, 3), np.float32), (3, 2, 17, 11), mask, None, device="cpu")
    with pytest.raises(GcfrError, match="uint8"):
        rig_fn(None, np.zeros((1, 30, 40, 3), np.float32), (3, 2, 17, 11), mask, None, None, device="cpu")
    photos = np.zeros((1, 30, 40, 3), np.uint8)
    for b in ((3, 2, 6, 11), (30, 2, 17, 11), (3.0, 2.0, 17.0, 11.0), [(3, 2, 17, 11)] * 2):
        with pytest.raises(GcfrError) as e:
            lights_fn(None, photos, b, mask, None, device="cpu")
        assert "no CPU path" not in str(e.value)
        with pytest.raises(GcfrError) as e:
            rig_fn(None, photos, b, mask, None, None, device="cpu")
        assert "no CPU path" not in str(e.value)
    with pytest.raises(GcfrError, match="mask_u8"):
        lights_fn(None, photos, (3, 2, 17, 11), np.zeros((2, 5, 7), np.uint8), None, device="cpu")
    with pytest.raises(GcfrError, match="no CPU path"):
        lights_fn(None, photos, (3, 2, 17, 11), mask, None, device="cpu")
    with pytest.raises(GcfrError, match="no CPU path"):
        inf.relight_lights_in_photograph_guided(None, photos, (3, 2, 17, 11), mask, None, device="cpu", range_sigma=8.0, paste=False)
