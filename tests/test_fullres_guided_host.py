"""CPU: the guided full-resolution composite's numpy restatement (tests/fullres_guided_emulation.py) held to independent statements,
and the host side of the entry (csrc/gcfr_fullres_guided.hip, postprocess.fullres_composites_device(upsample="guided")): every
refusal is made before any launch, so it is exercised without a GPU.

  tent        range_sigma = inf: den == 4 exactly, and a ramp is reproduced exactly away from the borders
  f64         an f64 evaluation of the same formulas (half-pixel positions in floating point, the weights normalised by one sum)
              agrees with v within 5e-4 grey levels.  The f32 statement rounds each of its ~40 operations per value to 2^-24
              relative; at |v| up to ~550 and values of r d up to ~1400 a product or sum carries up to 1400 x 2^-24 = 8e-5, and
              the few that act at full scale (r 255, r d, r d - p, p + m (.)) add up to a few 1e-4 at worst
  weight sum  the 16 wn sum to 1 within 4e-7: each wn is rounded twice (wt rcp, and rcp itself stands for 1 / den with den the
              rounded sum of 15 additions): (15 / 2 + 1 + 1 / 2) x 2^-24 = 5.4e-7 at worst, typically less
  identity    rendered == x_lo returns the photograph wherever the quotient is not clamped and xl >= floor
  step edge   what the feature exists for: across an edge inside a low-resolution pixel the guided composite follows the piecewise
              gain and does not leak through a one-sided mask; the bilinear restatement on the same input does both"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import fullres_emulation as bil
import fullres_guided_emulation as emu

F = np.float32
SHAPES = [(1, 7, 9), (2, 5, 3), (4, 3, 5), (8, 2, 3), (4, 20, 28), (4, 1, 1)]
LEVELS = np.array([0, 64, 128, 255], np.uint8)


def _inputs(seed, B, L, s, h, w, MB):
    rng = np.random.default_rng(seed)
    photo = rng.integers(0, 256, (B, s * h, s * w, 3), dtype=np.uint8)
    x_lo = (emu.ingest(photo, s) * (0.5 + rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (1.2 * rng.random((B, L, 3, h, w))).astype(np.float32)
    mask = LEVELS[rng.integers(0, 4, (MB, h, w))]
    return photo, x_lo, rendered, mask


def test_the_tent_alone_sums_to_four_and_reproduces_a_ramp():
    s, h, w = 4, 6, 8
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, (1, s * h, s * w, 3), dtype=np.uint8)
    x_lo = rng.random((1, h, w, 3), dtype=np.float32)
    wn, den = emu.weights(photo, x_lo, s, np.inf)
    assert (den == F(4.0)).all()
    for n_hi, n_lo in ((s * h, h), (s * w, w)):                                     # per axis the four weights sum to 2
        _, wint = emu.taps(n_hi, s, n_lo)
        assert (wint.sum(axis=1) == 8 * s).all() and (wint >= 0).all()
    ii, jj = np.mgrid[0:h, 0:w]
    ramp = (3 * jj + 5 * ii).astype(np.float32)[None]
    got = emu.up_j(ramp, wn, s)[0]
    Y, X = np.mgrid[0:s * h, 0:s * w]
    want = 3.0 * ((X + 0.5) / s - 0.5) + 5.0 * ((Y + 0.5) / s - 0.5)
    inner = (Y >= 2 * s) & (Y < s * h - 2 * s) & (X >= 2 * s) & (X < s * w - 2 * s)
    err = float(np.abs(got.astype(np.float64) - want)[inner].max())
    print("ramp: max error at %d inner pixels %.3g" % (int(inner.sum()), err))
    assert inner.sum() > 0 and err == 0.0
    # a constant field is returned within the rounding of the weights, with any range_sigma
    wn20, _ = emu.weights(photo, x_lo, s, 20.0)
    assert np.abs(emu.up_j(np.full((1, h, w), F(0.7)), wn20, s).astype(np.float64) - np.float64(F(0.7))).max() <= 4e-7


def _taps_f64(n_hi, s, n_lo):
    """the same taps from half-pixel positions in floating point: indices (n_hi,4) and f64 weights that sum to 2"""
    f = np.maximum((np.arange(n_hi) + 0.5) / s - 0.5, 0.0)
    y0 = np.floor(f)
    t = f - y0
    idx = np.clip(y0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_lo - 1)
    return idx, np.stack([(1 - t) / 2, (2 - t) / 2, (1 + t) / 2, t / 2], axis=1)


def _values_f64(photo, x_lo, rendered, mask, s, detail_clamp, floor, range_sigma):
    B, H, W, _ = photo.shape
    h, w = H // s, W // s
    iy, wy = _taps_f64(H, s, h)
    ix, wx = _taps_f64(W, s, w)
    g16 = lambda a: a.astype(np.float64)[..., iy[:, None, :, None], ix[None, :, None, :]]       # (..., H, W, 4, 4)
    p = photo.astype(np.float64)
    xt = np.stack([g16(x_lo[..., c]) for c in range(3)], axis=-1)                   # (B,H,W,4,4,3)
    d2 = ((p[:, :, :, None, None, :] - 255.0 * xt) ** 2).sum(axis=-1)
    wt = wy[:, None, :, None] * wx[None, :, None, :] / (1.0 + d2 / (float(range_sigma) ** 2))
    wn = wt / wt.sum(axis=(-1, -2), keepdims=True)
    xl = 255.0 * (wn[..., None] * xt).sum(axis=(3, 4))
    d = np.clip(p / np.maximum(xl, floor), 1.0 / detail_clamp, detail_clamp)
    m = (wn * g16(np.broadcast_to(mask / 255.0, (B, h, w)))).sum(axis=(-1, -2))
    r = 255.0 * (wn[:, None, None] * g16(rendered)).sum(axis=(-1, -2))             # (B,L,3,H,W)
    r = np.transpose(r, (0, 1, 3, 4, 2))
    return p[:, None] + m[:, None, :, :, None] * (r * d[:, None] - p[:, None]), wn


@pytest.mark.parametrize("s,h,w", SHAPES)
def test_the_statement_agrees_with_its_f64_evaluation_and_its_weights_sum_to_one(s, h, w):
    B, L = 2, 2
    worst, worst_sum, top = 0.0, 0.0, 0.0
    for sigma, MB in ((20.0, 1), (8.0, B)):
        photo, x_lo, rendered, mask = _inputs(10 * s + h + int(sigma), B, L, s, h, w, MB)
        v, _ = emu.values(photo, x_lo, rendered, mask, s, range_sigma=sigma)
        want, _ = _values_f64(photo, x_lo, rendered, mask, s, 4.0, 1.0, sigma)
        wn, _ = emu.weights(photo, x_lo, s, sigma)
        worst = max(worst, float(np.abs(v.astype(np.float64) - want).max()))
        worst_sum = max(worst_sum, float(np.abs(wn.astype(np.float64).sum(axis=(-1, -2)) - 1.0).max()))
        top = max(top, float(np.abs(want).max()))
    print("(%d,%d,%d): max |v - v_f64| %.3g at |v| up to %.0f; max |sum wn - 1| %.3g" % (s, h, w, worst, top, worst_sum))
    assert worst <= 5e-4
    assert worst_sum <= 4e-7


@pytest.mark.parametrize("s,h,w", SHAPES)
def test_identity_rendered_equal_to_x_lo_returns_the_photograph(s, h, w):
    rng = np.random.default_rng(10 * s + h)
    for B, MB in ((1, 1), (2, 2)):
        photo = rng.integers(64, 225, (B, s * h, s * w, 3), dtype=np.uint8)
        x_lo = emu.ingest(photo, s)
        rendered = np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2)))[:, None]
        mask = LEVELS[rng.integers(0, 4, (MB, h, w))]
        _, raw, _, xl, _ = emu.parts(photo, x_lo, mask, s)
        free = (raw > 0.25) & (raw < 4.0) & (xl >= 1.0)
        got = emu.composites(photo, x_lo, rendered, mask, s)
        assert got.shape == (B, 1, s * h, s * w, 3) and got.dtype == np.uint8
        assert free.mean() > 0.9
        np.testing.assert_array_equal(got[:, 0][free], photo[free])
        # the statement says more for these inputs: no pixel is clamped, so every byte is the photograph's
        assert free.all()
        np.testing.assert_array_equal(got[:, 0], photo)


# ------------------------------------------------------------------------------------------------
# the step edge
# ------------------------------------------------------------------------------------------------
def step_edge(s, off, seed=0):
    """(h, w) = (12, 16): a photograph that is (180,140,120) left of hi-res column e = 8 s + off and (30,25,20) from e on, plus
    integer noise in [-6, 6]; x_lo its ingest; rendered = x_lo times 0.5 on the low-res columns whose centre lies left of e and
    times 1 elsewhere.  -> photo, x_lo, rendered, e, the low-res columns with gain 0.5, the ideal output (float)"""
    h, w = 12, 16
    H, W = s * h, s * w
    e = 8 * s + off
    rng = np.random.default_rng(seed)
    base = np.where((np.arange(W) < e)[None, :, None], np.array([180, 140, 120]), np.array([30, 25, 20]))
    photo = (base + rng.integers(-6, 7, (H, W, 3))).astype(np.uint8)[None]
    x_lo = emu.ingest(photo, s)
    half = (np.arange(w) + 0.5) * s < e
    gain = np.where(half, F(0.5), F(1.0)).astype(np.float32)
    rendered = np.ascontiguousarray(np.transpose(x_lo * gain[None, None, :, None], (0, 3, 1, 2)))[:, None]
    ideal = photo[0].astype(np.float64) * np.where(np.arange(W) < e, 0.5, 1.0)[None, :, None]
    return photo, x_lo, rendered, e, half, ideal


def offsets(s):
    return sorted({1, 2 if s == 2 else s // 2, s - 1})


@pytest.mark.parametrize("s", [2, 4, 8])
def test_step_edge_the_guided_composite_follows_the_piecewise_gain(s):
    """condition (i), under a full mask"""
    h, w = 12, 16
    full = np.full((1, h, w), 255, np.uint8)
    for off in offsets(s):
        photo, x_lo, rendered, e, _, ideal = step_edge(s, off)
        rows, cols = slice(2 * s, s * h - 2 * s), slice(e - 2 * s, e + 2 * s)
        band = lambda out: float(np.abs(out[0, 0].astype(np.float64) - ideal)[rows, cols].mean())
        guided = band(emu.composites(photo, x_lo, rendered, full, s))
        bilinear = band(bil.composites(photo, x_lo, rendered, full, s))
        print("s %d off %d: mean |out - ideal| in the band: guided %.3f, bilinear %.3f (ratio %.1f)" % (s, off, guided, bilinear, bilinear / guided))
        assert guided <= 1.0
        assert 3.0 * guided <= bilinear


@pytest.mark.parametrize("s", [2, 4, 8])
def test_step_edge_nothing_leaks_through_a_one_sided_mask(s):
    """condition (ii), under a mask that is 255 on the gain-0.5 columns and 0 elsewhere"""
    worst_bilinear = 0
    for off in offsets(s):
        photo, x_lo, rendered, e, half, _ = step_edge(s, off)
        mask = np.broadcast_to(np.where(half, 255, 0).astype(np.uint8)[None, None, :], (1, 12, 16)).copy()
        moved = lambda out: int(np.abs(out[0, 0].astype(np.int64) - photo[0].astype(np.int64))[:, e:].max())
        guided = moved(emu.composites(photo, x_lo, rendered, mask, s))
        bilinear = moved(bil.composites(photo, x_lo, rendered, mask, s))
        print("s %d off %d: largest move right of the edge: guided %d, bilinear %d" % (s, off, guided, bilinear))
        assert guided <= 1
        worst_bilinear = max(worst_bilinear, bilinear)
    assert worst_bilinear >= 3


def test_nans_stay_where_the_statement_says():
    s, h, w = 4, 6, 8
    photo, x_lo, rendered, mask = _inputs(5, 1, 2, s, h, w, 1)
    mask[:] = 255
    clean = emu.composites(photo, x_lo, rendered, mask, s)
    iy, _ = emu.taps(s * h, s, h)
    ix, _ = emu.taps(s * w, s, w)
    rows, cols = np.nonzero((iy == 2).any(axis=1))[0], np.nonzero((ix == 3).any(axis=1))[0]
    # in `rendered` alone: byte 0 in that light and channel over the tap footprint, nothing else moves
    ren = rendered.copy()
    ren[0, 1, 2, 2, 3] = np.nan
    got = emu.composites(photo, x_lo, ren, mask, s)
    want = clean.copy()
    want[0, 1, rows[:, None], cols[None, :], 2] = 0
    np.testing.assert_array_equal(got, want)
    # in x_lo: the weights, hence m, are NaN there, and the photograph's bytes are kept in every light
    x = x_lo.copy()
    x[0, 2, 3, 1] = np.nan
    got = emu.composites(photo, x, rendered, mask, s)
    want = clean.copy()
    R, C = np.ix_(rows, cols)
    want[0][:, R, C, :] = photo[0][R, C][None]
    np.testing.assert_array_equal(got, want)
    assert (clean[0][:, R, C, :] != photo[0][R, C][None]).any()


# ------------------------------------------------------------------------------------------------
# the entries' host side
# ------------------------------------------------------------------------------------------------
def test_the_c_entry_refuses_before_any_launch():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = lambda v: ctypes.c_void_p(v)
    ok_c = dict(photo=p(64), x_lo=p(128), rendered=p(256), mask=p(512), mask_batch=1, B=2, L=3, h=5, w=3, s=2, floor=1.0, clamp=4.0,
                sigma=20.0, out=p(1024))

    def comp(**kw):
        a = dict(ok_c, **kw)
        return L.gcfr_fullres_composites_guided_u8(a["photo"], a["x_lo"], a["rendered"], a["mask"], a["mask_batch"], a["B"], a["L"],
                                                   a["h"], a["w"], a["s"], a["floor"], a["clamp"], a["sigma"], a["out"], None)

    for sigma in (0.0, -1.0, -float("inf"), float("nan")):
        assert comp(sigma=sigma) == -1, sigma
    # gcfr_fullres_composites_u8's refusals, through this symbol
    for name in ("photo", "x_lo", "rendered", "mask", "out"):
        assert comp(**{name: None}) == -1, name
    for s in (0, 3, 5, 6, 16, -2):
        assert comp(s=s) == -1, s
    assert comp(L=0) == -1 and comp(L=4097) == -1 and comp(L=-1) == -1
    assert comp(mask_batch=0) == -1 and comp(mask_batch=3) == -1
    assert comp(out=p(64)) == -1                                                  # out == photo
    assert comp(clamp=0.99) == -1 and comp(clamp=float("nan")) == -1
    assert comp(floor=0.0) == -1 and comp(floor=-1.0) == -1 and comp(floor=float("nan")) == -1
    assert comp(B=0) == -1 and comp(h=0) == -1 and comp(w=0) == -1
    assert comp(B=1, h=1 << 15, w=1 << 15, s=2) == -1                              # H W = 2^32
    assert comp(B=1, h=1 << 14, w=1 << 14, s=8) == -1                              # H W = 2^34
    assert comp(B=1 << 12, h=1 << 14, w=1 << 14, s=2) == -1                        # H W = 2^30, B chunks = 2^32


def _reached(*a, **k):
    raise AssertionError("a refused call reached the library")


def test_the_python_entry_refuses_before_anything_is_loaded_or_launched(monkeypatch):
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import postprocess as pp
    monkeypatch.setattr(_lib, "launch", _reached)
    monkeypatch.setattr(_lib, "load", _reached)
    B, L, h, w, s = 2, 3, 5, 3, 2
    photo = torch.zeros((B, s * h, s * w, 3), dtype=torch.uint8)
    x_lo = torch.zeros((B, h, w, 3))
    rendered = torch.zeros((B, L, 3, h, w))
    mask = torch.zeros((h, w), dtype=torch.uint8)
    bad = [
        dict(upsample="bicubic"), dict(upsample="Guided"), dict(upsample=""), dict(upsample=None), dict(upsample=1),
        dict(upsample="guided", range_sigma=0.0), dict(upsample="guided", range_sigma=-3.0),
        dict(upsample="guided", range_sigma=float("nan")), dict(upsample="guided", range_sigma="20"),
        dict(upsample="guided", range_sigma=None), dict(upsample="guided", range_sigma=True),
        dict(range_sigma=0.0),                                                   # refused with the default upsample as well
        # the operands' checks are the bilinear path's
        dict(upsample="guided", photo_u8=photo.float()), dict(upsample="guided", scale=3), dict(upsample="guided", x_lo=x_lo[:1]),
        dict(upsample="guided", rendered=rendered[:, :, :2]), dict(upsample="guided", mask_u8=mask.float()),
        dict(upsample="guided", detail_clamp=0.5), dict(upsample="guided", floor=0.0),
        dict(upsample="guided", out=torch.zeros((B, L, s * h, s * w, 3))),
    ]
    for kw in bad:
        a = dict(photo_u8=photo, x_lo=x_lo, rendered=rendered, mask_u8=mask, scale=s)
        a.update(kw)
        with pytest.raises(_lib.GcfrError) as e:
            pp.fullres_composites_device(**a)
        assert "no CPU path" not in str(e.value), (kw, str(e.value))
    # well-formed host tensors: there is no CPU path, with either upsample and with an infinite range_sigma
    for kw in (dict(upsample="guided"), dict(upsample="guided", range_sigma=float("inf")), dict(upsample="guided", range_sigma=8),
               dict(upsample="bilinear", range_sigma=5.0)):
        with pytest.raises(_lib.GcfrError, match="no CPU path"):
            pp.fullres_composites_device(photo, x_lo, rendered, mask, s, **kw)


def test_the_inference_entries_accept_the_two_keywords():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    for fn in (pp.fullres_composites_device, inf.relight_lights_fullres, inf.relight_lights_fullres_device, inf.relight_rig_fullres,
               inf.relight_rig_fullres_device):
        par = inspect.signature(fn).parameters
        assert par["upsample"].default == "bilinear" and par["range_sigma"].default == 20.0, fn.__name__
    with pytest.raises(GcfrError, match="uint8"):
        inf.relight_lights_fullres_device(None, np.zeros((1, 8, 8, 3), np.float32), None, None, 2, device="cpu", upsample="guided",
                                          range_sigma=8.0)
    with pytest.raises(GcfrError, match="uint8"):
        inf.relight_rig_fullres_device(None, np.zeros((1, 8, 8, 3), np.float32), None, None, None, 2, device="cpu", upsample="guided",
                                       range_sigma=8.0)
