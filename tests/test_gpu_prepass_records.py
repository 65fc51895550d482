"""GPU: what the prepass (csrc/gcfr_shadow.hip build_quad_kernel) leaves in the workspace for the march -- the depth-bounds
records and the 2 x 2 texels -- read back after a prepass-only call (gcfr_options.phase = 1) and compared with their
definition, restated in f64 numpy.

A record {a, b, c_lo, c_hi} of tile (ti, tj) at stride s bounds the 2s x 2s EXTENDED cells (er, ec) in [ti s, ti s + 2s) x
[tj s, tj s + 2s) with er <= H, ec <= W; extended cell (er, ec) is depth cell (er - 1, ec - 1), index -1 wrapping to the last
row / column; X = (ec - 1) - W/2, Y = H/2 - (er - 1).

Tolerances (none is taken from what the kernel gives):
  residuals  tol = 8 * 2^-24 * (4 (|X| + |Y| + 2) + |z|) per cell: the kernel forms a residual z - (a X + b Y) in at most five f32
             roundings of terms bounded by that sum (|a|, |b| <= 4).  The kernel's c_lo is min_k (res_k + e_k) with |e_k| <= tol_k,
             so  min_k (res_k - tol_k) <= c_lo <= min_k (res_k + tol_k): the right-hand side is validity (no cell below the band),
             the left-hand side tightness; c_hi likewise with maxima.
  slopes     16 * 2^-24 * max|z| over the tile: a 64-term f32 tree sum plus the division is at most 7 roundings per mean, four
             means are combined and scaled by 1/16 -- about 4 * 2^-24 * max|z|; the bound allows four times that.
Texels are compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SHAPES = [(2, 2), (16, 16), (24, 40), (30, 34), (64, 258), (256, 256)]
FAMILIES = ("dome", "plane", "noise", "constant", "offset", "nonfinite", "nan_quadrant")
# (H, W, N, stride the sample table must select): dt = 0.8 / N, group = 4 -> the footprint of a group is 3 dt max(H, W) cells
COARSE = [(256, 256, 64, 16), (256, 256, 32, 32), (30, 34, 13, 16), (30, 34, 5, 32)]


def _depth(family, B, H, W):
    """(B, H, W) f32, every image different"""
    rng = np.random.default_rng([FAMILIES.index(family), B, H, W])
    r, c = np.mgrid[0:H, 0:W].astype(np.float64)
    X, Y = c - 0.5 * W, 0.5 * H - r
    out = np.empty((B, H, W), np.float64)
    for b in range(B):
        if family in ("dome", "offset", "nonfinite", "nan_quadrant"):
            cx, cy = (0.1 + 0.2 * b) * W, (-0.15 + 0.1 * b) * H
            z = (60.0 + 15.0 * b) * np.exp(-(((X - cx) / (0.35 * W + 1.0)) ** 2 + ((Y - cy) / (0.3 * H + 1.0)) ** 2)) - 20.0
            z += 0.25 * rng.random((H, W))
            if family == "offset":
                z += 1000.0
        elif family == "plane":
            a, bb = ((0.5, -6.0), (6.0, 0.5), (-0.5, 0.25))[b % 3]   # slope 6 is clamped to 4
            z = a * X + bb * Y + 3.0
        elif family == "noise":
            z = rng.uniform(-100.0, 100.0, (H, W))
        else:
            z = np.full((H, W), 37.5 - 11.0 * b)
        out[b] = z
    out = out.astype(np.float32)
    if family == "nonfinite":
        for b in range(B):
            holes = rng.random((H, W)) < 0.06
            out[b][holes] = np.nan
            k = max(1, (H * W) // 400)
            out[b][rng.integers(0, H, k), rng.integers(0, W, k)] = np.inf
            out[b][rng.integers(0, H, k), rng.integers(0, W, k)] = -np.inf
            out[b, 0, 0] = np.nan                                    # a wrap partner among them
            out[b, H - 1, W - 1] = np.inf if b % 2 else np.nan
    if family == "nan_quadrant":
        for b in range(B):
            rs = slice(0, H // 2) if b % 2 == 0 else slice(H // 2, H)
            cs = slice(W // 2, W) if b % 3 == 0 else slice(0, W // 2)
            out[b][rs, cs] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def _prepass(family, B, H, W, N):
    """depth, the workspace's texels (B, H+1, W+1, 4), records (B, zb_max_tiles, 4) and log2 of the stride in tflag"""
    from geomconsistentfr_amd import _lib, block as R, RenderParams
    L_ = _lib.load()
    dev = torch.device("cuda:0")
    depth = _depth(family, B, H, W)
    d = torch.from_numpy(depth).to(dev)
    m = torch.ones((B, H, W), dtype=torch.uint8, device=dev)
    light = torch.tensor([[[1200.0, 2400.0, 3000.0]]], device=dev).repeat(B, 1, 1)
    prm = RenderParams(n_samples=N, dt=0.8 / N)
    tt = R.sample_table(prm, dev)
    md = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    ws_bytes = int(L_.gcfr_shadow_workspace_bytes(B, H, W))
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)   # (a pattern no record or texel of these inputs holds)
    opt = _lib.options(ksplit=0, phase=1)
    _lib.check(L_.gcfr_shadow_fwd(d.data_ptr(), m.data_ptr(), B, light.data_ptr(), B, 1, H, W, N, tt.data_ptr(), 0.0, None,
                                  md.data_ptr(), None, ws.data_ptr(), ws_bytes, None, _lib.opt_ref(opt)), "gcfr_shadow_fwd")
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    # workspace layout (csrc/gcfr_shadow.hip shadow_fwd_impl): texels | statistics boxes | [records | horizon tables] | z ranges | tflag
    n_raw = (H * W + 16383) // 16384
    n_stat = (H * W + 32767) // 32768 if 8 < n_raw <= 16 else n_raw
    n_tiles = ((H >> 3) + 1) * ((W >> 3) + 1) + 1
    zb_stride = (n_tiles + 63) & ~63
    slot = zb_stride + 4 * 1024 if (W % 4 == 0 and W <= 1024 and H <= 1024) else zb_stride
    texels = raw[:B * (H + 1) * (W + 1) * 16].view(np.float32).reshape(B, H + 1, W + 1, 4).copy()
    zb0 = B * (H + 1) * (W + 1) * 16 + B * n_stat * 16
    rec = raw[zb0:zb0 + B * slot * 16].view(np.float32).reshape(B, slot, 4)[:, :n_tiles].copy()
    tflag = raw[zb0 + B * slot * 16 + B * n_stat * 8:][:20].view(np.int32)
    assert tflag[1] & 0xff in (3, 4, 5), tflag
    return depth, texels, rec, int(tflag[1] & 0xff)


def _check_records(depth, rec, ls, label):
    B, H, W = depth.shape
    s = 1 << ls
    nth, ntw = (H >> ls) + 1, (W >> ls) + 1
    sentinel = ((H >> 3) + 1) * ((W >> 3) + 1)
    er, ec = np.arange(H + 1), np.arange(W + 1)
    Xc = np.full((ntw + 1) * s, np.nan)
    Yc = np.full((nth + 1) * s, np.nan)
    Xc[:W + 1] = (ec - 1) - 0.5 * W
    Yc[:H + 1] = 0.5 * H - (er - 1)
    win = np.lib.stride_tricks.sliding_window_view
    Xt = win(Xc, 2 * s)[::s][None, :, None, :]              # (1, ntw, 1, 2s)
    Yt = win(Yc, 2 * s)[::s][:, None, :, None]              # (nth, 1, 2s, 1)
    for b in range(B):
        z = depth[b].astype(np.float64)
        E = np.full(((nth + 1) * s, (ntw + 1) * s), np.nan)
        E[:H + 1, :W + 1] = z[(er - 1) % H][:, (ec - 1) % W]   # cells outside the plane: NaN, dropped like NaN cells
        T = win(E, (2 * s, 2 * s))[::s, ::s]                   # (nth, ntw, 2s, 2s): every tile's extended cells
        assert T.shape[:2] == (nth, ntw)
        g = rec[b, :nth * ntw].astype(np.float64).reshape(nth, ntw, 4)
        a, bb, c_lo, c_hi = g[..., 0], g[..., 1], g[..., 2], g[..., 3]
        assert np.isfinite(a).all() and np.isfinite(bb).all(), label
        assert (np.abs(a) <= 4.0).all() and (np.abs(bb) <= 4.0).all(), label
        assert rec[b, sentinel].tolist() == [0.0, 0.0, -np.inf, np.inf], (label, rec[b, sentinel])
        # bands: validity and tightness
        live = ~np.isnan(T)
        fin = np.isfinite(T)
        with np.errstate(invalid="ignore"):
            res = T - (a[..., None, None] * Xt + bb[..., None, None] * Yt)
            tol = 8.0 * EPS * (4.0 * (np.abs(Xt) + np.abs(Yt) + 2.0) + np.where(fin, np.abs(T), 0.0))
            lo_min = np.where(live, res - tol, np.inf).min(axis=(2, 3))
            lo_max = np.where(live, res + tol, np.inf).min(axis=(2, 3))
            hi_min = np.where(live, res - tol, -np.inf).max(axis=(2, 3))
            hi_max = np.where(live, res + tol, -np.inf).max(axis=(2, 3))
        bad = ~((lo_min <= c_lo) & (c_lo <= lo_max) & (hi_min <= c_hi) & (c_hi <= hi_max))
        assert not bad.any(), (label, b, np.argwhere(bad)[:6], g[bad][:3], lo_min[bad][:3], lo_max[bad][:3], hi_min[bad][:3], hi_max[bad][:3])
        # slopes: from the means of the finite proper cells of the four s x s quadrants
        P = E.copy()
        P[0, :] = np.nan
        P[:, 0] = np.nan
        P[~np.isfinite(P)] = np.nan
        Pq = P.reshape(nth + 1, s, ntw + 1, s)
        cnt = (~np.isnan(Pq)).sum(axis=(1, 3))
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.nansum(Pq, axis=(1, 3)) / cnt
            m00, m01, m10, m11 = mean[:-1, :-1], mean[:-1, 1:], mean[1:, :-1], mean[1:, 1:]
            a_ref = np.clip(((m01 + m11) - (m00 + m10)) * (0.5 / s), -4.0, 4.0)
            b_ref = -np.clip(((m10 + m11) - (m00 + m01)) * (0.5 / s), -4.0, 4.0)
        populated = (cnt[:-1, :-1] > 0) & (cnt[:-1, 1:] > 0) & (cnt[1:, :-1] > 0) & (cnt[1:, 1:] > 0)
        assert (a[~populated] == 0.0).all() and (bb[~populated] == 0.0).all(), (label, b)
        zmax = np.where(fin, np.abs(T), 0.0).max(axis=(2, 3))
        with np.errstate(invalid="ignore"):
            off = populated & ~((np.abs(a - a_ref) <= 16.0 * EPS * zmax) & (np.abs(bb - b_ref) <= 16.0 * EPS * zmax))
        assert not off.any(), (label, b, np.argwhere(off)[:6], g[off][:3], a_ref[off][:3], b_ref[off][:3])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_bounds_records_match_their_definition(H, W, B):
    for family in FAMILIES:
        depth, _, rec, ls = _prepass(family, B, H, W, 160)
        assert ls == 3, (H, W, ls)
        _check_records(depth, rec, ls, (family, B, H, W))


@pytest.mark.parametrize("H,W,N,stride", COARSE)
def test_bounds_records_of_the_coarser_strides(H, W, N, stride):
    for family in ("dome", "nonfinite"):
        depth, _, rec, ls = _prepass(family, 3, H, W, N)
        assert 1 << ls == stride, (H, W, N, ls)
        _check_records(depth, rec, ls, (family, H, W, N))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_texels_are_the_wrapped_neighbourhoods(H, W, B):
    for family in FAMILIES:
        depth, texels, _, _ = _prepass(family, B, H, W, 160)
        r0, r1 = (np.arange(H + 1) - 1) % H, np.arange(H + 1) % H       # build_quad_kernel: row -1 is the last row, row H row 0
        c0, c1 = (np.arange(W + 1) - 1) % W, np.arange(W + 1) % W
        for b in range(B):
            z = depth[b]
            want = np.stack([z[r0][:, c0], z[r0][:, c1], z[r1][:, c0], z[r1][:, c1]], axis=-1)
            same = want.view(np.uint32) == texels[b].view(np.uint32)
            assert same.all(), (family, b, H, W, np.argwhere(~same)[:6])
