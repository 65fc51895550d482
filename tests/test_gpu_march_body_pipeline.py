"""The group body of the six-wave inference grid march -- a rotating pair of texel gathers, the next group's prefetch
requested behind the body's last gather, the group's masked flags in one register -- against the plain kernel (no
workspace) and the C oracle: minimum distance bit for bit, every fused output byte for byte.

Under test: the grid kernels with the k-split forced off (`options(ksplit=0)`), from depth and with normals handed in, for
groups of 4, 2 and 1 and tile widths 8, 16, 32 and 64 (every unit compiles the same header).  What the schedule can break,
and the smallest inputs that show it:
  * n_samples in {1, 2, 3, 4, 5, 7, 9, 24}: the last group is shorter than the pair or the group, so the clamped index
    re-evaluates the last sample while a gather for it is in flight, and the late prefetch addresses the group behind the
    last one;
  * (H, W) in {(4, 16), (6, 10), (18, 34), (64, 64)} with B up to 3 and L up to 2: partial tiles, both half-parities;
  * masks: random with 30 % zeros, all ones, a single non-zero cell, a non-zero band one row wide (groups alternate body /
    skip / body: both placements of the prefetch, the hand-over to the trailing loop and back out of it);
  * depth: smooth, and noise large enough that some tiles give the bounds up (the rough loop: untouched, still equal);
  * every output inside one buffer with guard bands of a NaN pattern round it and the pattern in it: one comparison of the
    whole buffer says that the guards are untouched, every element was written and every bit is the reference's.
The CPU test says with the C oracle that the set is not vacuous: masked and unmasked minima both occur, some minimum is
taken at the first sample (a body in a tile's first group) and some at the last (a body in its last group).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

DEV = "cuda:0"
F, Z_OFF = 1570.0, 1610.0
T0 = 0.025
GUARD = 64

SHAPES = [(4, 16, 1, 2), (6, 10, 2, 2), (18, 34, 3, 2), (64, 64, 2, 1)]      # (H, W, B, L)
N_SAMPLES = (1, 2, 3, 4, 5, 7, 9, 24)
MASKS = ("random", "ones", "single", "band")
DEPTHS = ("smooth", "noise")
GROUPS = (4, 2, 1)
TILE_WS = (8, 16, 32, 64)
OUT_KEYS = ("unit_light_direction", "light_pt", "minimum_distance", "shadow_mask_weights", "full_shading", "final_shading",
            "rendered_images", "surface_normals")


def params(H, W, n):
    from geomconsistentfr_amd import RenderParams
    # a light 30 px away: some lights project inside the image (end points inside the box, the `inside` bonus), some outside;
    # the table ends at t = 0.925 whatever its length
    return RenderParams(n_samples=n, t0=T0, dt=0.9 / n, light_distance=30.0, inside_bonus=5.0,
                        bonus_box=(-(W / 2.0), W - W / 2.0 - 1, 1 - H / 2.0, H / 2.0))


@functools.lru_cache(maxsize=None)
def scene_np(H, W, B, L, mask_kind, depth_kind):
    """depth, mask, light, ambient, albedo (numpy); every face its own depth, albedo, lights and ambient values"""
    rng = np.random.default_rng(1000 * H + 10 * W + B + 7 * L)
    r, c = np.mgrid[0:H, 0:W]
    depth = np.stack([0.3 * max(H, W) * np.exp(-(((c - (0.45 + 0.05 * b) * W) / (0.3 * W)) ** 2 + ((r - 0.5 * H) / (0.3 * H)) ** 2))
                      for b in range(B)])
    if depth_kind == "noise":   # rougher than the rays rise: tiles give the bounds up
        depth = depth + 40.0 * rng.random((B, H, W))
    depth = depth.astype(np.float32)
    if mask_kind == "ones":
        mask = np.ones((B, H, W), np.uint8)
    elif mask_kind == "single":
        mask = np.zeros((B, H, W), np.uint8)
        mask[:, H // 2, W // 2] = 1
    elif mask_kind == "band":
        mask = np.zeros((B, H, W), np.uint8)
        mask[:, H // 2, :] = 1
    else:
        mask = (rng.random((B, H, W)) > 0.3).astype(np.uint8)
        mask[:, H // 2, W // 2] = 1      # (never empty)
        mask[:, 0, 0] = 0                # (never all ones)
    light = rng.standard_normal((B, L, 3)).astype(np.float32)
    light[..., 2] = np.abs(light[..., 2]) + 0.2
    ambient = (0.1 + rng.random((B, L))).astype(np.float32)
    albedo = (0.05 + rng.random((B, 3, H, W)) + np.arange(B)[:, None, None, None]).astype(np.float32)
    return depth, mask, light, ambient, albedo


@functools.lru_cache(maxsize=None)
def scene(H, W, B, L, mask_kind, depth_kind):
    return tuple(torch.from_numpy(a).to(DEV) for a in scene_np(H, W, B, L, mask_kind, depth_kind))


def camera_matrix(H, W):
    K = torch.zeros(1, 3, 3, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = F
    K[:, 2, 2] = 1.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    return K.to(DEV)


def layout(out):
    """(key, offset, elements) of every output inside the guarded buffer, and the buffer's length"""
    off, rows = GUARD, []
    for k in OUT_KEYS:
        if out.get(k) is not None:
            n = out[k].numel()
            rows.append((k, off, n))
            off += n + GUARD
    return rows, off


@functools.lru_cache(maxsize=None)
def reference(H, W, B, L, n, mask_kind, depth_kind):
    """The plain kernel (no workspace), then the stand-alone normals and shading kernels; its minimum distance is compared with
    the C oracle's here, once.  Returns the outputs by name and the two guarded buffers (normals handed in / from depth) a fused
    launch must reproduce bit for bit."""
    import c_oracle
    from geomconsistentfr_amd import light_prep, shadow_min_distance
    from geomconsistentfr_amd.block import shade
    from geomconsistentfr_amd.normals import depth_to_normals
    depth, mask, light, ambient, albedo = scene(H, W, B, L, mask_kind, depth_kind)
    prm = params(H, W, n)
    unit, pt = light_prep(light, prm)
    md, _ = shadow_min_distance(depth, mask, pt, prm, want_argmin=False, use_workspace=False)
    md_o, _ = c_oracle.shadow_min_distance(depth.cpu().numpy(), mask.cpu().numpy(), pt.cpu().numpy(), c_oracle.sample_table(T0, 0.9 / n, n),
                                           bonus=prm.inside_bonus, bonus_box=prm.bonus_box)
    np.testing.assert_array_equal(md.cpu().numpy(), md_o, err_msg="the plain kernel against the C oracle")
    nrm = depth_to_normals(depth[:, None], camera_matrix(H, W), z_offset=Z_OFF)
    out = shade(nrm, depth, albedo, pt, ambient, md, prm)
    out.update(minimum_distance=md, surface_normals=nrm, light_pt=pt, unit_light_direction=unit)
    bufs = {}
    for given in (True, False):
        named = {k: v for k, v in out.items() if k in OUT_KEYS and not (given and k == "surface_normals")}
        rows, total = layout(named)
        buf = torch.full((total,), float("nan"), dtype=torch.float32, device=DEV)
        for k, off, cnt in rows:
            buf[off:off + cnt] = named[k].reshape(-1)
        bufs[given] = buf
    return out, bufs


def fused_guarded(monkeypatch, H, W, B, L, n, mask_kind, depth_kind, given, options):
    """one fused launch with every output carved out of one NaN-filled buffer, guard bands between them: (outputs, buffer)"""
    from geomconsistentfr_amd import block as R
    depth, mask, light, ambient, albedo = scene(H, W, B, L, mask_kind, depth_kind)
    real_alloc = R._alloc_forward
    made = []

    def alloc(B_, L_, H_, W_, dev, want_argmin, normals_out, prepared=None):
        out, ws, ws_bytes = real_alloc(B_, L_, H_, W_, dev, want_argmin, normals_out, prepared)
        assert out["argmin"] is None
        rows, total = layout(out)
        buf = torch.full((total,), float("nan"), dtype=torch.float32, device=dev)
        for k, off, cnt in rows:
            out[k] = buf[off:off + cnt].view(out[k].shape)
        made.append(buf)
        return out, ws, ws_bytes

    monkeypatch.setattr(R, "_alloc_forward", alloc)
    try:
        normals = reference(H, W, B, L, n, mask_kind, depth_kind)[0]["surface_normals"] if given else None
        got = R.render_fwd(depth, mask, light, ambient, normals, albedo, params(H, W, n), want_argmin=False,
                           camera=None if given else (F, F, W / 2.0, H / 2.0, Z_OFF), options=options)
    finally:
        monkeypatch.setattr(R, "_alloc_forward", real_alloc)
    assert len(made) == 1
    return got, made[0]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_SAMPLES)
@pytest.mark.parametrize("H,W,B,L", SHAPES)
def test_grid_march_equals_the_plain_kernel_and_the_c_oracle_bit_for_bit(H, W, B, L, n, monkeypatch):
    """every mask, both depths, groups of 4 / 2 / 1, tile widths 8 ... 64, normals handed in and from depth, k-split off"""
    from geomconsistentfr_amd import _lib
    for mask_kind in MASKS:
        for depth_kind in DEPTHS:
            ref, bufs = reference(H, W, B, L, n, mask_kind, depth_kind)
            for group in GROUPS:
                for tile_w in TILE_WS:
                    opt = _lib.options(tile_w=tile_w, group=group, ksplit=0)
                    for given in (True, False):
                        got, buf = fused_guarded(monkeypatch, H, W, B, L, n, mask_kind, depth_kind, given, opt)
                        if same_bits(buf, bufs[given]):
                            continue
                        what = (mask_kind, depth_kind, "group %d" % group, "tile_w %d" % tile_w, "given" if given else "from depth")
                        for k in OUT_KEYS:   # say which: an output, or the guards
                            if got.get(k) is not None:
                                assert same_bits(got[k], ref[k].reshape(got[k].shape)), (what, k)
                        raise AssertionError((what, "a guard band was written"))


def test_the_cases_are_not_vacuous():
    """CPU, the C oracle: across the set masked and unmasked minima both occur, some pixel's minimum is its FIRST sample (its
    tile runs a body in its first group) and some pixel's its LAST one (a body in the last group), for every table longer than
    one group of four"""
    import c_oracle
    seen_masked = seen_lit = False
    for n in N_SAMPLES:
        first = last = False
        for H, W, B, L in SHAPES:
            for mask_kind in MASKS:
                for depth_kind in DEPTHS:
                    depth, mask, light, ambient, albedo = scene_np(H, W, B, L, mask_kind, depth_kind)
                    _, pt = c_oracle.light_prep(light.reshape(-1, 3), clamp_z_min=0.0, light_distance=30.0)
                    md, am = c_oracle.shadow_min_distance(depth, mask, pt.reshape(B, L, 3), c_oracle.sample_table(T0, 0.9 / n, n))
                    lit = md < 1e5
                    seen_masked |= bool((~lit).any())
                    seen_lit |= bool(lit.any())
                    first |= bool((am[lit] == 0).any())
                    last |= bool((am[lit] == n - 1).any())
        assert first and last, (n, first, last)
    assert seen_masked and seen_lit
