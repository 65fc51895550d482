"""GPU: the march's fused epilogue (gcfr_render_fwd, gcfr_render_from_depth_fwd) against the three-stage path
(shadow_min_distance, depth_to_normals, shade), bit for bit, at the smallest shapes at which the ORDER of the epilogue's
memory operations can go wrong.

The epilogue requests every operand it reads from memory -- its arguments, the 3 x 3 depth neighbourhood or the normals
handed in, the albedo planes, ambient[b, l] -- in one batch directly behind the sample loop, for the pixel a fresh lane id
re-derives, and only then stores.  What that can break: a pixel index derived differently for the loads and for the stores
(partial tiles, whose lanes are clamped to (H - 1, W - 1) and must leave before the first store); albedo / ambient taken
from the wrong face or light (albedo is indexed by b, ambient and the outputs by (b, l)); the batch placed outside the
k-split kernel's `wave 0` condition; a store outside its plane.

Shapes (H, W).  The library takes even H and W only (odd ones are GCFR_ERR_INVALID_ARGUMENT at the boundary, asserted
below), so the odd shapes one would reach for first, (5, 7) and (17, 33), are stood in for by their even neighbours:
(6, 10) a partial tile in each direction and a partial workgroup; (4, 16) exactly one 16 x 4 tile; (6, 18) partial tiles
in a second workgroup column; (8, 24) a partial tile with H/2 and W/2 even; (18, 34) with B = 3, L = 2 and a distinct
albedo, ambient and light per face and light -- the combination in which a value taken from the wrong face or light shows
up on a partial tile; (64, 64) whole tiles in several workgroups.  (6, 10), (6, 18) and (18, 34) have H/2 or W/2 odd:
the other half-parity instantiation of every kernel.  The schedule is chosen by the launch's tile count (k-split up to
2048 tiles: every one of these shapes at every B here), so each case runs as the library picks it AND with the k-split
forced off (the grid kernel the bench workload runs) AND forced on.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, Z_OFF = 1570.0, 1610.0
N_SAMPLES, T0, DT = 24, 0.025, 0.04      # (N >= 16: the k-split kernel takes tiny launches)
GUARD = 64

# (H, W, B, L)
CASES = [(6, 10, 1, 1), (6, 10, 2, 2), (4, 16, 1, 2), (4, 16, 2, 1), (6, 18, 1, 1), (6, 18, 2, 2), (8, 24, 2, 2), (18, 34, 3, 2),
         (64, 64, 1, 1), (64, 64, 2, 2), (64, 64, 3, 1)]
MODES = ("inference", "argmin", "mask")   # want_argmin=False | want_argmin=True | pixels="mask" (forces the argmin march)
FLOAT_KEYS = ("minimum_distance", "shadow_mask_weights", "full_shading", "final_shading", "rendered_images")


def params(H, W, mode):
    from geomconsistentfr_amd import RenderParams
    # a light 30 px away: some lights project inside the image (the `inside` bonus, end points inside the box), some outside
    return RenderParams(n_samples=N_SAMPLES, t0=T0, dt=DT, light_distance=30.0, inside_bonus=5.0,
                        bonus_box=(-(W / 2.0), W - W / 2.0 - 1, 1 - H / 2.0, H / 2.0),
                        pixels="mask" if mode == "mask" else "all")


@functools.lru_cache(maxsize=None)
def scene(H, W, B, L, mask_kind):
    """depth, mask, light, ambient, albedo on the device; every face its own depth, albedo, lights and ambient values"""
    rng = np.random.default_rng(1000 * H + 10 * W + B + 7 * L)
    r, c = np.mgrid[0:H, 0:W]
    depth = np.stack([0.3 * max(H, W) * np.exp(-(((c - (0.45 + 0.05 * b) * W) / (0.3 * W)) ** 2 + ((r - 0.5 * H) / (0.3 * H)) ** 2))
                      + 0.5 * rng.random((H, W)) for b in range(B)]).astype(np.float32)
    if mask_kind == "ones":
        mask = np.ones((B, H, W), np.uint8)
    else:
        mask = (rng.random((B, H, W)) > 0.3).astype(np.uint8)
        mask[:, H // 2, W // 2] = 1      # (never empty)
        mask[:, 0, 0] = 0                # (never all ones)
    light = rng.standard_normal((B, L, 3)).astype(np.float32)
    light[..., 2] = np.abs(light[..., 2]) + 0.2
    ambient = (0.1 + rng.random((B, L))).astype(np.float32)
    albedo = (0.05 + rng.random((B, 3, H, W)) + np.arange(B)[:, None, None, None]).astype(np.float32)   # face b: values in [b, b + 1.05]
    return tuple(torch.from_numpy(a).to(DEV) for a in (depth, mask, light, ambient, albedo))


def camera_matrix(H, W):
    K = torch.zeros(1, 3, 3, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = F
    K[:, 2, 2] = 1.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    return K.to(DEV)


def three_stage(depth, mask, light, ambient, albedo, prm, want_argmin):
    """the reference of every comparison here: each stage its own launch, in the stand-alone kernels"""
    from geomconsistentfr_amd import light_prep, shadow_min_distance
    from geomconsistentfr_amd.block import shade
    from geomconsistentfr_amd.normals import depth_to_normals
    B, H, W = depth.shape
    unit, pt = light_prep(light, prm)
    md, am = shadow_min_distance(depth, mask, pt, prm, want_argmin=want_argmin)
    n = depth_to_normals(depth[:, None], camera_matrix(H, W), z_offset=Z_OFF)
    out = shade(n, depth, albedo, pt, ambient, md, prm)
    out.update(minimum_distance=md, argmin=am, surface_normals=n, light_pt=pt, unit_light_direction=unit)
    return out


@functools.lru_cache(maxsize=None)
def reference(H, W, B, L, mask_kind, mode):
    depth, mask, light, ambient, albedo = scene(H, W, B, L, mask_kind)
    return three_stage(depth, mask, light, ambient, albedo, params(H, W, mode), mode != "inference")


def same_bits(a, b):
    """bit for bit, NaNs included"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def schedules(W):
    from geomconsistentfr_amd import _lib
    return [("auto", None), ("grid", _lib.options(ksplit=0)), ("ksplit", _lib.options(ksplit=1))]


def fused(H, W, B, L, mask_kind, mode, given, options):
    from geomconsistentfr_amd import block as R
    depth, mask, light, ambient, albedo = scene(H, W, B, L, mask_kind)
    normals = reference(H, W, B, L, mask_kind, mode)["surface_normals"] if given else None
    cam = None if given else (F, F, W / 2.0, H / 2.0, Z_OFF)
    return R.render_fwd(depth, mask, light, ambient, normals, albedo, params(H, W, mode), want_argmin=(mode == "argmin"),
                        camera=cam, options=options)


def compare(got, ref, mode, given, what):
    for k in FLOAT_KEYS + ("light_pt", "unit_light_direction"):
        assert same_bits(got[k], ref[k].reshape(got[k].shape)), (what, k)
    if mode == "inference":
        assert got["argmin"] is None, what
    else:
        assert torch.equal(got["argmin"], ref["argmin"]), (what, "argmin")
    if not given:
        assert same_bits(got["surface_normals"], ref["surface_normals"]), (what, "surface_normals")


@pytest.mark.parametrize("H,W,B,L", CASES)
def test_fused_epilogue_equals_the_three_stage_path_bit_for_bit(H, W, B, L):
    """every returned array of gcfr_render_fwd / gcfr_render_from_depth_fwd == shadow_min_distance, depth_to_normals, shade:
    normals handed in and from depth; inference, want_argmin, pixels = mask; an all-ones mask and one with zeros; every schedule"""
    for mask_kind in ("ones", "zeros"):
        for mode in MODES:
            ref = reference(H, W, B, L, mask_kind, mode)
            for given in (True, False):
                for sname, opt in schedules(W):
                    if mode == "mask" and sname == "ksplit":
                        continue      # (pixels = mask lives in the grid schedule's own kernel)
                    got = fused(H, W, B, L, mask_kind, mode, given, opt)
                    compare(got, ref, mode, given, (mask_kind, mode, "given" if given else "from depth", sname))


@pytest.mark.parametrize("H,W,B,L", CASES)
def test_minimum_distance_equals_the_c_oracle_bit_for_bit(H, W, B, L):
    """the fused forward's minimum_distance (and argmin) against the C oracle, as tests/test_gpu_parity.py compares them"""
    import c_oracle
    tt = c_oracle.sample_table(T0, DT, N_SAMPLES)
    for mask_kind in ("ones", "zeros"):
        depth, mask, light, ambient, albedo = scene(H, W, B, L, mask_kind)
        prm = params(H, W, "argmin")
        pt = reference(H, W, B, L, mask_kind, "argmin")["light_pt"].cpu().numpy()
        md_o, am_o = c_oracle.shadow_min_distance(depth.cpu().numpy(), mask.cpu().numpy(), pt, tt, bonus=prm.inside_bonus,
                                                  bonus_box=prm.bonus_box)
        lit = md_o < 1e5
        own_on = np.broadcast_to(mask.cpu().numpy()[:, None] != 0, md_o.shape)
        for mode in MODES:
            for given in (True, False):
                for sname, opt in schedules(W)[:2]:
                    got = fused(H, W, B, L, mask_kind, mode, given, opt)
                    md = got["minimum_distance"].cpu().numpy()
                    what = (mask_kind, mode, given, sname)
                    if mode == "mask":   # pixels outside the mask are not marched: the masked value (+ the bonus where the light is inside)
                        np.testing.assert_array_equal(md[own_on], md_o[own_on], err_msg=str(what))
                        assert (md[~own_on] >= 1e5).all(), what
                    else:
                        np.testing.assert_array_equal(md, md_o, err_msg=str(what))
                    if mode != "inference":
                        am = got["argmin"].cpu().numpy()
                        sel = lit & own_on if mode == "mask" else lit
                        assert np.all(am[~lit] == -1), what
                        np.testing.assert_array_equal(am[sel], am_o[sel], err_msg=str(what))


def guarded(shape, dtype, keep):
    """a tensor of `shape` inside a larger buffer: GUARD elements of a pattern before and after it, the pattern in it too"""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    else:
        buf = torch.full((n + 2 * GUARD,), -12345, dtype=dtype, device=DEV)
    keep.append((buf, n))
    return buf[GUARD:GUARD + n].view(shape)


def unwritten(t):
    return torch.isnan(t) if t.dtype == torch.float32 else (t == -12345)


@pytest.mark.parametrize("H,W,B,L", [(6, 10, 2, 2), (4, 16, 1, 2), (6, 18, 2, 2), (18, 34, 3, 2), (64, 64, 3, 1)])
def test_outputs_are_written_completely_and_nothing_outside_them(H, W, B, L, monkeypatch):
    """every output plane inside a larger buffer with 64 guard elements of a NaN pattern (argmin: a sentinel) either side and
    the pattern in the plane itself: afterwards the guards are untouched and every element of every output has been written"""
    from geomconsistentfr_amd import block as R
    real_alloc = R._alloc_forward
    for mask_kind in ("ones", "zeros"):
        for mode in MODES:
            for given in (True, False):
                for sname, opt in schedules(W):
                    if mode == "mask" and sname == "ksplit":
                        continue
                    keep = []

                    def alloc(B_, L_, H_, W_, dev, want_argmin, normals_out, prepared=None):
                        out, ws, ws_bytes = real_alloc(B_, L_, H_, W_, dev, want_argmin, normals_out, prepared)
                        for k, v in list(out.items()):
                            if v is not None:
                                out[k] = guarded(tuple(v.shape), v.dtype, keep)
                        return out, ws, ws_bytes

                    monkeypatch.setattr(R, "_alloc_forward", alloc)
                    got = fused(H, W, B, L, mask_kind, mode, given, opt)
                    torch.cuda.synchronize()
                    monkeypatch.setattr(R, "_alloc_forward", real_alloc)
                    what = (mask_kind, mode, given, sname)
                    assert len(keep) == sum(v is not None for v in got.values()), what
                    for buf, n in keep:
                        assert bool(unwritten(buf[:GUARD]).all()) and bool(unwritten(buf[GUARD + n:]).all()), what
                    for k, v in got.items():
                        if v is not None:
                            assert not bool(unwritten(v).any()), (what, k)
                    compare(got, reference(H, W, B, L, mask_kind, mode), mode, given, what)


def test_non_finite_depth_at_the_image_corner_poisons_exactly_its_neighbourhood():
    """6 x 10: the lanes of the partial tile are clamped to (H - 1, W - 1) and load there; a NaN in that cell and an inf at
    (0, 0) must poison exactly the normals whose clamped 3 x 3 neighbourhood holds them (include/gcfr.h), and the fused
    forward must still equal the three-stage path in every bit, NaNs included"""
    from geomconsistentfr_amd import block as R
    H, W, B, L = 6, 10, 2, 2
    depth, mask, light, ambient, albedo = scene(H, W, B, L, "zeros")
    clean = reference(H, W, B, L, "zeros", "argmin")
    bad = depth.clone()
    bad[0, H - 1, W - 1] = float("nan")
    bad[1, 0, 0] = float("inf")
    for mode in MODES:
        prm = params(H, W, mode)
        ref = three_stage(bad, mask, light, ambient, albedo, prm, mode != "inference")
        poisoned = ~torch.isfinite(ref["surface_normals"]).all(dim=1)
        expect = torch.zeros((B, H, W), dtype=torch.bool, device=DEV)
        expect[0, H - 2:, W - 2:] = True
        expect[1, :2, :2] = True
        assert torch.equal(poisoned, expect), mode
        ok = ~expect[:, None].expand(B, 3, H, W)
        assert same_bits(ref["surface_normals"][ok], clean["surface_normals"][ok]), mode
        for given in (True, False):
            for sname, opt in schedules(W):
                if mode == "mask" and sname == "ksplit":
                    continue
                got = R.render_fwd(bad, mask, light, ambient, ref["surface_normals"] if given else None, albedo, prm,
                                   want_argmin=(mode == "argmin"), camera=None if given else (F, F, W / 2.0, H / 2.0, Z_OFF),
                                   options=opt)
                compare(got, ref, mode, given, (mode, given, sname))


@pytest.mark.parametrize("H,W", [(5, 7), (17, 33), (6, 7), (5, 8)])
def test_odd_sizes_are_rejected_at_the_boundary(H, W):
    """why no case above has an odd H or W: every forward entry refuses them before anything is launched"""
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import block as R
    dev = torch.device(DEV)
    depth = torch.zeros((1, H, W), device=dev)
    mask = torch.ones((1, H, W), dtype=torch.uint8, device=dev)
    light = torch.tensor([[[0.1, 0.2, 0.9]]], device=dev)
    ambient = torch.full((1, 1), 0.5, device=dev)
    albedo = torch.ones((1, 3, H, W), device=dev)
    with pytest.raises(_lib.GcfrError):
        R.render_fwd(depth, mask, light, ambient, None, albedo, params(H, W, "inference"), want_argmin=False,
                     camera=(F, F, W / 2.0, H / 2.0, Z_OFF))
    with pytest.raises(_lib.GcfrError):
        R.render_fwd(depth, mask, light, ambient, torch.ones((1, 3, H, W), device=dev), albedo, params(H, W, "inference"),
                     want_argmin=False)
