"""The bilinear weights of the bounds variant of the grid march as two v_fract_f64 per axis (csrc/gcfr_march.hpp: FRACT,
csrc/gcfr_device.hpp: bilinear_weights) against the plain kernel (no workspace, three-stage path: the reference's
floor / ceil / two subtractions) and the C oracle: the fused entries, from depth and with normals handed in, byte for byte in every
output.  The argmin (training) march is compared on the same cases in minimum distance and argmin: its kernels keep the parent's
weights (the new ones were built there, measured and not kept -- profiles/fract_weights_ab.txt), so it is the control that the cases,
the aimed lights and the small images mean the same to a kernel without them.

Under test: the grid kernels with the k-split forced off (`options(tile_w=..., group=..., ksplit=0)`), tile widths 8 ... 64, groups
of 4, 2 and 1, both half-parities.  Sizes are written W x H:
  * 6 x 6 and 8 x 6: the smallest sizes the new weights serve (odd and even W/2);
  * 18 x 6: partial tiles; 64 x 16: four tiles side by side, so the waves of a workgroup hold different rays; 8 x 8: even in both;
  * 4 x 4, 2 x 2, 4 x 8 and 8 x 4: fewer than six rows or columns -- these march in the rough sibling whatever their depth (use_zb
    in march_tile: a position of theirs can fall inside 0 < |u| <= 2^-54, where the fract weights are not the reference's);
  * one 256 x 256 face of tools/scenes.py with the training script's constants (default shape, 16 x 4 tiles and groups of four).
Lights (small cases, one face, four lights; the light distance a power of two and the raw light's z searched in its last places until the
norm rounds to that distance, so that light_prep returns the raw light itself; asserted): Cx equal to column 0's x (dxf == 0 and ux = -0.0001 on every sample of column 0: wx1 = 0.9999, texel
column -1), Cy equal to row 0's y (the same for uy), a light straight over the interior pixel (H/2, W/2), a grazing light.
Masks with holes, a single cell, all ones; smooth depth and depth rougher than the rays rise; a NaN light and a NaN depth cell
(compared with the plain kernel only: the C oracle is host code for finite inputs).
Every output lives inside one buffer with guard bands of a NaN pattern round it: one comparison of the whole buffer says that
the guards are untouched, every element was written and every bit is the reference's.

`test_the_cases_are_not_vacuous`: the counting build (lib/audit.so, made by `__graft_entry__.build()`) says that bodies ran under
the bounds where a case is meant to have them, and that the images of fewer than six rows or columns ran NO body under the bounds;
without a current counting build it fails.

Mutant 32 (csrc/gcfr_mutants.hpp, `tools/build_variant.sh mut_32 -DGCFR_MUT=32`, this file with GCFR_HIP_LIB=<that library>): wx0 and
wx1 exchanged in the new form; how many of the cases fail it: profiles/fract_weights_ab.txt (the fused cases of six or more rows and
columns must; the images that never reach the bounds variant and the argmin march cannot).
"""
import collections
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEV = "cuda:0"
F, Z_OFF = 1570.0, 1610.0
T0 = 0.025
GUARD = 64
GROUPS = (4, 2, 1)
TILE_WS = (8, 16, 32, 64)
OUT_KEYS = ("unit_light_direction", "light_pt", "minimum_distance", "shadow_mask_weights", "full_shading", "final_shading",
            "rendered_images", "surface_normals")
AUDIT_LIB = os.path.join(ROOT, "geomconsistentfr_amd", "lib", "audit.so")

# bounds: bodies are MEANT to run under the bounds (asserted with the counting build's numbers); small: fewer than six rows / columns
Case = collections.namedtuple("Case", "H W n mask depth nonfinite bounds face")


def case(W, H, n=24, mask="holes", depth="smooth", nonfinite=False, bounds=True, face=False):
    return Case(H, W, n, mask, depth, nonfinite, bounds and min(H, W) >= 6 and depth == "smooth", face)


CASES = {
    "6x6": case(6, 6),
    "6x6_ones": case(6, 6, mask="ones"),
    "8x6": case(8, 6),
    "8x6_single": case(8, 6, mask="single"),
    "8x8_ones": case(8, 8, mask="ones"),
    "18x6": case(18, 6),
    "18x6_ones_table_5": case(18, 6, n=5, mask="ones"),
    "64x16": case(64, 16, n=40),
    "64x16_ones": case(64, 16, n=40, mask="ones"),
    "64x16_rough": case(64, 16, depth="noise"),
    "64x16_nonfinite": case(64, 16, nonfinite=True),
    "4x4": case(4, 4),
    "4x4_ones": case(4, 4, mask="ones"),
    "2x2_ones": case(2, 2, mask="ones"),
    "4x8": case(4, 8),
    "8x4_ones": case(8, 4, mask="ones"),
    "face_256": case(256, 256, n=160, face=True),
}


def light_distance(c):
    """a power of two, at least 2.5 image sides: a raw light whose norm rounds to it exactly is scaled to itself by light_prep"""
    return float(2 ** int(np.ceil(np.log2(2.5 * max(c.H, c.W)))))


def params(c):
    from geomconsistentfr_amd import RenderParams
    if c.face:
        return RenderParams()
    # the table ends at t = 0.925 whatever its length; no clamp of the light's z (the lights are what the search below made them)
    return RenderParams(n_samples=c.n, t0=T0, dt=0.9 / c.n, light_distance=light_distance(c), clamp_light_z_min=None, inside_bonus=5.0,
                        bonus_box=(-(c.W / 2.0), c.W - c.W / 2.0 - 1, 1 - c.H / 2.0, c.H / 2.0))


def aimed_light(c, axis):
    """a raw light whose light POINT (the oracle's light_prep, the library's bit for bit: asserted in reference()) has x == -W/2
    (axis 0: column 0's x) or y == H/2 (axis 1: row 0's y) exactly, the other in-plane coordinate 0.25"""
    import c_oracle
    d = light_distance(c)
    raw = np.zeros(3, np.float32)
    raw[axis], raw[1 - axis] = (-c.W / 2.0, c.H / 2.0)[axis], 0.25
    z0 = np.float32(np.sqrt(d * d - float(raw[0]) ** 2 - float(raw[1]) ** 2))
    for k in range(2 * 64):   # the last places of z either side: the norm walks through the floats round d
        raw[2] = (z0.view(np.int32) + (k // 2 if k % 2 == 0 else -(k // 2) - 1)).view(np.float32)
        _, pt = c_oracle.light_prep(raw[None], clamp_z_min=None, light_distance=d)
        if pt[0, axis] == raw[axis]:
            return raw.copy()
    raise AssertionError("no raw light found", c, axis)


@functools.lru_cache(maxsize=None)
def scene_np(name):
    """depth (B,H,W), mask (B,H,W), light (B,L,3), ambient (B,L), albedo (B,3,H,W)"""
    c = CASES[name]
    if c.face:
        import scenes
        depth, mask, albedo, _, light, amb = scenes.synth_faces(1, 3)
        return depth, mask, light.reshape(1, 1, 3), amb.reshape(1, 1), albedo
    H, W = c.H, c.W
    rng = np.random.default_rng(sorted(CASES).index(name))
    r, col = np.mgrid[0:H, 0:W]
    depth = 0.3 * min(H, W) * np.exp(-(((col - 0.45 * W) / (0.3 * W)) ** 2 + ((r - 0.5 * H) / (0.3 * H)) ** 2))[None]
    if c.depth == "noise":   # rougher than the rays rise: tiles give the bounds up
        depth = depth + 40.0 * rng.random((1, H, W))
    depth = depth.astype(np.float32)
    if c.mask == "ones":
        mask = np.ones((1, H, W), np.uint8)
    elif c.mask == "single":
        mask = np.zeros((1, H, W), np.uint8)
        mask[:, H // 2, W // 2] = 1
    else:   # holes
        mask = (rng.random((1, H, W)) > 0.35).astype(np.uint8)
        mask[:, H // 2, W // 2] = 1      # (never empty)
        mask[:, 0, W - 1] = 0            # (never all ones)
        mask[:, :, 0] = 1                # column 0 and row 0: the pixels whose every sample sits at u = -0.0001 under the aimed lights
        mask[:, 0, :W - 1] = 1
    # column 0's x, row 0's y, straight over pixel (H/2, W/2) -- x = y = 0 --, grazing
    light = np.stack([aimed_light(c, 0), aimed_light(c, 1), np.array([0.0, 0.0, 1.0], np.float32),
                      np.array([0.9, 0.3, 0.05], np.float32)])[None]
    if c.nonfinite:
        light[0, 3, 0] = np.nan
        depth[0, H // 2, W // 3] = np.nan
    ambient = (0.1 + rng.random((1, 4))).astype(np.float32)
    albedo = (0.05 + rng.random((1, 3, H, W))).astype(np.float32)
    return depth, mask, light, ambient, albedo


@functools.lru_cache(maxsize=None)
def scene(name):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in scene_np(name))


def camera_matrix(H, W):
    import torch
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


def guarded(named):
    import torch
    rows, total = layout(named)
    buf = torch.full((total,), float("nan"), dtype=torch.float32, device=DEV)
    for k, off, cnt in rows:
        buf[off:off + cnt] = named[k].reshape(-1)
    return buf


@functools.lru_cache(maxsize=None)
def reference(name):
    """The plain kernel (no workspace) with its argmin, then the stand-alone normals and shading kernels; minimum distance and
    argmin are compared with the C oracle's here, once (finite inputs only).  Returns the outputs by name, the two guarded buffers
    (normals handed in / from depth) a fused launch must reproduce and the guarded (minimum distance, argmin) buffer of the march."""
    import c_oracle
    import torch
    from geomconsistentfr_amd import light_prep, shadow_min_distance
    from geomconsistentfr_amd.block import shade
    from geomconsistentfr_amd.normals import depth_to_normals
    c = CASES[name]
    depth, mask, light, ambient, albedo = scene(name)
    prm = params(c)
    unit, pt = light_prep(light, prm)
    pt_np = pt.cpu().numpy()
    if not c.face:   # the aimed lights sit where they were aimed, and the overhead one over x = y = 0
        assert pt_np[0, 0, 0] == -c.W / 2.0 and pt_np[0, 1, 1] == c.H / 2.0 and pt_np[0, 2, 0] == 0.0 and pt_np[0, 2, 1] == 0.0, pt_np
    md, am = shadow_min_distance(depth, mask, pt, prm, want_argmin=True, use_workspace=False)
    md_np = md.cpu().numpy()
    if not c.nonfinite:   # (the C oracle is host code for finite inputs: it turns positions into indices unchecked)
        md_o, am_o = c_oracle.shadow_min_distance(depth.cpu().numpy(), mask.cpu().numpy(), pt_np, c_oracle.sample_table(prm.t0, prm.dt, prm.n_samples),
                                                  bonus=prm.inside_bonus, bonus_box=prm.bonus_box)
        np.testing.assert_array_equal(md_np, md_o, err_msg="the plain kernel against the C oracle")
        lit = md_o < 1e5   # (argmin: -1 marks "the minimum is a masked sample"; the oracle keeps that sample's index)
        am_np = am.cpu().numpy()
        np.testing.assert_array_equal(am_np[lit], am_o[lit], err_msg="the plain kernel's argmin against the C oracle's")
        assert np.all(am_np[~lit] == -1)
    else:                 # the plain kernel alone is the reference, as in tests/test_gpu_parity.py's adversarial inputs
        assert np.isnan(md_np[0, 3]).all() and np.isfinite(md_np[0, 0]).sum() > 0
    nrm = depth_to_normals(depth[:, None], camera_matrix(c.H, c.W), z_offset=Z_OFF)
    out = shade(nrm, depth, albedo, pt, ambient, md, prm)
    out.update(minimum_distance=md, surface_normals=nrm, light_pt=pt, unit_light_direction=unit)
    bufs = {given: guarded({k: v for k, v in out.items() if k in OUT_KEYS and not (given and k == "surface_normals")})
            for given in (True, False)}
    out["argmin"] = am
    march_buf = torch.full((march_layout(c)[2],), float("nan"), dtype=torch.float32, device=DEV)
    march_buf[march_layout(c)[0]] = md.reshape(-1)
    march_buf[march_layout(c)[1]] = am.view(torch.float32).reshape(-1)
    return out, bufs, march_buf


def march_layout(c, L=None):
    """where minimum distance and argmin live inside the march's guarded buffer, and its length"""
    n = (1 if c.face else 4) * c.H * c.W
    return slice(GUARD, GUARD + n), slice(2 * GUARD + n, 2 * GUARD + 2 * n), 3 * GUARD + 2 * n


def fused_guarded(monkeypatch, name, given, options):
    """one fused launch with every output carved out of one NaN-filled buffer, guard bands between them: (outputs, buffer)"""
    import torch
    from geomconsistentfr_amd import block as R
    c = CASES[name]
    depth, mask, light, ambient, albedo = scene(name)
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
        normals = reference(name)[0]["surface_normals"] if given else None
        got = R.render_fwd(depth, mask, light, ambient, normals, albedo, params(c), want_argmin=False,
                           camera=None if given else (F, F, c.W / 2.0, c.H / 2.0, Z_OFF), options=options)
    finally:
        monkeypatch.setattr(R, "_alloc_forward", real_alloc)
    assert len(made) == 1
    return got, made[0]


def march_guarded(name, options):
    """the argmin march (gcfr_shadow_fwd with its workspace: the five-wave training grid kernels) with minimum distance and argmin
    carved out of one NaN-filled buffer: (minimum distance, argmin, buffer)"""
    import torch
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import block as R
    c = CASES[name]
    depth, mask, _, _, _ = scene(name)
    prm = params(c)
    pt = reference(name)[0]["light_pt"].reshape(1, -1, 3).contiguous()
    B, L = 1, pt.shape[1]
    md_at, am_at, total = march_layout(c)
    assert md_at.stop - md_at.start == B * L * c.H * c.W
    buf = torch.full((total,), float("nan"), dtype=torch.float32, device=DEV)
    md = buf[md_at].view(B, L, c.H, c.W)
    am = buf[am_at].view(torch.int32).view(B, L, c.H, c.W)
    lib = _lib.load()
    ws_bytes = int(lib.gcfr_shadow_workspace_bytes(B, c.H, c.W))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    box = R.ctypes_float4(prm.bonus_box) if prm.bonus_box is not None else None
    R.launch("gcfr_shadow_fwd", depth.device, depth, mask, 1, pt, B, L, c.H, c.W, prm.n_samples, R.sample_table(prm, depth.device),
             float(prm.inside_bonus), box, md, am, ws, ws_bytes, R.STREAM, _lib.opt_ref(options))
    return md, am, buf


def same_bits(a, b, nonfinite=False):
    """the same bits; a case with non-finite inputs: NaNs in the same places (whatever their payload), the same bits elsewhere"""
    import torch
    if a.shape != b.shape:
        return False
    a, b = a.contiguous(), b.contiguous()
    eq = a.view(torch.int32) == b.view(torch.int32)
    if nonfinite:
        eq = eq | (torch.isnan(a) & torch.isnan(b))
    return bool(eq.all())


def shapes_of(c):
    """(group, tile width) pairs: all twelve units; the 256 x 256 face: the default shape and the two extreme tile widths"""
    return [(4, 16), (4, 8), (2, 64)] if c.face else [(g, t) for g in GROUPS for t in TILE_WS]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_grid_march_equals_the_plain_kernel_and_the_c_oracle_bit_for_bit(name, monkeypatch):
    """normals handed in and from depth, k-split off"""
    from geomconsistentfr_amd import _lib
    c = CASES[name]
    ref, bufs, _ = reference(name)
    for group, tile_w in shapes_of(c):
        opt = _lib.options(tile_w=tile_w, group=group, ksplit=0)
        for given in (True, False):
            got, buf = fused_guarded(monkeypatch, name, given, opt)
            if same_bits(buf, bufs[given], c.nonfinite):
                continue
            what = (name, "group %d" % group, "tile_w %d" % tile_w, "given" if given else "from depth")
            for k in OUT_KEYS:   # say which: an output, or the guards
                if got.get(k) is not None:
                    assert same_bits(got[k], ref[k].reshape(got[k].shape), c.nonfinite), (what, k)
            raise AssertionError((what, "a guard band was written"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_argmin_grid_march_equals_the_plain_kernel_and_the_c_oracle_bit_for_bit(name):
    """minimum distance and argmin of the training march (the parent's weights: the control), k-split off"""
    from geomconsistentfr_amd import _lib
    c = CASES[name]
    ref, _, march_buf = reference(name)
    for group, tile_w in shapes_of(c):
        md, am, buf = march_guarded(name, _lib.options(tile_w=tile_w, group=group, ksplit=0))
        what = (name, "group %d" % group, "tile_w %d" % tile_w)
        # (the argmin exactly, NaN input or not: a NaN distance is never a minimum; the NaN tolerance is for the distances alone)
        assert same_bits(md, ref["minimum_distance"], c.nonfinite), (what, "minimum_distance")
        assert bool((am == ref["argmin"]).all()), (what, "argmin")
        md.copy_(ref["minimum_distance"])   # what is left to compare: the guard bands
        assert same_bits(buf, march_buf), (what, "a guard band was written")


def executed_work(name):
    """(in a process that loaded a counting build) the tallies of the forced grid kernel, 16 x 4 tiles and groups of four, on one case"""
    import torch
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import block as R
    c = CASES[name]
    depth, mask, light, ambient, albedo = scene(name)
    L = light.shape[1]
    n_tiles = L * ((c.W + 15) // 16) * ((c.H + 3) // 4)
    counters = torch.zeros(_lib.N_COUNTERS + 4 * n_tiles, dtype=torch.int64, device=DEV)
    R.render_fwd(depth, mask, light, ambient, None, albedo, params(c), want_argmin=False, camera=(F, F, c.W / 2.0, c.H / 2.0, Z_OFF),
                 options=_lib.options(tile_w=16, group=4, ksplit=0, counters=counters.data_ptr()))
    torch.cuda.synchronize()
    return dict(zip(_lib.COUNTER_NAMES, counters[:_lib.N_COUNTERS].cpu().tolist()), n_tiles=n_tiles)


@pytest.mark.gpu
def test_the_cases_are_not_vacuous():
    from geomconsistentfr_amd import build as hip_build
    small = [n for n, c in CASES.items() if min(c.H, c.W) < 6]
    assert len(small) >= 4 and any(c.bounds and not c.face for c in CASES.values())
    # Only the counting build can say that a tile marched under the bounds or not -- nothing else in the suite would notice a wrong guard
    # for H, W < 6 --, so its absence is a failure here, not a weaker check: `__graft_entry__.build()` makes it.
    assert os.path.exists(AUDIT_LIB) and hip_build.variant_is_current(AUDIT_LIB), "no current counting build (lib/audit.so): run __graft_entry__.build()"
    names = [n for n in sorted(CASES) if not CASES[n].face]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--executed-work"] + names, env=dict(os.environ, GCFR_HIP_LIB=AUDIT_LIB),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-1500:])
    work = json.loads(r.stdout.strip().splitlines()[-1])
    for name in names:
        c, w = CASES[name], work[name]
        assert w["n_tiles"] <= w["tiles"] <= 2 * w["n_tiles"], (name, w)
        if c.bounds:      # bodies ran under the bounds: the new weights were used
            assert w["bodies"] > 0 and w["bound_tests"] > 0, (name, w)
        if name in small:         # every tile marched by the rough sibling: no body under the bounds, no bound tested
            assert w["bodies"] == 0 and w["bound_tests"] == 0 and w["rough_samples"] > 0, (name, w)
        if c.depth == "noise":    # tiles gave the bounds up after the prologue
            assert w["bounds_given_up"] > 0 and w["rough_samples"] > 0, (name, w)
        for k in w:
            assert not (k.startswith("audit_") and k.endswith("violations")) or w[k] == 0, (name, k, w[k])


if __name__ == "__main__" and "--executed-work" in sys.argv:
    print(json.dumps({name: executed_work(name) for name in sys.argv[sys.argv.index("--executed-work") + 1:]}))
