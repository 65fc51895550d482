"""The LDS annex of the six-wave fused inference grid march (csrc/gcfr_march.hpp: PARK) -- the sample positions a
group's prefetch computes are parked in LDS, one slot per sample, one plane per wave of the workgroup, and read back by the main
loop's bodies -- against the plain kernel (no workspace, three-stage path) and the C oracle: every fused output byte for byte.

Under test: the grid kernels with the k-split forced off (`options(tile_w=..., group=..., ksplit=0)`), from depth and with normals
handed in, tile widths 8, 16, 32 and 64, groups of 4 and 2 and -- the untouched control -- 1.  What parking can break, and the
smallest inputs that show it:
  * 64 x 8 pixels at tile width 16: four tiles side by side, so the four waves of ONE workgroup hold different rays (a plane
    shared between waves, mutant 31, shows here and nowhere narrower);
  * partial tiles (24 x 6, 18 x 6, 40 x 12): inactive and clamped lanes park and read like any other;
  * sample tables of 1, 2, 3, 5, 8 and 24 entries: a single group, and a last group shorter than the group, whose clamped
    samples are read back from slots that the late prefetch of the group in front wrote with clamped table values;
  * masks: zeros with holes, a band one row wide and a single cell (groups alternate "body" / "no body": a no-body group's
    prefetch overwrites the slots directly, in front of a body group's reads), random, all ones (the instantiation that parks
    the group's first and last position only);
  * smooth depth (tiles reach the trailing loop, whose leave path keeps its own positions, and come back out of it) and depth
    rougher than the rays rise (tiles hand themselves to the rough sibling after the prologue);
  * even and odd W/2 and H/2 (only the even half-parity parks: the odd one is the parent's kernel);
  * B L >= 3 with a mask per face and with one shared mask;
  * a NaN light (every ray of that light is non-finite) and a NaN depth cell: NaNs in the same places as the plain kernel's (the
    C oracle is host code for finite inputs and is not asked about this one case).
Every output lives inside one buffer with guard bands of a NaN pattern round it: one comparison of the whole buffer says that
the guards are untouched, every element was written and every bit is the reference's.

`test_the_cases_are_not_vacuous` asks the counting build (lib/audit.so, which `__graft_entry__.build()` makes: 16 x 4 tiles,
groups of four) what each case executed: the forced grid kernel ran, bodies were executed, the trailing loop was entered and
left where the case is meant to reach it, tiles gave the bounds up where it is meant to be rough.  Without that build the
conditions on the inputs stand in: lit and masked minima both occur (a lit minimum is a body that ran).

Mutants (csrc/gcfr_mutants.hpp, `tools/build_variant.sh mut_<n> -DGCFR_MUT=<n>`, this file with GCFR_HIP_LIB=<that library>):
30 (slot j ^ 1 read back) and 31 (one plane for all four waves); how many cases each fails: profiles/lds_park_ab.txt.
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

DEV = "cuda:0"
F, Z_OFF = 1570.0, 1610.0
T0 = 0.025
GUARD = 64
GROUPS = (4, 2, 1)
TILE_WS = (8, 16, 32, 64)
OUT_KEYS = ("unit_light_direction", "light_pt", "minimum_distance", "shadow_mask_weights", "full_shading", "final_shading",
            "rendered_images", "surface_normals")
AUDIT_LIB = os.path.join(ROOT, "geomconsistentfr_amd", "lib", "audit.so")

# trail / rough: what the case is MEANT to reach (asserted with the counting build's numbers)
Case = collections.namedtuple("Case", "H W B L n mask depth shared nonfinite trail rough")


def case(H, W, B, L, n, mask, depth="smooth", shared=False, nonfinite=False, trail=False, rough=False):
    return Case(H, W, B, L, n, mask, depth, shared, nonfinite, trail, rough)


CASES = {
    # four tiles side by side at tile width 16 (even W/2 and H/2: the kernels that park), every table length
    "table_1": case(8, 64, 1, 3, 1, "holes"),
    "table_2": case(8, 64, 1, 3, 2, "holes"),
    "table_3": case(8, 64, 1, 3, 3, "holes"),
    "table_5": case(8, 64, 1, 3, 5, "holes"),
    "table_8": case(8, 64, 1, 3, 8, "holes"),
    "table_24": case(8, 64, 1, 3, 24, "holes"),
    # the masks
    "band": case(8, 64, 1, 3, 24, "band"),
    "single": case(8, 64, 2, 2, 24, "single"),
    "random": case(8, 64, 2, 2, 24, "random"),
    "ones": case(8, 64, 1, 3, 24, "ones"),
    "ones_table_5": case(8, 64, 1, 3, 5, "ones"),
    # one mask for all faces
    "shared_mask": case(8, 64, 3, 1, 24, "holes", shared=True),
    # smooth depth on an image tall enough for rays that run on above the surface: the trailing loop and its leave path
    "trailing": case(64, 64, 2, 2, 40, "random", trail=True),
    "trailing_ones": case(64, 64, 1, 3, 40, "ones", trail=True),
    # rougher than the rays rise: the rough sibling after the prologue
    "rough": case(8, 64, 2, 2, 24, "random", depth="noise", rough=True),
    "rough_ones": case(8, 64, 1, 3, 24, "ones", depth="noise", rough=True),
    # partial tiles; 24 x 6 and 18 x 6 have an odd H/2 or W/2 (the parent's kernel), 40 x 12 is even in both.  (The library takes even
    # H and W only -- an odd one is GCFR_ERR_INVALID_ARGUMENT --, so 18 x 6 stands where 17 x 5 was asked for: the nearest accepted size.)
    "partial_24x6": case(6, 24, 2, 2, 8, "holes"),
    "partial_18x6": case(6, 18, 1, 3, 5, "random"),
    "partial_40x12": case(12, 40, 1, 3, 24, "holes"),
    # odd W/2, four tiles wide
    "odd_half": case(8, 66, 1, 3, 24, "holes"),
    # a NaN light and a NaN depth cell
    "nonfinite": case(8, 64, 1, 3, 24, "random", nonfinite=True),
}


def params(c):
    from geomconsistentfr_amd import RenderParams
    # a light 30 px away: some lights project inside the image, some outside; the table ends at t = 0.925 whatever its length
    return RenderParams(n_samples=c.n, t0=T0, dt=0.9 / c.n, light_distance=30.0, inside_bonus=5.0,
                        bonus_box=(-(c.W / 2.0), c.W - c.W / 2.0 - 1, 1 - c.H / 2.0, c.H / 2.0))


@functools.lru_cache(maxsize=None)
def scene_np(name):
    """depth (B,H,W), mask (B | 1,H,W), light (B,L,3), ambient (B,L), albedo (B,3,H,W): every face its own depth, albedo, lights"""
    c = CASES[name]
    H, W, B, L = c.H, c.W, c.B, c.L
    rng = np.random.default_rng(sorted(CASES).index(name))
    r, col = np.mgrid[0:H, 0:W]
    # (a bump as high as 0.3 of the SHORTER side: on 64 x 8 pixels one scaled by the longer side is steeper than the rays rise, and
    #  every tile gives the bounds up -- the counting build said so)
    depth = np.stack([0.3 * min(H, W) * np.exp(-(((col - (0.45 + 0.05 * b) * W) / (0.3 * W)) ** 2 + ((r - 0.5 * H) / (0.3 * H)) ** 2))
                      for b in range(B)])
    if c.depth == "noise":   # rougher than the rays rise: tiles give the bounds up
        depth = depth + 40.0 * rng.random((B, H, W))
    depth = depth.astype(np.float32)
    Bm = 1 if c.shared else B
    if c.mask == "ones":
        mask = np.ones((Bm, H, W), np.uint8)
    elif c.mask == "single":
        mask = np.zeros((Bm, H, W), np.uint8)
        mask[:, H // 2, W // 2] = 1
    elif c.mask == "band":
        mask = np.zeros((Bm, H, W), np.uint8)
        mask[:, H // 2, :] = 1
    elif c.mask == "holes":   # zeros with holes: most groups have no body, the ones across a hole do
        mask = np.zeros((Bm, H, W), np.uint8)
        mask[:, 1::3, 2::5] = 1
        mask[:, H // 2, W // 2] = 1
    else:
        mask = (rng.random((Bm, H, W)) > 0.3).astype(np.uint8)
        mask[:, H // 2, W // 2] = 1      # (never empty)
        mask[:, 0, 0] = 0                # (never all ones)
    light = rng.standard_normal((B, L, 3)).astype(np.float32)
    light[..., 2] = np.abs(light[..., 2]) + 0.2
    if c.nonfinite:
        light[0, 1, 0] = np.nan
        depth[0, H // 2, W // 3] = np.nan
    ambient = (0.1 + rng.random((B, L))).astype(np.float32)
    albedo = (0.05 + rng.random((B, 3, H, W)) + np.arange(B)[:, None, None, None]).astype(np.float32)
    return depth, mask, light, ambient, albedo


@functools.lru_cache(maxsize=None)
def scene(name):
    import torch
    return tuple(torch.from_numpy(a).to(DEV) for a in scene_np(name))


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


@functools.lru_cache(maxsize=None)
def reference(name):
    """The plain kernel (no workspace), then the stand-alone normals and shading kernels; its minimum distance is compared with
    the C oracle's here, once (finite inputs only).  Returns the outputs by name and the two guarded buffers (normals handed
    in / from depth) a fused launch must reproduce."""
    import c_oracle
    import torch
    from geomconsistentfr_amd import light_prep, shadow_min_distance
    from geomconsistentfr_amd.block import shade
    from geomconsistentfr_amd.normals import depth_to_normals
    c = CASES[name]
    depth, mask, light, ambient, albedo = scene(name)
    prm = params(c)
    unit, pt = light_prep(light, prm)
    md, _ = shadow_min_distance(depth, mask, pt, prm, want_argmin=False, use_workspace=False)
    if not c.nonfinite:   # (the C oracle is host code for finite inputs: it turns positions into indices unchecked)
        mask_all = np.ascontiguousarray(np.broadcast_to(mask.cpu().numpy(), (c.B, c.H, c.W)))
        md_o, _ = c_oracle.shadow_min_distance(depth.cpu().numpy(), mask_all, pt.cpu().numpy(), c_oracle.sample_table(T0, 0.9 / c.n, c.n),
                                               bonus=prm.inside_bonus, bonus_box=prm.bonus_box)
        np.testing.assert_array_equal(md.cpu().numpy(), md_o, err_msg="the plain kernel against the C oracle")
    else:                 # the plain kernel alone is the reference, as in tests/test_gpu_parity.py's adversarial inputs
        assert np.isnan(md.cpu().numpy()[0, 1]).all() and np.isfinite(md.cpu().numpy()[0, 0]).sum() > 0
    nrm = depth_to_normals(depth[:, None], camera_matrix(c.H, c.W), z_offset=Z_OFF)
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_parked_grid_march_equals_the_plain_kernel_and_the_c_oracle_bit_for_bit(name, monkeypatch):
    """tile widths 8 ... 64, groups of 4 / 2 / 1, normals handed in and from depth, k-split off"""
    from geomconsistentfr_amd import _lib
    c = CASES[name]
    ref, bufs = reference(name)
    for group in GROUPS:
        for tile_w in TILE_WS:
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


def executed_work(name):
    """(in a process that loaded a counting build) the tallies of the forced grid kernel, 16 x 4 tiles and groups of four, on one case"""
    import torch
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import block as R
    c = CASES[name]
    depth, mask, light, ambient, albedo = scene(name)
    n_tiles = c.B * c.L * ((c.W + 15) // 16) * ((c.H + 3) // 4)
    counters = torch.zeros(_lib.N_COUNTERS + 4 * n_tiles, dtype=torch.int64, device=DEV)
    R.render_fwd(depth, mask, light, ambient, None, albedo, params(c), want_argmin=False, camera=(F, F, c.W / 2.0, c.H / 2.0, Z_OFF),
                 options=_lib.options(tile_w=16, group=4, ksplit=0, counters=counters.data_ptr()))
    torch.cuda.synchronize()
    return dict(zip(_lib.COUNTER_NAMES, counters[:_lib.N_COUNTERS].cpu().tolist()), n_tiles=n_tiles)


@pytest.mark.gpu
def test_the_cases_are_not_vacuous():
    from geomconsistentfr_amd import build as hip_build
    if os.path.exists(AUDIT_LIB) and hip_build.variant_is_current(AUDIT_LIB):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--executed-work"], env=dict(os.environ, GCFR_HIP_LIB=AUDIT_LIB),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-400:], r.stderr[-1500:])
        work = json.loads(r.stdout.strip().splitlines()[-1])
        for name, c in CASES.items():
            w = work[name]
            # the forced grid kernel ran: it counts every tile, once (a tile that hands itself to the rough sibling is counted by both)
            assert w["n_tiles"] <= w["tiles"] <= 2 * w["n_tiles"], (name, w)
            if c.rough:
                assert w["bounds_given_up"] > 0 and w["rough_samples"] > 0, (name, w)
            elif c.n == 1:   # (a table of one sample is not an increasing one: every tile marches it in the rough sibling, by construction)
                assert w["bounds_given_up"] == w["n_tiles"] and w["rough_samples"] > 0, (name, w)
            else:
                assert w["bodies"] > 0 and w["bound_tests"] > 0, (name, w)
            if c.trail:
                assert w["trail_enter"] > 0 and w["trail_skips"] > 0 and w["trail_leave"] > 0, (name, w)
            for k in w:
                assert not (k.startswith("audit_") and k.endswith("violations")) or w[k] == 0, (name, k, w[k])
        return
    # no counting build: the conditions on the inputs
    for name, c in CASES.items():
        md = reference(name)[0]["minimum_distance"].cpu().numpy()
        lit = md < 1e5
        assert lit.any(), name                                    # some minimum was taken from a sample: a body ran
        assert c.mask == "ones" or (~lit).any(), name             # ... and some pixel saw only masked samples


if __name__ == "__main__" and "--executed-work" in sys.argv:
    print(json.dumps({name: executed_work(name) for name in sorted(CASES)}))
