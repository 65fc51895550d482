"""What GCFR_VISIT_TRIM changes in the bounds variant of the fused six-wave inference grid march (csrc/gcfr_march.hpp: TRIM, MINFORM;
DESIGN.md 4.1i) -- the ray's f32 direction and the product n * zb of the bounds and termination tests produced inside a volatile asm
from read-only operands (no copies in front of them), and in the main loop's bodies the running minimum as one v_min_f32 to which
masked lanes hand +inf, behind a wave-uniform skip of samples without an unmasked lane -- against the plain kernel (no workspace,
three-stage path) and the C oracle: the fused entries, from depth and with normals handed in, every output byte for byte.

Under test: the grid kernels with the k-split forced off (`options(tile_w=..., group=..., ksplit=0)`), tile widths 8 ... 64, groups of
4, 2 and 1.  Sizes are written W x H; the smallest at which these pieces can go wrong:
  * 6 x 6 (odd W/2 and H/2) and 8 x 8 (even): the smallest images the bounds variant marches; 18 x 6: partial tiles;
  * 64 x 16: four tiles side by side, so the four waves of a workgroup hold different rays and different running minima;
  * one 256 x 256 face of tools/scenes.py with the training script's constants (the default shape and the two extreme tile widths);
  * sample tables of 1, 3, 4, 5, 8 and 24 entries: one group, a clamped last sample (its S is handed to the minimum a second time),
    groups that straddle the table's end;
  * masks: zeros with holes, one cell, a band one row wide (most lanes of an evaluated sample are masked: they hand +inf), all ones,
    all zeros (every lane masked in every sample: the minimum distance is the masked value everywhere, asserted);
  * smooth depth and depth rougher than the rays rise (tiles hand themselves to the rough sibling, whose minimum is the parent's);
  * the first light straight over the interior pixel (H/2, W/2), the second grazing, the others random;
  * a NaN light and a NaN depth cell: S = NaN reaches v_min_f32, which keeps the running minimum as the parent's compare does
    (compared with the plain kernel only: the C oracle is host code for finite inputs);
  * a mask per face and one shared mask;
  * the prepass alone (`phase` = 1) and then the march alone (`phase` = 2) on the same workspace.
Every output lives inside one buffer with guard bands of a NaN pattern round it: one comparison of the whole buffer says that
the guards are untouched, every element was written and every bit is the reference's.

`test_the_cases_are_not_vacuous`: the counting build (lib/audit.so, made by `__graft_entry__.build()`; 16 x 4 tiles, groups of four)
says what each case executed -- bound tests and bodies where a case claims them, none where it claims none; without a current
counting build it fails.

Mutant 33 (csrc/gcfr_mutants.hpp, `tools/build_variant.sh mut_33 -DGCFR_MUT=33`): a masked lane hands its S to the minimum instead of
+inf.  `GCFR_HIP_LIB=<that library> python tests/test_gpu_march_visit_trim.py --mutant-report` runs every case on it and prints, per
family, how many cases fail; the numbers of record: profiles/visit_trim_ab.txt.
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
MASKED_DISTANCE = 1.0e6

# family: what the case is there for (the mutant report counts by it); bodies: bound tests and bodies are CLAIMED (counting build)
Case = collections.namedtuple("Case", "family H W B L n mask depth shared nonfinite bodies face")


def case(family, W, H, B=1, L=4, n=24, mask="holes", depth="smooth", shared=False, nonfinite=False, face=False):
    bodies = depth == "smooth" and n >= 2 and min(H, W) >= 6 and mask != "zeros"
    return Case(family, H, W, B, L, n, mask, depth, shared, nonfinite, bodies, face)


CASES = {
    "6x6": case("size", 6, 6),
    "8x8": case("size", 8, 8),
    "18x6": case("size", 18, 6),
    "64x16": case("size", 64, 16, n=40),
    "face_256": case("size", 256, 256, L=1, n=160, face=True),
    "table_1": case("table", 64, 16, n=1),
    "table_3": case("table", 64, 16, n=3),
    "table_4": case("table", 64, 16, n=4),
    "table_5": case("table", 64, 16, n=5),
    "table_8": case("table", 64, 16, n=8),
    "table_24_8x8": case("table", 8, 8, n=24, mask="random"),
    "single": case("mask", 64, 16, B=2, L=2, mask="single"),
    "band": case("mask", 64, 16, mask="band"),
    "random": case("mask", 64, 16, B=2, L=2, mask="random"),
    "ones": case("mask", 64, 16, mask="ones"),
    "ones_table_5": case("mask", 64, 16, n=5, mask="ones"),
    "zeros": case("mask", 64, 16, mask="zeros"),
    "shared_mask": case("mask", 64, 16, B=3, L=2, mask="random", shared=True),
    "rough": case("depth", 64, 16, B=2, L=2, mask="random", depth="noise"),
    "rough_ones": case("depth", 64, 16, mask="ones", depth="noise"),
    "nonfinite": case("nonfinite", 64, 16, mask="random", nonfinite=True),
    "nonfinite_6x6": case("nonfinite", 6, 6, mask="random", nonfinite=True),
}
PHASE_CASES = ("6x6", "64x16", "table_5", "shared_mask")


def params(c):
    from geomconsistentfr_amd import RenderParams
    if c.face:
        return RenderParams()
    # a light 30 px away: some lights project inside the image, some outside; the table ends at t = 0.925 whatever its length
    return RenderParams(n_samples=c.n, t0=T0, dt=0.9 / c.n, light_distance=30.0, inside_bonus=5.0,
                        bonus_box=(-(c.W / 2.0), c.W - c.W / 2.0 - 1, 1 - c.H / 2.0, c.H / 2.0))


@functools.lru_cache(maxsize=None)
def scene_np(name):
    """depth (B,H,W), mask (B | 1,H,W), light (B,L,3), ambient (B,L), albedo (B,3,H,W): every face its own depth, albedo, lights"""
    c = CASES[name]
    if c.face:
        import scenes
        depth, mask, albedo, _, light, amb = scenes.synth_faces(1, 3)
        return depth, mask, light.reshape(1, 1, 3), amb.reshape(1, 1), albedo
    H, W, B, L = c.H, c.W, c.B, c.L
    rng = np.random.default_rng(sorted(CASES).index(name))
    r, col = np.mgrid[0:H, 0:W]
    depth = np.stack([0.3 * min(H, W) * np.exp(-(((col - (0.45 + 0.05 * b) * W) / (0.3 * W)) ** 2 + ((r - 0.5 * H) / (0.3 * H)) ** 2))
                      for b in range(B)])
    if c.depth == "noise":   # rougher than the rays rise: tiles give the bounds up
        depth = depth + 40.0 * rng.random((B, H, W))
    depth = depth.astype(np.float32)
    Bm = 1 if c.shared else B
    if c.mask == "ones":
        mask = np.ones((Bm, H, W), np.uint8)
    elif c.mask == "zeros":
        mask = np.zeros((Bm, H, W), np.uint8)
    elif c.mask == "single":
        mask = np.zeros((Bm, H, W), np.uint8)
        mask[:, H // 2, W // 2] = 1
    elif c.mask == "band":
        mask = np.zeros((Bm, H, W), np.uint8)
        mask[:, H // 2, :] = 1
    elif c.mask == "holes":   # zeros with holes: most lanes of an evaluated sample are masked
        mask = np.zeros((Bm, H, W), np.uint8)
        mask[:, 1::3, 2::5] = 1
        mask[:, H // 2, W // 2] = 1
    else:
        mask = (rng.random((Bm, H, W)) > 0.3).astype(np.uint8)
        mask[:, H // 2, W // 2] = 1      # (never empty)
        mask[:, 0, 0] = 0                # (never all ones)
    light = rng.standard_normal((B, L, 3)).astype(np.float32)
    light[..., 2] = np.abs(light[..., 2]) + 0.2
    light[:, 0] = (0.0, 0.0, 1.0)                    # straight over x = y = 0, the interior pixel (H/2, W/2)
    if L >= 2:
        light[:, 1] = (0.9, 0.3, 0.05)               # grazing
    if c.nonfinite:
        light[0, L - 1, 0] = np.nan
        depth[0, H // 2, W // 3] = np.nan
    ambient = (0.1 + rng.random((B, L))).astype(np.float32)
    albedo = (0.05 + rng.random((B, 3, H, W)) + np.arange(B)[:, None, None, None]).astype(np.float32)
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
    md_np = md.cpu().numpy()
    if not c.nonfinite:   # (the C oracle is host code for finite inputs: it turns positions into indices unchecked)
        mask_all = np.ascontiguousarray(np.broadcast_to(mask.cpu().numpy(), (c.B, c.H, c.W)))
        md_o, _ = c_oracle.shadow_min_distance(depth.cpu().numpy(), mask_all, pt.cpu().numpy(),
                                               c_oracle.sample_table(prm.t0, prm.dt, prm.n_samples), bonus=prm.inside_bonus, bonus_box=prm.bonus_box)
        np.testing.assert_array_equal(md_np, md_o, err_msg="the plain kernel against the C oracle")
    else:                 # the plain kernel alone is the reference, as in tests/test_gpu_parity.py's adversarial inputs
        assert np.isnan(md_np[0, c.L - 1]).all() and np.isfinite(md_np[0, 0]).sum() > 0
    if c.mask == "zeros":  # every lane masked in every sample: the masked value (plus the bonus where the light is inside the box)
        assert np.isin(md_np, (np.float32(MASKED_DISTANCE), np.float32(MASKED_DISTANCE) + np.float32(prm.inside_bonus))).all()
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


def fused_guarded(monkeypatch, name, given, options, two_phases=False):
    """one fused launch -- or the prepass alone, then the march alone on its workspace -- with every output carved out of one
    NaN-filled buffer, guard bands between them: (outputs, buffer)"""
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
        if prepared is not None:
            torch.cuda.synchronize()   # (the prepass wrote the light's two outputs on its side stream)
        for k, off, cnt in rows:
            if prepared is not None and k in ("unit_light_direction", "light_pt"):
                buf[off:off + cnt] = out[k].reshape(-1)   # written by the prepass call: carried into the buffer as they are
            out[k] = buf[off:off + cnt].view(out[k].shape)
        made.append(buf)
        return out, ws, ws_bytes

    monkeypatch.setattr(R, "_alloc_forward", alloc)
    try:
        normals = reference(name)[0]["surface_normals"] if given else None
        pre = R.render_prepass(depth, mask, light, params(c), want_argmin=False, options=options) if two_phases else None
        got = R.render_fwd(depth, mask, light, ambient, normals, albedo, params(c), want_argmin=False,
                           camera=None if given else (F, F, c.W / 2.0, c.H / 2.0, Z_OFF), options=options, prepared=pre)
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


def shapes_of(c):
    """(group, tile width) pairs: all twelve units; the 256 x 256 face: the default shape and the two extreme tile widths"""
    return [(4, 16), (4, 8), (2, 64)] if c.face else [(g, t) for g in GROUPS for t in TILE_WS]


def check_case(monkeypatch, name, two_phases=False):
    from geomconsistentfr_amd import _lib
    c = CASES[name]
    ref, bufs = reference(name)
    for group, tile_w in shapes_of(c):
        opt = _lib.options(tile_w=tile_w, group=group, ksplit=0)
        for given in (True, False):
            got, buf = fused_guarded(monkeypatch, name, given, opt, two_phases)
            if same_bits(buf, bufs[given], c.nonfinite):
                continue
            what = (name, "group %d" % group, "tile_w %d" % tile_w, "given" if given else "from depth", "two phases" if two_phases else "one call")
            for k in OUT_KEYS:   # say which: an output, or the guards
                if got.get(k) is not None:
                    assert same_bits(got[k], ref[k].reshape(got[k].shape), c.nonfinite), (what, k)
            raise AssertionError((what, "a guard band was written"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_grid_march_equals_the_plain_kernel_and_the_c_oracle_bit_for_bit(name, monkeypatch):
    """tile widths 8 ... 64, groups of 4 / 2 / 1, normals handed in and from depth, k-split off"""
    check_case(monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PHASE_CASES)
def test_prepass_alone_then_march_alone_gives_the_same_bits(name, monkeypatch):
    """`phase` = 1, then `phase` = 2 on the workspace the first call filled"""
    check_case(monkeypatch, name, two_phases=True)


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
    # Only the counting build can say that a case tested a bound or executed a body, so its absence is a failure here, not a weaker
    # check: `__graft_entry__.build()` makes it.
    assert os.path.exists(AUDIT_LIB) and hip_build.variant_is_current(AUDIT_LIB), "no current counting build (lib/audit.so): run __graft_entry__.build()"
    names = sorted(CASES)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--executed-work"] + names, env=dict(os.environ, GCFR_HIP_LIB=AUDIT_LIB),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-1500:])
    work = json.loads(r.stdout.strip().splitlines()[-1])
    for name in names:
        c, w = CASES[name], work[name]
        print(name, {k: w[k] for k in ("n_tiles", "tiles", "bound_tests", "bodies", "wave_samples", "bounds_given_up", "rough_samples", "trail_enter", "trail_leave")})
        assert w["n_tiles"] <= w["tiles"] <= 2 * w["n_tiles"], (name, w)
        if c.bodies:
            assert w["bound_tests"] > 0 and w["bodies"] > 0 and w["wave_samples"] > 0, (name, w)
        elif c.mask == "zeros":   # no candidate sample anywhere: nothing is tested, nothing evaluated
            assert w["bound_tests"] == 0 and w["bodies"] == 0 and w["rough_samples"] == 0, (name, w)
        elif c.n == 1:            # (a table of one sample is not an increasing one: every tile marches it in the rough sibling, by construction)
            assert w["bounds_given_up"] == w["n_tiles"] and w["rough_samples"] > 0 and w["bound_tests"] == 0, (name, w)
        elif c.depth == "noise":  # tiles gave the bounds up after the prologue
            assert w["bounds_given_up"] > 0 and w["rough_samples"] > 0, (name, w)
        for k in w:
            assert not (k.startswith("audit_") and k.endswith("violations")) or w[k] == 0, (name, k, w[k])
    # the trailing loop's bounds test and horizon look-up (the re-derived direction and n * zb): entered on some of the small cases (the
    # counting build: 16 tiles), walked, terminated in and left again on the face
    assert sum(work[n]["trail_enter"] for n in names if not CASES[n].face) > 0
    w = work["face_256"]
    assert w["trail_enter"] > 0 and w["trail_skips"] > 0 and w["trail_leave"] > 0 and w["early_exits"] > 0, w


class _Patch:
    """what the report needs of pytest's monkeypatch"""
    @staticmethod
    def setattr(obj, name, value):
        setattr(obj, name, value)


def mutant_report():
    """every case on the library this process loaded (GCFR_HIP_LIB): which fail the comparison, by family"""
    from geomconsistentfr_amd import _lib
    failed = collections.defaultdict(list)
    for name in sorted(CASES):
        try:
            check_case(_Patch, name)
            bad = False
        except AssertionError:
            bad = True
        failed[CASES[name].family].append((name, bad))
    for fam, rows in sorted(failed.items()):
        print("%-10s %d of %d fail: %s" % (fam, sum(f for _, f in rows), len(rows), ", ".join(n for n, f in rows if f) or "-"))
    print("total      %d of %d cases fail on %s" % (sum(f for rows in failed.values() for _, f in rows), len(CASES),
                                                    os.environ.get("GCFR_HIP_LIB") or _lib.lib_path()))


if __name__ == "__main__" and "--executed-work" in sys.argv:
    print(json.dumps({name: executed_work(name) for name in sys.argv[sys.argv.index("--executed-work") + 1:]}))
elif __name__ == "__main__" and "--mutant-report" in sys.argv:
    mutant_report()
