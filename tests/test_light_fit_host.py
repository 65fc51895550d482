"""CPU: rig capture (csrc/gcfr_light_fit.hip; lighting.light_normal_equations / fit_light_rgb) -- the restatement
(tests/light_fit_emulation.py) held to an independent statement, the recovery of a known rig, and the refusal of every malformed
input before the library is loaded.

  restatement  gram, rhs and the solution (ridge = 0) against numpy's SVD least squares on the explicit weighted design matrix
               (columns sqrt(w) a_c f_l, target sqrt(w) I_c).  Both are exact up to rounding: the restatement is a sequential f64
               sum and a Cholesky solve, lstsq an SVD.  Gates: four times the largest difference measured here on the CPU over
               the shapes of tests/test_gpu_light_fit.py (light_fit_emulation.GATE_*), relative to the largest entry:
                   gram 1.43e-15 (at (1,4,256,256))   rhs 1.03e-14 (at (1,4,256,256))   solution 2.06e-14 (at (1,4,256,256);
                   1.81e-14 at (1,64,33,47), cond(G) = 480)
  recovery     the image synthesised as f32(a_c sum_l x_true f_l): the restatement's f32 solution returns x_true to 2.36e-7 of
               max|x_true| at L = 64, 33 x 47 (cond(G) = 495; lstsq: 2.22e-7, the restatement before its rounding: 2.22e-7) and to
               3.5e-8 at (2,5,21,37); gate four times the larger, light_fit_emulation.GATE_RECOVERY
  refusal      wrong rank, L = 0 and 65, a dtype other than f32, mixed devices, a wrong `out`, a bad layout or ridge, host tensors:
               GcfrError, with the library never loaded
  C level      the three symbols are declared, bound and exported; the workspace formula is the geometry Python mirrors; invalid
               arguments return GCFR_ERR_INVALID_ARGUMENT on the host, without a launch"""
import ctypes

import numpy as np
import pytest
import torch

import light_fit_emulation as emu
from test_abi import declared_symbols

SHAPES = emu.SHAPES


def _geometry(B, H, W):
    from geomconsistentfr_amd.lighting import light_fit_geometry
    return light_fit_geometry(B, H, W)


@pytest.fixture(scope="module")
def cases():
    """every shape once: inputs, the restatement and the independent statement (shared by the tests below, never modified)"""
    out = {}
    for i, (B, L, H, W, shared_w) in enumerate(SHAPES):
        final, albedo, image, w = emu.make_inputs(100 + i, B, L, H, W, "ones" if H * W == 1 else "mask", shared_weight=shared_w)
        chunk, groups = _geometry(B, H, W)
        gram, rhs = emu.normal_equations(final, albedo, image, w, True, chunk, groups)
        out[(B, L, H, W)] = (gram, rhs, emu.solve(gram, rhs, 0.0, False), emu.design_lstsq(final, albedo, image, w, True))
    return out


@pytest.mark.parametrize("B,L,H,W,shared_w", SHAPES)
def test_restatement_against_lstsq_on_the_design_matrix(cases, B, L, H, W, shared_w):
    gram, rhs, (rgb, info, x), (x_ref, gram_ref, rhs_ref, cond) = cases[(B, L, H, W)]
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    eg, er, ex = rel(gram, gram_ref), rel(rhs, rhs_ref), rel(x, x_ref)
    print("(%d,%d,%d,%d): cond(G) %.3g; gram %.3g (gate %.3g), rhs %.3g (gate %.3g), solution %.3g (gate %.3g)"
          % (B, L, H, W, cond.max(), eg, emu.GATE_GRAM, er, emu.GATE_RHS, ex, emu.GATE_SOLUTION))
    assert (info == 0).all()
    assert eg <= emu.GATE_GRAM and er <= emu.GATE_RHS and ex <= emu.GATE_SOLUTION
    for b in range(B):
        for c in range(3):
            assert np.array_equal(gram[b, c], gram[b, c].T)
    assert rgb.dtype == np.float32 and np.array_equal(rgb, x.astype(np.float32))


@pytest.mark.parametrize("B,L,H,W", [(1, 64, 33, 47), (2, 5, 21, 37)])
def test_recovery_of_a_known_rig(B, L, H, W):
    rng = np.random.default_rng(7)
    x_true = rng.uniform(-0.5, 1.5, (B, L, 3))
    final, albedo, image, w = emu.make_inputs(200 + L, B, L, H, W, "mask", x_true=x_true)
    chunk, groups = _geometry(B, H, W)
    gram, rhs = emu.normal_equations(final, albedo, image, w, True, chunk, groups)
    rgb, info, x = emu.solve(gram, rhs, 0.0, False)
    x_ref, _g, _r, cond = emu.design_lstsq(final, albedo, image, w, True)
    m = np.abs(x_true).max()
    err, err64, err_ref = [float(np.abs(v - x_true).max() / m) for v in (rgb, x, x_ref)]
    print("(%d,%d,%d,%d): cond(G) %.3g; |x - x_true| / max|x_true|: restatement f32 %.3g, before the rounding %.3g, lstsq %.3g; gate %.3g"
          % (B, L, H, W, cond.max(), err, err64, err_ref, emu.GATE_RECOVERY))
    assert (info == 0).all() and err <= emu.GATE_RECOVERY


def test_the_shared_rig_is_the_solve_of_the_summed_system_and_ridge_is_relative():
    B, L, H, W = 3, 4, 9, 11
    final, albedo, image, w = emu.make_inputs(31, B, L, H, W, "u8")
    chunk, groups = _geometry(B, H, W)
    gram, rhs = emu.normal_equations(final, albedo, image, w, True, chunk, groups)
    rgb, info, x = emu.solve(gram, rhs, 0.0, True)
    x_ref = emu.design_lstsq(final, albedo, image, w, True, shared=True)[0]
    assert rgb.shape == (1, L, 3) and (info == 0).all()
    assert np.abs(x - x_ref).max() / np.abs(x_ref).max() <= emu.GATE_SOLUTION
    # one face: shared and per face are the same operations
    one = emu.solve(gram[:1], rhs[:1], 1e-3, True)
    per = emu.solve(gram[:1], rhs[:1], 1e-3, False)
    assert np.array_equal(one[0], per[0])
    # the ridge is relative to the problem's scale: scaling the weights by 4 (exact in binary) leaves the solution unchanged
    g4, r4 = emu.normal_equations(final, albedo, image, (4.0 * w).astype(np.float32), True, chunk, groups)
    assert np.array_equal(emu.solve(g4, r4, 1e-3, False)[0], emu.solve(gram, rhs, 1e-3, False)[0])
    # ... and the ridged solution is that of A = G + ridge trace(G) / L I
    ridged = emu.solve(gram, rhs, 1e-3, False)[2]
    for b in range(B):
        for c in range(3):
            A = gram[b, c] + 1e-3 * np.trace(gram[b, c]) / L * np.eye(L)
            assert np.allclose(np.linalg.solve(A, rhs[b, c]), ridged[b, :, c], rtol=1e-10, atol=0)


def test_a_singular_system_reports_its_pivot():
    final, albedo, image, _ = emu.make_inputs(5, 1, 3, 4, 4, None)
    gram, rhs = emu.normal_equations(final, albedo, image, np.zeros((1, 4, 4), np.float32), True, 64, 1)
    rgb, info, _ = emu.solve(gram, rhs, 0.0, False)
    assert (info == 1).all() and np.isnan(rgb).all()
    final[:, 2] = final[:, 1]                                                     # two identical planes, ridge 1e-3: solvable
    gram, rhs = emu.normal_equations(final, albedo, image, None, True, 64, 1)
    rgb, info, _ = emu.solve(gram, rhs, 1e-3, False)
    assert (info == 0).all() and np.isfinite(rgb).all()


# ------------------------------------------------------------------------------------------------------------------------------
# early refusal: nothing below may load the library
# ------------------------------------------------------------------------------------------------------------------------------
def _good(B=2, L=3, H=4, W=5, device="meta"):
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
    return dict(final_shading=z(B, L, H, W), albedo=z(B, 3, H, W), image=z(B, H, W, 3))


MALFORMED = {
    "final_shading of rank 3": lambda a: a.update(final_shading=a["final_shading"][0]),
    "albedo of rank 3": lambda a: a.update(albedo=a["albedo"][0]),
    "image of rank 3": lambda a: a.update(image=a["image"][0]),
    "L = 0": lambda a: a.update(final_shading=a["final_shading"][:, :0]),
    "L = 65": lambda a: a.update(final_shading=torch.zeros(2, 65, 4, 5, device="meta")),
    "final_shading f64": lambda a: a.update(final_shading=a["final_shading"].double()),
    "albedo f16": lambda a: a.update(albedo=a["albedo"].half()),
    "image u8": lambda a: a.update(image=a["image"].to(torch.uint8)),
    "weight f64": lambda a: a.update(weight=torch.zeros(2, 4, 5, dtype=torch.float64, device="meta")),
    "weight of another shape": lambda a: a.update(weight=torch.zeros(3, 4, 5, device="meta")),
    "albedo with a light axis": lambda a: a.update(albedo=torch.zeros(2, 3, 3, 4, 5, device="meta")),
    "image in the other layout": lambda a: a.update(image=a["image"].permute(0, 3, 1, 2)),
    "an unknown layout": lambda a: a.update(image_layout="hwc"),
    "mixed devices": lambda a: a.update(albedo=torch.zeros(2, 3, 4, 5)),
    "a mixed-device weight": lambda a: a.update(weight=torch.zeros(2, 4, 5)),
    "out of a wrong shape": lambda a: a.update(out=torch.zeros(2, 3, 4, device="meta")),
    "out per face for a shared rig": lambda a: a.update(out=torch.zeros(2, 3, 3, device="meta"), shared=True),
    "out not contiguous": lambda a: a.update(out=torch.zeros(2, 3, 6, device="meta")[:, :, ::2]),
    "out f64": lambda a: a.update(out=torch.zeros(2, 3, 3, dtype=torch.float64, device="meta")),
    "a negative ridge": lambda a: a.update(ridge=-1.0),
    "a NaN ridge": lambda a: a.update(ridge=float("nan")),
    "not a tensor": lambda a: a.update(albedo=np.zeros((2, 3, 4, 5), np.float32)),
    "host tensors": lambda a: a.update(**_good(device="cpu")),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_inputs_raise_before_the_library_is_loaded(what, monkeypatch):
    from geomconsistentfr_amd import _lib, fit_light_rgb, light_normal_equations

    def no_load():
        raise AssertionError("the library was loaded for a malformed input (%s)" % what)

    monkeypatch.setattr(_lib, "load", no_load)
    args = _good()
    MALFORMED[what](args)
    with pytest.raises(_lib.GcfrError):
        fit_light_rgb(**args)
    if not {"out", "shared", "ridge"} & set(args):
        with pytest.raises(_lib.GcfrError):
            light_normal_equations(**args)


def test_capture_rig_refuses_too_many_lights_before_the_network_pass():
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import inference as inf

    class Never:
        def forward_lights(self, *a, **k):
            raise AssertionError("the network ran")

    with pytest.raises(_lib.GcfrError):
        inf.capture_rig(Never(), np.zeros((1, 8, 8, 3), np.float32), np.zeros((8, 8), np.uint8), np.zeros((65, 3), np.float32), device="cpu")


# ------------------------------------------------------------------------------------------------------------------------------
# the C level, on the host
# ------------------------------------------------------------------------------------------------------------------------------
NAMES = ("gcfr_light_fit_workspace_bytes", "gcfr_light_fit_normal", "gcfr_light_fit_solve")


def test_the_three_symbols_are_declared_bound_and_exported():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    for s in NAMES:
        assert s in declared_symbols(), s
        assert s in _lib.exported_symbols(), s
        assert hasattr(L, s), s
    assert L.gcfr_abi_version() == 6


def test_the_workspace_is_the_mirrored_geometry():
    from geomconsistentfr_amd import _lib
    lib = _lib.load()
    for B, L, H, W in [s[:4] for s in SHAPES] + [(8, 11, 256, 256), (8, 64, 256, 256), (600, 2, 3, 3), (1, 64, 1, 1)]:
        chunk, groups = _geometry(B, H, W)
        assert chunk == 64 and 1 <= groups <= (H * W + chunk - 1) // chunk
        assert lib.gcfr_light_fit_workspace_bytes(B, L, H, W) == 8 * B * groups * 3 * (L * (L + 3) // 2), (B, L, H, W)
    assert _geometry(1, 256, 256) == (64, 512) and _geometry(8, 256, 256) == (64, 64)       # the cap binds; chunks are walked in turns
    for bad in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 65, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (65536, 1, 1, 1), (1, 1, 65536, 32768)]:
        assert lib.gcfr_light_fit_workspace_bytes(*bad) == 0, bad


def test_invalid_arguments_are_refused_on_the_host():
    from geomconsistentfr_amd import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)
    normal = lambda **k: lib.gcfr_light_fit_normal(*[k.get(n, d) for n, d in (
        ("final", p), ("albedo", p), ("image", p), ("nhwc", 1), ("weight", None), ("wb", 1), ("B", 2), ("L", 3), ("H", 4), ("W", 5),
        ("ws", p), ("gram", p), ("rhs", p), ("stream", None))])
    for k in ("final", "albedo", "image", "ws", "gram", "rhs"):
        assert normal(**{k: None}) == -1, k
    for k, v in (("L", 0), ("L", 65), ("B", 0), ("B", 65536), ("H", 0), ("W", 0), ("nhwc", 2), ("ws", odd), ("gram", odd), ("rhs", odd)):
        assert normal(**{k: v}) == -1, (k, v)
    assert normal(weight=p, wb=3) == -1 and normal(weight=p, wb=0) == -1
    solve = lambda **k: lib.gcfr_light_fit_solve(*[k.get(n, d) for n, d in (
        ("gram", p), ("rhs", p), ("B", 2), ("L", 3), ("ridge", 1e-3), ("rigs", 2), ("rgb", p), ("info", p), ("stream", None))])
    for k in ("gram", "rhs", "rgb", "info"):
        assert solve(**{k: None}) == -1, k
    for k, v in (("L", 0), ("L", 65), ("B", 0), ("rigs", 3), ("rigs", 0), ("ridge", -1e-3), ("ridge", float("nan")), ("ridge", float("inf")),
                 ("gram", odd), ("rhs", odd)):
        assert solve(**{k: v}) == -1, (k, v)
