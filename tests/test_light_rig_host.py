"""CPU: the light-rig stage's host side (geomconsistentfr_amd/lighting.py) and its numpy restatement.

1. tests/light_rig_emulation.py (the kernels' operation order in numpy f32) against f64 torch autograd of the plain expression
   `(final[:,:,None] * rgb[...,None,None]).sum(1) * albedo`.  Gate: every output element within L * 2^-23 of the sum of the
   absolute values of the terms it is made of.  Where that follows from the roundings: shading_rgb is L rounded products and L-1
   rounded sums, rendered one product more, g_albedo likewise: at most (L + 1) roundings of 2^-24 relative each, which L * 2^-23
   covers for every L >= 1.  g_final is 5 roundings whatever L (u's product and sum, the channel product, two sums) and g_rgb 3
   (u's two and the final f32 rounding; the f64 sum itself contributes nothing at this scale), so for these two the gate is
   asserted on the cases with L >= 3, where L * 2^-23 >= 5 * 2^-24; the L = 1, 2 cases assert the three outputs it covers.
2. area_light: the properties of the rig it returns.
3. combine_lights refuses each malformed input before anything is launched (the launch is monkeypatched to fail if reached)."""
import numpy as np
import pytest
import torch

import light_rig_emulation as emu

EPS = 2.0 ** -23


def _case(seed, B, L, H, W, shared):
    rng = np.random.default_rng(seed)
    final = (1.2 * rng.random((B, L, H, W))).astype(np.float32)
    albedo = (0.1 + 0.8 * rng.random((B, 3, H, W))).astype(np.float32)
    rgb = rng.standard_normal((1 if shared else B, L, 3)).astype(np.float32)
    g_r = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    g_s = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    return final, albedo, rgb, g_r, g_s


@pytest.mark.parametrize("B,L,H,W,shared", [(1, 1, 3, 5, False), (2, 2, 4, 7, True), (2, 3, 5, 6, False), (3, 18, 7, 9, True),
                                            (2, 19, 6, 5, False), (1, 64, 4, 4, True)])
@pytest.mark.parametrize("which", ["both", "rendered", "shading"])
def test_restatement_against_f64_autograd(B, L, H, W, shared, which):
    final, albedo, rgb, g_r, g_s = _case(100 * L + B, B, L, H, W, shared)
    g_r = None if which == "shading" else g_r
    g_s = None if which == "rendered" else g_s
    rendered, sh = emu.forward(final, albedo, rgb)
    bw = emu.backward(final, albedo, rgb, g_r, g_s)

    t = lambda a: torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
    tf, ta, tr = t(final), t(albedo), t(rgb)
    sh64 = (tf[:, :, None] * tr[..., None, None]).sum(1)
    ren64 = sh64 * ta
    loss = 0.0
    if g_r is not None:
        loss = loss + (ren64 * torch.from_numpy(g_r.astype(np.float64))).sum()
    if g_s is not None:
        loss = loss + (sh64 * torch.from_numpy(g_s.astype(np.float64))).sum()
    loss.backward()

    f64 = lambda a: a.astype(np.float64)
    r_b = np.broadcast_to(f64(rgb), (B, L, 3))
    terms_sh = (np.abs(r_b)[..., None, None] * np.abs(f64(final))[:, :, None]).sum(1)                  # (B,3,H,W)
    terms_u = (0.0 if g_s is None else np.abs(f64(g_s))) + (0.0 if g_r is None else np.abs(f64(g_r)) * np.abs(f64(albedo)))
    terms = {"shading_rgb": terms_sh, "rendered": np.abs(f64(albedo)) * terms_sh,
             "g_albedo": (0.0 if g_r is None else np.abs(f64(g_r))) * terms_sh,
             "g_final": (np.abs(r_b)[..., None, None] * terms_u[:, None]).sum(2),                     # (B,L,H,W)
             "g_rgb": (np.abs(f64(final))[:, :, None] * terms_u[:, None]).sum(axis=(3, 4))}           # (B,L,3)
    if shared:
        terms["g_rgb"] = terms["g_rgb"].sum(0, keepdims=True)
    got = {"shading_rgb": sh, "rendered": rendered, "g_albedo": bw["g_albedo"], "g_final": bw["g_final"], "g_rgb": bw["g_rgb"]}
    g_albedo64 = ta.grad.numpy() if ta.grad is not None else np.zeros(albedo.shape)               # (no g_rendered: albedo is not reached)
    want = {"shading_rgb": sh64.detach().numpy(), "rendered": ren64.detach().numpy(), "g_albedo": g_albedo64,
            "g_final": tf.grad.numpy(), "g_rgb": tr.grad.numpy()}
    names = ["shading_rgb", "rendered", "g_albedo"] + (["g_final", "g_rgb"] if L >= 3 else [])
    for k in names:
        err = np.abs(f64(got[k]) - want[k])
        bound = L * EPS * terms[k]
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print("%s: largest error / bound = %.3f" % (k, worst))
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape
        assert (err <= bound).all(), (k, worst)
    # the f64 sum the GPU test measures g_rgb against, and its bound, are what they say
    np.testing.assert_allclose(bw["g_rgb_f64"], want["g_rgb"], rtol=0, atol=float((3 * EPS * terms["g_rgb"]).max()))
    assert (bw["g_rgb_bound"] <= EPS * terms["g_rgb"] * (1 + 1e-6)).all()


def test_restatement_first_product_initialises_and_nothing_is_clamped():
    """-0.0 survives (an add to +0.0 would turn it into +0.0), negative weights give negative shading, NaN stays in its pixel"""
    final = np.array([[[[0.0, 1.0, 2.0]]]], np.float32)
    albedo = np.ones((1, 3, 1, 3), np.float32)
    rgb = np.array([[[-1.0, 1.0, 0.0]]], np.float32)
    rendered, sh = emu.forward(final, albedo, rgb)
    assert np.signbit(sh[0, 0, 0, 0]) and sh[0, 0, 0, 0] == 0.0 and sh[0, 0, 0, 2] == -2.0 and rendered[0, 1, 0, 2] == 2.0
    final2 = np.stack([final[0, 0], final[0, 0]])[None].copy()
    final2[0, 1, 0, 1] = np.nan
    rendered, sh = emu.forward(final2, albedo, np.ones((1, 2, 3), np.float32))
    assert np.isnan(rendered[0, :, 0, 1]).all() and np.isnan(rendered).sum() == 3 and np.isnan(sh).sum() == 3


# ------------------------------------------------------------------------------------------------------------------------------
def _angles(lights, axis):
    L = lights.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(L, axis), axis=1), L @ axis)        # (arccos is ill-conditioned at 0)


@pytest.mark.parametrize("direction", [(0.0, 0.0, 1.0), (0.3, 0.6, 0.7), (-0.8138, -0.3420, 0.4698), (2.0, 0.0, 0.0)])
@pytest.mark.parametrize("radius", [0.0, 2.0, 15.0, 45.0, 90.0])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 18, 64])
def test_area_light_properties(direction, radius, n):
    from geomconsistentfr_amd.lighting import area_light
    colour = (1.0, 0.8, 0.5)
    lights, rgb = area_light(direction, radius, n, colour=colour)
    axis = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    assert lights.shape == (n, 3) and rgb.shape == (n, 3) and lights.dtype == rgb.dtype == np.float32
    assert np.abs(np.linalg.norm(lights.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert _angles(lights, axis).max() <= np.radians(radius) + 1e-6                # f32 rounding moves a direction by ~1e-7 rad
    mean = lights.astype(np.float64).mean(0)
    assert np.abs(mean / np.linalg.norm(mean) - axis).max() <= 1e-6
    np.testing.assert_allclose(rgb.astype(np.float64).sum(0), colour, rtol=0, atol=n * 2.0 ** -24)
    assert (rgb == rgb[0]).all()
    if n == 1:
        assert np.array_equal(lights[0], axis.astype(np.float32))
    elif radius > 0:
        assert _angles(lights, axis).max() >= 0.5 * np.radians(radius)             # the cap is used, not a point
        assert len({tuple(v) for v in lights.tolist()}) == n
    again = area_light(direction, radius, n, colour=colour)
    assert np.array_equal(again[0], lights) and np.array_equal(again[1], rgb)


def test_area_light_refuses_bad_arguments():
    from geomconsistentfr_amd.lighting import area_light
    for args in [((0, 0, 0), 10, 4), ((0, 0, 1), 10, 0), ((0, 0, 1), -1, 4), ((0, 0, 1), 91, 4), ((0, float("nan"), 1), 10, 4)]:
        with pytest.raises(ValueError):
            area_light(*args)


# ------------------------------------------------------------------------------------------------------------------------------
def test_combine_lights_refuses_malformed_inputs_before_any_launch(monkeypatch):
    from geomconsistentfr_amd import _lib, lighting
    from geomconsistentfr_amd import combine_lights

    def reached(*a, **k):
        raise AssertionError("a malformed input reached the launch")
    monkeypatch.setattr(_lib, "launch", reached)
    monkeypatch.setattr(_lib, "load", reached)
    B, L, H, W = 2, 3, 4, 5
    z = lambda *s, **k: torch.zeros(*s, dtype=k.get("dtype", torch.float32), device=k.get("device", "cpu"))
    good = (z(B, L, H, W), z(B, 3, H, W), z(B, L, 3))
    bad = {
        "final lacks the L axis": (z(B, H, W), good[1], good[2]),
        "final is (B,H,W) with B = L": (z(L, H, W), z(L, 3, H, W), z(1, L, 3)),
        "albedo carries an L axis": (good[0], z(B, L, 3, H, W), good[2]),
        "albedo has another size": (good[0], z(B, 3, H, W + 1), good[2]),
        "rgb with the wrong L": (good[0], good[1], z(B, L + 1, 3)),
        "rgb with batch neither 1 nor B": (good[0], good[1], z(B + 1, L, 3)),
        "rgb without the batch axis": (good[0], good[1], z(L, 3)),
        "rgb with four channels": (good[0], good[1], z(B, L, 4)),
        "f64 final": (z(B, L, H, W, dtype=torch.float64), good[1], good[2]),
        "f16 albedo": (good[0], z(B, 3, H, W, dtype=torch.float16), good[2]),
        "f64 rgb": (good[0], good[1], z(B, L, 3, dtype=torch.float64)),
        "mixed devices": (z(B, L, H, W, device="meta"), good[1], good[2]),
        "mixed devices (rgb)": (good[0], good[1], z(B, L, 3, device="meta")),
        "no lights": (z(B, 0, H, W), good[1], z(B, 0, 3)),
        "not a tensor": (good[0], good[1], np.zeros((B, L, 3), np.float32)),
    }
    for why, args in bad.items():
        with pytest.raises(_lib.GcfrError):
            combine_lights(*args)
            pytest.fail(why)
    # well-formed but on the host: refused as well (there is no CPU path), still before the launch
    with pytest.raises(_lib.GcfrError, match="no CPU path"):
        combine_lights(*good)
    with pytest.raises(_lib.GcfrError, match="no CPU path"):
        combine_lights(good[0], good[1], z(1, L, 3))


def test_library_refuses_unsupported_rig_shapes_before_a_launch():
    """the C entry points validate on the host (no GPU needed): NULLs, L out of range, rgb_batch neither 1 nor B, no upstream
    gradient, no output"""
    import ctypes
    from geomconsistentfr_amd import _lib
    L_ = _lib.load()
    p = ctypes.c_void_p(4096)
    ok = (p, p, p, 1, 2, 3, 4, 5)
    assert L_.gcfr_light_rig_fwd(None, p, p, 1, 2, 3, 4, 5, p, p, None) == -1
    assert L_.gcfr_light_rig_fwd(*ok, None, p, None) == -1                          # rendered is required
    for B, L, H, W, rb in [(0, 3, 4, 5, 1), (2, 0, 4, 5, 1), (2, 4097, 4, 5, 1), (2, 3, 0, 5, 1), (2, 3, 4, 0, 1), (2, 3, 4, 5, 3),
                           (2, 3, 4, 5, 0), (1, 1, 65536, 65536, 1)]:
        assert L_.gcfr_light_rig_fwd(p, p, p, rb, B, L, H, W, p, p, None) == -1, (B, L, H, W, rb)
        assert L_.gcfr_light_rig_bwd(p, p, p, rb, B, L, H, W, p, p, p, p, p, None) == -1, (B, L, H, W, rb)
    assert L_.gcfr_light_rig_bwd(*ok, None, None, p, p, p, None) == -1              # neither upstream gradient
    assert L_.gcfr_light_rig_bwd(*ok, p, p, None, None, None, None) == -1           # no output
    assert L_.gcfr_light_rig_bwd(*ok, p, p, p, p, ctypes.c_void_p(4100), None) == -1   # g_rgb is f64: 8-byte aligned


def test_relight_session_signature_keeps_its_defaults():
    import inspect
    from geomconsistentfr_amd import inference as inf
    sig = inspect.signature(inf.RelightSession.__init__)
    assert sig.parameters["light_rgb"].default is None
    assert list(sig.parameters)[-1] == "light_rgb"                                  # appended: positional callers are unaffected
    for name in ("relight_rig", "relight_rig_device"):
        assert list(inspect.signature(getattr(inf, name)).parameters)[:5] == ["model", "images", "mask_u8", "lights", "light_rgb"]
