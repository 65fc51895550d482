"""GPU: the light-rig stage (csrc/gcfr_light_rig.hip; lighting.combine_lights / render_rig_from_depth; inference.relight_rig /
RelightSession(light_rgb=...)) against its numpy-f32 restatement (tests/light_rig_emulation.py, itself held to f64 autograd by
tests/test_light_rig_host.py) and against the paths that are already pinned.

  kernels      rendered, shading_rgb, g_final, g_albedo: BIT-EQUAL to the restatement.  g_rgb: within 2^-23 sum_p |final u| of the
               restatement's f64 sum per entry (one f32 rounding of an f64 sum whose order is free; the bound is the restatement's).
  identity     one light of colour 1 is the block's own composite bit for bit; the per-light outputs are untouched by the stage.
  gradients    end to end against the torch composition over the many-lights outputs, under the gates
               tests/test_gpu_backward.py:291-295 applies to the many-lights entry (ambient rtol 1e-5; light rtol 1e-4 with
               atol 1e-5 max|g|; albedo and depth 1e-5 max|g|); the rig's own gradient, a small per-light vector like the
               light's, under the light's gate (line 293).
  bytes        relight_rig == the image kernel on combine_lights of the same forward_lights outputs; a point rig of one light ==
               relight_lights(...)[:, 0]; a captured RelightSession(light_rgb=...) == the eager relight_rig_device, byte for byte on
               fixed head outputs (the comparison tests/test_gpu_relight_lights.py:192 uses for session against eager).

Measured on an MI355X (largest figures over all cases of a test; every case prints its own before it asserts):
  kernels      all 28 kernel cases (shapes, upstream gradients alone and together, misaligned pointers, NaN): 0 elements differ in
               rendered, shading_rgb, g_final, g_albedo.  g_rgb, |error| against the f64 sum as a share of its bound: 0.45 at the
               largest (the two cases of 1 and 7 pixels, where the bound is one f32 rounding of a handful of terms), 0.14 or less
               from 36 pixels on, 0.006 at (2,18,256,256) (2.7e-5 absolute on sums of ~4e3 terms)
  gradients    end to end, max|diff| / max|g|: depth 5.5e-8 (8.0e-8 with the extra gradient on final_shading), light_rgb 1.1e-7,
               albedo, light and ambient 0; the two forward images identical
  bytes        every comparison byte for byte
"""
import numpy as np
import pytest
import torch

import light_rig_emulation as emu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

def _inputs(seed, B, L, H, W, shared, rgb_kind="random"):
    rng = np.random.default_rng(seed)
    final = (1.2 * rng.random((B, L, H, W))).astype(np.float32)
    albedo = (0.1 + 0.8 * rng.random((B, 3, H, W))).astype(np.float32)
    rgb = rng.standard_normal((1 if shared else B, L, 3)).astype(np.float32)
    if rgb_kind == "zeros_and_negatives":
        rgb[:, ::2, 0] = 0.0
        rgb[:, :, 1] = -np.abs(rgb[:, :, 1])
        rgb[:, -1] = 0.0
    g_r = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    g_s = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    return final, albedo, rgb, g_r, g_s


def _dev(a, misalign=False):
    """a device tensor of `a`; misalign: its first element sits 4 bytes past a 16-byte boundary (the scalar path)"""
    if not misalign:
        return torch.from_numpy(a).to(DEV)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _gpu(final, albedo, rgb, g_r, g_s, misalign=False):
    from geomconsistentfr_amd import combine_lights
    tf, ta, tr = [_dev(a, misalign).requires_grad_() for a in (final, albedo, rgb)]
    rendered, sh = combine_lights(tf, ta, tr)
    loss = 0.0
    if g_r is not None:
        loss = loss + (rendered * torch.from_numpy(g_r).to(DEV)).sum()
    if g_s is not None:
        loss = loss + (sh * torch.from_numpy(g_s).to(DEV)).sum()
    loss.backward()
    c = lambda t: t.detach().cpu().numpy()
    return {"rendered": c(rendered), "shading_rgb": c(sh), "g_final": c(tf.grad),
            "g_albedo": c(ta.grad), "g_rgb": c(tr.grad)}


def _same_bits(a, b):
    """bit-equal, any NaN matching any NaN in the same place (a NaN's payload is not part of the contract)"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and emu.bit_equal(np.where(na, np.float32(0), a), np.where(nb, np.float32(0), b))


def _check(label, got, final, albedo, rgb, g_r, g_s):
    rendered, sh = emu.forward(final, albedo, rgb)
    bw = emu.backward(final, albedo, rgb, g_r, g_s)
    want = {"rendered": rendered, "shading_rgb": sh, "g_final": bw["g_final"], "g_albedo": bw["g_albedo"]}
    diffs = {k: int((~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))).sum()) for k in want}
    err = np.abs(got["g_rgb"].astype(np.float64) - bw["g_rgb_f64"])
    ok = ~np.isnan(bw["g_rgb_f64"])
    ratio = float((err[ok] / np.maximum(bw["g_rgb_bound"][ok], 1e-300)).max()) if ok.any() else 0.0
    print("%s: elements that differ %s; g_rgb largest |error| %.3e = %.3f of its bound" % (label, diffs, float(err[ok].max()) if ok.any() else 0.0, ratio))
    for k in want:
        assert _same_bits(got[k], want[k]), (label, k, diffs[k])
    assert got["g_rgb"].shape == rgb.shape and got["g_rgb"].dtype == np.float32
    assert np.array_equal(np.isnan(got["g_rgb"]), ~ok), label
    assert (err[ok] <= bw["g_rgb_bound"][ok]).all(), (label, ratio)
    return bw


SHAPES = [  # (B, L, H, W, shared rig)
    (1, 1, 1, 1, False), (1, 3, 1, 7, False),                       # one pixel; shorter than a vector
    (2, 5, 21, 37, False),                                          # odd plane: misaligned albedo planes and lights, scalar path
    (1, 2, 1, 1023, False), (1, 2, 32, 32, False), (1, 2, 5, 205, False),      # plane sizes 1023, 1024, 1025: the chunk's edge
    (1, 2, 36, 36, False),                                          # vector path, a second, partial chunk
    (1, 1, 11, 11, False), (1, 2, 11, 11, False), (1, 18, 11, 11, False), (1, 19, 11, 11, False), (1, 64, 11, 11, False),
    (3, 5, 11, 11, True), (3, 5, 11, 11, False),                    # a shared rig (g_rgb sums over the faces); per-face rigs
    (3, 4, 6, 6, True),                                             # the same on the vector path
    (2, 1030, 1, 1100, True),                                       # more lights than the backward's LDS tile, two chunks
    (1, 4096, 1, 7, False),                                         # the most lights the entry takes
    (2, 18, 256, 256, False),                                       # the serving shape's kind: many chunks per face
]


@pytest.mark.parametrize("B,L,H,W,shared", SHAPES)
def test_kernels_equal_the_restatement(B, L, H, W, shared):
    final, albedo, rgb, g_r, g_s = _inputs(7 * L + H, B, L, H, W, shared)
    _check("(%d,%d,%d,%d)%s" % (B, L, H, W, " shared" if shared else ""), _gpu(final, albedo, rgb, g_r, g_s), final, albedo, rgb, g_r, g_s)


@pytest.mark.parametrize("which", ["shading_only", "rendered_only", "both"])
@pytest.mark.parametrize("B,L,H,W,shared", [(2, 5, 21, 37, True), (2, 6, 16, 24, False)])       # scalar and vector path
def test_upstream_gradients_alone_and_together(B, L, H, W, shared, which):
    final, albedo, rgb, g_r, g_s = _inputs(11, B, L, H, W, shared, rgb_kind="zeros_and_negatives")
    g_r = None if which == "shading_only" else g_r
    g_s = None if which == "rendered_only" else g_s
    got = _gpu(final, albedo, rgb, g_r, g_s)
    _check("%s (%d,%d,%d,%d)" % (which, B, L, H, W), got, final, albedo, rgb, g_r, g_s)
    assert (got["shading_rgb"][:, 1] <= 0).all() and (got["shading_rgb"] < 0).any()          # negative weights: nothing is clamped


def test_pointers_off_the_vector_alignment_take_the_scalar_path():
    """H W a multiple of 4 but every tensor 4 bytes past a 16-byte boundary: the same bits"""
    final, albedo, rgb, g_r, g_s = _inputs(5, 2, 3, 8, 12, False)
    _check("misaligned", _gpu(final, albedo, rgb, g_r, g_s, misalign=True), final, albedo, rgb, g_r, g_s)


@pytest.mark.parametrize("H,W", [(9, 7), (8, 8)])
def test_one_nan_stays_in_its_pixel(H, W):
    B, L = 2, 4
    final, albedo, rgb, g_r, g_s = _inputs(3, B, L, H, W, True)
    rgb[0, 2] = (0.0, 1.0, -1.0)                                    # 0 * NaN is NaN as well
    b, l, y, x = 1, 2, H // 2, W - 1
    final[b, l, y, x] = np.nan
    got = _gpu(final, albedo, rgb, g_r, g_s)
    _check("NaN %dx%d" % (H, W), got, final, albedo, rgb, g_r, g_s)
    where = np.zeros((B, 3, H, W), bool)
    where[b, :, y, x] = True
    for k in ("rendered", "shading_rgb", "g_albedo"):
        assert np.array_equal(np.isnan(got[k]), where), k
    assert not np.isnan(got["g_final"]).any()                       # g_final does not read final
    rig_nan = np.zeros(rgb.shape, bool)
    rig_nan[0, l] = True                                            # that light's three sums, and no other entry
    assert np.array_equal(np.isnan(got["g_rgb"]), rig_nan)


# ------------------------------------------------------------------------------------------------------------------------------
# the block + the stage
# ------------------------------------------------------------------------------------------------------------------------------
Hs, Ws = 32, 48


def _scene(B, L):
    """a scene of tools/scenes.py at 32 x 48: the 48 x 48 synthetic faces, rows 8 .. 40"""
    import scenes
    depth, mask, albedo, _n, light, amb = scenes.synth_faces_sized(B, 21, Ws, L)
    rows = slice((Ws - Hs) // 2, (Ws - Hs) // 2 + Hs)
    return (np.ascontiguousarray(depth[:, None, rows]), np.ascontiguousarray(mask[:, rows]), np.ascontiguousarray(albedo[:, :, rows]),
            np.ascontiguousarray(light.astype(np.float32)), (amb + 0.05 * np.arange(L, dtype=np.float32)).astype(np.float32))


def _camera():
    from geomconsistentfr_amd.inference import camera_matrix
    return camera_matrix(700.0, Hs, Ws)


def _params():
    from geomconsistentfr_amd import RenderParams
    return RenderParams(n_samples=40, dt=0.02)


def test_one_white_light_is_the_blocks_own_composite_and_the_per_light_outputs_are_untouched():
    from geomconsistentfr_amd import render_rig_from_depth
    from geomconsistentfr_amd.block import render_from_depth
    B = 2
    t = lambda a: torch.from_numpy(a).to(DEV)
    for L in (1, 3):
        depth, mask, albedo, light, amb = [t(a) for a in _scene(B, L)]
        rgb = torch.ones(B, L, 3, device=DEV) if L == 1 else torch.from_numpy(np.random.default_rng(2).standard_normal((1, L, 3)).astype(np.float32)).to(DEV)
        plain = render_from_depth(depth, albedo, light, amb, _camera(), 500.0, mask, _params())
        rig = render_rig_from_depth(depth, albedo, light, amb, rgb, _camera(), 500.0, mask, _params())
        assert tuple(rig["rig_rendered_images"].shape) == (B, 3, Hs, Ws) and tuple(rig["rig_shading"].shape) == (B, 3, Hs, Ws)
        for k, v in plain.items():                                   # the plain call's dict, bit for bit
            assert torch.equal(rig[k], v), (L, k)
        assert set(rig) == set(plain) | {"rig_rendered_images", "rig_shading"}
        assert float(plain["final_shading"].std()) > 0.01            # a lit face, not a constant
        if L == 1:
            assert torch.equal(rig["rig_rendered_images"], plain["rendered_images"][:, 0])
            assert torch.equal(rig["rig_shading"], plain["final_shading"][:, 0, None].expand(B, 3, Hs, Ws))


@pytest.mark.parametrize("extra_on_final", [False, True])
def test_end_to_end_gradients_equal_the_torch_composition(extra_on_final):
    """Both legs run the same gcfr_render_bwd; they differ in the rounding of g_final and in atomic order.  Gates:
    tests/test_gpu_backward.py:291-295 (see the module docstring).  extra_on_final: the caller also puts a gradient on
    final_shading itself -- autograd adds it to the stage's."""
    from geomconsistentfr_amd import render_rig_from_depth
    from geomconsistentfr_amd.block import render_from_depth
    B, L = 2, 3
    depth, mask, albedo, light, amb = _scene(B, L)
    rng = np.random.default_rng(8)
    rgb = (0.2 + rng.random((B, L, 3))).astype(np.float32)
    P = torch.from_numpy(rng.standard_normal((B, 3, Hs, Ws)).astype(np.float32)).to(DEV)
    Gf = torch.from_numpy(rng.standard_normal((B, L, Hs, Ws)).astype(np.float32)).to(DEV)
    mask_t = torch.from_numpy(mask).to(DEV)
    leaf = lambda a: torch.from_numpy(a).to(DEV).requires_grad_()

    def leg(use_stage, extra=extra_on_final):
        leaves = [leaf(a) for a in (depth, albedo, light, amb, rgb)]
        d, a, li, am, r = leaves
        if use_stage:
            o = render_rig_from_depth(d, a, li, am, r, _camera(), 500.0, mask_t, _params())
            out = o["rig_rendered_images"]
        else:
            o = render_from_depth(d, a, li, am, _camera(), 500.0, mask_t, _params())
            out = (o["final_shading"][:, :, None] * r[..., None, None]).sum(1) * a
        loss = (out * P).sum()
        if extra:
            loss = loss + (o["final_shading"] * Gf).sum()
        loss.backward()
        return [t.grad.cpu().numpy() for t in leaves], out.detach()

    (gd, ga, gl, gamb, grgb), out_s = leg(True)
    (gd0, ga0, gl0, gamb0, grgb0), out_t = leg(False)
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
    print("extra_on_final=%s: max|diff| / max|g|: depth %.2e albedo %.2e light %.2e ambient %.2e light_rgb %.2e; forward %.2e"
          % (extra_on_final, rel(gd, gd0), rel(ga, ga0), rel(gl, gl0), rel(gamb, gamb0), rel(grgb, grgb0),
             float((out_s - out_t).abs().max())))
    assert np.abs(gd0).max() > 0 and np.abs(gl0).max() > 0 and np.abs(grgb0).max() > 0
    np.testing.assert_allclose(gamb, gamb0, rtol=1e-5)                                              # test_gpu_backward.py:291
    np.testing.assert_allclose(gl, gl0, rtol=1e-4, atol=1e-5 * np.abs(gl0).max())                   # :293
    np.testing.assert_allclose(grgb, grgb0, rtol=1e-4, atol=1e-5 * np.abs(grgb0).max())             # :293, for the rig's vector
    assert np.abs(ga - ga0).max() <= 1e-5 * np.abs(ga0).max()                                       # :294
    assert np.abs(gd - gd0).max() <= 1e-5 * np.abs(gd0).max()                                       # :295
    if extra_on_final:                                              # the two contributions add: the stage's alone is another gradient
        (_d, _a, _l, gamb1, _r), _ = leg(True, extra=False)
        assert np.abs(gamb - gamb1).max() > 1e-3 * np.abs(gamb).max()


# ------------------------------------------------------------------------------------------------------------------------------
# bytes
# ------------------------------------------------------------------------------------------------------------------------------
def _fixed_net(B, size, seed=90):
    """RelightNetSingleImage on FIXED head outputs (MIOpen's convolutions are not run-to-run reproducible; the stage, the block and
    the image kernel are): features() returns given tensors and fires the prepass hook the way the real one does"""
    import scenes
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    depth, mask, albedo, _n, _l, _a = scenes.synth_faces_sized(B, seed, size, 1)
    rng = np.random.default_rng(seed)
    sl = np.concatenate([0.4 + 0.2 * rng.random((B, 1)), rng.standard_normal((B, 3))], 1).astype(np.float32).reshape(B, 1, 1, 4)
    dev_heads = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (albedo, depth[:, None], sl)]

    class Fixed(RelightNetSingleImage):
        def features(self, img, epoch, on_depth=None):
            a, d, SL = [t.clone() for t in dev_heads]
            if on_depth is not None:
                on_depth(d, SL)
            return a, d, SL

    return Fixed(img_height=size, img_width=size).to(DEV).eval(), (mask[0] * 255).astype(np.uint8)


def test_relight_rig_bytes():
    from geomconsistentfr_amd import area_light, combine_lights
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    B, S = 2, 64
    net, mask_u8 = _fixed_net(B, S)
    rng = np.random.default_rng(6)
    images = rng.random((B, S, S, 3), dtype=np.float32)
    lights, rgb = area_light((0.5145, 0.0, 0.8575), 12.0, 5, colour=(1.0, 0.9, 0.7))
    for fix in (False, True):
        got = inf.relight_rig(net, images, mask_u8, lights, rgb, device=DEV, fix_border=fix)
        assert got.shape == (B, S, S, 3) and got.dtype == np.uint8
        x = torch.from_numpy(images).to(DEV)
        m = torch.from_numpy(mask_u8).to(DEV)
        with torch.no_grad():
            out = net.forward_lights(x, 200, inf.camera_matrix(1570.0, S, S), (m.to(torch.float64).reshape(S, S, 1) / 255.0),
                                     torch.from_numpy(lights).to(DEV))
            rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(rgb).to(DEV)[None])
            want = pp.inference_images_device(x, rendered, m)["rendered_image"]
            if fix:
                want = pp.fix_border_artifacts_device(want, m)
        np.testing.assert_array_equal(got, want.cpu().numpy())
    assert got.std() > 10
    # a point rig: one light, no spread, white -- the many-lights call's first image
    d = (-0.5843, 0.0, 0.8115)
    l1, rgb1 = area_light(d, 0.0, 1)
    np.testing.assert_array_equal(inf.relight_rig(net, images, mask_u8, l1, rgb1, device=DEV),
                                  inf.relight_lights(net, images, mask_u8, l1, device=DEV)[:, 0])
    # a rig is not its first light
    assert np.abs(got.astype(int) - inf.relight_lights(net, images, mask_u8, lights[:1], device=DEV, fix_border=True)[:, 0].astype(int)).max() > 0


def test_relight_session_with_a_rig_replays_the_eager_pass():
    """B = 2, 64 x 64, L = 3, captured once and replayed twice; the machine's default number of hardware queues"""
    from geomconsistentfr_amd import inference as inf
    B, S = 2, 64
    net, mask_u8 = _fixed_net(B, S)
    rng = np.random.default_rng(4)
    imgs_a, imgs_b = rng.random((B, S, S, 3), dtype=np.float32), rng.random((B, S, S, 3), dtype=np.float32)
    lights = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)
    rgb = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)
    sess = inf.RelightSession(net, B, mask_u8, lights, device=DEV, H=S, W=S, light_rgb=rgb)
    assert sess.graph is not None
    for imgs in (imgs_a, imgs_b):
        got = sess.run(torch.from_numpy(imgs))
        assert tuple(got.shape) == (B, S, S, 3) and got.dtype == torch.uint8
        want = inf.relight_rig_device(net, imgs, mask_u8, lights, rgb, device=DEV)
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    # without light_rgb the session is what it was: (B,L,H,W,3)
    plain = inf.RelightSession(net, B, mask_u8, lights, device=DEV, H=S, W=S, graph=False)
    assert tuple(plain.run(torch.from_numpy(imgs_a)).shape) == (B, 3, S, S, 3)
