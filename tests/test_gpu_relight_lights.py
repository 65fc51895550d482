"""GPU: many lights per face at the boundary callers use (round 6; BASELINE configs[4]'s actual use).

`RelightNetSingleImage.forward_lights` / `RelightNetLightingTransfer.forward_lights` / `inference.relight_lights`: ONE network
pass, one prepass and one normals stage per face, L marches, one image-kernel launch -- against L calls of the one-light
forms (what the reference does: the whole model once per light, S1:582-588), at the eleven directions the reference ships
(S1:519-562).  The network's convolutions are MIOpen's (not run-to-run reproducible), so the bit-level comparisons run on
FIXED head outputs (a subclass whose features() returns given tensors and fires the prepass hook the way the real one does);
the real network with the shipped lighting-transfer checkpoint is compared within a byte tolerance."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = W = 256


def _lights11():
    from geomconsistentfr_amd.inference import LIGHT_DIRECTIONS
    return np.asarray(list(LIGHT_DIRECTIONS.values()), np.float32)


def _fixed_heads(B, seed):
    import scenes
    depth, mask, albedo, _n, _l, _a = scenes.synth_faces(B, seed)
    rng = np.random.default_rng(seed)
    sl = np.concatenate([0.4 + 0.2 * rng.random((B, 1)), rng.standard_normal((B, 3))], 1).astype(np.float32).reshape(B, 1, 1, 4)
    return depth[:, None], albedo, sl, (mask[0] * 255).astype(np.uint8)


def _fixed(cls, heads, **kw):
    d0, a0, sl0, _ = heads

    dev_heads = [torch.from_numpy(x).to(DEV) for x in (a0, d0, sl0)]      # uploaded once (a session captures features() in a graph)

    class Fixed(cls):
        def features(self, img, epoch, on_depth=None):
            albedo, depth, SL = [t.clone() for t in dev_heads]
            if on_depth is not None:
                on_depth(depth, SL)
            return albedo, depth, SL

    return Fixed(**kw).to(DEV).eval()


def _K(f):
    from geomconsistentfr_amd.inference import camera_matrix
    return camera_matrix(f, H, W, DEV)


@pytest.mark.parametrize("hoist", [True, False])
def test_single_image_forward_lights_equals_eleven_forwards(hoist):
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    B = 3
    heads = _fixed_heads(B, 40)
    net = _fixed(RelightNetSingleImage, heads)
    net.hoist_prepass = hoist
    lights = _lights11()
    img = torch.zeros(B, H, W, 3, device=DEV)
    mask = torch.from_numpy(heads[3].astype(np.float64) / 255.0).reshape(H, W, 1).to(DEV)
    with torch.no_grad():
        many = net.forward_lights(img, 200, _K(1570.0), mask, lights)
        assert len(many) == 10 and tuple(many[5].shape) == (B, 11, 3, H, W) and tuple(many[2].shape) == (B, 11, H, W)
        assert tuple(many[6].shape) == (B, 11, 3, 1, 1) and tuple(many[7].shape) == (B, 11, 1, 1) and tuple(many[9].shape) == (B, 3, H, W)
        for l in range(11):
            tl = torch.from_numpy(np.repeat(lights[l][None], B, 0)).reshape(B, 3, 1, 1).to(DEV)
            one = net(img, 200, _K(1570.0), mask, tl, torch.zeros(B, 1, 1, device=DEV), mask[None])
            for k in (2, 3, 4, 5, 6, 7, 8):
                assert torch.equal(many[k][:, l], one[k]), (k, l)
            assert torch.equal(many[9], one[9]) and torch.equal(many[0], one[0]) and torch.equal(many[1], one[1])
        # per-face light sets (B,L,3): face b under its own rotation of the eleven
        per_face = np.stack([np.roll(lights, b, axis=0)[:4] for b in range(B)])
        pf = net.forward_lights(img, 200, _K(1570.0), mask, per_face)
        for b in range(B):
            for l in range(4):
                assert torch.equal(pf[5][b, l], many[5][b, (l - b) % 11])


def test_lighting_transfer_forward_lights_equals_forwards():
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    B = 2
    heads = _fixed_heads(B, 7)
    net = _fixed(RelightNetLightingTransfer, heads)
    lights = _lights11()[:5]
    ambs = np.array([0.5, 0.45, 0.6, 0.3, 0.55], np.float32)
    img = torch.zeros(B, H, W, 3, device=DEV)
    mask = (torch.from_numpy(heads[3]).to(DEV).reshape(H, W, 1) / 255.0)                      # f32, as SLT:540
    with torch.no_grad():
        many = net.forward_lights(img, 200, _K(700.0), mask, lights, ambs)
        assert len(many) == 12
        for l in range(5):
            tl = torch.from_numpy(np.repeat(lights[l][None], B, 0)).reshape(B, 3, 1, 1).to(DEV)
            one = net(img, 200, _K(700.0), mask, tl, torch.full((B, 1, 1), float(ambs[l]), device=DEV))
            for k in (2, 3, 4, 5, 6, 7, 8):
                assert torch.equal(many[k][:, l], one[k]), (k, l)
            for k in (9, 10, 11):
                assert torch.equal(many[k], one[k])


@pytest.mark.parametrize("transfer", [False, True])
def test_relight_lights_bytes_equal_eleven_relight_images_calls(transfer):
    """(B,11) uint8 composites from ONE forward_lights + ONE image-kernel launch == eleven relight_images() calls, byte for byte,
    border fix included."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer, RelightNetSingleImage
    B = 2
    heads = _fixed_heads(B, 90)
    net = _fixed(RelightNetLightingTransfer if transfer else RelightNetSingleImage, heads)
    rng = np.random.default_rng(3)
    images = rng.random((B, H, W, 3), dtype=np.float32)
    lights = _lights11()
    for fix in (False, True):
        got = inf.relight_lights(net, images, heads[3], lights, ambient=0.5, device=DEV, fix_border=fix)
        assert got.shape == (B, 11, H, W, 3) and got.dtype == np.uint8
        for l in range(11):
            one = inf.relight_images(net, images, heads[3], np.repeat(lights[l][None], B, 0), ambient=0.5, device=DEV, fix_border=fix)
            np.testing.assert_array_equal(got[:, l], one, err_msg="light %d fix_border %s" % (l, fix))
    assert got.std() > 10                                                                # not a blank image


def test_image_kernel_many_lights_equals_per_light_launches():
    """gcfr_inference_images_u8 with L relit images per photograph (ABI 6): the photograph is read in place once per light --
    the same bytes as L launches, diagnostic maps included, both mask modes, per-face masks."""
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(12)
    B, L, Hs, Ws = 3, 4, 40, 56
    f = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32)).to(DEV)
    x, ren, w, fin = f(B, Hs, Ws, 3), f(B, L, 3, Hs, Ws) * 1.2 - 0.1, f(B, L, Hs, Ws), f(B, L, Hs, Ws) * 1.1
    alb, depth, nrm = f(B, 3, Hs, Ws), f(B, 1, Hs, Ws) * 80 - 40, f(B, 3, Hs, Ws) * 2 - 1
    masks = torch.from_numpy(rng.choice([0, 64, 128, 255], size=(B, Hs, Ws)).astype(np.uint8)).to(DEV)
    for mask_f32 in (False, True):
        for m in (masks, masks[:1]):
            many = pp.inference_images_device(x, ren, m, albedo=alb, depth=depth, shadow_mask_weights=w, final_shading=fin,
                                              surface_normals=nrm, mask_f32=mask_f32)
            assert tuple(many["rendered_image"].shape) == (B, L, Hs, Ws, 3) and tuple(many["albedo"].shape) == (B, Hs, Ws, 3)
            for l in range(L):
                one = pp.inference_images_device(x, ren[:, l], m, albedo=alb, depth=depth, shadow_mask_weights=w[:, l],
                                                 final_shading=fin[:, l], surface_normals=nrm, mask_f32=mask_f32)
                for k in ("rendered_image", "shadow_mask", "shading"):
                    assert torch.equal(many[k][:, l], one[k]), (k, l)
                for k in ("albedo", "depth", "surface_normals"):
                    assert torch.equal(many[k], one[k]), k


def test_relight_lights_with_the_shipped_checkpoint_close_to_per_light_runs():
    """The real network (the reference's lighting-transfer checkpoint, tests/golden/slt_checkpoint_epoch106.npz) on the
    reference's own input photographs: relight_lights against per-light relight_images.  Two network passes need not agree to
    the last bit (MIOpen), a shadow decision can flip on isolated pixels: >= 99.9 % of the bytes identical, >= 99.99 % within 1."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "slt_checkpoint_epoch106.npz")).items()}
    net = RelightNetLightingTransfer()
    net.load_state_dict(sd, strict=True)
    net = net.float().to(DEV).eval()
    za, zb = [np.load(os.path.join(GOLDEN, "slt_main_%s.npz" % t)) for t in ("a", "b")]
    images = np.stack([za["input_u8"] / 255.0, zb["input_u8"] / 255.0]).astype(np.float32)
    lights = _lights11()
    got = inf.relight_lights(net, images, za["mask_u8"], lights, ambient=0.5, device=DEV)
    assert got.shape == (2, 11, H, W, 3)
    for l in (0, 5, 10):
        one = inf.relight_images(net, images, za["mask_u8"], np.repeat(lights[l][None], 2, 0), ambient=0.5, device=DEV)
        diff = np.abs(got[:, l].astype(int) - one.astype(int))
        assert (diff == 0).mean() >= 0.999 and (diff <= 1).mean() >= 0.9999, (l, (diff == 0).mean(), diff.max())
    # the lights differ from each other (eleven different images, not one repeated)
    assert np.abs(got[:, 0].astype(int) - got[:, 4].astype(int)).mean() > 1.0


@pytest.mark.parametrize("graph", [True, False])
def test_relight_session_replays_the_eager_pass(graph):
    """inference.RelightSession: the whole pass (network forward, render block, image kernel) captured once into a hipGraph on
    static buffers.  On FIXED head outputs the replay gives the eager pass's bytes exactly (the block and the image kernel are
    deterministic); new photographs copied into the static input reach the composites (outside the mask the composite IS the
    photograph, S1:612-618)."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    B = 2
    heads = _fixed_heads(B, 90)
    net = _fixed(RelightNetSingleImage, heads)
    rng = np.random.default_rng(4)
    imgs_a, imgs_b = rng.random((B, H, W, 3), dtype=np.float32), rng.random((B, H, W, 3), dtype=np.float32)
    lights = _lights11()
    sess = inf.RelightSession(net, B, heads[3], lights, device=DEV, graph=graph)
    assert (sess.graph is not None) == graph
    for imgs in (imgs_a, imgs_b, imgs_a):
        got = sess.run(torch.from_numpy(imgs)).cpu().numpy()
        want = inf.relight_lights(net, imgs, heads[3], lights, device=DEV)
        np.testing.assert_array_equal(got, want)
    off = heads[3] == 0
    assert np.array_equal(got[0, 3][off], np.round(imgs_a[0][off] * 255.0).astype(np.uint8)) or \
        np.abs(got[0, 3][off].astype(int) - (imgs_a[0][off] * 255.0)).max() <= 0.5 + 1e-3


def test_relight_session_with_the_real_network_matches_the_eager_pass():
    """The shipped lighting-transfer checkpoint through a captured session (MIOpen's convolutions inside the graph) against the
    eager relight_lights: >= 99.9 % of the bytes identical, >= 99.99 % within 1 (MIOpen is not run-to-run reproducible)."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "slt_checkpoint_epoch106.npz")).items()}
    net = RelightNetLightingTransfer()
    net.load_state_dict(sd, strict=True)
    net = net.float().to(DEV).eval()
    za, zb = [np.load(os.path.join(GOLDEN, "slt_main_%s.npz" % t)) for t in ("a", "b")]
    images = np.stack([za["input_u8"] / 255.0, zb["input_u8"] / 255.0]).astype(np.float32)
    lights = _lights11()
    sess = inf.RelightSession(net, 2, za["mask_u8"], lights, ambient=0.5, device=DEV)
    got = sess.run(images).cpu().numpy()
    want = inf.relight_lights(net, images, za["mask_u8"], lights, ambient=0.5, device=DEV)
    diff = np.abs(got.astype(int) - want.astype(int))
    assert (diff == 0).mean() >= 0.999 and (diff <= 1).mean() >= 0.9999, ((diff == 0).mean(), diff.max())
    assert got.std() > 10


def test_relight_session_miopen_find_restores_the_flag():
    """`miopen_find=True` switches `torch.backends.cudnn.benchmark` on for the session's warm-up only (MIOpen searches its solvers
    there: bench.py's leg and tools/relight_bench.py run it on the real network, +14 %) and restores whatever the caller had set.
    On fixed head outputs (no convolution runs: the test costs no search) the composites are the eager pass's."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    heads = _fixed_heads(1, 12)
    net = _fixed(RelightNetSingleImage, heads)
    images = np.random.default_rng(2).random((1, H, W, 3), dtype=np.float32)
    lights = _lights11()[:3]
    for before in (False, True):
        torch.backends.cudnn.benchmark = before
        try:
            for graph in (True, False):
                sess = inf.RelightSession(net, 1, heads[3], lights, device=DEV, miopen_find=True, graph=graph)
                assert torch.backends.cudnn.benchmark is before
                np.testing.assert_array_equal(sess.run(images).cpu().numpy(), inf.relight_lights(net, images, heads[3], lights, device=DEV))
        finally:
            torch.backends.cudnn.benchmark = False


def test_two_sessions_in_flight_on_two_streams_do_not_disturb_each_other():
    """bench.py's throughput form of the end-to-end leg: two RelightSessions (own static buffers, own graphs) replayed
    round-robin on two HIP streams.  Each must give the bytes it gives alone."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    B = 2
    heads = _fixed_heads(B, 90)
    net = _fixed(RelightNetSingleImage, heads)
    rng = np.random.default_rng(8)
    imgs = [torch.from_numpy(rng.random((B, H, W, 3), dtype=np.float32)).to(DEV) for _ in range(2)]
    lights = _lights11()
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    sess = []
    for st in streams:
        with torch.cuda.stream(st):
            sess.append(inf.RelightSession(net, B, heads[3], lights, device=DEV))
    torch.cuda.synchronize()
    alone = []
    for i in range(2):
        alone.append(sess[i].run(imgs[i]).clone())
        torch.cuda.synchronize()
    outs = [None, None]
    for rep in range(6):
        i = rep % 2
        streams[i].wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(streams[i]):
            outs[i] = sess[i].run(imgs[i])
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(outs[i], alone[i]), i
    assert not torch.equal(alone[0], alone[1])


@pytest.mark.parametrize("graph", [True, False])
def test_sessions_leave_the_model_they_share_untouched(graph):
    """Hoisting is an argument of `forward_lights`, not a flag a session writes on the model and puts back: after construction
    and a run the model has no `hoist_prepass` of its own (the class default still shows through), and two sessions on ONE model
    -- a plain one and a rig -- return the eager entries' bytes on the same inputs (fixed head outputs: exactly)."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    heads = _fixed_heads(1, 12)
    net = _fixed(RelightNetSingleImage, heads)
    rng = np.random.default_rng(5)
    images = torch.from_numpy(rng.random((1, H, W, 3), dtype=np.float32)).to(DEV)
    lights = _lights11()[:3]
    rgb = rng.random((3, 3), dtype=np.float32)
    plain = inf.RelightSession(net, 1, heads[3], lights, device=DEV, graph=graph)
    rig = inf.RelightSession(net, 1, heads[3], lights, device=DEV, graph=graph, light_rgb=rgb)
    assert (plain.graph is not None) == graph and (rig.graph is not None) == graph
    got_plain, got_rig = plain.run(images).clone(), rig.run(images).clone()
    assert "hoist_prepass" not in vars(net) and net.hoist_prepass is True
    assert torch.equal(got_plain, inf.relight_lights_device(net, images, heads[3], lights, device=DEV))
    assert torch.equal(got_rig, inf.relight_rig_device(net, images, heads[3], lights, rgb, device=DEV))
    assert torch.equal(plain.run(images), got_plain)                               # the rig session in between changed nothing
    assert tuple(got_plain.shape) == (1, 3, H, W, 3) and tuple(got_rig.shape) == (1, H, W, 3) and got_rig.float().std() > 1
    assert "hoist_prepass" not in vars(net)


def test_folded_batchnorm_copy_relights_to_the_same_bytes():
    """inference.fold_batchnorm: the eval-mode BatchNorms folded into the convolutions in front of them (56 elementwise kernels
    per pass fewer).  Network outputs agree to ~1e-5 relative with the two-step evaluation, the composites on >= 99.9 % of the
    bytes (>= 99.99 % within 1); the original model is untouched and a training-mode model is refused."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "slt_checkpoint_epoch106.npz")).items()}
    net = RelightNetLightingTransfer()
    net.load_state_dict(sd, strict=True)
    net = net.float().to(DEV)
    with pytest.raises(ValueError):
        inf.fold_batchnorm(net.train())
    net = net.eval()
    folded = inf.fold_batchnorm(net)
    assert sum(isinstance(m, torch.nn.BatchNorm2d) for m in folded.modules()) == 0
    assert sum(isinstance(m, torch.nn.BatchNorm2d) for m in net.modules()) == 56          # the original keeps its BatchNorms
    za, zb = [np.load(os.path.join(GOLDEN, "slt_main_%s.npz" % t)) for t in ("a", "b")]
    images = np.stack([za["input_u8"] / 255.0, zb["input_u8"] / 255.0]).astype(np.float32)
    x = torch.from_numpy(images).to(DEV)
    with torch.no_grad():
        a, b = net.features(x, 200), folded.features(x, 200)
    for u, v in zip(a, b):
        assert float((u - v).abs().max()) <= 2e-5 * float(u.abs().max())
    lights = _lights11()
    got = inf.relight_lights(folded, images, za["mask_u8"], lights, ambient=0.5, device=DEV)
    want = inf.relight_lights(net, images, za["mask_u8"], lights, ambient=0.5, device=DEV)
    diff = np.abs(got.astype(int) - want.astype(int))
    assert (diff == 0).mean() >= 0.999 and (diff <= 1).mean() >= 0.9999, ((diff == 0).mean(), diff.max())


@pytest.mark.parametrize("L", [1, 16, 18])
def test_forward_lights_at_the_normals_stage_crossover(L):
    """From 16 lights per face on the normals stencil runs as its own launch in front of the march (block.normals_stage_for) --
    also behind a hoisted prepass.  L = 1 (a light axis of length one), 16 and 18 (BASELINE configs[4]'s count) against single
    forwards, bit for bit on fixed head outputs."""
    from geomconsistentfr_amd import block as R
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    import scenes
    B = 2
    heads = _fixed_heads(B, 5)
    net = _fixed(RelightNetSingleImage, heads)
    lights = scenes.LIGHTS18[:L]
    assert R.normals_stage_for(L) == ("kernel" if L >= 16 else "fused")
    img = torch.zeros(B, H, W, 3, device=DEV)
    mask = torch.from_numpy(heads[3].astype(np.float64) / 255.0).reshape(H, W, 1).to(DEV)
    with torch.no_grad():
        many = net.forward_lights(img, 200, _K(1570.0), mask, lights)
        assert tuple(many[5].shape) == (B, L, 3, H, W)
        for l in sorted({0, L // 2, L - 1}):
            tl = torch.from_numpy(np.repeat(lights[l][None], B, 0)).reshape(B, 3, 1, 1).to(DEV)
            one = net(img, 200, _K(1570.0), mask, tl, torch.zeros(B, 1, 1, device=DEV), mask[None])
            for k in (2, 4, 5, 6, 8):
                assert torch.equal(many[k][:, l], one[k]), (k, l)
            assert torch.equal(many[9], one[9])


def test_inference_mode_gives_the_no_grad_bytes():
    """RelightNet.forward (eval, prepass hoisted), RelightNetSingleImage.forward_lights and inference.relight_images under
    torch.inference_mode() give the bytes they give under torch.no_grad().  Every tensor made inside inference mode -- the head
    outputs the prepass signs (block.source_signature), the host camera matrix (block.camera_scalars) -- has no version counter."""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNet, RelightNetSingleImage
    B = 3
    heads = _fixed_heads(B, 21)
    train_form, single = _fixed(RelightNet, heads), _fixed(RelightNetSingleImage, heads)
    assert train_form.hoist_prepass and single.hoist_prepass
    images = np.random.default_rng(6).random((B, H, W, 3), dtype=np.float32)
    lights = _lights11()[:4]

    def run():
        img = torch.from_numpy(images).to(DEV)
        masks = torch.from_numpy(heads[3].astype(np.float64) / 255.0).reshape(1, H, W, 1).expand(B, -1, -1, -1).contiguous().to(DEV)
        K = inf.camera_matrix(1570.0, H, W)                                  # a host tensor made in the mode under test
        out = list(train_form(img, 200, K, masks))
        out += list(single.forward_lights(img, 200, K, masks[0], lights))
        out.append(torch.from_numpy(inf.relight_images(single, images, heads[3], np.repeat(lights[:1], B, 0), device=DEV)))
        return [o.cpu() for o in out]

    with torch.no_grad():
        want = run()
    with torch.inference_mode():
        got = run()
    assert len(got) == len(want) == 19
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
