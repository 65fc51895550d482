"""GPU: the forward's two launches as two enqueues (gcfr_options.phase, round 5): the prepass issued early on a side stream
(`block.render_prepass` / `RenderFwdPlan.capture_split` / `RelightNet.forward`'s hook behind the depth decoder) and the march
behind it must give the bits of the one-call form -- they are the same two launches with the same arguments."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _inputs(B=3, L=2, H=96, W=128, seed=5):
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:H, 0:W]
    depth = (30 * np.exp(-(((c - 60) / 30.0) ** 2 + ((r - 50) / 35.0) ** 2)) + rng.random((B, H, W))).astype(np.float32)
    mask = (((c - 64) / 50.0) ** 2 + ((r - 48) / 40.0) ** 2 < 1).astype(np.uint8)[None].repeat(B, 0)
    mask[1] = (rng.random((H, W)) > 0.3)
    light = rng.standard_normal((B, L, 3)).astype(np.float32)
    amb = (0.3 + 0.4 * rng.random((B, L))).astype(np.float32)
    nrm = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    alb = rng.random((B, 3, H, W)).astype(np.float32)
    return [torch.from_numpy(t).to(DEV) for t in (depth, mask, light, amb, nrm, alb)]


@pytest.mark.parametrize("from_depth", [False, True])
@pytest.mark.parametrize("pixels", ["all", "mask"])
def test_prepass_then_march_equals_the_one_call_form(from_depth, pixels):
    from geomconsistentfr_amd import RenderParams
    from geomconsistentfr_amd import block as R
    depth, mask, light, amb, nrm, alb = _inputs()
    prm = RenderParams(n_samples=64, dt=0.0125, pixels=pixels)
    cam = (1570.0, 1570.0, 64.0, 48.0, 1610.0) if from_depth else None
    ref = R.render_fwd(depth, mask, light, amb, None if from_depth else nrm, alb, prm, want_argmin=True, camera=cam)
    pre = R.render_prepass(depth, mask, light, prm, want_argmin=True)
    # work on the main stream between the two halves (what the albedo decoder is in RelightNet.forward)
    junk = torch.randn(512, 512, device=DEV)
    for _ in range(4):
        junk = junk @ junk * 1e-3
    out = R.render_fwd(depth, mask, light, amb, None if from_depth else nrm, alb, prm, want_argmin=True, camera=cam, prepared=pre)
    torch.cuda.synchronize()
    for k, v in ref.items():
        if v is not None:
            assert torch.equal(out[k], v), k
    # a march issued with other parameters than its prepass is refused, not run on a stale workspace
    from geomconsistentfr_amd._lib import GcfrError
    with pytest.raises(GcfrError):
        R.render_fwd(depth, mask, light, amb, None if from_depth else nrm, alb, RenderParams(n_samples=32, dt=0.025, pixels=pixels),
                     want_argmin=True, camera=cam, prepared=pre)


def test_plan_split_graphs_replay_the_one_graph_bits():
    from geomconsistentfr_amd import RenderParams
    from geomconsistentfr_amd import block as R
    depth, mask, light, amb, nrm, alb = _inputs(B=4, L=1, H=128, W=128, seed=9)
    prm = RenderParams(n_samples=80, dt=0.01)
    cam = (1570.0, 1570.0, 64.0, 64.0, 1610.0)
    one = R.RenderFwdPlan(4, 1, 128, 128, prm, DEV, want_argmin=True, camera=cam).capture(depth, mask, light, amb, None, alb)
    ref = {k: v.clone() for k, v in one.replay().items() if v is not None}
    two = R.RenderFwdPlan(4, 1, 128, 128, prm, DEV, want_argmin=True, camera=cam).capture_split(depth, mask, light, amb, None, alb)
    for v in two.out.values():
        if v is not None:
            v.zero_()
    two.ws.zero_()
    side, main = torch.cuda.Stream(device=DEV), torch.cuda.current_stream(DEV)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        two.replay_prepass()
        ev = torch.cuda.Event()
        ev.record(side)
    main.wait_event(ev)
    out = two.replay_march()
    torch.cuda.synchronize()
    for k, v in ref.items():
        assert torch.equal(out[k], v), k
    # the march alone again on the prepared workspace (it only reads it): the same bits -- what bench.py times as the latency
    # of one batch with the prepass pre-issued
    out["minimum_distance"].zero_()
    two.replay_march()
    torch.cuda.synchronize()
    assert torch.equal(out["minimum_distance"], ref["minimum_distance"])


def test_relightnet_forward_with_the_prepass_hoisted_equals_the_serial_forward_and_backward():
    """RelightNet.forward puts the prepass on the side stream as soon as the depth decoder is done.  The convolutions in front
    are MIOpen's (not run-to-run reproducible), so the two forms are compared on FIXED head outputs: a subclass whose
    features() returns given tensors and fires the hook the way the real one does."""
    from geomconsistentfr_amd.relightnet import RelightNet
    rng = np.random.default_rng(21)
    B = 2
    r, c = np.mgrid[0:256, 0:256]
    d0 = (60 * np.exp(-(((c - 128) / 60.0) ** 2 + ((r - 120) / 70.0) ** 2)) + 2 * rng.random((B, 1, 256, 256))).astype(np.float32)
    a0 = rng.random((B, 3, 256, 256)).astype(np.float32)
    sl0 = np.array([[[[0.5, 0.3, 0.4, 0.8]]], [[[0.4, -0.5, 0.2, 0.7]]]], np.float32)
    masks = torch.from_numpy(((((c - 128) / 90.0) ** 2 + ((r - 128) / 110.0) ** 2) < 1).astype(np.float32)[None].repeat(B, 0)).to(DEV)
    K = torch.zeros(1, 3, 3, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = 1570.0
    K[:, 2, 2] = 1.0
    K[:, 0, 2] = K[:, 1, 2] = 128.0

    class Fixed(RelightNet):
        def features(self, img, epoch, on_depth=None):
            self.leaves = [torch.from_numpy(x).to(DEV).requires_grad_() for x in (a0, d0, sl0)]
            albedo, depth, SL = self.leaves
            if on_depth is not None:
                on_depth(depth, SL)
            return albedo, depth, SL

    img = torch.zeros(B, 256, 256, 3, device=DEV)
    res = {}
    for hoist in (False, True):
        net = Fixed().to(DEV)
        net.hoist_prepass = hoist
        out = net(img, 200, K, masks)
        loss = (out[5] * masks[:, None]).sum() + out[2].sum() * 0.1
        loss.backward()
        torch.cuda.synchronize()
        res[hoist] = ([o.detach().clone() for o in out], [leaf.grad.clone() for leaf in net.leaves])
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b)
    # gradients: the backward's atomics make grad_depth order-dependent in the last bits; albedo's gradient is a plain store
    assert torch.equal(res[False][1][0], res[True][1][0])
    g0, g1 = res[False][1][1], res[True][1][1]
    assert float((g0 - g1).abs().max()) <= 1e-5 * float(g0.abs().max())
    assert float(g0.abs().max()) > 0


def test_phase_one_needs_no_albedo_and_phase_two_needs_its_operands():
    from geomconsistentfr_amd import RenderParams, _lib
    from geomconsistentfr_amd import block as R
    L_ = _lib.load()
    depth, mask, light, amb, nrm, alb = _inputs(B=2, L=1, H=64, W=64)
    prm = RenderParams(n_samples=32, dt=0.025)
    tt = R.sample_table(prm, DEV)
    unit, pt = torch.empty(2, 1, 3, device=DEV), torch.empty(2, 1, 3, device=DEV)
    ws_bytes = int(L_.gcfr_shadow_workspace_bytes(2, 64, 64))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def call(phase, albedo_ptr):
        return L_.gcfr_render_from_depth_fwd(light.data_ptr(), 1, 0.0, 4013.0, depth.data_ptr(), mask.data_ptr(), 2, 1570.0, 1570.0, 32.0, 32.0,
                                             1610.0, 1, albedo_ptr, None, 2, 1, 64, 64, 32, tt.data_ptr(), 0.0, None, 0.5, unit.data_ptr(),
                                             pt.data_ptr(), None, None, None, None, None, None, None, ws.data_ptr(), ws_bytes, None,
                                             ctypes.byref(_lib.options(phase=phase)))
    assert call(1, None) == 0                     # the prepass: depth, mask, light, table
    assert call(2, None) == -1 and call(0, None) == -1
    torch.cuda.synchronize()
    _, pt_ref = R.light_prep(light, prm)
    assert torch.equal(pt, pt_ref)


def test_a_stale_prepared_is_refused_not_rendered():
    """Round-5 advisor finding: render_fwd(prepared=...) used to substitute the prepass's own tensors BEFORE comparing, so a
    Prepared built from other (or since overwritten) depth / light of the same shapes rendered the old data without an error
    and autograd returned gradients for the wrong input.  The caller's tensors are now compared with the prepass's record
    (address, in-place version, shape, strides, dtype)."""
    from geomconsistentfr_amd import RenderParams
    from geomconsistentfr_amd import block as R
    from geomconsistentfr_amd._lib import GcfrError
    depth, mask, light, amb, nrm, alb = _inputs()
    prm = RenderParams(n_samples=64, dt=0.0125)
    cam = (1570.0, 1570.0, 64.0, 48.0, 1610.0)
    kw = dict(want_argmin=True, camera=cam)
    pre = R.render_prepass(depth, mask, light, prm, want_argmin=True)
    with pytest.raises(GcfrError):                                            # another depth tensor of the same shape
        R.render_fwd(depth.clone(), mask, light, amb, None, alb, prm, prepared=pre, **kw)
    with pytest.raises(GcfrError):                                            # another light
        R.render_fwd(depth, mask, light + 0.1, amb, None, alb, prm, prepared=pre, **kw)
    with pytest.raises(GcfrError):                                            # another mask
        R.render_fwd(depth, 1 - mask, light, amb, None, alb, prm, prepared=pre, **kw)
    ok = R.render_fwd(depth, mask, light, amb, None, alb, prm, prepared=pre, **kw)      # the very tensors: accepted
    ok = {k: v.clone() for k, v in ok.items() if v is not None}
    original = depth.clone()
    depth.add_(1.0)                                                           # written in place since the prepass
    with pytest.raises(GcfrError):
        R.render_fwd(depth, mask, light, amb, None, alb, prm, prepared=pre, **kw)
    torch.cuda.synchronize()
    depth.copy_(original)
    ref = R.render_fwd(depth, mask, light, amb, None, alb, prm, **kw)
    assert torch.equal(ok["rendered_images"], ref["rendered_images"])
    # the differentiable wrapper: the same check, through render_from_depth_prepass / render_from_depth
    K = torch.zeros(1, 3, 3, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = 1570.0
    K[:, 2, 2] = 1.0
    K[:, 0, 2], K[:, 1, 2] = 64.0, 48.0
    d4 = depth[:, None].clone().requires_grad_()
    l2 = light[:, 0].clone().requires_grad_()
    pre = R.render_from_depth_prepass(d4, l2, K, mask, prm)
    with pytest.raises(GcfrError):
        R.render_from_depth(d4.detach().clone().requires_grad_(), alb, l2, amb[:, 0], K, 1610.0, mask, prm, prepared=pre)
    r = R.render_from_depth(d4, alb, l2, amb[:, 0], K, 1610.0, mask, prm, prepared=pre)
    r["rendered_images"].sum().backward()
    r2 = R.render_from_depth(d4.detach(), alb, l2.detach(), amb[:, 0], K, 1610.0, mask, prm)
    assert torch.equal(r["rendered_images"], r2["rendered_images"]) and float(d4.grad.abs().max()) > 0


@pytest.mark.parametrize("L", [1, 16])
def test_every_form_of_the_forward_issues_the_one_call_bits(L):
    """One marshalling path (block._Forward) behind render_fwd, render_prepass and RenderFwdPlan: every form is the same
    launches with the same arguments, so every output equals the one-call form's bit for bit -- at a shape whose last
    16 x 4 tiles are ragged, with the normals stage fused (L = 1) and as its own launch (L = 16, and forced at L = 1).  The
    one-call form's minimum distance is held to the C oracle on face 0, so that six identically wrong forms do not pass."""
    import c_oracle
    from geomconsistentfr_amd import RenderParams
    from geomconsistentfr_amd import block as R
    B, H, W = 2, 20, 36
    depth, mask, light, amb, _, alb = _inputs(B=B, L=L, H=H, W=W)
    prm = RenderParams(n_samples=24, dt=0.03)
    cam = (1570.0, 1570.0, 18.0, 10.0, 1610.0)
    args = (depth, mask, light, amb, None, alb)
    assert R.normals_stage_for(L) == ("kernel" if L == 16 else "fused")
    ref = R.render_fwd(*args, prm, want_argmin=True, camera=cam)                                          # (a)
    ref = {k: v.clone() for k, v in ref.items() if v is not None}
    assert set(ref) == {"unit_light_direction", "light_pt", "minimum_distance", "argmin", "shadow_mask_weights", "full_shading",
                        "final_shading", "rendered_images", "surface_normals"}
    plan = lambda **kw: R.RenderFwdPlan(B, L, H, W, prm, DEV, want_argmin=True, camera=cam, **kw)

    def same(name, out):
        torch.cuda.synchronize()
        for k, v in ref.items():
            assert torch.equal(out[k], v), (name, k)

    pre = R.render_prepass(depth, mask, light, prm, want_argmin=True)
    same("prepass, then march", R.render_fwd(*args, prm, want_argmin=True, camera=cam, prepared=pre))    # (b)
    p = plan()
    same("plan, eager", p(*args))                                                                         # (c)
    same("plan, one graph", p.capture(*args).replay())                                                    # (d)
    two = plan().capture_split(*args)                                                                     # (e)
    for v in list(two.out.values()) + [two.ws]:
        if v is not None:
            v.zero_()
    two.replay_prepass()
    same("plan, two graphs", two.replay_march())
    if L == 1:
        k = plan(normals_stage="kernel")                                                                  # (f)
        assert k.normals_stage == "kernel"
        same("plan, normals stage as its own launch", k(*args))
    _, pt_o = c_oracle.light_prep(light[0].cpu().numpy(), clamp_z_min=0.0)
    md_o, _ = c_oracle.shadow_min_distance(depth[:1].cpu().numpy(), mask[:1].cpu().numpy(), pt_o.reshape(1, L, 3),
                                           c_oracle.sample_table(prm.t0, prm.dt, prm.n_samples))
    assert np.array_equal(ref["minimum_distance"][:1].cpu().numpy(), md_o)
