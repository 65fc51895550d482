"""GPU: the non-negative rig fit (gcfr_light_fit_solve_nonneg in csrc/gcfr_light_fit.hip; lighting.fit_light_rgb(nonnegative=True);
inference.capture_rig / rig_lighting_transfer(nonnegative=True)) against its numpy f64 restatement
(tests/light_fit_nonneg_emulation.py, itself held to a KKT certificate, a brute force over all supports and scipy's nnls by
tests/test_light_fit_nonneg_host.py).

  bits         rgb, info and solves BIT-EQUAL to the restatement for ridge 0 and 1e-3: from pixels at the shapes of
               light_fit_nonneg_emulation.PIXEL_SHAPES (the last with one weight and one rig shared by three faces), from Gram matrices
               of the mixed-sign family handed straight to the C entry at L = 1, 2, 5, 64, and on the all-negative right-hand side,
               the cap of one factorisation and the NaN in rhs
  properties   every entry >= 0; where the unconstrained fit is positive everywhere the two entries return the same bits; the
               objective of the non-negative rig, evaluated over the pixels in numpy f64, is <= that of the unconstrained rig clamped at 0
  round trip   combine_lights of a rig with exact zeros -> fit_light_rgb(nonnegative=True) returns it within the host test's gate
  serving      `out=` refills a captured RelightSession between replays; the entry runs inside a stream capture; two calls and a
               side stream return the same bits; rig_lighting_transfer(nonnegative=True) equals relight_rig_device under
               capture_rig(nonnegative=True) byte for byte on fixed head outputs
  refusals     the C entry rejects NULLs, misalignment, max_solves < 0 and a bad rgb_batch without a launch; Python raises before one"""
import numpy as np
import pytest
import torch

import light_fit_emulation as lfe
import light_fit_nonneg_emulation as emu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _c_entry(gram, rhs, ridge, rigs, max_solves=0):
    """gcfr_light_fit_solve_nonneg itself on host arrays -> (rgb, info, solves) as numpy; rgb and the counts start as a sentinel"""
    from geomconsistentfr_amd import _lib
    B, _, L, _ = gram.shape
    g, r = _dev(gram), _dev(rhs)
    rgb = torch.full((rigs, L, 3), -7.0, device=DEV)
    info = torch.full((rigs, 3), 99, dtype=torch.int32, device=DEV)
    solves = torch.full((rigs, 3), 99, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().gcfr_light_fit_solve_nonneg(g.data_ptr(), r.data_ptr(), B, L, ridge, rigs, max_solves, rgb.data_ptr(),
                                                       info.data_ptr(), solves.data_ptr(), _lib.stream_ptr(DEV)), "gcfr_light_fit_solve_nonneg")
    torch.cuda.synchronize(DEV)
    return rgb.cpu().numpy(), info.cpu().numpy(), solves.cpu().numpy()


def _assert_equal(got, want, what):
    rgb, info, solves = got
    w_rgb, w_info, w_solves = want[:3]
    nan = np.isnan(w_rgb)
    print("%s: f32 entries that differ %d of %d, info %s (want %s), solves %s (want %s)"
          % (what, int((rgb.view(np.uint32) != w_rgb.view(np.uint32))[~nan].sum()), rgb.size, info.ravel().tolist(), w_info.ravel().tolist(),
             solves.ravel().tolist(), w_solves.ravel().tolist()))
    assert rgb.shape == w_rgb.shape and rgb.dtype == np.float32 and info.dtype == solves.dtype == np.int32
    assert np.array_equal(info, w_info) and np.array_equal(solves, w_solves)
    assert np.array_equal(np.isnan(rgb), nan) and np.array_equal(rgb.view(np.uint32)[~nan], w_rgb.view(np.uint32)[~nan])
    assert not np.signbit(rgb[~nan]).any()                                            # >= 0, and a zero is +0


def _objective(final, albedo, image, w, ridge, gram, shared, rgb):
    """sum_p w (I_c - a_c sum_l x f_l)^2 + ridge trace(G_c) / L |x_c|^2 over the pixels, numpy f64, summed over rigs and channels"""
    B, L, H, W = final.shape
    f = final.reshape(B, L, -1).astype(np.float64)
    a = albedo.reshape(B, 3, -1).astype(np.float64)
    im = image.reshape(B, -1, 3).transpose(0, 2, 1).astype(np.float64)
    wt = np.broadcast_to(w.reshape(w.shape[0], -1).astype(np.float64), (B, H * W))
    x = np.broadcast_to(rgb.astype(np.float64), (B, L, 3))
    res = im - a * np.einsum("blc,blp->bcp", x, f)
    G = gram.sum(axis=0, keepdims=True) if shared else gram
    shift = ridge * np.trace(G, axis1=2, axis2=3) / L                                 # (rigs,3)
    return float((wt[:, None] * res ** 2).sum() + (shift * (rgb.astype(np.float64) ** 2).sum(axis=1)).sum())


@pytest.mark.parametrize("ridge", emu.RIDGES)
@pytest.mark.parametrize("key", emu.PIXEL_SHAPES)
def test_from_pixels_rgb_info_and_solves_equal_the_restatement_bit_for_bit(key, ridge):
    from geomconsistentfr_amd import fit_light_rgb
    B, L, H, W, shared = key
    final, albedo, image, w, gram, rhs = emu.pixel_case(*key)
    want = emu.solved("pixels", key, ridge)
    args = [_dev(a) for a in (final, albedo, image, w)]
    rgb, info, solves = fit_light_rgb(*args, ridge=ridge, shared=shared, nonnegative=True, return_info=True)
    assert rgb.is_cuda and info.is_cuda and solves.is_cuda and tuple(solves.shape) == ((1 if shared else B), 3)
    got = (rgb.cpu().numpy(), info.cpu().numpy(), solves.cpu().numpy())
    _assert_equal(got, want, "%s ridge %g" % (key, ridge))
    assert (got[0] >= 0).all() and (got[1] == 0).all()
    # against the unconstrained fit of the same call
    free = fit_light_rgb(*args, ridge=ridge, shared=shared).cpu().numpy()
    f_nonneg = _objective(final, albedo, image, w, ridge, gram, shared, got[0])
    f_clamped = _objective(final, albedo, image, w, ridge, gram, shared, np.maximum(free, 0))
    print("    unconstrained: %d of %d entries negative; objective non-negative %.9g, unconstrained clamped at 0 %.9g"
          % (int((free < 0).sum()), free.size, f_nonneg, f_clamped))
    assert f_nonneg <= f_clamped
    for rig in range(free.shape[0]):
        for c in range(3):
            if (free[rig, :, c] > 0).all():
                assert np.array_equal(free[rig, :, c].view(np.uint32), got[0][rig, :, c].view(np.uint32)), (rig, c)
    if L >= 63:
        assert (free < 0).any() and (got[0] == 0).any()


@pytest.mark.parametrize("ridge", emu.RIDGES)
@pytest.mark.parametrize("L", emu.GRAM_LIGHTS)
def test_from_gram_matrices_of_the_mixed_sign_family(L, ridge):
    gram, rhs = emu.gram_case(L)[3:]
    want = emu.solved("gram", L, ridge)
    got = _c_entry(gram, rhs, ridge, gram.shape[0])
    _assert_equal(got, want, "gram L = %d ridge %g" % (L, ridge))
    assert (got[0] == 0).any() and (got[1] == 0).all()                                # the family's fits have excluded lights


def test_the_all_negative_right_hand_side_the_cap_of_one_and_the_nan():
    gram, rhs = emu.all_negative_rhs()
    got = _c_entry(gram, rhs, 1e-3, 2)
    _assert_equal(got, emu.solve(gram, rhs, 1e-3, False), "all-negative r")
    assert (got[0] == 0).all() and (got[2] == 0).all()
    gram, rhs = emu.gram_case(5)[3:]
    got = _c_entry(gram, rhs, 1e-3, 2, max_solves=1)
    _assert_equal(got, emu.solve(gram, rhs, 1e-3, False, max_solves=1), "max_solves = 1")
    assert (got[1] == -1).all() and (got[2] == 1).all() and (got[0] >= 0).all()
    gram, rhs = emu.one_nan_in_rhs()
    got = _c_entry(gram, rhs, 1e-3, 2)
    _assert_equal(got, emu.solve(gram, rhs, 1e-3, False), "one NaN in rhs")
    assert (got[1] == 0).all() and np.isfinite(got[0]).all() and got[0][0, 2, 1] == 0
    # solves = NULL is allowed; a singular channel reports the LIGHT whose pivot failed
    from geomconsistentfr_amd import _lib
    g = np.zeros((1, 3, 3, 3))
    g[0, :] = np.diag([1.0, 0.0, 1.0])
    r = np.ones((1, 3, 3))
    tg, tr = _dev(g), _dev(r)
    rgb, info = torch.zeros(1, 3, 3, device=DEV), torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    assert _lib.load().gcfr_light_fit_solve_nonneg(tg.data_ptr(), tr.data_ptr(), 1, 3, 0.0, 1, 0, rgb.data_ptr(), info.data_ptr(), None,
                                                   _lib.stream_ptr(DEV)) == 0
    torch.cuda.synchronize(DEV)
    w_rgb, w_info, _s, _x, _c = emu.solve(g, r, 0.0, False)
    assert (w_info == 2).all() and np.array_equal(info.cpu().numpy(), w_info) and torch.isnan(rgb).all() and np.isnan(w_rgb).all()


@pytest.mark.parametrize("B,L,H,W", [(2, 5, 21, 37), (1, 64, 33, 47)])
def test_a_positive_unconstrained_fit_comes_back_in_its_own_bits(B, L, H, W):
    from geomconsistentfr_amd import fit_light_rgb
    x_true = np.random.default_rng(11).uniform(0.2, 1.0, (B, L, 3))
    final, albedo, image, w = lfe.make_inputs(600 + L, B, L, H, W, "mask", x_true=x_true)
    args = [_dev(a) for a in (final, albedo, image, w)]
    for ridge in emu.RIDGES:
        free, free_info = fit_light_rgb(*args, ridge=ridge, return_info=True)
        rgb, info, solves = fit_light_rgb(*args, ridge=ridge, nonnegative=True, return_info=True)
        print("(%d,%d,%d,%d) ridge %g: solves %s" % (B, L, H, W, ridge, solves.cpu().numpy().ravel().tolist()))
        assert (free > 0).all() and (free_info == 0).all() and (info == 0).all() and (solves >= L).all()
        assert np.array_equal(_bits(free), _bits(rgb))


@pytest.mark.parametrize("B,L,H,W", [(2, 5, 21, 37), (1, 64, 33, 47)])
def test_round_trip_of_a_rig_with_exact_zeros_through_the_rig_stage(B, L, H, W):
    from geomconsistentfr_amd import combine_lights, fit_light_rgb
    rgb_true = emu.sparse_rig(300 + L, B, L)
    final, albedo, _im, _w = lfe.make_inputs(400 + L, B, L, H, W, None)
    tf, ta = _dev(final), _dev(albedo)
    rendered, _ = combine_lights(tf, ta, _dev(rgb_true))
    image = rendered.permute(0, 2, 3, 1).contiguous()
    got, info, solves = fit_light_rgb(tf, ta, image, ridge=0.0, nonnegative=True, return_info=True)
    got = got.cpu().numpy()
    err = float(np.abs(got - rgb_true).max() / np.abs(rgb_true).max())
    print("(%d,%d,%d,%d): %d of %d true zeros, %d returned; |x - rgb_true| / max|rgb_true| = %.3g (gate %.3g); solves %s"
          % (B, L, H, W, int((rgb_true == 0).sum()), rgb_true.size, int((got == 0).sum()), err, emu.GATE_RECOVERY,
             solves.cpu().numpy().ravel().tolist()))
    assert (rgb_true == 0).any() and (info == 0).all() and (got >= 0).all() and err <= emu.GATE_RECOVERY


def test_two_calls_and_a_side_stream_return_the_same_bits():
    from geomconsistentfr_amd import fit_light_rgb
    key = (1, 64, 33, 47, False)
    args = [_dev(a) for a in emu.pixel_case(*key)[:4]]
    first = fit_light_rgb(*args, nonnegative=True, return_info=True)
    again = fit_light_rgb(*args, nonnegative=True, return_info=True)
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = fit_light_rgb(*args, nonnegative=True, return_info=True)
    side.synchronize()
    for t in (again, other):
        assert np.array_equal(_bits(first[0]), _bits(t[0])) and torch.equal(first[1], t[1]) and torch.equal(first[2], t[2])
    assert (first[1] == 0).all() and (first[0] == 0).any() and (first[0] >= 0).all()


def test_the_entry_runs_inside_a_stream_capture():
    from geomconsistentfr_amd import fit_light_rgb
    key = (1, 64, 33, 47, False)
    args = [_dev(a) for a in emu.pixel_case(*key)[:4]]
    eager = fit_light_rgb(*args, nonnegative=True, return_info=True)                  # (also loads the library outside the capture)
    torch.cuda.synchronize(DEV)
    buf = torch.full((1, 64, 3), float("nan"), device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ret, info, solves = fit_light_rgb(*args, out=buf, nonnegative=True, return_info=True)
    buf.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert ret.data_ptr() == buf.data_ptr()
    assert np.array_equal(_bits(buf), _bits(eager[0])) and torch.equal(info, eager[1]) and torch.equal(solves, eager[2])
    # new data in the static inputs reaches the replay
    args[2].copy_(torch.from_numpy(np.random.default_rng(10).random((1, 33, 47, 3), dtype=np.float32)))
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert np.array_equal(_bits(buf), _bits(fit_light_rgb(*args, nonnegative=True))) and not torch.equal(buf, eager[0])


def test_out_refills_a_captured_session_without_recapture():
    from geomconsistentfr_amd import fit_light_rgb
    from geomconsistentfr_amd import inference as inf
    from test_gpu_light_rig import _fixed_net
    B, S = 2, 64
    net, mask_u8 = _fixed_net(B, S)
    images = np.random.default_rng(4).random((B, S, S, 3), dtype=np.float32)
    lights = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)
    sess = inf.RelightSession(net, B, mask_u8, lights, device=DEV, H=S, W=S, light_rgb=torch.zeros(B, 3, 3, device=DEV))
    assert sess.graph is not None
    ptr = sess.light_rgb.data_ptr()
    seen = []
    for seed in (1, 2):
        photo = torch.from_numpy(np.random.default_rng(seed).random((B, S, S, 3), dtype=np.float32)).to(DEV)
        out, cm, _t = inf._lights_pass(net, photo, mask_u8, lights, 0.5, None, DEV, None, 200)
        ret = fit_light_rgb(out[8], out[0], photo, weight=cm, out=sess.light_rgb, nonnegative=True)
        assert ret.data_ptr() == ptr and sess.light_rgb.data_ptr() == ptr
        fresh = inf.capture_rig(net, photo, mask_u8, lights, device=DEV, nonnegative=True)
        assert fresh.data_ptr() != ptr and torch.equal(fresh, sess.light_rgb) and (fresh >= 0).all()
        got = sess.run(torch.from_numpy(images))
        want = inf.relight_rig_device(net, images, mask_u8, lights, fresh, device=DEV)
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        seen.append(got.cpu().numpy())
    assert np.abs(seen[0].astype(int) - seen[1].astype(int)).max() > 0


def test_rig_lighting_transfer_is_relight_rig_under_the_captured_non_negative_rig():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import sphere_directions
    from test_gpu_light_fit import _shipped_transfer_net
    net, photos, mask_u8 = _shipped_transfer_net()
    refs, inputs = photos, photos[::-1].copy()
    B, H, W, _ = photos.shape
    L = 24                                                                            # close lights: the unconstrained rig has negative entries
    lights = sphere_directions(L, 0.3)
    free = inf.capture_rig(net, refs, mask_u8, lights, device=DEV)
    rgb = inf.capture_rig(net, refs, mask_u8, lights, device=DEV, nonnegative=True)
    print("captured rigs, %d lights: unconstrained %d of %d entries negative; non-negative %d zero" % (L, int((free < 0).sum()), free.numel(), int((rgb == 0).sum())))
    assert tuple(rgb.shape) == (B, L, 3) and rgb.dtype == torch.float32 and rgb.is_cuda and (rgb >= 0).all()
    assert torch.equal(inf.capture_rig(net, refs, mask_u8, lights, device=DEV, nonnegative=False), free)
    got = inf.rig_lighting_transfer(net, inputs, refs, mask_u8, lights, device=DEV, nonnegative=True)
    assert tuple(got.shape) == (B, H, W, 3) and got.dtype == torch.uint8
    assert torch.equal(got, inf.relight_rig_device(net, inputs, mask_u8, lights, rgb, device=DEV))
    shared = inf.capture_rig(net, refs, mask_u8, lights, shared=True, device=DEV, nonnegative=True)
    assert tuple(shared.shape) == (1, L, 3) and (shared >= 0).all()
    one = inf.rig_lighting_transfer(net, inputs, refs, mask_u8, lights, shared=True, device=DEV, nonnegative=True)
    assert torch.equal(one, inf.relight_rig_device(net, inputs, mask_u8, lights, shared, device=DEV))


def test_bad_arguments_are_refused_without_a_launch():
    from geomconsistentfr_amd import _lib, fit_light_rgb
    lib = _lib.load()
    f = torch.full((64,), -7.0, device=DEV)
    d = torch.ones(4096, dtype=torch.float64, device=DEV)
    i = torch.full((16,), 99, dtype=torch.int32, device=DEV)
    p, q, n = f.data_ptr(), d.data_ptr(), i.data_ptr()
    solve = lambda L=3, ridge=1e-3, gram=q, rhs=q, rigs=2, cap=0, rgb=p, info=n: lib.gcfr_light_fit_solve_nonneg(
        gram, rhs, 2, L, ridge, rigs, cap, rgb, info, n + 32, None)
    assert solve(L=65) == -1 and solve(L=0) == -1 and solve(ridge=-1.0) == -1 and solve(ridge=float("nan")) == -1
    assert solve(gram=None) == -1 and solve(rhs=None) == -1 and solve(rgb=None) == -1 and solve(info=None) == -1
    assert solve(gram=q + 4) == -1 and solve(rhs=q + 4) == -1 and solve(cap=-1) == -1 and solve(rigs=3) == -1 and solve(rigs=0) == -1
    args = [torch.rand(2, 3, 4, 5, device=DEV), torch.rand(2, 3, 4, 5, device=DEV), torch.rand(2, 4, 5, 3, device=DEV)]
    out = torch.full((2, 3, 3), -7.0, device=DEV)
    for bad in (-1, 2.5, None):
        with pytest.raises(_lib.GcfrError):
            fit_light_rgb(*args, out=out, nonnegative=True, max_solves=bad)
    torch.cuda.synchronize(DEV)
    assert (f == -7.0).all() and (i == 99).all() and (out == -7.0).all()
