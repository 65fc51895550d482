"""GPU: rig capture (csrc/gcfr_light_fit.hip; lighting.light_normal_equations / fit_light_rgb; inference.capture_rig /
rig_lighting_transfer) against its numpy f64 restatement (tests/light_fit_emulation.py, itself held to numpy's SVD least squares by
tests/test_light_fit_host.py) and against the rig paths that are already pinned.

  normal equations   gram and rhs BIT-EQUAL to the restatement at every shape of light_fit_emulation.SHAPES, for weights {0,1}, k / 255
                     (given as u8) and none, both image layouts, and with non-finite pixels under a weight of 0; gram exactly
                     symmetric; two calls and a side stream return the same bits
  solve              info = 0 and ||A x - r||_2 <= 2^-23 ||A||_F ||x||_2 in numpy f64 (DERIVED: rounding x to f32 moves each entry
                     by 2^-24 relative at the most, so the residual by ||A|| ||dx|| at the most; the factor two is the margin; the
                     f64 factorisation's own error is eight orders below); the solution within the host test's gate of the
                     restatement's; a shared rig = the solve of the summed system; singular systems reported through info
  round trip         combine_lights -> fit_light_rgb returns the rig within the host test's recovery gate
  serving            `out=` into a captured RelightSession's light_rgb changes the next replay without recapture; the entries run
                     inside a stream capture and the replay returns the eager bits; rig_lighting_transfer equals relight_rig_device
                     under capture_rig's rig byte for byte on the shipped lighting-transfer checkpoint's recorded head outputs"""
import ctypes
import os

import numpy as np
import pytest
import torch

import light_fit_emulation as emu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _dev(a, misalign=False):
    """a device tensor of `a`; misalign: its first element sits 4 bytes past a 16-byte boundary"""
    if a is None:
        return None
    if not misalign:
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _geometry(B, H, W):
    from geomconsistentfr_amd.lighting import light_fit_geometry
    return light_fit_geometry(B, H, W)


def _same_bits(a, b):
    """f64 arrays: the same shape and bits, except that a NaN equals a NaN of any sign and payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(nan, np.isnan(b)) \
        and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def _gpu_normal(final, albedo, image, weight, layout="nhwc", misalign=False):
    from geomconsistentfr_amd import light_normal_equations
    img = image if layout == "nhwc" else np.ascontiguousarray(image.transpose(0, 3, 1, 2))
    gram, rhs = light_normal_equations(_dev(final, misalign), _dev(albedo, misalign), _dev(img, misalign), _dev(weight), image_layout=layout)
    assert gram.dtype == rhs.dtype == torch.float64
    return gram.cpu().numpy(), rhs.cpu().numpy()


def _as_u8(w):
    return np.rint(w.astype(np.float64) * 255.0).astype(np.uint8)


@pytest.mark.parametrize("B,L,H,W,shared_w", emu.SHAPES)
def test_gram_and_rhs_equal_the_restatement_bit_for_bit(B, L, H, W, shared_w):
    chunk, groups = _geometry(B, H, W)
    for kind in ("mask", "u8", None):
        final, albedo, image, w = emu.make_inputs(7 * L + W, B, L, H, W, "ones" if (kind == "mask" and H * W == 1) else kind,
                                                  shared_weight=shared_w)
        want_g, want_r = emu.normal_equations(final, albedo, image, w, True, chunk, groups)
        for layout in ("nhwc", "nchw"):
            given = _as_u8(w) if kind == "u8" else w                                  # k / 255: handed over as the u8 mask itself
            got_g, got_r = _gpu_normal(final, albedo, image, given, layout, misalign=(H * W) % 4 != 0)
            dg, dr = int((got_g != want_g).sum()), int((got_r != want_r).sum())
            print("(%d,%d,%d,%d) groups %d weight %s %s: gram entries that differ %d of %d, rhs %d of %d"
                  % (B, L, H, W, groups, kind, layout, dg, want_g.size, dr, want_r.size))
            assert got_g.shape == (B, 3, L, L) and got_r.shape == (B, 3, L)
            assert _same_bits(got_g, want_g) and _same_bits(got_r, want_r), (kind, layout)
            assert np.array_equal(got_g, got_g.transpose(0, 1, 3, 2))
            if kind != "mask" or H * W > 1:
                assert np.abs(got_g).max() > 0


def test_non_finite_pixels_under_a_weight_of_zero_reach_exactly_their_entries():
    B, L, H, W = 2, 5, 21, 37
    final, albedo, image, w = emu.make_inputs(3, B, L, H, W, "mask")
    chunk, groups = _geometry(B, H, W)
    w[1, 4, 9] = w[0, 11, 30] = 0.0
    image[1, 4, 9, 2] = np.nan                                                    # -> rhs[1, 2, :]
    final[0, 3, 11, 30] = np.nan                                                  # -> gram[0, :, 3, :], gram[0, :, :, 3], rhs[0, :, 3]
    want_g, want_r = emu.normal_equations(final, albedo, image, w, True, chunk, groups)
    got_g, got_r = _gpu_normal(final, albedo, image, w)
    assert _same_bits(got_g, want_g) and _same_bits(got_r, want_r)
    nan_g = np.zeros((B, 3, L, L), bool)
    nan_g[0, :, 3, :] = nan_g[0, :, :, 3] = True
    nan_r = np.zeros((B, 3, L), bool)
    nan_r[1, 2, :] = nan_r[0, :, 3] = True
    assert np.array_equal(np.isnan(got_g), nan_g) and np.array_equal(np.isnan(got_r), nan_r)


def test_two_calls_and_a_side_stream_return_the_same_bits():
    from geomconsistentfr_amd import fit_light_rgb
    B, L, H, W = 2, 11, 40, 56
    final, albedo, image, w = emu.make_inputs(4, B, L, H, W, "u8")
    args = [_dev(a) for a in (final, albedo, image, w)]
    first = fit_light_rgb(*args, return_info=True)
    again = fit_light_rgb(*args, return_info=True)
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = fit_light_rgb(*args, return_info=True)
    side.synchronize()
    for t in (again, other):
        assert torch.equal(first[0].view(torch.int32), t[0].view(torch.int32)) and torch.equal(first[1], t[1])
    assert (first[1] == 0).all() and tuple(first[0].shape) == (B, L, 3) and first[0].dtype == torch.float32
    g0, r0 = _gpu_normal(final, albedo, image, w)
    g1, r1 = _gpu_normal(final, albedo, image, w)
    assert _same_bits(g0, g1) and _same_bits(r0, r1)


def _residual_ratio(gram, rhs, ridge, rgb):
    """largest ||A x - r||_2 / (2^-23 ||A||_F ||x||_2) over the systems, in numpy f64"""
    worst = 0.0
    for b in range(gram.shape[0]):
        for c in range(3):
            L = gram.shape[2]
            A = gram[b, c] + ridge * (np.trace(gram[b, c]) / L) * np.eye(L)
            x = rgb[b, :, c].astype(np.float64)
            worst = max(worst, float(np.linalg.norm(A @ x - rhs[b, c]) / (2.0 ** -23 * np.linalg.norm(A) * np.linalg.norm(x))))
    return worst


@pytest.mark.parametrize("ridge", [0.0, 1e-3])
@pytest.mark.parametrize("B,L,H,W", [(1, 64, 33, 47), (2, 5, 21, 37), (1, 1, 1, 1)])
def test_solve_residual_and_the_restatements_solution(B, L, H, W, ridge):
    from geomconsistentfr_amd import fit_light_rgb
    final, albedo, image, w = emu.make_inputs(500 + L, B, L, H, W, "ones" if H * W == 1 else "mask")
    chunk, groups = _geometry(B, H, W)
    gram, rhs = emu.normal_equations(final, albedo, image, w, True, chunk, groups)
    want, want_info, _ = emu.solve(gram, rhs, ridge, False)
    rgb, info = fit_light_rgb(_dev(final), _dev(albedo), _dev(image), _dev(w), ridge=ridge, return_info=True)
    rgb, info = rgb.cpu().numpy(), info.cpu().numpy()
    ratio = _residual_ratio(gram, rhs, ridge, rgb)
    err = float(np.abs(rgb.astype(np.float64) - want).max() / np.abs(want).max())
    print("(%d,%d,%d,%d) ridge %g: residual %.3f of its gate; |x - restatement| / max|x| = %.3g (gate %.3g), f32 entries that differ %d"
          % (B, L, H, W, ridge, ratio, err, emu.GATE_SOLUTION, int((rgb != want).sum())))
    assert info.dtype == np.int32 and (info == 0).all() and (want_info == 0).all()
    assert ratio <= 1.0
    assert err <= emu.GATE_SOLUTION


def test_a_shared_rig_is_the_solve_of_the_summed_system():
    from geomconsistentfr_amd import fit_light_rgb
    B, L, H, W = 3, 4, 9, 11
    final, albedo, image, w = emu.make_inputs(31, B, L, H, W, "u8", shared_weight=True)
    chunk, groups = _geometry(B, H, W)
    gram, rhs = emu.normal_equations(final, albedo, image, w, True, chunk, groups)
    for ridge in (0.0, 1e-3):
        want, _i, _x = emu.solve(gram, rhs, ridge, True)
        rgb, info = fit_light_rgb(_dev(final), _dev(albedo), _dev(image), _dev(w), ridge=ridge, shared=True, return_info=True)
        assert tuple(rgb.shape) == (1, L, 3) and tuple(info.shape) == (1, 3) and (info == 0).all()
        rgb = rgb.cpu().numpy()
        summed = (gram.sum(axis=0, keepdims=True), rhs.sum(axis=0, keepdims=True))
        ratio = _residual_ratio(summed[0], summed[1], ridge, rgb)
        err = float(np.abs(rgb.astype(np.float64) - want).max() / np.abs(want).max())
        print("shared, ridge %g: residual %.3f of its gate, |x - restatement| / max|x| = %.3g" % (ridge, ratio, err))
        assert ratio <= 1.0 and err <= emu.GATE_SOLUTION
    # one face: the shared rig is the per-face rig, bit for bit
    one = [_dev(a[:1]) for a in (final, albedo, image)] + [_dev(w)]
    a = fit_light_rgb(*one, shared=True)
    b = fit_light_rgb(*one, shared=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_info_reports_a_singular_system():
    from geomconsistentfr_amd import fit_light_rgb
    B, L, H, W = 2, 3, 8, 9
    final, albedo, image, _ = emu.make_inputs(5, B, L, H, W, None)
    args = [_dev(a) for a in (final, albedo, image)]
    rgb, info = fit_light_rgb(*args, weight=torch.zeros(B, H, W, device=DEV), ridge=0.0, return_info=True)
    assert (info == 1).all() and torch.isnan(rgb).all() and tuple(info.shape) == (B, 3)
    final[:, 2] = final[:, 1]                                                     # two identical planes
    args[0] = _dev(final)
    rgb, info = fit_light_rgb(*args, ridge=0.0, return_info=True)
    rgb, info = rgb.cpu().numpy(), info.cpu().numpy()
    for b in range(B):
        for c in range(3):
            assert (info[b, c] == 0) == bool(np.isfinite(rgb[b, :, c]).all()), (b, c, info[b, c])
            assert info[b, c] == 0 or np.isnan(rgb[b, :, c]).all()
    rgb, info = fit_light_rgb(*args, ridge=1e-3, return_info=True)
    assert (info == 0).all() and torch.isfinite(rgb).all()


@pytest.mark.parametrize("B,L,H,W", [(2, 5, 21, 37), (1, 64, 33, 47)])
def test_round_trip_through_the_rig_stage(B, L, H, W):
    from geomconsistentfr_amd import combine_lights, fit_light_rgb
    rng = np.random.default_rng(300 + L)
    rgb_true = rng.uniform(-0.5, 1.5, (B, L, 3)).astype(np.float32)
    final, albedo, _im, _w = emu.make_inputs(400 + L, B, L, H, W, None)
    tf, ta = _dev(final), _dev(albedo)
    rendered, _ = combine_lights(tf, ta, _dev(rgb_true))
    image = rendered.permute(0, 2, 3, 1).contiguous()
    got, info = fit_light_rgb(tf, ta, image, ridge=0.0, return_info=True)
    got = got.cpu().numpy()
    ref = emu.design_lstsq(final, albedo, image.cpu().numpy(), None, True)[0]
    m = float(np.abs(rgb_true).max())
    err, err_ref = float(np.abs(got - rgb_true).max() / m), float(np.abs(ref - rgb_true).max() / m)
    print("(%d,%d,%d,%d): |x - rgb_true| / max|rgb_true|: fit_light_rgb %.3g, lstsq on the same inputs %.3g; gate %.3g"
          % (B, L, H, W, err, err_ref, emu.GATE_RECOVERY))
    assert (info == 0).all() and err <= emu.GATE_RECOVERY


def test_out_refills_a_captured_session_without_recapture():
    from geomconsistentfr_amd import fit_light_rgb
    from geomconsistentfr_amd import inference as inf
    from test_gpu_light_rig import _fixed_net
    B, S = 2, 64
    net, mask_u8 = _fixed_net(B, S)
    rng = np.random.default_rng(4)
    images = rng.random((B, S, S, 3), dtype=np.float32)
    lights = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)
    sess = inf.RelightSession(net, B, mask_u8, lights, device=DEV, H=S, W=S, light_rgb=torch.zeros(B, 3, 3, device=DEV))
    assert sess.graph is not None
    ptr = sess.light_rgb.data_ptr()
    seen = []
    for seed in (1, 2):
        photo = torch.from_numpy(np.random.default_rng(seed).random((B, S, S, 3), dtype=np.float32)).to(DEV)
        out, cm, _t = inf._lights_pass(net, photo, mask_u8, lights, 0.5, None, DEV, None, 200)
        ret = fit_light_rgb(out[8], out[0], photo, weight=cm, out=sess.light_rgb)
        assert ret.data_ptr() == ptr and sess.light_rgb.data_ptr() == ptr
        fresh = inf.capture_rig(net, photo, mask_u8, lights, device=DEV)
        assert fresh.data_ptr() != ptr and torch.equal(fresh, sess.light_rgb) and torch.isfinite(fresh).all()
        got = sess.run(torch.from_numpy(images))
        want = inf.relight_rig_device(net, images, mask_u8, lights, fresh, device=DEV)
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        seen.append(got.cpu().numpy())
    assert np.abs(seen[0].astype(int) - seen[1].astype(int)).max() > 0


def test_the_entries_run_inside_a_stream_capture():
    from geomconsistentfr_amd import fit_light_rgb
    B, L, H, W = 2, 11, 40, 56
    final, albedo, image, w = emu.make_inputs(9, B, L, H, W, "mask")
    args = [_dev(a) for a in (final, albedo, image, w)]
    eager, eager_info = fit_light_rgb(*args, return_info=True)                     # (also loads the library outside the capture)
    torch.cuda.synchronize(DEV)
    buf = torch.full((B, L, 3), float("nan"), device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ret, info = fit_light_rgb(*args, out=buf, return_info=True)
    buf.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert ret.data_ptr() == buf.data_ptr()
    assert torch.equal(buf.view(torch.int32), eager.view(torch.int32)) and torch.equal(info, eager_info)
    # new data in the static inputs reaches the replay
    args[2].copy_(torch.from_numpy(np.random.default_rng(10).random((B, H, W, 3), dtype=np.float32)))
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert torch.equal(buf.view(torch.int32), fit_light_rgb(*args).view(torch.int32)) and not torch.equal(buf, eager)


def _shipped_transfer_net():
    """the shipped lighting-transfer checkpoint (tests/golden/slt_checkpoint_epoch106.npz) on FIXED head outputs: its own albedo and
    depth of the two shipped photographs, as the reference's unmodified main() recorded them (tests/golden/slt_main_*.npz,
    model_albedo / model_depth), and the lighting head's recorded estimate.  No convolution runs: MIOpen's are not run-to-run
    reproducible, the block and the stages are (the comparison tests/test_gpu_environment.py makes on its fixed net).
    -> (net, photographs (2,256,256,3) f32, mask_u8)"""
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    za, zb = [np.load(os.path.join(GOLDEN, "slt_main_%s.npz" % t)) for t in ("a", "b")]
    sl = np.stack([np.concatenate([z["estimated_ambient"], z["estimated_light"]]) for z in (za, zb)]).astype(np.float32).reshape(2, 1, 1, 4)
    heads = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in
             (np.concatenate([za["model_albedo"], zb["model_albedo"]]), np.concatenate([za["model_depth"], zb["model_depth"]]), sl)]

    class Fixed(RelightNetLightingTransfer):
        def features(self, img, epoch, on_depth=None):
            a, d, SL = [t.clone() for t in heads]
            if on_depth is not None:
                on_depth(d, SL)
            return a, d, SL

    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "slt_checkpoint_epoch106.npz")).items()}
    net = Fixed()
    net.load_state_dict(sd, strict=True)
    photos = np.stack([za["input_u8"] / 255.0, zb["input_u8"] / 255.0]).astype(np.float32)
    return net.float().to(DEV).eval(), photos, za["mask_u8"]


def test_rig_lighting_transfer_is_relight_rig_under_the_captured_rig():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import sphere_directions
    net, photos, mask_u8 = _shipped_transfer_net()
    refs, inputs = photos, photos[::-1].copy()                                    # the rig of each photograph lights the other one
    B, H, W, _ = photos.shape
    L = 6
    lights = sphere_directions(L, 0.3)
    rgb = inf.capture_rig(net, refs, mask_u8, lights, device=DEV)
    assert tuple(rgb.shape) == (B, L, 3) and rgb.dtype == torch.float32 and rgb.is_cuda and torch.isfinite(rgb).all()
    for fix in (False, True):
        got = inf.rig_lighting_transfer(net, inputs, refs, mask_u8, lights, device=DEV, fix_border=fix)
        assert tuple(got.shape) == (B, H, W, 3) and got.dtype == torch.uint8 and got.is_cuda
        want = inf.relight_rig_device(net, inputs, mask_u8, lights, rgb, device=DEV, fix_border=fix)
        assert torch.equal(got, want)
    assert got.float().std() > 10
    shared = inf.capture_rig(net, refs, mask_u8, lights, shared=True, device=DEV)
    assert tuple(shared.shape) == (1, L, 3) and torch.isfinite(shared).all()
    one = inf.rig_lighting_transfer(net, inputs, refs, mask_u8, lights, shared=True, device=DEV)
    assert torch.equal(one, inf.relight_rig_device(net, inputs, mask_u8, lights, shared, device=DEV))
    # a photograph under its own captured rig (the heads are the checkpoint's for these photographs) comes closer to itself than
    # under a rig of equal white lights
    own = inf.relight_rig_device(net, refs, mask_u8, lights, rgb, device=DEV).float()
    flat = inf.relight_rig_device(net, refs, mask_u8, lights, np.full((L, 3), 1.0 / L, np.float32), device=DEV).float()
    target = torch.from_numpy(refs).to(DEV) * 255.0
    e_own, e_flat = float(((own - target) ** 2).mean()), float(((flat - target) ** 2).mean())
    print("mean squared error to the photograph, uint8 units: captured rig %.2f, equal white lights %.2f" % (e_own, e_flat))
    assert e_own < e_flat


def test_the_c_entries_refuse_bad_arguments_without_a_launch():
    from geomconsistentfr_amd import _lib
    lib = _lib.load()
    f = torch.zeros(2 * 3 * 4 * 5, device=DEV)
    d = torch.zeros(4096, dtype=torch.float64, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    p, q = f.data_ptr(), d.data_ptr()
    normal = lambda L=3, final=p, ws=q, gram=q, rhs=q: lib.gcfr_light_fit_normal(final, p, p, 1, None, 1, 2, L, 4, 5, ws, gram, rhs, None)
    assert normal(L=65) == -1 and normal(L=0) == -1
    assert normal(final=None) == -1 and normal(ws=None) == -1 and normal(gram=None) == -1 and normal(rhs=None) == -1
    solve = lambda L=3, ridge=1e-3, gram=q, rgb=p, info=i.data_ptr(): lib.gcfr_light_fit_solve(gram, q, 2, L, ridge, 2, rgb, info, None)
    assert solve(L=65) == -1 and solve(ridge=-1.0) == -1 and solve(ridge=float("nan")) == -1
    assert solve(gram=None) == -1 and solve(rgb=None) == -1 and solve(info=None) == -1
    torch.cuda.synchronize(DEV)
    assert float(d.abs().sum()) == 0 and float(f.abs().sum()) == 0 and int(i.abs().sum()) == 0 and ctypes.sizeof(ctypes.c_double) == 8
