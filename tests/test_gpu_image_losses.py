"""GPU: the fused image-loss head (losses.image_losses, csrc/gcfr_losses.hip) against the project's CPU restatement in f64 --
`train.ssim` (held to a naive numpy SSIM by tests/test_train_host.py and to the reference loop's printed DSSIM by
tests/test_train_vs_reference.py) and the torch expressions of `train.generator_losses`, evaluated in f64 on the f32 inputs.

Gates (they are the ones tests/test_gpu_ssim_blur.py applies to the two existing GPU forms of the SSIM, for the reason given there:
the same f32 sums of the same eleven products in another order):
  composite                      bit-equal to the torch f32 expression
  ssim per (image, channel)      2e-6 relative;  the DSSIM value formed from it: 2e-6 relative
  recon_sq_sum, mask_sum         2e-6 relative (f32 terms of <= ~3 ulp each, non-negative, added in f64)
  gradient w.r.t. rendered       within 2e-5 of its largest entry -- for all upstream gradients together AND for each of the three
                                 alone (under a random gradient on the composite, entries of order 1, the SSIM's part of order
                                 1 / (H W) would be invisible)
  two calls on the same inputs   bit-equal outputs and gradient
Each case prints its measured figures before it asserts.
Then the training step: one step with TrainConfig.image_losses "torch" and "hip" logs the same losses within 1e-4 relative (the gate
and the reasoning of test_one_training_step_logs_the_same_losses_with_either_blur), six steps with "hip" follow the reference loop
under tests/test_gpu_train_steps.py's comparator and TOL, unchanged, and the comparator reports the op's gradient scaled by 2.

These gates hold in THIS file's regime only: `_pair()` is white noise, window variance 1/12 against C2 = 9e-4, the best-conditioned
input an SSIM can get.  On smooth or flat images -- what the training step feeds the head -- f32 SSIM in any operation order is further
from f64, by up to two orders of magnitude and more for the SSIM's own gradient; the measured figures per input family, for the head and
for the three torch f32 forms, are the table of DESIGN.md 4.5 (one copy, not repeated here).  tests/test_gpu_image_losses_regimes.py
measures them and, instead of "close to f64", pins the head bit for bit to a numpy-f32 restatement of its operation order
(tests/image_losses_emulation.py).

Measured on an MI355X (largest over the 25 value-and-gradient cases below): ssim per (image, channel) 5.0e-8 relative, DSSIM 1.1e-6
(the fractional mask at 2x64x40: 1 - mean is small there), recon_sq_sum 5.5e-8, mask_sum 3.1e-8; gradient, as a fraction of its largest
entry: 8.4e-8 all upstreams together, 3.9e-8 composite alone, 3.0e-7 recon alone, 1.5e-6 SSIM alone.  One step torch / hip: every
logged loss within 3.1e-5 relative (PatchGAN's term; MIOpen's run-to-run noise).  Six steps: largest relative loss difference from the
reference loop 3.0e-5 at iteration 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SHAPES = [(4, 256, 256), (2, 64, 40), (1, 33, 47), (3, 21, 128)]


def _pair(B, H, W, seed=0):
    """inputs as in test_gpu_ssim_blur._pair"""
    rng = np.random.default_rng(seed)
    Y = rng.random((B, 3, H, W), dtype=np.float32)
    X = np.clip(Y + 0.08 * rng.standard_normal(Y.shape).astype(np.float32), 0, 1)
    return X, Y


def _mask(kind, B, H, W, seed=1):
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    if kind == "fractional":
        return rng.random((B, H, W), dtype=np.float32)
    r, c = np.mgrid[0:H, 0:W]
    m = np.stack([(((c - W / 2.0 - i) / (0.36 * W)) ** 2 + ((r - H / 2.0 + i) / (0.42 * H)) ** 2) < 1 for i in range(B)])
    return m.astype(np.float32)                                   # a face-shaped {0,1} mask, a little different per image


def _ssim_bc(X, Y, data_range=1.0):
    """`train.ssim` per (image, channel), before the relu: every channel as an image of its own"""
    from geomconsistentfr_amd.train import ssim
    B, C, H, W = X.shape
    return ssim(X.reshape(B * C, 1, H, W), Y.reshape(B * C, 1, H, W), data_range=data_range, size_average=False,
                nonnegative_ssim=False).reshape(B, C)


def _dssim(s):
    return 8.0 * (1 - torch.relu(s).mean(1).mean()) / 2.0


def _upstreams(B, H, W, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, 3, H, W)).astype(np.float32), rng.standard_normal((B, 3)).astype(np.float32),
            np.float32(0.37))


def _reference(X, Y, M, ups):
    """f64 on the CPU: values, and the gradient for each selection of upstream gradients"""
    x = torch.from_numpy(X).double().requires_grad_()
    y = torch.from_numpy(Y).double()
    m3 = torch.ones_like(y) if M is None else torch.from_numpy(M).double()[:, None].expand(-1, 3, -1, -1)
    comp = x * m3 + (1.0 - m3) * y
    sq = ((x * m3 - y * m3) ** 2).sum()
    s = _ssim_bc(comp, y)
    x32, y32 = torch.from_numpy(X), torch.from_numpy(Y)
    m32 = torch.ones_like(y32) if M is None else torch.from_numpy(M)[:, None].expand(-1, 3, -1, -1)
    comp32 = x32 * m32 + (1.0 - m32) * y32                          # the torch f32 expression (T8:619)
    Gc, Gs, gq = (torch.from_numpy(np.asarray(u)).double() for u in ups)
    terms = dict(composite=(comp * Gc).sum(), ssim=(s * Gs).sum(), recon=gq * sq)
    grads = {k: torch.autograd.grad(v, x, retain_graph=True)[0].numpy() for k, v in terms.items()}
    grads["all"] = grads["composite"] + grads["ssim"] + grads["recon"]
    return dict(composite=comp32.numpy(), sq=float(sq.detach()), msum=float(m3.sum()), ssim=s.detach().numpy(), dssim=float(_dssim(s.detach())),
                grads=grads)


def _run_op(X, Y, M, ups, layout):
    from geomconsistentfr_amd.losses import image_losses
    x = torch.from_numpy(X).to(DEV).requires_grad_()
    y = torch.from_numpy(Y).to(DEV)
    if layout == "nhwc":
        y = y.permute(0, 2, 3, 1).contiguous()
    m = None if M is None else torch.from_numpy(M).to(DEV)
    comp, sq, msum, s = image_losses(x, y, m, images_layout=layout)
    Gc, Gs, gq = (torch.from_numpy(np.asarray(u)).to(DEV) for u in ups)
    terms = dict(composite=(comp * Gc).sum(), ssim=(s * Gs).sum(), recon=gq * sq)
    grads = {k: torch.autograd.grad(v, x, retain_graph=True)[0].cpu().numpy() for k, v in terms.items()}
    grads["all"] = torch.autograd.grad(sum(terms.values()), x)[0].cpu().numpy()
    assert not msum.requires_grad
    return dict(composite=comp.detach().cpu().numpy(), sq=float(sq.detach()), msum=float(msum), ssim=s.detach().cpu().numpy(),
                dssim=float(_dssim(s.detach().double())), grads=grads)


def _hold(got, ref, tag):
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))
    e_ssim, e_dssim = rel(got["ssim"], ref["ssim"]), rel(got["dssim"], ref["dssim"])
    e_sq, e_m = rel(got["sq"], ref["sq"]), rel(got["msum"], ref["msum"])
    e_g = {k: float(np.abs(got["grads"][k] - ref["grads"][k]).max() / np.abs(ref["grads"][k]).max()) for k in ref["grads"]}
    print("%s: ssim %.2e dssim %.2e sq %.2e msum %.2e grad %s" % (tag, e_ssim, e_dssim, e_sq, e_m,
                                                                   " ".join("%s %.2e" % kv for kv in sorted(e_g.items()))))
    assert np.array_equal(got["composite"], ref["composite"]), (tag, "composite is not bit-equal to the torch f32 expression")
    assert e_ssim <= 2e-6 and e_dssim <= 2e-6, (tag, e_ssim, e_dssim)
    assert e_sq <= 2e-6 and e_m <= 2e-6, (tag, e_sq, e_m)
    for k, e in e_g.items():
        assert np.abs(ref["grads"][k]).max() > 0
        assert e <= 2e-5, (tag, k, e)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("mask", ["face", "fractional", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_values_and_gradients_against_the_f64_restatement(shape, mask, layout):
    B, H, W = shape
    X, Y = _pair(B, H, W)
    M, ups = _mask(mask, B, H, W), _upstreams(B, H, W)
    _hold(_run_op(X, Y, M, ups, layout), _reference(X, Y, M, ups), "%s %s %s" % (shape, mask, layout))


def test_values_and_gradients_at_the_training_batch():
    B, H, W = 32, 256, 256
    X, Y = _pair(B, H, W)
    M, ups = _mask("face", B, H, W), _upstreams(B, H, W)
    _hold(_run_op(X, Y, M, ups, "nhwc"), _reference(X, Y, M, ups), "(32, 256, 256) face nhwc")


def test_negative_ssim_is_returned_raw_and_the_clamp_zeroes_its_gradient():
    """Y uniform random, X[0] = 1 - Y[0] (anti-correlated: SSIM about -0.97), X[1] = a noisy copy of Y[1] (about +0.96).  The op
    returns the raw negative means; `relu` in the DSSIM formula then gives image 0 exactly no gradient and image 1 some."""
    from geomconsistentfr_amd.losses import image_losses
    rng = np.random.default_rng(11)
    Y = rng.random((2, 3, 64, 40), dtype=np.float32)
    X = np.stack([1.0 - Y[0], np.clip(Y[1] + 0.05 * rng.standard_normal(Y[1].shape).astype(np.float32), 0, 1)]).astype(np.float32)
    ref = _ssim_bc(torch.from_numpy(X).double(), torch.from_numpy(Y).double()).numpy()
    x = torch.from_numpy(X).to(DEV).requires_grad_()
    _, _, _, s = image_losses(x, torch.from_numpy(Y).to(DEV), None, images_layout="nchw")
    got = s.detach().cpu().numpy()
    print("per-image SSIM: op %s, f64 restatement %s" % (got.mean(1), ref.mean(1)))
    assert (ref[0] < -0.9).all() and (ref[1] > 0.9).all()
    assert (got[0] < 0).all()
    np.testing.assert_allclose(got, ref, rtol=2e-6)
    _dssim(s).backward()
    g = x.grad.cpu().numpy()
    assert (g[0] == 0).all()
    assert np.abs(g[1]).max() > 0


def test_two_calls_return_the_same_bits():
    from geomconsistentfr_amd.losses import image_losses
    B, H, W = 4, 256, 256
    X, Y = _pair(B, H, W, seed=4)
    M, (Gc, Gs, gq) = _mask("fractional", B, H, W), _upstreams(B, H, W)
    y = torch.from_numpy(Y).to(DEV).permute(0, 2, 3, 1).contiguous()
    m = torch.from_numpy(M).to(DEV)
    runs = []
    for _ in range(2):
        x = torch.from_numpy(X).to(DEV).requires_grad_()
        comp, sq, msum, s = image_losses(x, y, m)
        ((comp * torch.from_numpy(Gc).to(DEV)).sum() + (s * torch.from_numpy(Gs).to(DEV)).sum() + float(gq) * sq).backward()
        runs.append([t.detach().clone() for t in (comp, sq, msum, s, x.grad)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_one_training_step_logs_the_same_losses_with_either_image_loss_head():
    from geomconsistentfr_amd.train import TrainConfig, Trainer, synthetic_batch
    logs = {}
    for kind in ("torch", "hip"):
        torch.manual_seed(77)
        tr = Trainer(TrainConfig(image_losses=kind), device=DEV)
        batch = synthetic_batch(4, 0, device=DEV)
        logs[kind] = tr.step(batch, 200, 0, log=True)
    assert set(logs["torch"]) == set(logs["hip"]) and "DSSIM" in logs["hip"] and "discriminator" in logs["hip"]
    for k, v in logs["torch"].items():
        print("%s: torch %.9g hip %.9g" % (k, v, logs["hip"][k]))
    for k, v in logs["torch"].items():
        assert abs(v - logs["hip"][k]) <= 1e-4 * max(abs(v), 1e-3), (k, v, logs["hip"][k])


def test_an_unknown_switch_value_is_refused_at_step_time():
    from geomconsistentfr_amd.train import TrainConfig, Trainer, synthetic_batch
    tr = Trainer(TrainConfig(), device=DEV)
    tr.cfg.image_losses = "cuda"
    with pytest.raises(ValueError, match="image_losses"):
        tr.step(synthetic_batch(1, 0, device=DEV), 200, 0)


def _use_hip(tr):
    tr.cfg.image_losses = "hip"


def test_six_training_steps_with_the_hip_head_follow_the_reference_loop():
    import test_gpu_train_steps as T
    import train_steps_record as TSR
    fix, faces = T._fixture()
    got = T.run_steps(fix, faces, 6, perturb=_use_hip)
    bad, obs = TSR.compare(fix, got["arrays"], got["logs"], T.TOL)
    print({k: "%.3g" % v for k, v in obs.items() if k.startswith("loss_") or k.endswith("_sign_checked")})
    assert not bad, "\n".join(bad[:30])
    assert obs["G0_sign_checked"] > 1000 and obs["D0_sign_checked"] > 100, obs
    assert list(fix["patchgan_calls"]) == [3] * 6 and got["calls"] == [3, 1, 1, 1, 1, 3]


def test_the_comparator_reports_the_heads_gradient_scaled_by_two(monkeypatch):
    import test_gpu_train_steps as T
    import train_steps_record as TSR
    from geomconsistentfr_amd import losses
    orig = losses._ImageLossesFunction.backward

    def backward(ctx, *grads):
        g = list(orig(ctx, *grads))
        g[0] = g[0] * 2.0                   # grad_rendered
        return tuple(g)

    monkeypatch.setattr(losses._ImageLossesFunction, "backward", staticmethod(backward))
    fix, faces = T._fixture()
    got = T.run_steps(fix, faces, 1, perturb=_use_hip)
    bad, _ = TSR.compare(fix, got["arrays"], got["logs"], T.TOL, n_iter=1)
    assert any(b.startswith("G0 ") and ("grad_norm" in b or "sampled gradient" in b) for b in bad), \
        "\n".join(bad[:30]) or "no mismatch reported"
