"""GPU: `Trainer.step` with TrainConfig.supervised_losses = "hip" (the fused supervised-loss head, losses.supervised_losses) against
the reference loop's recorded six iterations -- tests/test_gpu_train_steps.py's fixture, recorder, comparator and TOL, unchanged --
alone and together with the image-loss head; the control that the comparator sees this head (its depth gradient scaled by 2 is
reported); and one step from identical weights with the head on and off logging the same losses within 2e-6 relative."""
import pytest
import torch

from test_gpu_train_steps import TOL, _fixture, run_steps
from train_steps_record import compare

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _supervised_hip(tr):
    tr.cfg.supervised_losses = "hip"


def _both_hip(tr):
    tr.cfg.supervised_losses = "hip"
    tr.cfg.image_losses = "hip"


@pytest.mark.parametrize("perturb", [_supervised_hip, _both_hip], ids=["supervised", "supervised+image"])
def test_six_training_steps_with_the_supervised_head_follow_the_reference_loop(perturb):
    fix, faces = _fixture()
    got = run_steps(fix, faces, 6, perturb=perturb)
    bad, obs = compare(fix, got["arrays"], got["logs"], TOL)
    print({k: "%.3g" % v for k, v in obs.items() if k.startswith("loss_") or k.endswith("_sign_checked")})
    assert not bad, "\n".join(bad[:30])
    assert obs["G0_sign_checked"] > 1000 and obs["D0_sign_checked"] > 100, obs
    assert got["calls"] == [3, 1, 1, 1, 1, 3]


def test_the_comparator_reports_the_heads_depth_gradient_scaled_by_two(monkeypatch):
    from geomconsistentfr_amd import losses
    orig = losses._SupervisedLossesFunction.backward

    def backward(ctx, *grads):
        g = list(orig(ctx, *grads))
        g[0] = g[0] * 2.0                   # grad_depth
        return tuple(g)

    monkeypatch.setattr(losses._SupervisedLossesFunction, "backward", staticmethod(backward))
    fix, faces = _fixture()
    got = run_steps(fix, faces, 1, perturb=_supervised_hip)
    bad, _ = compare(fix, got["arrays"], got["logs"], TOL, n_iter=1)
    assert any(b.startswith("G0 ") and ("grad_norm" in b or "sampled gradient" in b) for b in bad), \
        "\n".join(bad[:30]) or "no mismatch reported"


def test_an_unknown_switch_value_is_refused_at_step_time():
    from geomconsistentfr_amd.train import TrainConfig, Trainer, synthetic_batch
    tr = Trainer(TrainConfig(), device=DEV)
    tr.cfg.supervised_losses = "cuda"
    with pytest.raises(ValueError, match="supervised_losses"):
        tr.step(synthetic_batch(1, 0, device=DEV), 200, 0)


def one_step_logs(kind, j):
    """the logged losses of step `j` of a fresh Trainer on the fixture's seeded weights and first batch"""
    from geomconsistentfr_amd.relightnet import PatchGAN, RelightNet
    from geomconsistentfr_amd.train import TrainConfig, Trainer
    from seeded_init import SEED_D, SEED_G, seeded_init_
    from test_gpu_train_steps import _batches
    _, faces = _fixture()
    tr = Trainer(TrainConfig(miopen_find=False), device=DEV, model=seeded_init_(RelightNet("3x3"), SEED_G),
                 patchgan=seeded_init_(PatchGAN(), SEED_D))
    tr.cfg.supervised_losses = kind
    return tr.step(_batches(faces[:1])[0], 0, j)


def test_one_step_from_identical_weights_logs_the_same_losses_with_either_head():
    """The step is j = 1: no discriminator step runs in front of the generator's, so PatchGAN's weights are the seeded ones in
    both runs and the head's inputs are the same launches on the same weights.  Every logged entry is held to 2e-6 relative.
    (At j = 0 the discriminator steps first; its backward through MIOpen is not reproducible from run to run, PatchGAN's weights
    and with them the logits differ, and the `generator` entry moves between any two runs, two "torch" runs included: measured on
    an MI355X 9.6e-5 torch against torch, 4.8e-5 and 7.1e-5 hip against torch.  At j = 1: `generator` 1.2e-6 torch against torch,
    8.9e-7 and 1.3e-6 hip against torch -- PatchGAN's forward is not bit-reproducible either, so the gate's margin on that entry is
    the noise's, not the head's, which is within 1e-7 of torch on the same logits; every other entry 3.7e-7 or less.)"""
    logs = {kind: one_step_logs(kind, 1) for kind in ("torch", "hip")}
    assert list(logs["torch"]) == list(logs["hip"]) and "depth" in logs["hip"] and "total" in logs["hip"]
    assert "discriminator" not in logs["hip"]
    for k, v in logs["torch"].items():
        print("%s: torch %.9g hip %.9g rel %.2e" % (k, v, logs["hip"][k], abs(v - logs["hip"][k]) / abs(v)))
    for k, v in logs["torch"].items():
        assert abs(v - logs["hip"][k]) <= 2e-6 * abs(v), (k, v, logs["hip"][k])
