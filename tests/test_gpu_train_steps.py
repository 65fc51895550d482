"""GPU: six iterations of `Trainer.step` against six iterations of the reference's own training loop (T8:589-656).

tests/golden/t8_train_steps*.npz (oracle/make_golden_train_steps.py) holds what the unmodified `main()` did on CPU from the
seeded weights of tests/seeded_init.py over six synthetic faces in the batch order 0,1,0,1,0,1: the eleven numbers each iteration
prints, every optimiser step's gradients, Adam moments and parameter moves (tests/train_steps_record.py), and the loader's bytes.
Here the same faces go through `dataset.assemble_batch`, the same weights through Trainer -- the T8-form network with batch-statistic
BatchNorm, the HIP forward with its hoisted prepass (`prepared=`), the fused HIP backward inside `loss.backward()`, the D-step
schedule and both Adams -- and the same recorder.

What differs is arithmetic: MIOpen's convolutions against the CPU's, f32 where the reference's f64 camera matrix promotes the
render block to f64, f32 atomics in the backward, and argmin flips under ~1e-6 depth noise.  At the seeded untrained weights the
march's minima are full of near-ties, so the LIGHT gradient is chaotic: linear_SL2's gradient norm differs from the reference's by
7-10 % at iteration 0 and by ~3 % between two GPU runs (MIOpen's convolutions are not run-to-run reproducible), while the eleven
losses agree to 3e-5.  After the first step Adam moves every element by ~lr whatever its gradient, noise-level ones included, and
the trajectories part: the reference itself, run twice on the same CPU, differs by 3e-7, 2e-4, 2e-3, 3e-3, 1e-2 in its printed
losses at iterations 1-5.  Measured on an MI355X (largest relative difference over ssim_blur aten / miopen, iterations 0-5):
losses 2.9e-5, 1.6e-2, 2.0e-2, 4.7e-1, 2.2e-1, 4.8e-1; G gradient norms / sampled elements 0.17, 4.6, 2.0, 3.8, 4.8, 2.1 (iteration
0: linear_SL2; D: 0.016 at j = 0, 0.26 at j = 5); Adam's first moment 0.12, 1.2, 1.1, 1.4, 1.7, 1.1; second 0.30, 3.7, 3.3, 2.9,
2.8, 2.7; parameter moves 1.6e-3 (D), 0.26, 0.25, 0.28, 0.32, 0.32.  TOL is ~4x those.  The strong checks are the exact ones: the
step schedule, zero-versus-non-zero gradients of every tensor at every step, iteration 0's losses, and the sign of the first update
on ~1,750 sampled G elements and ~170 D elements whose reference gradient stands above the measured difference.

PatchGAN's running BatchNorm buffers differ on purpose: the reference runs PatchGAN on the fake and the real images at EVERY
iteration and steps D only when j % 5 == 0 (T8:619-626); Trainer runs those two forwards only on D-step iterations.  Losses and
parameters do not see it (training-mode BatchNorm normalises with batch statistics); the buffers and num_batches_tracked do.

Negative controls: the same comparator must report a mismatch for G's Adam betas (0.85, 0.999) (the first moment is 1.5x), for
gd_ratio = 1 (a D step at j = 1), and for the light gradient of the render block's backward scaled by 2.  A scale of 1.01 is below
the light gradient's measured noise at these weights and would pass unseen."""


import os

import numpy as np
import pytest
import torch

import train_steps_record as TSR
from seeded_init import SEED_D, SEED_G, seeded_init_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# per iteration j = 0..5: ~4x the measured relative differences of the module docstring
TOL = dict(loss=[1.2e-4, 6.5e-2, 8e-2, 1.9, 0.9, 1.9],
           grad=[0.7, 18.0, 8.0, 15.0, 19.0, 8.5],
           m=[0.45, 5.0, 4.6, 5.7, 6.8, 4.3],         # (iteration 0 below 0.5: the betas control moves every tensor's by exactly that)
           v=[1.2, 15.0, 13.0, 12.0, 11.5, 11.0],
           delta=[6.5e-3, 1.05, 1.0, 1.15, 1.3, 1.3])


def _fixture():
    """(trajectory, [the loader's arrays of batch 0, of batch 1])"""
    load = lambda name: dict(np.load(os.path.join(GOLDEN, name)))
    return load("t8_train_steps.npz"), [load("t8_train_steps_faces%d.npz" % b) for b in (0, 1)]


def _batches(faces):
    from geomconsistentfr_amd.dataset import assemble_batch
    out = []
    for f in faces:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        batch = assemble_batch(up(f["images"]), up(f["masks"]), up(f["face_masks"]), up(f["albedo"]))
        batch.update(lightings=up(f["lightings"]), depths=up(f["depths"]))
        out.append(batch)
    return out


def run_steps(fix, faces, n_iter, ssim_blur="aten", gd_ratio=5, perturb=None):
    """Trainer from the fixture's initial weights over the fixture's batches, recorded as the generator recorded the reference."""
    from geomconsistentfr_amd.relightnet import PatchGAN, RelightNet
    from geomconsistentfr_amd.train import TrainConfig, Trainer
    tr = Trainer(TrainConfig(miopen_find=False, ssim_blur=ssim_blur, gd_ratio=gd_ratio), device=DEV,
                 model=seeded_init_(RelightNet("3x3"), SEED_G), patchgan=seeded_init_(PatchGAN(), SEED_D))
    if perturb is not None:
        perturb(tr)
    rec = TSR.StepRecorder(index=TSR.index_of(fix))
    rec.add("G", tr.model)
    rec.add("D", tr.patchgan)
    calls = []
    hook = tr.patchgan.register_forward_pre_hook(lambda _m, _x: calls.__setitem__(-1, calls[-1] + 1))
    batches, logs = _batches(faces), []
    try:
        with rec:
            for j in range(n_iter):
                rec.iteration = j
                calls.append(0)
                logs.append(tr.step(batches[int(fix["order"][j])], 0, j))
    finally:
        hook.remove()
    return dict(arrays=rec.arrays(), logs=logs, calls=calls, patchgan=tr.patchgan)


@pytest.mark.parametrize("ssim_blur", ["aten", "miopen"])
def test_six_training_steps_follow_the_reference_loop(ssim_blur):
    fix, faces = _fixture()
    got = run_steps(fix, faces, 6, ssim_blur)
    bad, obs = TSR.compare(fix, got["arrays"], got["logs"], TOL)
    assert not bad, "\n".join(bad[:30])
    assert obs["G0_sign_checked"] > 1000 and obs["D0_sign_checked"] > 100, obs
    # PatchGAN's buffers: 3 forwards per iteration in the reference, 3 on D-step iterations and 1 (the generator's) otherwise here
    assert list(fix["patchgan_calls"]) == [3] * 6 and got["calls"] == [3, 1, 1, 1, 1, 3]
    for bn in ("bn2", "bn3", "bn4"):
        mine = getattr(got["patchgan"], bn)
        assert int(fix["D_buf_%s.num_batches_tracked" % bn]) == 18 and int(mine.num_batches_tracked) == 10
        assert not np.allclose(mine.running_mean.cpu().numpy(), fix["D_buf_%s.running_mean" % bn], rtol=1e-2, atol=0)


def _betas(tr):
    tr.opt.param_groups[0]["betas"] = (0.85, 0.999)


@pytest.mark.parametrize("perturbation", ["adam_betas", "gd_ratio_1", "light_grad_x2"])
def test_the_comparator_reports_a_perturbed_step(perturbation, monkeypatch):
    from geomconsistentfr_amd import block as R
    fix, faces = _fixture()
    kw, n_iter = {}, 1
    if perturbation == "adam_betas":
        kw["perturb"], expect = _betas, "m_norm"
    elif perturbation == "gd_ratio_1":
        kw["gd_ratio"], n_iter, expect = 1, 2, "schedule"
    else:
        orig = R._RenderFromDepthFunction.backward

        def backward(ctx, *grads):
            g = list(orig(ctx, *grads))
            g[2] = g[2] * 2.0                   # the light's gradient
            return tuple(g)

        monkeypatch.setattr(R._RenderFromDepthFunction, "backward", staticmethod(backward))
        expect = "linear_SL2"
    got = run_steps(fix, faces, n_iter, **kw)
    bad, _ = TSR.compare(fix, got["arrays"], got["logs"], TOL, n_iter=n_iter)
    assert any(expect in b for b in bad), "\n".join(bad[:30]) or "no mismatch reported"
