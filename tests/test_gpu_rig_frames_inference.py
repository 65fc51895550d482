"""GPU: the inference entries of the rig-frames feature (inference.relight_rig_frames(_device); relight_environment_frames with
`fused=True`) byte for byte against the entries they must equal, on FIXED head outputs (test_gpu_light_rig._fixed_net: MIOpen's
convolutions are not run-to-run reproducible; the block, the stages and the image kernels are)."""
import numpy as np
import pytest
import torch

from test_gpu_environment import _rotation_y
from test_gpu_light_rig import _fixed_net

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, S = 2, 64


def _case(seed):
    net, mask_u8 = _fixed_net(B, S)
    images = np.random.default_rng(seed).random((B, S, S, 3), dtype=np.float32)
    return net, mask_u8, images


@pytest.mark.parametrize("fix_border", [False, True])
def test_three_rigs_in_one_call_are_three_relight_rig_calls(fix_border):
    from geomconsistentfr_amd import inference as inf
    net, mask_u8, images = _case(21)
    lights = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)
    key = np.asarray([(0.9, 0.8, 0.6), (0.0, 0.0, 0.0), (0.1, 0.1, 0.1)], np.float32)
    fill = np.asarray([(0.0, 0.0, 0.0), (0.3, 0.4, 0.7), (0.1, 0.1, 0.1)], np.float32)
    rigs = np.stack([key, np.float32(0.5) * (key + fill), fill])                                # a key fading into a fill: (F,L,3)
    got = inf.relight_rig_frames_device(net, images, mask_u8, lights, rigs, device=DEV, fix_border=fix_border)
    assert tuple(got.shape) == (B, 3, S, S, 3) and got.dtype == torch.uint8
    for f in range(3):
        one = inf.relight_rig_device(net, images, mask_u8, lights, rigs[f], device=DEV, fix_border=fix_border)
        assert torch.equal(got[:, f], one), f
    assert not torch.equal(got[:, 0], got[:, 1]) and not torch.equal(got[:, 1], got[:, 2]) and got.float().std() > 10
    # rigs per face: face 1 runs the fade backwards
    per_face = np.stack([rigs, rigs[::-1]])                                                    # (B,F,L,3)
    got2 = inf.relight_rig_frames_device(net, images, mask_u8, lights, per_face, device=DEV, fix_border=fix_border)
    assert torch.equal(got2[0], got[0]) and torch.equal(got2[1, 0], got[1, 2]) and torch.equal(got2[1, 2], got[1, 0])
    host = inf.relight_rig_frames(net, images, mask_u8, lights, rigs, device=DEV, fix_border=fix_border)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, got.cpu().numpy())


@pytest.mark.parametrize("fix_border", [False, True])
def test_the_fused_turntable_returns_the_loops_bytes(fix_border):
    from geomconsistentfr_amd import inference as inf
    net, mask_u8, images = _case(22)
    rng = np.random.default_rng(5)
    env = (2.0 * rng.random((8, 16, 3))).astype(np.float32)
    env[:, 8:] *= np.float32(4.0)                                                              # one side of the world is brighter
    rotations = np.stack([_rotation_y(a) for a in (0.0, 2.1, 4.2)])
    loop = inf.relight_environment_frames(net, images, mask_u8, env, rotations, n_lights=6, device=DEV, fix_border=fix_border)
    fused = inf.relight_environment_frames(net, images, mask_u8, env, rotations, n_lights=6, device=DEV, fix_border=fix_border,
                                           fused=True)
    assert tuple(fused.shape) == (B, 3, S, S, 3) and fused.dtype == torch.uint8
    print("bytes that differ between the loop and the fused turntable: %d of %d" % (int((loop != fused).sum()), fused.numel()))
    assert torch.equal(fused, loop)
    assert not torch.equal(fused[:, 0], fused[:, 1]) and not torch.equal(fused[:, 1], fused[:, 2])
    # a map per face
    both = np.stack([env, np.float32(0.25) * env])
    per_face = inf.relight_environment_frames(net, images, mask_u8, both, rotations, n_lights=6, device=DEV, fused=True)
    assert torch.equal(per_face, inf.relight_environment_frames(net, images, mask_u8, both, rotations, n_lights=6, device=DEV))
