"""GPU: the inference entries of the full-resolution feature (inference.relight_lights_fullres(_device), relight_rig_fullres(_device))
against the steps they are made of, on FIXED head outputs (test_gpu_light_rig._fixed_net: MIOpen's convolutions are not run-to-run
reproducible; the block, the stages and the image kernels are).  The network runs at 64 x 64, the smallest size the inference tests
use; the photographs are 128 x 128 (s = 2)."""
import numpy as np
import pytest
import torch

from test_fullres_host import TIE, TIE_SHARE
from test_gpu_light_rig import _fixed_net

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, S, SCALE = 2, 64, 2
LIGHTS = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)


def _case(seed, scale=SCALE):
    net, mask_u8 = _fixed_net(B, S)
    photos = np.random.default_rng(seed).integers(0, 256, (B, scale * S, scale * S, 3), dtype=np.uint8)
    return net, mask_u8, photos


def _pass(net, x, mask_u8, lights):
    from geomconsistentfr_amd import inference as inf
    m = torch.from_numpy(mask_u8).to(DEV)
    with torch.no_grad():
        return net.forward_lights(x, 200, inf.camera_matrix(1570.0, S, S), (m.to(torch.float64).reshape(S, S, 1) / 255.0),
                                  torch.from_numpy(lights).to(DEV)), m


def test_relight_lights_fullres_is_ingest_pass_and_the_fullres_launch():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(31)
    got = inf.relight_lights_fullres_device(net, photos, mask_u8, LIGHTS, SCALE, device=DEV)
    assert tuple(got.shape) == (B, 3, SCALE * S, SCALE * S, 3) and got.dtype == torch.uint8
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_photographs_device(p, SCALE)
    out, m = _pass(net, x, mask_u8, LIGHTS)
    want = pp.fullres_composites_device(p, x, out[5], m, SCALE)
    assert torch.equal(got, want)
    # the face is relit and differs between lights; outside the upsampled mask the photograph is returned
    g = got.cpu().numpy()
    assert (g[:, 0] != g[:, 1]).any() and (g[:, 0] != photos).any()
    import fullres_emulation as emu
    outside = emu.mask_up(mask_u8[None], SCALE)[0] == 0
    assert outside.any() and (g[:, :, outside] == photos[:, None][:, :, outside]).all()
    host = inf.relight_lights_fullres(net, photos, mask_u8, LIGHTS, SCALE, device=DEV)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, g)
    # a second compositing mask, other clamp and floor: passed through
    cm = np.where(mask_u8 > 0, 255, 0).astype(np.uint8)
    got2 = inf.relight_lights_fullres_device(net, photos, mask_u8, LIGHTS, SCALE, device=DEV, composite_mask_u8=cm, detail_clamp=2.0, floor=4.0)
    want2 = pp.fullres_composites_device(p, x, out[5], torch.from_numpy(cm).to(DEV), SCALE, detail_clamp=2.0, floor=4.0)
    assert torch.equal(got2, want2)


def test_relight_rig_fullres_with_one_white_light_is_the_first_light():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(32)
    white = np.ones((1, 3), np.float32)
    rig = inf.relight_rig_fullres(net, photos, mask_u8, LIGHTS[:1], white, SCALE, device=DEV)
    assert rig.shape == (B, SCALE * S, SCALE * S, 3) and rig.dtype == np.uint8
    np.testing.assert_array_equal(rig, inf.relight_lights_fullres(net, photos, mask_u8, LIGHTS[:1], SCALE, device=DEV)[:, 0])
    # a coloured rig of three lights: the rig stage's `rendered` at L = 1 through the same launch
    rgb = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)
    got = inf.relight_rig_fullres_device(net, photos, mask_u8, LIGHTS, rgb, SCALE, device=DEV)
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_photographs_device(p, SCALE)
    out, m = _pass(net, x, mask_u8, LIGHTS)
    rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(rgb).to(DEV)[None])
    assert torch.equal(got, pp.fullres_composites_device(p, x, rendered, m, SCALE))
    assert (got.cpu().numpy() != rig).any()


def test_scale_one_under_a_full_mask_agrees_with_relight_lights():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, _ = _case(33)
    photos = np.random.default_rng(33).integers(64, 225, (B, S, S, 3), dtype=np.uint8)
    full = np.full((S, S), 255, np.uint8)
    got = inf.relight_lights_fullres(net, photos, mask_u8, LIGHTS, 1, device=DEV, composite_mask_u8=full)
    x = pp.ingest_photographs_device(torch.from_numpy(photos).to(DEV), 1)
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), np.float32(photos / 255.0).view(np.uint32))
    want = inf.relight_lights(net, x, mask_u8, LIGHTS, device=DEV, composite_mask_u8=full)
    out, _ = _pass(net, x, mask_u8, LIGHTS)
    value = np.transpose((np.float32(255.0) * out[5].cpu().numpy()).astype(np.float64), (0, 1, 3, 4, 2))
    near_tie = np.abs(value - np.floor(value) - 0.5) <= TIE
    share = float(near_tie.mean())
    diff = (got != want) & ~near_tie
    print("s = 1: %d values, %d near a tie (%.4f %%), %d differ away from ties" % (got.size, int(near_tie.sum()), 100 * share, int(diff.sum())))
    assert got.shape == want.shape == (B, 3, S, S, 3)
    assert share <= TIE_SHARE and not diff.any() and got.std() > 10
