"""GPU: the guided inference entries of the box feature (inference.relight_lights_in_photograph_guided(_device),
relight_rig_in_photograph_guided(_device)) against the steps they are made of, on FIXED head outputs (test_gpu_light_rig._fixed_net),
as tests/test_gpu_fullres_box_inference.py holds the bilinear ones.  The network runs at 64 x 64; the photographs are 150 x 171 with
one 93 x 77 box per face, and 256 x 256 for the power-of-two anchor at s = 4."""
import numpy as np
import pytest
import torch

from test_gpu_fullres_box_inference import B, BOXES, DEV, HP, LIGHTS, S, WP, _case, _pass

pytestmark = pytest.mark.gpu
RGB = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)


def test_relight_lights_in_photograph_guided_is_box_ingest_pass_and_the_guided_box_launch():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(51)
    got = inf.relight_lights_in_photograph_guided_device(net, photos, BOXES, mask_u8, LIGHTS, device=DEV)
    assert tuple(got.shape) == (B, 3, HP, WP, 3) and got.dtype == torch.uint8
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_box_device(p, BOXES, (S, S))
    out, m = _pass(net, x, mask_u8, LIGHTS)
    want = pp.fullres_box_composites_device(p, BOXES, x, out[5], m, upsample="guided")
    assert torch.equal(got, want)
    assert not torch.equal(got, pp.fullres_box_composites_device(p, BOXES, x, out[5], m))          # not the bilinear launch
    # the face is relit and differs between lights; outside the box the photograph is returned
    g = got.cpu().numpy()
    assert (g[:, 0] != g[:, 1]).any() and (g[:, 0] != photos).any()
    outside = np.ones((B, HP, WP), bool)
    for b, (x0, y0, bw, bh) in enumerate(BOXES):
        outside[b, y0:y0 + bh, x0:x0 + bw] = False
    for l in range(3):
        np.testing.assert_array_equal(g[:, l][outside], photos[outside])
    host = inf.relight_lights_in_photograph_guided(net, photos, BOXES.tolist(), mask_u8, LIGHTS, device=DEV)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, g)
    # a second compositing mask, other clamp, floor and range_sigma, the box alone: passed through
    cm = np.where(mask_u8 > 0, 255, 0).astype(np.uint8)
    got2 = inf.relight_lights_in_photograph_guided_device(net, photos, BOXES, mask_u8, LIGHTS, device=DEV, composite_mask_u8=cm,
                                                          detail_clamp=2.0, floor=4.0, paste=False, range_sigma=6.0)
    want2 = pp.fullres_box_composites_device(p, BOXES, x, out[5], torch.from_numpy(cm).to(DEV), detail_clamp=2.0, floor=4.0, paste=False,
                                             upsample="guided", range_sigma=6.0)
    assert tuple(got2.shape) == (B, 3, 77, 93, 3) and torch.equal(got2, want2)
    assert not torch.equal(got2, pp.fullres_box_composites_device(p, BOXES, x, out[5], torch.from_numpy(cm).to(DEV), detail_clamp=2.0,
                                                                  floor=4.0, paste=False, upsample="guided"))


def test_relight_rig_in_photograph_guided_with_one_white_light_is_the_first_light():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(53)
    white = np.ones((1, 3), np.float32)
    for paste in (True, False):
        rig = inf.relight_rig_in_photograph_guided(net, photos, BOXES, mask_u8, LIGHTS[:1], white, device=DEV, paste=paste)
        assert rig.shape == ((B, HP, WP, 3) if paste else (B, 77, 93, 3)) and rig.dtype == np.uint8
        np.testing.assert_array_equal(rig, inf.relight_lights_in_photograph_guided(net, photos, BOXES, mask_u8, LIGHTS[:1], device=DEV,
                                                                                  paste=paste)[:, 0])
    # a coloured rig of three lights: the rig stage's `rendered` at L = 1 through the same launch
    got = inf.relight_rig_in_photograph_guided_device(net, photos, BOXES, mask_u8, LIGHTS, RGB, device=DEV, range_sigma=12.0)
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_box_device(p, BOXES, (S, S))
    out, m = _pass(net, x, mask_u8, LIGHTS)
    rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(RGB).to(DEV)[None])
    assert torch.equal(got, pp.fullres_box_composites_device(p, BOXES, x, rendered, m, upsample="guided", range_sigma=12.0))
    assert (got.cpu().numpy() != inf.relight_rig_in_photograph_guided(net, photos, BOXES, mask_u8, LIGHTS[:1], white, device=DEV)).any()


def test_a_whole_photograph_box_at_four_times_the_network_is_relight_lights_fullres_guided():
    from geomconsistentfr_amd import inference as inf
    net, mask_u8, photos = _case(54, 4 * S, 4 * S)
    whole = (0, 0, 4 * S, 4 * S)
    want = inf.relight_lights_fullres_device(net, photos, mask_u8, LIGHTS, 4, device=DEV, upsample="guided")
    for paste in (True, False):
        got = inf.relight_lights_in_photograph_guided_device(net, photos, whole, mask_u8, LIGHTS, device=DEV, paste=paste)
        assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(inf.relight_rig_in_photograph_guided_device(net, photos, whole, mask_u8, LIGHTS, RGB, device=DEV, range_sigma=9.0),
                       inf.relight_rig_fullres_device(net, photos, mask_u8, LIGHTS, RGB, 4, device=DEV, upsample="guided", range_sigma=9.0))
