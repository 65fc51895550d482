"""GPU: the `upsample` / `range_sigma` keywords of the full-resolution inference entries (inference.relight_lights_fullres(_device),
relight_rig_fullres(_device)) against the steps they are made of, on tests/test_gpu_fullres_inference.py's fixtures (fixed head
outputs, the network at 64 x 64, photographs of 128 x 128)."""
import numpy as np
import pytest
import torch

from test_gpu_fullres_inference import B, DEV, LIGHTS, S, SCALE, _case, _pass

pytestmark = pytest.mark.gpu


def test_relight_lights_fullres_guided_is_ingest_pass_and_the_guided_launch():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(41)
    got = inf.relight_lights_fullres_device(net, photos, mask_u8, LIGHTS, SCALE, device=DEV, upsample="guided")
    assert tuple(got.shape) == (B, 3, SCALE * S, SCALE * S, 3) and got.dtype == torch.uint8
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_photographs_device(p, SCALE)
    out, m = _pass(net, x, mask_u8, LIGHTS)
    want = pp.fullres_composites_device(p, x, out[5], m, SCALE, upsample="guided")
    assert torch.equal(got, want)
    g = got.cpu().numpy()
    assert (g[:, 0] != g[:, 1]).any() and (g[:, 0] != photos).any()
    host = inf.relight_lights_fullres(net, photos, mask_u8, LIGHTS, SCALE, device=DEV, upsample="guided")
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, g)
    # range_sigma, the clamp and the floor are passed through
    got2 = inf.relight_lights_fullres_device(net, photos, mask_u8, LIGHTS, SCALE, device=DEV, detail_clamp=2.0, floor=4.0,
                                             upsample="guided", range_sigma=8.0)
    want2 = pp.fullres_composites_device(p, x, out[5], m, SCALE, detail_clamp=2.0, floor=4.0, upsample="guided", range_sigma=8.0)
    assert torch.equal(got2, want2) and not torch.equal(got2, got)
    # the defaults are unchanged: without the keywords, and with upsample="bilinear", the bilinear launch
    plain = pp.fullres_composites_device(p, x, out[5], m, SCALE)
    assert torch.equal(inf.relight_lights_fullres_device(net, photos, mask_u8, LIGHTS, SCALE, device=DEV), plain)
    assert torch.equal(inf.relight_lights_fullres_device(net, photos, mask_u8, LIGHTS, SCALE, device=DEV, upsample="bilinear"), plain)
    assert not torch.equal(got, plain)


def test_relight_rig_fullres_guided_with_one_white_light_is_the_first_light():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(42)
    white = np.ones((1, 3), np.float32)
    rig = inf.relight_rig_fullres(net, photos, mask_u8, LIGHTS[:1], white, SCALE, device=DEV, upsample="guided", range_sigma=12.0)
    assert rig.shape == (B, SCALE * S, SCALE * S, 3) and rig.dtype == np.uint8
    np.testing.assert_array_equal(rig, inf.relight_lights_fullres(net, photos, mask_u8, LIGHTS[:1], SCALE, device=DEV, upsample="guided",
                                                                  range_sigma=12.0)[:, 0])
    # a coloured rig of three lights: the rig stage's `rendered` at L = 1 through the guided launch
    rgb = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)
    got = inf.relight_rig_fullres_device(net, photos, mask_u8, LIGHTS, rgb, SCALE, device=DEV, upsample="guided")
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_photographs_device(p, SCALE)
    out, m = _pass(net, x, mask_u8, LIGHTS)
    rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(rgb).to(DEV)[None])
    assert torch.equal(got, pp.fullres_composites_device(p, x, rendered, m, SCALE, upsample="guided"))
    # the default is the bilinear launch
    assert torch.equal(inf.relight_rig_fullres_device(net, photos, mask_u8, LIGHTS, rgb, SCALE, device=DEV),
                       pp.fullres_composites_device(p, x, rendered, m, SCALE))
