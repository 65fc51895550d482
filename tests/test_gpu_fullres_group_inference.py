"""GPU: the inference entries of the group-photograph feature (inference.relight_lights_in_group_photograph(_device),
relight_rig_in_group_photograph(_device)) against the steps they are made of, on FIXED head outputs (test_gpu_light_rig._fixed_net,
as tests/test_gpu_fullres_anybox_inference.py).  The network runs at 64 x 64 on 3 faces over 2 photographs of 90 x 101: faces 0 and
2 live in photograph 0 and overlap (a 40 x 36 box, smaller than the network, and a 70 x 66 one), face 1 is wide and flat in
photograph 1."""
import numpy as np
import pytest
import torch

from test_gpu_light_rig import _fixed_net

import fullres_group_emulation as group

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, P, S = 3, 2, 64
HP, WP = 90, 101
BOXES = np.array([(11, 40, 40, 36), (26, 3, 75, 9), (20, 15, 70, 66)])              # (x0, y0, bw, bh)
INDEX = [0, 1, 0]
LIGHTS = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)


def _case(seed):
    net, mask_u8 = _fixed_net(B, S)
    photos = np.random.default_rng(seed).integers(0, 256, (P, HP, WP, 3), dtype=np.uint8)
    return net, mask_u8, photos


def _pass(net, x, mask_u8, lights):
    from geomconsistentfr_amd import inference as inf
    m = torch.from_numpy(mask_u8).to(DEV)
    with torch.no_grad():
        return net.forward_lights(x, 200, inf.camera_matrix(1570.0, S, S), (m.to(torch.float64).reshape(S, S, 1) / 255.0),
                                  torch.from_numpy(lights).to(DEV)), m


def test_the_lights_entry_is_its_own_stages_chained_by_hand():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(51)
    relit = group.relit_counts(BOXES, INDEX, mask_u8[None], P, HP, WP, S, S)
    assert (relit[0] == 2).any() and (relit == 1).any() and (relit == 0).any()     # two faces of photograph 0 relight some pixels
    got = inf.relight_lights_in_group_photograph_device(net, photos, BOXES, INDEX, mask_u8, LIGHTS, device=DEV)
    assert tuple(got.shape) == (P, 3, HP, WP, 3) and got.dtype == torch.uint8
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_group_device(p, BOXES, INDEX, (S, S))
    assert tuple(x.shape) == (B, S, S, 3)
    out, m = _pass(net, x, mask_u8, LIGHTS)
    want = pp.fullres_group_composites_device(p, BOXES, INDEX, x, out[5], m)
    assert torch.equal(got, want)
    # and the chain of the any-size entry over the faces, per photograph
    run = p[:, None].repeat(1, 3, 1, 1, 1)
    for b, q in enumerate(INDEX):
        run[q] = pp.fullres_anybox_composites_device(run[q], tuple(int(v) for v in BOXES[b]), x[b:b + 1].expand(3, -1, -1, -1),
                                                     out[5][b].contiguous(), m)
    assert torch.equal(got, run)
    # the faces are relit and differ between lights; where no face relights a pixel the photograph is returned
    g = got.cpu().numpy()
    assert (g[:, 0] != g[:, 1]).any() and (g[0, 0] != photos[0]).any() and (g[1, 0] != photos[1]).any()
    for l in range(3):
        np.testing.assert_array_equal(g[:, l][relit == 0], photos[relit == 0])
    host = inf.relight_lights_in_group_photograph(net, photos, BOXES.tolist(), np.array(INDEX), mask_u8, LIGHTS, device=DEV)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, g)
    # a second compositing mask, other clamp and floor: passed through
    cm = np.where(mask_u8 > 0, 255, 0).astype(np.uint8)
    got2 = inf.relight_lights_in_group_photograph_device(net, photos, BOXES, INDEX, mask_u8, LIGHTS, device=DEV, composite_mask_u8=cm,
                                                         detail_clamp=2.0, floor=4.0)
    want2 = pp.fullres_group_composites_device(p, BOXES, INDEX, x, out[5], torch.from_numpy(cm).to(DEV), detail_clamp=2.0, floor=4.0)
    assert torch.equal(got2, want2)


def test_the_rig_entry_with_one_white_light_is_the_first_light():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import postprocess as pp
    net, mask_u8, photos = _case(53)
    white = np.ones((1, 3), np.float32)
    rig = inf.relight_rig_in_group_photograph(net, photos, BOXES, INDEX, mask_u8, LIGHTS[:1], white, device=DEV)
    assert rig.shape == (P, HP, WP, 3) and rig.dtype == np.uint8
    np.testing.assert_array_equal(rig, inf.relight_lights_in_group_photograph(net, photos, BOXES, INDEX, mask_u8, LIGHTS[:1], device=DEV)[:, 0])
    # a coloured rig of three lights: the rig stage's `rendered` at L = 1 through the same launch
    rgb = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)
    got = inf.relight_rig_in_group_photograph_device(net, photos, BOXES, INDEX, mask_u8, LIGHTS, rgb, device=DEV)
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_group_device(p, BOXES, INDEX, (S, S))
    out, m = _pass(net, x, mask_u8, LIGHTS)
    rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(rgb).to(DEV)[None])
    assert torch.equal(got, pp.fullres_group_composites_device(p, BOXES, INDEX, x, rendered, m))
    assert (got.cpu().numpy() != rig).any()
    np.testing.assert_array_equal(inf.relight_rig_in_group_photograph(net, photos, BOXES, INDEX, mask_u8, LIGHTS, rgb, device=DEV), got.cpu().numpy())


def test_a_single_photograph_with_no_index():
    from geomconsistentfr_amd import inference as inf
    net, mask_u8, photos = _case(54)
    one = inf.relight_lights_in_group_photograph_device(net, photos[0], BOXES, None, mask_u8, LIGHTS, device=DEV)
    assert tuple(one.shape) == (1, 3, HP, WP, 3)
    assert torch.equal(one, inf.relight_lights_in_group_photograph_device(net, photos[:1], BOXES, [0, 0, 0], mask_u8, LIGHTS, device=DEV))
    assert (one.cpu().numpy()[0, 0] != photos[0]).any()
    rig = inf.relight_rig_in_group_photograph(net, photos[0], BOXES, None, mask_u8, LIGHTS[:1], np.ones((1, 3), np.float32), device=DEV)
    np.testing.assert_array_equal(rig, one.cpu().numpy()[:, 0])
