"""GPU: the inference entries of the any-size box feature (inference.relight_lights_in_photograph_anybox(_device),
relight_rig_in_photograph_anybox(_device)) against the steps they are made of, on FIXED head outputs (test_gpu_light_rig._fixed_net,
as tests/test_gpu_fullres_box_inference.py).  The network runs at 64 x 64; the photographs are 90 x 101 with, per case, one box per
face that is smaller than the network on both axes (40 x 36) or wide and flat (75 x 9: the columns are lerped, the rows averaged)."""
import numpy as np
import pytest
import torch

from test_gpu_light_rig import _fixed_net

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, S = 2, 64
HP, WP = 90, 101
CASES = {"small": np.array([(11, 40, 40, 36), (60, 3, 40, 36)]), "mixed": np.array([(11, 40, 75, 9), (26, 3, 75, 9)])}   # (x0, y0, bw, bh)
LIGHTS = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)


def _case(seed):
    net, mask_u8 = _fixed_net(B, S)
    photos = np.random.default_rng(seed).integers(0, 256, (B, HP, WP, 3), dtype=np.uint8)
    return net, mask_u8, photos


def _pass(net, x, mask_u8, lights):
    from geomconsistentfr_amd import inference as inf
    m = torch.from_numpy(mask_u8).to(DEV)
    with torch.no_grad():
        return net.forward_lights(x, 200, inf.camera_matrix(1570.0, S, S), (m.to(torch.float64).reshape(S, S, 1) / 255.0),
                                  torch.from_numpy(lights).to(DEV)), m


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_lights_entry_is_its_own_stages_chained_by_hand(case):
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    import fullres_anybox_emulation as anybox
    boxes = CASES[case]
    net, mask_u8, photos = _case(41)
    got = inf.relight_lights_in_photograph_anybox_device(net, photos, boxes, mask_u8, LIGHTS, device=DEV)
    assert tuple(got.shape) == (B, 3, HP, WP, 3) and got.dtype == torch.uint8
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_anybox_device(p, boxes, (S, S))
    out, m = _pass(net, x, mask_u8, LIGHTS)
    want = pp.fullres_anybox_composites_device(p, boxes, x, out[5], m)
    assert torch.equal(got, want)
    # the face is relit and differs between lights; outside the box and the carried mask the photograph is returned
    g = got.cpu().numpy()
    assert (g[:, 0] != g[:, 1]).any() and (g[:, 0] != photos).any()
    relit = np.zeros((B, HP, WP), bool)
    for b, (x0, y0, bw, bh) in enumerate(boxes):
        relit[b, y0:y0 + bh, x0:x0 + bw] = anybox.carry(mask_u8.astype(np.float32) / np.float32(255.0), bh, bw) > 0
    assert relit.any() and not relit.all()
    for l in range(3):
        np.testing.assert_array_equal(g[:, l][~relit], photos[~relit])
    host = inf.relight_lights_in_photograph_anybox(net, photos, boxes.tolist(), mask_u8, LIGHTS, device=DEV)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, g)
    # a second compositing mask, other clamp and floor: passed through
    cm = np.where(mask_u8 > 0, 255, 0).astype(np.uint8)
    got2 = inf.relight_lights_in_photograph_anybox_device(net, photos, boxes, mask_u8, LIGHTS, device=DEV, composite_mask_u8=cm,
                                                          detail_clamp=2.0, floor=4.0)
    want2 = pp.fullres_anybox_composites_device(p, boxes, x, out[5], torch.from_numpy(cm).to(DEV), detail_clamp=2.0, floor=4.0)
    assert torch.equal(got2, want2)


@pytest.mark.parametrize("case", sorted(CASES))
def test_paste_false_is_the_box_cut_out_of_paste_true(case):
    from geomconsistentfr_amd import inference as inf
    boxes = CASES[case]
    net, mask_u8, photos = _case(42)
    full = inf.relight_lights_in_photograph_anybox_device(net, photos, boxes, mask_u8, LIGHTS, device=DEV)
    alone = inf.relight_lights_in_photograph_anybox_device(net, photos, boxes, mask_u8, LIGHTS, device=DEV, paste=False)
    assert tuple(alone.shape) == (B, 3, int(boxes[0, 3]), int(boxes[0, 2]), 3)
    for b, (x0, y0, bw, bh) in enumerate(boxes):
        assert torch.equal(alone[b], full[b, :, y0:y0 + bh, x0:x0 + bw])
    x0, y0, bw, bh = boxes[0]
    assert (alone.cpu().numpy()[0] != photos[0, y0:y0 + bh, x0:x0 + bw]).any()


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_rig_entry_with_one_white_light_is_the_first_light(case):
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import postprocess as pp
    boxes = CASES[case]
    net, mask_u8, photos = _case(43)
    white = np.ones((1, 3), np.float32)
    for paste in (True, False):
        rig = inf.relight_rig_in_photograph_anybox(net, photos, boxes, mask_u8, LIGHTS[:1], white, device=DEV, paste=paste)
        assert rig.shape == ((B, HP, WP, 3) if paste else (B, int(boxes[0, 3]), int(boxes[0, 2]), 3)) and rig.dtype == np.uint8
        np.testing.assert_array_equal(rig, inf.relight_lights_in_photograph_anybox(net, photos, boxes, mask_u8, LIGHTS[:1], device=DEV,
                                                                                   paste=paste)[:, 0])
    # a coloured rig of three lights: the rig stage's `rendered` at L = 1 through the same launch
    rgb = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)
    got = inf.relight_rig_in_photograph_anybox_device(net, photos, boxes, mask_u8, LIGHTS, rgb, device=DEV)
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_anybox_device(p, boxes, (S, S))
    out, m = _pass(net, x, mask_u8, LIGHTS)
    rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(rgb).to(DEV)[None])
    assert torch.equal(got, pp.fullres_anybox_composites_device(p, boxes, x, rendered, m))
    assert (got.cpu().numpy() != inf.relight_rig_in_photograph_anybox(net, photos, boxes, mask_u8, LIGHTS[:1], white, device=DEV)).any()
