"""GPU: the inference entries of the group-affine feature (inference.relight_lights_in_group_photograph_affine(_device),
relight_rig_in_group_photograph_affine(_device)) against the steps they are made of: ingest, the lights pass, composite.  The network
is a RelightNetSingleImage with tests/seeded_init.py's weights at its own 256 x 256 (the hourglass takes no other size).  MIOpen's
convolutions are not run-to-run reproducible, so the heads' outputs for one input are computed ONCE and replayed for the same input,
as tests/test_gpu_fullres_affine_inference.py does: an entry and its by-hand sequence then see the same heads exactly when they ingest
the same bits.  ONE photograph of 300 x 340 carries three tilted faces that overlap: 30 degrees at scale 1.2 (it hangs over the
edges), -40 degrees at scale 0.7 (the composite's K = 2) and exactly 90 degrees at scale 0.5."""
import numpy as np
import pytest
import torch

from test_gpu_fullres_affine_inference import DEV, LIGHTS, S, _net, _pass

pytestmark = pytest.mark.gpu
B = 3
HP, WP = 300, 340
FACES = ((170.0, 150.0, 1.2, 30.0), (200.0, 140.0, 0.7, -40.0), (120.0, 170.0, 0.5, 90.0))      # (cx, cy, scale, degrees)
PIDX = [0, 0, 0]


def _case(seed):
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(seed)
    # a smooth photograph (a random field blurred by repetition), so that the heads see an image and not noise
    photo = np.repeat(np.repeat(rng.integers(0, 256, (HP // 6 + 1, WP // 6 + 1, 3), dtype=np.uint8), 6, axis=0), 6, axis=1)[:HP, :WP]
    photo = np.ascontiguousarray(photo)
    A = np.stack([pp.affine_from_rotated_box(cx, cy, s * S, s * S, deg, S) for cx, cy, s, deg in FACES])
    yy, xx = np.mgrid[0:S, 0:S]
    mask_u8 = np.where((yy - S / 2.0) ** 2 / (0.42 * S) ** 2 + (xx - S / 2.0) ** 2 / (0.33 * S) ** 2 <= 1.0, 255, 0).astype(np.uint8)
    return photo, A, mask_u8


def test_the_four_entries_are_their_own_stages_chained_by_hand():
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    import fullres_affine_emulation as affine
    import fullres_group_affine_emulation as tilted
    net = _net()
    photo, A, mask_u8 = _case(43)
    got = inf.relight_lights_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, LIGHTS, device=DEV)
    assert tuple(got.shape) == (1, 3, HP, WP, 3) and got.dtype == torch.uint8
    p = torch.from_numpy(photo).to(DEV)[None]
    x = pp.ingest_group_affine_device(p, A, PIDX, (S, S))
    assert tuple(x.shape) == (B, S, S, 3)
    out, m = _pass(net, x, mask_u8, LIGHTS)                                        # the network runs once on all B faces
    want = pp.fullres_group_affine_composites_device(p, A, PIDX, x, out[5], m)
    assert torch.equal(got, want)
    # every face is relit, the faces overlap, and outside the quads and the carried masks the photograph is returned
    g = got.cpu().numpy()
    assert (g[:, 0] != g[:, 1]).any() and (g[:, 0] != photo[None]).any()
    _, I = affine.quantise(A)
    assert [affine.sub_samples(i) for i in I] == [1, 2, 2]
    relit = tilted.relit_counts(I, PIDX, mask_u8[None], 1, HP, WP, S, S)
    assert (relit >= 2).any() and (relit == 1).any() and (relit == 0).any()
    for b in range(B):
        assert (tilted.relit_counts(I[b:b + 1], [0], mask_u8[None], 1, HP, WP, S, S) == 1).any()
    for l in range(3):
        np.testing.assert_array_equal(g[:, l][relit == 0], photo[None][relit == 0])
    # photo_index=None: every face in the one photograph; the host entry; the integer pair in the place of the matrix
    assert torch.equal(inf.relight_lights_in_group_photograph_affine_device(net, photo, A, None, mask_u8, LIGHTS, device=DEV), got)
    host = inf.relight_lights_in_group_photograph_affine(net, photo[None], A.tolist(), PIDX, mask_u8, LIGHTS, device=DEV)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, g)
    pair = pp.quantise_affine(A)
    assert torch.equal(inf.relight_lights_in_group_photograph_affine_device(net, photo, pair, PIDX, mask_u8, LIGHTS, device=DEV), got)
    # a second compositing mask, other clamp and floor: passed through
    cm = np.where(mask_u8 > 0, 128, 0).astype(np.uint8)
    got2 = inf.relight_lights_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, LIGHTS, device=DEV, composite_mask_u8=cm,
                                                                detail_clamp=2.0, floor=4.0)
    assert torch.equal(got2, pp.fullres_group_affine_composites_device(p, A, PIDX, x, out[5], torch.from_numpy(cm).to(DEV),
                                                                       detail_clamp=2.0, floor=4.0))
    # the rig entries: one white light is the first light; a coloured rig is the rig stage's `rendered` through the same launch
    white = np.ones((1, 3), np.float32)
    rig = inf.relight_rig_in_group_photograph_affine(net, photo, A, PIDX, mask_u8, LIGHTS[:1], white, device=DEV)
    assert rig.shape == (1, HP, WP, 3) and rig.dtype == np.uint8
    np.testing.assert_array_equal(rig, inf.relight_lights_in_group_photograph_affine(net, photo, A, PIDX, mask_u8, LIGHTS[:1], device=DEV)[:, 0])
    rgb = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)
    got3 = inf.relight_rig_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, LIGHTS, rgb, device=DEV)
    rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(rgb).to(DEV)[None])
    assert torch.equal(got3, pp.fullres_group_affine_composites_device(p, A, PIDX, x, rendered, m))
    assert (got3.cpu().numpy() != rig).any()


def test_lights_in_the_photographs_frame_are_each_faces_lights_turned_by_hand():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    net = _net()
    photo, A, mask_u8 = _case(44)
    _, I = pp.quantise_affine(A)
    # by hand, in f64, per face: the angle's cosine and sine from the integers the composite reads; y is up in the lights' frame
    turned = np.empty((B, 3, 3), np.float32)
    for b in range(B):
        si, co = float(I[b, 1, 0] - I[b, 0, 1]), float(I[b, 0, 0] + I[b, 1, 1])
        n = np.hypot(si, co)
        si, co = si / n, co / n
        assert abs(np.degrees(np.arctan2(si, co)) + FACES[b][3]) < 0.01            # the map photograph -> network turns back by the face's angle
        x, y = LIGHTS[:, 0].astype(np.float64), LIGHTS[:, 1].astype(np.float64)
        turned[b] = np.stack([co * x + si * y, co * y - si * x, LIGHTS[:, 2].astype(np.float64)], -1).astype(np.float32)
    assert np.abs(turned[0] - turned[1]).max() > 0.3 and np.abs(turned[1] - turned[2]).max() > 0.3   # every head gets its own copy
    got = inf.relight_lights_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, LIGHTS, device=DEV, light_frame="photograph")
    want = inf.relight_lights_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, turned, device=DEV, light_frame="face")
    assert torch.equal(got, want)
    plain = inf.relight_lights_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, LIGHTS, device=DEV)
    assert (got != plain).any()
    white = np.ones((1, 3), np.float32)
    rig = inf.relight_rig_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, LIGHTS[:1], white, device=DEV, light_frame="photograph")
    assert torch.equal(rig, inf.relight_rig_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, turned[:, :1], white, device=DEV))
    with pytest.raises(GcfrError, match="light_frame"):
        inf.relight_lights_in_group_photograph_affine_device(net, photo, A, PIDX, mask_u8, LIGHTS, device=DEV, light_frame="camera")
    with pytest.raises(GcfrError, match="HOST"):
        inf.relight_lights_in_group_photograph_affine_device(net, photo, torch.from_numpy(A).to(DEV), PIDX, mask_u8, LIGHTS, device=DEV)
    with pytest.raises(GcfrError, match="HOST"):
        inf.relight_lights_in_group_photograph_affine_device(net, photo, A, torch.tensor(PIDX).to(DEV), mask_u8, LIGHTS, device=DEV)
