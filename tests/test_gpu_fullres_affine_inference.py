"""GPU: the inference entries of the rotated-face feature (inference.relight_lights_in_photograph_affine(_device),
relight_rig_in_photograph_affine(_device)) against the steps they are made of: ingest, the lights pass, composite.  The network is
a RelightNetSingleImage with tests/seeded_init.py's weights at its own 256 x 256 (the hourglass takes no other size).  MIOpen's convolutions are not run-to-run reproducible, so
the heads' outputs for one input are computed ONCE and replayed for the same input (the stage, the block and the kernels are
reproducible): an entry and its by-hand sequence then see the same heads exactly when they ingest the same bits.  The photographs
are 300 x 340 with one tilted face each: 30 degrees at scale 1.2 (it hangs over the edges) and -40 degrees at scale 0.7 (the composite's K = 2)."""
import numpy as np
import pytest
import torch

from seeded_init import SEED_G, seeded_init_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, S = 2, 256
HP, WP = 300, 340
ANGLES, SCALES = (30.0, -40.0), (1.2, 0.7)
LIGHTS = np.asarray([(0.7518, 0.0, 0.6594), (-0.5843, 0.0, 0.8115), (0.0, 0.7071, 0.7071)], np.float32)
_NET = []


def _net():
    """the seeded network, built once; features() replays the heads it computed for the same input bits"""
    from geomconsistentfr_amd.relightnet import RelightNetSingleImage
    if _NET:
        return _NET[0]

    class Replayed(RelightNetSingleImage):
        heads = {}

        def features(self, img, epoch, on_depth=None):
            key = img.detach().cpu().numpy().tobytes()
            if key not in self.heads:
                fresh = super().features(img, epoch, None)
                self.heads[key] = [t.clone() for t in fresh]
            a, d, SL = [t.clone() for t in self.heads[key]]
            if on_depth is not None:
                on_depth(d, SL)
            return a, d, SL

    _NET.append(seeded_init_(Replayed(img_height=S, img_width=S), SEED_G).to(DEV).eval())
    return _NET[0]


def _case(seed):
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(seed)
    # smooth photographs (a random field blurred by repetition), so that the heads see an image and not noise
    photos = np.repeat(np.repeat(rng.integers(0, 256, (B, HP // 6 + 1, WP // 6 + 1, 3), dtype=np.uint8), 6, axis=1), 6, axis=2)[:, :HP, :WP]
    photos = np.ascontiguousarray(photos)
    A = np.stack([pp.affine_from_rotated_box(170.0, 150.0, s * S, s * S, deg, S) for deg, s in zip(ANGLES, SCALES)])
    yy, xx = np.mgrid[0:S, 0:S]
    mask_u8 = np.where((yy - S / 2.0) ** 2 / (0.42 * S) ** 2 + (xx - S / 2.0) ** 2 / (0.33 * S) ** 2 <= 1.0, 255, 0).astype(np.uint8)
    return photos, A, mask_u8


def _pass(net, x, mask_u8, lights):
    from geomconsistentfr_amd import inference as inf
    m = torch.from_numpy(mask_u8).to(DEV)
    lights = lights if torch.is_tensor(lights) else torch.from_numpy(lights).to(DEV)
    with torch.no_grad():
        return net.forward_lights(x, 200, inf.camera_matrix(1570.0, S, S), (m.to(torch.float64).reshape(S, S, 1) / 255.0), lights), m


def test_the_four_entries_are_their_own_stages_chained_by_hand():
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    import fullres_affine_emulation as affine
    net = _net()
    photos, A, mask_u8 = _case(41)
    got = inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, LIGHTS, device=DEV)
    assert tuple(got.shape) == (B, 3, HP, WP, 3) and got.dtype == torch.uint8
    p = torch.from_numpy(photos).to(DEV)
    x = pp.ingest_affine_device(p, A, (S, S))
    out, m = _pass(net, x, mask_u8, LIGHTS)
    want = pp.fullres_affine_composites_device(p, A, x, out[5], m)
    assert torch.equal(got, want)
    # the face is relit and differs between lights; outside the quad and the carried mask the photograph is returned
    g = got.cpu().numpy()
    assert (g[:, 0] != g[:, 1]).any() and (g[:, 0] != photos).any()
    _, I = affine.quantise(A)
    assert [affine.sub_samples(i) for i in I] == [1, 2]
    relit = np.stack([affine.inside(I[b], HP, WP, S, S) & (affine.carry(mask_u8.astype(np.float32) / np.float32(255.0), I[b], HP, WP) > 0)
                      for b in range(B)])
    assert relit.any() and not relit.all()
    for l in range(3):
        np.testing.assert_array_equal(g[:, l][~relit], photos[~relit])
    host = inf.relight_lights_in_photograph_affine(net, photos, A.tolist(), mask_u8, LIGHTS, device=DEV)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, g)
    # the integer pair in the place of the matrix; a second compositing mask, other clamp and floor: passed through
    pair = pp.quantise_affine(A)
    assert torch.equal(inf.relight_lights_in_photograph_affine_device(net, photos, pair, mask_u8, LIGHTS, device=DEV), got)
    cm = np.where(mask_u8 > 0, 128, 0).astype(np.uint8)
    got2 = inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, LIGHTS, device=DEV, composite_mask_u8=cm,
                                                          detail_clamp=2.0, floor=4.0)
    assert torch.equal(got2, pp.fullres_affine_composites_device(p, A, x, out[5], torch.from_numpy(cm).to(DEV), detail_clamp=2.0, floor=4.0))
    # the rig entries: one white light is the first light; a coloured rig is the rig stage's `rendered` through the same launch
    white = np.ones((1, 3), np.float32)
    rig = inf.relight_rig_in_photograph_affine(net, photos, A, mask_u8, LIGHTS[:1], white, device=DEV)
    assert rig.shape == (B, HP, WP, 3) and rig.dtype == np.uint8
    np.testing.assert_array_equal(rig, inf.relight_lights_in_photograph_affine(net, photos, A, mask_u8, LIGHTS[:1], device=DEV)[:, 0])
    rgb = np.asarray([(0.6, 0.5, 0.4), (0.1, 0.2, 0.4), (0.3, 0.3, 0.2)], np.float32)
    got3 = inf.relight_rig_in_photograph_affine_device(net, photos, A, mask_u8, LIGHTS, rgb, device=DEV)
    rendered, _ = combine_lights(out[8], out[0], torch.from_numpy(rgb).to(DEV)[None])
    assert torch.equal(got3, pp.fullres_affine_composites_device(p, A, x, rendered, m))
    assert (got3.cpu().numpy() != rig).any()


def test_lights_in_the_photographs_frame_are_the_faces_lights_turned_by_hand():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    net = _net()
    photos, A, mask_u8 = _case(42)
    _, I = pp.quantise_affine(A)
    # by hand, in f64: the angle's cosine and sine from the integers the composite reads; y is up in the lights' frame
    turned = np.empty((B, 3, 3), np.float32)
    for b in range(B):
        si, co = float(I[b, 1, 0] - I[b, 0, 1]), float(I[b, 0, 0] + I[b, 1, 1])
        n = np.hypot(si, co)
        si, co = si / n, co / n
        assert abs(np.degrees(np.arctan2(si, co)) + ANGLES[b]) < 0.01            # the map photograph -> network turns back by the face's angle
        x, y = LIGHTS[:, 0].astype(np.float64), LIGHTS[:, 1].astype(np.float64)
        turned[b] = np.stack([co * x + si * y, co * y - si * x, LIGHTS[:, 2].astype(np.float64)], -1).astype(np.float32)
    assert np.abs(turned[0] - LIGHTS).max() > 0.3                                  # 30 degrees is not a nuance
    got = inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, LIGHTS, device=DEV, light_frame="photograph")
    want = inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, turned, device=DEV, light_frame="face")
    assert torch.equal(got, want)
    plain = inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, LIGHTS, device=DEV)
    assert (got != plain).any()
    # (B,L,3) lights in the photograph's frame, on the device; the rig entry takes the keyword too
    per_face = torch.from_numpy(np.stack([LIGHTS, LIGHTS[::-1].copy()])).to(DEV)
    got = inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, per_face, device=DEV, light_frame="photograph")
    hand = torch.from_numpy(np.stack([turned[0], turned[1][::-1].copy()])).to(DEV)
    assert torch.equal(got, inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, hand, device=DEV))
    white = np.ones((1, 3), np.float32)
    rig = inf.relight_rig_in_photograph_affine_device(net, photos, A, mask_u8, LIGHTS[:1], white, device=DEV, light_frame="photograph")
    assert torch.equal(rig, inf.relight_rig_in_photograph_affine_device(net, photos, A, mask_u8, turned[:, :1], white, device=DEV))
    with pytest.raises(GcfrError, match="light_frame"):
        inf.relight_lights_in_photograph_affine_device(net, photos, A, mask_u8, LIGHTS, device=DEV, light_frame="camera")
    with pytest.raises(GcfrError, match="HOST"):
        inf.relight_lights_in_photograph_affine_device(net, photos, torch.from_numpy(A).to(DEV), mask_u8, LIGHTS, device=DEV)
