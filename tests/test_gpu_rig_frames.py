"""GPU: the rig-frames kernel (csrc/gcfr_rig_frames.hip; lighting.rig_frames_u8) byte for byte against the two-stage path it fuses
-- lighting.combine_lights with rig f, then postprocess.inference_images_device -- and against the numpy statement
(tests/rig_frames_emulation.py: the rig stage's restatement, then the scripts' paste and cv2's quantisation).

  shapes   one pixel; an odd plane (the element path) with a remainder in the light loop's unrolling; frame counts around the
           kernel's frame tile (lighting.RIG_FRAMES_TILE) on the vector path; more lights than any unrolling, two frames.
  inputs   rigs and masks shared or per face, mask values {0, 1, 128, 255}, the mask's quotient in f64 and in f32, every operand
           and the output off its alignment, a negative rig (bytes 0), a large one (bytes 255), a NaN (byte 0 in its pixel only),
           `out=` between guard bands, a side stream, a captured graph whose rig buffer is refilled between replays, two calls.
  identity one white light, one frame: the many-lights path's own composite."""
import numpy as np
import pytest
import torch

import rig_frames_emulation as emu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _tile():
    from geomconsistentfr_amd import lighting
    return lighting.RIG_FRAMES_TILE


def _inputs(seed, B, L, F, H, W, shared_rig, shared_mask, scale=0.6):
    rng = np.random.default_rng(seed)
    final = (0.2 + rng.random((B, L, H, W))).astype(np.float32)
    albedo = (0.1 + 0.8 * rng.random((B, 3, H, W))).astype(np.float32)
    images = rng.random((B, H, W, 3), dtype=np.float32)
    MB = 1 if shared_mask else B
    mask = np.resize(np.array([255, 0, 1, 128], np.uint8), MB * H * W)             # all four values as soon as there are four pixels
    if H * W >= 4:
        mask = np.stack([rng.permutation(m) for m in mask.reshape(MB, H * W)])
    mask = mask.reshape(MB, H, W)
    rgb = (scale * rng.standard_normal((1 if shared_rig else B, F, L, 3)) / np.sqrt(L)).astype(np.float32)
    rgb[:, :, :, 0] += np.float32(1.0 / L)                                        # red around 1 x albedo x final: bytes across the range
    return final, albedo, images, mask, rgb


def _dev(a, misalign=False):
    """a device tensor of `a`; misalign: its first element sits one element past an aligned allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.to(DEV)
    buf = torch.empty(a.size + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(a.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _two_stage(final, albedo, images, mask, rgb, mask_f32):
    """the path the kernel fuses, on device tensors: per frame the rig stage, then the image kernel at one image per photograph"""
    from geomconsistentfr_amd import combine_lights
    from geomconsistentfr_amd import postprocess as pp
    frames = []
    for f in range(rgb.shape[1]):
        rendered, _ = combine_lights(final, albedo, rgb[:, f].contiguous())
        frames.append(pp.inference_images_device(images, rendered, mask, mask_f32=mask_f32)["rendered_image"])
    return torch.stack(frames, dim=1)


def _check(label, arrays, mask_f32, misalign=(), **kw):
    from geomconsistentfr_amd import rig_frames_u8
    names = ("final", "albedo", "images", "mask", "rgb")
    t = {n: _dev(a, n in misalign) for n, a in zip(names, arrays)}
    got = rig_frames_u8(t["final"], t["albedo"], t["images"], t["mask"], t["rgb"], mask_f32=mask_f32, **kw)
    two = _two_stage(t["final"], t["albedo"], t["images"], t["mask"], t["rgb"], mask_f32)
    want = emu.frames(*arrays, mask_f32)
    g = got.cpu().numpy()
    B, L, H, W = arrays[0].shape
    assert g.shape == (B, arrays[4].shape[1], H, W, 3) and g.dtype == np.uint8
    print("%s: bytes that differ from the two-stage path %d, from the statement %d, of %d"
          % (label, int((g != two.cpu().numpy()).sum()), int((g != want).sum()), g.size))
    assert torch.equal(got, two), label
    np.testing.assert_array_equal(g, want, err_msg=label)
    return got, t


def _shapes():
    Ft = _tile()
    return [(1, 1, 1, 1, 1), (2, 5, 3, 5, 7)] + [(3, 9, F, 8, 12) for F in sorted({1, Ft - 1, Ft, Ft + 1, 2 * Ft + 1} - {0})] + [(1, 65, 2, 16, 16)]


SHAPES = _shapes()


@pytest.mark.parametrize("mask_f32", [False, True])
@pytest.mark.parametrize("B,L,F,H,W", SHAPES)
def test_frames_equal_the_two_stage_path_and_the_statement(B, L, F, H, W, mask_f32):
    case = SHAPES.index((B, L, F, H, W))
    shared_rig, shared_mask = case % 2 == 0, case % 3 == 0
    arrays = _inputs(10 * case + F, B, L, F, H, W, shared_rig, shared_mask)
    if H * W >= 4:
        assert set(np.unique(arrays[3])) == {0, 1, 128, 255}
    got, _ = _check("(%d,%d,%d,%d,%d)" % (B, L, F, H, W), arrays, mask_f32)
    if F > 1 and H * W >= 35:
        assert not torch.equal(got[:, 0], got[:, 1])


@pytest.mark.parametrize("shared_rig", [True, False])
@pytest.mark.parametrize("shared_mask", [True, False])
def test_rigs_and_masks_shared_or_per_face(shared_rig, shared_mask):
    B, L, F, H, W = 3, 9, _tile() + 1, 8, 12
    for mask_f32 in (False, True):
        got, _ = _check("shared rig %s, shared mask %s" % (shared_rig, shared_mask),
                        _inputs(3, B, L, F, H, W, shared_rig, shared_mask), mask_f32)
    assert not torch.equal(got[0], got[1])


@pytest.mark.parametrize("which", ["final", "albedo", "images", "mask", "rgb", "out", "all"])
def test_every_operand_off_its_alignment(which):
    """H W = 96 is a multiple of four: aligned, this shape takes the vector path; one operand one element off, and the element path
    must return the same bytes"""
    B, L, F, H, W = 3, 9, _tile() + 1, 8, 12
    arrays = _inputs(4, B, L, F, H, W, False, False)
    mis = ("final", "albedo", "images", "mask", "rgb") if which == "all" else (which,)
    kw = {}
    if which in ("out", "all"):
        buf = torch.full((B * F * H * W * 3 + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        kw["out"] = buf[1:].view(B, F, H, W, 3)
        assert kw["out"].data_ptr() % 4 == 1
    got, _ = _check("misaligned " + which, arrays, which in ("mask", "all"), misalign=mis, **kw)
    if kw:
        assert got.data_ptr() == kw["out"].data_ptr() and int(buf[0]) == 0xAB


def test_a_negative_rig_gives_zeros_and_a_large_one_255():
    B, L, F, H, W = 2, 5, 2, 8, 12
    final, albedo, images, mask, rgb = _inputs(5, B, L, F, H, W, True, True)
    rgb[:, 0] = -np.abs(rgb[:, 0]) - np.float32(0.01)
    rgb[:, 1] = np.float32(100.0)
    got, _ = _check("negative / large", (final, albedo, images, mask, rgb), False)
    g = got.cpu().numpy()
    inside, full = mask[0] > 0, mask[0] == 255
    assert (g[:, 0][:, inside] == 0).all() and (g[:, 1][:, full] == 255).all()
    keep = emu.pps.to_uint8(images.astype(np.float64) * 255.0)
    np.testing.assert_array_equal(g[:, 0][:, ~inside], keep[:, ~inside])


@pytest.mark.parametrize("H,W", [(5, 7), (8, 12)])
def test_one_nan_gives_zero_in_its_pixel_of_every_frame_and_nowhere_else(H, W):
    B, L, F = 2, 5, _tile() + 1
    final, albedo, images, mask, rgb = _inputs(6, B, L, F, H, W, False, True)
    rgb[:, 1, 2] = 0.0                                                            # 0 * NaN is NaN as well
    (y0, x0), (y1, x1) = (H // 2, W - 1), (1, 2)
    mask[0, y0, x0], mask[0, y1, x1] = 128, 0                                     # pasted / kept
    clean, _ = _check("before the NaN", (final, albedo, images, mask, rgb), False)
    final[1, 2, y0, x0] = np.nan
    final[0, 4, y1, x1] = np.nan                                                  # under a mask of 0: the photograph is kept
    got, _ = _check("NaN", (final, albedo, images, mask, rgb), False)
    g, c = got.cpu().numpy(), clean.cpu().numpy()
    assert (g[1, :, y0, x0] == 0).all() and (c[1, :, y0, x0, 0] > 0).any()
    c[1, :, y0, x0] = 0
    np.testing.assert_array_equal(g, c)


@pytest.mark.parametrize("H,W", [(5, 7), (8, 12)])
def test_out_is_written_in_place_between_untouched_guard_bands(H, W):
    from geomconsistentfr_amd import rig_frames_u8
    B, L, F = 2, 5, _tile() + 1
    arrays = _inputs(7, B, L, F, H, W, True, False)
    n = B * F * H * W * 3
    buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(B, F, H, W, 3)
    got, t = _check("out=", arrays, True, out=out)
    assert got.data_ptr() == out.data_ptr() and (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all()
    again = rig_frames_u8(t["final"], t["albedo"], t["images"], t["mask"], t["rgb"], mask_f32=True)      # two calls: the same bytes
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)


def test_a_side_stream():
    from geomconsistentfr_amd import rig_frames_u8
    arrays = _inputs(8, 2, 5, 3, 8, 12, False, False)
    t = [_dev(a) for a in arrays]
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = rig_frames_u8(*t)
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), emu.frames(*arrays, False))


def test_a_captured_graph_whose_rig_buffer_is_refilled_between_replays():
    """one stream, one kernel node: the machine's default number of hardware queues"""
    from geomconsistentfr_amd import rig_frames_u8
    B, L, F, H, W = 2, 5, _tile() + 1, 8, 12
    arrays = _inputs(9, B, L, F, H, W, False, True)
    final, albedo, images, mask, rgb = [_dev(a) for a in arrays]
    out = torch.zeros((B, F, H, W, 3), dtype=torch.uint8, device=DEV)
    rig_frames_u8(final, albedo, images, mask, rgb, out=out)                      # outside the capture: the library is loaded
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig_frames_u8(final, albedo, images, mask, rgb, out=out)
    seen = []
    for k in range(2):
        new = arrays[4] * np.float32(1.0 - 0.5 * k) + np.float32(0.05 * k)
        rgb.copy_(torch.from_numpy(new))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(DEV)
        np.testing.assert_array_equal(out.cpu().numpy(), emu.frames(*arrays[:4], new, False))
        seen.append(out.cpu().numpy())
    assert (seen[0] != seen[1]).any()


def test_one_white_light_and_one_frame_is_the_many_lights_composite():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd import rig_frames_u8
    from test_gpu_light_rig import _fixed_net
    B, S = 2, 64
    net, mask_u8 = _fixed_net(B, S)
    x = torch.from_numpy(np.random.default_rng(2).random((B, S, S, 3), dtype=np.float32)).to(DEV)
    m = torch.from_numpy(mask_u8).to(DEV)
    light = torch.tensor([[-0.5843, 0.0, 0.8115]], device=DEV)
    with torch.no_grad():
        out = net.forward_lights(x, 200, inf.camera_matrix(1570.0, S, S), (m.to(torch.float64).reshape(S, S, 1) / 255.0), light)
    want = pp.inference_images_device(x, out[5], m)["rendered_image"]             # (B,1,H,W,3): relight_lights' composite path
    got = rig_frames_u8(out[8], out[0], x, m, torch.ones(1, 1, 1, 3, device=DEV))
    assert tuple(got.shape) == (B, 1, S, S, 3) and torch.equal(got, want) and got.float().std() > 10


@pytest.mark.parametrize("mask_f32", [False, True])
def test_byte_lattice_every_mask_byte_on_the_half_way_points(mask_f32):
    """One white light, one frame, final = 1: the frame's rendered value IS the albedo plane, which carries the composite's
    half-way lattice (tests/device_primitives_reference.py `byte_lattice`: every mask byte, 255 r m at k + 0.5 or one f32 step
    beside it; a NaN, a +inf, a negative value under mask 255) -- byte for byte the statement, and the image kernel's bytes."""
    import device_primitives_reference as ref
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd import rig_frames_u8
    lat = ref.byte_lattice(mask_f32)
    H = W = ref.SIDE
    arrays = (np.ones((1, 1, H, W), np.float32), lat["rendered"][None], lat["input"][None], lat["mask_u8"][None],
              np.ones((1, 1, 1, 3), np.float32))
    t = [_dev(a) for a in arrays]
    got = rig_frames_u8(*t, mask_f32=mask_f32)
    g = got.cpu().numpy()
    want = emu.frames(*arrays, mask_f32)
    assert g.shape == (1, 1, H, W, 3)
    kept = lat["kept"]["rendered_image"]
    print("lattice bytes that differ from the statement: %d of %d" % (int(((g[0, 0] != want[0, 0]) & kept).sum()), int(kept.sum())))
    np.testing.assert_array_equal(g, want)
    np.testing.assert_array_equal(g[0, 0], ref.lattice_expected(lat, mask_f32)["rendered_image"])
    image = pp.inference_images_device(t[2], t[1], t[3], mask_f32=mask_f32)["rendered_image"]
    assert torch.equal(got[0], image)
    assert list(g[0, 0, 255, 253:, 0]) == [0, 255, 0]                                     # NaN, +inf, negative
