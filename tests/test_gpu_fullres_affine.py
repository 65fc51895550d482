"""GPU: the affine kernels (csrc/gcfr_fullres_affine.hip; postprocess.ingest_affine_device / fullres_affine_composites_device) bit for
bit against the numpy restatement (tests/fullres_affine_emulation.py): x_lo as uint32, composites as bytes, no tolerance.  Every
composite is written into one guarded buffer with bands on both sides and compared as a whole.

  network  24 x 20; photographs 61 x 53 (Wp odd: one element at a time) and 64 x 48 (Wp a multiple of four: three dwords per lane),
           both more than one workgroup per face; L = 3
  faces    one launch of B = 4 with mixed K: 17 degrees at scale 2.3; -40 degrees at scale 0.6 (the composite's K = 2); exactly 90
           degrees at scale 1; 25 degrees at scale 5.1 hanging over the photograph's corner (the ingest's K = 8, replicated taps)
  calls    the mask with zero regions, shared and per face; `out=` at an odd byte offset (the element path on the 64 x 48 photograph:
           the same bytes); B = 33 on an 8 x 8 network and 16 x 16 photographs for the second launch; the integer pair in the
           place of the f64 matrix
  and      the anchor on the device (axis-aligned maps at s in {1, 2, 4} return ingest_box_device's bits and
           fullres_box_composites_device(paste=True)'s bytes); every refusal is raised before a launch."""
import numpy as np
import pytest
import torch

import fullres_affine_emulation as affine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LEVELS = np.array([255, 0, 64, 128], np.uint8)
H, W, L = 24, 20, 3
PHOTOS = {"scalar": (61, 53), "vector": (64, 48)}
BAND = 64


def _faces(Hp, Wp):
    """the four maps network -> photograph (4,2,3) f64"""
    from geomconsistentfr_amd import postprocess as pp
    spec = [(17.0, 2.3, 0.45 * Wp, 0.5 * Hp), (-40.0, 0.6, 0.4 * Wp, 0.4 * Hp), (90.0, 1.0, 0.5 * Wp, 0.5 * Hp),
            (25.0, 5.1, 0.9 * Wp, 0.85 * Hp)]
    return np.stack([pp.affine_from_rotated_box(cx, cy, s * W, s * H, deg, (H, W)) for deg, s, cx, cy in spec])


def _inputs(seed, A, h, w, Hp, Wp, shared_mask, lights=L):
    """photo (B,Hp,Wp,3) u8, x_lo (B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (1|B,h,w) u8 with a zero block and four grey levels"""
    B = A.shape[0]
    rng = np.random.default_rng(seed)
    photo = rng.integers(0, 256, (B, Hp, Wp, 3), dtype=np.uint8)
    F, _ = affine.quantise(A)
    x_lo = (affine.ingest(photo, F, h, w) * (0.1 + 1.9 * rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 1.5 * rng.standard_normal((B, lights, 3, h, w))).astype(np.float32)
    MB = 1 if shared_mask else B
    mask = rng.choice(LEVELS, (MB, h, w), p=[0.55, 0.15, 0.15, 0.15])
    mask[:, : h // 3, : w // 2] = 0
    return photo, x_lo, rendered, mask


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(shape, offset=0):
    """a view of `shape` inside a buffer of 0xAB with BAND + offset bytes in front of it and BAND behind"""
    n = int(np.prod(shape))
    buf = torch.full((BAND + offset + n + BAND,), 0xAB, dtype=torch.uint8, device=DEV)
    return buf, buf[BAND + offset:BAND + offset + n].view(shape)


def _check(label, arrays, net_to_photo, I, offset=0, **kw):
    """the composite into a guarded buffer; the WHOLE buffer against the restatement between its bands"""
    from geomconsistentfr_amd import postprocess as pp
    photo, x_lo, rendered, mask = arrays
    want = affine.composites(photo, I, x_lo, rendered, mask, **kw)
    buf, out = _guarded(want.shape, offset)
    assert out.data_ptr() % 4 == offset % 4
    got = pp.fullres_affine_composites_device(_dev(photo), net_to_photo, _dev(x_lo), _dev(rendered), _dev(mask), out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    whole = np.concatenate([np.full(BAND + offset, 0xAB, np.uint8), want.reshape(-1), np.full(BAND, 0xAB, np.uint8)])
    g = buf.cpu().numpy()
    print("%s: bytes that differ from the statement %d of %d; relit %d" % (label, int((g != whole).sum()), g.size, int((want != photo[:, None]).sum())))
    np.testing.assert_array_equal(g, whole, err_msg=label)
    return out, want


@pytest.mark.parametrize("shared_mask", [True, False])
@pytest.mark.parametrize("path", sorted(PHOTOS))
def test_four_faces_of_mixed_K_in_one_launch_equal_the_statement(path, shared_mask):
    from geomconsistentfr_amd import postprocess as pp
    Hp, Wp = PHOTOS[path]
    A = _faces(Hp, Wp)
    F, I = affine.quantise(A)
    assert [affine.sub_samples(m) for m in F] == [4, 1, 1, 8] and [affine.sub_samples(m) for m in I] == [1, 2, 1, 1]
    arrays = _inputs(7 + shared_mask, A, H, W, Hp, Wp, shared_mask)
    out, want = _check("%s shared %s" % (path, shared_mask), arrays, A, I)
    # every face is relit somewhere and left alone somewhere; the fourth hangs over the corner
    for b in range(4):
        ins = affine.inside(I[b], Hp, Wp, H, W)
        assert ins.any() and not ins.all() and (want[b] != arrays[0][b][None]).any()
    assert affine.inside(I[3], Hp, Wp, H, W)[Hp - 1, Wp - 1]
    # the ingest, as bits; the integer pair in the place of the matrix: the same bits and bytes
    x_want = affine.ingest(arrays[0], F, H, W)
    for given in (A, (F, I), torch.from_numpy(A)):
        x = pp.ingest_affine_device(_dev(arrays[0]), given, (H, W))
        assert tuple(x.shape) == (4, H, W, 3) and x.dtype == torch.float32
        np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), x_want.view(np.uint32))
    again = pp.fullres_affine_composites_device(_dev(arrays[0]), (F, I), *[_dev(a) for a in arrays[1:]])
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)
    # other clamp and floor; a rendered without the light axis, in f64
    _check("clamp 2, floor 8", arrays, A, I, detail_clamp=2.0, floor=8.0)
    one = pp.fullres_affine_composites_device(_dev(arrays[0]), A, _dev(arrays[1]), _dev(arrays[2][:, 1]).double(), _dev(arrays[3]))
    assert one.dim() == 4 and torch.equal(one, out[:, 1])


def test_out_at_an_odd_byte_offset_takes_the_element_path_and_gives_the_same_bytes():
    Hp, Wp = PHOTOS["vector"]
    A = _faces(Hp, Wp)
    _, I = affine.quantise(A)
    arrays = _inputs(21, A, H, W, Hp, Wp, False)
    aligned, _ = _check("aligned", arrays, A, I)
    for offset in (1, 3):
        odd, _ = _check("offset %d" % offset, arrays, A, I, offset=offset)
        assert odd.data_ptr() % 4 == offset and torch.equal(odd, aligned)


@pytest.mark.parametrize("Wp", [16, 15])
def test_thirty_three_faces_cross_the_launch_limit(Wp):
    from geomconsistentfr_amd import postprocess as pp
    h = w = 8
    Hp, B = 16, 33
    rng = np.random.default_rng(33)
    A = np.stack([pp.affine_from_rotated_box(4.0 + 8.0 * rng.random(), 4.0 + 8.0 * rng.random(), (0.5 + 1.5 * rng.random()) * w,
                                             (0.5 + 1.5 * rng.random()) * h, 360.0 * rng.random() - 180.0, (h, w)) for _ in range(B)])
    F, I = affine.quantise(A)
    assert {affine.sub_samples(m) for m in I} == {1, 2} and {affine.sub_samples(m) for m in F} == {1, 2}
    arrays = _inputs(34, A, h, w, Hp, Wp, False)
    out, want = _check("B 33", arrays, A, I)
    assert (want[32] != arrays[0][32][None]).any()                                 # the face of the second launch is relit
    x = pp.ingest_affine_device(_dev(arrays[0]), A, h)
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), affine.ingest(arrays[0], F, h, w).view(np.uint32))


@pytest.mark.parametrize("path", sorted(PHOTOS))
@pytest.mark.parametrize("s", [1, 2, 4])
def test_axis_aligned_maps_return_the_box_entries_bits_and_bytes(s, path):
    """the anchor, with no tolerance: two kernels, one statement"""
    from geomconsistentfr_amd import postprocess as pp
    h, w = 12, 10
    Hp, Wp = PHOTOS[path]
    boxes = np.array([(2, 1, s * w, s * h), (Wp - s * w, Hp - s * h, s * w, s * h)])
    A = np.stack([[[float(s), 0.0, float(x0)], [0.0, float(s), float(y0)]] for x0, y0, _, _ in boxes])
    arrays = _inputs(60 + s, A, h, w, Hp, Wp, s == 2)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    xa, xb = pp.ingest_affine_device(photo, A, (h, w)), pp.ingest_box_device(photo, boxes, (h, w))
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    got = pp.fullres_affine_composites_device(photo, A, x_lo, rendered, mask)
    want = pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, paste=True)
    assert (want != photo[:, None]).any() and torch.equal(got, want)
    if s == 1:                                                                     # s = 8 on the way in only: the ingest's K = 8
        big = np.array([(0, 0, 8 * 5, 8 * 6)])
        xa = pp.ingest_affine_device(photo[:1], np.array([[8.0, 0.0, 0.0], [0.0, 8.0, 0.0]]), (6, 5))
        assert torch.equal(xa.view(torch.int32), pp.ingest_box_device(photo[:1], big, (6, 5)).view(torch.int32))


def test_a_side_stream():
    from geomconsistentfr_amd import postprocess as pp
    Hp, Wp = PHOTOS["vector"]
    A = _faces(Hp, Wp)
    F, I = affine.quantise(A)
    arrays = _inputs(14, A, H, W, Hp, Wp, True)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x_dev = pp.ingest_affine_device(photo, A, (H, W))
        got = pp.fullres_affine_composites_device(photo, A, x_lo, rendered, mask)
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), affine.composites(arrays[0], I, *arrays[1:]))
    np.testing.assert_array_equal(x_dev.cpu().numpy().view(np.uint32), affine.ingest(arrays[0], F, H, W).view(np.uint32))


def test_every_refusal_is_raised_before_a_launch():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    Hp, Wp = PHOTOS["vector"]
    A = _faces(Hp, Wp)
    F, I = affine.quantise(A)
    arrays = _inputs(1, A, H, W, Hp, Wp, True)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    buf, out = _guarded((4, L, Hp, Wp, 3))

    def refused(match, net_to_photo=A, ph=photo, x=x_lo, r=rendered, m=mask, o=out, **kw):
        with pytest.raises(GcfrError, match=match):
            pp.fullres_affine_composites_device(ph, net_to_photo, x, r, m, out=o, **kw)

    refused("HOST", torch.from_numpy(A).to(DEV))
    refused("HOST", (torch.from_numpy(F).to(DEV), torch.from_numpy(I)))
    refused("determinant", A * np.array([[1.0], [-1.0]])[None])                    # a mirror image
    refused("determinant", (F, I * np.array([[1], [-1]])[None]))
    refused("column", A * 0.1)                                                     # a face of a tenth of the network's size
    refused("integers", (F.astype(np.float64), I))
    refused(r"\(4,2,3\)", A[:3])
    refused("detail_clamp", detail_clamp=0.5)
    refused("detail_clamp", floor=0.0)
    refused("rendered", r=rendered[:, :, :, :-1])
    refused("mask_u8", m=mask[:, :-1])
    refused("no CPU path", ph=photo.cpu())
    refused("overlap", o=photo.view(-1)[: 1 * 3 * Hp * Wp].view(1, Hp, Wp, 3), ph=photo[:1], net_to_photo=A[0], x=x_lo[:1],
            r=rendered[:1, 0], m=mask)
    with pytest.raises(GcfrError, match="HOST"):
        pp.ingest_affine_device(photo, torch.from_numpy(A).to(DEV), (H, W))
    with pytest.raises(GcfrError, match="column"):
        pp.ingest_affine_device(photo, A * 9.0, (H, W))
    with pytest.raises(GcfrError, match="size"):
        pp.ingest_affine_device(photo, A, (H, 0))
    with pytest.raises(GcfrError, match="uint8"):
        pp.ingest_affine_device(photo.float(), A, (H, W))
    torch.cuda.synchronize(DEV)
    assert (buf == 0xAB).all()                                                     # nothing was launched
