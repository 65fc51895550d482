"""GPU: the group-affine kernels (csrc/gcfr_fullres_group_affine.hip; postprocess.ingest_group_affine_device /
fullres_group_affine_composites_device) bit for bit against the numpy restatement (tests/fullres_group_affine_emulation.py) AND
against the three anchors of include/gcfr.h on the device: x_lo as uint32, composites as bytes, no tolerance anywhere.

  anchor 1   the chain of postprocess.fullres_affine_composites_device calls that the entry replaces: one call per face, the lights
             as its batch, the running images as its photographs
  anchor 2   photo_index = arange(B), P = B: ONE fullres_affine_composites_device call and ONE ingest_affine_device call; B = 33
             crosses the launch's limit of 32 photographs
  anchor 3   axis-aligned maps with integer origins at 1, 2 and 4 times the network's side, overlapping each other:
             postprocess.fullres_group_composites_device on the same boxes
The cases are tests/fullres_group_affine_cases.py's (network 24 x 20; photographs 61 x 53, the scalar path, and 64 x 48, the vector
path; three tilted faces per photograph, one of them with K = 2 on the way out; the seam of 34 small quads in one photograph).
tests/test_fullres_group_affine_host.py shows on the CPU alone that they bite: some pixel is relit by two faces, swapping those two
faces changes bytes, a face crosses another where its own carried mask is zero, both saturations and both sides of detail_clamp
occur, and faces 32 and 33 of the seam relight, in a continuation launch, what an earlier launch's faces relit.
And: a NaN in `rendered` under a zero mask; every operand one element off its alignment, `out` included; `out=` between guard
bands, then over its own result; a side stream; device tensors as map or index refused."""
import numpy as np
import pytest
import torch

import fullres_group_affine_cases as cases
import fullres_group_affine_emulation as tilted

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("photo", "x_lo", "rendered", "mask")
H, W = cases.H, cases.W


def _dev(a, misalign=False):
    """a device tensor of `a`; misalign: its first element sits one element past an aligned allocation"""
    t = torch.from_numpy(np.array(a))
    if not misalign:
        return t.to(DEV)
    buf = torch.empty(a.size + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(a.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _device_chain(t, pair, pidx, **kw):
    """anchor 1: one fullres_affine_composites_device call per face, in ascending face index, the lights as its batch"""
    from geomconsistentfr_amd import postprocess as pp
    photo, x_lo, rendered, mask = (t[n] for n in NAMES)
    L = rendered.shape[1]
    run = photo[:, None].repeat(1, L, 1, 1, 1)
    for b, q in enumerate(pidx):
        mk = mask[b:b + 1] if mask.shape[0] > 1 else mask
        run[q] = pp.fullres_affine_composites_device(run[q], (pair[0][b], pair[1][b]), x_lo[b:b + 1].expand(L, -1, -1, -1),
                                                     rendered[b].contiguous(), mk, **kw)
    return run


def _check(label, arrays, pair, pidx, want=None, misalign=(), chain=True, **kw):
    from geomconsistentfr_amd import postprocess as pp
    t = {n: _dev(a, n in misalign) for n, a in zip(NAMES, arrays)}
    got = pp.fullres_group_affine_composites_device(t["photo"], pair, list(pidx), t["x_lo"], t["rendered"], t["mask"], **kw)
    rest = {k: v for k, v in kw.items() if k != "out"}
    if want is None:
        want = tilted.composites(arrays[0], pair[1], pidx, *arrays[1:], **rest)
    g = got.cpu().numpy()
    print("%s: bytes that differ from the statement %d of %d" % (label, int((g != want).sum()), g.size))
    assert g.shape == want.shape and g.dtype == np.uint8
    np.testing.assert_array_equal(g, want, err_msg=label)
    if chain:
        assert torch.equal(got, _device_chain(t, pair, pidx, **rest)), label + ": the chain on the device"
    return got, t


def _check_ingest(photo, pair, pidx, h, w):
    from geomconsistentfr_amd import postprocess as pp
    want = tilted.ingest(photo, pair[0], pidx, h, w)
    for mis in (False, True):
        p = _dev(photo, mis)
        got = pp.ingest_group_affine_device(p, pair, list(pidx), (h, w))
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        gathered = pp.ingest_affine_device(p[torch.as_tensor(list(pidx), device=DEV)], pair, (h, w))
        assert torch.equal(got.view(torch.int32), gathered.view(torch.int32))


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("which", sorted(cases.INDICES))
@pytest.mark.parametrize("aligned", [True, False])
def test_composites_and_ingest_equal_the_statement_and_the_chain(aligned, which, L, shared):
    arrays, pair, pidx, want = cases.case(aligned, which, L, shared)
    P = cases.N_PHOTOS[which]
    got, t = _check("%s L %d aligned %s shared %s" % (which, L, aligned, shared), arrays, pair, pidx, want)
    assert tuple(got.shape) == (P, L) + arrays[0].shape[1:]
    if which == "gap":                                                             # the photograph without faces, for every light
        for l in range(L):
            assert torch.equal(got[1, l], t["photo"][1])
    assert (got.cpu().numpy() != arrays[0][:, None]).any()
    _check_ingest(arrays[0], pair, pidx, H, W)


def test_lists_tensors_matrices_and_a_rendered_without_the_light_axis():
    from geomconsistentfr_amd import postprocess as pp
    arrays, pair, pidx, want = cases.case(True, "three", 3, False)
    Hp, Wp = cases.SIZES[True]
    A, F, I = cases.maps(pidx, Hp, Wp)
    got, t = _check("as the integer pair", arrays, pair, pidx, want, chain=False)
    # the f64 matrices quantise to the same integers: a list, a CPU tensor; the indices as an array and as a tensor
    again = pp.fullres_group_affine_composites_device(t["photo"], A.tolist(), np.array(pidx, np.uint8), t["x_lo"], t["rendered"], t["mask"])
    assert torch.equal(again, got)
    one = pp.fullres_group_affine_composites_device(t["photo"], torch.from_numpy(A), torch.tensor(pidx), t["x_lo"],
                                                    t["rendered"][:, 2].double(), t["mask"])
    assert one.dim() == 4 and torch.equal(one, got[:, 2])
    x = pp.ingest_group_affine_device(t["photo"], A, pidx, (H, W))
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), tilted.ingest(arrays[0], F, pidx, H, W).view(np.uint32))
    _check("clamp 2, floor 8", arrays, pair, pidx, detail_clamp=2.0, floor=8.0)
    # photo_index=None: every face in the one photograph
    arrays, pair, pidx, want = cases.case(False, "one", 3, True)
    t = {n: _dev(a) for n, a in zip(NAMES, arrays)}
    none = pp.fullres_group_affine_composites_device(t["photo"], pair, None, t["x_lo"], t["rendered"], t["mask"])
    np.testing.assert_array_equal(none.cpu().numpy(), want)
    x = pp.ingest_group_affine_device(t["photo"], pair, None, (H, W))
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), tilted.ingest(arrays[0], pair[0], pidx, H, W).view(np.uint32))


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("aligned", [True, False])
def test_thirty_four_quads_in_one_photograph_cross_the_launch_seam(aligned, L, shared):
    arrays, pair, pidx, want = cases.seam_case(aligned, L, shared)
    h, w = cases.SEAM_NET
    assert [q for q in pidx].count(1) == 34
    _check("the seam, aligned %s L %d shared %s" % (aligned, L, shared), arrays, pair, pidx, want)
    _check_ingest(arrays[0], pair, pidx, h, w)


@pytest.mark.parametrize("aligned", [True, False])
def test_one_face_per_photograph_is_one_affine_call(aligned):
    """anchor 2, with no tolerance: photo_index = arange(B), P = B; 33 photographs cross the launch's limit of 32"""
    from geomconsistentfr_amd import postprocess as pp
    Hp, Wp = cases.SIZES[aligned]
    for B, L in ((3, 3), (33, 1)):
        pidx = list(range(B))
        _, F, I = cases.maps([0] * B, Hp, Wp)                                      # the three kinds in turn
        arrays = cases.inputs(80 + B, B, L, H, W, Hp, Wp, F, pidx, B == 3)
        t = {n: _dev(a) for n, a in zip(NAMES, arrays)}
        got = pp.fullres_group_affine_composites_device(t["photo"], (F, I), pidx, t["x_lo"], t["rendered"], t["mask"])
        assert torch.equal(got, pp.fullres_affine_composites_device(t["photo"], (F, I), t["x_lo"], t["rendered"], t["mask"]))
        assert (got != t["photo"][:, None]).any()
        xa, xb = pp.ingest_group_affine_device(t["photo"], (F, I), pidx, (H, W)), pp.ingest_affine_device(t["photo"], (F, I), (H, W))
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("aligned", [True, False])
def test_upright_maps_are_the_group_entry_on_the_same_overlapping_boxes(aligned, shared):
    """anchor 3, with no tolerance"""
    from geomconsistentfr_amd import postprocess as pp
    arrays, pair, boxes, pidx = cases.upright_case(aligned, 3, shared)
    h, w = cases.UPRIGHT_NET
    got, t = _check("upright, aligned %s shared %s" % (aligned, shared), arrays, pair, pidx)
    boxed = pp.fullres_group_composites_device(t["photo"], boxes, pidx, t["x_lo"], t["rendered"], t["mask"])
    assert torch.equal(got, boxed)
    xa, xb = pp.ingest_group_affine_device(t["photo"], pair, pidx, (h, w)), pp.ingest_group_device(t["photo"], boxes, pidx, (h, w))
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))


def test_a_nan_under_a_zero_mask_reaches_nothing():
    arrays, pair, pidx, want = cases.case(True, "three", 3, False)
    photo, x_lo, rendered, mask = arrays
    assert (mask[:, :, :2] == 0).all()
    rendered = rendered.copy()
    rendered[:, :, :, :, 0] = np.nan                                               # every tap beside column 0 has mask 0
    _check("NaN under the zero mask", (photo, x_lo, rendered, mask), pair, pidx, want)
    # a `rendered` of NaNs alone leaves every byte that no face relights the photograph's
    rendered[:] = np.nan
    got, _ = _check("all NaN", (photo, x_lo, rendered, mask), pair, pidx)
    kept = tilted.relit_counts(pair[1], pidx, mask, *photo.shape[:3], H, W) == 0
    g = got.cpu().numpy()
    for l in range(3):
        np.testing.assert_array_equal(g[:, l][kept], photo[kept])
    assert (g[:, 0][~kept] == 0).all()


@pytest.mark.parametrize("which", ["photo", "x_lo", "rendered", "mask", "out", "all"])
def test_every_operand_off_its_alignment(which):
    """Wp is a multiple of four: aligned, the vector path runs; with the output one byte off, the element path must return the
    same bytes; the photograph, the f32 operands and the mask need no alignment on either path"""
    arrays, pair, pidx, want = cases.case(True, "three", 3, False)
    mis = NAMES if which == "all" else (which,)
    kw = {}
    if which in ("out", "all"):
        buf = torch.full((want.size + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        kw["out"] = buf[1:].view(want.shape)
        assert kw["out"].data_ptr() % 4 == 1
    got, _ = _check("misaligned " + which, arrays, pair, pidx, want, misalign=mis, chain=False, **kw)
    if kw:
        assert got.data_ptr() == kw["out"].data_ptr() and int(buf[0]) == 0xAB


@pytest.mark.parametrize("aligned", [True, False])
def test_out_is_written_in_place_between_untouched_guard_bands(aligned):
    from geomconsistentfr_amd import postprocess as pp
    arrays, pair, pidx, want = cases.case(aligned, "gap", 3, True)                 # (more than one workgroup per photograph)
    assert want.shape[2] * want.shape[3] > 1024
    n = want.size
    buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(want.shape)
    got, t = _check("out=", arrays, pair, pidx, want, chain=False, out=out)
    assert got.data_ptr() == out.data_ptr() and (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all()
    again = pp.fullres_group_affine_composites_device(t["photo"], pair, pidx, t["x_lo"], t["rendered"], t["mask"])   # two calls: the same bytes
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)
    again = pp.fullres_group_affine_composites_device(t["photo"], pair, pidx, t["x_lo"], t["rendered"], t["mask"], out=out)   # over its own result
    assert torch.equal(again, torch.from_numpy(np.array(want)).to(DEV))
    assert (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all()
    np.testing.assert_array_equal(t["photo"].cpu().numpy(), arrays[0])


def test_a_side_stream():
    from geomconsistentfr_amd import postprocess as pp
    arrays, pair, pidx, want = cases.seam_case(True, 3, False)
    t = {n: _dev(a) for n, a in zip(NAMES, arrays)}
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x_dev = pp.ingest_group_affine_device(t["photo"], pair, list(pidx), cases.SEAM_NET)
        got = pp.fullres_group_affine_composites_device(t["photo"], pair, list(pidx), t["x_lo"], t["rendered"], t["mask"])
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(x_dev.cpu().numpy().view(np.uint32), tilted.ingest(arrays[0], pair[0], pidx, *cases.SEAM_NET).view(np.uint32))


def test_device_tensors_as_map_or_index_are_refused_and_nothing_is_written():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    arrays, pair, pidx, want = cases.case(True, "three", 1, True)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    A = cases.maps(pidx, *cases.SIZES[True])[0]
    n = want.size
    buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(want.shape)
    with pytest.raises(GcfrError, match="HOST"):
        pp.fullres_group_affine_composites_device(photo, pair, torch.tensor(pidx).to(DEV), x_lo, rendered, mask, out=out)
    with pytest.raises(GcfrError, match="HOST"):
        pp.fullres_group_affine_composites_device(photo, torch.from_numpy(A).to(DEV), pidx, x_lo, rendered, mask, out=out)
    with pytest.raises(GcfrError, match="HOST"):
        pp.fullres_group_affine_composites_device(photo, (torch.from_numpy(np.array(pair[0])).to(DEV), pair[1]), pidx, x_lo, rendered, mask, out=out)
    with pytest.raises(GcfrError, match="HOST"):
        pp.ingest_group_affine_device(photo, pair, torch.tensor(pidx).to(DEV), (H, W))
    with pytest.raises(GcfrError, match="HOST"):
        pp.ingest_group_affine_device(photo, torch.from_numpy(A).to(DEV), pidx, (H, W))
    with pytest.raises(GcfrError, match="overlap"):
        pp.fullres_group_affine_composites_device(photo, pair, pidx, x_lo, rendered[:, 0], mask, out=photo)
    torch.cuda.synchronize(DEV)
    assert (buf == 0xAB).all(), "the guarded buffer is untouched"
    np.testing.assert_array_equal(photo.cpu().numpy(), arrays[0])
