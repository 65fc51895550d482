"""GPU: the group-photograph kernels (csrc/gcfr_fullres_group.hip; postprocess.ingest_group_device /
fullres_group_composites_device) bit for bit against the numpy restatement (tests/fullres_group_emulation.py) AND against the chain
of postprocess.fullres_anybox_composites_device calls on the device that the entry replaces (one call per face, the lights as its
batch, the running images as its photographs): x_lo as uint32, composites as bytes, no tolerance anywhere.

  networks (h, w) in {(5,7), (23,17)}; photographs (2h + 8) x (4w + 4 | 4w + 5): the vector and the scalar path
  faces    per photograph a LARGE box (2h+1, 2w+1), a SMALL one (h-1, w-1) inside the large one's relit part (both carried masks
           are positive there) and a MIXED one (h-2, 4w), whose carried mask is zero on its left where it crosses the large one;
           the three come in a different order in every photograph
  calls    P = 1 with [0, 0, 0]; P = 3 with [2, 0, 2, 1, 0, 2, 1, 0, 1] (unordered) and with [2, 0, 2, 0, 2, 0] (photograph 1 has no
           face); L in {1, 3}; the mask shared and per face, over the grey levels {0, 64, 128, 255} with its left columns zero;
           `rendered` well outside [0, 1]; x_lo scaled away from the photograph's means
  seam     34 faces in ONE photograph on network (4, 8): 3 x 3 and 1 x 1 boxes on a stride-2 grid (a 3 x 3 box overlaps its
           neighbours), so that faces 32 and 33 arrive in a CONTINUATION launch and relight pixels that faces 26 and 27 relit;
           another photograph with a single face shares the call
  and      a NaN in `rendered` under a zero mask; every operand one element off its alignment; `out=` between guard bands; a side
           stream; the anchor photo_index = arange(B), P = B against ONE fullres_anybox_composites_device call; the ingest's bits
           against ingest_anybox_device on the gathered photo[photo_index].
What makes the cases bite is asserted once, on the CPU alone and before anything runs on the device: some pixel is relit by two
faces, swapping those two faces changes bytes, a face crosses another where its own carried mask is zero, and both saturations
and both sides of detail_clamp occur."""
import functools

import numpy as np
import pytest
import torch

import fullres_anybox_emulation as anybox
import fullres_group_emulation as group

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LEVELS = np.array([255, 0, 64, 128], np.uint8)
NAMES = ("photo", "x_lo", "rendered", "mask")
NETS = [(5, 7), (23, 17)]
INDICES = {"one": [0, 0, 0], "three": [2, 0, 2, 1, 0, 2, 1, 0, 1], "gap": [2, 0, 2, 0, 2, 0]}
N_PHOTOS = {"one": 1, "three": 3, "gap": 3}


def _photo_size(h, w, aligned):
    return 2 * h + 8, 4 * w + (4 if aligned else 5)


def _boxes(h, w, pidx):
    """(B,4) (x0, y0, bw, bh): the k-th face of photograph q is of kind (k + q) % 3 -- large, small, mixed -- shifted by q"""
    seen, rows = {}, []
    for q in pidx:
        k = seen.get(q, 0)
        seen[q] = k + 1
        dx, dy = q % 2, q
        rows.append([(1 + dx, 2 + dy, 2 * w + 1, 2 * h + 1), (1 + w + dx, 3 + dy, w - 1, h - 1), (4 - dx, h + 1 + dy, 4 * w, h - 2)][(k + q) % 3])
    return np.array(rows)


def _masks(rng, MB, h, w):
    """the four grey levels in random order, the left columns zero"""
    mask = np.stack([rng.permutation(m) for m in np.resize(LEVELS, MB * h * w).reshape(MB, h * w)]).reshape(MB, h, w)
    mask[:, :, :max(2, w // 3)] = 0
    assert set(np.unique(mask)) == set(LEVELS.tolist())
    return mask


def _inputs(seed, P, L, h, w, Hp, Wp, boxes, pidx, shared):
    """photo (P,Hp,Wp,3) u8, x_lo (B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (1|B,h,w) u8"""
    rng = np.random.default_rng(seed)
    B = len(pidx)
    photo = rng.integers(0, 256, (P, Hp, Wp, 3), dtype=np.uint8)
    x_lo = (group.ingest(photo, boxes, pidx, h, w) * (0.1 + 1.9 * rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 1.5 * rng.standard_normal((B, L, 3, h, w))).astype(np.float32)
    return photo, x_lo, rendered, _masks(rng, 1 if shared else B, h, w)


@functools.lru_cache(maxsize=None)
def _case(h, w, aligned, which, L, shared):
    """the inputs of a case and the restatement's bytes, computed once and shared (read only)"""
    Hp, Wp = _photo_size(h, w, aligned)
    pidx = INDICES[which]
    boxes = _boxes(h, w, pidx)
    arrays = _inputs(7 * h + L + 2 * aligned + shared + len(pidx), N_PHOTOS[which], L, h, w, Hp, Wp, boxes, pidx, shared)
    want = group.composites(arrays[0], boxes, pidx, *arrays[1:])
    for a in arrays + (want, boxes):
        a.setflags(write=False)
    return arrays, boxes, pidx, want


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


def _device_chain(t, boxes, pidx, **kw):
    """what the entry replaces: one fullres_anybox_composites_device call per face, in ascending face index, the lights as its batch"""
    from geomconsistentfr_amd import postprocess as pp
    photo, x_lo, rendered, mask = (t[n] for n in NAMES)
    L = rendered.shape[1]
    run = photo[:, None].repeat(1, L, 1, 1, 1)
    for b, q in enumerate(pidx):
        mk = mask[b:b + 1] if mask.shape[0] > 1 else mask
        run[q] = pp.fullres_anybox_composites_device(run[q], tuple(int(v) for v in boxes[b]), x_lo[b:b + 1].expand(L, -1, -1, -1),
                                                     rendered[b].contiguous(), mk, **kw)
    return run


def _check(label, arrays, boxes, pidx, want=None, misalign=(), chain=True, **kw):
    from geomconsistentfr_amd import postprocess as pp
    t = {n: _dev(a, n in misalign) for n, a in zip(NAMES, arrays)}
    got = pp.fullres_group_composites_device(t["photo"], boxes, pidx, t["x_lo"], t["rendered"], t["mask"], **kw)
    rest = {k: v for k, v in kw.items() if k != "out"}
    if want is None:
        want = group.composites(arrays[0], boxes, pidx, *arrays[1:], **rest)
    g = got.cpu().numpy()
    print("%s: bytes that differ from the statement %d of %d" % (label, int((g != want).sum()), g.size))
    assert g.shape == want.shape and g.dtype == np.uint8
    np.testing.assert_array_equal(g, want, err_msg=label)
    if chain:
        assert torch.equal(got, _device_chain(t, boxes, pidx, **rest)), label + ": the chain on the device"
    return got, t


def _check_ingest(photo, boxes, pidx, h, w):
    from geomconsistentfr_amd import postprocess as pp
    want = group.ingest(photo, boxes, pidx, h, w)
    for mis in (False, True):
        p = _dev(photo, mis)
        got = pp.ingest_group_device(p, boxes, pidx, (h, w))
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        gathered = pp.ingest_anybox_device(p[torch.as_tensor(pidx, device=DEV)], boxes, (h, w))
        assert torch.equal(got.view(torch.int32), gathered.view(torch.int32))


@pytest.mark.parametrize("h,w", NETS)
def test_the_cases_bite_on_the_cpu_alone(h, w):
    """nothing here touches the device"""
    arrays, boxes, pidx, want = _case(h, w, True, "three", 3, False)
    photo, x_lo, rendered, mask = arrays
    P, Hp, Wp, _ = photo.shape
    relit = group.relit_counts(boxes, pidx, mask, P, Hp, Wp, h, w)
    inside = group.relit_counts(boxes, pidx, np.full_like(mask, 255), P, Hp, Wp, h, w)
    assert (relit >= 2).any(), "some pixel is relit by two faces"
    assert ((inside >= 2) & (relit == 1)).any(), "a face crosses another where its own carried mask is zero"
    assert (inside == 0).any() and ((inside == 1) & (relit == 0)).any()
    # photograph 0: faces 1, 4, 7 are its large, small and mixed box; the small one lies in the large one's relit part
    kinds = {tuple(boxes[b, 2:]): b for b in (1, 4, 7)}
    big, small = kinds[(2 * w + 1, 2 * h + 1)], kinds[(w - 1, h - 1)]
    both = np.zeros((Hp, Wp), np.int64)
    for b in (big, small):
        both += group.relit_counts(boxes[b:b + 1], [0], mask[b:b + 1], 1, Hp, Wp, h, w)[0]
    assert (both == 2).any()
    order = list(range(len(pidx)))
    order[big], order[small] = small, big
    swapped = group.composites(photo, boxes, pidx, x_lo, rendered, mask, order=order)
    differ = (swapped != want).any(axis=(1, 4))
    assert differ[0].any(), "swapping the two faces changes bytes"
    assert not differ[1:].any() and not (differ[0] & (both < 2)).any(), "order matters where both relight a pixel and nowhere else"
    # the regimes, on the faces' first composites and on a second one
    d_all, v_all = [], []
    for b in range(len(pidx)):
        x0, y0, bw, bh = boxes[b]
        for source in (photo[pidx[b]], want[pidx[b], 0]):
            v, m, d, _ = anybox.box_terms(source[y0:y0 + bh, x0:x0 + bw], x_lo[b], rendered[b], mask[b])
            d_all.append(d.ravel())
            v_all.append(v[np.broadcast_to(m[None, :, :, None] > 0, v.shape)])
    d_all, v_all = np.concatenate(d_all), np.concatenate(v_all)
    assert (d_all == 4.0).any() and (d_all == 0.25).any(), "both sides of detail_clamp"
    assert (v_all < -0.5).any() and (v_all > 255.5).any(), "both saturations"


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("which", sorted(INDICES))
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("h,w", NETS)
def test_composites_and_ingest_equal_the_statement_and_the_chain(h, w, aligned, which, L, shared):
    arrays, boxes, pidx, want = _case(h, w, aligned, which, L, shared)
    P = N_PHOTOS[which]
    got, t = _check("(%d,%d) %s L %d aligned %s shared %s" % (h, w, which, L, aligned, shared), arrays, boxes, pidx, want)
    assert tuple(got.shape) == (P, L) + arrays[0].shape[1:]
    if which == "gap":                                                             # the photograph without faces, for every light
        for l in range(L):
            assert torch.equal(got[1, l], t["photo"][1])
    assert (got.cpu().numpy() != arrays[0][:, None]).any()
    _check_ingest(arrays[0], boxes, pidx, h, w)


@pytest.mark.parametrize("h,w", NETS)
def test_lists_tensors_and_a_rendered_without_the_light_axis(h, w):
    from geomconsistentfr_amd import postprocess as pp
    arrays, boxes, pidx, want = _case(h, w, True, "three", 3, False)
    got, t = _check("as arrays", arrays, boxes, pidx, want, chain=False)
    again = pp.fullres_group_composites_device(t["photo"], boxes.tolist(), np.array(pidx, np.uint8), t["x_lo"], t["rendered"], t["mask"])
    assert torch.equal(again, got)
    one = pp.fullres_group_composites_device(t["photo"], torch.from_numpy(np.array(boxes)).to(torch.int16), torch.tensor(pidx),
                                             t["x_lo"], t["rendered"][:, 2].double(), t["mask"])
    assert one.dim() == 4 and torch.equal(one, got[:, 2])
    _check("clamp 2, floor 8", arrays, boxes, pidx, detail_clamp=2.0, floor=8.0)
    # photo_index=None: every face in the one photograph
    arrays, boxes, pidx, want = _case(h, w, False, "one", 3, True)
    t = {n: _dev(a) for n, a in zip(NAMES, arrays)}
    none = pp.fullres_group_composites_device(t["photo"], boxes, None, t["x_lo"], t["rendered"], t["mask"])
    np.testing.assert_array_equal(none.cpu().numpy(), want)
    x = pp.ingest_group_device(t["photo"], boxes, None, (h, w))
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), group.ingest(arrays[0], boxes, pidx, h, w).view(np.uint32))


def _seam_case(aligned, L, shared):
    """34 faces in photograph 1 on a stride-2 grid, six to a row, every fifth 1 x 1 and the others 3 x 3; face 10 of the call is the
    one face of photograph 0"""
    h, w, Hp, Wp = 4, 8, 14, 16 if aligned else 15
    rows, pidx = [], []
    for f in range(34):
        n = 1 if f % 5 == 4 else 3
        rows.append((2 * (f % 6), 2 * (f // 6), n, n))
        pidx.append(1)
    rows.insert(10, (3, 2, 9, 7))
    pidx.insert(10, 0)
    boxes = np.array(rows)
    rng = np.random.default_rng(34 + L + aligned)
    B = len(pidx)
    photo = rng.integers(0, 256, (2, Hp, Wp, 3), dtype=np.uint8)
    x_lo = (group.ingest(photo, boxes, pidx, h, w) * (0.1 + 1.9 * rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 1.5 * rng.standard_normal((B, L, 3, h, w))).astype(np.float32)
    MB = 1 if shared else B
    mask = np.stack([rng.permutation(m) for m in np.resize(LEVELS, MB * h * w).reshape(MB, h * w)]).reshape(MB, h, w)
    return (photo, x_lo, rendered, mask), boxes, pidx


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("aligned", [True, False])
def test_thirty_four_faces_in_one_photograph_cross_the_launch_seam(aligned, L, shared):
    arrays, boxes, pidx = _seam_case(aligned, L, shared)
    h, w = 4, 8
    photo, mask = arrays[0], arrays[3]
    P, Hp, Wp, _ = photo.shape
    in_1 = [b for b, q in enumerate(pidx) if q == 1]
    assert len(in_1) == 34 and pidx.count(0) == 1
    pick = lambda faces: (boxes[faces], [pidx[b] for b in faces], mask if shared else mask[faces])
    early = group.relit_counts(*pick(in_1[:32]), P, Hp, Wp, h, w)[1]
    late = group.relit_counts(*pick(in_1[32:]), P, Hp, Wp, h, w)[1]
    assert ((early > 0) & (late > 0)).any(), "a face of the continuation launch relights what an earlier launch's face relit"
    assert (early >= 2).any() and (early == 0).any()
    _check("the seam, aligned %s L %d shared %s" % (aligned, L, shared), arrays, boxes, pidx)
    _check_ingest(photo, boxes, pidx, h, w)


def test_a_nan_under_a_zero_mask_reaches_nothing():
    for h, w in NETS:
        arrays, boxes, pidx, want = _case(h, w, True, "three", 3, False)
        photo, x_lo, rendered, mask = arrays
        assert (mask[:, :, :2] == 0).all()
        rendered = rendered.copy()
        rendered[:, :, :, :, 0] = np.nan                                           # every tap beside column 0 has mask 0
        got, _ = _check("NaN under the zero mask", (photo, x_lo, rendered, mask), boxes, pidx, want)
        # a `rendered` of NaNs alone leaves every byte that no face relights the photograph's
        rendered[:] = np.nan
        got, _ = _check("all NaN", (photo, x_lo, rendered, mask), boxes, pidx)
        kept = group.relit_counts(boxes, pidx, mask, *photo.shape[:3], h, w) == 0
        g = got.cpu().numpy()
        for l in range(3):
            np.testing.assert_array_equal(g[:, l][kept], photo[kept])
        assert (g[:, 0][~kept] == 0).all()


@pytest.mark.parametrize("which", ["photo", "x_lo", "rendered", "mask", "out", "all"])
def test_every_operand_off_its_alignment(which):
    """Wp is a multiple of four: aligned, the vector path runs; with the output one byte off, the element path must return the
    same bytes; the photograph, the f32 operands and the mask need no alignment on either path"""
    h, w = 23, 17
    arrays, boxes, pidx, want = _case(h, w, True, "three", 3, False)
    mis = NAMES if which == "all" else (which,)
    kw = {}
    if which in ("out", "all"):
        buf = torch.full((want.size + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        kw["out"] = buf[1:].view(want.shape)
        assert kw["out"].data_ptr() % 4 == 1
    got, _ = _check("misaligned " + which, arrays, boxes, pidx, want, misalign=mis, chain=False, **kw)
    if kw:
        assert got.data_ptr() == kw["out"].data_ptr() and int(buf[0]) == 0xAB


@pytest.mark.parametrize("aligned", [True, False])
def test_out_is_written_in_place_between_untouched_guard_bands(aligned):
    from geomconsistentfr_amd import postprocess as pp
    h, w = 23, 17                                                                  # (54 x 72: more than one workgroup per photograph)
    arrays, boxes, pidx, want = _case(h, w, aligned, "gap", 3, True)
    n = want.size
    buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(want.shape)
    got, t = _check("out=", arrays, boxes, pidx, want, chain=False, out=out)
    assert got.data_ptr() == out.data_ptr() and (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all()
    again = pp.fullres_group_composites_device(t["photo"], boxes, pidx, t["x_lo"], t["rendered"], t["mask"])   # two calls: the same bytes
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)
    again = pp.fullres_group_composites_device(t["photo"], boxes, pidx, t["x_lo"], t["rendered"], t["mask"], out=out)   # over its own result
    assert torch.equal(again, torch.from_numpy(np.array(want)).to(DEV))
    np.testing.assert_array_equal(t["photo"].cpu().numpy(), arrays[0])


def test_a_side_stream():
    from geomconsistentfr_amd import postprocess as pp
    arrays, boxes, pidx = _seam_case(True, 3, False)
    t = {n: _dev(a) for n, a in zip(NAMES, arrays)}
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x_dev = pp.ingest_group_device(t["photo"], boxes, pidx, (4, 8))
        got = pp.fullres_group_composites_device(t["photo"], boxes, pidx, t["x_lo"], t["rendered"], t["mask"])
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), group.composites(arrays[0], boxes, pidx, *arrays[1:]))
    np.testing.assert_array_equal(x_dev.cpu().numpy().view(np.uint32), group.ingest(arrays[0], boxes, pidx, 4, 8).view(np.uint32))


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("h,w", NETS)
def test_one_face_per_photograph_is_one_anybox_call(h, w, aligned):
    """the anchor, with no tolerance: photo_index = arange(B), P = B; 33 photographs cross the launch's limit of 32"""
    from geomconsistentfr_amd import postprocess as pp
    Hp, Wp = _photo_size(h, w, aligned)
    for B, L in ((3, 3), (33, 1)):
        pidx = list(range(B))
        boxes = np.array([_boxes(h, w, [0, 0, 0])[b % 3] for b in range(B)])              # large, small, mixed, large, ...
        arrays = _inputs(80 + B, B, L, h, w, Hp, Wp, boxes, pidx, B == 3)
        t = {n: _dev(a) for n, a in zip(NAMES, arrays)}
        got = pp.fullres_group_composites_device(t["photo"], boxes, pidx, t["x_lo"], t["rendered"], t["mask"])
        assert torch.equal(got, pp.fullres_anybox_composites_device(t["photo"], boxes, t["x_lo"], t["rendered"], t["mask"]))
        xa, xb = pp.ingest_group_device(t["photo"], boxes, pidx, (h, w)), pp.ingest_anybox_device(t["photo"], boxes, (h, w))
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))


def test_device_indices_and_boxes_are_refused():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    h, w = 5, 7
    arrays, boxes, pidx, _ = _case(h, w, True, "three", 1, True)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    with pytest.raises(GcfrError, match="HOST"):
        pp.fullres_group_composites_device(photo, boxes, torch.tensor(pidx).to(DEV), x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="HOST"):
        pp.fullres_group_composites_device(photo, torch.from_numpy(np.array(boxes)).to(DEV), pidx, x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="HOST"):
        pp.ingest_group_device(photo, boxes, torch.tensor(pidx).to(DEV), (h, w))
    with pytest.raises(GcfrError, match="overlap"):
        pp.fullres_group_composites_device(photo, boxes, pidx, x_lo, rendered[:, 0], mask, out=photo)
