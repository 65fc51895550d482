"""GPU: the any-size box kernels (csrc/gcfr_fullres_anybox.hip; postprocess.ingest_anybox_device /
fullres_anybox_composites_device) bit for bit against the numpy restatement (tests/fullres_anybox_emulation.py): x_lo as uint32,
composites as bytes.

  networks (h, w) in {(5,7), (4,8), (3,5), (23,17)}; on the last a 3-row box makes a photograph row cover NINE network rows, the most
           the rules allow, and a 3-column box seven columns
  boxes    (bh, bw) per network: (h-1, w-1); the smallest allowed (ceil(h/8), ceil(w/8)), 1 x 1 on the small networks; (h, w-1) and
           (h-1, w), one axis at the boundary; (2h+1, w-2) and (h-2, 4w), a lerp axis mixed with an area axis both ways;
           (h//2+1, 4), the vector path of paste=False; (h, w); each in all four corners and in the interior of photographs whose Wp
           is a multiple of four (the vector path of paste=True) and is not
  calls    B in {1, 2, 33}, every face its own box; in the pasted calls large, small and mixed boxes share a launch (the mode
           branch is per workgroup); L in {1, 3}; paste both ways; the mask shared and per face with grey levels {0, 64, 128, 255};
           `rendered` well outside [0, 1] and x_lo scaled away from the photograph's means (both saturations and both sides of
           detail_clamp occur: asserted once)
  and      every operand off its alignment; `out=` between guard bands; a side stream; a NaN under a zero mask; the anchor on the
           device (the box entries' bytes on their box sizes, fullres_composites_device's on whole power-of-two boxes); the same
           box content at another origin in another photograph returns the same box bytes."""
import numpy as np
import pytest
import torch

import fullres_anybox_emulation as anybox

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LEVELS = np.array([255, 0, 64, 128], np.uint8)
NAMES = ("photo", "x_lo", "rendered", "mask")
NETS = [(5, 7), (4, 8), (3, 5), (23, 17)]


def _sizes(h, w):
    """(bh, bw): see the module's docstring"""
    return [(h - 1, w - 1), (-(-h // 8), -(-w // 8)), (h, w - 1), (h - 1, w), (2 * h + 1, w - 2), (h - 2, 4 * w), (h // 2 + 1, 4), (h, w)]


def _photo_size(h, w, aligned):
    return 2 * h + 4, 4 * w + (4 if aligned else 5)


def _origins(Hp, Wp, bh, bw):
    """the four corners and an interior position"""
    return [(0, 0), (Wp - bw, 0), (0, Hp - bh), (Wp - bw, Hp - bh), ((Wp - bw) // 2, (Hp - bh + 1) // 2)]


def _inputs(seed, B, L, h, w, Hp, Wp, boxes, shared_mask):
    """photo (B,Hp,Wp,3) u8, x_lo (B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (1|B,h,w) u8"""
    rng = np.random.default_rng(seed)
    photo = rng.integers(0, 256, (B, Hp, Wp, 3), dtype=np.uint8)
    x_lo = (anybox.ingest(photo, boxes, h, w) * (0.1 + 1.9 * rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 1.5 * rng.standard_normal((B, L, 3, h, w))).astype(np.float32)
    MB = 1 if shared_mask else B
    mask = np.stack([rng.permutation(m) for m in np.resize(LEVELS, MB * h * w).reshape(MB, h * w)]).reshape(MB, h, w)
    return photo, x_lo, rendered, mask


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


def _check(label, arrays, boxes, misalign=(), **kw):
    from geomconsistentfr_amd import postprocess as pp
    t = {n: _dev(a, n in misalign) for n, a in zip(NAMES, arrays)}
    got = pp.fullres_anybox_composites_device(t["photo"], boxes, t["x_lo"], t["rendered"], t["mask"], **kw)
    photo, x_lo, rendered, mask = arrays
    want = anybox.composites(photo, boxes, x_lo, rendered, mask, **{k: v for k, v in kw.items() if k != "out"})
    g = got.cpu().numpy()
    print("%s: bytes that differ from the statement %d of %d" % (label, int((g != want).sum()), g.size))
    assert g.shape == want.shape and g.dtype == np.uint8
    np.testing.assert_array_equal(g, want, err_msg=label)
    return got, t


def _check_ingest(photo, boxes, h, w):
    from geomconsistentfr_amd import postprocess as pp
    want = anybox.ingest(photo, boxes, h, w)
    for mis in (False, True):
        got = pp.ingest_anybox_device(_dev(photo, mis), boxes, (h, w))
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("size", range(8))
@pytest.mark.parametrize("h,w", NETS)
def test_composites_and_ingest_equal_the_statement(h, w, size, aligned):
    bh, bw = _sizes(h, w)[size]
    Hp, Wp = _photo_size(h, w, aligned)
    origins = _origins(Hp, Wp, bh, bw)
    case = 100 * NETS.index((h, w)) + 10 * size + aligned
    for i, (B, L) in enumerate([(1, 1), (2, 3), (1, 3), (2, 1), (1, 1)]):          # every origin comes first once
        boxes = np.array([(x0, y0, bw, bh) for x0, y0 in (origins[i:] + origins)[:B]])
        shared = (case + i) % 2 == 0
        arrays = _inputs(1000 * case + i, B, L, h, w, Hp, Wp, boxes, shared)
        assert set(np.unique(arrays[3])) == set(LEVELS.tolist())
        for paste in (True, False):
            got, _ = _check("(%d,%d) box %dx%d in %dx%d B %d L %d paste %s" % (h, w, bh, bw, Hp, Wp, B, L, paste), arrays, boxes, paste=paste)
            assert tuple(got.shape) == ((B, L, Hp, Wp, 3) if paste else (B, L, bh, bw, 3))
        _check_ingest(arrays[0], boxes, h, w)
    # the interior box given once for every face, as a tuple
    one = tuple(int(v) for v in (origins[4] + (bw, bh)))
    arrays = _inputs(case, 2, 3, h, w, Hp, Wp, np.array(one), True)
    _check("one box for both faces", arrays, one)
    _check_ingest(arrays[0], one, h, w)


def _mixed_boxes(h, w, Hp, Wp, B):
    """B boxes that walk through every size of the network and every origin: large, small and mixed in one launch"""
    rows = []
    for f in range(B):
        bh, bw = _sizes(h, w)[f % 8]
        x0, y0 = _origins(Hp, Wp, bh, bw)[(f // 8 + f) % 5]
        rows.append((x0, y0, bw, bh))
    return np.array(rows)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("B,L", [(2, 3), (33, 3), (33, 1)])
@pytest.mark.parametrize("h,w", NETS)
def test_large_small_and_mixed_boxes_share_a_pasted_launch(h, w, B, L, aligned):
    from geomconsistentfr_amd import postprocess as pp
    Hp, Wp = _photo_size(h, w, aligned)
    boxes = _mixed_boxes(h, w, Hp, Wp, B)
    if B == 2:                                                                     # a small box beside a large one
        boxes = np.array([tuple(_origins(Hp, Wp, *_sizes(h, w)[1])[3]) + _sizes(h, w)[1][::-1], (0, 0, 4 * w, 2 * h + 1)])
    assert B == 2 or len({tuple(b) for b in boxes.tolist()}) >= 28                 # (on (3,5) two of the eight sizes coincide)
    for shared in (True, False):
        arrays = _inputs(50 + B + L + h, B, L, h, w, Hp, Wp, boxes, shared)
        got, t = _check("(%d,%d) mixed B %d L %d shared %s" % (h, w, B, L, shared), arrays, boxes)
    _check_ingest(arrays[0], boxes, h, w)
    # boxes as a list and as a CPU tensor of another integer type: the same bytes; a rendered without the light axis; f64
    again = pp.fullres_anybox_composites_device(t["photo"], boxes.tolist(), t["x_lo"], t["rendered"], t["mask"])
    assert torch.equal(again, got)
    one = pp.fullres_anybox_composites_device(t["photo"], torch.from_numpy(boxes).to(torch.int16), t["x_lo"], t["rendered"][:, L - 1].double(),
                                              t["mask"])
    assert one.dim() == 4 and torch.equal(one, got[:, L - 1])


@pytest.mark.parametrize("bh,bw", [(12, 4), (3, 3), (3, 8), (30, 5)])
def test_thirty_three_faces_alone_cross_the_launch_limit(bh, bw):
    h, w, B, L = 23, 17, 33, 3
    Hp, Wp = 37, 44
    rng = np.random.default_rng(33 + bh)
    boxes = np.stack([rng.integers(0, Wp - bw + 1, B), rng.integers(0, Hp - bh + 1, B), np.full(B, bw), np.full(B, bh)], axis=1)
    assert len({tuple(b) for b in boxes.tolist()}) >= 25
    arrays = _inputs(34, B, L, h, w, Hp, Wp, boxes, False)
    got, _ = _check("B 33 alone %dx%d" % (bh, bw), arrays, boxes, paste=False)
    assert tuple(got.shape) == (B, L, bh, bw, 3)
    _check_ingest(arrays[0], boxes, h, w)


def test_both_saturations_and_both_sides_of_the_clamp_occur():
    h, w = 23, 17
    Hp, Wp = _photo_size(h, w, True)
    for bh, bw in ((h - 1, w - 1), (2 * h + 1, w - 2)):
        boxes = np.array([(3, 1, bw, bh)])
        photo, x_lo, rendered, mask = _inputs(3, 1, 3, h, w, Hp, Wp, boxes, True)
        crop = photo[0, 1:1 + bh, 3:3 + bw]
        v, m, d, _ = anybox.box_terms(crop, x_lo[0], rendered[0], mask[0])
        inside = np.broadcast_to(m[None, :, :, None] > 0, v.shape)
        assert (d == 4.0).any() and (d == 0.25).any(), "both sides of detail_clamp"
        assert (v[inside] < -0.5).any() and (v[inside] > 255.5).any(), "both saturations"
        _check("regimes", (photo, x_lo, rendered, mask), boxes)
        _check("clamp 2, floor 8", (photo, x_lo, rendered, mask), boxes, detail_clamp=2.0, floor=8.0)


def test_device_boxes_are_refused():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    h, w = 5, 7
    boxes = np.array([(3, 1, 4, 3)])
    arrays = _inputs(1, 1, 1, h, w, 14, 32, boxes, True)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    with pytest.raises(GcfrError, match="HOST"):
        pp.fullres_anybox_composites_device(photo, torch.from_numpy(boxes).to(DEV), x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="HOST"):
        pp.ingest_anybox_device(photo, torch.from_numpy(boxes).to(DEV), (h, w))
    with pytest.raises(GcfrError, match="integers"):
        pp.ingest_anybox_device(photo, boxes.astype(np.float32), (h, w))
    with pytest.raises(GcfrError, match="eighth"):
        pp.ingest_anybox_device(photo, (3, 1, 4, 3), (25, 7))
    with pytest.raises(GcfrError, match="overlap"):
        pp.fullres_anybox_composites_device(photo, (0, 0, 32, 14), x_lo, rendered[:, 0], mask, out=photo)


def test_a_nan_under_a_zero_mask_reaches_nothing_and_one_inside_gives_zero_where_its_taps_reach():
    h, w, B, L = 23, 17, 2, 3
    Hp, Wp = 40, 44
    for bh, bw in ((9, 7), (9, 40), (30, 7)):
        boxes = np.array([(2, 3, bw, bh), (4, 8, bw, bh)])
        photo, x_lo, rendered, mask = _inputs(11, B, L, h, w, Hp, Wp, boxes, True)
        mask[:] = 255
        mask[0, :8, :8] = 0                                                        # every tap beside network pixel (3, 3) has mask 0
        clean, _ = _check("before the NaN", (photo, x_lo, rendered, mask), boxes)
        rendered[0, 0, 0, 3, 3] = np.nan                                           # under the zero mask: nothing changes
        got, _ = _check("NaN under the zero mask", (photo, x_lo, rendered, mask), boxes)
        assert torch.equal(got, clean)
        (b, l, c), (yy, xx) = (1, 1, 2), (15, 12)                                  # inside the mask
        rendered[b, l, c, yy, xx] = np.nan
        got, _ = _check("NaN", (photo, x_lo, rendered, mask), boxes)
        g, want = got.cpu().numpy(), clean.cpu().numpy().copy()
        changed = np.argwhere(g != want)
        assert len(changed) > 0 and (changed[:, 0] == b).all() and (changed[:, 1] == l).all() and (changed[:, 4] == c).all()
        assert (g[g != want] == 0).all()
        # a `rendered` of NaNs alone leaves every byte outside the boxes the photograph's
        rendered[:] = np.nan
        got, _ = _check("all NaN", (photo, x_lo, rendered, mask), boxes)
        outside = np.ones((B, Hp, Wp), bool)
        for i, (x0, y0, _, _) in enumerate(boxes):
            outside[i, y0:y0 + bh, x0:x0 + bw] = False
        g = got.cpu().numpy()
        for l in range(L):
            np.testing.assert_array_equal(g[:, l][outside], photo[outside])


@pytest.mark.parametrize("which", ["photo", "x_lo", "rendered", "mask", "out", "all"])
@pytest.mark.parametrize("paste", [True, False])
def test_every_operand_off_its_alignment(paste, which):
    """Wp and bw are multiples of four: aligned, both windows take the vector path; with the output one byte off, the element path
    must return the same bytes; the photograph, the f32 operands and the mask need no alignment on either path"""
    h, w, B, L = 23, 17, 2, 3
    Hp, Wp = 50, 68
    for bh, bw in ((11, 8), (30, 12), (7, 36)):
        boxes = np.array([(5, 3, bw, bh), (31, 0, bw, bh)])
        arrays = _inputs(12, B, L, h, w, Hp, Wp, boxes, False)
        mis = NAMES if which == "all" else (which,)
        kw = {}
        shape = (B, L, Hp, Wp, 3) if paste else (B, L, bh, bw, 3)
        if which in ("out", "all"):
            buf = torch.full((int(np.prod(shape)) + 1,), 0xAB, dtype=torch.uint8, device=DEV)
            kw["out"] = buf[1:].view(shape)
            assert kw["out"].data_ptr() % 4 == 1
        got, _ = _check("misaligned " + which, arrays, boxes, misalign=mis, paste=paste, **kw)
        if kw:
            assert got.data_ptr() == kw["out"].data_ptr() and int(buf[0]) == 0xAB


@pytest.mark.parametrize("paste", [True, False])
@pytest.mark.parametrize("Wp,bw", [(68, 12), (67, 11)])
def test_out_is_written_in_place_between_untouched_guard_bands(Wp, bw, paste):
    from geomconsistentfr_amd import postprocess as pp
    h, w, B, L = 23, 17, 2, 3
    Hp, bh = 40, 13                                                                # more than one workgroup per face, pasted
    boxes = np.array([(5, 3, bw, bh), (Wp - bw, Hp - bh, bw, bh)])
    arrays = _inputs(13, B, L, h, w, Hp, Wp, boxes, True)
    shape = (B, L, Hp, Wp, 3) if paste else (B, L, bh, bw, 3)
    n = int(np.prod(shape))
    buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(shape)
    got, t = _check("out=", arrays, boxes, paste=paste, out=out)
    assert got.data_ptr() == out.data_ptr() and (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all()
    again = pp.fullres_anybox_composites_device(t["photo"], boxes, t["x_lo"], t["rendered"], t["mask"], paste=paste)   # two calls: the same bytes
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)
    # the ingest writes its own output and nothing else
    x = pp.ingest_anybox_device(t["photo"], boxes, (h, w))
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), anybox.ingest(arrays[0], boxes, h, w).view(np.uint32))
    np.testing.assert_array_equal(t["photo"].cpu().numpy(), arrays[0])


def test_a_side_stream():
    from geomconsistentfr_amd import postprocess as pp
    h, w = 20, 28
    Hp, Wp = 90, 124
    boxes = np.array([(7, 5, 11, 13), (20, 0, 100, 9)])
    arrays = _inputs(14, 2, 3, h, w, Hp, Wp, boxes, False)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x_dev = pp.ingest_anybox_device(photo, boxes, (h, w))
        got = pp.fullres_anybox_composites_device(photo, boxes, x_lo, rendered, mask)
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), anybox.composites(arrays[0], boxes, *arrays[1:]))
    np.testing.assert_array_equal(x_dev.cpu().numpy().view(np.uint32), anybox.ingest(arrays[0], boxes, h, w).view(np.uint32))


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("h,w", [(5, 7), (4, 8), (3, 5)])
def test_on_the_box_entries_sizes_the_new_entries_return_their_bytes(h, w, aligned):
    """the anchor, with no tolerance: two kernels, one statement"""
    from geomconsistentfr_amd import postprocess as pp
    sizes = [(h, w), ((13 * h + 4) // 5, (13 * w + 4) // 5), (4 * h - 1, 4 * w - 1), (4 * h + 1, 4 * w + 1), (2 * h + 1, 8 * w), (4 * h, w),
             (3 * h, 4 * ((3 * w + 3) // 4)), (h + 1, 4 * w)]
    Hp, Wp = 4 * h + 3, 8 * w + (4 if aligned else 5)
    for i, (bh, bw) in enumerate(sizes):
        origins = _origins(Hp, Wp, bh, bw)
        boxes = np.array([origins[i % 5] + (bw, bh), origins[(i + 2) % 5] + (bw, bh)])
        arrays = _inputs(60 + i, 2, 3, h, w, Hp, Wp, boxes, i % 2 == 0)
        photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
        xa, xb = pp.ingest_anybox_device(photo, boxes, (h, w)), pp.ingest_box_device(photo, boxes, (h, w))
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
        for paste in (True, False):
            got = pp.fullres_anybox_composites_device(photo, boxes, x_lo, rendered, mask, paste=paste)
            assert torch.equal(got, pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, paste=paste)), (bh, bw, paste)


@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("h,w", [(4, 8), (5, 3), (20, 28)])
def test_a_whole_photograph_power_of_two_box_is_the_fullres_entries_bytes(h, w, s):
    from geomconsistentfr_amd import postprocess as pp
    B, L = 2, 3
    whole = (0, 0, s * w, s * h)
    arrays = _inputs(20 + s, B, L, h, w, s * h, s * w, np.array(whole), False)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    xa, xb = pp.ingest_anybox_device(photo, whole, (h, w)), pp.ingest_photographs_device(photo, s)
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    want = pp.fullres_composites_device(photo, x_lo, rendered, mask, s)
    for paste in (True, False):
        got = pp.fullres_anybox_composites_device(photo, whole, x_lo, rendered, mask, paste=paste)
        assert got.shape == want.shape and torch.equal(got, want)


def test_the_same_box_content_at_another_origin_in_another_photograph():
    from geomconsistentfr_amd import postprocess as pp
    h, w, L = 23, 17, 3
    rng = np.random.default_rng(40)
    for bh, bw in ((9, 8), (30, 5), (4, 40)):
        crop = rng.integers(0, 256, (bh, bw, 3), dtype=np.uint8)
        results = []
        for (Hp, Wp), (x0, y0) in (((33, 60), (0, 0)), ((33, 60), (60 - bw, 3)), ((40, 43), (1, 40 - bh)), ((bh, bw), (0, 0))):
            photo = rng.integers(0, 256, (1, Hp, Wp, 3), dtype=np.uint8)
            photo[0, y0:y0 + bh, x0:x0 + bw] = crop
            b = (x0, y0, bw, bh)
            x = pp.ingest_anybox_device(_dev(photo), b, (h, w))
            if not results:
                rendered = _dev((0.5 + 0.5 * rng.standard_normal((1, L, 3, h, w))).astype(np.float32))
                mask = _dev(rng.choice(LEVELS, (1, h, w)))
            alone = pp.fullres_anybox_composites_device(_dev(photo), b, x, rendered, mask, paste=False)
            pasted = pp.fullres_anybox_composites_device(_dev(photo), b, x, rendered, mask)
            assert torch.equal(pasted[:, :, y0:y0 + bh, x0:x0 + bw], alone)
            results.append((x, alone))
        for x, alone in results[1:]:
            assert torch.equal(x.view(torch.int32), results[0][0].view(torch.int32)) and torch.equal(alone, results[0][1])
        assert (results[0][1].cpu().numpy() != crop).any()
