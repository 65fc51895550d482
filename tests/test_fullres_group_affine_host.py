"""CPU: the group-affine feature's numpy restatement (tests/fullres_group_affine_emulation.py: per photograph the chain of
tests/fullres_affine_emulation.py's one-face composite over the photograph's faces) held to what include/gcfr.h says follows from it,
the cases of tests/test_gpu_fullres_group_affine.py shown to bite before anything runs on a device, and the host side of the entries
(csrc/gcfr_fullres_group_affine.hip, postprocess.ingest_group_affine_device / fullres_group_affine_composites_device, the
inference.relight_*_in_group_photograph_affine entries): every refusal is made before any launch, so it is exercised without a GPU.

  disjoint   faces whose quads are disjoint commute
  one mask   faces whose quads overlap but of whose carried masks at most one is positive at every pixel commute too
  two masks  a pixel relit by two faces does not commute: order matters there and nowhere else
  upright    axis-aligned maps at s in {1, 2, 4} are tests/fullres_group_emulation.py's bytes on the same overlapping boxes
  no face    a photograph without faces comes back unchanged, for every light
  anchor     one face per photograph with photo_index = arange(B) is tests/fullres_affine_emulation.py's `composites`"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import fullres_affine_emulation as affine
import fullres_group_affine_cases as cases
import fullres_group_affine_emulation as tilted
import fullres_group_emulation as group

H, W = 5, 7
LEVELS = np.array([0, 64, 128, 255], np.uint8)


def _maps(boxes):
    """(cx, cy, bw, bh, angle) per face -> (F, I)"""
    return affine.quantise(np.stack([cases.rotated_box(*b, H, W) for b in boxes]))


def _inputs(seed, P, Hp, Wp, F, pidx, L=2, mask=None):
    rng = np.random.default_rng(seed)
    B = len(pidx)
    photo = rng.integers(0, 256, (P, Hp, Wp, 3), dtype=np.uint8)
    x_lo = (tilted.ingest(photo, F, pidx, H, W) * (0.5 + rng.random((B, H, W, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 0.6 * rng.standard_normal((B, L, 3, H, W))).astype(np.float32)
    if mask is None:
        mask = rng.choice(LEVELS[1:], (B, H, W))
    return photo, x_lo, rendered, mask


def _all_orders(photo, I, pidx, x_lo, rendered, mask):
    return [tilted.composites(photo, I, pidx, x_lo, rendered, mask, order=list(o)) for o in itertools.permutations(range(len(pidx)))]


def test_disjoint_quads_commute():
    F, I = _maps([(6, 6, 9, 7, 20.0), (19, 5, 4, 3, -35.0), (8, 16, 10, 4, 90.0), (21, 14, 6, 9, 150.0)])
    pidx = [0, 0, 0, 0]
    arrays = _inputs(1, 1, 22, 26, F, pidx)
    inside = tilted.relit_counts(I, pidx, np.full((1, H, W), 255, np.uint8), 1, 22, 26, H, W)
    assert inside.max() == 1 and all((affine.inside(m, 22, 26, H, W)).any() for m in I)
    results = _all_orders(arrays[0], I, pidx, *arrays[1:])
    for r in results[1:]:
        np.testing.assert_array_equal(r, results[0])
    assert (results[0] != arrays[0][:, None]).any()
    # and each face's quad holds the one-face composite's bytes
    one = affine.composites(arrays[0][[0] * 4], I, *arrays[1:])
    for b, Im in enumerate(I):
        ins = affine.inside(Im, 22, 26, H, W)
        np.testing.assert_array_equal(results[0][0][:, ins], one[b][:, ins])


def test_overlapping_quads_with_at_most_one_positive_mask_per_pixel_commute():
    F, I = _maps([(9, 8, 14, 10, 12.0), (15, 9, 14, 10, -8.0), (5, 4, 6, 4, 30.0)])
    pidx = [0, 0, 0]
    mask = np.zeros((3, H, W), np.uint8)
    mask[0, :, 5:] = (255, 128)                                                    # face 0 relights its right, inside face 1's zero part
    mask[1, :, 6:] = 64                                                            # face 1 its right edge, beyond face 0
    mask[2, :1, 3:4] = 128                                                         # face 2 a patch on top, over face 0's zero part
    photo, x_lo, rendered, _ = _inputs(2, 1, 18, 26, F, pidx)
    relit = tilted.relit_counts(I, pidx, mask, 1, 18, 26, H, W)
    inside = tilted.relit_counts(I, pidx, np.full_like(mask, 255), 1, 18, 26, H, W)
    assert relit.max() == 1 and (inside >= 2).any() and ((inside >= 2) & (relit == 1)).any()
    assert all((tilted.relit_counts(I[b:b + 1], [0], mask[b:b + 1], 1, 18, 26, H, W) == 1).any() for b in range(3))
    results = _all_orders(photo, I, pidx, x_lo, rendered, mask)
    for r in results[1:]:
        np.testing.assert_array_equal(r, results[0])
    assert (results[0][0, 0][relit[0] == 1] != photo[0][relit[0] == 1]).any()
    np.testing.assert_array_equal(results[0][0, 1][relit[0] == 0], photo[0][relit[0] == 0])


def test_a_doubly_relit_pixel_does_not_commute_and_nothing_else_depends_on_order():
    F, I = _maps([(9, 8, 14, 10, 12.0), (15, 9, 14, 10, -8.0), (22, 2, 4, 3, 45.0)])
    pidx = [0, 0, 0]
    photo, x_lo, rendered, mask = _inputs(3, 1, 18, 26, F, pidx)
    relit = tilted.relit_counts(I, pidx, mask, 1, 18, 26, H, W)[0]
    assert relit.max() == 2 and (relit == 1).any() and (relit == 0).any()
    ab = tilted.composites(photo, I, pidx, x_lo, rendered, mask)
    ba = tilted.composites(photo, I, pidx, x_lo, rendered, mask, order=[1, 0, 2])
    differ = (ab != ba).any(axis=(1, 4))[0]
    assert differ.any() and not (differ & (relit < 2)).any()
    # the second face's composite is the one-face composite ON THE FIRST FACE'S RESULT: its gain multiplies that result
    first = affine.composites(photo, I[0], x_lo[:1], rendered[:1], mask[:1])[0]                   # (L,Hp,Wp,3)
    second = affine.composites(first, I[1], np.repeat(x_lo[1:2], 2, 0), rendered[1][:, None], mask[1:2])
    third = affine.composites(second[:, 0], I[2], np.repeat(x_lo[2:3], 2, 0), rendered[2][:, None], mask[2:3])
    np.testing.assert_array_equal(ab[0], third[:, 0])


@pytest.mark.parametrize("aligned", [True, False])
def test_upright_maps_are_the_group_restatement_on_the_same_overlapping_boxes(aligned):
    arrays, (F, I), boxes, pidx = cases.upright_case(aligned)
    h, w = cases.UPRIGHT_NET
    photo, x_lo, rendered, mask = arrays
    P, Hp, Wp, _ = photo.shape
    assert {int(b[2]) // w for b in boxes} == {1, 2, 4}
    relit = tilted.relit_counts(I, pidx, mask, P, Hp, Wp, h, w)
    assert (relit[0] >= 2).any() and (relit[1] >= 2).any(), "the boxes overlap where both relight"
    np.testing.assert_array_equal(relit, group.relit_counts(boxes, pidx, mask, P, Hp, Wp, h, w))
    got = tilted.composites(photo, I, pidx, x_lo, rendered, mask)
    np.testing.assert_array_equal(got, group.composites(photo, boxes, pidx, x_lo, rendered, mask))
    assert (got != photo[:, None]).any()
    # (the ingests agree at every scale: one block mean)
    np.testing.assert_array_equal(tilted.ingest(photo, F, pidx, h, w).view(np.uint32), group.ingest(photo, boxes, pidx, h, w).view(np.uint32))


def test_a_photograph_without_faces_comes_back_unchanged_and_indices_may_come_in_any_order():
    F, I = _maps([(9, 8, 14, 10, 12.0), (15, 9, 14, 10, -8.0), (5, 5, 4, 3, 200.0), (12, 8, 24, 16, 3.0)])
    pidx = [2, 0, 2, 0]
    photo, x_lo, rendered, mask = _inputs(4, 3, 16, 24, F, pidx, L=3)
    got = tilted.composites(photo, I, pidx, x_lo, rendered, mask)
    assert got.shape == (3, 3, 16, 24, 3) and got.dtype == np.uint8
    for l in range(3):
        np.testing.assert_array_equal(got[1, l], photo[1])
    # every photograph on its own: the chain over its faces in ascending face index
    for q, faces in ((0, [1, 3]), (2, [0, 2])):
        alone = tilted.composites(photo[q:q + 1], I[faces], [0, 0], x_lo[faces], rendered[faces], mask[faces])
        np.testing.assert_array_equal(got[q], alone[0])
        assert (got[q] != photo[q][None]).any()
    # the ingest reads photograph photo_index[b] through F[b]
    x = tilted.ingest(photo, F, pidx, H, W)
    np.testing.assert_array_equal(x.view(np.uint32), affine.ingest(photo[pidx], F, H, W).view(np.uint32))


def test_one_face_per_photograph_is_the_affine_restatement():
    rng = np.random.default_rng(5)
    F, I = _maps([(10, 8, 7, 5, 0.0), (20, 15, 23, 17, 33.0), (9, 11, 3, 2, -70.0), (16, 4, 30, 3, 5.0)])
    pidx = list(range(4))
    for shared in (True, False):
        photo, x_lo, rendered, mask = _inputs(5, 4, 30, 40, F, pidx, L=3, mask=rng.choice(LEVELS, (1 if shared else 4, H, W)))
        np.testing.assert_array_equal(tilted.composites(photo, I, pidx, x_lo, rendered, mask), affine.composites(photo, I, x_lo, rendered, mask))
        np.testing.assert_array_equal(tilted.ingest(photo, F, pidx, H, W).view(np.uint32), affine.ingest(photo, F, H, W).view(np.uint32))


# ------------------------------------------------------------------------------------------------
# the cases of the GPU test bite
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
def test_the_cases_of_the_gpu_test_bite(aligned):
    """nothing here touches a device"""
    h, w = cases.H, cases.W
    arrays, (F, I), pidx, want = cases.case(aligned, "three", 3, False)
    photo, x_lo, rendered, mask = arrays
    P, Hp, Wp, _ = photo.shape
    assert [affine.sub_samples(I[b]) for b in (1, 4, 7)] == [1, 2, 1], "the small face is sub-sampled on the way out"
    relit = tilted.relit_counts(I, pidx, mask, P, Hp, Wp, h, w)
    inside = tilted.relit_counts(I, pidx, np.full_like(mask, 255), P, Hp, Wp, h, w)
    counts = [int((relit[q] >= 2).sum()) for q in range(P)], [int((relit[q] == 3).sum()) for q in range(P)]
    print("relit by two or more %s, by all three %s, inside two quads and relit by one %s, in no quad %s"
          % (counts + ([int(((inside[q] >= 2) & (relit[q] == 1)).sum()) for q in range(P)], [int((inside[q] == 0).sum()) for q in range(P)])))
    for q in range(P):
        assert (inside[q] == 0).sum() == cases.NO_QUAD[aligned], "the geometry of the issue"
        assert (relit[q] >= 2).any(), "some pixel is relit by two faces"
        assert (relit[q] == 3).any(), "and some by all three"
        assert ((inside[q] >= 2) & (relit[q] == 1)).any(), "a face crosses another where its own carried mask is zero"
        assert ((inside[q] == 1) & (relit[q] == 0)).any()
    # photograph 0: faces 1, 4, 7 are its 17-degree, its -40-degree and its quarter-turn face
    assert [cases.kinds_of(pidx)[b] for b in (1, 4, 7)] == [0, 1, 2]
    big, small = 1, 4
    both = np.zeros((Hp, Wp), np.int64)
    for b in (big, small):
        both += tilted.relit_counts(I[b:b + 1], [0], mask[b:b + 1], 1, Hp, Wp, h, w)[0]
    assert (both == 2).any()
    order = list(range(len(pidx)))
    order[big], order[small] = small, big
    swapped = tilted.composites(photo, I, pidx, x_lo, rendered, mask, order=order)
    differ = (swapped != want).any(axis=(1, 4))
    assert differ[0].any(), "swapping the two faces changes bytes"
    assert not differ[1:].any() and not (differ[0] & (both < 2)).any(), "order matters where both relight a pixel and nowhere else"
    # the regimes, on the faces' first composites and on a second one
    d_all, v_all = [], []
    for b in range(len(pidx)):
        for source in (photo[pidx[b]], want[pidx[b], 0]):
            v, m, d, ins = affine.face_terms(source, I[b], x_lo[b], rendered[b], mask[b])
            d_all.append(d[ins].ravel())
            v_all.append(v[np.broadcast_to(((m > 0) & ins)[None, :, :, None], v.shape)])
    d_all, v_all = np.concatenate(d_all), np.concatenate(v_all)
    assert (d_all == 4.0).any() and (d_all == 0.25).any(), "both sides of detail_clamp"
    assert (v_all < -0.5).any() and (v_all > 255.5).any(), "both saturations"


@pytest.mark.parametrize("aligned", [True, False])
def test_the_seam_case_relights_in_the_continuation_what_an_earlier_launch_relit(aligned):
    arrays, (F, I), pidx, want = cases.seam_case(aligned, 1, False)
    h, w = cases.SEAM_NET
    photo, mask = arrays[0], arrays[3]
    P, Hp, Wp, _ = photo.shape
    in_1 = [b for b, q in enumerate(pidx) if q == 1]
    assert len(in_1) == 34 and pidx.count(0) == 1 and pidx[10] == 0
    pick = lambda faces: (I[faces], [pidx[b] for b in faces], mask[faces])
    early = tilted.relit_counts(*pick(in_1[:32]), P, Hp, Wp, h, w)[1]
    late = tilted.relit_counts(*pick(in_1[32:]), P, Hp, Wp, h, w)[1]
    assert ((early > 0) & (late > 0)).any(), "a face of the continuation launch relights what an earlier launch's face relit"
    assert (early >= 2).any() and (early == 0).any()
    # and it shows in the bytes: without faces 32 and 33 the result differs
    keep = [b for b in range(len(pidx)) if b not in in_1[32:]]
    without = tilted.composites(photo, I[keep], [pidx[b] for b in keep], arrays[1][keep], arrays[2][keep], mask[keep])
    assert (without[1] != want[1]).any() and (without[0] == want[0]).all()


# ------------------------------------------------------------------------------------------------
# the entries' host side
# ------------------------------------------------------------------------------------------------
ONE = 1 << 14
GOOD_MAPS = [[[2 * ONE, 0, 3 * ONE], [0, 2 * ONE, 2 * ONE]], [[ONE, -ONE, 20 * ONE], [ONE, ONE, 5 * ONE]], [[0, -ONE // 2, 9 * ONE], [ONE // 2, 0, 4 * ONE]]]


def _host(values, dtype):
    a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_the_c_entries_refuse_before_any_launch():
    """junk device pointers throughout: every call below must return before it launches"""
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = lambda v: ctypes.c_void_p(v)
    ok = dict(photo=p(1 << 20), x_lo=p(128), rendered=p(256), mask=p(512), mask_batch=1, P=2, B=3, L=3, Hp=30, Wp=40, h=17, w=23,
              floor=1.0, clamp=4.0, out=p(1 << 30), maps=GOOD_MAPS, index=[1, 0, 1])

    def comp(**kw):
        a = dict(ok, **kw)
        km, mp = (None, None) if a["maps"] is None else _host(a["maps"], np.int64)
        ki, ip = (None, None) if a["index"] is None else _host(a["index"], np.int32)
        return L.gcfr_fullres_composites_group_affine_u8(a["photo"], a["x_lo"], a["rendered"], a["mask"], a["mask_batch"], a["P"], a["B"],
                                                         a["L"], a["Hp"], a["Wp"], mp, ip, a["h"], a["w"], a["floor"], a["clamp"], a["out"],
                                                         None)

    def ing(**kw):
        a = dict(ok, **kw)
        km, mp = (None, None) if a["maps"] is None else _host(a["maps"], np.int64)
        ki, ip = (None, None) if a["index"] is None else _host(a["index"], np.int32)
        return L.gcfr_ingest_group_affine_u8(a["photo"], a["P"], a["Hp"], a["Wp"], mp, ip, a["B"], a["h"], a["w"], a["x_lo"], None)

    for name in ("photo", "x_lo", "rendered", "mask", "out", "maps", "index"):
        assert comp(**{name: None}) == -1, name
    for name in ("photo", "x_lo", "maps", "index"):
        assert ing(**{name: None}) == -1, name
    for index in ([1, 0, 2], [-1, 0, 1], [1, 0, 1 << 30], [2, 2, 2]):                # outside [0, P)
        assert comp(index=index) == -1 and ing(index=index) == -1, index
    last = lambda m: GOOD_MAPS[:2] + [m]
    bad_maps = [last([[ONE, 0, 0], [0, -ONE, 0]]), last([[0, ONE, 0], [ONE, 0, 0]]), last([[ONE, ONE, 0], [ONE, ONE, 0]]),      # det <= 0
                last([[0, 0, 0], [0, 0, 0]]),
                last([[8 * ONE + 1, 0, 0], [0, ONE, 0]]), last([[6 * ONE, -6 * ONE, 0], [6 * ONE, 6 * ONE, 0]]),                # a column > 8
                last([[ONE, 0, (1 << 40) + 1], [0, ONE, 0]]), last([[ONE, 0, 0], [0, ONE, -(1 << 40) - 1]]),                    # translations
                [[[ONE, 0, 0], [0, -ONE, 0]]] + GOOD_MAPS[1:]]
    for m in bad_maps:
        assert comp(maps=m) == -1 and ing(maps=m) == -1, m
    # a refused map behind the first 32 faces
    many = [GOOD_MAPS[b % 3] for b in range(40)]
    many[37] = [[ONE, 0, 0], [0, -ONE, 0]]
    assert comp(B=40, maps=many, index=[b % 2 for b in range(40)]) == -1 and ing(B=40, maps=many, index=[b % 2 for b in range(40)]) == -1
    # Hp Wp, h w and P chunks in 31 bits
    one = dict(P=1, B=1, index=[0], maps=GOOD_MAPS[:1])
    for d in (dict(one, Hp=1 << 16, Wp=1 << 16), dict(one, h=1 << 16, w=1 << 16), dict(one, P=1 << 12, Hp=1 << 15, Wp=1 << 15)):
        assert comp(**d) == -1 and ing(**d) == -1
    for name in ("P", "B", "h", "w", "Hp", "Wp"):
        assert comp(**{name: 0}) == -1 and ing(**{name: 0}) == -1 and comp(**{name: -1}) == -1 and ing(**{name: -1}) == -1, name
    # what gcfr_fullres_composites_u8 refuses
    assert comp(L=0) == -1 and comp(L=4097) == -1 and comp(L=-1) == -1
    assert comp(mask_batch=0) == -1 and comp(mask_batch=2) == -1 and comp(mask_batch=4) == -1       # 1 or B = 3; P = 2 is not it
    assert comp(clamp=0.99) == -1 and comp(clamp=float("nan")) == -1
    assert comp(floor=0.0) == -1 and comp(floor=-1.0) == -1 and comp(floor=float("nan")) == -1
    # an out that overlaps the photographs (2 x 30 x 40 x 3 = 7200 bytes from 1 << 20; out is 3 x 7200 bytes)
    for out in ((1 << 20), (1 << 20) + 7199, (1 << 20) - 1, (1 << 20) - 3 * 7200 + 1):
        assert comp(out=p(out)) == -1, out
    assert ing(x_lo=p(1 << 20)) == -1                                             # x_lo_out == photo


def test_the_python_entries_refuse_malformed_operands_without_a_gpu():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    P, B, L, h, w, Hp, Wp = 2, 3, 3, 17, 23, 30, 40
    photo = torch.zeros((P, Hp, Wp, 3), dtype=torch.uint8)
    x_lo = torch.zeros((B, h, w, 3))
    rendered = torch.zeros((B, L, 3, h, w))
    mask = torch.zeros((h, w), dtype=torch.uint8)
    A = np.array(GOOD_MAPS, np.float64) / ONE
    pair = pp.quantise_affine(A)
    index = [1, 0, 1]
    bad_index = [[1, 0, 2], [-1, 0, 1], [1, 0], [1, 0, 1, 0], [[1, 0, 1]], 1, [1.0, 0.0, 1.0], np.zeros(B, np.float32), torch.zeros(B),
                 np.zeros(B, bool), "101", None, []]                               # (None: all zeros, which needs P == 1)
    mirror = A.copy()
    mirror[2, 1] *= -1.0
    bad_maps = [A[:2], np.concatenate([A, A[:1]]), A[0, :, :2], "map", None, mirror, A * 9.0, A * np.nan, (pair[0], pair[1][:2]),
                (pair[0].astype(np.float64), pair[1]), (pair[0], -pair[1])]
    bad = [dict(photo_index=i) for i in bad_index] + [dict(net_to_photo=m) for m in bad_maps] + [
        dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(photo_u8=photo.numpy()), dict(photo_u8=photo[..., :2]),
        dict(x_lo=x_lo[:2]), dict(x_lo=x_lo.double()), dict(x_lo=x_lo.permute(0, 3, 1, 2)), dict(x_lo=x_lo[0]),
        dict(rendered=rendered[:, :, :2]), dict(rendered=rendered[:2]), dict(rendered=rendered[0, 0]), dict(rendered=rendered.to(torch.int32)),
        dict(rendered=torch.zeros((B, 0, 3, h, w))), dict(rendered=torch.zeros((P, L, 3, h, w))),
        dict(mask_u8=mask.float()), dict(mask_u8=torch.zeros((4, 5), dtype=torch.uint8)), dict(mask_u8=torch.zeros((P, h, w), dtype=torch.uint8)),
        dict(detail_clamp=0.5), dict(detail_clamp=float("nan")), dict(floor=0.0), dict(floor=-2.0),
        dict(out=torch.zeros((P, L, Hp, Wp, 3))), dict(out=torch.zeros((P, Hp, Wp, 3), dtype=torch.uint8)),
        dict(out=torch.zeros((B, L, Hp, Wp, 3), dtype=torch.uint8)), dict(out=torch.zeros((P, L, Hp, Wp, 3), dtype=torch.uint8)[:, :, :, ::1, :2]),
    ]
    for kw in bad:
        a = dict(photo_u8=photo, net_to_photo=A, photo_index=index, x_lo=x_lo, rendered=rendered, mask_u8=mask)
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.fullres_group_affine_composites_device(**a)
    for kw in (dict(paste=False), dict(upsample="guided")):                        # neither exists here
        with pytest.raises(TypeError):
            pp.fullres_group_affine_composites_device(photo, A, index, x_lo, rendered, mask, **kw)
    with pytest.raises(GcfrError, match=r"\[0, 2\)"):
        pp.fullres_group_affine_composites_device(photo, A, [1, 0, 2], x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="one photograph"):
        pp.fullres_group_affine_composites_device(photo, A, None, x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="determinant"):
        pp.fullres_group_affine_composites_device(photo, mirror, index, x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="longer than 8"):
        pp.ingest_group_affine_device(photo, A * 9.0, index, (h, w))
    # `out` overlapping the photographs: one buffer, the photographs in front and the result behind, one byte too early
    n_photo, n_out = photo.numel(), P * L * Hp * Wp * 3
    buf = torch.zeros(n_photo + n_out, dtype=torch.uint8)
    ph = buf[:n_photo].view(P, Hp, Wp, 3)
    with pytest.raises(GcfrError, match="overlap"):
        pp.fullres_group_affine_composites_device(ph, A, index, x_lo, rendered, mask, out=buf[n_photo - 1:n_photo - 1 + n_out].view(P, L, Hp, Wp, 3))
    with pytest.raises(GcfrError, match="overlap"):
        pp.fullres_group_affine_composites_device(photo, A, index, x_lo, rendered[:, 0], mask, out=photo)
    with pytest.raises(GcfrError, match="no CPU path"):                           # right behind them: allowed
        pp.fullres_group_affine_composites_device(ph, A, index, x_lo, rendered, mask, out=buf[n_photo:].view(P, L, Hp, Wp, 3))
    # well-formed host tensors: there is no CPU path.  The indices as a list, an array or a CPU tensor; the map as f64 numbers, as the
    # integer pair, as one matrix for every face
    for i in (index, np.array(index), np.array(index, dtype=np.uint8), torch.tensor(index), torch.tensor(index, dtype=torch.int16), [0, 0, 0]):
        for m in (A, A.tolist(), torch.from_numpy(A), pair, (torch.from_numpy(pair[0]), pair[1]), A[1], (pair[0][1], pair[1][1])):
            with pytest.raises(GcfrError, match="no CPU path"):
                pp.fullres_group_affine_composites_device(photo, m, i, x_lo, rendered, mask)
            with pytest.raises(GcfrError, match="no CPU path"):
                pp.ingest_group_affine_device(photo, m, i, (h, w))
    with pytest.raises(GcfrError, match="no CPU path"):                           # None with ONE photograph: every face in it
        pp.fullres_group_affine_composites_device(photo[:1], A, None, x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="no CPU path"):                           # ... and the ingest takes B from the map
        pp.ingest_group_affine_device(photo[:1], A, None, 23)
    with pytest.raises(GcfrError, match="no CPU path"):
        pp.ingest_group_affine_device(photo[:1], pair, None, 23)
    for kw in [dict(photo_index=i) for i in bad_index[:1] + bad_index[1:2] + bad_index[4:]] + [dict(net_to_photo=m) for m in bad_maps] + [
            dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(size=0), dict(size=(5,)), dict(size=(5.0, 7.0)), dict(size=None)]:
        a = dict(photo_u8=photo, net_to_photo=A, photo_index=index, size=(h, w))
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.ingest_group_affine_device(**a)
    # the ingest takes B from the indices: two faces or four need as many maps
    for i in ([1, 0], [1, 0, 1, 0]):
        with pytest.raises(GcfrError, match="map"):
            pp.ingest_group_affine_device(photo, A, i, (h, w))


def test_the_inference_entries_exist_and_refuse_malformed_operands():
    import inspect
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd._lib import GcfrError
    names = ("relight_lights_in_group_photograph_affine", "relight_lights_in_group_photograph_affine_device",
             "relight_rig_in_group_photograph_affine", "relight_rig_in_group_photograph_affine_device")
    for name in names:
        sig = inspect.signature(getattr(inf, name))
        assert "upsample" not in sig.parameters and "paste" not in sig.parameters and sig.parameters["light_frame"].default == "face"
        assert list(sig.parameters)[1:4] == ["photos_u8", "net_to_photo", "photo_index"]
    mask = np.zeros((17, 23), np.uint8)
    photos = np.zeros((2, 30, 40, 3), np.uint8)
    A = np.array(GOOD_MAPS, np.float64) / ONE
    lights = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    with pytest.raises(GcfrError, match="uint8"):
        inf.relight_lights_in_group_photograph_affine_device(None, photos.astype(np.float32), A, [1, 0, 1], mask, lights, device="cpu")
    with pytest.raises(GcfrError, match="light_frame"):
        inf.relight_lights_in_group_photograph_affine_device(None, photos, A, [1, 0, 1], mask, lights, device="cpu", light_frame="world")
    mirror = A.copy()
    mirror[2, 1] *= -1.0
    for m, i in ((A, [1, 0, 2]), (A, [1, 0]), (A, None), (A, [1.0, 0.0, 1.0]), (A[:2], [1, 0, 1]), (mirror, [1, 0, 1]), (A * 9.0, [1, 0, 1])):
        for frame in ("face", "photograph"):
            with pytest.raises(GcfrError):
                inf.relight_lights_in_group_photograph_affine_device(None, photos, m, i, mask, lights, device="cpu", light_frame=frame)
            with pytest.raises(GcfrError):
                inf.relight_rig_in_group_photograph_affine_device(None, photos, m, i, mask, lights, None, device="cpu", light_frame=frame)
            with pytest.raises(GcfrError):
                inf.relight_lights_in_group_photograph_affine(None, photos, m, i, mask, lights, device="cpu", light_frame=frame)
            with pytest.raises(GcfrError):
                inf.relight_rig_in_group_photograph_affine(None, photos, m, i, mask, lights, None, device="cpu", light_frame=frame)
    with pytest.raises(GcfrError, match="mask_u8"):
        inf.relight_lights_in_group_photograph_affine_device(None, photos, A, [1, 0, 1], np.zeros((2, 17, 23), np.uint8), lights, device="cpu")
    # well-formed: every check passes; a single (Hp,Wp,3) photograph with photo_index=None; the lights in the photograph's frame
    with pytest.raises(GcfrError, match="no CPU path"):
        inf.relight_lights_in_group_photograph_affine_device(None, photos, A, [1, 0, 1], mask, lights, device="cpu")
    with pytest.raises(GcfrError, match="no CPU path"):
        inf.relight_rig_in_group_photograph_affine_device(None, photos[0], A, None, mask, lights, None, device="cpu", light_frame="photograph")
