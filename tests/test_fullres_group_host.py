"""CPU: the group-photograph feature's numpy restatement (tests/fullres_group_emulation.py: per photograph and light the chain of
tests/fullres_anybox_emulation.py's one-face composite over the photograph's faces) held to what include/gcfr.h says follows from
it, and the host side of its entries (csrc/gcfr_fullres_group.hip, postprocess.ingest_group_device /
fullres_group_composites_device, the inference.relight_*_in_group_photograph entries): every refusal is made before any launch, so
it is exercised without a GPU.

  disjoint   faces whose boxes are disjoint commute
  one mask   faces whose boxes overlap but of whose carried masks at most one is positive at every pixel commute too
  two masks  a pixel relit by two faces does not commute: order matters there and nowhere else
  no face    a photograph without faces comes back unchanged, for every light
  anchor     one face per photograph with photo_index = arange(B) is tests/fullres_anybox_emulation.py's `composites`"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import fullres_anybox_emulation as anybox
import fullres_group_emulation as group

H, W = 5, 7
LEVELS = np.array([0, 64, 128, 255], np.uint8)


def _inputs(seed, P, Hp, Wp, boxes, pidx, L=2, mask=None):
    rng = np.random.default_rng(seed)
    B = len(pidx)
    photo = rng.integers(0, 256, (P, Hp, Wp, 3), dtype=np.uint8)
    x_lo = (group.ingest(photo, boxes, pidx, H, W) * (0.5 + rng.random((B, H, W, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 0.6 * rng.standard_normal((B, L, 3, H, W))).astype(np.float32)
    if mask is None:
        mask = rng.choice(LEVELS[1:], (B, H, W))
    return photo, x_lo, rendered, mask


def _all_orders(photo, boxes, pidx, x_lo, rendered, mask):
    return [group.composites(photo, boxes, pidx, x_lo, rendered, mask, order=list(o)) for o in itertools.permutations(range(len(pidx)))]


def test_disjoint_boxes_commute():
    boxes = np.array([(0, 0, 9, 6), (9, 0, 4, 3), (2, 6, 20, 4), (22, 7, 3, 11)])      # a large, a small, two mixed; they touch
    pidx = [0, 0, 0, 0]
    arrays = _inputs(1, 1, 20, 26, boxes, pidx)
    inside = group.relit_counts(boxes, pidx, np.full((1, H, W), 255, np.uint8), 1, 20, 26, H, W)
    assert inside.max() == 1
    results = _all_orders(arrays[0], boxes, pidx, *arrays[1:])
    for r in results[1:]:
        np.testing.assert_array_equal(r, results[0])
    assert (results[0] != arrays[0][:, None]).any()
    # and each face's box holds the one-face composite's bytes
    one = anybox.composites(arrays[0][[0] * 4], boxes, *arrays[1:])
    for b, (x0, y0, bw, bh) in enumerate(boxes):
        np.testing.assert_array_equal(results[0][0, :, y0:y0 + bh, x0:x0 + bw], one[b, :, y0:y0 + bh, x0:x0 + bw])


def test_overlapping_boxes_with_at_most_one_positive_mask_per_pixel_commute():
    boxes = np.array([(1, 2, 14, 10), (8, 4, 14, 10), (10, 1, 6, 4)])
    pidx = [0, 0, 0]
    mask = np.zeros((3, H, W), np.uint8)
    mask[0, :, :2] = (255, 128)                                                    # face 0 relights its left
    mask[1, :, 5:] = (64, 255)                                                     # face 1 its right
    mask[2, :2, 3:5] = 128                                                         # face 2 a patch on top, over face 0's zero part
    photo, x_lo, rendered, _ = _inputs(2, 1, 16, 24, boxes, pidx)
    relit = group.relit_counts(boxes, pidx, mask, 1, 16, 24, H, W)
    inside = group.relit_counts(boxes, pidx, np.full_like(mask, 255), 1, 16, 24, H, W)
    assert relit.max() == 1 and (inside >= 2).any() and ((inside >= 2) & (relit == 1)).any()
    results = _all_orders(photo, boxes, pidx, x_lo, rendered, mask)
    for r in results[1:]:
        np.testing.assert_array_equal(r, results[0])
    assert (results[0][0, 0][relit[0] == 1] != photo[0][relit[0] == 1]).any()
    np.testing.assert_array_equal(results[0][0, 1][relit[0] == 0], photo[0][relit[0] == 0])


def test_a_doubly_relit_pixel_does_not_commute_and_nothing_else_depends_on_order():
    boxes = np.array([(1, 2, 14, 10), (8, 4, 14, 10), (20, 0, 4, 3)])
    pidx = [0, 0, 0]
    photo, x_lo, rendered, mask = _inputs(3, 1, 16, 24, boxes, pidx)
    relit = group.relit_counts(boxes, pidx, mask, 1, 16, 24, H, W)[0]
    assert relit.max() == 2 and (relit == 1).any() and (relit == 0).any()
    ab = group.composites(photo, boxes, pidx, x_lo, rendered, mask)
    ba = group.composites(photo, boxes, pidx, x_lo, rendered, mask, order=[1, 0, 2])
    differ = (ab != ba).any(axis=(1, 4))[0]
    assert differ.any() and not (differ & (relit < 2)).any()
    # the second face's composite is the one-face composite ON THE FIRST FACE'S RESULT: its gain multiplies that result
    first = anybox.composites(photo, boxes[0], x_lo[:1], rendered[:1], mask[:1])[0]              # (L,Hp,Wp,3)
    second = anybox.composites(first, boxes[1], np.repeat(x_lo[1:2], 2, 0), rendered[1][:, None], mask[1:2])
    third = anybox.composites(second[:, 0], boxes[2], np.repeat(x_lo[2:3], 2, 0), rendered[2][:, None], mask[2:3])
    np.testing.assert_array_equal(ab[0], third[:, 0])


def test_a_photograph_without_faces_comes_back_unchanged_and_indices_may_come_in_any_order():
    boxes = np.array([(1, 2, 14, 10), (8, 4, 14, 10), (3, 3, 4, 3), (0, 0, 24, 16)])
    pidx = [2, 0, 2, 0]
    photo, x_lo, rendered, mask = _inputs(4, 3, 16, 24, boxes, pidx, L=3)
    got = group.composites(photo, boxes, pidx, x_lo, rendered, mask)
    assert got.shape == (3, 3, 16, 24, 3) and got.dtype == np.uint8
    for l in range(3):
        np.testing.assert_array_equal(got[1, l], photo[1])
    # every photograph on its own: the chain over its faces in ascending face index
    for q, faces in ((0, [1, 3]), (2, [0, 2])):
        alone = group.composites(photo[q:q + 1], boxes[faces], [0, 0], x_lo[faces], rendered[faces], mask[faces])
        np.testing.assert_array_equal(got[q], alone[0])
        assert (got[q] != photo[q][None]).any()
    # the ingest reads box b of photograph photo_index[b]
    x = group.ingest(photo, boxes, pidx, H, W)
    np.testing.assert_array_equal(x.view(np.uint32), anybox.ingest(photo[pidx], boxes, H, W).view(np.uint32))


def test_one_face_per_photograph_is_the_anybox_restatement():
    rng = np.random.default_rng(5)
    boxes = np.array([(0, 0, 7, 5), (3, 9, 23, 17), (8, 10, 3, 2), (1, 1, 30, 3)])
    pidx = list(range(4))
    for shared in (True, False):
        photo, x_lo, rendered, mask = _inputs(5, 4, 30, 40, boxes, pidx, L=3, mask=rng.choice(LEVELS, (1 if shared else 4, H, W)))
        np.testing.assert_array_equal(group.composites(photo, boxes, pidx, x_lo, rendered, mask),
                                      anybox.composites(photo, boxes, x_lo, rendered, mask))
        np.testing.assert_array_equal(group.ingest(photo, boxes, pidx, H, W).view(np.uint32), anybox.ingest(photo, boxes, H, W).view(np.uint32))


# ------------------------------------------------------------------------------------------------
# the entries' host side
# ------------------------------------------------------------------------------------------------
def _host_ints(values, cols):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1, cols) if cols > 1 else np.asarray(values, dtype=np.int32))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_the_c_entries_refuse_before_any_launch():
    """junk device pointers throughout: every call below must return before it launches"""
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = lambda v: ctypes.c_void_p(v)
    # a (17, 23) network: a 5 x 4 box is allowed (8 x 5 >= 23, 8 x 4 >= 17), a 2-wide or 2-high one is not
    ok = dict(photo=p(1 << 20), x_lo=p(128), rendered=p(256), mask=p(512), mask_batch=1, P=2, B=3, L=3, Hp=30, Wp=40, h=17, w=23,
              floor=1.0, clamp=4.0, out=p(1 << 30), boxes=[(3, 2, 5, 4), (20, 15, 5, 4), (4, 3, 30, 20)], index=[1, 0, 1])

    def comp(**kw):
        a = dict(ok, **kw)
        kb, bp = (None, None) if a["boxes"] is None else _host_ints(a["boxes"], 4)
        ki, ip = (None, None) if a["index"] is None else _host_ints(a["index"], 1)
        return L.gcfr_fullres_composites_group_u8(a["photo"], a["x_lo"], a["rendered"], a["mask"], a["mask_batch"], a["P"], a["B"], a["L"],
                                                  a["Hp"], a["Wp"], bp, ip, a["h"], a["w"], a["floor"], a["clamp"], a["out"], None)

    def ing(**kw):
        a = dict(ok, **kw)
        kb, bp = (None, None) if a["boxes"] is None else _host_ints(a["boxes"], 4)
        ki, ip = (None, None) if a["index"] is None else _host_ints(a["index"], 1)
        return L.gcfr_ingest_group_u8(a["photo"], a["P"], a["Hp"], a["Wp"], bp, ip, a["B"], a["h"], a["w"], a["x_lo"], None)

    for name in ("photo", "x_lo", "rendered", "mask", "out", "boxes", "index"):
        assert comp(**{name: None}) == -1, name
    for name in ("photo", "x_lo", "boxes", "index"):
        assert ing(**{name: None}) == -1, name
    for index in ([1, 0, 2], [-1, 0, 1], [1, 0, 1 << 30], [2, 2, 2]):                # outside [0, P)
        assert comp(index=index) == -1 and ing(index=index) == -1, index
    last = lambda *b: [(3, 2, 5, 4), (20, 15, 5, 4), b]
    bad_boxes = [last(-1, 15, 5, 4), last(20, -1, 5, 4), last(36, 15, 5, 4), last(20, 27, 5, 4),                       # outside
                 last(20, 15, 2, 4), last(20, 15, 5, 2), last(20, 15, 0, 4), last(20, 15, 5, 0), last(20, 15, -5, 4),  # 8 nb < n, nb < 1
                 last(0, 0, 41, 4), last(0, 0, 5, 31), last(2 ** 31 - 4, 0, 5, 4), [(38, 2, 5, 4), (20, 15, 5, 4), (4, 3, 30, 20)]]
    for b in bad_boxes:
        assert comp(boxes=b) == -1 and ing(boxes=b) == -1, b
    # 2 bh h, 2 bw w in 31 bits; Hp Wp and P chunks in 31 bits
    one = dict(P=1, B=1, index=[0])
    for d in (dict(one, Hp=1 << 15, Wp=1, h=1 << 15, w=1, boxes=[(0, 0, 1, 1 << 15)]), dict(one, Hp=1, Wp=1 << 14, h=1, w=1 << 16, boxes=[(0, 0, 1 << 14, 1)]),
              dict(one, Hp=1 << 16, Wp=1 << 16, boxes=[(0, 0, 5, 4)]), dict(one, P=1 << 12, Hp=1 << 15, Wp=1 << 15, boxes=[(0, 0, 5, 4)])):
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
    boxes = [(3, 2, 5, 4), (20, 15, 5, 4), (4, 3, 30, 20)]
    index = [1, 0, 1]
    bad_index = [[1, 0, 2], [-1, 0, 1], [1, 0], [1, 0, 1, 0], [[1, 0, 1]], 1, [1.0, 0.0, 1.0], np.zeros(B, np.float32), torch.zeros(B),
                 np.zeros(B, bool), "101", None, []]                               # (None: all zeros, which needs P == 1)
    bad_boxes = [boxes[:2], boxes + boxes[:1], (3, 2, 5), [(3.0, 2.0, 5.0, 4.0)] * 3, np.zeros((B, 4), np.float32), "box", None,
                 (-1, 2, 5, 4), (36, 2, 5, 4), (3, 27, 5, 4), (3, 2, 2, 4), (3, 2, 5, 2), (3, 2, 0, 4), (0, 0, 41, 4), (0, 0, 5, 31)]
    bad = [dict(photo_index=i) for i in bad_index] + [dict(boxes=b) for b in bad_boxes] + [
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
        a = dict(photo_u8=photo, boxes=boxes, photo_index=index, x_lo=x_lo, rendered=rendered, mask_u8=mask)
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.fullres_group_composites_device(**a)
    for kw in (dict(paste=False), dict(upsample="guided")):                        # neither exists here
        with pytest.raises(TypeError):
            pp.fullres_group_composites_device(photo, boxes, index, x_lo, rendered, mask, **kw)
    with pytest.raises(GcfrError, match=r"\[0, 2\)"):
        pp.fullres_group_composites_device(photo, boxes, [1, 0, 2], x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="one photograph"):
        pp.fullres_group_composites_device(photo, boxes, None, x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="eighth"):
        pp.fullres_group_composites_device(photo, [(3, 2, 5, 4), (20, 15, 2, 4), (4, 3, 30, 20)], index, x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="inside"):
        pp.ingest_group_device(photo, [(3, 2, 5, 4), (36, 15, 5, 4), (4, 3, 30, 20)], index, (h, w))
    # `out` overlapping the photographs: one buffer, the photographs in front and the result behind, one byte too early
    n_photo, n_out = photo.numel(), P * L * Hp * Wp * 3
    buf = torch.zeros(n_photo + n_out, dtype=torch.uint8)
    ph = buf[:n_photo].view(P, Hp, Wp, 3)
    with pytest.raises(GcfrError, match="overlap"):
        pp.fullres_group_composites_device(ph, boxes, index, x_lo, rendered, mask, out=buf[n_photo - 1:n_photo - 1 + n_out].view(P, L, Hp, Wp, 3))
    with pytest.raises(GcfrError, match="overlap"):
        pp.fullres_group_composites_device(photo, boxes, index, x_lo, rendered[:, 0], mask, out=photo)
    with pytest.raises(GcfrError, match="no CPU path"):                           # right behind them: allowed
        pp.fullres_group_composites_device(ph, boxes, index, x_lo, rendered, mask, out=buf[n_photo:].view(P, L, Hp, Wp, 3))
    # well-formed host tensors: there is no CPU path.  The indices as a list, an array or a CPU tensor; one box for every face
    for i in (index, np.array(index), np.array(index, dtype=np.uint8), torch.tensor(index), torch.tensor(index, dtype=torch.int16), [0, 0, 0]):
        for b in (boxes, np.array(boxes), torch.tensor(boxes), (3, 2, 5, 4)):
            with pytest.raises(GcfrError, match="no CPU path"):
                pp.fullres_group_composites_device(photo, b, i, x_lo, rendered, mask)
            with pytest.raises(GcfrError, match="no CPU path"):
                pp.ingest_group_device(photo, b, i, (h, w))
    with pytest.raises(GcfrError, match="no CPU path"):                           # None with ONE photograph: every face in it
        pp.fullres_group_composites_device(photo[:1], boxes, None, x_lo, rendered, mask)
    with pytest.raises(GcfrError, match="no CPU path"):
        pp.ingest_group_device(photo[:1], boxes, None, 23)
    for kw in [dict(photo_index=i) for i in bad_index[:1] + bad_index[1:2] + bad_index[4:]] + [dict(boxes=b) for b in bad_boxes] + [
            dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(size=0), dict(size=(5,)), dict(size=(5.0, 7.0)), dict(size=None),
            dict(size=(33, 23)), dict(size=(17, 41))]:
        a = dict(photo_u8=photo, boxes=boxes, photo_index=index, size=(h, w))
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.ingest_group_device(**a)
    # the ingest takes B from the indices: two faces or four need as many boxes
    for i in ([1, 0], [1, 0, 1, 0]):
        with pytest.raises(GcfrError, match="boxes"):
            pp.ingest_group_device(photo, boxes, i, (h, w))


def test_the_inference_entries_exist_and_refuse_malformed_operands():
    import inspect
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd._lib import GcfrError
    names = ("relight_lights_in_group_photograph", "relight_lights_in_group_photograph_device", "relight_rig_in_group_photograph",
             "relight_rig_in_group_photograph_device")
    for name in names:
        sig = inspect.signature(getattr(inf, name))
        assert "upsample" not in sig.parameters and "paste" not in sig.parameters and list(sig.parameters)[1:4] == ["photos_u8", "boxes", "photo_index"]
    mask = np.zeros((17, 23), np.uint8)
    photos = np.zeros((2, 30, 40, 3), np.uint8)
    boxes = [(3, 2, 5, 4), (20, 15, 5, 4), (4, 3, 30, 20)]
    with pytest.raises(GcfrError, match="uint8"):
        inf.relight_lights_in_group_photograph_device(None, photos.astype(np.float32), boxes, [1, 0, 1], mask, None, device="cpu")
    for b, i in ((boxes, [1, 0, 2]), (boxes, [1, 0]), (boxes, None), (boxes, [1.0, 0.0, 1.0]), (boxes[:2], [1, 0, 1]),
                 ([(3, 2, 2, 4)] * 3, [1, 0, 1]), ([(38, 2, 5, 4)] * 3, [1, 0, 1])):
        with pytest.raises(GcfrError):
            inf.relight_lights_in_group_photograph_device(None, photos, b, i, mask, None, device="cpu")
        with pytest.raises(GcfrError):
            inf.relight_rig_in_group_photograph_device(None, photos, b, i, mask, None, None, device="cpu")
        with pytest.raises(GcfrError):
            inf.relight_lights_in_group_photograph(None, photos, b, i, mask, None, device="cpu")
        with pytest.raises(GcfrError):
            inf.relight_rig_in_group_photograph(None, photos, b, i, mask, None, None, device="cpu")
    with pytest.raises(GcfrError, match="mask_u8"):
        inf.relight_lights_in_group_photograph_device(None, photos, boxes, [1, 0, 1], np.zeros((2, 17, 23), np.uint8), None, device="cpu")
    # well-formed: every check passes; a single (Hp,Wp,3) photograph with photo_index=None
    with pytest.raises(GcfrError, match="no CPU path"):
        inf.relight_lights_in_group_photograph_device(None, photos, boxes, [1, 0, 1], mask, None, device="cpu")
    with pytest.raises(GcfrError, match="no CPU path"):
        inf.relight_rig_in_group_photograph_device(None, photos[0], boxes, None, mask, None, None, device="cpu")
