"""CPU: the affine statement (include/gcfr.h; tests/fullres_affine_emulation.py restates it in numpy) and the host side of the affine
entries (postprocess.quantise_affine / affine_from_rotated_box, inference.lights_in_face_frame).

  anchors     for the axis-aligned map of a box at s in {1, 2, 4, 8} the ingest has tests/fullres_box_emulation.py's BITS, and with the
              exact inverse at s in {1, 2, 4} the composite has its BYTES: no tolerance
  rot90       the ingest commutes exactly with np.rot90 of the photograph and the matching integer change of F
  grid_sample against torch's f64 grid_sample (bilinear, align_corners=False, border) on the dequantised matrix, averaged over the K^2
              sub-sample grids, at K = 1, 2, 4, 8: within 2^-25 + 2^-40.  The statement's S / (255 K^2 den^2) is the exact value
              of that mean, rounded once to f32; values lie in [0, 1], where half an ulp of f32 is at most 2^-25; the f64 reference
              carries its own rounding, of the order of 2^-50 per operation over a few hundred operations, which 2^-40 covers
  identity    with rendered == x_lo under a full mask the photograph comes back at every byte where neither floor nor detail_clamp
              acts
  K(M)        at its three thresholds, on both sides of each; the inside test on the network square's edge
  host        quantise_affine's refusals, affine_from_rotated_box at angle 0, the light_frame rotation at 0, 90 and 30 degrees"""
import numpy as np
import pytest
import torch

import fullres_affine_emulation as affine
import fullres_box_emulation as box

ONE = affine.ONE


def _axis_aligned(s, x0, y0):
    return np.array([[s * ONE, 0, x0 * ONE], [0, s * ONE, y0 * ONE]], np.int64)


def _inputs(seed, B, L, h, w, Hp, Wp):
    rng = np.random.default_rng(seed)
    photo = rng.integers(0, 256, (B, Hp, Wp, 3), dtype=np.uint8)
    x_lo = (0.05 + 0.9 * rng.random((B, h, w, 3))).astype(np.float32)
    rendered = (0.5 + 1.5 * rng.standard_normal((B, L, 3, h, w))).astype(np.float32)
    mask = rng.choice(np.array([255, 0, 64, 128], np.uint8), (B, h, w))
    return photo, x_lo, rendered, mask


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_the_ingest_of_an_axis_aligned_map_has_the_box_ingests_bits(s):
    h, w = 5, 7
    Hp, Wp = 8 * h + 3, 8 * w + 5
    photo = np.random.default_rng(s).integers(0, 256, (2, Hp, Wp, 3), dtype=np.uint8)
    origins = [(2, 1), (Wp - s * w, Hp - s * h)]
    F = np.stack([_axis_aligned(s, x0, y0) for x0, y0 in origins])
    assert all(affine.sub_samples(m) == s for m in F)
    got = affine.ingest(photo, F, h, w)
    want = box.ingest(photo, [(x0, y0, s * w, s * h) for x0, y0 in origins], h, w)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("s", [1, 2, 4])
def test_the_composite_of_an_axis_aligned_map_has_the_box_composites_bytes(s):
    from geomconsistentfr_amd import postprocess as pp
    h, w, B, L = 5, 7, 2, 3
    Hp, Wp = 4 * h + 3, 4 * w + 5
    origins = [(2, 1), (Wp - s * w, Hp - s * h)]
    photo, x_lo, rendered, mask = _inputs(10 + s, B, L, h, w, Hp, Wp)
    A = np.stack([_axis_aligned(s, x0, y0) for x0, y0 in origins]).astype(np.float64) / ONE
    F, I = affine.quantise(A)
    for (x0, y0), m in zip(origins, I):                                            # the exact inverse
        np.testing.assert_array_equal(m, np.array([[ONE // s, 0, -x0 * ONE // s], [0, ONE // s, -y0 * ONE // s]]))
        assert (x0 * ONE) % s == 0 and (y0 * ONE) % s == 0 and affine.sub_samples(m) == 1
    Fp, Ip = pp.quantise_affine(A)
    np.testing.assert_array_equal(Fp, F)
    np.testing.assert_array_equal(Ip, I)
    got = affine.composites(photo, I, x_lo, rendered, mask)
    want = box.composites(photo, [(x0, y0, s * w, s * h) for x0, y0 in origins], x_lo, rendered, mask)
    assert (want != photo[:, None]).any()
    np.testing.assert_array_equal(got, want)
    # the taps, t and the clamps coincide with the box's, per axis
    j0, j1, tx = affine.axis_taps(affine.tap_coordinates(I[0], 1, Hp, Wp)[0][0, 0, 0, origins[0][0]:origins[0][0] + s * w], 2 * ONE, w)
    b0, b1, bt = box.taps(s * w, w)
    np.testing.assert_array_equal(j0, b0)
    np.testing.assert_array_equal(j1, b1)
    np.testing.assert_array_equal(tx.view(np.uint32), bt.view(np.uint32))


def _rotated(deg, scale, h, w, cx, cy):
    from geomconsistentfr_amd import postprocess as pp
    return pp.affine_from_rotated_box(cx, cy, scale * w, scale * h, deg, (h, w))


@pytest.mark.parametrize("deg,scale", [(17.0, 2.3), (-40.0, 0.6), (25.0, 5.1), (90.0, 1.0)])
def test_the_ingest_commutes_with_rot90(deg, scale):
    """np.rot90(photo, 1) (counter-clockwise) sends pixel coordinate (X, Y) of a photograph (Hp, Wp) to (Y, Wp - X): the map
    (X', Y') = (Y, Wp - X) composed with F is again an integer matrix"""
    h, w, Hp, Wp = 6, 5, 23, 31
    photo = np.random.default_rng(3).integers(0, 256, (1, Hp, Wp, 3), dtype=np.uint8)
    F, _ = affine.quantise(_rotated(deg, scale, h, w, 14.2, 9.7))
    G = np.array([[F[1, 0], F[1, 1], F[1, 2]], [-F[0, 0], -F[0, 1], Wp * ONE - F[0, 2]]], np.int64)
    assert affine.sub_samples(G) == affine.sub_samples(F) and affine.determinant(G) == affine.determinant(F)
    a = affine.ingest(photo, F, h, w)
    b = affine.ingest(np.ascontiguousarray(np.rot90(photo, 1, axes=(1, 2))), G, h, w)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("K,deg,scale", [(1, 17.0, 0.9), (2, -40.0, 1.7), (4, 25.0, 3.3), (8, 31.0, 5.1)])
def test_the_ingest_is_f64_grid_sample_rounded_once(K, deg, scale):
    h, w, Hp, Wp = 12, 10, 61, 53
    photo = np.random.default_rng(K).integers(0, 256, (1, Hp, Wp, 3), dtype=np.uint8)
    F, _ = affine.quantise(_rotated(deg, scale, h, w, 30.0, 33.0))                 # (at 5.1 the face hangs over the photograph's edges)
    assert affine.sub_samples(F) == K
    got = affine.ingest(photo, F, h, w)[0].astype(np.float64)
    A = F.astype(np.float64) / ONE
    img = torch.from_numpy(photo[0].astype(np.float64) / 255.0).permute(2, 0, 1)[None]
    acc = torch.zeros(3, h, w, dtype=torch.float64)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    for b in range(K):
        for a in range(K):
            u, v = j + (2 * a + 1) / (2.0 * K), i + (2 * b + 1) / (2.0 * K)
            X, Y = A[0, 0] * u + A[0, 1] * v + A[0, 2], A[1, 0] * u + A[1, 1] * v + A[1, 2]
            grid = torch.from_numpy(np.stack([2.0 * X / Wp - 1.0, 2.0 * Y / Hp - 1.0], -1))[None]
            acc += torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)[0]
    want = (acc / (K * K)).permute(1, 2, 0).numpy()
    err = float(np.abs(got - want).max())
    print("K %d: max |statement - f64 grid_sample| = %.4f x 2^-25" % (K, err * 2.0 ** 25))
    assert err <= 2.0 ** -25 + 2.0 ** -40


@pytest.mark.parametrize("deg,scale", [(17.0, 2.3), (90.0, 1.0), (-40.0, 0.6)])
def test_rendered_equal_to_x_lo_under_a_full_mask_returns_the_photograph(deg, scale):
    """v = p + 1 (r d - p) with r = xl and d = p / xl.  Where floor acts (xl < floor) or detail_clamp does (d outside the clamp) the
    product is something else; every other byte inside the face must be the photograph's: counted, and all required"""
    h, w, Hp, Wp = 24, 20, 61, 53
    photo = np.random.default_rng(5).integers(0, 256, (1, Hp, Wp, 3), dtype=np.uint8)
    F, I = affine.quantise(_rotated(deg, scale, h, w, 30.0, 27.0))
    x_lo = affine.ingest(photo, F, h, w)
    mask = np.full((1, h, w), 255, np.uint8)
    got = affine.composites(photo, I, x_lo, np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2))[:, None]), mask)
    _, m, d, ins = affine.face_terms(photo[0], I, x_lo[0], np.transpose(x_lo[0], (2, 0, 1))[None], mask[0])
    xl = np.transpose(affine.carry(np.ascontiguousarray(np.transpose(x_lo[0], (2, 0, 1))), I, Hp, Wp), (1, 2, 0)) * np.float32(255.0)
    free = ins[:, :, None] & (xl >= 1.0) & (d > 0.25) & (d < 4.0)
    assert (m[ins] == 1.0).all() and ins.sum() > 100 and not ins.all()
    same = got[0, 0] == photo[0]
    print("%g degrees, scale %g: %d bytes inside, %d free of floor and clamp, %d of them the photograph's"
          % (deg, scale, 3 * int(ins.sum()), int(free.sum()), int((same & free).sum())))
    assert free.sum() > 0.5 * 3 * ins.sum()
    assert int((same & free).sum()) == int(free.sum())
    assert same[~ins].all()


def test_sub_samples_at_its_thresholds():
    from geomconsistentfr_amd import postprocess as pp
    for K, nxt in ((1, 2), (2, 4), (4, 8), (8, None)):
        on = np.array([[K * ONE, 0, 0], [0, ONE, 0]], np.int64)                    # a column of exactly K: K sub-samples
        over = np.array([[K * ONE, 0, 0], [1, ONE, 0]], np.int64)                  # one unit of 2^-14 longer: the next K
        for f in (affine.sub_samples, pp.affine_sub_samples):
            assert f(on) == K and f(over) == nxt
            assert f(on[:, [1, 0, 2]]) == K and f(over[:, [1, 0, 2]]) == nxt        # the other column
    # a rotated column: 3^2 + 4^2 = 5^2 exactly
    m = np.array([[3 * ONE // 5 * 2, -ONE, 0], [4 * ONE // 5 * 2, ONE, 0]], np.int64)
    assert affine.sub_samples(m) == 2 and m[0, 0] ** 2 + m[1, 0] ** 2 <= (2 * ONE) ** 2


def test_a_centre_on_the_squares_edge():
    """c0 == 0 is inside, c0 == 2 ONE w is outside: the half-open square [0, w) x [0, h)"""
    h, w, Hp, Wp = 3, 4, 6, 9
    # X - 1/2 = u: pixel x has c0 = ONE (2x + 1) - ONE = 2 ONE x, so x = 0 lands on u = 0 and x = w on u = w
    I = np.array([[ONE, 0, -ONE // 2], [0, ONE, -ONE // 2]], np.int64)
    ins = affine.inside(I, Hp, Wp, h, w)
    want = np.zeros((Hp, Wp), bool)
    want[0:h, 0:w] = True
    np.testing.assert_array_equal(ins, want)
    one_less = I.copy()
    one_less[0, 2] -= 1                                                            # c0 = 2 ONE x - 2: column 0 falls out, column w comes in
    ins = affine.inside(one_less, Hp, Wp, h, w)
    want = np.zeros((Hp, Wp), bool)
    want[0:h, 1:w + 1] = True
    np.testing.assert_array_equal(ins, want)
    # and the composite follows the test: under a full mask exactly those pixels may change
    photo, x_lo, rendered, mask = _inputs(8, 1, 2, h, w, Hp, Wp)
    mask[:] = 255
    out = affine.composites(photo, one_less, x_lo, rendered, mask)
    changed = (out != photo[:, None]).any(axis=(0, 1, 4))
    assert changed.any() and not changed[~want].any()


def test_quantise_affine_refuses_what_the_entries_cannot_take():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    good = np.array([[1.5, -0.5, 10.0], [0.5, 1.5, 20.0]])
    F, I = pp.quantise_affine(good)
    assert F.dtype == np.int64 and I.dtype == np.int64 and F.shape == (2, 3) and I.shape == (2, 3)
    Fe, Ie = affine.quantise(good)
    np.testing.assert_array_equal(F, Fe)
    np.testing.assert_array_equal(I, Ie)
    Fb, Ib = pp.quantise_affine(np.stack([good, good]))
    assert Fb.shape == (2, 2, 3) and (Fb == F).all() and (Ib == I).all()
    # F I is the identity up to the quantisation of I
    prod = (F[:, :2].astype(np.float64) / ONE) @ (I[:, :2].astype(np.float64) / ONE)
    assert np.abs(prod - np.eye(2)).max() < 4.0 / ONE
    bad = good.copy()
    bad[0, 1] = np.nan
    with pytest.raises(GcfrError, match="finite"):
        pp.quantise_affine(bad)
    bad[0, 1] = np.inf
    with pytest.raises(GcfrError, match="finite"):
        pp.quantise_affine(bad)
    with pytest.raises(GcfrError, match="determinant"):
        pp.quantise_affine(good * np.array([[1.0], [-1.0]]))                       # a mirror image
    with pytest.raises(GcfrError, match="determinant"):
        pp.quantise_affine(np.array([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]]))           # singular
    with pytest.raises(GcfrError, match="column"):
        pp.quantise_affine(np.array([[8.0, 0.0, 0.0], [0.01, 8.0, 0.0]]))          # F's column longer than 8
    with pytest.raises(GcfrError, match="column"):
        pp.quantise_affine(np.array([[0.12, 0.0, 0.0], [0.0, 0.12, 0.0]]))         # I's column longer than 8
    pp.quantise_affine(np.array([[8.0, 0.0, 0.0], [0.0, 0.125, 0.0]]))             # both exactly at 8
    with pytest.raises(GcfrError, match=r"\(2,3\)"):
        pp.quantise_affine(np.eye(3))
    with pytest.raises(GcfrError, match="2\\^2[67]"):
        pp.quantise_affine(np.array([[1.0, 0.0, 2.0 ** 26 + 1.0], [0.0, 1.0, 0.0]]))


def test_affine_from_rotated_box_at_angle_zero_is_the_boxes_map():
    from geomconsistentfr_amd import postprocess as pp
    h, w = 5, 7
    for (x0, y0, bw, bh) in ((2, 1, 14, 10), (0, 3, 7, 20), (4, 4, 28, 5)):
        A = pp.affine_from_rotated_box(x0 + bw / 2.0, y0 + bh / 2.0, bw, bh, 0.0, (h, w))
        np.testing.assert_array_equal(A, np.array([[bw / w, 0.0, x0], [0.0, bh / h, y0]]))
    # a quarter turn is exact, and the network's centre lands on (cx, cy) at any angle
    A = pp.affine_from_rotated_box(20.0, 30.0, 14, 10, 90.0, (h, w))
    np.testing.assert_array_equal(A[:, :2], np.array([[0.0, -2.0], [2.0, 0.0]]))
    for deg in (0.0, 17.0, 90.0, -40.0, 180.0, 270.0):
        A = pp.affine_from_rotated_box(20.0, 30.0, 14, 10, deg, (h, w))
        np.testing.assert_allclose(A @ np.array([w / 2.0, h / 2.0, 1.0]), [20.0, 30.0], atol=1e-12)
        assert np.linalg.det(A[:, :2]) > 0
    # clockwise as displayed: at +90 degrees the network's +u (right) points down the photograph (+Y)
    A = pp.affine_from_rotated_box(20.0, 30.0, 7, 5, 90.0, (h, w))
    np.testing.assert_array_equal(A[:, :2] @ np.array([1.0, 0.0]), [0.0, 1.0])


@pytest.mark.parametrize("deg,R", [(0.0, [[1.0, 0.0], [0.0, 1.0]]), (90.0, [[0.0, -1.0], [1.0, 0.0]]),
                                   (30.0, [[0.8660254037844387, -0.5], [0.5, 0.8660254037844387]])])
def test_lights_in_face_frame_against_a_hand_written_rotation(deg, R):
    """a face turned clockwise by `deg` in the photograph (y down) sees a light of the photograph's frame (y up) turned
    counter-clockwise by `deg` in its own: at 90 degrees the photograph's left, (-1, 0), is the face's below, (0, -1)"""
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    _, I = pp.quantise_affine(pp.affine_from_rotated_box(40.0, 50.0, 46, 46, deg, 20))
    lights = np.array([(-1.0, 0.0, 0.5), (0.0, 1.0, 0.25), (0.6, -0.3, 0.7)], np.float32)
    got = inf.lights_in_face_frame(lights, I, 2)
    assert tuple(got.shape) == (2, 3, 3) and got.dtype == torch.float32
    want = np.concatenate([lights[:, :2] @ np.array(R, np.float64).T, lights[:, 2:]], axis=1)
    np.testing.assert_allclose(got[0].numpy(), want, atol=2e-4)                    # (I is quantised to 2^-14)
    np.testing.assert_array_equal(got[0].numpy(), got[1].numpy())
    np.testing.assert_array_equal(got[..., 2].numpy(), np.broadcast_to(lights[:, 2], (2, 3)))
    if deg == 90.0:
        np.testing.assert_array_equal(got[0, 0].numpy(), np.array([0.0, -1.0, 0.5], np.float32))
    # per-face lights and per-face maps
    _, I2 = pp.quantise_affine(np.stack([pp.affine_from_rotated_box(40.0, 50.0, 46, 46, d, 20) for d in (deg, 0.0)]))
    both = inf.lights_in_face_frame(np.stack([lights, lights]), I2, 2)
    np.testing.assert_array_equal(both[0].numpy(), got[0].numpy())
    np.testing.assert_array_equal(both[1].numpy(), lights)


def test_the_c_entries_refuse_before_any_launch():
    """argument validation happens on the host, so it runs without a GPU: dummy non-null pointers, then one bad argument at a time"""
    import ctypes
    from geomconsistentfr_amd import _lib
    lib = _lib.load()
    d, o = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    host = lambda a: np.ascontiguousarray(a, np.int64).ctypes.data_as(ctypes.c_void_p)
    good = np.array([[[2 * ONE, -ONE, 5 * ONE], [ONE, 2 * ONE, 7 * ONE]]], np.int64)

    def ingest(M=good, photo=d, x=o, B=1, Hp=40, Wp=30, h=8, w=6):
        return lib.gcfr_ingest_affine_u8(photo, B, Hp, Wp, None if M is None else host(M), h, w, x, None)

    def composite(M=good, photo=d, out=o, B=1, L=2, mask_batch=1, Hp=40, Wp=30, h=8, w=6, floor=1.0, clamp=4.0):
        return lib.gcfr_fullres_composites_affine_u8(photo, d, d, d, mask_batch, B, L, Hp, Wp, None if M is None else host(M), h, w, floor,
                                                     clamp, out, None)

    def changed(i, j, v):
        m = good.copy()
        m[0, i, j] = v
        return m

    for call in (ingest, composite):
        assert call(M=None) == -1 and call(photo=None) == -1 and call(B=0) == -1 and call(h=0) == -1 and call(Wp=0) == -1
        assert call(M=good * np.array([[1], [-1]])) == -1                          # a mirror image
        assert call(M=changed(1, 1, -ONE // 2)) == -1                              # det = 0
        assert call(M=changed(0, 0, 8 * ONE)) == -1                                # a column longer than 8
        assert call(M=changed(0, 2, (1 << 40) + 1)) == -1 and call(M=changed(1, 2, -(1 << 40) - 1)) == -1
        assert call(Hp=1 << 16, Wp=1 << 15) == -1                                  # Hp Wp = 2^31
    assert ingest(x=None) == -1 and ingest(x=d) == -1
    assert composite(out=None) == -1 and composite(out=d) == -1                    # out overlapping the photograph
    assert composite(out=ctypes.c_void_p((1 << 20) + 3 * 40 * 30 - 1)) == -1
    assert composite(L=0) == -1 and composite(L=4097) == -1 and composite(mask_batch=2) == -1
    assert composite(clamp=0.5) == -1 and composite(floor=0.0) == -1
