"""The cases of the group-affine tests (helper module, no tests): the geometry and the inputs that tests/test_gpu_fullres_group_affine.py
runs on the device and that tests/test_fullres_group_affine_host.py shows, on the CPU alone, to bite.  Everything is built from the
numpy restatements (tests/fullres_affine_emulation.py, tests/fullres_group_affine_emulation.py); nothing here touches a device.

  network   (h, w) = (24, 20); photographs (Hp, Wp) = (61, 53), the scalar path, and (64, 48), the vector path
  faces     per photograph three tilted faces, in a different order in each photograph:
              17 degrees at scale 2.3 at the photograph's centre (Wp / 2, Hp / 2)
              -40 degrees at scale 0.6 at (Wp / 2 + 4, Hp / 2 + 3): K = 2 on the way out
              exactly 90 degrees at scale 1 at (Wp / 2 - 6, Hp / 2 + 8)
            764 pixels of the 61 x 53 photograph and 668 of the 64 x 48 one lie in no quad
  calls     photo_index [0, 0, 0]; an unordered nine over P = 3; six over P = 3 with photograph 1 empty
  masks     the grey levels {0, 64, 128, 255} with the left third of the columns zero, shared or per face
  seam      34 small quads in ONE photograph on a network of (4, 8): stride-2 centres, mixed angles, 4 x 3 and 1.6 x 1 pixels (K = 2
            and K = 8 on the way out); faces 32 and 33 arrive in a continuation launch; another photograph with a single face
            shares the call
  upright   axis-aligned maps with integer origins at 1, 2 and 4 times a network of (5, 7), overlapping each other"""
import functools

import numpy as np

import fullres_affine_emulation as affine
import fullres_group_affine_emulation as tilted

H, W = 24, 20
LEVELS = np.array([255, 0, 64, 128], np.uint8)
SIZES = {True: (64, 48), False: (61, 53)}                  # aligned (the vector path) or not
NO_QUAD = {True: 668, False: 764}
INDICES = {"one": [0, 0, 0], "three": [2, 0, 2, 1, 0, 2, 1, 0, 1], "gap": [2, 0, 2, 0, 2, 0]}
N_PHOTOS = {"one": 1, "three": 3, "gap": 3}
KINDS = ((17.0, 2.3, 0.0, 0.0), (-40.0, 0.6, 4.0, 3.0), (90.0, 1.0, -6.0, 8.0))     # (angle, scale, dx, dy) from the centre


def rotated_box(cx, cy, bw, bh, angle_degrees, h, w):
    """the map network -> photograph (2,3) f64 of a box of bw x bh photograph pixels centred at (cx, cy), turned clockwise as
    displayed about its centre; whole quarter turns have exact sines"""
    quarter = angle_degrees / 90.0
    if quarter == np.floor(quarter):
        co, si = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter) % 4]
    else:
        co, si = float(np.cos(np.radians(angle_degrees))), float(np.sin(np.radians(angle_degrees)))
    sx, sy = bw / w, bh / h
    A = np.array([[co * sx, -si * sy, 0.0], [si * sx, co * sy, 0.0]], np.float64)
    A[:, 2] = np.array([cx, cy]) - A[:, :2] @ np.array([w / 2.0, h / 2.0])
    return A


def kinds_of(pidx):
    """the kind of every face: the k-th face of photograph q is of kind (k + q) % 3"""
    seen, kinds = {}, []
    for q in pidx:
        k = seen.get(q, 0)
        seen[q] = k + 1
        kinds.append((k + q) % 3)
    return kinds


def maps(pidx, Hp, Wp, h=H, w=W):
    """-> (A (B,2,3) f64, F, I (B,2,3) int64)"""
    A = np.stack([rotated_box(Wp / 2 + dx, Hp / 2 + dy, s * w, s * h, ang, h, w) for ang, s, dx, dy in (KINDS[k] for k in kinds_of(pidx))])
    F, I = affine.quantise(A)
    return A, F, I


def masks(rng, MB, h, w):
    """the four grey levels in random order, the left third of the columns zero"""
    mask = np.stack([rng.permutation(m) for m in np.resize(LEVELS, MB * h * w).reshape(MB, h * w)]).reshape(MB, h, w)
    mask[:, :, :w // 3] = 0
    assert set(np.unique(mask)) == set(LEVELS.tolist())
    return mask


def inputs(seed, P, L, h, w, Hp, Wp, F, pidx, shared, zero_left=True):
    """photo (P,Hp,Wp,3) u8, x_lo (B,h,w,3) f32 scaled away from the photograph's means, rendered (B,L,3,h,w) f32 well outside
    [0, 1], mask (1|B,h,w) u8"""
    rng = np.random.default_rng(seed)
    B = len(pidx)
    photo = rng.integers(0, 256, (P, Hp, Wp, 3), dtype=np.uint8)
    x_lo = (tilted.ingest(photo, F, pidx, h, w) * (0.1 + 1.9 * rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 1.5 * rng.standard_normal((B, L, 3, h, w))).astype(np.float32)
    MB = 1 if shared else B
    if zero_left:
        mask = masks(rng, MB, h, w)
    else:
        mask = np.stack([rng.permutation(m) for m in np.resize(LEVELS, MB * h * w).reshape(MB, h * w)]).reshape(MB, h, w)
    return photo, x_lo, rendered, mask


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(aligned, which, L, shared):
    """-> (arrays, (F, I), pidx, want): the inputs of a case and the restatement's bytes, computed once and shared (read only)"""
    Hp, Wp = SIZES[aligned]
    pidx = INDICES[which]
    _, F, I = maps(pidx, Hp, Wp)
    arrays = inputs(11 + L + 2 * aligned + 4 * shared + len(pidx), N_PHOTOS[which], L, H, W, Hp, Wp, F, pidx, shared)
    want = tilted.composites(arrays[0], I, pidx, *arrays[1:])
    _freeze(F, I, want, *arrays)
    return arrays, (F, I), pidx, want


SEAM_NET = (4, 8)


@functools.lru_cache(maxsize=None)
def seam_case(aligned, L, shared):
    """34 faces in photograph 1 with centres on a stride-2 grid, six to a row, every fifth 1.6 x 1 pixels and the others 4 x 3, at
    mixed angles (every fourth a whole quarter turn); face 10 of the call is the one face of photograph 0.
    -> (arrays, (F, I), pidx, want)"""
    h, w = SEAM_NET
    Hp, Wp = 14, 16 if aligned else 15
    rows, pidx = [], []
    for f in range(34):
        bw, bh = (1.6, 1.0) if f % 5 == 4 else (4.0, 3.0)
        angle = 90.0 * (f // 4) if f % 4 == 0 else float((37 * f) % 360)
        rows.append(rotated_box(2 * (f % 6) + 1.5, 2 * (f // 6) + 1.5, bw, bh, angle, h, w))
        pidx.append(1)
    rows.insert(10, rotated_box(Wp / 2, Hp / 2, 9.0, 7.0, 25.0, h, w))
    pidx.insert(10, 0)
    F, I = affine.quantise(np.stack(rows))
    for m in list(F) + list(I):
        assert affine.sub_samples(m) is not None and affine.determinant(m) > 0     # no column longer than 8 after the quantisation
    assert {affine.sub_samples(m) for m in I} >= {1, 2, 8}
    arrays = inputs(34 + L + aligned, 2, L, h, w, Hp, Wp, F, pidx, shared, zero_left=False)
    want = tilted.composites(arrays[0], I, pidx, *arrays[1:])
    _freeze(F, I, want, *arrays)
    return arrays, (F, I), tuple(pidx), want


UPRIGHT_NET = (5, 7)


def upright_case(aligned, L=3, shared=False):
    """axis-aligned maps with integer origins at s = 4, 2, 1, 2 times the network's side, overlapping, over two photographs
    -> (arrays, (F, I), boxes (B,4), pidx)"""
    h, w = UPRIGHT_NET
    Hp, Wp = 30, 40 if aligned else 41
    spec = [(4, 3, 2, 0), (2, 9, 7, 0), (1, 12, 9, 0), (2, 20, 15, 0), (4, 10, 8, 1), (1, 11, 9, 1), (2, 5, 3, 1)]   # (s, x0, y0, q)
    pidx = [q for *_, q in spec]
    boxes = np.array([(x0, y0, s * w, s * h) for s, x0, y0, _ in spec])
    A = np.array([[[s, 0, x0], [0, s, y0]] for s, x0, y0, _ in spec], np.float64)
    F, I = affine.quantise(A)
    for (s, x0, y0, _), Fm, Im in zip(spec, F, I):                                 # I is the exact inverse
        assert Fm.tolist() == [[s * affine.ONE, 0, x0 * affine.ONE], [0, s * affine.ONE, y0 * affine.ONE]]
        assert Im.tolist() == [[affine.ONE // s, 0, -x0 * affine.ONE // s], [0, affine.ONE // s, -y0 * affine.ONE // s]]
        assert (x0 * affine.ONE) % s == 0 and (y0 * affine.ONE) % s == 0
    arrays = inputs(55 + aligned, 2, L, h, w, Hp, Wp, F, pidx, shared)
    return arrays, (F, I), boxes, pidx
