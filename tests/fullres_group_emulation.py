"""The group-photograph kernels' contract (csrc/gcfr_fullres_group.hip, include/gcfr.h), stated in numpy (helper module, no tests):
B faces spread over P photographs, face b in photograph photo_index[b].  The ingest is tests/fullres_anybox_emulation.py's of box b
of that photograph; the composite is, per photograph and light, the CHAIN of that module's one-face composite (`box_bytes`) over
the photograph's faces in ascending face index on a running copy of the photograph: a face reads the running bytes where the
one-face composite reads the photograph's, and every step ends in bytes.  It shares no code with the kernels.

Arrays in the C ABI's layouts: photo (P,Hp,Wp,3) u8, boxes (B,4) integers (x0, y0, bw, bh), photo_index (B,) integers, x_lo
(B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (MB,h,w) u8 with MB in {1, B} in the box's frame; -> (P,L,Hp,Wp,3) u8."""
import numpy as np

from fullres_anybox_emulation import box_allowed, box_bytes, box_rows, carry, ingest_crop


def ingest(photo_u8, boxes, photo_index, h, w):
    """-> (B,h,w,3) f32"""
    assert photo_u8.dtype == np.uint8
    P, Hp, Wp, _ = photo_u8.shape
    pi = np.asarray(photo_index, dtype=np.int64)
    B = len(pi)
    out = np.empty((B, h, w, 3), np.float32)
    for b, (x0, y0, bw, bh) in enumerate(box_rows(boxes, B).tolist()):
        assert box_allowed(x0, y0, bw, bh, Hp, Wp, h, w) and 0 <= pi[b] < P
        out[b] = ingest_crop(photo_u8[pi[b], y0:y0 + bh, x0:x0 + bw], h, w)
    return out


def composites(photo_u8, boxes, photo_index, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, order=None):
    """-> (P,L,Hp,Wp,3) u8.  `order`: the faces in another order than ascending b (the tests' question whether order matters)"""
    P, Hp, Wp, _ = photo_u8.shape
    B, L = rendered.shape[:2]
    h, w = x_lo.shape[1:3]
    pi = np.asarray(photo_index, dtype=np.int64)
    rows = box_rows(boxes, B).tolist()
    assert pi.shape == (B,) and x_lo.shape == (B, h, w, 3) and x_lo.dtype == np.float32
    assert rendered.shape == (B, L, 3, h, w) and rendered.dtype == np.float32
    assert mask_u8.shape in ((1, h, w), (B, h, w)) and mask_u8.dtype == np.uint8
    out = np.stack([photo_u8] * L, axis=1)                                         # the running images
    for b in (range(B) if order is None else order):
        x0, y0, bw, bh = rows[b]
        assert box_allowed(x0, y0, bw, bh, Hp, Wp, h, w) and 0 <= pi[b] < P
        mk = mask_u8[b] if mask_u8.shape[0] > 1 else mask_u8[0]
        for l in range(L):
            crop = out[pi[b], l, y0:y0 + bh, x0:x0 + bw].copy()
            out[pi[b], l, y0:y0 + bh, x0:x0 + bw] = box_bytes(crop, x_lo[b], rendered[b, l:l + 1], mk, detail_clamp, floor)[0]
    return out


def relit_counts(boxes, photo_index, mask_u8, P, Hp, Wp, h, w):
    """-> (P,Hp,Wp) integers: by how many faces a pixel is relit (inside the face's box with its carried mask positive)"""
    pi = np.asarray(photo_index, dtype=np.int64)
    n = np.zeros((P, Hp, Wp), np.int64)
    for b, (x0, y0, bw, bh) in enumerate(box_rows(boxes, len(pi)).tolist()):
        mk = mask_u8[b] if mask_u8.shape[0] > 1 else mask_u8[0]
        n[pi[b], y0:y0 + bh, x0:x0 + bw] += carry(mk.astype(np.float32) / np.float32(255.0), bh, bw) > 0
    return n
