"""The group-affine kernels' contract (csrc/gcfr_fullres_group_affine.hip, include/gcfr.h), stated in numpy (helper module, no tests):
B tilted faces spread over P photographs, face b in photograph photo_index[b] under its own pair of integer maps F[b], I[b].  The
ingest is tests/fullres_affine_emulation.py's of that photograph through F[b]; the composite is, per photograph, the CHAIN of that
module's one-face `composites` over the photograph's faces in ascending face index on running copies of the photograph, one per
light: a face reads the running bytes where the one-face composite reads the photograph's, and every step ends in bytes.  It shares
no code with the kernels.

Arrays in the C ABI's layouts: photo (P,Hp,Wp,3) u8, F / I (B,2,3) int64 in units of 2^-14, photo_index (B,) integers, x_lo
(B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (MB,h,w) u8 with MB in {1, B} in the network's frame; -> (P,L,Hp,Wp,3) u8."""
import numpy as np

import fullres_affine_emulation as affine


def ingest(photo_u8, F, photo_index, h, w):
    """-> (B,h,w,3) f32"""
    assert photo_u8.dtype == np.uint8
    pi = np.asarray(photo_index, dtype=np.int64)
    assert pi.ndim == 1 and (pi >= 0).all() and (pi < photo_u8.shape[0]).all()
    return affine.ingest(photo_u8[pi], affine.as_maps(F, len(pi)), h, w)


def composites(photo_u8, I, photo_index, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, order=None):
    """-> (P,L,Hp,Wp,3) u8.  `order`: the faces in another order than ascending b (the tests' question whether order matters)"""
    P, Hp, Wp, _ = photo_u8.shape
    B, L = rendered.shape[:2]
    h, w = x_lo.shape[1:3]
    pi = np.asarray(photo_index, dtype=np.int64)
    maps = affine.as_maps(I, B)
    assert pi.shape == (B,) and (pi >= 0).all() and (pi < P).all()
    assert x_lo.shape == (B, h, w, 3) and x_lo.dtype == np.float32
    assert rendered.shape == (B, L, 3, h, w) and rendered.dtype == np.float32
    assert mask_u8.shape in ((1, h, w), (B, h, w)) and mask_u8.dtype == np.uint8
    out = np.stack([photo_u8] * L, axis=1)                                         # the running images
    for b in (range(B) if order is None else order):
        mk = mask_u8[b] if mask_u8.shape[0] > 1 else mask_u8[0]
        # the one-face composite with the L running images as its photographs and the lights as its batch
        step = affine.composites(out[pi[b]], maps[b], np.broadcast_to(x_lo[b], (L, h, w, 3)), rendered[b][:, None], mk[None],
                                 detail_clamp, floor)
        out[pi[b]] = step[:, 0]
    return out


def relit_counts(I, photo_index, mask_u8, P, Hp, Wp, h, w):
    """-> (P,Hp,Wp) integers: by how many faces a pixel is relit (inside the face's quad with its carried mask positive)"""
    pi = np.asarray(photo_index, dtype=np.int64)
    n = np.zeros((P, Hp, Wp), np.int64)
    for b, Im in enumerate(affine.as_maps(I, len(pi))):
        mk = mask_u8[b] if mask_u8.shape[0] > 1 else mask_u8[0]
        n[pi[b]] += (affine.carry(mk.astype(np.float32) / np.float32(255.0), Im, Hp, Wp) > 0) & affine.inside(Im, Hp, Wp, h, w)
    return n
