"""The affine kernels' contract (csrc/gcfr_fullres_affine.hip, include/gcfr.h), stated in numpy (helper module, no tests): the ingest of
a face through a 2 x 3 map network -> photograph, the carrier that takes a plane at the network's resolution through the map
photograph -> network onto the photograph's pixels, and the quotient / detail-transfer composite.  All geometry is integer, fixed
point with 14 fractional bits; every numpy operation on f32 arrays below is one separately rounded IEEE f32 operation, as the
library's are under -ffp-contract=off.  It shares no code with the kernels, and none with the other restatements but the byte
quantisation.

Arrays in the C ABI's layouts: photo (B,Hp,Wp,3) u8, F / I (B,2,3) int64 in units of 2^-14, x_lo (B,h,w,3) f32, rendered (B,L,3,h,w)
f32, mask (MB,h,w) u8 with MB in {1, B} in the network's frame; -> (B,L,Hp,Wp,3) u8."""
import numpy as np

from fullres_emulation import quantise_u8

ONE = 1 << 14
F32 = np.float32


def as_maps(M, B):
    m = np.asarray(M)
    assert m.dtype == np.int64 and m.shape in ((2, 3), (B, 2, 3)), (m.dtype, m.shape)
    return np.broadcast_to(m, (B, 2, 3))


def quantise(A):
    """(2,3) | (B,2,3) f64 network -> photograph -> (F, I) int64: F = rint(A 2^14); I = rint(inverse(F / 2^14) 2^14), the inverse
    written out in f64: det = a d - b c, the linear part (d, -b; -c, a) / det, the translation -(linear part) t"""
    A = np.asarray(A, np.float64)
    Fq = np.rint(A * ONE).astype(np.int64)
    f = Fq.astype(np.float64) / ONE
    a, b, tx, c, d, ty = (f[..., 0, 0], f[..., 0, 1], f[..., 0, 2], f[..., 1, 0], f[..., 1, 1], f[..., 1, 2])
    det = a * d - b * c
    i00, i01, i10, i11 = d / det, -b / det, -c / det, a / det
    inv = np.stack([np.stack([i00, i01, -(i00 * tx + i01 * ty)], -1), np.stack([i10, i11, -(i10 * tx + i11 * ty)], -1)], -2)
    return Fq, np.rint(inv * ONE).astype(np.int64)


def sub_samples(M):
    """K(M): the smallest of 1, 2, 4, 8 with K^2 ONE^2 >= the longer column's squared length, in exact integers; None above 8"""
    m = [[int(v) for v in row] for row in np.asarray(M)]
    n2 = max(m[0][0] ** 2 + m[1][0] ** 2, m[0][1] ** 2 + m[1][1] ** 2)
    for K in (1, 2, 4, 8):
        if K * K * ONE * ONE >= n2:
            return K
    return None


def determinant(M):
    m = [[int(v) for v in row] for row in np.asarray(M)]
    return m[0][0] * m[1][1] - m[0][1] * m[1][0]


def tap_coordinates(M, K, rows, cols):
    """-> P0, P1 (K, K, rows, cols) int64, indexed [b, a, y, x]: the source tap coordinate of sub-sample (a, b) of destination pixel
    (x, y), in units of 1 / (2 K ONE), already shifted by the half pixel"""
    m = np.asarray(M, np.int64)
    b, a, y, x = np.meshgrid(np.arange(K, dtype=np.int64), np.arange(K, dtype=np.int64), np.arange(rows, dtype=np.int64),
                             np.arange(cols, dtype=np.int64), indexing="ij")
    ex, ey = 2 * K * x + 2 * a + 1, 2 * K * y + 2 * b + 1
    return [m[r, 0] * ex + m[r, 1] * ey + 2 * K * m[r, 2] - K * ONE for r in (0, 1)]


def ingest_face(photo_u8, Fm, h, w):
    """one face: (Hp,Wp,3) u8 -> (S (h,w,3) int64, K)"""
    Hp, Wp, _ = photo_u8.shape
    K = sub_samples(Fm)
    assert K is not None and determinant(Fm) > 0
    den = 2 * K * ONE
    P0, P1 = tap_coordinates(Fm, K, h, w)
    x0, y0 = P0 // den, P1 // den                                                  # (floor)
    fx, fy = P0 - x0 * den, P1 - y0 * den
    ph = photo_u8.astype(np.int64)
    S = np.zeros((h, w, 3), np.int64)
    for dy, wy in ((0, den - fy), (1, fy)):
        yy = np.clip(y0 + dy, 0, Hp - 1)
        for dx, wx in ((0, den - fx), (1, fx)):
            xx = np.clip(x0 + dx, 0, Wp - 1)
            S += ((wy * wx)[..., None] * ph[yy, xx]).sum(axis=(0, 1))
    return S, K


def ingest(photo_u8, F, h, w):
    """-> (B,h,w,3) f32: the integer sum over the K^2 sub-samples' four taps, one f64 division, one rounding to f32"""
    assert photo_u8.dtype == np.uint8
    B = photo_u8.shape[0]
    out = np.empty((B, h, w, 3), np.float32)
    for b, Fm in enumerate(as_maps(F, B)):
        S, K = ingest_face(photo_u8[b], Fm, h, w)
        assert int(S.max()) < 1 << 53
        den = np.float64(2 * K * ONE)
        out[b] = (S.astype(np.float64) / (255.0 * K * K * den * den)).astype(np.float32)
    return out


def inside(Im, Hp, Wp, h, w):
    """(Hp,Wp) bool: the photograph pixels whose centre lands in the network square"""
    m = np.asarray(Im, np.int64)
    y, x = np.meshgrid(np.arange(Hp, dtype=np.int64), np.arange(Wp, dtype=np.int64), indexing="ij")
    c0 = m[0, 0] * (2 * x + 1) + m[0, 1] * (2 * y + 1) + 2 * m[0, 2]
    c1 = m[1, 0] * (2 * x + 1) + m[1, 1] * (2 * y + 1) + 2 * m[1, 2]
    return (c0 >= 0) & (c0 < 2 * ONE * w) & (c1 >= 0) & (c1 < 2 * ONE * h)


def axis_taps(P, den, n):
    U = np.maximum(P, 0)
    q = U // den
    i0 = np.minimum(q, n - 1)
    fu = U - q * den
    t = (fu.astype(np.float64) / np.float64(den)).astype(np.float32)
    return i0, np.minimum(i0 + 1, n - 1), t


def carry(a, Im, Hp, Wp):
    """the carrier: a (..., h, w) f32 -> (..., Hp, Wp) f32, at EVERY photograph pixel (the taps are clamped into the network)"""
    a = np.asarray(a)
    assert a.dtype == np.float32
    h, w = a.shape[-2:]
    K = sub_samples(Im)
    assert K is not None and determinant(Im) > 0
    den = 2 * K * ONE
    P0, P1 = tap_coordinates(Im, K, Hp, Wp)
    j0, j1, tx = axis_taps(P0, den, w)
    i0, i1, ty = axis_taps(P1, den, h)
    with np.errstate(invalid="ignore", over="ignore"):
        a00, a01, a10, a11 = a[..., i0, j0], a[..., i0, j1], a[..., i1, j0], a[..., i1, j1]       # (..., K, K, Hp, Wp)
        top = a00 + tx * (a01 - a00)
        bot = a10 + tx * (a11 - a10)
        v = top + ty * (bot - top)
        assert v.dtype == np.float32
        if K == 1:
            return v[..., 0, 0, :, :]
        acc = np.zeros(v.shape[:-4] + (Hp, Wp), np.float64)
        for b in range(K):
            for s in range(K):
                acc = acc + v[..., b, s, :, :].astype(np.float64)
        return (acc / np.float64(K * K)).astype(np.float32)


def face_terms(photo_u8, Im, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0):
    """one face: photo (Hp,Wp,3) u8, x_lo (h,w,3), rendered (L,3,h,w), mask (h,w) u8 -> v (L,Hp,Wp,3) f32 before the quantisation,
    m (Hp,Wp) f32, d (Hp,Wp,3) f32 and the inside test (Hp,Wp) bool"""
    Hp, Wp, _ = photo_u8.shape
    h, w = mask_u8.shape
    p = photo_u8.astype(np.float32)
    xl = np.transpose(carry(np.ascontiguousarray(np.transpose(x_lo, (2, 0, 1))), Im, Hp, Wp), (1, 2, 0)) * F32(255.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.fmin(np.fmax(p / np.fmax(xl, F32(floor)), F32(1.0) / F32(detail_clamp)), F32(detail_clamp))
    m = carry(mask_u8.astype(np.float32) / F32(255.0), Im, Hp, Wp)
    r = np.transpose(carry(rendered, Im, Hp, Wp), (0, 2, 3, 1)) * F32(255.0)        # (L,Hp,Wp,3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = p[None] + m[None, :, :, None] * (r * d[None] - p[None])
    assert v.dtype == np.float32 and d.dtype == np.float32 and m.dtype == np.float32
    return v, m, d, inside(Im, Hp, Wp, h, w)


def composites(photo_u8, I, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0):
    """-> (B,L,Hp,Wp,3) u8: the photograph relit where a pixel's centre lands in the network square and the carried mask is positive"""
    B, Hp, Wp, _ = photo_u8.shape
    L = rendered.shape[1]
    h, w = x_lo.shape[1:3]
    assert x_lo.shape == (B, h, w, 3) and x_lo.dtype == np.float32
    assert rendered.shape == (B, L, 3, h, w) and rendered.dtype == np.float32
    assert mask_u8.shape in ((1, h, w), (B, h, w)) and mask_u8.dtype == np.uint8
    out = np.repeat(photo_u8[:, None], L, axis=1)
    for b, Im in enumerate(as_maps(I, B)):
        v, m, _, ins = face_terms(photo_u8[b], Im, x_lo[b], rendered[b], mask_u8[b if mask_u8.shape[0] > 1 else 0], detail_clamp, floor)
        relit = ((m > 0) & ins)[None, :, :, None]
        out[b] = np.where(relit, quantise_u8(v), photo_u8[b][None])
    return out
