"""The any-size box kernels' contract (csrc/gcfr_fullres_anybox.hip, include/gcfr.h), stated in numpy (helper module, no tests): the
ingest of a face box that may be SMALLER than the network's input on either axis, the per-axis carrying operator (a lerp where the
box axis is at least the network's, an exact-footprint area mean where it is shorter) and the quotient / detail-transfer
composite.  Every numpy operation on f32 arrays below is one separately rounded IEEE f32 operation and every one on f64 arrays one
f64 operation, as the library's are under -ffp-contract=off.  It shares no code with the kernels and none with
tests/fullres_box_emulation.py or tests/fullres_emulation.py: the tests compare against those.

Arrays in the C ABI's layouts: photo (B,Hp,Wp,3) u8, boxes (B,4) integers (x0, y0, bw, bh), x_lo (B,h,w,3) f32, rendered
(B,L,3,h,w) f32, mask (MB,h,w) u8 with MB in {1, B} in the box's frame; -> (B,L,Hp,Wp,3) u8 (paste) or (B,L,bh,bw,3) u8."""
import numpy as np

F32 = np.float32
MAX_TAPS = 9                        # of a minified axis: 8 nb >= n


def box_rows(boxes, B):
    a = np.asarray(boxes, dtype=np.int64)
    return np.tile(a, (B, 1)) if a.ndim == 1 else a


def box_allowed(x0, y0, bw, bh, Hp, Wp, h, w):
    """the box rules of include/gcfr.h for one box"""
    return (x0 >= 0 and y0 >= 0 and bw >= 1 and bh >= 1 and 8 * bw >= w and 8 * bh >= h and x0 + bw <= Wp and y0 + bh <= Hp
            and 2 * bh * h <= 0x7fffffff and 2 * bw * w <= 0x7fffffff)


def ingest_weights(nb, n):
    """one axis of the ingest: the integer weights W (n, nb) of box index y in network index i, and their common row sum D"""
    W = np.zeros((n, nb), np.int64)
    if nb >= n:                                                       # area mean
        for i in range(n):
            for y in range(nb):
                W[i, y] = max(0, min((y + 1) * n, (i + 1) * nb) - max(y * n, i * nb))
        D = nb
    else:                                                             # magnify: two taps, half-pixel centres, in integers
        for i in range(n):
            N = max((2 * i + 1) * nb - n, 0)
            i0 = N // (2 * n)
            rem = N - i0 * 2 * n
            i1 = min(i0 + 1, nb - 1)
            W[i, i0] += 2 * n - rem
            W[i, i1] += rem
        D = 2 * n
    assert (W.sum(axis=1) == D).all()
    return W, D


def ingest_crop(crop_u8, h, w):
    """(bh,bw,3) u8 -> (h,w,3) f32: S as an exact integer, one f64 division, one rounding"""
    bh, bw, _ = crop_u8.shape
    Wy, Dy = ingest_weights(bh, h)
    Wx, Dx = ingest_weights(bw, w)
    S = np.einsum("iy,jx,yxc->ijc", Wy, Wx, crop_u8.astype(np.int64))
    return (S.astype(np.float64) / (255.0 * Dy * Dx)).astype(np.float32)


def ingest(photo_u8, boxes, h, w):
    """-> (B,h,w,3) f32"""
    assert photo_u8.dtype == np.uint8
    B, Hp, Wp, _ = photo_u8.shape
    out = np.empty((B, h, w, 3), np.float32)
    for b, (x0, y0, bw, bh) in enumerate(box_rows(boxes, B).tolist()):
        assert box_allowed(x0, y0, bw, bh, Hp, Wp, h, w)
        out[b] = ingest_crop(photo_u8[b, y0:y0 + bh, x0:x0 + bw], h, w)
    return out


def lerp_taps(nb, n):
    """an axis with nb >= n: per box index the two network taps and the f32 weight of the second"""
    y = np.arange(nb, dtype=np.int64)
    N = np.maximum((2 * y + 1) * n - nb, 0)
    i0 = N // (2 * nb)
    rem = N - i0 * (2 * nb)
    t = (rem.astype(np.float64) / np.float64(2 * nb)).astype(np.float32)
    return i0, np.minimum(i0 + 1, n - 1), t


def area_taps(nb, n):
    """an axis with nb < n: per box index the first and the last network tap"""
    y = np.arange(nb, dtype=np.int64)
    first = (y * n) // nb
    last = -((-(y + 1) * n) // nb) - 1                                 # ceil((y+1) n / nb) - 1
    assert (last - first + 1 <= MAX_TAPS).all() and last[-1] == n - 1 and first[0] == 0
    return first, last


def carry_last_axis(a, nb):
    """the carrying operator along the LAST axis: a (..., n) f32 -> (..., nb) f32"""
    assert a.dtype == np.float32
    n = a.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        if nb >= n:
            i0, i1, t = lerp_taps(nb, n)
            a0, a1 = a[..., i0], a[..., i1]
            out = a0 + t * (a1 - a0)
        else:
            first, last = area_taps(nb, n)
            y = np.arange(nb, dtype=np.int64)
            acc = np.zeros(a.shape[:-1] + (nb,), np.float64)
            for k in range(MAX_TAPS):                                  # ascending i; a tap past `last` is not touched
                i = first + k
                live = i <= last
                ic = np.minimum(i, n - 1)
                wt = np.minimum((ic + 1) * nb, (y + 1) * n) - np.maximum(ic * nb, y * n)
                assert (wt[live] > 0).all()
                term = wt.astype(np.float64) * a[..., ic].astype(np.float64)
                acc = np.where(live, acc + term, acc)
            out = (acc / np.float64(n)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def carry(a, bh, bw):
    """a (..., h, w) f32 -> (..., bh, bw) f32: horizontal first on every row, rounded to f32, then vertical"""
    hz = carry_last_axis(np.ascontiguousarray(a, dtype=np.float32), bw)            # (..., h, bw)
    vt = carry_last_axis(np.ascontiguousarray(np.swapaxes(hz, -1, -2)), bh)        # (..., bw, bh)
    return np.ascontiguousarray(np.swapaxes(vt, -1, -2))


def to_byte(v):
    """f32 -> u8: rint of the f64 value (half to even), saturated, NaN -> 0"""
    r = np.rint(v.astype(np.float64))
    r = np.where(np.isnan(r), 0.0, r)
    return np.minimum(np.maximum(r, 0.0), 255.0).astype(np.uint8)


def box_terms(crop_u8, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0):
    """one face: crop (bh,bw,3) u8, x_lo (h,w,3), rendered (L,3,h,w), mask (h,w) u8 -> v (L,bh,bw,3) f32, m (bh,bw) f32,
    d (bh,bw,3) f32 and xl (bh,bw,3) f32 in grey levels"""
    bh, bw, _ = crop_u8.shape
    p = crop_u8.astype(np.float32)
    xl = np.moveaxis(carry(np.moveaxis(x_lo, 2, 0), bh, bw), 0, 2) * F32(255.0)
    lo, hi = F32(1.0) / F32(detail_clamp), F32(detail_clamp)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.fmin(np.fmax(p / np.fmax(xl, F32(floor)), lo), hi)
        m = carry(mask_u8.astype(np.float32) / F32(255.0), bh, bw)
        r = np.moveaxis(carry(rendered, bh, bw), 1, 3) * F32(255.0)                # (L,bh,bw,3)
        v = p[None] + m[None, :, :, None] * (r * d[None] - p[None])
    assert v.dtype == np.float32 and d.dtype == np.float32 and m.dtype == np.float32
    return v, m, d, xl


def box_bytes(crop_u8, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0):
    """one face -> (L,bh,bw,3) u8"""
    v, m, _, _ = box_terms(crop_u8, x_lo, rendered, mask_u8, detail_clamp, floor)
    return np.where(m[None, :, :, None] > 0, to_byte(v), crop_u8[None])


def composites(photo_u8, boxes, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, paste=True):
    """-> (B,L,Hp,Wp,3) u8, or with paste=False (B,L,bh,bw,3) u8"""
    B, Hp, Wp, _ = photo_u8.shape
    L = rendered.shape[1]
    h, w = x_lo.shape[1:3]
    rows = box_rows(boxes, B).tolist()
    assert x_lo.shape == (B, h, w, 3) and x_lo.dtype == np.float32
    assert rendered.shape == (B, L, 3, h, w) and rendered.dtype == np.float32
    assert mask_u8.shape in ((1, h, w), (B, h, w)) and mask_u8.dtype == np.uint8
    if paste:
        out = np.stack([photo_u8] * L, axis=1)
    else:
        assert all(r[2:] == rows[0][2:] for r in rows)
        out = np.empty((B, L, rows[0][3], rows[0][2], 3), np.uint8)
    for b, (x0, y0, bw, bh) in enumerate(rows):
        assert box_allowed(x0, y0, bw, bh, Hp, Wp, h, w)
        mk = mask_u8[b] if mask_u8.shape[0] > 1 else mask_u8[0]
        relit = box_bytes(photo_u8[b, y0:y0 + bh, x0:x0 + bw], x_lo[b], rendered[b], mk, detail_clamp, floor)
        if paste:
            out[b, :, y0:y0 + bh, x0:x0 + bw] = relit
        else:
            out[b] = relit
    return out
