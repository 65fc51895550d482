"""The full-resolution kernels' contract (csrc/gcfr_fullres.hip, include/gcfr.h), stated in numpy (helper module, no tests): the
ingest, the bilinear upsample Up and the quotient / detail-transfer composite, f32 throughout -- every numpy operation below is one
separately rounded IEEE f32 operation on f32 arrays, as the library's are under -ffp-contract=off.  It shares no code with the
kernels.

Arrays in the C ABI's layouts: photo (B, s h, s w, 3) u8, x_lo (B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (MB,h,w) u8 with MB
in {1, B}; -> (B,L, s h, s w, 3) u8."""
import numpy as np

F = np.float32


def ingest(photo_u8, s):
    """(B, s h, s w, 3) u8 -> (B,h,w,3) f32: the integer sum of every s x s block, one f64 division, one rounding to f32"""
    assert photo_u8.dtype == np.uint8
    B, H, W, _ = photo_u8.shape
    assert H % s == 0 and W % s == 0
    S = photo_u8.reshape(B, H // s, s, W // s, s, 3).astype(np.int64).sum(axis=(2, 4))
    return (S.astype(np.float64) / (255.0 * s * s)).astype(np.float32)


def taps(n_hi, s, n_lo):
    """one axis of Up: for every hi-res index the two low-res taps and the f32 weight of the second"""
    y = np.arange(n_hi, dtype=np.float32)
    f = np.maximum((y + F(0.5)) / F(s) - F(0.5), F(0.0))
    i0 = np.floor(f)
    t = f - i0
    assert f.dtype == np.float32 and t.dtype == np.float32
    i0 = i0.astype(np.int64)
    return i0, np.minimum(i0 + 1, n_lo - 1), t


def up(a, s):
    """bilinear, half-pixel centres: a (..., h, w) f32 -> (..., s h, s w) f32.  Horizontal first, a0 + tx (a1 - a0) on every row,
    then top + ty (bot - top)"""
    a = np.asarray(a)
    assert a.dtype == np.float32
    h, w = a.shape[-2:]
    y0, y1, ty = taps(s * h, s, h)
    x0, x1, tx = taps(s * w, s, w)
    with np.errstate(invalid="ignore", over="ignore"):
        a0, a1 = a[..., :, x0], a[..., :, x1]
        hz = a0 + tx * (a1 - a0)
        top, bot = hz[..., y0, :], hz[..., y1, :]
        out = top + ty[:, None] * (bot - top)
    assert out.dtype == np.float32
    return out


def quantise_u8(v):
    """saturate_cast<uchar>(cvRound(v)) on f64: round half to even, clip, NaN -> 0"""
    r = np.rint(np.asarray(v, dtype=np.float64))
    return np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0)).astype(np.uint8)


def detail(photo_u8, x_lo, s, detail_clamp=4.0, floor=1.0):
    """d (B,H,W,3) f32 and the photograph as f32"""
    p = photo_u8.astype(np.float32)
    xl = np.transpose(up(np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2))), s), (0, 2, 3, 1)) * F(255.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.fmin(np.fmax(p / np.fmax(xl, F(floor)), F(1.0) / F(detail_clamp)), F(detail_clamp))
    assert d.dtype == np.float32
    return d, p


def mask_up(mask_u8, s):
    """m (MB,H,W) f32"""
    assert mask_u8.dtype == np.uint8
    return up(mask_u8.astype(np.float32) / F(255.0), s)


def values(photo_u8, x_lo, rendered, mask_u8, s, detail_clamp=4.0, floor=1.0):
    """v (B,L,H,W,3) f32 before the quantisation, and m broadcast to (B,1,H,W,1) f32"""
    B, H, W, _ = photo_u8.shape
    h, w = H // s, W // s
    L = rendered.shape[1]
    assert x_lo.shape == (B, h, w, 3) and x_lo.dtype == np.float32
    assert rendered.shape == (B, L, 3, h, w) and rendered.dtype == np.float32
    assert mask_u8.shape in ((1, h, w), (B, h, w))
    d, p = detail(photo_u8, x_lo, s, detail_clamp, floor)
    m = np.broadcast_to(mask_up(mask_u8, s), (B, H, W))[:, None, :, :, None]       # (B,1,H,W,1)
    r = np.transpose(up(rendered, s), (0, 1, 3, 4, 2)) * F(255.0)                   # (B,L,H,W,3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = p[:, None] + m * (r * d[:, None] - p[:, None])
    assert v.dtype == np.float32
    return v, m


def composites(photo_u8, x_lo, rendered, mask_u8, s, detail_clamp=4.0, floor=1.0):
    """-> (B,L,H,W,3) u8"""
    v, m = values(photo_u8, x_lo, rendered, mask_u8, s, detail_clamp, floor)
    return np.where(m > 0, quantise_u8(v), photo_u8[:, None])


def raw_quotient(photo_u8, x_lo, s, floor=1.0):
    """p / max(255 Up(x_lo), floor) before the clamp to [1 / detail_clamp, detail_clamp], (B,H,W,3) f32"""
    xl = np.transpose(up(np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2))), s), (0, 2, 3, 1)) * F(255.0)
    return photo_u8.astype(np.float32) / np.fmax(xl, F(floor))


def tap_footprint(n_hi, s, n_lo, index):
    """the hi-res indices of one axis whose two taps include low-res `index`"""
    i0, i1, _ = taps(n_hi, s, n_lo)
    return np.nonzero((i0 == index) | (i1 == index))[0]
