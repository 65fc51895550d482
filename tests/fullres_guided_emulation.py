"""The guided full-resolution composite's contract (csrc/gcfr_fullres_guided.hip, include/gcfr.h), stated in numpy (helper module,
no tests): the joint-bilateral upsample Up_J and the quotient / detail-transfer composite with Up_J in all three places, f32
throughout -- every numpy operation below is one separately rounded IEEE f32 operation on f32 arrays, as the library's are under
-ffp-contract=off.  It shares no code with the kernel; the ingest, the quantisation and the layouts are tests/fullres_emulation.py's.

Arrays in the C ABI's layouts: photo (B, s h, s w, 3) u8, x_lo (B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (MB,h,w) u8 with MB
in {1, B}; -> (B,L, s h, s w, 3) u8."""
import numpy as np

from fullres_emulation import ingest, quantise_u8  # noqa: F401  (re-exported: one import serves a test)

F = np.float32


def taps(n_hi, s, n_lo):
    """one axis of Up_J, in integers: for every hi-res index the four clamped low-res taps (n_hi,4) and their integer weights
    (2 s - r, 4 s - r, 2 s + r, r), to be taken over 4 s"""
    y = np.arange(n_hi, dtype=np.int64)
    u = np.maximum(2 * y + 1 - s, 0)
    y0, r = u // (2 * s), u % (2 * s)
    idx = np.clip(y0[:, None] - 1 + np.arange(4)[None, :], 0, n_lo - 1)
    wint = np.stack([2 * s - r, 4 * s - r, 2 * s + r, r], axis=1)
    return idx, wint


def spatial(n_hi, s, n_lo):
    """the taps and their weights as f32 (exact: s is a power of two)"""
    idx, wint = taps(n_hi, s, n_lo)
    wf = wint.astype(np.float32) / F(4 * s)
    assert wf.dtype == np.float32 and (wf.astype(np.float64) * (4 * s) == wint).all()
    return idx, wf


def gather(a, s):
    """a (..., h, w) -> (..., H, W, 4, 4): the 16 taps of every hi-res pixel, [j][i] = a[row tap j, column tap i]"""
    h, w = a.shape[-2:]
    iy, _ = taps(s * h, s, h)
    ix, _ = taps(s * w, s, w)
    return a[..., iy[:, None, :, None], ix[None, :, None, :]]


def inverse_sigma2(range_sigma):
    """inv = 1.0f / (range_sigma range_sigma), in f32 as the host forms it"""
    sg = F(range_sigma)
    with np.errstate(over="ignore", divide="ignore", under="ignore"):
        return F(1.0) / (sg * sg)


def weights(photo_u8, x_lo, s, range_sigma=20.0):
    """the normalised weights wn (B,H,W,4,4) f32 of every hi-res pixel, and den (B,H,W) f32"""
    assert photo_u8.dtype == np.uint8 and x_lo.dtype == np.float32
    B, H, W, _ = photo_u8.shape
    h, w = H // s, W // s
    assert x_lo.shape == (B, h, w, 3)
    _, sy = spatial(H, s, h)
    _, sx = spatial(W, s, w)
    inv = inverse_sigma2(range_sigma)
    p = photo_u8.astype(np.float32)                                                 # (B,H,W,3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = [gather(np.ascontiguousarray(x_lo[..., c]) * F(255.0), s) for c in range(3)]   # 3 x (B,H,W,4,4)
        e = [p[..., c][..., None, None] - g[c] for c in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        k = F(1.0) / (F(1.0) + d2 * inv)
        wt = (sy[:, None, :, None] * sx[None, :, None, :]) * k                      # (B,H,W,4,4)
        den = wt[..., 0, 0]
        for t in range(1, 16):
            den = den + wt[..., t // 4, t % 4]
        rcp = F(1.0) / den
        wn = wt * rcp[..., None, None]
    assert wn.dtype == np.float32 and den.dtype == np.float32
    return wn, den


def up_j(a, wn, s):
    """Up_J: a (..., h, w) f32 with leading axes that broadcast against wn's (..., H, W, 4, 4) -> (..., H, W) f32.  The sum runs
    row-major over the 16 taps; the first product starts it"""
    a = np.asarray(a)
    assert a.dtype == np.float32 and wn.dtype == np.float32
    t16 = gather(a, s)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = wn[..., 0, 0] * t16[..., 0, 0]
        for t in range(1, 16):
            acc = acc + wn[..., t // 4, t % 4] * t16[..., t // 4, t % 4]
    assert acc.dtype == np.float32
    return acc


def parts(photo_u8, x_lo, mask_u8, s, detail_clamp=4.0, floor=1.0, range_sigma=20.0):
    """what is formed once per pixel: wn (B,H,W,4,4), the raw quotient and d (B,H,W,3), xl (B,H,W,3), m (B,H,W), all f32"""
    B, H, W, _ = photo_u8.shape
    h, w = H // s, W // s
    assert mask_u8.dtype == np.uint8 and mask_u8.shape in ((1, h, w), (B, h, w))
    wn, _ = weights(photo_u8, x_lo, s, range_sigma)
    p = photo_u8.astype(np.float32)
    xl = np.stack([up_j(np.ascontiguousarray(x_lo[..., c]), wn, s) for c in range(3)], axis=-1) * F(255.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        raw = p / np.fmax(xl, F(floor))
        d = np.fmin(np.fmax(raw, F(1.0) / F(detail_clamp)), F(detail_clamp))
    m = up_j(np.broadcast_to(mask_u8.astype(np.float32) / F(255.0), (B, h, w)), wn, s)
    assert d.dtype == np.float32 and m.dtype == np.float32
    return wn, raw, d, xl, m


def values(photo_u8, x_lo, rendered, mask_u8, s, detail_clamp=4.0, floor=1.0, range_sigma=20.0):
    """v (B,L,H,W,3) f32 before the quantisation, and m broadcast to (B,1,H,W,1) f32"""
    B, H, W, _ = photo_u8.shape
    h, w = H // s, W // s
    L = rendered.shape[1]
    assert rendered.shape == (B, L, 3, h, w) and rendered.dtype == np.float32
    wn, _, d, _, m = parts(photo_u8, x_lo, mask_u8, s, detail_clamp, floor, range_sigma)
    p = photo_u8.astype(np.float32)
    r = np.transpose(up_j(rendered, wn[:, None, None], s), (0, 1, 3, 4, 2)) * F(255.0)   # (B,L,H,W,3)
    m = m[:, None, :, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        v = p[:, None] + m * (r * d[:, None] - p[:, None])
    assert v.dtype == np.float32
    return v, m


def composites(photo_u8, x_lo, rendered, mask_u8, s, detail_clamp=4.0, floor=1.0, range_sigma=20.0):
    """-> (B,L,H,W,3) u8"""
    v, m = values(photo_u8, x_lo, rendered, mask_u8, s, detail_clamp, floor, range_sigma)
    return np.where(m > 0, quantise_u8(v), photo_u8[:, None])
