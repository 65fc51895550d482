"""The guided box composite's contract (csrc/gcfr_fullres_box_guided.hip, include/gcfr.h), stated in numpy (helper module, no
tests): the joint-bilateral upsample Up_J over a face box of any integer size and the quotient / detail-transfer composite with Up_J
in all three places, f32 throughout -- every numpy operation on f32 arrays below is one separately rounded IEEE f32 operation, as
the library's are under -ffp-contract=off.  It shares no code with the kernels; the boxes, the box ingest and the byte quantisation
are the existing restatements'.

Arrays in the C ABI's layouts: photo (B,Hp,Wp,3) u8, boxes (B,4) integers (x0, y0, bw, bh), x_lo (B,h,w,3) f32, rendered
(B,L,3,h,w) f32, mask (MB,h,w) u8 with MB in {1, B} in the box's frame; -> (B,L,Hp,Wp,3) u8 (paste) or (B,L,bh,bw,3) u8."""
import numpy as np

from fullres_box_emulation import as_boxes, ingest  # noqa: F401  (re-exported: one import serves a test)
from fullres_emulation import quantise_u8

F = np.float32


def taps(n_box, n_lo):
    """one axis of Up_J over a box, in integers: for every box-relative index the four clamped low-res taps (n_box,4) and their
    integer weights (2 b - rem, 4 b - rem, 2 b + rem, rem), to be taken over 4 b"""
    y = np.arange(n_box, dtype=np.int64)
    N = np.maximum((2 * y + 1) * n_lo - n_box, 0)
    y0 = N // (2 * n_box)
    rem = N - y0 * 2 * n_box
    idx = np.clip(y0[:, None] - 1 + np.arange(4)[None, :], 0, n_lo - 1)
    wint = np.stack([2 * n_box - rem, 4 * n_box - rem, 2 * n_box + rem, rem], axis=1)
    return idx, wint


def spatial(n_box, n_lo):
    """the taps and their f32 weights: each the f64 quotient k / (4 b) of two exact integers, rounded once to f32"""
    idx, wint = taps(n_box, n_lo)
    wf = (wint.astype(np.float64) / np.float64(4 * n_box)).astype(np.float32)
    return idx, wf


def gather(a, bh, bw):
    """a (..., h, w) -> (..., bh, bw, 4, 4): the 16 taps of every box pixel, [j][i] = a[row tap j, column tap i]"""
    h, w = a.shape[-2:]
    iy, _ = taps(bh, h)
    ix, _ = taps(bw, w)
    return a[..., iy[:, None, :, None], ix[None, :, None, :]]


def inverse_sigma2(range_sigma):
    """inv = 1.0f / (range_sigma range_sigma), in f32 as the host forms it"""
    sg = F(range_sigma)
    with np.errstate(over="ignore", divide="ignore", under="ignore"):
        return F(1.0) / (sg * sg)


def weights(crop_u8, x_lo, range_sigma=20.0):
    """one face: crop (bh,bw,3) u8, x_lo (h,w,3) f32 -> the normalised weights wn (bh,bw,4,4) f32 and den (bh,bw) f32"""
    assert crop_u8.dtype == np.uint8 and x_lo.dtype == np.float32
    bh, bw, _ = crop_u8.shape
    h, w, _ = x_lo.shape
    _, sy = spatial(bh, h)
    _, sx = spatial(bw, w)
    inv = inverse_sigma2(range_sigma)
    p = crop_u8.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = [gather(np.ascontiguousarray(x_lo[..., c]) * F(255.0), bh, bw) for c in range(3)]   # 3 x (bh,bw,4,4)
        e = [p[..., c][..., None, None] - g[c] for c in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        k = F(1.0) / (F(1.0) + d2 * inv)
        wt = (sy[:, None, :, None] * sx[None, :, None, :]) * k                      # the product of the two weights is rounded
        den = wt[..., 0, 0]
        for t in range(1, 16):
            den = den + wt[..., t // 4, t % 4]
        rcp = F(1.0) / den
        wn = wt * rcp[..., None, None]
    assert wn.dtype == np.float32 and den.dtype == np.float32
    return wn, den


def up_j(a, wn):
    """Up_J: a (..., h, w) f32 with leading axes that broadcast against wn's (bh, bw, 4, 4) -> (..., bh, bw) f32.  The sum runs
    row-major over the 16 taps; the first product starts it"""
    a = np.asarray(a)
    assert a.dtype == np.float32 and wn.dtype == np.float32
    bh, bw = wn.shape[-4:-2]
    t16 = gather(a, bh, bw)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = wn[..., 0, 0] * t16[..., 0, 0]
        for t in range(1, 16):
            acc = acc + wn[..., t // 4, t % 4] * t16[..., t // 4, t % 4]
    assert acc.dtype == np.float32
    return acc


def box_parts(crop_u8, x_lo, mask_u8, detail_clamp=4.0, floor=1.0, range_sigma=20.0):
    """one face, what is formed once per pixel: wn (bh,bw,4,4), the raw quotient and d (bh,bw,3), xl (bh,bw,3), m (bh,bw), all f32"""
    assert mask_u8.dtype == np.uint8 and mask_u8.shape == x_lo.shape[:2]
    wn, _ = weights(crop_u8, x_lo, range_sigma)
    p = crop_u8.astype(np.float32)
    xl = np.stack([up_j(np.ascontiguousarray(x_lo[..., c]), wn) for c in range(3)], axis=-1) * F(255.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        raw = p / np.fmax(xl, F(floor))
        d = np.fmin(np.fmax(raw, F(1.0) / F(detail_clamp)), F(detail_clamp))
    m = up_j(mask_u8.astype(np.float32) / F(255.0), wn)
    assert d.dtype == np.float32 and m.dtype == np.float32
    return wn, raw, d, xl, m


def box_values(crop_u8, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, range_sigma=20.0):
    """one face: crop (bh,bw,3) u8, x_lo (h,w,3), rendered (L,3,h,w), mask (h,w) u8 -> v (L,bh,bw,3) f32 before the quantisation,
    m (bh,bw) f32 and d (bh,bw,3) f32"""
    assert rendered.dtype == np.float32 and rendered.shape[1:] == (3,) + x_lo.shape[:2]
    wn, _, d, _, m = box_parts(crop_u8, x_lo, mask_u8, detail_clamp, floor, range_sigma)
    p = crop_u8.astype(np.float32)
    r = np.transpose(up_j(rendered, wn), (0, 2, 3, 1)) * F(255.0)                   # (L,bh,bw,3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = p[None] + m[None, :, :, None] * (r * d[None] - p[None])
    assert v.dtype == np.float32
    return v, m, d


def box_composite(crop_u8, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, range_sigma=20.0):
    """one face -> (L,bh,bw,3) u8"""
    v, m, _ = box_values(crop_u8, x_lo, rendered, mask_u8, detail_clamp, floor, range_sigma)
    return np.where(m[None, :, :, None] > 0, quantise_u8(v), crop_u8[None])


def composites(photo_u8, boxes, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, paste=True, range_sigma=20.0):
    """-> (B,L,Hp,Wp,3) u8, the photograph relit inside each face's box, or with paste=False (B,L,bh,bw,3) u8, the boxes alone"""
    B, Hp, Wp, _ = photo_u8.shape
    L = rendered.shape[1]
    h, w = x_lo.shape[1:3]
    bx = as_boxes(boxes, B)
    assert x_lo.shape == (B, h, w, 3) and x_lo.dtype == np.float32
    assert rendered.shape == (B, L, 3, h, w) and rendered.dtype == np.float32
    assert mask_u8.shape in ((1, h, w), (B, h, w)) and mask_u8.dtype == np.uint8
    if paste:
        out = np.repeat(photo_u8[:, None], L, axis=1)
    else:
        assert (bx[:, 2:] == bx[0, 2:]).all()
        out = np.empty((B, L, int(bx[0, 3]), int(bx[0, 2]), 3), np.uint8)
    for b, (x0, y0, bw, bh) in enumerate(bx):
        box = box_composite(photo_u8[b, y0:y0 + bh, x0:x0 + bw], x_lo[b], rendered[b], mask_u8[b if mask_u8.shape[0] > 1 else 0],
                            detail_clamp, floor, range_sigma)
        if paste:
            out[b, :, y0:y0 + bh, x0:x0 + bw] = box
        else:
            out[b] = box
    return out


def tap_footprint(n_box, n_lo, index):
    """the box-relative indices of one axis whose four taps include low-res `index`"""
    idx, _ = taps(n_box, n_lo)
    return np.nonzero((idx == index).any(axis=1))[0]
