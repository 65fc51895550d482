"""The box kernels' contract (csrc/gcfr_fullres_box.hip, include/gcfr.h), stated in numpy (helper module, no tests): the ingest of a
face box inside a larger photograph, the bilinear upsample Up over the box and the quotient / detail-transfer composite, f32
throughout -- every numpy operation on f32 arrays below is one separately rounded IEEE f32 operation, as the library's are under
-ffp-contract=off.  It shares no code with the kernels, and none with tests/fullres_emulation.py but the byte quantisation.

Arrays in the C ABI's layouts: photo (B,Hp,Wp,3) u8, boxes (B,4) integers (x0, y0, bw, bh), x_lo (B,h,w,3) f32, rendered
(B,L,3,h,w) f32, mask (MB,h,w) u8 with MB in {1, B} in the box's frame; -> (B,L,Hp,Wp,3) u8 (paste) or (B,L,bh,bw,3) u8."""
import numpy as np

from fullres_emulation import quantise_u8

F = np.float32


def as_boxes(boxes, B):
    b = np.asarray(boxes, dtype=np.int64)
    return np.broadcast_to(b, (B, 4)) if b.ndim == 1 else b


def area_sum(crop, h, w):
    """(bh,bw,3) integers -> (h,w,3) int64: every row repeated h times and regrouped into h groups of bh rows, every column
    repeated w times and regrouped into w groups of bw columns, summed.  Each low-resolution cell receives bh bw terms"""
    bh, bw, _ = crop.shape
    r = np.repeat(crop.astype(np.int64), h, axis=0).reshape(h, bh, bw, 3).sum(axis=1)
    return np.repeat(r, w, axis=1).reshape(h, w, bw, 3).sum(axis=2)


def overlap(n_box, n_lo):
    """(n_lo, n_box) int64: w(i,y) = max(0, min((y+1) n_lo, (i+1) n_box) - max(y n_lo, i n_box))"""
    i, y = np.arange(n_lo, dtype=np.int64)[:, None], np.arange(n_box, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((y + 1) * n_lo, (i + 1) * n_box) - np.maximum(y * n_lo, i * n_box))


def overlap_sum(crop, h, w):
    """the same integer as `area_sum`, by the statement's overlap weights"""
    bh, bw, _ = crop.shape
    return np.einsum("iy,jx,yxc->ijc", overlap(bh, h), overlap(bw, w), crop.astype(np.int64))


def ingest(photo_u8, boxes, h, w):
    """-> (B,h,w,3) f32: the integer area sum of each face's box, one f64 division by 255 bh bw, one rounding to f32"""
    assert photo_u8.dtype == np.uint8
    B = photo_u8.shape[0]
    out = np.empty((B, h, w, 3), np.float32)
    for b, (x0, y0, bw, bh) in enumerate(as_boxes(boxes, B)):
        S = area_sum(photo_u8[b, y0:y0 + bh, x0:x0 + bw], h, w)
        out[b] = (S.astype(np.float64) / (255.0 * bh * bw)).astype(np.float32)
    return out


def taps(n_box, n_lo):
    """one axis of Up over a box: for every box-relative index the two low-res taps and the f32 weight of the second"""
    y = np.arange(n_box, dtype=np.int64)
    N = np.maximum((2 * y + 1) * n_lo - n_box, 0)
    i0 = N // (2 * n_box)
    rem = N - i0 * 2 * n_box
    t = (rem.astype(np.float64) / np.float64(2 * n_box)).astype(np.float32)
    return i0, np.minimum(i0 + 1, n_lo - 1), t


def up(a, bh, bw):
    """bilinear, half-pixel centres: a (..., h, w) f32 -> (..., bh, bw) f32.  Horizontal first, a0 + tx (a1 - a0) on every row,
    then top + ty (bot - top)"""
    a = np.asarray(a)
    assert a.dtype == np.float32
    h, w = a.shape[-2:]
    y0, y1, ty = taps(bh, h)
    x0, x1, tx = taps(bw, w)
    with np.errstate(invalid="ignore", over="ignore"):
        a0, a1 = a[..., :, x0], a[..., :, x1]
        hz = a0 + tx * (a1 - a0)
        top, bot = hz[..., y0, :], hz[..., y1, :]
        out = top + ty[:, None] * (bot - top)
    assert out.dtype == np.float32
    return out


def box_values(crop_u8, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0):
    """one face: crop (bh,bw,3) u8, x_lo (h,w,3), rendered (L,3,h,w), mask (h,w) u8 -> v (L,bh,bw,3) f32 before the quantisation,
    m (bh,bw) f32 and d (bh,bw,3) f32"""
    bh, bw, _ = crop_u8.shape
    p = crop_u8.astype(np.float32)
    xl = np.transpose(up(np.ascontiguousarray(np.transpose(x_lo, (2, 0, 1))), bh, bw), (1, 2, 0)) * F(255.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.fmin(np.fmax(p / np.fmax(xl, F(floor)), F(1.0) / F(detail_clamp)), F(detail_clamp))
    m = up(mask_u8.astype(np.float32) / F(255.0), bh, bw)
    r = np.transpose(up(rendered, bh, bw), (0, 2, 3, 1)) * F(255.0)                 # (L,bh,bw,3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = p[None] + m[None, :, :, None] * (r * d[None] - p[None])
    assert v.dtype == np.float32 and d.dtype == np.float32 and m.dtype == np.float32
    return v, m, d


def box_composite(crop_u8, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0):
    """one face -> (L,bh,bw,3) u8"""
    v, m, _ = box_values(crop_u8, x_lo, rendered, mask_u8, detail_clamp, floor)
    return np.where(m[None, :, :, None] > 0, quantise_u8(v), crop_u8[None])


def composites(photo_u8, boxes, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, paste=True):
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
                            detail_clamp, floor)
        if paste:
            out[b, :, y0:y0 + bh, x0:x0 + bw] = box
        else:
            out[b] = box
    return out


def tap_footprint(n_box, n_lo, index):
    """the box-relative indices of one axis whose two taps include low-res `index`"""
    i0, i1, _ = taps(n_box, n_lo)
    return np.nonzero((i0 == index) | (i1 == index))[0]
