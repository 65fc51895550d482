// Full-resolution relighting of a FACE BOX inside a larger photograph, gfx950: gcfr_fullres.hip's two ends of the inference path
// for a box (x0, y0, bw, bh) of any integer size and position in a photograph (Hp, Wp) of any size, bw >= w and bh >= h.
//   ingest      the box of the uint8 photograph -> the network's f32 input (B, h, w, 3): the exact area mean / 255
//   composite   the relit low-resolution `rendered` (B,L,3,h,w) of ONE pass carried back onto the box's own pixels -> the
//               photograph relit inside the box and untouched outside it (paste = 1: (B,L,Hp,Wp,3)) or the box alone (paste = 0:
//               (B,L,bh,bw,3)), ONE launch for all L lights
// The two axes are independent: bh / h need not equal bw / w, and neither needs to be an integer.  With the box the whole
// photograph and bh = s h, bw = s w, s in {1, 2, 4, 8}, both kernels return gcfr_fullres.hip's bits.
//
// Arithmetic (built with -ffp-contract=off: every operation is one separately rounded IEEE f32 operation unless marked).
//   Ingest      On the row axis photograph row y of the box and low-resolution row i overlap by the integer
//               wy(i,y) = max(0, min((y+1) h, (i+1) bh) - max(y h, i bh)) in [0, h]; columns likewise.  S[i,j,c] = sum wy wx byte,
//               an exact integer of at most 255 bh bw (64 bits); x_lo = (float)((double)S / (255.0 bh bw)): the denominator is
//               exact in f64, the quotient is rounded once.
//   Up          per axis and box-relative index y: N = max((2y+1) h - bh, 0), y0 = N div 2 bh, rem = N - y0 2 bh,
//               t = (float)((double)rem / (double)(2 bh)), y1 = min(y0 + 1, h - 1): integers but for the one rounding of t.  The
//               lerps and their order are gcfr_fullres.hpp's bilerp; both taps are always read.
//   Composite   inside the box gcfr_fullres.hip's p, xl, d, m, r, v and byte, through the SAME device functions
//               (gcfr_fullres.hpp: bilerp / detail_of / fullres_value / fullres_byte; the scalar path is its composite_pixel over
//               a Bilinear4 filled from box_tap); a pixel of the output window outside the box is the photograph's byte for every
//               light.
//
// The boxes arrive in a HOST array, are validated on the host and travel BY VALUE in the kernel's argument block (BoxArgs, in
// gcfr_fullres.hpp: up to kBoxFaces faces per launch; more faces are a short loop of launches): nothing is uploaded, no device scratch,
// capture-safe.
//
// Work split of the composite (gcfr_fullres.hip's): a workgroup of 256 lanes owns kQuadChunk = 1024 consecutive pixels of ONE face's
// output WINDOW -- the photograph (paste = 1) or the box (paste = 0); the two differ in the window's origin and size only.  A lane
// forms the photograph's bytes, the tap indices, both weights, d[3][4] and m[4] ONCE, then walks the L lights: per light only the
// taps of `rendered` are fetched (cache-served: each is shared by about (bh / h)(bw / w) pixels) and 12 bytes are stored.  The
// `m > 0` select and the inside-the-box select are ONE byte mask (gcfr_fullres.hpp: quad_select_mask) formed once per lane; the
// light loop has no division and no branch.  A pixel outside the box computes on the box's nearest pixel (its indices are clamped: every address stays in range)
// and its bytes are masked away; a lane whose four pixels are all outside copies its three dwords L times instead.
// VEC (the window's width a multiple of four, out 4-byte aligned): lane t owns pixels 4 t .. 4 t + 3 of the chunk, all in one row;
// every light's 12 bytes leave as three dwords.  The photograph's 12 bytes arrive as three dword loads that need no alignment (a
// box starts at any column).  Each pixel loads its own two column taps on the lane's two rows.  Otherwise lane t owns pixels
// t, t + 256, t + 512, t + 768 and everything moves one element at a time: the same bytes.
#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

// one axis of Up over a box: box-relative index i of a box axis of nb over a low-resolution axis of n (2 nb n < 2^31)
__device__ inline void box_tap(uint32_t i, uint32_t n, uint32_t nb, uint32_t &i0, uint32_t &i1, float &t)
{
    const uint32_t a = (2u * i + 1u) * n;
    const uint32_t N = a > nb ? a - nb : 0u;
    const uint32_t den = 2u * nb;
    i0 = N / den;                                                                  // (<= n - 1)
    const uint32_t rem = N - i0 * den;
    t = (float)((double)rem / (double)den);
    i1 = i0 + 1u < n ? i0 + 1u : n - 1u;
}

// WW, WN: the window's width and pixel count (paste: Wp, Hp Wp; else the faces' common bw, bh bw)
template <bool VEC>
__global__ __launch_bounds__(kQuadLanes) void fullres_composites_box_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t Wp, uint32_t HWp,
    uint32_t WW, uint32_t WN, uint32_t chunks, int32_t paste, float floor, float lo, float hi, BoxArgs boxes,
    uint8_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kQuadChunk);
    const int32_t bx0 = boxes.x0[b], by0 = boxes.y0[b], bw = boxes.bw[b], bh = boxes.bh[b];
    const int32_t ox = paste ? 0 : bx0, oy = paste ? 0 : by0;                      // the window's origin in the photograph
    const uint32_t hw = h * w;
    const FacePlanes f = face_planes(photo, x_lo, rendered, mask, out, b, mask_stride, L, hw, HWp, WN);
    if (VEC) {
        if (q >= WN)                                                               // all four pixels in range or none
            return;
        const uint32_t wy = q / WW, wx = q - wy * WW;
        const int32_t py = oy + (int32_t)wy, px = ox + (int32_t)wx;
        const uint8_t *pp = f.photo + 3u * ((size_t)py * Wp + (size_t)px);
        const uint32_t w3[3] = {load_dword_any(pp), load_dword_any(pp + 4), load_dword_any(pp + 8)};
        bool in_y, in_x[4], any = false;
        const uint32_t ry = box_clamp(py, by0, bh, in_y);
        uint32_t rx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rx[k] = box_clamp(px + k, bx0, bw, in_x[k]);
            in_x[k] = in_x[k] && in_y;
            any = any || in_x[k];
        }
        if (!any) {                                                                // the photograph's bytes for every light
            for (uint32_t l = 0; l < L; ++l) {
                uint32_t *ow = reinterpret_cast<uint32_t *>(f.out + 3u * ((size_t)l * WN + q));
                ow[0] = w3[0], ow[1] = w3[1], ow[2] = w3[2];
            }
            return;
        }
        uint32_t y0, y1, roff[2], c0[4], c1[4];
        float ty, tx[4];
        box_tap(ry, h, (uint32_t)bh, y0, y1, ty);
        roff[0] = y0 * w, roff[1] = y1 * w;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            box_tap(rx[k], w, (uint32_t)bw, c0[k], c1[k], tx[k]);
        float p[4][3];
        quad_unpack_u8x3(w3, p);
        float d[3][4], m[4];
        bool relit[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t t00 = roff[0] + c0[k], t01 = roff[0] + c1[k], t10 = roff[1] + c0[k], t11 = roff[1] + c1[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float up = bilerp(f.x_lo[3u * (size_t)t00 + c], f.x_lo[3u * (size_t)t01 + c], f.x_lo[3u * (size_t)t10 + c],
                                        f.x_lo[3u * (size_t)t11 + c], tx[k], ty);
                d[c][k] = detail_of(p[k][c], up, floor, lo, hi);
            }
            m[k] = bilerp(mask_quotient_f32(f.mask[t00]), mask_quotient_f32(f.mask[t01]), mask_quotient_f32(f.mask[t10]),
                          mask_quotient_f32(f.mask[t11]), tx[k], ty);
            relit[k] = m[k] > 0.0f && in_x[k];
        }
        uint32_t keep[3];                                                          // relit ? the relit byte : the photograph's
        quad_select_mask(relit, keep);
        // the taps' BYTE offsets in a plane of `rendered` (4 h w < 2^32: 2 bh h, 2 bw w < 2^31 with bh >= h, bw >= w), so that a
        // light's loads are a uniform plane address plus one 32-bit register each
        uint32_t off[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            off[k][0] = 4u * (roff[0] + c0[k]), off[k][1] = 4u * (roff[0] + c1[k]);
            off[k][2] = 4u * (roff[1] + c0[k]), off[k][3] = 4u * (roff[1] + c1[k]);
        }
        for (uint32_t l = 0; l < L; ++l) {
            const float *re_l = f.rendered + (size_t)l * 3u * hw;                  // (uniform)
            float tap[3][4][4];                                                    // a light's 48 taps, requested together
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const PlaneF32 plane(re_l + (size_t)c * hw, hw);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        tap[c][k][j] = plane.at(off[k][j]);
            }
            quad_store_selected(f.out + 3u * ((size_t)l * WN + q), w3, keep, [&](int k, int c) {
                const float r = bilerp(tap[c][k][0], tap[c][k][1], tap[c][k][2], tap[c][k][3], tx[k], ty);
                return quantise_u8((double)fullres_value(p[k][c], m[k], d[c][k], r));
            });
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const uint32_t px_w = quad_pixel<false>(q, k);
            if (px_w >= WN)
                continue;
            const uint32_t wy = px_w / WW, wx = px_w - wy * WW;
            const int32_t py = oy + (int32_t)wy, px = ox + (int32_t)wx;
            const uint8_t *pp = f.photo + 3u * ((size_t)py * Wp + (size_t)px);
            const uint8_t pb[3] = {pp[0], pp[1], pp[2]};
            bool in_y, in_x;
            const uint32_t ry = box_clamp(py, by0, bh, in_y), rx = box_clamp(px, bx0, bw, in_x);
            if (!(in_y && in_x)) {
                for (uint32_t l = 0; l < L; ++l) {
                    uint8_t *o = f.out + 3u * ((size_t)l * WN + px_w);
                    o[0] = pb[0], o[1] = pb[1], o[2] = pb[2];
                }
                continue;
            }
            uint32_t y0, y1, x0, x1;
            float ty, tx;
            box_tap(ry, h, (uint32_t)bh, y0, y1, ty);
            box_tap(rx, w, (uint32_t)bw, x0, x1, tx);
            composite_pixel(Bilinear4(y0, y1, x0, x1, w, tx, ty), pb, f, L, hw, WN, px_w, floor, lo, hi);
        }
    }
}

// Ingest: a workgroup owns kQuadChunk consecutive LOW-resolution pixels of one face; lane t owns pixels t, t + 256, t + 512,
// t + 768.  A low-resolution pixel walks the photograph rows and columns its cell overlaps (at most bh / h + 2 by bw / w + 2), one
// byte at a time: a box starts at any byte of the photograph, so there is one path.  A row's sum of wx byte is at most 255 bw and
// stays in 32 bits; the rows are added in 64.
__global__ __launch_bounds__(kQuadLanes) void ingest_box_kernel(const uint8_t *__restrict__ photo, uint32_t h, uint32_t w, uint32_t Wp,
                                                                uint32_t HWp, uint32_t chunks, BoxArgs boxes,
                                                                float *__restrict__ x_lo)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<false>(ch * (uint32_t)kQuadChunk);
    const uint32_t bx0 = (uint32_t)boxes.x0[b], by0 = (uint32_t)boxes.y0[b], bw = (uint32_t)boxes.bw[b], bh = (uint32_t)boxes.bh[b];
    const uint32_t hw = h * w;
    const uint8_t *ph_b = photo + (size_t)b * 3u * HWp;
    float *xl_b = x_lo + (size_t)b * 3u * hw;
    const double den = 255.0 * (double)bh * (double)bw;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const uint32_t px = quad_pixel<false>(q, k);
        if (px >= hw)
            continue;
        const uint32_t i = px / w, j = px - i * w;
        const uint32_t ya = i * bh, yb = ya + bh, xa = j * bw, xb = xa + bw;       // the cell in units of 1 / h, 1 / w of a pixel
        const uint32_t yf = ya / h, yl = (yb + h - 1u) / h, xf = xa / w, xl = (xb + w - 1u) / w;
        uint64_t acc[3] = {0u, 0u, 0u};
        for (uint32_t y = yf; y < yl; ++y) {
            const uint32_t wy = min((y + 1u) * h, yb) - max(y * h, ya);
            const uint8_t *row = ph_b + 3u * ((size_t)(by0 + y) * Wp + (size_t)bx0);
            uint32_t s[3] = {0u, 0u, 0u};
            for (uint32_t x = xf; x < xl; ++x) {
                const uint32_t wx = min((x + 1u) * w, xb) - max(x * w, xa);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    s[c] += wx * row[3u * (size_t)x + c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                acc[c] += (uint64_t)wy * s[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            xl_b[3u * (size_t)px + c] = (float)((double)acc[c] / den);
    }
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_ingest_box_u8(const uint8_t *photo_u8, int32_t B, int32_t Hp, int32_t Wp, const int32_t *boxes, int32_t h,
                                  int32_t w, float *x_lo_out, void *stream)
{
    uint32_t HWp, hw;
    if (!photo_u8 || !x_lo_out || !boxes || (const void *)photo_u8 == (const void *)x_lo_out || !box_shape(B, Hp, Wp, h, w, HWp, hw) ||
        !boxes_ok(boxes, B, Hp, Wp, h, w, false))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (hw + kQuadChunk - 1) / kQuadChunk;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        hipLaunchKernelGGL(ingest_box_kernel, dim3((uint32_t)n * chunks), dim3(kQuadLanes), 0, st, photo_u8 + (size_t)b0 * 3u * HWp,
                           (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, chunks, box_args(boxes + 4 * b0, n),
                           x_lo_out + (size_t)b0 * 3u * hw);
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_fullres_composites_box_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                              int32_t mask_batch, int32_t B, int32_t L, int32_t Hp, int32_t Wp, const int32_t *boxes,
                                              int32_t h, int32_t w, int32_t paste, float floor, float detail_clamp, uint8_t *out_u8,
                                              void *stream)
{
    uint32_t HWp, hw, mask_stride;
    float lo;
    if (!boxes || (paste != 0 && paste != 1) || !box_shape(B, Hp, Wp, h, w, HWp, hw) ||
        !fullres_operands(photo_u8, x_lo, rendered, mask_u8, out_u8, L, mask_batch, B, hw, detail_clamp, floor, mask_stride, lo) ||
        !boxes_ok(boxes, B, Hp, Wp, h, w, paste == 0))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t WW = paste ? (uint32_t)Wp : (uint32_t)boxes[2];
    const uint32_t WN = paste ? HWp : (uint32_t)boxes[2] * (uint32_t)boxes[3];     // (<= Hp Wp)
    // out must not overlap the photographs
    const uintptr_t pa = (uintptr_t)photo_u8, pe = pa + (uintptr_t)B * 3u * HWp;
    const uintptr_t oa = (uintptr_t)out_u8, oe = oa + (uintptr_t)B * (uintptr_t)L * 3u * WN;
    if (oa < pe && pa < oe)
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (WN + kQuadChunk - 1) / kQuadChunk;
    const bool vec = WW % 4u == 0 && aligned4(out_u8);
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        const dim3 grid((uint32_t)n * chunks);
        const BoxArgs args = box_args(boxes + 4 * b0, n);
        const uint8_t *ph = photo_u8 + (size_t)b0 * 3u * HWp;
        const float *xl = x_lo + (size_t)b0 * 3u * hw, *re = rendered + (size_t)b0 * (size_t)L * 3u * hw;
        const uint8_t *mk = mask_u8 + (size_t)b0 * mask_stride;
        uint8_t *o = out_u8 + (size_t)b0 * (size_t)L * 3u * WN;
        with_flag(vec, [&](auto V) {
            hipLaunchKernelGGL((fullres_composites_box_kernel<decltype(V)::value>), grid, dim3(kQuadLanes), 0, st, ph, xl, re, mk,
                               mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, WW, WN, chunks, paste, floor, lo,
                               detail_clamp, args, o);
        });
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
