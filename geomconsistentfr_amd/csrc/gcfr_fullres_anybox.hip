// Full-resolution relighting of a face box of ANY size inside a larger photograph, gfx950: gcfr_fullres_box.hip's two ends without
// its rule bw >= w, bh >= h.  A box axis of nb pixels meets a network axis of n with nb >= 1 and 8 nb >= n; each axis is treated on
// its own, so that a 300 x 200 box over a 256 x 256 network shrinks its columns and stretches its rows.
//   ingest      the box of the uint8 photograph -> the network's f32 input (B, h, w, 3): one exact integer, one rounding
//   composite   the relit low-resolution `rendered` (B,L,3,h,w) of ONE pass carried onto the box's own pixels -> the photograph
//               relit inside the box (paste = 1: (B,L,Hp,Wp,3)) or the box alone (paste = 0: (B,L,bh,bw,3)), ONE launch for all L
//               lights
// With bw >= w and bh >= h every formula below is gcfr_fullres_box.hip's and both kernels return its bits.
//
// Arithmetic (built with -ffp-contract=off: every operation is one separately rounded IEEE operation).
//   Ingest      x_lo[i,j,c] = (float)((double)S / (255.0 Dy Dx)), S = sum_y sum_x wy wx byte in 64 bits.  An axis with nb >= n: the
//               area mean's overlap wy(i,y) = max(0, min((y+1) n, (i+1) nb) - max(y n, i nb)), D = nb.  An axis with nb < n
//               (magnify): N = max((2i+1) nb - n, 0), i0 = N div 2n, rem = N - i0 2n, i1 = min(i0 + 1, nb - 1); tap i0 weighs
//               2n - rem, tap i1 weighs rem (the two may be one pixel), D = 2n.
//   Carry       the operator that takes a plane at the network's resolution to the box, separable, horizontal first on every tap
//               row (each result rounded to f32), then vertical.  An axis with nb >= n: gcfr_fullres_box.hip's two taps and the lerp
//               a0 + t (a1 - a0).  An axis with nb < n (minify): box index y overlaps network index i by
//               wt(y,i) = max(0, min((i+1) nb, (y+1) n) - max(i nb, y n)), i from (y n) div nb to ceil((y+1) n / nb) - 1 (at most
//               nine taps: 8 nb >= n); the value is (float)(acc / (double)n), acc the f64 sum, from +0, of (double)wt (double)v in
//               ascending i: wt <= nb < 2^15 (2 nb n < 2^31), so every product is exact.
//   Composite   inside the box gcfr_fullres.hip's p, xl, d, m, r, v and byte through the SAME device functions (gcfr_fullres.hpp);
//               a pixel of the output window outside the box is the photograph's byte for every light.
//
// Work split (gcfr_fullres_box.hip's): a workgroup of 256 lanes owns kQuadChunk consecutive pixels of ONE face's output window, so
// the two axis modes are uniform over a workgroup and are BRANCHED on.  A lane forms the photograph's bytes, the taps, d and m
// once, then walks the L lights.  VEC (the window's width a multiple of four, out 4-byte aligned): a lane's four pixels lie in one
// row, the photograph's 12 bytes arrive as three dword loads at any alignment and every light's leave as three dword stores; a
// lane whose four pixels are all outside the box copies its three dwords L times.  With both axes lerped the light loop is
// gcfr_fullres_box.hip's (48 taps behind buffer descriptors, requested together); with a minified axis the taps are walked by
// run-time loops that recompute the overlap weight from the index: no per-lane array is indexed dynamically, no scratch, no LDS.
#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"
#include "gcfr_fullres_anybox.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

// WW, WN: the window's width and pixel count (paste: Wp, Hp Wp; else the faces' common bw, bh bw)
template <bool VEC>
__global__ __launch_bounds__(kQuadLanes) void anybox_composites_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t Wp, uint32_t HWp,
    uint32_t WW, uint32_t WN, uint32_t chunks, int32_t paste, float floor, float lo, float hi, BoxArgs boxes,
    uint8_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kQuadChunk);
    const int32_t bx0 = boxes.x0[b], by0 = boxes.y0[b], bw = boxes.bw[b], bh = boxes.bh[b];
    const int32_t ox = paste ? 0 : bx0, oy = paste ? 0 : by0;                      // the window's origin in the photograph
    const bool ay = (uint32_t)bh < h, ax = (uint32_t)bw < w;                       // (uniform) the minified axes
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
        const CarryAxis Y = carry_axis(ay, ry, h, (uint32_t)bh);
        AnyCarrier up[4];
        float p[4][3];
        quad_unpack_u8x3(w3, p);
        float d[3][4], m[4];
        bool relit[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            up[k] = AnyCarrier{ay, ax, h, w, (uint32_t)bh, (uint32_t)bw, Y, carry_axis(ax, rx[k], w, (uint32_t)bw)};
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[c][k] = detail_of(p[k][c], up[k]([&](uint32_t t) { return f.x_lo[3u * (size_t)t + c]; }), floor, lo, hi);
            m[k] = up[k]([&](uint32_t t) { return mask_quotient_f32(f.mask[t]); });
            relit[k] = m[k] > 0.0f && in_x[k];
        }
        uint32_t keep[3];                                                          // relit ? the relit byte : the photograph's
        quad_select_mask(relit, keep);
        if (!ay && !ax) {
            // gcfr_fullres_box.hip's light loop: the taps' BYTE offsets in a plane of `rendered` (4 h w < 2^32: 2 bh h, 2 bw w <
            // 2^31 with bh >= h, bw >= w), a light's 48 taps requested together
            uint32_t off[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                off[k][0] = 4u * (Y.i0 * w + up[k].X.i0), off[k][1] = 4u * (Y.i0 * w + up[k].X.i1);
                off[k][2] = 4u * (Y.i1 * w + up[k].X.i0), off[k][3] = 4u * (Y.i1 * w + up[k].X.i1);
            }
            for (uint32_t l = 0; l < L; ++l) {
                const float *re_l = f.rendered + (size_t)l * 3u * hw;              // (uniform)
                float tap[3][4][4];
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
                    const float r = bilerp(tap[c][k][0], tap[c][k][1], tap[c][k][2], tap[c][k][3], up[k].X.t, Y.t);
                    return quantise_u8((double)fullres_value(p[k][c], m[k], d[c][k], r));
                });
            }
        } else {
            // a minified axis: h w may pass 2^30 here (8 nb >= n only), so the planes are read through flat addresses
            for (uint32_t l = 0; l < L; ++l) {
                const float *re_l = f.rendered + (size_t)l * 3u * hw;              // (uniform)
                quad_store_selected(f.out + 3u * ((size_t)l * WN + q), w3, keep, [&](int k, int c) {
                    const float *plane = re_l + (size_t)c * hw;
                    const float r = up[k]([&](uint32_t t) { return plane[t]; });
                    return quantise_u8((double)fullres_value(p[k][c], m[k], d[c][k], r));
                });
            }
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
            const AnyCarrier up{ay, ax, h, w, (uint32_t)bh, (uint32_t)bw, carry_axis(ay, ry, h, (uint32_t)bh),
                                carry_axis(ax, rx, w, (uint32_t)bw)};
            composite_pixel(up, pb, f, L, hw, WN, px_w, floor, lo, hi);
        }
    }
}

// Ingest (gcfr_fullres_box.hip's work split): a workgroup owns kQuadChunk consecutive network pixels of one face, lane t pixels t,
// t + 256, t + 512, t + 768, one byte at a time.  A row's sum of wx byte is at most 255 max(bw, 2 w) and stays in 32 bits; the
// rows are added in 64.
__global__ __launch_bounds__(kQuadLanes) void anybox_ingest_kernel(const uint8_t *__restrict__ photo, uint32_t h, uint32_t w,
                                                                   uint32_t Wp, uint32_t HWp, uint32_t chunks, BoxArgs boxes,
                                                                   float *__restrict__ x_lo)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<false>(ch * (uint32_t)kQuadChunk);
    const uint32_t bx0 = (uint32_t)boxes.x0[b], by0 = (uint32_t)boxes.y0[b], bw = (uint32_t)boxes.bw[b], bh = (uint32_t)boxes.bh[b];
    const bool my = bh < h, mx = bw < w;                                           // (uniform) the magnified axes
    const uint32_t hw = h * w;
    const uint8_t *ph_b = photo + (size_t)b * 3u * HWp;
    float *xl_b = x_lo + (size_t)b * 3u * hw;
    const double den = 255.0 * (double)(my ? 2u * h : bh) * (double)(mx ? 2u * w : bw);
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const uint32_t px = quad_pixel<false>(q, k);
        if (px >= hw)
            continue;
        const uint32_t i = px / w, j = px - i * w;
        const IngestAxis Y = ingest_axis(my, i, h, bh), X = ingest_axis(mx, j, w, bw);
        uint64_t acc[3] = {0u, 0u, 0u};
        for (uint32_t sy = 0; sy < Y.count; ++sy) {
            uint32_t wy;
            const uint32_t y = ingest_tap(my, Y, sy, h, wy);
            const uint8_t *row = ph_b + 3u * ((size_t)(by0 + y) * Wp + (size_t)bx0);
            uint32_t s[3] = {0u, 0u, 0u};
            for (uint32_t sx = 0; sx < X.count; ++sx) {
                uint32_t wx;
                const uint32_t x = ingest_tap(mx, X, sx, w, wx);
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

extern "C" int gcfr_ingest_anybox_u8(const uint8_t *photo_u8, int32_t B, int32_t Hp, int32_t Wp, const int32_t *boxes, int32_t h,
                                     int32_t w, float *x_lo_out, void *stream)
{
    uint32_t HWp, hw;
    if (!photo_u8 || !x_lo_out || !boxes || (const void *)photo_u8 == (const void *)x_lo_out || !box_shape(B, Hp, Wp, h, w, HWp, hw) ||
        !anyboxes_ok(boxes, B, Hp, Wp, h, w, false))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (hw + kQuadChunk - 1) / kQuadChunk;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        hipLaunchKernelGGL(anybox_ingest_kernel, dim3((uint32_t)n * chunks), dim3(kQuadLanes), 0, st,
                           photo_u8 + (size_t)b0 * 3u * HWp, (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, chunks,
                           box_args(boxes + 4 * b0, n), x_lo_out + (size_t)b0 * 3u * hw);
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_fullres_composites_anybox_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered,
                                                 const uint8_t *mask_u8, int32_t mask_batch, int32_t B, int32_t L, int32_t Hp,
                                                 int32_t Wp, const int32_t *boxes, int32_t h, int32_t w, int32_t paste, float floor,
                                                 float detail_clamp, uint8_t *out_u8, void *stream)
{
    uint32_t HWp, hw, mask_stride;
    float lo;
    if (!boxes || (paste != 0 && paste != 1) || !box_shape(B, Hp, Wp, h, w, HWp, hw) ||
        !fullres_operands(photo_u8, x_lo, rendered, mask_u8, out_u8, L, mask_batch, B, hw, detail_clamp, floor, mask_stride, lo) ||
        !anyboxes_ok(boxes, B, Hp, Wp, h, w, paste == 0))
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
            hipLaunchKernelGGL((anybox_composites_kernel<decltype(V)::value>), grid, dim3(kQuadLanes), 0, st, ph, xl, re, mk,
                               mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, WW, WN, chunks, paste, floor,
                               lo, detail_clamp, args, o);
        });
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
