// Full-resolution relighting of a FACE BOX inside a larger photograph with the EDGE-AWARE (joint-bilateral) upsample Up_J, gfx950:
// gcfr_fullres_box.hip's composite with gcfr_fullres_guided.hip's Up_J, its taps generalised from s in {1, 2, 4, 8} to a box of any
// integer size (bw >= w, bh >= h; the two ratios independent, neither an integer).  Operands, layouts, box rules and `paste` are
// gcfr_fullres_composites_box_u8's, plus `range_sigma` (grey levels).  With the box the whole photograph and bh = s h, bw = s w,
// s in {1, 2, 4, 8}, the bytes are gcfr_fullres_composites_guided_u8's.
//
// Arithmetic (-ffp-contract=off: every operation is one separately rounded IEEE f32 operation unless marked).
//   Taps        per axis, box-relative index y, box extent b, low-resolution extent n; the integers are box_tap's:
//               N = max((2y+1) n - b, 0), y0 = N div 2b, rem = N - y0 2b.  The four taps are clamp(y0 - 1 + j, 0, n - 1), j = 0..3,
//               their weights the integers (2b - rem, 4b - rem, 2b + rem, rem) over 4b, each (float)((double)k / (double)(4b)):
//               ONE rounding.  A tent of radius two low-resolution pixels about the pixel's half-pixel centre; the integers sum to
//               8b; a tap replicated at a border keeps its own weight; 4b < 2^32 follows from 2 b n < 2^31.  At b = s n the
//               weights are the guided kernel's exact k / (4s).
//   Weights     gcfr_fullres_guided.hip's, in formula and order: k = guided_range (1 / (1 + d2 inv)), wt = (sy[j] sx[i]) k with the
//               product sy[j] sx[i] now ROUNDED, den the row-major sum from wt[0][0], rcp = 1.0f / den, wn = wt rcp.
//   Up_J        the row-major sum of wn a[tap], the first product starting it; all 16 taps are always read.
//   Composite   Up_J in all three places with the same wn, through gcfr_fullres.hpp's detail_of / fullres_value / fullres_byte
//               (the scalar path is its composite_pixel over a Guided16 filled from box_tap4); a pixel of the output window
//               outside the box is the photograph's byte for every light.  mask_u8 is low-resolution, in the box's frame.
//
// Work split: gcfr_fullres_box.hip's.  256 lanes own kQuadChunk consecutive pixels of ONE face's output window; the boxes travel by
// value in BoxArgs, 32 faces per launch.  ONCE per pixel: the taps, the 16 normalised weights (48 guide values, 16 divisions for k,
// one for rcp), d[3] and m.  PER LIGHT: 3 x 16 products and sums per pixel, the blend and the quantisation -- no division and no
// branch in the light loop; `m > 0` and inside-the-box are ONE byte mask formed once per lane.  A pixel outside the box computes on
// the box's nearest pixel (its coordinates are clamped: every address stays in range) and is masked away; a lane whose four pixels
// are all outside copies its three dwords L times and leaves.
// VEC (the window's width a multiple of four, out 4-byte aligned): lane t owns pixels 4 t .. 4 t + 3 of the chunk, all in one row:
// they share their four tap rows and sy.  The photograph's 12 bytes arrive as three dword loads that need no alignment, every
// light's 12 bytes leave as three dwords.  The four pixels' first taps lie within ceil(3 w / bw) <= 3 low-resolution columns of
// each other (their half-pixel positions are 3 w / bw apart), so per light, plane and tap row the lane loads ONE window of
// NW = MAXO + 4 consecutive columns, clamped to [0, w - 1] when loaded, through the plane's buffer descriptor (PlaneF32): 4 NW loads
// per plane instead of 64.  Pixel k's tap i is window column o[k] + i with o[k] = its first tap less pixel 0's, a value in
// 0 .. MAXO known only at run time: the tap is SELECTED among MAXO + 1 registers by the bits of o[k] (one v_cndmask per tap at
// MAXO = 1, five per two taps at MAXO = 3), never addressed.  MAXO is a template argument chosen per launch: 1 where every face has
// bw >= 3 w, else 3.  The NEXT light's windows are requested in front of the current light's arithmetic, as in
// gcfr_fullres_guided.hip; the registers allow one wave per SIMD.  Otherwise lane t owns pixels t, t + 256, t + 512, t + 768 and
// everything moves one element at a time: the same bytes.
#include <algorithm>

#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

// tap j of the four whose second is low-resolution index i0, clamped into an axis of n (n < 2^31)
__device__ inline uint32_t tap_clamp(uint32_t i0, int j, uint32_t n)
{
    const int32_t c = (int32_t)i0 - 1 + j;
    return c < 0 ? 0u : ((uint32_t)c < n - 1u ? (uint32_t)c : n - 1u);
}

// one axis of Up_J over a box: box-relative index i of a box axis of nb over a low-resolution axis of n (2 nb n < 2^31, so
// 4 nb < 2^32): i0 (the taps are tap_clamp(i0, 0..3, n)) and the four weights, each rounded once
__device__ inline void box_tap4(uint32_t i, uint32_t n, uint32_t nb, uint32_t &i0, float (&wgt)[4])
{
    const uint32_t a = (2u * i + 1u) * n;
    const uint32_t N = a > nb ? a - nb : 0u;
    const uint32_t den = 2u * nb;
    i0 = N / den;                                                                  // (<= n - 1)
    const uint32_t rem = N - i0 * den;
    const double q = (double)(2u * den);
    wgt[0] = (float)((double)(den - rem) / q), wgt[1] = (float)((double)(2u * den - rem) / q);
    wgt[2] = (float)((double)(den + rem) / q), wgt[3] = (float)((double)rem / q);
}

// A pointer that is the same in every active lane, said to be so.  The light loop's running pointer to a light's planes is uniform,
// but the compiler forms it in vector registers; the planes' buffer descriptors would then be vector values too, and every load
// through them a loop over their distinct values (one trip, some ten instructions per load).
__device__ inline const float *uniform_pointer(const float *p)
{
    const uint64_t a = (uint64_t)p;
    return reinterpret_cast<const float *>((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a) |
                                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32);
}

// WW, WN: the window's width and pixel count (paste: Wp, Hp Wp; else the faces' common bw, bh bw).  MAXO (VEC only; 0 otherwise):
// 1 or 3, every face of the launch has bw MAXO >= 3 w
template <bool VEC, int MAXO>
__global__ __launch_bounds__(kQuadLanes) void fullres_composites_box_guided_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t Wp, uint32_t HWp,
    uint32_t WW, uint32_t WN, uint32_t chunks, int32_t paste, float floor, float lo, float hi, float inv, BoxArgs boxes,
    uint8_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kQuadChunk);
    const int32_t bx0 = boxes.x0[b], by0 = boxes.y0[b], bw = boxes.bw[b], bh = boxes.bh[b];
    const int32_t ox = paste ? 0 : bx0, oy = paste ? 0 : by0;                      // the window's origin in the photograph
    const uint32_t hw = h * w;
    const FacePlanes f = face_planes(photo, x_lo, rendered, mask, out, b, mask_stride, L, hw, HWp, WN);
    if constexpr (VEC) {
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
        uint32_t y0, roff[4], c0[4];
        float sy[4], sx[4][4];
        box_tap4(ry, h, (uint32_t)bh, y0, sy);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            roff[j] = tap_clamp(y0, j, h) * w;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            box_tap4(rx[k], w, (uint32_t)bw, c0[k], sx[k]);
        // the lane's window of NW columns from pixel 0's first tap on; pixel k's taps start o[k] = c0[k] - c0[0] columns into it
        // (0 <= o[k] <= MAXO: rx is non-decreasing in k and rx[3] - rx[0] <= 3); its two bits select the tap
        constexpr int NW = MAXO + 4;
        uint32_t woff[4][NW];                                                      // BYTE offsets in a plane of `rendered`
        bool sa[4], sb[4];
#pragma unroll
        for (int e = 0; e < NW; ++e) {
            const uint32_t col = tap_clamp(c0[0], e, w);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                woff[j][e] = 4u * (roff[j] + col);                                 // (4 h w < 2^32: 2 bh h, 2 bw w < 2^31, bh >= h, bw >= w)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t o = c0[k] - c0[0];
            sa[k] = (o & 1u) != 0u;
            sb[k] = (o & 2u) != 0u;
        }
        // tap (j, i) of pixel k in a loaded window: selected among values, not addresses
        auto tap_of = [&](const float (&win)[4][NW], int k, int j, int i) {
            if (k == 0)                                                            // (compile time: o[0] = 0)
                return win[j][i];
            const float v0 = win[j][i], v1 = win[j][i + 1];                        // (two values, not a choice between addresses)
            const float a = sa[k] ? v1 : v0;
            if constexpr (MAXO == 1) {
                return a;
            } else {
                const float v2 = win[j][i + 2], v3 = win[j][i + 3];
                const float b = sa[k] ? v3 : v2;
                return sb[k] ? b : a;
            }
        };
        float p[4][3];
        quad_unpack_u8x3(w3, p);
        // once per pixel, from its own 16 taps of x_lo and the mask: the weights from the guide, then d and m
        float wn[4][16], d[3][4], m[4];
        bool relit[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t tap[16];
            float g[3][16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                tap[t] = roff[t / 4] + tap_clamp(c0[k], t % 4, w);
                const float *gp = f.x_lo + 3u * (size_t)tap[t];
                g[0][t] = gp[0], g[1][t] = gp[1], g[2][t] = gp[2];
            }
            float den = 0.0f;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                wn[k][t] = (sy[t / 4] * sx[k][t % 4]) * guided_range(p[k], g[0][t], g[1][t], g[2][t], inv);
                den = t == 0 ? wn[k][0] : den + wn[k][t];
            }
            const float rcp = 1.0f / den;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                wn[k][t] = wn[k][t] * rcp;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float acc = wn[k][0] * g[c][0];
#pragma unroll
                for (int t = 1; t < 16; ++t)
                    acc = acc + wn[k][t] * g[c][t];
                d[c][k] = detail_of(p[k][c], acc, floor, lo, hi);
            }
            float acc = wn[k][0] * mask_quotient_f32(f.mask[tap[0]]);
#pragma unroll
            for (int t = 1; t < 16; ++t)
                acc = acc + wn[k][t] * mask_quotient_f32(f.mask[tap[t]]);
            m[k] = acc;
            relit[k] = m[k] > 0.0f && in_x[k];
        }
        uint32_t keep[3];                                                          // relit ? the relit byte : the photograph's
        quad_select_mask(relit, keep);
        // a light's three windows; the NEXT light's are requested before this light's arithmetic, which then covers their way
        // from the cache (one trip past the end reloads the last light: in bounds, unused)
        auto load_light = [&](const float *re, float (&dst)[3][4][NW]) {
            const float *re_u = uniform_pointer(re);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const PlaneF32 plane(re_u + (size_t)c * hw, hw);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < NW; ++e)
                        dst[c][j][e] = plane.at(woff[j][e]);
            }
        };
        float cur[3][4][NW], nxt[3][4][NW];
        const float *re_l = f.rendered;                                            // (uniform) light l's three planes
        const size_t light_stride = 3u * (size_t)hw;
        load_light(re_l, cur);
        for (uint32_t l = 0; l < L; ++l) {
            re_l += l + 1u < L ? light_stride : 0u;
            load_light(re_l, nxt);
            __builtin_amdgcn_sched_barrier(0);                                     // (the loads stay in front of the arithmetic)
            float r[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float acc = wn[k][0] * tap_of(cur[c], k, 0, 0);
#pragma unroll
                    for (int t = 1; t < 16; ++t)
                        acc = acc + wn[k][t] * tap_of(cur[c], k, t / 4, t % 4);
                    r[c][k] = acc;
                }
            quad_store_selected(f.out + 3u * ((size_t)l * WN + q), w3, keep, [&](int k, int c) {
                return quantise_u8((double)fullres_value(p[k][c], m[k], d[c][k], r[c][k]));
            });
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < NW; ++e)
                        cur[c][j][e] = nxt[c][j][e];
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
            uint32_t y0, x0;
            float sy[4], sx[4];
            box_tap4(ry, h, (uint32_t)bh, y0, sy);
            box_tap4(rx, w, (uint32_t)bw, x0, sx);
            Guided16 up;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                up.tap[t] = tap_clamp(y0, t / 4, h) * w + tap_clamp(x0, t % 4, w);
            const float p[3] = {(float)pb[0], (float)pb[1], (float)pb[2]};
            float den = 0.0f;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float *g = f.x_lo + 3u * (size_t)up.tap[t];
                up.wn[t] = (sy[t / 4] * sx[t % 4]) * guided_range(p, g[0], g[1], g[2], inv);
                den = t == 0 ? up.wn[0] : den + up.wn[t];
            }
            const float rcp = 1.0f / den;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                up.wn[t] = up.wn[t] * rcp;
            composite_pixel(up, pb, f, L, hw, WN, px_w, floor, lo, hi);
        }
    }
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_fullres_composites_box_guided_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered,
                                                     const uint8_t *mask_u8, int32_t mask_batch, int32_t B, int32_t L, int32_t Hp,
                                                     int32_t Wp, const int32_t *boxes, int32_t h, int32_t w, int32_t paste, float floor,
                                                     float detail_clamp, float range_sigma, uint8_t *out_u8, void *stream)
{
    uint32_t HWp, hw, mask_stride;
    float lo;
    if (!boxes || (paste != 0 && paste != 1) || !(range_sigma > 0.0f) || !box_shape(B, Hp, Wp, h, w, HWp, hw) ||
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
    const float inv = 1.0f / (range_sigma * range_sigma);                          // +inf -> 0: the spatial tent alone
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        const dim3 grid((uint32_t)n * chunks);
        const BoxArgs args = box_args(boxes + 4 * b0, n);
        const uint8_t *ph = photo_u8 + (size_t)b0 * 3u * HWp;
        const float *xl = x_lo + (size_t)b0 * 3u * hw, *re = rendered + (size_t)b0 * (size_t)L * 3u * hw;
        const uint8_t *mk = mask_u8 + (size_t)b0 * mask_stride;
        uint8_t *o = out_u8 + (size_t)b0 * (size_t)L * 3u * WN;
        // the window's class: 1 where bw >= 3 w for every face of this launch, else 3 (bw >= w)
        int maxo = 0;
        for (int32_t b = b0; vec && b < b0 + n; ++b)
            maxo = std::max(maxo, (int64_t)boxes[4 * b + 2] >= 3 * (int64_t)w ? 1 : 3);
        auto launch = [&](auto V, auto M) {
            hipLaunchKernelGGL((fullres_composites_box_guided_kernel<decltype(V)::value, decltype(M)::value>), grid, dim3(kQuadLanes),
                               0, st, ph, xl, re, mk, mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, WW, WN,
                               chunks, paste, floor, lo, detail_clamp, inv, args, o);
        };
        switch (maxo) {
        case 0: launch(std::false_type{}, std::integral_constant<int, 0>{}); break;
        case 1: launch(std::true_type{}, std::integral_constant<int, 1>{}); break;
        default: launch(std::true_type{}, std::integral_constant<int, 3>{}); break;
        }
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
