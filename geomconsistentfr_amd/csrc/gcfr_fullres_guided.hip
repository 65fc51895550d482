// Full-resolution relighting, gfx950: the composite of gcfr_fullres.hip with an EDGE-AWARE (joint-bilateral) upsample Up_J in
// place of the bilinear Up, guided by the photograph itself.  Same operands, layouts and limits as gcfr_fullres_composites_u8,
// plus `range_sigma` (grey levels).  s is 1, 2, 4 or 8.
//
// Arithmetic (-ffp-contract=off: every operation below is one separately rounded IEEE f32 operation unless marked f64; max / min
// are fmaxf / fminf; the divisions are the correctly rounded f32 division).
//   Taps        per axis and hi-res index y of a low-resolution axis of n, in integers: u = max(2 y + 1 - s, 0), y0 = u div 2 s,
//               r = u mod 2 s (Up's u and y0).  The four taps are clamp(y0 - 1 + j, 0, n - 1), j = 0..3, with the integer weights
//               (2 s - r, 4 s - r, 2 s + r, r) over 4 s: a tent of radius two low-resolution pixels.  The four sum to 2 and each
//               is exact in f32, sy[j], sx[i]; sy[j] sx[i] is exact.  A tap replicated at a border keeps its own weight.
//   Weights     once per hi-res pixel P, the same for every light.  p[c] = (float)photo_u8[P, c]; for tap (j, i) at low-resolution
//               pixel q, g[c] = x_lo[q, c] 255.0f:
//                 e[c] = p[c] - g[c];  d2 = (e[0] e[0] + e[1] e[1]) + e[2] e[2];  k = 1.0f / (1.0f + d2 inv)
//                 wt = (sy[j] sx[i]) k;  den = the sum of the 16 wt, row-major (j outer, i inner) from wt[0][0];  rcp = 1.0f / den
//                 wn = wt rcp
//               inv = 1.0f / (range_sigma range_sigma) is formed once on the host in f32.  k is a Lorentzian: no transcendental.
//   Up_J(a)(P)  the sum over the 16 taps, row-major, of wn[j][i] a[tap]: the first product starts the sum, every product and sum
//               is rounded.  All 16 taps are always read: a tap of weight 0 still carries a NaN.
//   Composite   gcfr_fullres.hip's with Up_J in all three places and the SAME wn: d = detail_of(p, Up_J(x_lo[..., c])),
//               m = Up_J((float)mask_u8 / 255.0f), v = fullres_value(p, m, d, Up_J(rendered[b, l, c])),
//               byte = m > 0 ? quantise_u8((double)v) : photo_u8   (gcfr_fullres.hpp, gcfr_composite.hpp: called, not copied;
//               the scalar path is gcfr_fullres.hpp's composite_pixel over a Guided16, the vector path's 12 bytes go through its
//               quad_select_mask / quad_store_selected)
//
// Work split: gcfr_fullres.hip's.  A workgroup of 256 lanes owns kQuadChunk = 1024 consecutive hi-res pixels of ONE face, four per
// lane.  ONCE per pixel: the 16 normalised weights (48 guide values, 16 divisions for k and one for rcp), d[3] and m.  PER LIGHT:
// 3 x 16 products and sums per pixel, the blend and the quantisation -- no division and no branch in the light loop; the `m > 0`
// select is a byte mask formed once per lane.  The registers allow one wave per SIMD (two at s = 8), so nothing but the lane's own
// arithmetic covers a load: the NEXT light's windows are requested in front of the current light's arithmetic.
// VEC (W a multiple of four, photograph and output 4-byte aligned): lane t owns pixels 4 t .. 4 t + 3 of the chunk, all in one row;
// the photograph's 12 bytes arrive as three dwords and every light's 12 bytes leave as three.  The four pixels share their four tap
// rows and a WINDOW of kGWin<S> consecutive low-resolution columns, loaded once per lane, plane and row (4 x kGWin loads per plane
// instead of 64) and clamped to [0, w - 1] when loaded.  The window starts at x0 - 1 of the first pixel; pixel k's first tap is
// window column kP0<S>(k).  Only at the left border (x = 0 and s > 1, where u was clamped to 0 for the pixels with 2 k + 1 < s)
// does this differ: at s = 8 all four pixels are clamped and the window simply starts at -1; at s = 2 and 4 the window starts at
// -2 and the clamped pixels read one window column further right.  Otherwise lane t owns pixels t, t + 256, t + 512, t + 768 and
// everything moves one element at a time: the same bytes.
#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

// the window's width: the last pixel's offset plus its four taps
template <int S>
constexpr int kGWin() { return kP0<S>(3) + 4; }

// one axis of Up_J for hi-res index i of a low-resolution axis of n: the four taps and their weights, all exact
template <int S>
__device__ inline void guided_tap(uint32_t i, uint32_t n, uint32_t (&tap)[4], float (&wgt)[4])
{
    const uint32_t u2 = 2u * i + 1u;                                               // (i < 2^31)
    const uint32_t u = u2 < (uint32_t)S ? 0u : u2 - (uint32_t)S;
    const int32_t i0 = (int32_t)(u >> (log2_of<S>() + 1));
    const uint32_t r = u & (2u * S - 1u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t c = i0 - 1 + j;                                              // (n < 2^31)
        tap[j] = c < 0 ? 0u : ((uint32_t)c < n - 1u ? (uint32_t)c : n - 1u);
    }
    constexpr float q = 1.0f / (float)(4 * S);
    wgt[0] = (float)(2u * S - r) * q, wgt[1] = (float)(4u * S - r) * q, wgt[2] = (float)(2u * S + r) * q, wgt[3] = (float)r * q;
}

template <int S, bool VEC>
__global__ __launch_bounds__(kQuadLanes) void fullres_composites_guided_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t W, uint32_t HW,
    uint32_t chunks, float floor, float lo, float hi, float inv, uint8_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kQuadChunk);
    const uint32_t hw = h * w;
    const FacePlanes f = face_planes(photo, x_lo, rendered, mask, out, b, mask_stride, L, hw, HW, HW);
    if (VEC) {
        if (q >= HW)                                                               // all four pixels in range or none
            return;
        const uint32_t y = q / W, x = q - y * W;
        uint32_t ty[4], roff[4], unused[4];
        float sy[4];
        guided_tap<S>(y, h, ty, sy);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            roff[j] = ty[j] * w;
        constexpr int NW = kGWin<S>();
        constexpr bool kShift = S == 2 || S == 4;                                  // clamped pixels beside unclamped ones in a lane
        const bool left = 2u * x + 1u < (uint32_t)S;                               // x = 0 and s > 1
        const int32_t cb = left ? (kShift ? -2 : -1) : (int32_t)((2u * x + 1u - (uint32_t)S) >> (log2_of<S>() + 1)) - 1;
        uint32_t col[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int32_t c = cb + i;
            col[i] = c < 0 ? 0u : ((uint32_t)c < w - 1u ? (uint32_t)c : w - 1u);
        }
        // tap (j, i) of pixel k in a loaded window win[row][column]
        auto tap_of = [&](const float (&win)[4][NW], int k, int j, int i) {
            const int c = kP0<S>(k) + i;
            const float here = win[j][c];
            if (kShift && 2 * k + 1 < S) {                                         // (compile time)
                const float right = win[j][c + 1];                                 // two values, not a choice between two addresses
                return left ? right : here;
            }
            return here;
        };
        // the photograph's 12 bytes
        const uint32_t *pw = reinterpret_cast<const uint32_t *>(f.photo + 3u * (size_t)q);
        const uint32_t w3[3] = {pw[0], pw[1], pw[2]};
        float p[4][3];
        quad_unpack_u8x3(w3, p);
        // Up_J of one plane at the lane's four pixels
        float wn[4][16];
        auto up4 = [&](const float (&win)[4][NW], float (&v)[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float acc = wn[k][0] * tap_of(win, k, 0, 0);
#pragma unroll
                for (int t = 1; t < 16; ++t)
                    acc = acc + wn[k][t] * tap_of(win, k, t / 4, t % 4);
                v[k] = acc;
            }
        };
        // once per pixel: the weights from the guide, then d and m
        float d[3][4], m[4], v[4];
        {
            float xw[3][4][NW];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < NW; ++i)
                        xw[c][j][i] = f.x_lo[3u * (size_t)(roff[j] + col[i]) + c];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float sx[4];
                guided_tap<S>(x + (uint32_t)k, w, unused, sx);
                float den = 0.0f;
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int j = t / 4, i = t % 4;
                    const float kr = guided_range(p[k], tap_of(xw[0], k, j, i), tap_of(xw[1], k, j, i), tap_of(xw[2], k, j, i), inv);
                    wn[k][t] = (sy[j] * sx[i]) * kr;
                    den = t == 0 ? wn[k][0] : den + wn[k][t];
                }
                const float rcp = 1.0f / den;
#pragma unroll
                for (int t = 0; t < 16; ++t)
                    wn[k][t] = wn[k][t] * rcp;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                up4(xw[c], v);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    d[c][k] = detail_of(p[k][c], v[k], floor, lo, hi);
            }
            float mw[4][NW];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < NW; ++i)
                    mw[j][i] = mask_quotient_f32(f.mask[roff[j] + col[i]]);
            up4(mw, m);
        }
        const bool relit[4] = {m[0] > 0.0f, m[1] > 0.0f, m[2] > 0.0f, m[3] > 0.0f};
        uint32_t inside[3];                                                        // m > 0 ? the relit byte : the photograph's
        quad_select_mask(relit, inside);
        // a light's three windows; the NEXT light's are requested before this light's arithmetic, which then covers their way
        // from the cache (one trip past the end reloads the last light: in bounds, unused)
        auto load_light = [&](uint32_t l, float (&dst)[3][4][NW]) {
            const float *re_l = f.rendered + (size_t)l * 3u * hw;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < NW; ++i)
                        dst[c][j][i] = re_l[(size_t)c * hw + roff[j] + col[i]];
        };
        float cur[3][4][NW], nxt[3][4][NW];
        load_light(0u, cur);
        for (uint32_t l = 0; l < L; ++l) {
            load_light(l + 1u < L ? l + 1u : l, nxt);
            __builtin_amdgcn_sched_barrier(0);                                     // (the loads stay in front of the arithmetic)
            float r[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                up4(cur[c], r[c]);
            quad_store_selected(f.out + 3u * ((size_t)l * HW + q), w3, inside, [&](int k, int c) {
                return quantise_u8((double)fullres_value(p[k][c], m[k], d[c][k], r[c][k]));
            });
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < NW; ++i)
                        cur[c][j][i] = nxt[c][j][i];
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const uint32_t px = quad_pixel<false>(q, k);
            if (px >= HW)
                continue;
            const uint32_t y = px / W, x = px - y * W;
            uint32_t ty[4], tx[4];
            float sy[4], sx[4];
            guided_tap<S>(y, h, ty, sy);
            guided_tap<S>(x, w, tx, sx);
            Guided16 up;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                up.tap[t] = ty[t / 4] * w + tx[t % 4];
            const uint8_t *pp = f.photo + 3u * (size_t)px;
            const uint8_t pb[3] = {pp[0], pp[1], pp[2]};
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
            composite_pixel(up, pb, f, L, hw, HW, px, floor, lo, hi);
        }
    }
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_fullres_composites_guided_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered,
                                                 const uint8_t *mask_u8, int32_t mask_batch, int32_t B, int32_t L, int32_t h, int32_t w,
                                                 int32_t s, float floor, float detail_clamp, float range_sigma, uint8_t *out_u8,
                                                 void *stream)
{
    uint32_t HW, hw, mask_stride;
    float lo;
    if (!fullres_shape(B, h, w, s, HW, hw) ||
        !fullres_operands(photo_u8, x_lo, rendered, mask_u8, out_u8, L, mask_batch, B, hw, detail_clamp, floor, mask_stride, lo) ||
        out_u8 == photo_u8 || !(range_sigma > 0.0f))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (HW + kQuadChunk - 1) / kQuadChunk, W = (uint32_t)w * (uint32_t)s;
    const bool vec = W % 4u == 0 && aligned4(photo_u8) && aligned4(out_u8);
    const float inv = 1.0f / (range_sigma * range_sigma);                          // +inf -> 0: the spatial tent alone
    const dim3 grid((uint32_t)B * chunks);
    hipStream_t st = (hipStream_t)stream;
    with_scale(s, [&](auto S) {
        with_flag(vec, [&](auto V) {
            hipLaunchKernelGGL((fullres_composites_guided_kernel<decltype(S)::value, decltype(V)::value>), grid, dim3(kQuadLanes), 0,
                               st, photo_u8, x_lo, rendered, mask_u8, mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, W, HW,
                               chunks, floor, lo, detail_clamp, inv, out_u8);
        });
    });
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
