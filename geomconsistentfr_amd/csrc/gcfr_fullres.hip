// Full-resolution relighting, gfx950: the two ends of the inference path around the network's resolution (h, w).
//   ingest      the uint8 photograph (B, s h, s w, 3) -> the network's f32 input (B, h, w, 3): the mean of each s x s block / 255
//   composite   the relit low-resolution `rendered` (B,L,3,h,w) of ONE pass carried back onto the photograph's own pixels by
//               quotient / detail transfer -> (B, L, s h, s w, 3) uint8, ONE launch for all L lights
// s is 1, 2, 4 or 8: every bilinear weight is a multiple of 1 / (2 s), exact in f32.
//
// Arithmetic (the library is built with -ffp-contract=off: every operation below is one separately rounded IEEE f32 operation
// unless marked f64; max / min are fmaxf / fminf, which return the other operand for a NaN).
//   Ingest      x_lo[b,i,j,c] = (float)((double)S / (255.0 s s)), S the integer sum of the block's s s bytes (exact); the division
//               is f64, rounded once to f32.  At s = 1 this is np.float32(img / 255.0).
//   Up(a)       bilinear, half-pixel centres.  Per axis and hi-res index y: fy = max((y + 0.5) / s - 0.5, 0), y0 = floor(fy),
//               t = fy - y0, y1 = min(y0 + 1, n - 1); all exact, and formed here in integers: 2 s fy = max(2 y + 1 - s, 0).
//               Horizontal first on both rows, a0 + tx (a1 - a0); then top + ty (bot - top).  This form returns a constant field
//               exactly.  Both taps are always read: a tap of weight 0 still carries a NaN or an infinity into its pixel.
//   Composite   per hi-res pixel, light l and channel c:
//     p  = (float)photo_u8
//     xl = Up(x_lo[..., c]) 255.0f
//     d  = min(max(p / max(xl, floor), 1.0f / detail_clamp), detail_clamp)
//     m  = Up((float)mask_u8 / 255.0f)
//     r  = Up(rendered[b, l, c]) 255.0f
//     v  = p + m (r d - p)
//     byte = m > 0 ? quantise_u8((double)v) : photo_u8          (gcfr_composite.hpp: rint, saturate, NaN -> 0)
//
// Work split of the composite: a workgroup of 256 lanes owns kQuadChunk = 1024 consecutive hi-res pixels of ONE face, four per lane
// (gcfr_reduce.hpp).  A lane loads the photograph's bytes, forms d[3][4] and m[4] ONCE, then walks the L lights: per light only the
// low-resolution taps of `rendered` are fetched -- each is shared by s s hi-res pixels and comes from cache -- and 12 bytes are
// stored; the `m > 0` select is a byte mask formed once per lane and applied to the three dwords of every light
// (gcfr_fullres.hpp: quad_select_mask / quad_store_selected).  A light's 6 kWin<S> taps are requested together, in front of its
// arithmetic.  The photograph, x_lo and the mask are read once per pixel, not once per light.
// VEC (W a multiple of four, photograph and output 4-byte aligned): lane t owns pixels 4 t .. 4 t + 3 of the chunk, all in one row;
// the photograph's 12 bytes arrive as three dwords and every light's 12 bytes leave as three.  The four pixels share their two rows
// and a WINDOW of kWin<S> consecutive low-resolution columns that starts at cb = floor((x + 0.5) / s - 0.5) of the first pixel
// (-1 at the left border; columns are clamped to [0, w - 1] when loaded): pixel k's left tap is window column kP0<S>(k), a
// compile-time constant, and its right tap the next one.  Only a pixel whose fy was clamped to 0 at the left border (2 x + 1 < s)
// differs: its taps are columns 0 and min(1, w - 1), the latter one window column further right.  2 x kWin loads per plane instead
// of 16.  Otherwise lane t owns pixels t, t + 256, t + 512, t + 768 and everything moves one element at a time: the same bytes
// (gcfr_fullres.hpp: composite_pixel over a Bilinear4 filled from up_tap<S>).
// Bytes per hi-res pixel: 3 read, 3 L written; the low-resolution planes (x_lo 12, mask 1, rendered 12 L per low-res pixel) once
// from memory.
#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

// the window of the vector path: pixel k's left tap is column kP0<S>(k) (gcfr_fullres.hpp) of a window this wide
template <int S>
constexpr int kWin() { return S == 1 ? 5 : S == 2 ? 4 : 3; }

// one axis of Up for hi-res index i of a low-resolution axis of n: the two taps and the weight of the second, all exact
template <int S>
__device__ inline void up_tap(uint32_t i, uint32_t n, uint32_t &i0, uint32_t &i1, float &t)
{
    const uint32_t u2 = 2u * i + 1u;                                               // (i < 2^31)
    const uint32_t u = u2 < (uint32_t)S ? 0u : u2 - (uint32_t)S;                   // 2 s fy
    i0 = u >> (log2_of<S>() + 1);
    t = (float)(u & (2u * S - 1u)) * (1.0f / (float)(2 * S));
    i1 = i0 + 1u < n ? i0 + 1u : n - 1u;
}

template <int S, bool VEC>
__global__ __launch_bounds__(kQuadLanes) void fullres_composites_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t W, uint32_t HW,
    uint32_t chunks, float floor, float lo, float hi, uint8_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kQuadChunk);
    const uint32_t hw = h * w;
    const FacePlanes f = face_planes(photo, x_lo, rendered, mask, out, b, mask_stride, L, hw, HW, HW);
    if (VEC) {
        if (q >= HW)                                                               // all four pixels in range or none
            return;
        const uint32_t y = q / W, x = q - y * W;
        uint32_t y0, y1, roff[2];
        float ty;
        up_tap<S>(y, h, y0, y1, ty);
        roff[0] = y0 * w, roff[1] = y1 * w;
        constexpr int NW = kWin<S>();
        const bool left = 2u * x + 1u < (uint32_t)S;                               // the window starts at column -1
        uint32_t col[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            uint32_t c = left ? (i == 0 ? 0u : (uint32_t)i - 1u) : ((2u * x + 1u - (uint32_t)S) >> (log2_of<S>() + 1)) + (uint32_t)i;
            col[i] = c < w - 1u ? c : w - 1u;
        }
        float tx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t x0, x1;
            up_tap<S>(x + (uint32_t)k, w, x0, x1, tx[k]);
        }
        // Up of one plane at the lane's four pixels, from a loaded window win[row][column]
        auto up4 = [&](const float (&win)[2][NW], float (&v)[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p0 = kP0<S>(k);
                float a01 = win[0][p0 + 1], a11 = win[1][p0 + 1];
                if (2 * k + 1 < S) {                                               // (compile time) clamped exactly in the lane at the
                    a01 = left ? win[0][p0 + 2] : a01;                             // left border: x is a multiple of four, so
                    a11 = left ? win[1][p0 + 2] : a11;                             // 2 (x + k) + 1 < S means x = 0
                }
                v[k] = bilerp(win[0][p0], a01, win[1][p0], a11, tx[k], ty);
            }
        };
        // the photograph's 12 bytes
        const uint32_t *pw = reinterpret_cast<const uint32_t *>(f.photo + 3u * (size_t)q);
        const uint32_t w3[3] = {pw[0], pw[1], pw[2]};
        float p[4][3];
        quad_unpack_u8x3(w3, p);
        // the windows of one light's three planes
        auto load_light = [&](uint32_t l, float (&dst)[3][2][NW]) {
            const float *re_l = f.rendered + (size_t)l * 3u * hw;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int i = 0; i < NW; ++i)
                        dst[c][r][i] = re_l[(size_t)c * hw + roff[r] + col[i]];
        };
        float cur[3][2][NW];
        float win[2][NW], d[3][4], m[4], v[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < NW; ++i)
                    win[r][i] = f.x_lo[3u * (size_t)(roff[r] + col[i]) + c];
            up4(win, v);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                d[c][k] = detail_of(p[k][c], v[k], floor, lo, hi);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < NW; ++i)
                win[r][i] = mask_quotient_f32(f.mask[roff[r] + col[i]]);
        up4(win, m);
        const bool relit[4] = {m[0] > 0.0f, m[1] > 0.0f, m[2] > 0.0f, m[3] > 0.0f};
        uint32_t inside[3];                                                        // m > 0 ? the relit byte : the photograph's
        quad_select_mask(relit, inside);
        for (uint32_t l = 0; l < L; ++l) {
            load_light(l, cur);
            float r[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                up4(cur[c], r[c]);
            quad_store_selected(f.out + 3u * ((size_t)l * HW + q), w3, inside, [&](int k, int c) {
                return quantise_u8((double)fullres_value(p[k][c], m[k], d[c][k], r[c][k]));
            });
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const uint32_t px = quad_pixel<false>(q, k);
            if (px >= HW)
                continue;
            const uint32_t y = px / W, x = px - y * W;
            uint32_t y0, y1, x0, x1;
            float ty, tx;
            up_tap<S>(y, h, y0, y1, ty);
            up_tap<S>(x, w, x0, x1, tx);
            const uint8_t *pp = f.photo + 3u * (size_t)px;
            const uint8_t pb[3] = {pp[0], pp[1], pp[2]};
            composite_pixel(Bilinear4(y0, y1, x0, x1, w, tx, ty), pb, f, L, hw, HW, px, floor, lo, hi);
        }
    }
}

// Ingest: a workgroup owns kQuadChunk consecutive LOW-resolution pixels of one face, four per lane.  VEC (w a multiple of four, the
// photograph 4-byte aligned, x_lo 16-byte aligned): the lane's four pixels are consecutive in one row; each of the s photograph rows
// under them is 12 s consecutive bytes, read as 3 s dwords, and the 12 floats leave in three 16-byte stores.
template <int S, bool VEC>
__global__ __launch_bounds__(kQuadLanes) void ingest_photographs_kernel(const uint8_t *__restrict__ photo, uint32_t w, uint32_t hw,
                                                                        uint32_t chunks, float *__restrict__ x_lo)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kQuadChunk);
    const size_t W = (size_t)w * S;
    const uint8_t *ph_b = photo + (size_t)b * 3u * hw * (size_t)(S * S);
    float *xl_b = x_lo + (size_t)b * 3u * hw;
    const double den = 255.0 * (double)S * (double)S;
    if (VEC) {
        if (q >= hw)
            return;
        const uint32_t y = q / w, x = q - y * w;
        uint32_t acc[4][3] = {};
        for (int r = 0; r < S; ++r) {
            const uint32_t *row = reinterpret_cast<const uint32_t *>(ph_b + 3u * (((size_t)y * S + r) * W + (size_t)x * S));
#pragma unroll
            for (int dw = 0; dw < 3 * S; ++dw) {
                const uint32_t word = row[dw];
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    const int i = 4 * dw + bb;
                    acc[(i / 3) / S][i % 3] += (word >> (8 * bb)) & 0xffu;
                }
            }
        }
        float f[12];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                f[3 * k + c] = (float)((double)acc[k][c] / den);
        float4 *o = reinterpret_cast<float4 *>(xl_b + 3u * (size_t)q);
        o[0] = make_float4(f[0], f[1], f[2], f[3]), o[1] = make_float4(f[4], f[5], f[6], f[7]);
        o[2] = make_float4(f[8], f[9], f[10], f[11]);
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const uint32_t px = quad_pixel<false>(q, k);
            if (px >= hw)
                continue;
            const uint32_t y = px / w, x = px - y * w;
            uint32_t acc[3] = {0u, 0u, 0u};
            for (int r = 0; r < S; ++r) {
                const uint8_t *row = ph_b + 3u * (((size_t)y * S + r) * W + (size_t)x * S);
#pragma unroll
                for (int i = 0; i < 3 * S; ++i)
                    acc[i % 3] += row[i];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                xl_b[3u * (size_t)px + c] = (float)((double)acc[c] / den);
        }
    }
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_ingest_photographs_u8(const uint8_t *photo_u8, int32_t B, int32_t h, int32_t w, int32_t s, float *x_lo_out,
                                          void *stream)
{
    uint32_t HW, hw;
    if (!photo_u8 || !x_lo_out || (const void *)photo_u8 == (const void *)x_lo_out || !fullres_shape(B, h, w, s, HW, hw))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (hw + kQuadChunk - 1) / kQuadChunk;
    const bool vec = (uint32_t)w % 4u == 0 && aligned4(photo_u8) && aligned16(x_lo_out);
    const dim3 grid((uint32_t)B * chunks);
    hipStream_t st = (hipStream_t)stream;
    with_scale(s, [&](auto S) {
        with_flag(vec, [&](auto V) {
            hipLaunchKernelGGL((ingest_photographs_kernel<decltype(S)::value, decltype(V)::value>), grid, dim3(kQuadLanes), 0, st,
                               photo_u8, (uint32_t)w, hw, chunks, x_lo_out);
        });
    });
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_fullres_composites_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                          int32_t mask_batch, int32_t B, int32_t L, int32_t h, int32_t w, int32_t s, float floor,
                                          float detail_clamp, uint8_t *out_u8, void *stream)
{
    uint32_t HW, hw, mask_stride;
    float lo;
    if (!fullres_shape(B, h, w, s, HW, hw) ||
        !fullres_operands(photo_u8, x_lo, rendered, mask_u8, out_u8, L, mask_batch, B, hw, detail_clamp, floor, mask_stride, lo) ||
        out_u8 == photo_u8)
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (HW + kQuadChunk - 1) / kQuadChunk, W = (uint32_t)w * (uint32_t)s;
    const bool vec = W % 4u == 0 && aligned4(photo_u8) && aligned4(out_u8);
    const dim3 grid((uint32_t)B * chunks);
    hipStream_t st = (hipStream_t)stream;
    with_scale(s, [&](auto S) {
        with_flag(vec, [&](auto V) {
            hipLaunchKernelGGL((fullres_composites_kernel<decltype(S)::value, decltype(V)::value>), grid, dim3(kQuadLanes), 0, st,
                               photo_u8, x_lo, rendered, mask_u8, mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, W, HW, chunks,
                               floor, lo, detail_clamp, out_u8);
        });
    });
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
