// Full-resolution relighting of a ROTATED face, gfx950: gcfr_fullres_box.hip's two ends for a face under a 2 x 3 affine map -- what a
// face aligner reports -- in the place of an axis-aligned box.
//   ingest      the uint8 photograph sampled through F (network -> photograph) -> the network's f32 input (B, h, w, 3)
//   composite   the relit low-resolution `rendered` (B,L,3,h,w) of ONE pass carried through I (photograph -> network) onto the
//               photograph's own pixels -> (B,L,Hp,Wp,3), the photograph relit where a pixel's centre lands in the network square
//               and untouched elsewhere, ONE launch for all L lights
// include/gcfr.h is the statement.  All geometry is INTEGER, fixed point with 14 fractional bits (ONE = 2^14): no float decides a tap
// or a weight, and every value is rounded once.
//
// Arithmetic (built with -ffp-contract=off: every operation is one separately rounded IEEE operation).
//   K(M)        sub-samples per axis of a destination pixel: the smallest of 1, 2, 4, 8 with K^2 ONE^2 >= the longer column of M
//               squared (the host decides; uniform per face).  den = 2 K ONE, a power of two: every div is a shift, every rem a mask.
//   P           sub-sample (a, b) of destination pixel (x, y): P0 = M00 (2Kx + 2a + 1) + M01 (2Ky + 2b + 1) + 2K M02 - K ONE, P1 with
//               row 1, in units of 1 / den (64 bits).  The multiplications are done once per pixel; neighbours and sub-samples are
//               reached by additions.
//   Ingest      per sub-sample x0 = floor(P0 / den), fx = P0 - x0 den; taps x0, x0 + 1 CLAMPED into the photograph with weights
//               den - fx, fx; rows likewise.  S = sum wy wx byte < 2^53; x_lo = (float)((double)S / (255.0 K K den den)).
//   Carrier     per sub-sample U = max(P0, 0), j0 = min(U div den, w - 1), fu = U mod den, j1 = min(j0 + 1, w - 1),
//               tx = (float)fu / den (exact); rows likewise; the value is gcfr_fullres.hpp's bilerp.  K > 1: the f64 sum of the K K
//               values from +0.0, b outer and a inner, over (double)(K K), rounded to f32.
//   Composite   where c0 = I00 (2x+1) + I01 (2y+1) + 2 I02 lies in [0, 2 ONE w) and c1 in [0, 2 ONE h): gcfr_fullres.hip's p, xl, d,
//               m, r, v and byte through the SAME device functions; every other pixel is the photograph's byte for every light.
//
// The matrices arrive in a HOST array, are validated on the host and travel BY VALUE in the kernel's argument block (AffineArgs: up
// to kBoxFaces faces per launch; more faces are a short loop of launches): nothing is uploaded, no device scratch, capture-safe.
//
// Work split of the composite (gcfr_fullres_box.hip's): a workgroup of 256 lanes owns kQuadChunk consecutive pixels of ONE face's
// copy of the photograph, so K is uniform over a workgroup and is BRANCHED on.  A workgroup whose rows all lie outside the rows the
// face's quad can reach (AffineArgs::y_lo / y_hi, a superset the host computes) copies without any 64-bit work.  Otherwise a lane
// forms the inside test, the taps, d and m ONCE, then walks the L lights.  VEC (Wp a multiple of four, out 4-byte aligned): a lane's
// four pixels lie in one row, the photograph's 12 bytes arrive as three dword loads and every light's leave as three dword stores; a
// lane whose four pixels all fail the inside test copies its three dwords L times.  With K = 1 (and 4 h w < 2^32) the light loop is
// gcfr_fullres_box.hip's: 48 taps behind buffer descriptors, requested together.  With K > 1 the sub-samples are walked by run-time
// loops that recompute the taps from the indices: no per-lane array is indexed dynamically, no scratch, no LDS.
#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"
#include "gcfr_fullres_affine.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

// buf: 4 h w < 2^32, so that a tap's byte offset in a plane of `rendered` fits a buffer load's 32-bit offset
template <bool VEC>
__global__ __launch_bounds__(kQuadLanes) void affine_composites_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t Wp, uint32_t HWp,
    uint32_t chunks, int32_t buf, float floor, float lo, float hi, AffineArgs maps, uint8_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q0 = ch * (uint32_t)kQuadChunk;
    const uint32_t q = quad_first<VEC>(q0);
    const uint32_t hw = h * w;
    const FacePlanes f = face_planes(photo, x_lo, rendered, mask, out, b, mask_stride, L, hw, HWp, HWp);
    // (uniform) the chunk's rows against the rows the face can reach
    const uint32_t q_last = q0 + (uint32_t)kQuadChunk - 1u < HWp ? q0 + (uint32_t)kQuadChunk - 1u : HWp - 1u;
    const bool reach = (int32_t)(q_last / Wp) >= maps.y_lo[b] && (int32_t)(q0 / Wp) < maps.y_hi[b];
    const AffineMap M(maps, b);
    const uint64_t lim0 = (uint64_t)(2 * kAffineOne) * w, lim1 = (uint64_t)(2 * kAffineOne) * h;
    if (VEC) {
        if (q >= HWp)                                                              // all four pixels in range or none
            return;
        const uint8_t *pp = f.photo + 3u * (size_t)q;
        const uint32_t w3[3] = {load_dword_any(pp), load_dword_any(pp + 4), load_dword_any(pp + 8)};
        bool in[4] = {false, false, false, false}, any = false;
        const uint32_t py = q / Wp, px = q - py * Wp;
        int64_t c0 = 0, c1 = 0;
        if (reach) {
            c0 = M.m00 * (int64_t)(2u * (uint64_t)px + 1u) + M.m01 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m02;
            c1 = M.m10 * (int64_t)(2u * (uint64_t)px + 1u) + M.m11 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m12;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                in[k] = affine_inside(c0 + 2 * k * M.m00, c1 + 2 * k * M.m10, lim0, lim1);
                any = any || in[k];
            }
        }
        if (!any) {                                                                // the photograph's bytes for every light
            for (uint32_t l = 0; l < L; ++l) {
                uint32_t *ow = reinterpret_cast<uint32_t *>(f.out + 3u * ((size_t)l * HWp + q));
                ow[0] = w3[0], ow[1] = w3[1], ow[2] = w3[2];
            }
            return;
        }
        int64_t P0, P1;
        M.origin(px, py, P0, P1);
        const int64_t dx0 = 2 * M.m00 * (int64_t)M.K(), dx1 = 2 * M.m10 * (int64_t)M.K();  // (uniform) P's step of one pixel in x
        AffineCarrier up[4];
        float p[4][3];
        quad_unpack_u8x3(w3, p);
        float d[3][4], m[4];
        bool relit[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            up[k] = AffineCarrier(M, P0 + k * dx0, P1 + k * dx1, h, w);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[c][k] = detail_of(p[k][c], up[k]([&](uint32_t t) { return f.x_lo[3u * (size_t)t + c]; }), floor, lo, hi);
            m[k] = up[k]([&](uint32_t t) { return mask_quotient_f32(f.mask[t]); });
            relit[k] = m[k] > 0.0f && in[k];
        }
        uint32_t keep[3];                                                          // relit ? the relit byte : the photograph's
        quad_select_mask(relit, keep);
        if (M.lk == 0u && buf) {
            // gcfr_fullres_box.hip's light loop: the taps' BYTE offsets in a plane of `rendered`, a light's 48 taps requested together
            uint32_t off[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                off[k][0] = 4u * up[k].t00, off[k][1] = 4u * up[k].t01, off[k][2] = 4u * up[k].t10, off[k][3] = 4u * up[k].t11;
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
                quad_store_selected(f.out + 3u * ((size_t)l * HWp + q), w3, keep, [&](int k, int c) {
                    const float r = bilerp(tap[c][k][0], tap[c][k][1], tap[c][k][2], tap[c][k][3], up[k].tx, up[k].ty);
                    return quantise_u8((double)fullres_value(p[k][c], m[k], d[c][k], r));
                });
            }
        } else {
            // sub-sampled (or a network of 2^30 pixels and more): the planes are read through flat addresses
            for (uint32_t l = 0; l < L; ++l) {
                const float *re_l = f.rendered + (size_t)l * 3u * hw;              // (uniform)
                quad_store_selected(f.out + 3u * ((size_t)l * HWp + q), w3, keep, [&](int k, int c) {
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
            if (px_w >= HWp)
                continue;
            const uint8_t *pp = f.photo + 3u * (size_t)px_w;
            const uint8_t pb[3] = {pp[0], pp[1], pp[2]};
            const uint32_t py = px_w / Wp, px = px_w - py * Wp;
            bool in = false;
            if (reach) {
                const int64_t c0 = M.m00 * (int64_t)(2u * (uint64_t)px + 1u) + M.m01 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m02;
                const int64_t c1 = M.m10 * (int64_t)(2u * (uint64_t)px + 1u) + M.m11 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m12;
                in = affine_inside(c0, c1, lim0, lim1);
            }
            if (!in) {
                for (uint32_t l = 0; l < L; ++l) {
                    uint8_t *o = f.out + 3u * ((size_t)l * HWp + px_w);
                    o[0] = pb[0], o[1] = pb[1], o[2] = pb[2];
                }
                continue;
            }
            int64_t P0, P1;
            M.origin(px, py, P0, P1);
            composite_pixel(AffineCarrier(M, P0, P1, h, w), pb, f, L, hw, HWp, px_w, floor, lo, hi);
        }
    }
}

// Ingest (gcfr_fullres_box.hip's work split): a workgroup owns kQuadChunk consecutive network pixels of one face, lane t pixels t,
// t + 256, t + 512, t + 768, one byte at a time.  A sub-sample's row sum of wx byte is at most 255 den < 2^26; the rows are added
// in 64 bits.
__global__ __launch_bounds__(kQuadLanes) void affine_ingest_kernel(const uint8_t *__restrict__ photo, uint32_t h, uint32_t w,
                                                                   uint32_t Hp, uint32_t Wp, uint32_t HWp, uint32_t chunks,
                                                                   AffineArgs maps, float *__restrict__ x_lo)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<false>(ch * (uint32_t)kQuadChunk);
    const AffineMap M(maps, b);
    const uint32_t K = M.K(), shift = M.shift();
    const uint32_t den = 1u << shift, low = den - 1u;
    const int64_t s00 = 2 * M.m00, s01 = 2 * M.m01, s10 = 2 * M.m10, s11 = 2 * M.m11;
    const uint32_t hw = h * w;
    const uint8_t *ph_b = photo + (size_t)b * 3u * HWp;
    float *xl_b = x_lo + (size_t)b * 3u * hw;
    const double scale = 255.0 * (double)(K * K) * (double)den * (double)den;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const uint32_t px = quad_pixel<false>(q, k);
        if (px >= hw)
            continue;
        const uint32_t i = px / w, j = px - i * w;
        int64_t r0, r1;
        M.origin(j, i, r0, r1);
        uint64_t acc[3] = {0u, 0u, 0u};
        for (uint32_t sv = 0; sv < K; ++sv, r0 += s01, r1 += s11) {
            int64_t p0 = r0, p1 = r1;
            for (uint32_t su = 0; su < K; ++su, p0 += s00, p1 += s10) {
                const int64_t x0 = p0 >> shift, y0 = p1 >> shift;                  // (floor: an arithmetic shift)
                const uint32_t fx = (uint32_t)p0 & low, fy = (uint32_t)p1 & low;
                const int64_t xm = (int64_t)Wp - 1, ym = (int64_t)Hp - 1;
                const uint32_t xa = (uint32_t)(x0 < 0 ? 0 : x0 > xm ? xm : x0), xb = (uint32_t)(x0 + 1 < 0 ? 0 : x0 + 1 > xm ? xm : x0 + 1);
                const uint32_t ya = (uint32_t)(y0 < 0 ? 0 : y0 > ym ? ym : y0), yb = (uint32_t)(y0 + 1 < 0 ? 0 : y0 + 1 > ym ? ym : y0 + 1);
                const uint8_t *top = ph_b + 3u * ((size_t)ya * Wp), *bot = ph_b + 3u * ((size_t)yb * Wp);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t s_top = (den - fx) * top[3u * (size_t)xa + c] + fx * top[3u * (size_t)xb + c];
                    const uint32_t s_bot = (den - fx) * bot[3u * (size_t)xa + c] + fx * bot[3u * (size_t)xb + c];
                    acc[c] += (uint64_t)(den - fy) * s_top + (uint64_t)fy * s_bot;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            xl_b[3u * (size_t)px + c] = (float)((double)acc[c] / scale);
    }
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_ingest_affine_u8(const uint8_t *photo_u8, int32_t B, int32_t Hp, int32_t Wp, const int64_t *F, int32_t h,
                                     int32_t w, float *x_lo_out, void *stream)
{
    uint32_t HWp, hw;
    if (!photo_u8 || !x_lo_out || !F || (const void *)photo_u8 == (const void *)x_lo_out || !box_shape(B, Hp, Wp, h, w, HWp, hw))
        return GCFR_ERR_INVALID_ARGUMENT;
    AffineArgs probe;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces)                                  // every refusal before any launch
        if (!affine_args(F + 6 * (size_t)b0, B - b0 < kBoxFaces ? B - b0 : kBoxFaces, false, Hp, h, w, probe))
            return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (hw + kQuadChunk - 1) / kQuadChunk;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        AffineArgs args;
        affine_args(F + 6 * (size_t)b0, n, false, Hp, h, w, args);
        hipLaunchKernelGGL(affine_ingest_kernel, dim3((uint32_t)n * chunks), dim3(kQuadLanes), 0, st, photo_u8 + (size_t)b0 * 3u * HWp,
                           (uint32_t)h, (uint32_t)w, (uint32_t)Hp, (uint32_t)Wp, HWp, chunks, args, x_lo_out + (size_t)b0 * 3u * hw);
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_fullres_composites_affine_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered,
                                                 const uint8_t *mask_u8, int32_t mask_batch, int32_t B, int32_t L, int32_t Hp,
                                                 int32_t Wp, const int64_t *I, int32_t h, int32_t w, float floor, float detail_clamp,
                                                 uint8_t *out_u8, void *stream)
{
    uint32_t HWp, hw, mask_stride;
    float lo;
    if (!I || !box_shape(B, Hp, Wp, h, w, HWp, hw) ||
        !fullres_operands(photo_u8, x_lo, rendered, mask_u8, out_u8, L, mask_batch, B, hw, detail_clamp, floor, mask_stride, lo))
        return GCFR_ERR_INVALID_ARGUMENT;
    AffineArgs probe;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces)                                  // every refusal before any launch
        if (!affine_args(I + 6 * (size_t)b0, B - b0 < kBoxFaces ? B - b0 : kBoxFaces, true, Hp, h, w, probe))
            return GCFR_ERR_INVALID_ARGUMENT;
    // out must not overlap the photographs
    const uintptr_t pa = (uintptr_t)photo_u8, pe = pa + (uintptr_t)B * 3u * HWp;
    const uintptr_t oa = (uintptr_t)out_u8, oe = oa + (uintptr_t)B * (uintptr_t)L * 3u * HWp;
    if (oa < pe && pa < oe)
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (HWp + kQuadChunk - 1) / kQuadChunk;
    const bool vec = (uint32_t)Wp % 4u == 0 && aligned4(out_u8);
    const int32_t buf = hw <= 0x3fffffffu;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        const dim3 grid((uint32_t)n * chunks);
        AffineArgs args;
        affine_args(I + 6 * (size_t)b0, n, true, Hp, h, w, args);
        const uint8_t *ph = photo_u8 + (size_t)b0 * 3u * HWp;
        const float *xl = x_lo + (size_t)b0 * 3u * hw, *re = rendered + (size_t)b0 * (size_t)L * 3u * hw;
        const uint8_t *mk = mask_u8 + (size_t)b0 * mask_stride;
        uint8_t *o = out_u8 + (size_t)b0 * (size_t)L * 3u * HWp;
        with_flag(vec, [&](auto V) {
            hipLaunchKernelGGL((affine_composites_kernel<decltype(V)::value>), grid, dim3(kQuadLanes), 0, st, ph, xl, re, mk,
                               mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, chunks, buf, floor, lo,
                               detail_clamp, args, o);
        });
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
