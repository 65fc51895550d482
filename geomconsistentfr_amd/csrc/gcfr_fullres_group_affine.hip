// Rotated faces in group photographs, gfx950: EVERY tilted face of a photograph relit in one pass over the photograph's bytes.
// gcfr_fullres_group.hip does this for axis-aligned boxes, gcfr_fullres_affine.hip takes a 2 x 3 map but one face per photograph;
// here P photographs carry B faces, face b living in photograph photo_index[b] under its own pair of maps F[b], I[b].
//   ingest      photograph photo_index[b] sampled through F[b] -> the network's f32 input (B, h, w, 3): gcfr_fullres_affine.hip's
//               ingest with the photograph taken from a per-slot index; the photographs are neither gathered nor copied
//   composite   per photograph q and light l the CHAIN of gcfr_fullres_affine.hip's composite over the faces of q in ascending face
//               index: the running image starts as the photograph, face b relights it where a pixel's centre lands in the network
//               square under I[b] and its carried mask is positive, reading the RUNNING byte where that composite reads the
//               photograph's (in the blend and in the quotient d), and every step rounds to a byte.  (P, L, Hp, Wp, 3).
// The arithmetic is gcfr_fullres_affine.hpp's (maps, carrier, inside test) and gcfr_fullres.hpp's (detail_of, fullres_value,
// fullres_byte, quantise_u8, composite_pixel).  Built with -ffp-contract=off.
//
// Work split (gcfr_fullres_group.hip's): a workgroup of kQuadLanes lanes owns kQuadChunk consecutive pixels of ONE PHOTOGRAPH; VEC
// where Wp is a multiple of four and out is 4-byte aligned.  The I maps with log2 K and the rows each quad can reach (an AffineArgs,
// affine_args(rows = true)), the faces' global indices and each photograph's range of face slots travel BY VALUE in the argument
// block, about 2.2 KB: nothing is uploaded, no device scratch, capture-safe.  The workgroup walks its photograph's slots in
// ascending order in a uniform loop; a slot whose rows [y_lo, y_hi) miss the chunk's rows is skipped by the whole workgroup without
// any 64-bit work, and K, uniform per face, is branched on.  Per face a lane forms the four inside tests (neighbours by additions of
// the matrix column), the four carriers, m and the carried x_lo ONCE and then walks the L lights: with K = 1 and 4 h w < 2^32 the taps
// go through buffer descriptors, otherwise through the flat-address sub-sample loops.  The running bytes live in `out`: the first
// face that relights one of a lane's pixels takes the photograph's dwords and forms d once; a later face reads back, per light, what
// THIS LANE stored through the same pointer and forms d per light.  No atomics, no LDS, no barrier.  A lane that no face relights
// copies its 12 bytes L times.
// A launch covers whole photographs with at most kBoxFaces face slots in all and at most kTiltedPhotos photographs.  A photograph
// with more faces is launched alone, kBoxFaces faces at a time: the CONTINUATION launches (cont = 1) run on the same stream, start
// from `out` instead of the photograph and write only what their faces relight.
#include <algorithm>
#include <vector>

#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"
#include "gcfr_fullres_affine.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kTiltedPhotos = 32;              // photographs per launch

// the faces of one composite launch: slot s is face `face[s]` with the map, K and rows maps.*[s]; photograph j of the launch owns
// the slots begin[j] .. begin[j + 1] - 1, in ascending face index
struct TiltedGroupArgs {
    AffineArgs maps;
    int32_t face[kBoxFaces];
    int32_t begin[kTiltedPhotos + 1];
};

// the faces of one ingest launch: slot s reads photograph `photo[s]` through maps.m[s]
struct TiltedIngestArgs {
    AffineArgs maps;
    int32_t photo[kBoxFaces];
};

// One face over a lane's four pixels at `oq` for all L lights (the vector path).  FIRST: the running bytes are the photograph's w3
// for every light and d is formed once; otherwise they are what this lane stored at `oq` for that light, and d is formed per light.
// xl: the carried x_lo; r_up(re_l, k, c): the carried `rendered` of the light whose planes start at re_l.
template <bool FIRST, class R>
__device__ inline void tilted_quad_lights(uint8_t *oq, size_t light, const float *re, uint32_t L, uint32_t hw, const uint32_t (&w3)[3],
                                          const uint32_t (&keep)[3], const float (&xl)[4][3], const float (&m)[4], float floor, float lo,
                                          float hi, R r_up)
{
    float p[4][3], d[4][3];
    if (FIRST) {
        quad_unpack_u8x3(w3, p);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[k][c] = detail_of(p[k][c], xl[k][c], floor, lo, hi);
    }
    for (uint32_t l = 0; l < L; ++l) {
        uint8_t *ol = oq + (size_t)l * light;
        const float *re_l = re + (size_t)l * 3u * hw;                              // (uniform)
        uint32_t run[3] = {w3[0], w3[1], w3[2]};
        if (!FIRST) {
            const uint32_t *ow = reinterpret_cast<const uint32_t *>(ol);
            run[0] = ow[0], run[1] = ow[1], run[2] = ow[2];
            quad_unpack_u8x3(run, p);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    d[k][c] = detail_of(p[k][c], xl[k][c], floor, lo, hi);
        }
        quad_store_selected(ol, run, keep, [&](int k, int c) {
            return quantise_u8((double)fullres_value(p[k][c], m[k], d[k][c], r_up(re_l, k, c)));
        });
    }
}

// The scalar path's later face: pixel px of the photograph whose output starts at f.out, relit (m > 0) over the running bytes this
// lane stored, one element at a time.  (The first face is gcfr_fullres.hpp's composite_pixel.)
__device__ inline void tilted_pixel_again(const AffineCarrier &up, const FacePlanes &f, uint32_t L, uint32_t hw, uint32_t WN, uint32_t px,
                                          float m, float floor, float lo, float hi)
{
    float xl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        xl[c] = up([&](uint32_t t) { return f.x_lo[3u * (size_t)t + c]; });
    for (uint32_t l = 0; l < L; ++l) {
        const float *re_l = f.rendered + (size_t)l * 3u * hw;
        uint8_t *o = f.out + 3u * ((size_t)l * WN + px);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *plane = re_l + (size_t)c * hw;
            const uint8_t rb = o[c];
            const float p = (float)rb;
            o[c] = fullres_byte(rb, p, m, detail_of(p, xl[c], floor, lo, hi), up([&](uint32_t t) { return plane[t]; }));
        }
    }
}

// photo / out: the launch's first photograph.  cont: a continuation launch (the running bytes are already in `out`).
// buf: 4 h w < 2^32, so that a tap's byte offset in a plane of `rendered` fits a buffer load's 32-bit offset
template <bool VEC>
__global__ __launch_bounds__(kQuadLanes) void tilted_group_composites_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t Wp, uint32_t HWp,
    uint32_t chunks, int32_t cont, int32_t buf, float floor, float lo, float hi, TiltedGroupArgs g, uint8_t *out)
{
    const uint32_t j = blockIdx.x / chunks, ch = blockIdx.x - j * chunks;          // (uniform; j < kTiltedPhotos)
    const uint32_t q0 = ch * (uint32_t)kQuadChunk;
    const uint32_t q = quad_first<VEC>(q0);
    const uint32_t hw = h * w;
    const uint32_t last = min(q0 + (uint32_t)kQuadChunk, HWp) - 1u;
    const int32_t row0 = (int32_t)(q0 / Wp), row1 = (int32_t)(last / Wp);          // (uniform) the chunk's rows
    const uint8_t *ph = photo + (size_t)j * 3u * HWp;
    uint8_t *o = out + (size_t)j * L * 3u * HWp;
    const size_t light = 3u * (size_t)HWp;
    const uint64_t lim0 = (uint64_t)(2 * kAffineOne) * w, lim1 = (uint64_t)(2 * kAffineOne) * h;
    const int32_t s0 = g.begin[j], s1 = g.begin[j + 1];
    if (VEC) {
        if (q >= HWp)                                                              // all four pixels in range or none
            return;
        const uint32_t py = q / Wp, px = q - py * Wp;
        const uint8_t *pp = ph + 3u * (size_t)q;
        const uint32_t w3[3] = {load_dword_any(pp), load_dword_any(pp + 4), load_dword_any(pp + 8)};
        uint8_t *oq = o + 3u * (size_t)q;
        bool in_out = cont != 0;                                                   // do the running bytes stand in `out`?
        for (int32_t s = s0; s < s1; ++s) {
            if (g.maps.y_lo[s] > row1 || g.maps.y_hi[s] <= row0)                   // (uniform) the face's rows miss the chunk's
                continue;
            const AffineMap M(g.maps, (uint32_t)s);
            const int64_t c0 = M.m00 * (int64_t)(2u * (uint64_t)px + 1u) + M.m01 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m02;
            const int64_t c1 = M.m10 * (int64_t)(2u * (uint64_t)px + 1u) + M.m11 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m12;
            bool in[4], any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                in[k] = affine_inside(c0 + 2 * k * M.m00, c1 + 2 * k * M.m10, lim0, lim1);
                any = any || in[k];
            }
            if (!any)
                continue;
            const uint32_t b = (uint32_t)g.face[s];
            const float *xl_b = x_lo + (size_t)b * 3u * hw;
            const float *re_b = rendered + (size_t)b * L * 3u * hw;
            const uint8_t *mk_b = mask + (size_t)b * mask_stride;
            int64_t P0, P1;
            M.origin(px, py, P0, P1);
            const int64_t dx0 = 2 * M.m00 * (int64_t)M.K(), dx1 = 2 * M.m10 * (int64_t)M.K();  // (uniform) P's step of one pixel in x
            AffineCarrier up[4];
            float m[4];
            bool relit[4], some = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                up[k] = AffineCarrier(M, P0 + k * dx0, P1 + k * dx1, h, w);
                m[k] = up[k]([&](uint32_t t) { return mask_quotient_f32(mk_b[t]); });
                relit[k] = m[k] > 0.0f && in[k];
                some = some || relit[k];
            }
            if (!some)                                                             // the running bytes are kept
                continue;
            float xl[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    xl[k][c] = up[k]([&](uint32_t t) { return xl_b[3u * (size_t)t + c]; });
            uint32_t keep[3];                                                      // relit ? the relit byte : the running one
            quad_select_mask(relit, keep);
            if (M.lk == 0u && buf) {
                // gcfr_fullres_box.hip's taps: BYTE offsets in a plane of `rendered` behind a buffer descriptor
                uint32_t off[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    off[k][0] = 4u * up[k].t00, off[k][1] = 4u * up[k].t01, off[k][2] = 4u * up[k].t10, off[k][3] = 4u * up[k].t11;
                auto r_up = [&](const float *re_l, int k, int c) {
                    const PlaneF32 plane(re_l + (size_t)c * hw, hw);
                    return bilerp(plane.at(off[k][0]), plane.at(off[k][1]), plane.at(off[k][2]), plane.at(off[k][3]), up[k].tx, up[k].ty);
                };
                if (!in_out)
                    tilted_quad_lights<true>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
                else
                    tilted_quad_lights<false>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
            } else {
                // sub-sampled (or a network of 2^30 pixels and more): the planes are read through flat addresses
                auto r_up = [&](const float *re_l, int k, int c) {
                    const float *plane = re_l + (size_t)c * hw;
                    return up[k]([&](uint32_t t) { return plane[t]; });
                };
                if (!in_out)
                    tilted_quad_lights<true>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
                else
                    tilted_quad_lights<false>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
            }
            in_out = true;
        }
        if (!in_out)                                                               // no face relights these pixels: the photograph's
            for (uint32_t l = 0; l < L; ++l) {
                uint32_t *ow = reinterpret_cast<uint32_t *>(oq + (size_t)l * light);
                ow[0] = w3[0], ow[1] = w3[1], ow[2] = w3[2];
            }
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const uint32_t px_w = quad_pixel<false>(q, k);
            if (px_w >= HWp)
                continue;
            const uint32_t py = px_w / Wp, px = px_w - py * Wp;
            const uint8_t *pp = ph + 3u * (size_t)px_w;
            const uint8_t pb[3] = {pp[0], pp[1], pp[2]};
            bool in_out = cont != 0;
            for (int32_t s = s0; s < s1; ++s) {
                if (g.maps.y_lo[s] > row1 || g.maps.y_hi[s] <= row0)               // (uniform)
                    continue;
                const AffineMap M(g.maps, (uint32_t)s);
                const int64_t c0 = M.m00 * (int64_t)(2u * (uint64_t)px + 1u) + M.m01 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m02;
                const int64_t c1 = M.m10 * (int64_t)(2u * (uint64_t)px + 1u) + M.m11 * (int64_t)(2u * (uint64_t)py + 1u) + 2 * M.m12;
                if (!affine_inside(c0, c1, lim0, lim1))
                    continue;
                const uint32_t b = (uint32_t)g.face[s];
                const FacePlanes f{ph, x_lo + (size_t)b * 3u * hw, mask + (size_t)b * mask_stride, rendered + (size_t)b * L * 3u * hw, o};
                int64_t P0, P1;
                M.origin(px, py, P0, P1);
                const AffineCarrier up(M, P0, P1, h, w);
                const float m = up([&](uint32_t t) { return mask_quotient_f32(f.mask[t]); });
                if (!(m > 0.0f))
                    continue;
                if (!in_out)
                    composite_pixel(up, pb, f, L, hw, HWp, px_w, floor, lo, hi);
                else
                    tilted_pixel_again(up, f, L, hw, HWp, px_w, m, floor, lo, hi);
                in_out = true;
            }
            if (!in_out)
                for (uint32_t l = 0; l < L; ++l) {
                    uint8_t *ol = o + 3u * ((size_t)l * HWp + px_w);
                    ol[0] = pb[0], ol[1] = pb[1], ol[2] = pb[2];
                }
        }
    }
}

// gcfr_fullres_affine.hip's ingest loop nest; slot b's photograph is g.photo[b].  x_lo: the launch's first face.
__global__ __launch_bounds__(kQuadLanes) void tilted_group_ingest_kernel(const uint8_t *__restrict__ photo, uint32_t h, uint32_t w,
                                                                         uint32_t Hp, uint32_t Wp, uint32_t HWp, uint32_t chunks,
                                                                         TiltedIngestArgs g, float *__restrict__ x_lo)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<false>(ch * (uint32_t)kQuadChunk);
    const AffineMap M(g.maps, b);
    const uint32_t K = M.K(), shift = M.shift();
    const uint32_t den = 1u << shift, low = den - 1u;
    const int64_t s00 = 2 * M.m00, s01 = 2 * M.m01, s10 = 2 * M.m10, s11 = 2 * M.m11;
    const uint32_t hw = h * w;
    const uint8_t *ph_b = photo + (size_t)(uint32_t)g.photo[b] * 3u * HWp;
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

// every map of the call under include/gcfr.h's rules, and every face's photograph in [0, P)
inline bool tilted_faces_ok(const int64_t *maps, const int32_t *photo_index, int32_t B, int32_t P)
{
    for (int32_t b = 0; b < B; ++b)
        if (affine_log2k(maps + 6 * (size_t)b) < 0 || photo_index[b] < 0 || photo_index[b] >= P)
            return false;
    return true;
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_ingest_group_affine_u8(const uint8_t *photo_u8, int32_t P, int32_t Hp, int32_t Wp, const int64_t *F,
                                           const int32_t *photo_index, int32_t B, int32_t h, int32_t w, float *x_lo_out, void *stream)
{
    uint32_t HWp, hw;
    if (!photo_u8 || !x_lo_out || !F || !photo_index || (const void *)photo_u8 == (const void *)x_lo_out || B < 1 ||
        !box_shape(P, Hp, Wp, h, w, HWp, hw) || !tilted_faces_ok(F, photo_index, B, P))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (hw + kQuadChunk - 1) / kQuadChunk;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        TiltedIngestArgs g = {};
        affine_args(F + 6 * (size_t)b0, n, false, Hp, h, w, g.maps);
        for (int32_t s = 0; s < n; ++s)
            g.photo[s] = photo_index[b0 + s];
        hipLaunchKernelGGL(tilted_group_ingest_kernel, dim3((uint32_t)n * chunks), dim3(kQuadLanes), 0, st, photo_u8, (uint32_t)h,
                           (uint32_t)w, (uint32_t)Hp, (uint32_t)Wp, HWp, chunks, g, x_lo_out + (size_t)b0 * 3u * hw);
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_fullres_composites_group_affine_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered,
                                                       const uint8_t *mask_u8, int32_t mask_batch, int32_t P, int32_t B, int32_t L,
                                                       int32_t Hp, int32_t Wp, const int64_t *I, const int32_t *photo_index, int32_t h,
                                                       int32_t w, float floor, float detail_clamp, uint8_t *out_u8, void *stream)
{
    uint32_t HWp, hw, mask_stride;
    float lo;
    if (!I || !photo_index || B < 1 || !box_shape(P, Hp, Wp, h, w, HWp, hw) ||
        !fullres_operands(photo_u8, x_lo, rendered, mask_u8, out_u8, L, mask_batch, B, hw, detail_clamp, floor, mask_stride, lo) ||
        !tilted_faces_ok(I, photo_index, B, P))
        return GCFR_ERR_INVALID_ARGUMENT;
    // out must not overlap the photographs
    const uintptr_t pa = (uintptr_t)photo_u8, pe = pa + (uintptr_t)P * 3u * HWp;
    const uintptr_t oa = (uintptr_t)out_u8, oe = oa + (uintptr_t)P * (uintptr_t)L * 3u * HWp;
    if (oa < pe && pa < oe)
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (HWp + kQuadChunk - 1) / kQuadChunk;
    const bool vec = (uint32_t)Wp % 4u == 0 && aligned4(out_u8);
    const int32_t buf = hw <= 0x3fffffffu;
    hipStream_t st = (hipStream_t)stream;
    // the faces by photograph, within a photograph in ascending face index
    std::vector<int32_t> order((size_t)B);
    for (int32_t b = 0; b < B; ++b)
        order[(size_t)b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return photo_index[a] < photo_index[b]; });
    TiltedGroupArgs g = {};
    int64_t maps[kBoxFaces][6];                                                    // the slots' maps, for affine_args
    int32_t photos = 0, slots = 0, first = 0;                                      // the launch being filled
    auto add = [&](const int32_t *faces, int32_t n) {                              // one more photograph with these faces
        g.begin[photos] = slots;
        for (int32_t k = 0; k < n; ++k, ++slots) {
            for (int i = 0; i < 6; ++i)
                maps[slots][i] = I[6 * (size_t)faces[k] + i];
            g.face[slots] = faces[k];
        }
        g.begin[++photos] = slots;
    };
    auto flush = [&](int32_t cont) {
        if (!photos)
            return;
        affine_args(&maps[0][0], slots, true, Hp, h, w, g.maps);
        const uint8_t *ph = photo_u8 + (size_t)first * 3u * HWp;
        uint8_t *o = out_u8 + (size_t)first * (size_t)L * 3u * HWp;
        const dim3 grid((uint32_t)photos * chunks);
        with_flag(vec, [&](auto V) {
            hipLaunchKernelGGL((tilted_group_composites_kernel<decltype(V)::value>), grid, dim3(kQuadLanes), 0, st, ph, x_lo, rendered,
                               mask_u8, mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, chunks, cont, buf, floor,
                               lo, detail_clamp, g, o);
        });
        g = TiltedGroupArgs{};
        photos = slots = 0;
    };
    int32_t at = 0;
    for (int32_t q = 0; q < P; ++q) {
        int32_t n = 0;
        while (at + n < B && photo_index[order[(size_t)(at + n)]] == q)
            ++n;
        if (n > kBoxFaces || photos == kTiltedPhotos || slots + n > kBoxFaces)
            flush(0);
        if (!photos)
            first = q;
        if (n <= kBoxFaces) {
            add(order.data() + at, n);
        } else {                                                                   // alone, kBoxFaces faces per launch
            for (int32_t k = 0; k < n; k += kBoxFaces) {
                first = q;
                add(order.data() + at + k, n - k < kBoxFaces ? n - k : kBoxFaces);
                flush(k > 0);
            }
        }
        at += n;
    }
    flush(0);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
