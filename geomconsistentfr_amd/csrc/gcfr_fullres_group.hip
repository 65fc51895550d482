// Group photographs, gfx950: EVERY face of a photograph relit in one pass over the photograph's bytes.  gcfr_fullres_anybox.hip takes
// one box per photograph and returns one photograph per face; here P photographs carry B faces, face b living in photograph
// photo_index[b], and ONE photograph per photograph comes back with all of its faces relit.
//   ingest      box b of photograph photo_index[b] -> the network's f32 input (B, h, w, 3): gcfr_fullres_anybox.hip's ingest with the
//               photograph taken from a per-slot index; the photographs are neither gathered nor copied
//   composite   per photograph q and light l the CHAIN of gcfr_fullres_anybox.hip's pasted composite over the faces of q in ascending
//               face index: the running image starts as the photograph, face b relights it inside its box where its carried mask
//               is positive, reading the RUNNING byte where that composite reads the photograph's (in the blend and in the quotient
//               d), and every step rounds to a byte.  (P, L, Hp, Wp, 3).
// The arithmetic is gcfr_fullres_anybox.hpp's (carrier, ingest axes) and gcfr_fullres.hpp's (detail_of, fullres_value,
// fullres_byte, quantise_u8): nothing is restated here.  Built with -ffp-contract=off.
//
// Work split: a workgroup of kQuadLanes lanes owns kQuadChunk consecutive pixels of ONE PHOTOGRAPH (gcfr_fullres_box.hip's split;
// VEC as there: Wp a multiple of four and out 4-byte aligned, a lane's four pixels then lie in one row and move as three dwords).
// The boxes, the faces' global indices and each photograph's range of face slots travel BY VALUE in the argument block: nothing is
// uploaded.  The workgroup walks its photograph's slots in order, in a uniform loop; a face whose rows miss the chunk's rows is
// skipped by the whole workgroup, and the two axis modes, uniform per face, are branched on.  Per face a lane forms the taps, m and
// the carried x_lo once and then walks the L lights.  L reaches 4096, so the running bytes live in `out`: the first face that relights
// one of a lane's pixels takes the photograph's bytes as the running value (and forms d once, as gcfr_fullres_anybox.hip does); a
// later face reads back, per light, the dwords or bytes THIS LANE stored -- the same thread through the same pointer, no other lane
// ever writes them: no atomics, no LDS -- and forms d per light, because p now depends on the light.  A lane that no face relights
// copies its 12 bytes L times.
// A launch covers whole photographs with at most kBoxFaces face slots in all.  A photograph with more faces gets CONTINUATION
// launches on the same stream (cont = 1): they start from `out` instead of the photograph and write only what their faces relight.
#include <algorithm>
#include <vector>

#include "gcfr_device.hpp"
#include "gcfr_fullres.hpp"
#include "gcfr_fullres_anybox.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kGroupPhotos = 32;               // photographs per launch

// the faces of one composite launch: slot s is face `face[s]` with box `boxes.*[s]`; photograph j of the launch owns the slots
// begin[j] .. begin[j + 1] - 1, in ascending face index
struct GroupArgs {
    BoxArgs boxes;
    int32_t face[kBoxFaces];
    int32_t begin[kGroupPhotos + 1];
};

// the faces of one ingest launch: slot s reads photograph `photo[s]`
struct GroupIngestArgs {
    BoxArgs boxes;
    int32_t photo[kBoxFaces];
};

// One face over a lane's four pixels at `oq` for all L lights (the vector path).  FIRST: the running bytes are the photograph's w3
// for every light and d is formed once; otherwise they are what this lane stored at `oq` for that light, and d is formed per light.
// xl: the carried x_lo; r_up(re_l, k, c): the carried `rendered` of the light whose planes start at re_l.
template <bool FIRST, class R>
__device__ inline void group_quad_lights(uint8_t *oq, size_t light, const float *re, uint32_t L, uint32_t hw, const uint32_t (&w3)[3],
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
__device__ inline void group_pixel_again(const AnyCarrier &up, const FacePlanes &f, uint32_t L, uint32_t hw, uint32_t WN, uint32_t px,
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
template <bool VEC>
__global__ __launch_bounds__(kQuadLanes) void group_composites_kernel(
    const uint8_t *__restrict__ photo, const float *__restrict__ x_lo, const float *__restrict__ rendered,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, uint32_t L, uint32_t h, uint32_t w, uint32_t Wp, uint32_t HWp,
    uint32_t chunks, int32_t cont, float floor, float lo, float hi, GroupArgs g, uint8_t *out)
{
    const uint32_t j = blockIdx.x / chunks, ch = blockIdx.x - j * chunks;          // (uniform; j < kGroupPhotos)
    const uint32_t c0 = ch * (uint32_t)kQuadChunk;
    const uint32_t q = quad_first<VEC>(c0);
    const uint32_t hw = h * w;
    const uint32_t last = min(c0 + (uint32_t)kQuadChunk, HWp) - 1u;
    const int32_t row0 = (int32_t)(c0 / Wp), row1 = (int32_t)(last / Wp);          // (uniform) the chunk's rows
    const uint8_t *ph = photo + (size_t)j * 3u * HWp;
    uint8_t *o = out + (size_t)j * L * 3u * HWp;
    const size_t light = 3u * (size_t)HWp;
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
            const int32_t bx0 = g.boxes.x0[s], by0 = g.boxes.y0[s], bw = g.boxes.bw[s], bh = g.boxes.bh[s];
            if (by0 > row1 || by0 + bh <= row0)                                    // (uniform) the face's rows miss the chunk's
                continue;
            const bool ay = (uint32_t)bh < h, ax = (uint32_t)bw < w;               // (uniform) the minified axes
            const uint32_t b = (uint32_t)g.face[s];
            const float *xl_b = x_lo + (size_t)b * 3u * hw;
            const float *re_b = rendered + (size_t)b * L * 3u * hw;
            const uint8_t *mk_b = mask + (size_t)b * mask_stride;
            bool in_y, in_x[4], any = false;
            const uint32_t ry = box_clamp((int32_t)py, by0, bh, in_y);
            uint32_t rx[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                rx[k] = box_clamp((int32_t)px + k, bx0, bw, in_x[k]);
                in_x[k] = in_x[k] && in_y;
                any = any || in_x[k];
            }
            if (!any)
                continue;
            const CarryAxis Y = carry_axis(ay, ry, h, (uint32_t)bh);
            AnyCarrier up[4];
            float m[4];
            bool relit[4], some = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                up[k] = AnyCarrier{ay, ax, h, w, (uint32_t)bh, (uint32_t)bw, Y, carry_axis(ax, rx[k], w, (uint32_t)bw)};
                m[k] = up[k]([&](uint32_t t) { return mask_quotient_f32(mk_b[t]); });
                relit[k] = m[k] > 0.0f && in_x[k];
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
            if (!ay && !ax) {
                // gcfr_fullres_box.hip's taps: BYTE offsets in a plane of `rendered` behind a buffer descriptor (4 h w < 2^32:
                // 2 bh h, 2 bw w < 2^31 with bh >= h, bw >= w)
                uint32_t off[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    off[k][0] = 4u * (Y.i0 * w + up[k].X.i0), off[k][1] = 4u * (Y.i0 * w + up[k].X.i1);
                    off[k][2] = 4u * (Y.i1 * w + up[k].X.i0), off[k][3] = 4u * (Y.i1 * w + up[k].X.i1);
                }
                auto r_up = [&](const float *re_l, int k, int c) {
                    const PlaneF32 plane(re_l + (size_t)c * hw, hw);
                    return bilerp(plane.at(off[k][0]), plane.at(off[k][1]), plane.at(off[k][2]), plane.at(off[k][3]), up[k].X.t, Y.t);
                };
                if (!in_out)
                    group_quad_lights<true>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
                else
                    group_quad_lights<false>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
            } else {
                // a minified axis: h w may pass 2^30 here (8 nb >= n only), so the planes are read through flat addresses
                auto r_up = [&](const float *re_l, int k, int c) {
                    const float *plane = re_l + (size_t)c * hw;
                    return up[k]([&](uint32_t t) { return plane[t]; });
                };
                if (!in_out)
                    group_quad_lights<true>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
                else
                    group_quad_lights<false>(oq, light, re_b, L, hw, w3, keep, xl, m, floor, lo, hi, r_up);
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
                const int32_t bx0 = g.boxes.x0[s], by0 = g.boxes.y0[s], bw = g.boxes.bw[s], bh = g.boxes.bh[s];
                if (by0 > row1 || by0 + bh <= row0)                                // (uniform)
                    continue;
                bool in_y, in_x;
                const uint32_t ry = box_clamp((int32_t)py, by0, bh, in_y), rx = box_clamp((int32_t)px, bx0, bw, in_x);
                if (!(in_y && in_x))
                    continue;
                const bool ay = (uint32_t)bh < h, ax = (uint32_t)bw < w;
                const uint32_t b = (uint32_t)g.face[s];
                const FacePlanes f{ph, x_lo + (size_t)b * 3u * hw, mask + (size_t)b * mask_stride, rendered + (size_t)b * L * 3u * hw, o};
                const AnyCarrier up{ay, ax, h, w, (uint32_t)bh, (uint32_t)bw, carry_axis(ay, ry, h, (uint32_t)bh),
                                    carry_axis(ax, rx, w, (uint32_t)bw)};
                const float m = up([&](uint32_t t) { return mask_quotient_f32(f.mask[t]); });
                if (!(m > 0.0f))
                    continue;
                if (!in_out)
                    composite_pixel(up, pb, f, L, hw, HWp, px_w, floor, lo, hi);
                else
                    group_pixel_again(up, f, L, hw, HWp, px_w, m, floor, lo, hi);
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

// gcfr_fullres_anybox.hip's ingest loop nest; slot b's photograph is g.photo[b].  x_lo: the launch's first face.
__global__ __launch_bounds__(kQuadLanes) void group_ingest_kernel(const uint8_t *__restrict__ photo, uint32_t h, uint32_t w, uint32_t Wp,
                                                                  uint32_t HWp, uint32_t chunks, GroupIngestArgs g,
                                                                  float *__restrict__ x_lo)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform; b < kBoxFaces)
    const uint32_t q = quad_first<false>(ch * (uint32_t)kQuadChunk);
    const uint32_t bx0 = (uint32_t)g.boxes.x0[b], by0 = (uint32_t)g.boxes.y0[b], bw = (uint32_t)g.boxes.bw[b], bh = (uint32_t)g.boxes.bh[b];
    const bool my = bh < h, mx = bw < w;                                           // (uniform) the magnified axes
    const uint32_t hw = h * w;
    const uint8_t *ph_b = photo + (size_t)(uint32_t)g.photo[b] * 3u * HWp;
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

// the faces' photographs lie in [0, P)
inline bool photo_index_ok(const int32_t *photo_index, int32_t B, int32_t P)
{
    for (int32_t b = 0; b < B; ++b)
        if (photo_index[b] < 0 || photo_index[b] >= P)
            return false;
    return true;
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_ingest_group_u8(const uint8_t *photo_u8, int32_t P, int32_t Hp, int32_t Wp, const int32_t *boxes,
                                    const int32_t *photo_index, int32_t B, int32_t h, int32_t w, float *x_lo_out, void *stream)
{
    uint32_t HWp, hw;
    if (!photo_u8 || !x_lo_out || !boxes || !photo_index || (const void *)photo_u8 == (const void *)x_lo_out || B < 1 ||
        !box_shape(P, Hp, Wp, h, w, HWp, hw) || !anyboxes_ok(boxes, B, Hp, Wp, h, w, false) || !photo_index_ok(photo_index, B, P))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (hw + kQuadChunk - 1) / kQuadChunk;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += kBoxFaces) {
        const int32_t n = B - b0 < kBoxFaces ? B - b0 : kBoxFaces;
        GroupIngestArgs g = {};
        g.boxes = box_args(boxes + 4 * b0, n);
        for (int32_t s = 0; s < n; ++s)
            g.photo[s] = photo_index[b0 + s];
        hipLaunchKernelGGL(group_ingest_kernel, dim3((uint32_t)n * chunks), dim3(kQuadLanes), 0, st, photo_u8, (uint32_t)h, (uint32_t)w,
                           (uint32_t)Wp, HWp, chunks, g, x_lo_out + (size_t)b0 * 3u * hw);
    }
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_fullres_composites_group_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                                int32_t mask_batch, int32_t P, int32_t B, int32_t L, int32_t Hp, int32_t Wp,
                                                const int32_t *boxes, const int32_t *photo_index, int32_t h, int32_t w, float floor,
                                                float detail_clamp, uint8_t *out_u8, void *stream)
{
    uint32_t HWp, hw, mask_stride;
    float lo;
    if (!boxes || !photo_index || B < 1 || !box_shape(P, Hp, Wp, h, w, HWp, hw) ||
        !fullres_operands(photo_u8, x_lo, rendered, mask_u8, out_u8, L, mask_batch, B, hw, detail_clamp, floor, mask_stride, lo) ||
        !anyboxes_ok(boxes, B, Hp, Wp, h, w, false) || !photo_index_ok(photo_index, B, P))
        return GCFR_ERR_INVALID_ARGUMENT;
    // out must not overlap the photographs
    const uintptr_t pa = (uintptr_t)photo_u8, pe = pa + (uintptr_t)P * 3u * HWp;
    const uintptr_t oa = (uintptr_t)out_u8, oe = oa + (uintptr_t)P * (uintptr_t)L * 3u * HWp;
    if (oa < pe && pa < oe)
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t chunks = (HWp + kQuadChunk - 1) / kQuadChunk;
    const bool vec = (uint32_t)Wp % 4u == 0 && aligned4(out_u8);
    hipStream_t st = (hipStream_t)stream;
    // the faces by photograph, within a photograph in ascending face index
    std::vector<int32_t> order((size_t)B);
    for (int32_t b = 0; b < B; ++b)
        order[(size_t)b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return photo_index[a] < photo_index[b]; });
    GroupArgs g = {};
    int32_t photos = 0, slots = 0, first = 0;                                      // the launch being filled
    auto add = [&](const int32_t *faces, int32_t n) {                              // one more photograph with these faces
        g.begin[photos] = slots;
        for (int32_t k = 0; k < n; ++k, ++slots) {
            const int32_t *bx = boxes + 4 * (size_t)faces[k];
            g.boxes.x0[slots] = bx[0], g.boxes.y0[slots] = bx[1], g.boxes.bw[slots] = bx[2], g.boxes.bh[slots] = bx[3];
            g.face[slots] = faces[k];
        }
        g.begin[++photos] = slots;
    };
    auto flush = [&](int32_t cont) {
        if (!photos)
            return;
        const uint8_t *ph = photo_u8 + (size_t)first * 3u * HWp;
        uint8_t *o = out_u8 + (size_t)first * (size_t)L * 3u * HWp;
        const dim3 grid((uint32_t)photos * chunks);
        with_flag(vec, [&](auto V) {
            hipLaunchKernelGGL((group_composites_kernel<decltype(V)::value>), grid, dim3(kQuadLanes), 0, st, ph, x_lo, rendered, mask_u8,
                               mask_stride, (uint32_t)L, (uint32_t)h, (uint32_t)w, (uint32_t)Wp, HWp, chunks, cont, floor, lo,
                               detail_clamp, g, o);
        });
        g = GroupArgs{};
        photos = slots = 0;
    };
    int32_t at = 0;
    for (int32_t q = 0; q < P; ++q) {
        int32_t n = 0;
        while (at + n < B && photo_index[order[(size_t)(at + n)]] == q)
            ++n;
        if (n > kBoxFaces || photos == kGroupPhotos || slots + n > kBoxFaces)
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
