// What the four full-resolution composites share so that they cannot drift (gcfr_fullres.hip: bilinear Up; gcfr_fullres_guided.hip:
// joint-bilateral Up_J; gcfr_fullres_box.hip: bilinear Up over a face box; gcfr_fullres_box_guided.hip: Up_J over a face box).
// include/gcfr.h is the statement; here is its ONE text:
//   arithmetic   bilerp, detail_of (the quotient), fullres_value (the blend), fullres_byte (the byte), guided_range (Up_J's range
//                kernel)
//   vector path  the 12-byte lane's select mask and its select-and-store (the pack / unpack pair is gcfr_reduce.hpp's), the
//                column offsets kP0 of a lane's four pixels, load_dword_any (a box starts at any byte) and PlaneF32 (a plane of
//                `rendered` behind a buffer descriptor)
//   scalar path  composite_pixel: the whole pixel, over an upsampler object whose one operation is up(value_at); Bilinear4 is the
//                upsampler of both bilinear kernels, filled from up_tap<S> or from box_tap; Guided16 that of both guided kernels,
//                filled from guided_tap<S> or from box_tap4
//   per face     FacePlanes / face_planes: the five base pointers of a workgroup's face; BoxArgs: the boxes of a launch, by value;
//                box_clamp: a photograph coordinate in a box's frame
//   host         the shape checks, the operand check of the composite entries, the box rules (boxes_ok, box_shape, box_args), and
//                with_scale / with_flag, which turn the run-time (s, vec) into template arguments
// The vector-path upsamplers and the tap functions (up_tap<S>, guided_tap<S>: shifts; box_tap, box_tap4: divisions) stay with
// their kernels.
// gcfr_fullres_anybox.hip (a box smaller than the network's input on either axis) is a fifth user: the same arithmetic, vector-path
// pieces, composite_pixel (over its own carrier, AnyCarrier) and per-face pieces, and the relaxed box rules anyboxes_ok below.
// gcfr_fullres_group.hip (every face of a photograph in one launch) is a sixth: that carrier (gcfr_fullres_anybox.hpp) over the
// same arithmetic, with the running bytes in the place of the photograph's.
// gcfr_fullres_affine.hip (a rotated face under a 2 x 3 affine map) is a seventh: the same arithmetic, vector-path pieces,
// composite_pixel (over its own carrier, AffineCarrier), per-face pieces, box_shape and fullres_operands; its maps travel in a
// block of its own (AffineArgs) with kBoxFaces faces per launch.
// gcfr_fullres_group_affine.hip (every TILTED face of a photograph in one launch) is an eighth: that carrier and those maps
// (gcfr_fullres_affine.hpp) over the same arithmetic, with the running bytes in the place of the photograph's.
#pragma once

#include <type_traits>

#include "gcfr_composite.hpp"
#include "gcfr_reduce.hpp"

namespace gcfr {

constexpr int kFullresMaxLights = 4096;        // the image kernel's limit

template <int S>
constexpr int log2_of() { return S == 1 ? 0 : S == 2 ? 1 : S == 4 ? 2 : 3; }
// the vector path (a lane's four pixels x .. x + 3, x a multiple of four): pixel k's x0 = floor((2 (x + k) + 1 - S) / (2 S))
// less pixel 0's
template <int S>
constexpr int kP0(int k) { return S == 1 ? k : S == 2 ? (k + 1) / 2 : S == 4 ? k / 2 : 0; }

// Up from its four taps: horizontal first on both rows, then vertical
__device__ inline float bilerp(float a00, float a01, float a10, float a11, float tx, float ty)
{
    const float top = a00 + tx * (a01 - a00);
    const float bot = a10 + tx * (a11 - a10);
    return top + ty * (bot - top);
}

__device__ inline float detail_of(float p, float xl_up, float floor, float lo, float hi)
{
    const float xl = xl_up * 255.0f;
    return fminf(fmaxf(p / fmaxf(xl, floor), lo), hi);
}

// v of the statement, and the byte where the mask is not zero
__device__ inline float fullres_value(float p, float m, float d, float r_up)
{
    const float r = r_up * 255.0f;
    return p + m * (r * d - p);
}

__device__ inline uint8_t fullres_byte(uint8_t photo, float p, float m, float d, float r_up)
{
    return m > 0.0f ? quantise_u8((double)fullres_value(p, m, d, r_up)) : photo;
}

// The vector path's 12 bytes (gcfr_reduce.hpp: quad_unpack_u8x3 / quad_pack_u8x3).  sel: the bytes of the three dwords whose pixel
// is relit, formed once per lane; then per light `byte_of(k, c)` where sel is set and the photograph's own byte w3 elsewhere.
__device__ inline void quad_select_mask(const bool (&relit)[4], uint32_t (&sel)[3])
{
    sel[0] = sel[1] = sel[2] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int i = 3 * k + c;
            sel[i / 4] |= relit[k] ? 0xffu << (8 * (i % 4)) : 0u;
        }
}

template <class F>
__device__ inline void quad_store_selected(uint8_t *dst, const uint32_t (&w3)[3], const uint32_t (&sel)[3], F byte_of)
{
    uint32_t o[3];
    quad_pack_u8x3(o, byte_of);
    uint32_t *ow = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        ow[j] = (o[j] & sel[j]) | (w3[j] & ~sel[j]);
}

// the base pointers of face b: PN the photograph's pixels per face, WN the output window's (the same but for a box)
struct FacePlanes {
    const uint8_t *photo;                          // (PN,3)
    const float *x_lo;                             // (h,w,3)
    const uint8_t *mask;                           // (h,w)
    const float *rendered;                         // (L,3,h,w)
    uint8_t *out;                                  // (L,WN,3)
};

__device__ inline FacePlanes face_planes(const uint8_t *photo, const float *x_lo, const float *rendered, const uint8_t *mask,
                                         uint8_t *out, uint32_t b, uint32_t mask_stride, uint32_t L, uint32_t hw, uint32_t PN,
                                         uint32_t WN)
{
    return {photo + (size_t)b * 3u * PN, x_lo + (size_t)b * 3u * hw, mask + (size_t)b * mask_stride,
            rendered + (size_t)b * L * 3u * hw, out + (size_t)b * L * 3u * WN};
}

// the bilinear upsampler of one pixel: Up of the plane whose value at low-resolution pixel t is value_at(t)
struct Bilinear4 {
    uint32_t t00, t01, t10, t11;
    float tx, ty;
    __device__ Bilinear4(uint32_t y0, uint32_t y1, uint32_t x0, uint32_t x1, uint32_t w, float tx_, float ty_)
        : t00(y0 * w + x0), t01(y0 * w + x1), t10(y1 * w + x0), t11(y1 * w + x1), tx(tx_), ty(ty_) {}
    template <class V>
    __device__ float operator()(V value_at) const
    {
        return bilerp(value_at(t00), value_at(t01), value_at(t10), value_at(t11), tx, ty);
    }
};

// The scalar path: pixel px of face f's window of WN pixels, whose photograph bytes are pb, for all L lights, one element at a
// time: d and m once, then per light the byte.
template <class Up>
__device__ inline void composite_pixel(const Up &up, const uint8_t (&pb)[3], const FacePlanes &f, uint32_t L, uint32_t hw,
                                       uint32_t WN, uint32_t px, float floor, float lo, float hi)
{
    float p[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p[c] = (float)pb[c];
        d[c] = detail_of(p[c], up([&](uint32_t t) { return f.x_lo[3u * (size_t)t + c]; }), floor, lo, hi);
    }
    const float m = up([&](uint32_t t) { return mask_quotient_f32(f.mask[t]); });
    for (uint32_t l = 0; l < L; ++l) {
        const float *re_l = f.rendered + (size_t)l * 3u * hw;
        uint8_t *o = f.out + 3u * ((size_t)l * WN + px);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *plane = re_l + (size_t)c * hw;
            o[c] = fullres_byte(pb[c], p[c], m, d[c], up([&](uint32_t t) { return plane[t]; }));
        }
    }
}

// the range kernel's weight of one tap
__device__ inline float guided_range(const float (&p)[3], float x0, float x1, float x2, float inv)
{
    const float e0 = p[0] - x0 * 255.0f, e1 = p[1] - x1 * 255.0f, e2 = p[2] - x2 * 255.0f;
    const float d2 = (e0 * e0 + e1 * e1) + e2 * e2;
    return 1.0f / (1.0f + d2 * inv);
}

// the joint-bilateral upsampler of one pixel (the scalar path): the 16 taps and their normalised weights, row-major; Up_J of the
// plane whose value at low-resolution pixel t is value_at(t)
struct Guided16 {
    uint32_t tap[16];
    float wn[16];
    template <class V>
    __device__ float operator()(V value_at) const
    {
        float acc = wn[0] * value_at(tap[0]);
#pragma unroll
        for (int t = 1; t < 16; ++t)
            acc = acc + wn[t] * value_at(tap[t]);
        return acc;
    }
};

// the boxes of one launch of a box kernel, by value in its argument block
constexpr int kBoxFaces = 32;                  // faces per launch: 4 x 32 int32 in the argument block

struct BoxArgs {
    int32_t x0[kBoxFaces], y0[kBoxFaces], bw[kBoxFaces], bh[kBoxFaces];
};

// box-relative coordinate of photograph coordinate p for a box that starts at b0 and is nb long, clamped into the box
__device__ inline uint32_t box_clamp(int32_t p, int32_t b0, int32_t nb, bool &in)
{
    const int32_t r = p - b0;
    in = r >= 0 && r < nb;
    return (uint32_t)(r < 0 ? 0 : r < nb ? r : nb - 1);
}

// A plane of n floats (4 n < 2^32) behind a buffer descriptor: a load is the plane's uniform descriptor plus ONE 32-bit register of
// byte offset per lane, where a flat load holds a 64-bit address per tap (48 of them per light, each advanced per light).
struct PlaneF32 {
    __amdgpu_buffer_rsrc_t rs;
    __device__ PlaneF32(const float *plane, uint32_t n)
        : rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(plane), 0, (int)(4u * n), 0x00020000)) {}
    __device__ float at(uint32_t byte_offset) const
    {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)byte_offset, 0, 0));
    }
};

__device__ inline uint32_t load_dword_any(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

inline bool fullres_scale_ok(int32_t s) { return s == 1 || s == 2 || s == 4 || s == 8; }

// (B, h, w, s) -> the hi-res and the low-res pixel counts per face; false where a per-face pixel count or a chunk count does not
// fit 31 bits
inline bool fullres_shape(int32_t B, int32_t h, int32_t w, int32_t s, uint32_t &HW, uint32_t &hw)
{
    if (B < 1 || h < 1 || w < 1 || !fullres_scale_ok(s))
        return false;
    const uint64_t hw64 = (uint64_t)h * (uint64_t)w, HW64 = hw64 * (uint64_t)(s * s);
    if (hw64 > 0x7fffffffull || HW64 > 0x7fffffffull || (uint64_t)w * (uint64_t)s > 0x7fffffffull ||
        (uint64_t)B * ((HW64 + kQuadChunk - 1) / kQuadChunk) > 0x7fffffffull)
        return false;
    HW = (uint32_t)HW64, hw = (uint32_t)hw64;
    return true;
}

// the operands every composite entry takes, for B faces of hw low-resolution pixels -> the mask's stride per face and the lower
// clamp of d; false where one is refused
inline bool fullres_operands(const void *photo, const void *x_lo, const void *rendered, const void *mask, const void *out, int32_t L,
                             int32_t mask_batch, int32_t B, uint32_t hw, float detail_clamp, float floor, uint32_t &mask_stride,
                             float &lo)
{
    if (!photo || !x_lo || !rendered || !mask || !out || L < 1 || L > kFullresMaxLights || (mask_batch != 1 && mask_batch != B) ||
        !(detail_clamp >= 1.0f) || !(floor > 0.0f))
        return false;
    mask_stride = mask_batch == 1 ? 0u : hw;
    lo = 1.0f / detail_clamp;
    return true;
}

// The box rules of include/gcfr.h for `n` faces; with `same` every box has the first one's size.
inline bool boxes_ok(const int32_t *boxes, int32_t n, int32_t Hp, int32_t Wp, int32_t h, int32_t w, bool same)
{
    for (int32_t b = 0; b < n; ++b) {
        const int64_t x0 = boxes[4 * b], y0 = boxes[4 * b + 1], bw = boxes[4 * b + 2], bh = boxes[4 * b + 3];
        if (x0 < 0 || y0 < 0 || bw < w || bh < h || x0 + bw > Wp || y0 + bh > Hp || 2 * bh * h > 0x7fffffffll ||
            2 * bw * w > 0x7fffffffll)
            return false;
        if (same && (bw != boxes[2] || bh != boxes[3]))
            return false;
    }
    return true;
}

// The relaxed box rules of include/gcfr.h (gcfr_fullres_anybox.hip): boxes_ok with `bw >= w, bh >= h` replaced by `bw, bh >= 1 and
// 8 bw >= w, 8 bh >= h`.
inline bool anyboxes_ok(const int32_t *boxes, int32_t n, int32_t Hp, int32_t Wp, int32_t h, int32_t w, bool same)
{
    for (int32_t b = 0; b < n; ++b) {
        const int64_t x0 = boxes[4 * b], y0 = boxes[4 * b + 1], bw = boxes[4 * b + 2], bh = boxes[4 * b + 3];
        if (x0 < 0 || y0 < 0 || bw < 1 || bh < 1 || 8 * bw < w || 8 * bh < h || x0 + bw > Wp || y0 + bh > Hp ||
            2 * bh * h > 0x7fffffffll || 2 * bw * w > 0x7fffffffll)
            return false;
        if (same && (bw != boxes[2] || bh != boxes[3]))
            return false;
    }
    return true;
}

// (B, Hp, Wp, h, w) -> the photograph's and the network's pixel counts; false where a count does not fit 31 bits
inline bool box_shape(int32_t B, int32_t Hp, int32_t Wp, int32_t h, int32_t w, uint32_t &HWp, uint32_t &hw)
{
    if (B < 1 || Hp < 1 || Wp < 1 || h < 1 || w < 1)
        return false;
    const uint64_t HW64 = (uint64_t)Hp * (uint64_t)Wp, hw64 = (uint64_t)h * (uint64_t)w;
    if (HW64 > 0x7fffffffull || hw64 > 0x7fffffffull || (uint64_t)B * ((HW64 + kQuadChunk - 1) / kQuadChunk) > 0x7fffffffull)
        return false;
    HWp = (uint32_t)HW64, hw = (uint32_t)hw64;
    return true;
}

inline BoxArgs box_args(const int32_t *boxes, int32_t n)
{
    BoxArgs a = {};
    for (int32_t f = 0; f < n; ++f)
        a.x0[f] = boxes[4 * f], a.y0[f] = boxes[4 * f + 1], a.bw[f] = boxes[4 * f + 2], a.bh[f] = boxes[4 * f + 3];
    return a;
}

// f(std::integral_constant<int, S>{}) for the scale s (fullres_scale_ok), f(std::bool_constant<v>{}) for a flag: a kernel's
// template arguments from run-time values, so that an entry names its kernel and its arguments once
template <class F>
inline void with_scale(int32_t s, F f)
{
    switch (s) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

template <class F>
inline void with_flag(bool v, F f)
{
    if (v)
        f(std::true_type{});
    else
        f(std::false_type{});
}

}  // namespace gcfr
