// What the two full-resolution composites (gcfr_fullres.hip: bilinear Up; gcfr_fullres_guided.hip: joint-bilateral Up_J) share so
// that they cannot drift: the quotient, the blend and the byte of the statement (include/gcfr.h), the vector path's column
// offsets, and the host-side shape checks.
#pragma once

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

inline bool fullres_aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }
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

}  // namespace gcfr
