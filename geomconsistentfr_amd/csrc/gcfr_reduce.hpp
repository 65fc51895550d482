// Device primitives shared by the fused heads (gcfr_losses.hip, gcfr_supervised_losses.hip, gcfr_light_rig.hip, gcfr_rig_frames.hip), the
// full-resolution composites (gcfr_fullres.hpp) and the metrics of gcfr_dataset.hip: the fixed-order f64 sums, the four-pixels-per-lane
// access and, for the composites, a lane's 12 bytes of four uint8 RGB pixels.  (gcfr_backward.hip keeps its own DPP
// reductions, whose totals live in lane 0 only.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gcfr {

// The sum of a wave's 64 values, in every lane: the xor-shuffle tree, off = 32 .. 1.
__device__ inline double wave_sum_f64(double v)
{
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off);
    return v;
}

// The sums of K doubles per lane over a workgroup of 256 lanes: `__shared__ BlockSum<K> red; red.reduce(vals);`, then any lane
// reads red.total(k).  THE ORDER OF ADDITION IS A CONTRACT: each wave's xor tree above, then the four waves as
// (w0 + w1) + (w2 + w3).  With a fixed order inside each lane (every caller adds its items in ascending order) and no
// floating-point atomic, two calls on the same inputs return the same bits -- what both loss heads promise (include/gcfr.h) and
// their tests pin.  reduce() ends with the workgroup's barrier, so every lane must call it.
template <int K>
struct BlockSum {
    double w[4][K];                                   // [wave][k]

    __device__ void reduce(const double (&v)[K])
    {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double s = wave_sum_f64(v[k]);
            if (lane == 0)
                w[wave][k] = s;
        }
        __syncthreads();
    }
    __device__ double total(uint32_t k) const { return (w[0][k] + w[1][k]) + (w[2][k] + w[3][k]); }
};

// Four pixels per lane: a workgroup of kQuadLanes lanes owns kQuadChunk consecutive pixels of a range of n.  VEC (n % 4 == 0 and
// every plane 16-byte aligned, quad_vec_ok below): lane t owns pixels 4 t .. 4 t + 3 of the chunk and moves them as one 16-byte
// access per plane, all four in range or none.  Otherwise lane t owns pixels t, t + 256, t + 512, t + 768, each a checked 4-byte
// access.  Pixels out of range read as 0 and are not written.
constexpr int kQuadLanes = 256;
constexpr int kQuadChunk = 4 * kQuadLanes;

// the lane's first pixel in the chunk that starts at `chunk0`, and its pixel k
template <bool VEC>
__device__ inline uint32_t quad_first(uint32_t chunk0) { return chunk0 + (VEC ? 4u * threadIdx.x : threadIdx.x); }
template <bool VEC>
__device__ inline uint32_t quad_pixel(uint32_t q, int k) { return q + (uint32_t)(VEC ? k : k * kQuadLanes); }

template <bool VEC>
__device__ inline void quad_load(const float *__restrict__ plane, uint32_t q, uint32_t n, float (&v)[4])
{
    if (VEC) {
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q < n)
            t = *reinterpret_cast<const float4 *>(plane + q);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t p = quad_pixel<false>(q, k);
            v[k] = p < n ? plane[p] : 0.0f;
        }
    }
}

template <bool VEC>
__device__ inline void quad_store(float *__restrict__ plane, uint32_t q, uint32_t n, const float (&v)[4])
{
    if (VEC) {
        if (q < n)
            *reinterpret_cast<float4 *>(plane + q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t p = quad_pixel<false>(q, k);
            if (p < n)
                plane[p] = v[k];
        }
    }
}

// A lane's four pixels of three interleaved uint8 channels are 12 consecutive bytes, three dwords: byte 3 k + c is channel c of
// pixel k.  The pair below turns the dwords into p[k][c] and packs `byte_of(k, c)` (-> uint8_t) into them, a channel at a time (the
// order the full-resolution composites were measured with; gcfr_rig_frames.hip packs a pixel at a time and keeps its own loop:
// through this one its vector kernel came out seven instructions longer).
__device__ inline void quad_unpack_u8x3(const uint32_t (&w3)[3], float (&p)[4][3])
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int i = 3 * k + c;
            p[k][c] = (float)(uint8_t)(w3[i / 4] >> (8 * (i % 4)));
        }
}

template <class F>
__device__ inline void quad_pack_u8x3(uint32_t (&o)[3], F byte_of)
{
    o[0] = o[1] = o[2] = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = 3 * k + c;
            o[i / 4] |= (uint32_t)byte_of(k, c) << (8 * (i % 4));
        }
}

inline bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// may the planes of HW pixels each behind these pointers be moved 16 bytes at a time?  (an absent plane, NULL, counts as aligned)
template <class... P>
inline bool quad_vec_ok(uint32_t HW, const P *...planes)
{
    return HW % 4u == 0 && (aligned16(planes) && ...);
}

}  // namespace gcfr
