// The light-rig stage, gfx950: L weighted, coloured directional lights combined into ONE relit image per face.  It sits on the
// many-lights path's `final_shading` (B,L,H,W) -- what the march epilogue writes per light, T8:518 -- and on the albedo:
//   shading_rgb[b,c,p] = sum_l rgb[b,l,c] final[b,l,p]            rgb = colour x weight of light l, (B,L,3) or one rig (1,L,3)
//   rendered[b,c,p]    = albedo[b,c,p] shading_rgb[b,c,p]         (T8:519-522's composite with a coloured shading)
// as ONE forward launch and ONE backward launch, instead of a (B,L,3,H,W) product, its reduction and their autograd in ATen.
// Per pixel the forward reads 4 L + 12 bytes and writes 12 (rendered) or 24 (+ shading_rgb); the backward reads 4 L + up to 36
// and writes 4 L + 12.
//
// Arithmetic (the library is built with -ffp-contract=off: every product and sum below is one separately rounded IEEE f32
// operation): the l = 0 product initialises the accumulator (no add to zero), lights 1 .. L-1 follow in ascending order as
// acc = acc + rgb[l,c] final[l], the albedo product comes last.  Nothing is clamped; non-finite values propagate.
// Backward, u[c] = g_shading_rgb[c] + g_rendered[c] albedo[c] (an absent term is not formed):
//   g_final[l]  = (rgb[l,0] u[0] + rgb[l,1] u[1]) + rgb[l,2] u[2]      g_albedo[c] = g_rendered[c] shading_rgb[c] (recomputed)
//   g_rgb[l,c] += sum_p final[l,p] u[c,p]                               in f64, as gcfr_render_bwd's grad_light_pt / grad_ambient
//
// Work split: a workgroup of 256 lanes owns chunks of kRigChunk = 1024 consecutive pixels of ONE face, four pixels per lane
// (gcfr_reduce.hpp: quad_load / quad_store), and a lane walks the L lights in order.  When H W is a multiple of four and every
// plane pointer is 16-byte aligned, every plane is read and written with 16-byte accesses (all planes of all lights and channels
// keep the alignment, their strides being multiples of H W); otherwise (an odd H W misaligns the second albedo plane and every
// second light) with 4-byte accesses.  The face, hence the rig, is the same for the whole workgroup: the 3 L rig values are read
// through wave-uniform addresses.
// g_rgb: per light a lane adds its four products in f64, the wave reduces the three sums through an xor-shuffle tree, lane 0 adds
// them (LDS f64 atomic) to the workgroup's accumulators, kRigLightTile lights at a time; a workgroup walks several chunks of its
// face (the grid is capped near four workgroups per CU) and adds its accumulators to g_rgb with one global f64 atomic per entry at
// the end (rigs longer than the tile: per chunk and tile).  The order of these f64 additions is the only freedom in the results.
#include "gcfr_device.hpp"
#include "gcfr_reduce.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kRigLanes = kQuadLanes;
constexpr int kRigChunk = kQuadChunk;         // pixels per workgroup and step (gcfr_reduce.hpp: four per lane)
constexpr int kRigLightTile = 1024;           // lights whose g_rgb partial sums a workgroup keeps in LDS (24 KiB)
constexpr int kRigMaxLights = 4096;
constexpr uint32_t kRigBwdGroups = 1024;      // the backward's grid is capped near this many workgroups (four per CU)

template <bool VEC>
__global__ __launch_bounds__(kRigLanes) void light_rig_fwd_kernel(
    const float *__restrict__ final_shading, const float *__restrict__ albedo, const float *__restrict__ rgb, uint32_t rgb_stride,
    uint32_t L, uint32_t HW, uint32_t chunks, float *__restrict__ rendered, float *__restrict__ shading_rgb)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kRigChunk);
    const float *rig = rgb + (size_t)b * rgb_stride;
    const float *fb = final_shading + (size_t)b * L * HW;
    const size_t plane3 = (size_t)b * 3u * HW;
    float al[3][4], f[4], acc[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        quad_load<VEC>(albedo + plane3 + (size_t)c * HW, q, HW, al[c]);
    quad_load<VEC>(fb, q, HW, f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = rig[c];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            acc[c][k] = r * f[k];
    }
#pragma unroll 4
    for (uint32_t l = 1; l < L; ++l) {
        quad_load<VEC>(fb + (size_t)l * HW, q, HW, f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = rig[3u * l + c];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                acc[c][k] = acc[c][k] + r * f[k];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (shading_rgb)
            quad_store<VEC>(shading_rgb + plane3 + (size_t)c * HW, q, HW, acc[c]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            al[c][k] = al[c][k] * acc[c][k];
        quad_store<VEC>(rendered + plane3 + (size_t)c * HW, q, HW, al[c]);
    }
}

// the workgroup's accumulators of `n` (light, channel) entries to g_rgb (+=), and back to zero; between two barriers of the caller
__device__ inline void rig_flush(double *sAcc, double *__restrict__ dst, uint32_t n)
{
    for (uint32_t i = threadIdx.x; i < n; i += kRigLanes) {
        atomicAdd(dst + i, sAcc[i]);
        sAcc[i] = 0.0;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kRigLanes) void light_rig_bwd_kernel(
    const float *__restrict__ final_shading, const float *__restrict__ albedo, const float *__restrict__ rgb, uint32_t rgb_stride,
    uint32_t L, uint32_t HW, uint32_t chunks, uint32_t groups, const float *__restrict__ g_rendered,
    const float *__restrict__ g_shading_rgb, float *__restrict__ g_final, float *__restrict__ g_albedo, double *__restrict__ g_rgb)
{
    __shared__ double sAcc[3 * kRigLightTile];
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x / groups, j = blockIdx.x - b * groups;           // (uniform)
    const float *rig = rgb + (size_t)b * rgb_stride;
    const float *fb = final_shading + (size_t)b * L * HW;
    float *gfb = g_final ? g_final + (size_t)b * L * HW : nullptr;
    double *grig = g_rgb ? g_rgb + (size_t)b * rgb_stride : nullptr;               // (the shared rig: every face adds to the same entries)
    const size_t plane3 = (size_t)b * 3u * HW;
    const bool want_sh = g_albedo != nullptr && g_rendered != nullptr;             // (uniform, like every pointer test below)
    const bool tiled = L > (uint32_t)kRigLightTile;
    if (grig) {
        for (uint32_t i = tid; i < 3u * (uint32_t)kRigLightTile; i += kRigLanes)
            sAcc[i] = 0.0;
        __syncthreads();
    }
    for (uint32_t ch = j; ch < chunks; ch += groups) {                             // (uniform trip count: the barriers below are safe)
        const uint32_t q = quad_first<VEC>(ch * (uint32_t)kRigChunk);
        float u[3][4], gr[3][4], sh[3][4], f[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t off = plane3 + (size_t)c * HW;
            if (g_rendered) {
                float al[4];
                quad_load<VEC>(g_rendered + off, q, HW, gr[c]);
                quad_load<VEC>(albedo + off, q, HW, al);
                if (g_shading_rgb) {
                    quad_load<VEC>(g_shading_rgb + off, q, HW, u[c]);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        u[c][k] = u[c][k] + gr[c][k] * al[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        u[c][k] = gr[c][k] * al[k];
                }
            } else {
                quad_load<VEC>(g_shading_rgb + off, q, HW, u[c]);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    gr[c][k] = 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                sh[c][k] = 0.0f;
        }
        for (uint32_t t0 = 0; t0 < L; t0 += (uint32_t)kRigLightTile) {
            const uint32_t t1 = L - t0 < (uint32_t)kRigLightTile ? L : t0 + (uint32_t)kRigLightTile;
            for (uint32_t l = t0; l < t1; ++l) {
                quad_load<VEC>(fb + (size_t)l * HW, q, HW, f);
                const float r0 = rig[3u * l], r1 = rig[3u * l + 1u], r2 = rig[3u * l + 2u];
                const float r[3] = {r0, r1, r2};
                if (want_sh) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float t = r[c] * f[k];
                            sh[c][k] = l == 0 ? t : sh[c][k] + t;                  // the first product initialises
                        }
                }
                if (gfb) {
                    float g[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        g[k] = r0 * u[0][k];
                        g[k] = g[k] + r1 * u[1][k];
                        g[k] = g[k] + r2 * u[2][k];
                    }
                    quad_store<VEC>(gfb + (size_t)l * HW, q, HW, g);
                }
                if (grig) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double s = (double)f[0] * (double)u[c][0];                 // (a product of two f32 is exact in f64)
                        s += (double)f[1] * (double)u[c][1];
                        s += (double)f[2] * (double)u[c][2];
                        s += (double)f[3] * (double)u[c][3];
                        s = wave_sum_f64(s);
                        if ((tid & 63u) == 0)
                            atomicAdd(&sAcc[3u * (l - t0) + (uint32_t)c], s);
                    }
                }
            }
            if (grig && tiled) {
                __syncthreads();
                rig_flush(sAcc, grig + 3u * (size_t)t0, 3u * (t1 - t0));
                __syncthreads();
            }
        }
        if (g_albedo) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float ga[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    ga[k] = gr[c][k] * sh[c][k];                                   // (no g_rendered: 0 * 0)
                quad_store<VEC>(g_albedo + plane3 + (size_t)c * HW, q, HW, ga);
            }
        }
    }
    if (grig && !tiled) {
        __syncthreads();
        rig_flush(sAcc, grig, 3u * L);
    }
}

inline bool rig_shape_ok(int32_t B, int32_t L, int32_t H, int32_t W, int32_t rgb_batch)
{
    if (B < 1 || L < 1 || L > kRigMaxLights || H < 1 || W < 1 || (rgb_batch != 1 && rgb_batch != B))
        return false;
    const uint64_t HW = (uint64_t)H * (uint64_t)W;
    if (HW > 0x7fffffffull)
        return false;
    return (uint64_t)B * ((HW + kRigChunk - 1) / kRigChunk) <= 0x7fffffffull;      // one workgroup per face and chunk fits the grid
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_light_rig_fwd(const float *final_shading, const float *albedo, const float *rgb, int32_t rgb_batch, int32_t B,
                                  int32_t L, int32_t H, int32_t W, float *rendered, float *shading_rgb, void *stream)
{
    if (!final_shading || !albedo || !rgb || !rendered || !rig_shape_ok(B, L, H, W, rgb_batch))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t HW = (uint32_t)H * (uint32_t)W, chunks = (HW + kRigChunk - 1) / kRigChunk;
    const uint32_t stride = rgb_batch == 1 ? 0u : 3u * (uint32_t)L;
    const bool vec = quad_vec_ok(HW, final_shading, albedo, rendered, shading_rgb);
    const dim3 grid((uint32_t)B * chunks), block(kRigLanes);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(light_rig_fwd_kernel<true>, grid, block, 0, st, final_shading, albedo, rgb, stride, (uint32_t)L, HW, chunks,
                           rendered, shading_rgb);
    else
        hipLaunchKernelGGL(light_rig_fwd_kernel<false>, grid, block, 0, st, final_shading, albedo, rgb, stride, (uint32_t)L, HW, chunks,
                           rendered, shading_rgb);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_light_rig_bwd(const float *final_shading, const float *albedo, const float *rgb, int32_t rgb_batch, int32_t B,
                                  int32_t L, int32_t H, int32_t W, const float *g_rendered, const float *g_shading_rgb,
                                  float *g_final, float *g_albedo, double *g_rgb, void *stream)
{
    if (!final_shading || !albedo || !rgb || (!g_rendered && !g_shading_rgb) || (!g_final && !g_albedo && !g_rgb) ||
        ((uintptr_t)g_rgb & 7u) || !rig_shape_ok(B, L, H, W, rgb_batch))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t HW = (uint32_t)H * (uint32_t)W, chunks = (HW + kRigChunk - 1) / kRigChunk;
    const uint32_t stride = rgb_batch == 1 ? 0u : 3u * (uint32_t)L;
    uint32_t groups = (kRigBwdGroups + (uint32_t)B - 1) / (uint32_t)B;             // workgroups per face
    groups = groups > chunks ? chunks : groups;
    const bool vec = quad_vec_ok(HW, final_shading, albedo, g_rendered, g_shading_rgb, g_final, g_albedo);
    const dim3 grid((uint32_t)B * groups), block(kRigLanes);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(light_rig_bwd_kernel<true>, grid, block, 0, st, final_shading, albedo, rgb, stride, (uint32_t)L, HW, chunks,
                           groups, g_rendered, g_shading_rgb, g_final, g_albedo, g_rgb);
    else
        hipLaunchKernelGGL(light_rig_bwd_kernel<false>, grid, block, 0, st, final_shading, albedo, rgb, stride, (uint32_t)L, HW, chunks,
                           groups, g_rendered, g_shading_rgb, g_final, g_albedo, g_rgb);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
