// Environment-map lighting, gfx950: a lat-long radiance map (E,He,We,3) integrated into the colour x weight per light that the
// light-rig stage (gcfr_light_rig.hip) takes.  Every texel belongs to the light direction nearest to it (its `cell`); a light's
// rgb is the solid-angle-weighted sum of its cell's texels.  Three launches, none of which evaluates a transcendental function:
// all trigonometry arrives in host-built tables (rows: sin / cos of the row's polar angle, cols: sin / cos of the column's
// azimuth, row_w: the row's solid-angle weight per texel), the way t_table and the SSIM window do.
//
//   cells    one lane = one texel.  omega = (sin_t sin_p, cos_t, sin_t cos_p); best = -inf, cell = -1; for l ascending
//            s = (omega_x d_x + omega_y d_y) + omega_z d_z, `if (s > best) { best = s; cell = l; }` (a tie keeps the lowest index,
//            a NaN score never wins); afterwards `if (!(best >= min_cos)) cell = -1`.  Every product and sum is one IEEE f32
//            operation (the library is built with -ffp-contract=off).  The light index is the same for every lane, so the three
//            components of a direction are read through wave-uniform addresses: scalar loads into SGPRs, which the multiplies take
//            as operands directly -- no LDS, no barrier, no per-lane load in the loop.
//   forward  one workgroup of 256 lanes per (map e, light l).  Lane i walks texels i, i + 256, ... in ascending order and adds
//            (double)env[e,t,c] * row_w[row(t)] for the texels of cell l to its three f64 sums (the products and sums are f64
//            operations, unfused); BlockSum<3> (gcfr_reduce.hpp) adds the 256 lanes' sums in its fixed order: each wave's xor
//            tree, then (w0 + w1) + (w2 + w3).  Lanes 0 .. 2 round the three totals to f32 and store them.  No floating-point
//            atomic; every element of rgb is written exactly once; an empty cell gives +0; two calls return the same bits.
//   frames   gcfr_environment_cells_frames / gcfr_environment_fwd_frames: F direction sets (a turntable's rotations) -> F cell maps
//            -> rgb (E,F,L,3) in one launch each, the frame riding in a grid dimension.  Per frame they run the SAME device
//            functions as the two kernels above (env_texel_cell, env_cell_sums): frame f is those kernels on dirs_map[f], bit for bit.
//   backward a gather, one lane = one float of g_env: g_env[e,t,c] = (float)row_w[row(t)] * g_rgb[e,cell[t],c], one f32 product;
//            +0 where cell[t] = -1.  There is no gradient with respect to the directions: the cell map is piecewise constant.
//
// Bytes (He We = T texels): cells reads 8 (He + We) + 12 L and writes 4 T; the forward reads, per (e, l), 4 T of cells plus the
// 12 bytes of each texel it owns, in all 4 E L T + 12 E T, and writes 12 E L; the backward reads 4 T per channel plane of cells
// (cached) + 12 E L and writes 12 E T.  At the usual sizes (64 x 128 texels, 64 lights: 32 KiB of cells, 96 KiB of radiance)
// all three are latency-bound.
#include "gcfr_reduce.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kEnvLanes = 256;
constexpr int kEnvMaxLights = 4096;
constexpr uint32_t kEnvMaxTexels = 1u << 24;
constexpr int kEnvMaxMaps = 65535;            // E rides in blockIdx.y
constexpr int kEnvMaxFrames = 4096;           // F rides in blockIdx.y (cells) / blockIdx.z (integration)

// the cell of texel t under the L directions `dirs`: the per-texel score loop of the cell map, shared by both of its kernels
__device__ inline int32_t env_texel_cell(const float *__restrict__ rows, const float *__restrict__ cols,
                                         const float *__restrict__ dirs, uint32_t We, uint32_t L, float min_cos, uint32_t t)
{
    const uint32_t r = t / We, c = t - r * We;
    const float sin_t = rows[2u * r], cos_t = rows[2u * r + 1u];
    const float ox = sin_t * cols[2u * c], oy = cos_t, oz = sin_t * cols[2u * c + 1u];
    float best = -__builtin_huge_valf();
    int32_t cell = -1;
#pragma unroll 4                                                                   // (four lights' scalar loads in flight at a time)
    for (uint32_t l = 0; l < L; ++l) {                                             // (uniform: the three loads are scalar)
        const float dx = dirs[3u * l], dy = dirs[3u * l + 1u], dz = dirs[3u * l + 2u];
        const float s = (ox * dx + oy * dy) + oz * dz;
        if (s > best) {
            best = s;
            cell = (int32_t)l;
        }
    }
    if (!(best >= min_cos))
        cell = -1;
    return cell;
}

__global__ __launch_bounds__(kEnvLanes) void environment_cells_kernel(
    const float *__restrict__ rows, const float *__restrict__ cols, const float *__restrict__ dirs, uint32_t We, uint32_t T,
    uint32_t L, float min_cos, int32_t *__restrict__ cell_out)
{
    const uint32_t t = blockIdx.x * (uint32_t)kEnvLanes + threadIdx.x;
    if (t >= T)
        return;
    cell_out[t] = env_texel_cell(rows, cols, dirs, We, L, min_cos, t);
}

// F direction sets (F,L,3) -> F cell maps (F,He,We) in one launch: the frame rides in blockIdx.y (uniform)
__global__ __launch_bounds__(kEnvLanes) void environment_cells_frames_kernel(
    const float *__restrict__ rows, const float *__restrict__ cols, const float *__restrict__ dirs, uint32_t We, uint32_t T,
    uint32_t L, float min_cos, int32_t *__restrict__ cell_out)
{
    const uint32_t t = blockIdx.x * (uint32_t)kEnvLanes + threadIdx.x, f = blockIdx.y;
    if (t >= T)
        return;
    cell_out[(size_t)f * T + t] = env_texel_cell(rows, cols, dirs + (size_t)f * 3u * L, We, L, min_cos, t);
}

// the three f64 sums of cell l of one map, in every lane's red.total(c) afterwards: the lane walk and the workgroup's fixed-order
// sum, shared by both integration kernels.  Ends with the workgroup's barrier: every lane calls it.
__device__ inline void env_cell_sums(BlockSum<3> &red, const float *__restrict__ map, const double *__restrict__ row_w,
                                     const int32_t *__restrict__ cell, uint32_t We, uint32_t T, uint32_t l)
{
    double acc[3] = {0.0, 0.0, 0.0};
    for (uint32_t t = threadIdx.x; t < T; t += (uint32_t)kEnvLanes) {
        if (cell[t] != (int32_t)l)
            continue;
        const double w = row_w[t / We];
        const float *px = map + 3u * (size_t)t;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            acc[c] = acc[c] + (double)px[c] * w;
    }
    red.reduce(acc);
}

__global__ __launch_bounds__(kEnvLanes) void environment_fwd_kernel(
    const float *__restrict__ env, const double *__restrict__ row_w, const int32_t *__restrict__ cell, uint32_t We, uint32_t T,
    uint32_t L, float *__restrict__ rgb_out)
{
    __shared__ BlockSum<3> red;
    const uint32_t l = blockIdx.x, e = blockIdx.y;                                  // (uniform)
    env_cell_sums(red, env + (size_t)e * 3u * T, row_w, cell, We, T, l);
    if (threadIdx.x < 3u)
        rgb_out[((size_t)e * L + l) * 3u + threadIdx.x] = (float)red.total(threadIdx.x);
}

// F cell maps (F,He,We) -> rgb (E,F,L,3), the layout gcfr_light_rig_frames_u8 takes: one workgroup per (l, e, f)
__global__ __launch_bounds__(kEnvLanes) void environment_fwd_frames_kernel(
    const float *__restrict__ env, const double *__restrict__ row_w, const int32_t *__restrict__ cell, uint32_t We, uint32_t T,
    uint32_t L, uint32_t F, float *__restrict__ rgb_out)
{
    __shared__ BlockSum<3> red;
    const uint32_t l = blockIdx.x, e = blockIdx.y, f = blockIdx.z;                  // (uniform)
    env_cell_sums(red, env + (size_t)e * 3u * T, row_w, cell + (size_t)f * T, We, T, l);
    if (threadIdx.x < 3u)
        rgb_out[(((size_t)e * F + f) * L + l) * 3u + threadIdx.x] = (float)red.total(threadIdx.x);
}

__global__ __launch_bounds__(kEnvLanes) void environment_bwd_kernel(
    const float *__restrict__ g_rgb, const double *__restrict__ row_w, const int32_t *__restrict__ cell, uint32_t We, uint32_t T,
    uint32_t L, float *__restrict__ g_env)
{
    const uint32_t i = blockIdx.x * (uint32_t)kEnvLanes + threadIdx.x, e = blockIdx.y;   // i: (texel, channel) of map e
    if (i >= 3u * T)
        return;
    const uint32_t t = i / 3u, c = i - 3u * t;
    const int32_t l = cell[t];
    float g = 0.0f;
    if (l >= 0 && (uint32_t)l < L)                                                  // (a cell map from elsewhere cannot index out of g_rgb)
        g = (float)row_w[t / We] * g_rgb[((size_t)e * L + (uint32_t)l) * 3u + c];
    g_env[(size_t)e * 3u * T + i] = g;
}

inline bool env_shape_ok(int32_t E, int32_t He, int32_t We, int32_t L)
{
    if (E < 1 || E > kEnvMaxMaps || He < 1 || We < 1 || L < 1 || L > kEnvMaxLights)
        return false;
    return (uint64_t)He * (uint64_t)We <= (uint64_t)kEnvMaxTexels;
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_environment_cells(const float *rows, const float *cols, const float *dirs_map, int32_t He, int32_t We, int32_t L,
                                      float min_cos, int32_t *cell_out, void *stream)
{
    if (!rows || !cols || !dirs_map || !cell_out || !env_shape_ok(1, He, We, L))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t T = (uint32_t)He * (uint32_t)We;
    const dim3 grid((T + kEnvLanes - 1) / kEnvLanes), block(kEnvLanes);
    hipLaunchKernelGGL(environment_cells_kernel, grid, block, 0, (hipStream_t)stream, rows, cols, dirs_map, (uint32_t)We, T,
                       (uint32_t)L, min_cos, cell_out);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_environment_fwd(const float *env, int32_t E, int32_t He, int32_t We, const double *row_w, const int32_t *cell,
                                    int32_t L, float *rgb_out, void *stream)
{
    if (!env || !row_w || ((uintptr_t)row_w & 7u) || !cell || !rgb_out || !env_shape_ok(E, He, We, L))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t T = (uint32_t)He * (uint32_t)We;
    const dim3 grid((uint32_t)L, (uint32_t)E), block(kEnvLanes);
    hipLaunchKernelGGL(environment_fwd_kernel, grid, block, 0, (hipStream_t)stream, env, row_w, cell, (uint32_t)We, T, (uint32_t)L,
                       rgb_out);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_environment_cells_frames(const float *rows, const float *cols, const float *dirs_map, int32_t F, int32_t He,
                                             int32_t We, int32_t L, float min_cos, int32_t *cell_out, void *stream)
{
    if (!rows || !cols || !dirs_map || !cell_out || F < 1 || F > kEnvMaxFrames || !env_shape_ok(1, He, We, L))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t T = (uint32_t)He * (uint32_t)We;
    const dim3 grid((T + kEnvLanes - 1) / kEnvLanes, (uint32_t)F), block(kEnvLanes);
    hipLaunchKernelGGL(environment_cells_frames_kernel, grid, block, 0, (hipStream_t)stream, rows, cols, dirs_map, (uint32_t)We, T,
                       (uint32_t)L, min_cos, cell_out);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_environment_fwd_frames(const float *env, int32_t E, int32_t He, int32_t We, const double *row_w,
                                           const int32_t *cell, int32_t F, int32_t L, float *rgb_out, void *stream)
{
    if (!env || !row_w || ((uintptr_t)row_w & 7u) || !cell || !rgb_out || F < 1 || F > kEnvMaxFrames || !env_shape_ok(E, He, We, L) ||
        (uint64_t)L * (uint64_t)E * (uint64_t)F > 0x7fffffffull)                    // one workgroup per (l, e, f)
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t T = (uint32_t)He * (uint32_t)We;
    const dim3 grid((uint32_t)L, (uint32_t)E, (uint32_t)F), block(kEnvLanes);
    hipLaunchKernelGGL(environment_fwd_frames_kernel, grid, block, 0, (hipStream_t)stream, env, row_w, cell, (uint32_t)We, T,
                       (uint32_t)L, (uint32_t)F, rgb_out);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_environment_bwd(const float *g_rgb, const double *row_w, const int32_t *cell, int32_t E, int32_t He, int32_t We,
                                    int32_t L, float *g_env, void *stream)
{
    if (!g_rgb || !row_w || ((uintptr_t)row_w & 7u) || !cell || !g_env || !env_shape_ok(E, He, We, L))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t T = (uint32_t)He * (uint32_t)We;
    const dim3 grid((3u * T + kEnvLanes - 1) / kEnvLanes, (uint32_t)E), block(kEnvLanes);
    hipLaunchKernelGGL(environment_bwd_kernel, grid, block, 0, (hipStream_t)stream, g_rgb, row_w, cell, (uint32_t)We, T, (uint32_t)L,
                       g_env);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
