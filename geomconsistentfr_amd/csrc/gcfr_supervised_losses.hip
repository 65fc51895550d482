// The training step's supervised-loss head, gfx950: what train_raytracing_relighting_CelebAHQ_DSSIM_8x.py does with the render
// block's OTHER outputs -- depth, albedo, unit_light_direction, ambient_values -- and with PatchGAN's logits between the render
// block and loss.backward():
//   T8:634   depth      = sum |depth m - gt_depth m| / sum m                       (masked L1, m = the skin mask)
//   T8:635   ambient    = 2.5 mean_b |ambient_b - lightings[b,0]|
//   T8:636   lighting   = sum_b (1 - sum_c unit_light[b,c] lightings[b,1+c]) / B
//   T8:639   albedo     = 5 sum |grey mf - gt_albedo mf| / sum mf                  (grey = the mean of the three albedo channels,
//                                                                                   mf = mask_fill_nose_and_mouth)
//   T8:642   generator  = 0.01 mean softplus(-logit)                               (BCE with logits against ones)
// -- as ONE forward launch plus one finishing launch, and ONE backward launch, instead of ~35 ATen launches forward and ~30 in
// autograd's replay.  The image-loss head (gcfr_losses.hip) has the three terms that read rendered_images.
//
// Arithmetic: every product, sum and quotient is one separately rounded IEEE f32 operation (the library is built with
// -ffp-contract=off), in the order of the torch expressions: the two products, their difference, its absolute value.  The grey
// value is ((a0 + a1) + a2) * (1.0f / 3.0f), the order and the reciprocal factor of ATen's mean over a dimension of three.
//
// Forward: a workgroup of 256 lanes owns kSupChunk = 1024 consecutive pixels of the flat (B H W) range, four per lane, through
// the four-pixel access of gcfr_reduce.hpp: one float4 per plane when H W is a multiple of four and every plane is 16-byte
// aligned (eight loads in flight; B H W is then a multiple of four, so no vector straddles the end), otherwise (the three albedo
// planes of an image start H W floats apart, so they lose their alignment) pixels t, t + 256, t + 512, t + 768 with 4-byte loads.
// A lane adds |depth m - gt m|, m, |grey mf - a mf| and mf of its pixels, in ascending order, in f64; the logits are spread over the
// whole grid (element i belongs to global lane i mod lanes) and their softplus is evaluated and added in f64.  The workgroup
// reduces the five sums with the fixed-order block sum (gcfr_reduce.hpp, BlockSum) into five doubles of the caller's workspace.
// The finishing launch (one workgroup) adds the workgroups' partials and the per-image ambient and lighting addends the same way
// and evaluates the five scalar formulas in f32.  No floating-point atomics: two calls return the same bits.
//
// Backward: the same chunks; every gradient element is written once by one lane.  The five upstream gradients and the two mask
// sums are read from device memory (no host synchronisation).  The small outputs (grad_unit_light, grad_ambient_values,
// grad_logits) are spread over the grid like the logits in the forward.  The logits' gradient needs e^x: exp_plain() below is
// built from separately rounded f32 operations only, so that the f32 restatement (tests/supervised_losses_emulation.py) returns
// the same bits.
#include "gcfr_device.hpp"
#include "gcfr_reduce.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kSupLanes = kQuadLanes;
constexpr int kSupChunk = kQuadChunk;         // pixels per workgroup (gcfr_reduce.hpp: four per lane)
constexpr int kSupPartials = 5;               // per workgroup: S_depth, M, S_albedo, M_fill, S_softplus
constexpr int kSupFinish = 7;                 // + the ambient and lighting sums of the finishing launch
constexpr float kThird = 1.0f / 3.0f;

// sign(0) = 0, as l1_loss's backward has it; NaN gives 0
__device__ inline float sup_sgn(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// e^x from separately rounded f32 operations (no fma; Cody-Waite reduction, Cephes' degree-5 polynomial), within ~2 ulp.  x is
// clamped to [-87, 88] (results stay normal and finite); NaN passes through.
__device__ inline float exp_plain(float x)
{
    x = x < -87.0f ? -87.0f : x;
    x = x > 88.0f ? 88.0f : x;
    const float n = rintf(x * 1.44269504f);
    const float r = (x - n * 0.693359375f) - n * -2.12194440e-4f;      // n * 0.693359375 is exact (9 x 8 significant bits)
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float y = (p * (r * r) + r) + 1.0f;
    return ldexpf(y, (int)n);
}

__device__ inline void sup_pixel_fwd(float d, float g, float m, float a0, float a1, float a2, float ga, float mf, double (&acc)[4])
{
    const float dm = d * m, gm = g * m;                                // T8:634
    acc[0] += (double)fabsf(dm - gm);
    acc[1] += (double)m;
    const float grey = ((a0 + a1) + a2) * kThird;                      // T8:638
    const float xm = grey * mf, ym = ga * mf;                          // T8:639
    acc[2] += (double)fabsf(xm - ym);
    acc[3] += (double)mf;
}

// The albedo planes of a lane's four pixels.  Pixel p = b H W + hw of the flat (B H W) range has its channel c at
// albedo[p + (2 b + c) H W].  VEC: the four pixels lie in one image (H W % 4 == 0); otherwise each may lie in another one.
template <bool VEC>
struct SupAlbedoQuad {
    uint32_t q, HW, N;
    size_t shift[VEC ? 1 : 4];                                         // 2 b H W, per pixel

    __device__ SupAlbedoQuad(uint32_t q_, uint32_t HW_, uint32_t N_) : q(q_), HW(HW_), N(N_)
    {
#pragma unroll
        for (int k = 0; k < (VEC ? 1 : 4); ++k) {
            const uint32_t p = quad_pixel<VEC>(q, k);
            shift[k] = p < N ? 2u * (size_t)(p / HW) * HW : 0u;
        }
    }
    __device__ void load(const float *__restrict__ albedo, int c, float (&v)[4]) const
    {
        if constexpr (VEC) {
            quad_load<true>(albedo + shift[0] + (size_t)c * HW, q, N, v);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t p = quad_pixel<false>(q, k);
                v[k] = p < N ? albedo[shift[k] + (size_t)c * HW + p] : 0.0f;
            }
        }
    }
    __device__ void store(float *__restrict__ grad, int c, const float (&v)[4]) const
    {
        if constexpr (VEC) {
            quad_store<true>(grad + shift[0] + (size_t)c * HW, q, N, v);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t p = quad_pixel<false>(q, k);
                if (p < N)
                    grad[shift[k] + (size_t)c * HW + p] = v[k];
            }
        }
    }
};

// the four pixels of a lane, added into acc in ascending order
template <bool VEC>
__device__ inline void sup_quad_fwd(const float *__restrict__ depth, const float *__restrict__ gt_depth, const float *__restrict__ mask,
                                    const float *__restrict__ albedo, const float *__restrict__ gt_albedo,
                                    const float *__restrict__ mask_fill, uint32_t HW, uint32_t N, double (&acc)[4])
{
    const uint32_t q = quad_first<VEC>(blockIdx.x * (uint32_t)kSupChunk);  // (N < 2^31: the chunk's last pixel fits)
    if (q < N) {                                                       // (the lane's first pixel; under it the vector accesses need
        const SupAlbedoQuad<VEC> alb(q, HW, N);                        //  no test of their own: eight loads in flight)
        float d[4], g[4], m[4], a[3][4], ga[4], mf[4];
        quad_load<VEC>(depth, q, N, d);
        quad_load<VEC>(gt_depth, q, N, g);
        quad_load<VEC>(mask, q, N, m);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            alb.load(albedo, c, a[c]);
        quad_load<VEC>(gt_albedo, q, N, ga);
        quad_load<VEC>(mask_fill, q, N, mf);
#pragma unroll
        for (int k = 0; k < 4; ++k)                                    // (a pixel past the end reads as zeros and adds +0.0: no change)
            sup_pixel_fwd(d[k], g[k], m[k], a[0][k], a[1][k], a[2][k], ga[k], mf[k], acc);
    }
}

__global__ __launch_bounds__(kSupLanes) void supervised_losses_fwd_kernel(
    const float *__restrict__ depth, const float *__restrict__ gt_depth, const float *__restrict__ mask,
    const float *__restrict__ albedo, const float *__restrict__ gt_albedo, const float *__restrict__ mask_fill,
    const float *__restrict__ logits, uint32_t n_logits, uint32_t HW, uint32_t N, int vec, double *__restrict__ partials)
{
    __shared__ BlockSum<kSupPartials> red;
    const uint32_t tid = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (vec)                                                           // (uniform)
        sup_quad_fwd<true>(depth, gt_depth, mask, albedo, gt_albedo, mask_fill, HW, N, acc);
    else
        sup_quad_fwd<false>(depth, gt_depth, mask, albedo, gt_albedo, mask_fill, HW, N, acc);
    double acc_g = 0.0;
    if (logits) {                                                      // (uniform) T8:642: -log sigmoid(x) = max(-x, 0) + log1p(e^-|x|)
        const uint32_t stride = gridDim.x * (uint32_t)kSupLanes;       // (grid <= 2^21 workgroups: fits)
        for (uint64_t i = blockIdx.x * (uint32_t)kSupLanes + tid; i < n_logits; i += stride) {
            const double x = (double)logits[i];
            acc_g += fmax(-x, 0.0) + log1p(exp(-fabs(x)));
        }
    }
    const double vals[kSupPartials] = {acc[0], acc[1], acc[2], acc[3], acc_g};
    red.reduce(vals);
    if (tid < (uint32_t)kSupPartials)
        partials[(size_t)blockIdx.x * kSupPartials + tid] = red.total(tid);
}

// one workgroup: the workgroups' partials (lane t takes t, t + 256, ...), the images' ambient and lighting addends (likewise), the
// same block sum, then the five scalar formulas in f32
__global__ __launch_bounds__(kSupLanes) void supervised_losses_finish_kernel(
    const double *__restrict__ partials, uint32_t n_groups, const float *__restrict__ unit_light, const float *__restrict__ ambient,
    const float *__restrict__ lightings, uint32_t B, uint32_t n_logits, float *__restrict__ terms, double *__restrict__ sums)
{
    __shared__ BlockSum<kSupFinish> red;
    const uint32_t tid = threadIdx.x;
    double acc[kSupFinish] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t t = tid; t < n_groups; t += kSupLanes) {
        const double *p = partials + (size_t)t * kSupPartials;
#pragma unroll
        for (int k = 0; k < kSupPartials; ++k)
            acc[k] += p[k];
    }
    for (uint32_t b = tid; b < B; b += kSupLanes) {
        const float *l = lightings + 4 * (size_t)b, *u = unit_light + 3 * (size_t)b;
        acc[5] += (double)fabsf(ambient[b] - l[0]);                    // T8:635
        const float dot = (u[0] * l[1] + u[1] * l[2]) + u[2] * l[3];   // T8:636
        acc[6] += (double)(1.0f - dot);
    }
    red.reduce(acc);
    if (tid == 0) {
        double r[kSupFinish];
#pragma unroll
        for (int k = 0; k < kSupFinish; ++k)
            r[k] = red.total(k);
        const float fB = (float)B;
        terms[0] = (float)r[0] / (float)r[1];                          // 0 / 0 = NaN for an all-zero mask, as torch
        terms[1] = 2.5f * ((float)r[5] / fB);
        terms[2] = (float)r[6] / fB;
        terms[3] = 5.0f * ((float)r[2] / (float)r[3]);
        terms[4] = n_logits ? 0.01f * ((float)r[4] / (float)n_logits) : 0.0f;
        sums[0] = r[0];
        sums[1] = r[1];
        sums[2] = r[2];
        sums[3] = r[3];
    }
}

struct SupBwdArgs {
    const float *depth, *gt_depth, *mask, *albedo, *gt_albedo, *mask_fill, *ambient, *lightings, *logits;
    const double *sums;
    const float *g_depth, *g_ambient, *g_lighting, *g_albedo, *g_generator;
    float *grad_depth, *grad_albedo, *grad_unit_light, *grad_ambient, *grad_logits;
    uint32_t n_logits, B, HW, N;
    int vec;
};

// d term / d (depth m): (g / M) sgn(depth m - gt m), then the product's backward
__device__ inline float sup_pixel_bwd_depth(float d, float g, float m, float sd)
{
    const float dm = d * m, gm = g * m;
    return (sd * sup_sgn(dm - gm)) * m;
}
// per channel: (((5 g) / M_fill) sgn(grey mf - a mf)) mf, then the mean's backward
__device__ inline float sup_pixel_bwd_albedo(float a0, float a1, float a2, float ga, float mf, float sa)
{
    const float grey = ((a0 + a1) + a2) * kThird;
    const float xm = grey * mf, ym = ga * mf;
    return ((sa * sup_sgn(xm - ym)) * mf) * kThird;
}

// grad_depth and grad_albedo at the four pixels of a lane
template <bool VEC>
__device__ inline void sup_quad_bwd(const SupBwdArgs &a)
{
    const uint32_t N = a.N, q = quad_first<VEC>(blockIdx.x * (uint32_t)kSupChunk);
    const bool do_d = a.g_depth != nullptr, do_a = a.g_albedo != nullptr;         // (uniform)
    const float sd = do_d ? a.g_depth[0] / (float)a.sums[1] : 0.0f;
    const float sa = do_a ? (a.g_albedo[0] * 5.0f) / (float)a.sums[3] : 0.0f;
    if (q < N) {                                                                  // (as in the forward)
        const SupAlbedoQuad<VEC> alb(q, a.HW, N);
        float od[4] = {0.0f, 0.0f, 0.0f, 0.0f}, oa[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (do_d) {
            float d[4], g[4], m[4];
            quad_load<VEC>(a.depth, q, N, d);
            quad_load<VEC>(a.gt_depth, q, N, g);
            quad_load<VEC>(a.mask, q, N, m);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                od[k] = sup_pixel_bwd_depth(d[k], g[k], m[k], sd);
        }
        if (do_a) {
            float c[3][4], ga[4], mf[4];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                alb.load(a.albedo, ch, c[ch]);
            quad_load<VEC>(a.gt_albedo, q, N, ga);
            quad_load<VEC>(a.mask_fill, q, N, mf);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                oa[k] = sup_pixel_bwd_albedo(c[0][k], c[1][k], c[2][k], ga[k], mf[k], sa);
        }
        quad_store<VEC>(a.grad_depth, q, N, od);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            alb.store(a.grad_albedo, ch, oa);
    }
}

__global__ __launch_bounds__(kSupLanes) void supervised_losses_bwd_kernel(SupBwdArgs a)
{
    const uint32_t tid = threadIdx.x;
    if (a.vec)                                                                    // (uniform)
        sup_quad_bwd<true>(a);
    else
        sup_quad_bwd<false>(a);
    // the small outputs, spread over the grid
    const uint32_t stride = gridDim.x * (uint32_t)kSupLanes;
    const uint32_t gid = blockIdx.x * (uint32_t)kSupLanes + tid;
    const float fB = (float)a.B;
    const float s_amb = a.g_ambient ? (a.g_ambient[0] * 2.5f) / fB : 0.0f;
    for (uint64_t i = gid; i < a.B; i += stride)                                  // T8:635
        a.grad_ambient[i] = a.g_ambient ? s_amb * sup_sgn(a.ambient[i] - a.lightings[4 * i]) : 0.0f;
    const float s_l = a.g_lighting ? -(a.g_lighting[0] / fB) : 0.0f;
    for (uint64_t i = gid; i < 3ull * a.B; i += stride) {                         // T8:636
        const uint64_t b = i / 3u, c = i - 3u * b;
        a.grad_unit_light[i] = a.g_lighting ? s_l * a.lightings[4 * b + 1 + c] : 0.0f;
    }
    if (a.logits) {                                                               // T8:642: d softplus(-x) / dx = -1 / (1 + e^x)
        const float s_g = a.g_generator ? (a.g_generator[0] * 0.01f) / (float)a.n_logits : 0.0f;
        for (uint64_t i = gid; i < a.n_logits; i += stride)
            a.grad_logits[i] = a.g_generator ? s_g * -(1.0f / (1.0f + exp_plain(a.logits[i]))) : 0.0f;
    }
}

inline bool sup_shape_ok(int32_t B, int32_t H, int32_t W)
{
    return B >= 1 && B <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096 && (uint64_t)B * (uint64_t)H * (uint64_t)W <= 0x7fffffffull;
}
inline uint32_t sup_groups(int32_t B, int32_t H, int32_t W)
{
    return (uint32_t)(((uint64_t)B * H * W + kSupChunk - 1) / kSupChunk);
}

}  // namespace gcfr

using namespace gcfr;

extern "C" size_t gcfr_supervised_losses_workspace_bytes(int32_t B, int32_t H, int32_t W)
{
    if (!sup_shape_ok(B, H, W))
        return 0;
    return (size_t)sup_groups(B, H, W) * kSupPartials * sizeof(double);
}

extern "C" int gcfr_supervised_losses_fwd(const float *depth, const float *gt_depth, const float *mask, const float *albedo,
                                          const float *gt_albedo, const float *mask_fill, const float *unit_light,
                                          const float *ambient_values, const float *lightings, const float *logits,
                                          int64_t n_logits, int32_t B, int32_t H, int32_t W, float *terms, double *sums,
                                          void *workspace, size_t workspace_bytes, void *stream)
{
    if (!depth || !gt_depth || !mask || !albedo || !gt_albedo || !mask_fill || !unit_light || !ambient_values || !lightings ||
        !terms || !sums || !sup_shape_ok(B, H, W) || (logits && (n_logits < 1 || n_logits > 0x7fffffffll)) || !workspace ||
        ((uintptr_t)workspace & 7u) || ((uintptr_t)sums & 7u) || workspace_bytes < gcfr_supervised_losses_workspace_bytes(B, H, W))
        return GCFR_ERR_INVALID_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t HW = (uint32_t)H * (uint32_t)W, N = (uint32_t)B * HW, groups = sup_groups(B, H, W);
    const uint32_t nl = logits ? (uint32_t)n_logits : 0u;
    double *partials = (double *)workspace;
    const int vec = quad_vec_ok(HW, depth, gt_depth, mask, albedo, gt_albedo, mask_fill);
    hipLaunchKernelGGL(supervised_losses_fwd_kernel, dim3(groups), dim3(kSupLanes), 0, st, depth, gt_depth, mask, albedo, gt_albedo,
                       mask_fill, logits, nl, HW, N, vec, partials);
    hipLaunchKernelGGL(supervised_losses_finish_kernel, dim3(1), dim3(kSupLanes), 0, st, partials, groups, unit_light, ambient_values,
                       lightings, (uint32_t)B, nl, terms, sums);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_supervised_losses_bwd(const float *depth, const float *gt_depth, const float *mask, const float *albedo,
                                          const float *gt_albedo, const float *mask_fill, const float *ambient_values,
                                          const float *lightings, const float *logits, int64_t n_logits, int32_t B, int32_t H,
                                          int32_t W, const double *sums, const float *g_depth, const float *g_ambient,
                                          const float *g_lighting, const float *g_albedo, const float *g_generator,
                                          float *grad_depth, float *grad_albedo, float *grad_unit_light, float *grad_ambient_values,
                                          float *grad_logits, void *stream)
{
    if (!depth || !gt_depth || !mask || !albedo || !gt_albedo || !mask_fill || !ambient_values || !lightings || !sums ||
        ((uintptr_t)sums & 7u) || !grad_depth || !grad_albedo || !grad_unit_light || !grad_ambient_values || !sup_shape_ok(B, H, W) ||
        (logits && (n_logits < 1 || n_logits > 0x7fffffffll || !grad_logits)))
        return GCFR_ERR_INVALID_ARGUMENT;
    SupBwdArgs a;
    a.depth = depth, a.gt_depth = gt_depth, a.mask = mask, a.albedo = albedo, a.gt_albedo = gt_albedo, a.mask_fill = mask_fill;
    a.ambient = ambient_values, a.lightings = lightings, a.logits = logits, a.sums = sums;
    a.g_depth = g_depth, a.g_ambient = g_ambient, a.g_lighting = g_lighting, a.g_albedo = g_albedo;
    a.g_generator = logits ? g_generator : nullptr;
    a.grad_depth = grad_depth, a.grad_albedo = grad_albedo, a.grad_unit_light = grad_unit_light, a.grad_ambient = grad_ambient_values;
    a.grad_logits = grad_logits;
    a.n_logits = logits ? (uint32_t)n_logits : 0u;
    a.B = (uint32_t)B, a.HW = (uint32_t)H * (uint32_t)W, a.N = a.B * a.HW;
    a.vec = quad_vec_ok(a.HW, depth, gt_depth, mask, albedo, gt_albedo, mask_fill, grad_depth, grad_albedo);
    hipLaunchKernelGGL(supervised_losses_bwd_kernel, dim3(sup_groups(B, H, W)), dim3(kSupLanes), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
