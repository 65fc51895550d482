// Data formats either side of the render block, gfx950: what the training script's load_data() /
// batch slicing does to the bytes it reads (train_raytracing_relighting_CelebAHQ_DSSIM_8x.py:527-558, 607-615), and the
// two offline metrics of the MATLAB evaluation scripts (MSE_MP.m:24, DSSIM_MP_RGB.m:24-26) as device reductions.
//
// The reference converts every image to float64 when it LOADS it and keeps the whole dataset that way (29,890 faces =
// 110 GB of host memory, T8:528-533); here the dataset stays uint8 on the host (7.3 GB) and a batch is converted on the
// device by one streaming kernel: 6 B read, 24 B written per pixel -- HBM-bound by construction, one lane per pixel,
// coalesced planes, no LDS, no MFMA.  Arithmetic as the script's, op for op:
//   images        imread(jpg)/255.0  (f64 division)  ...  .float()                  T8:550, 618
//   masks         imread(png) ... /255.0 (f64)                                       T8:546, 610   -> f32 here (the losses' weights)
//   masks_fill    max(face mask, depth mask); > 128 -> 255, else 0; /255.0           T8:552-556, 612
//   albedo        imread(jpg) ... /255.0                                             T8:551, 615
//
// Metrics (per image, f64 throughout as MATLAB's double()):
//   MSE_MP.m:24        sum |r m - g m|^2 / (3 sum m),  r, g, m = uint8 / 255.0
//   DSSIM_MP_RGB.m     (1 - sum(ssimmap .* m3) / sum(m3)) / 2 with MATLAB's ssim(A, ref) on an M x N x 3 volume: Gaussian
//                      sigma 1.5, radius ceil(3 sigma) = 5, replicate padding on ALL THREE axes (the channel axis too),
//                      C1 = 0.01^2, C2 = 0.03^2 (dynamic range 1 for double images).  PARITY UNPINNED: MATLAB is not
//                      available; this follows its documented defaults exactly as oracle/postprocess_statements.py does.
//   Two passes over a workspace of 15 doubles per pixel (the five fields A, R, A^2, R^2, A R of three channels): rows,
//   then columns + channels + the SSIM map + both masked sums (gcfr_reduce.hpp's block sum, one f64 atomic per workgroup and sum).
#include "gcfr_device.hpp"
#include "gcfr_reduce.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

// ----------------------------------------------------------------------------------------------
// batch assembly
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assemble_batch_kernel(const uint8_t *__restrict__ img_u8, const uint8_t *__restrict__ dmask_u8,
                                                             const uint8_t *__restrict__ fmask_u8, const uint8_t *__restrict__ alb_u8,
                                                             size_t n_pixels, float *__restrict__ images, float *__restrict__ masks,
                                                             float *__restrict__ masks_fill, float *__restrict__ albedo)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels)
        return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        images[3 * p + ch] = (float)((double)img_u8[3 * p + ch] / 255.0);  // imread/255.0 is f64, then .float()
    const uint8_t dm = dmask_u8[p];
    if (masks)
        masks[p] = (float)((double)dm / 255.0);
    if (masks_fill) {  // T8:552-556
        const uint8_t fm = fmask_u8[p];
        const uint8_t mx = fm > dm ? fm : dm;
        masks_fill[p] = mx > 128 ? 1.0f : 0.0f;  // 255.0 / 255.0, 0.0 / 255.0
    }
    if (albedo)
        albedo[p] = (float)((double)alb_u8[p] / 255.0);
}

// ----------------------------------------------------------------------------------------------
// masked MSE / DSSIM
// ----------------------------------------------------------------------------------------------
constexpr int kGaussR = 5, kGaussTaps = 2 * kGaussR + 1;
struct MetricConsts {
    double k[kGaussTaps];  // normalised Gaussian, sigma 1.5
    double wc[3][3];       // the same filter along the channel axis (3 entries, replicate padding), folded: out[c] = sum wc[c][i] in[i]
};

// pass 1: the five fields of the three channels, filtered along the ROWS axis (replicate padding) -> fields (B, P, 15)
__global__ __launch_bounds__(256) void metrics_rows_kernel(const uint8_t *__restrict__ recon, const uint8_t *__restrict__ gt, int H, int W,
                                                           MetricConsts mc, double *__restrict__ fields)
{
    const size_t P = (size_t)H * W;
    const int b = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P)
        return;
    const int r = (int)(p / W), c = (int)(p - (size_t)r * W);
    const uint8_t *A8 = recon + (size_t)b * P * 3, *R8 = gt + (size_t)b * P * 3;
    double acc[15];
#pragma unroll
    for (int i = 0; i < 15; ++i)
        acc[i] = 0.0;
    for (int t = 0; t < kGaussTaps; ++t) {
        int rr = r + t - kGaussR;
        rr = rr < 0 ? 0 : (rr > H - 1 ? H - 1 : rr);
        const size_t q = ((size_t)rr * W + c) * 3;
        const double w = mc.k[t];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double a = (double)A8[q + ch] / 255.0, g = (double)R8[q + ch] / 255.0;
            acc[0 + ch] += w * a;
            acc[3 + ch] += w * g;
            acc[6 + ch] += w * (a * a);
            acc[9 + ch] += w * (g * g);
            acc[12 + ch] += w * (a * g);
        }
    }
    double *o = fields + ((size_t)b * P + p) * 15;
#pragma unroll
    for (int i = 0; i < 15; ++i)
        o[i] = acc[i];
}

// pass 2: columns, then channels, the SSIM map, and the masked sums {sum ssim m3, sum m3, sum |r m - g m|^2, sum m}
__global__ __launch_bounds__(256) void metrics_cols_kernel(const uint8_t *__restrict__ recon, const uint8_t *__restrict__ gt,
                                                           const uint8_t *__restrict__ mask, int mask_batch, int H, int W,
                                                           MetricConsts mc, const double *__restrict__ fields, double *__restrict__ sums)
{
    const size_t P = (size_t)H * W;
    const int b = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double part[4] = {0.0, 0.0, 0.0, 0.0};
    if (p < P) {
        const int r = (int)(p / W), c = (int)(p - (size_t)r * W);
        double f[15];
#pragma unroll
        for (int i = 0; i < 15; ++i)
            f[i] = 0.0;
        for (int t = 0; t < kGaussTaps; ++t) {
            int cc = c + t - kGaussR;
            cc = cc < 0 ? 0 : (cc > W - 1 ? W - 1 : cc);
            const double *q = fields + ((size_t)b * P + (size_t)r * W + cc) * 15;
            const double w = mc.k[t];
#pragma unroll
            for (int i = 0; i < 15; ++i)
                f[i] += w * q[i];
        }
        const double m = (double)mask[(size_t)(mask_batch == 1 ? 0 : b) * P + p] / 255.0;
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        double ssim_sum = 0.0, se = 0.0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            double g5[5];  // the channel-axis filter of the five fields
#pragma unroll
            for (int k = 0; k < 5; ++k)
                g5[k] = (mc.wc[ch][0] * f[3 * k + 0] + mc.wc[ch][1] * f[3 * k + 1]) + mc.wc[ch][2] * f[3 * k + 2];
            const double mux = g5[0], muy = g5[1];
            const double sx = g5[2] - mux * mux, sy = g5[3] - muy * muy, sxy = g5[4] - mux * muy;
            ssim_sum += ((2.0 * mux * muy + C1) * (2.0 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sx + sy + C2));
            const double a = (double)recon[((size_t)b * P + p) * 3 + ch] / 255.0, g = (double)gt[((size_t)b * P + p) * 3 + ch] / 255.0;
            const double d = a * m - g * m;
            se += d * d;
        }
        part[0] = ssim_sum * m;
        part[1] = 3.0 * m;
        part[2] = se;
        part[3] = m;
    }
    __shared__ BlockSum<4> red;
    red.reduce(part);
    if (threadIdx.x < 4)
        atomicAdd(sums + 4 * (size_t)b + threadIdx.x, red.total(threadIdx.x));
}

__global__ void metrics_finish_kernel(const double *__restrict__ sums, int B, double *__restrict__ mse, double *__restrict__ dssim)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B)
        return;
    const double *s = sums + 4 * (size_t)b;
    if (mse)
        mse[b] = s[2] / (3.0 * s[3]);                 // MSE_MP.m:24
    if (dssim)
        dssim[b] = (1.0 - s[0] / s[1]) / 2.0;         // DSSIM_MP_RGB.m:25-26
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_assemble_batch_u8(const uint8_t *images_u8, const uint8_t *depth_mask_u8, const uint8_t *face_mask_u8,
                                      const uint8_t *albedo_u8, int32_t B, int32_t H, int32_t W, float *images, float *masks,
                                      float *masks_fill, float *albedo, void *stream)
{
    if (!images_u8 || !depth_mask_u8 || !images || B <= 0 || H <= 0 || W <= 0)
        return GCFR_ERR_INVALID_ARGUMENT;
    if ((masks_fill && !face_mask_u8) || (albedo && !albedo_u8))
        return GCFR_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)B * H * W;
    if (n > 0x7fffffffull * 256ull)
        return GCFR_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(assemble_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images_u8,
                       depth_mask_u8, face_mask_u8, albedo_u8, n, images, masks, masks_fill, albedo);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" size_t gcfr_masked_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W)
{
    if (B <= 0 || H <= 0 || W <= 0)
        return 0;
    return ((size_t)B * H * W * 15 + 4 * (size_t)B) * sizeof(double);
}

extern "C" int gcfr_masked_metrics_u8(const uint8_t *recon_u8, const uint8_t *gt_u8, const uint8_t *mask_u8, int32_t mask_batch,
                                      int32_t B, int32_t H, int32_t W, double *mse_out, double *dssim_out, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (!recon_u8 || !gt_u8 || !mask_u8 || (!mse_out && !dssim_out) || B <= 0 || H <= 0 || W <= 0 || B > 65535 ||
        (mask_batch != 1 && mask_batch != B) || !workspace || ((uintptr_t)workspace & 7u) ||
        workspace_bytes < gcfr_masked_metrics_workspace_bytes(B, H, W))
        return GCFR_ERR_INVALID_ARGUMENT;
    MetricConsts mc;
    double ksum = 0.0;
    for (int i = 0; i < kGaussTaps; ++i) {
        const double d = (double)(i - kGaussR);
        mc.k[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        ksum += mc.k[i];
    }
    for (int i = 0; i < kGaussTaps; ++i)
        mc.k[i] /= ksum;
    for (int c = 0; c < 3; ++c) {
        for (int i = 0; i < 3; ++i)
            mc.wc[c][i] = 0.0;
        for (int t = 0; t < kGaussTaps; ++t) {  // taps in the statement's order: the replicate-padded axis is walked low to high
            int cc = c + t - kGaussR;
            cc = cc < 0 ? 0 : (cc > 2 ? 2 : cc);
            mc.wc[c][cc] += mc.k[t];
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)H * W;
    double *fields = (double *)workspace;
    double *sums = fields + (size_t)B * P * 15;
    if (hipMemsetAsync(sums, 0, 4 * (size_t)B * sizeof(double), st) != hipSuccess)
        return GCFR_ERR_LAUNCH;
    const dim3 grid((unsigned)((P + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(metrics_rows_kernel, grid, dim3(256), 0, st, recon_u8, gt_u8, H, W, mc, fields);
    hipLaunchKernelGGL(metrics_cols_kernel, grid, dim3(256), 0, st, recon_u8, gt_u8, mask_u8, mask_batch, H, W, mc, fields, sums);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, sums, B, mse_out, dssim_out);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
