// The training step's image-loss head, gfx950: what train_raytracing_relighting_CelebAHQ_DSSIM_8x.py does with
// `rendered_images` between the render block and loss.backward() --
//   T8:619 / 641   composite = rendered * m + (1 - m) * img            (the mask paste, once for PatchGAN, once for the DSSIM)
//   T8:633         sum (rendered * m - img * m)^2  and  sum m           (the masked reconstruction L2's two sums)
//   T8:643         pytorch_msssim.ssim(composite, img): Gaussian window 11 / sigma 1.5, separable 'valid' filtering,
//                  K = (0.01, 0.03), the per-(image, channel) mean of the map (the raw mean: relu and the batch mean stay in torch)
// -- as ONE forward launch (plus a fixed-order finishing step) and ONE backward launch, instead of ~140 ATen launches.
//
// Arithmetic: every product and sum separately rounded (the library is built with -ffp-contract=off), so the composite is
// bit-equal to the torch expression; the blurs are the same f32 sums of the same eleven products as the depthwise
// convolutions (along H first, then along W, as train.ssim filters), added tap 0 to tap 10.
//
// Forward: a workgroup of 256 lanes owns a 16 x 32 tile of pixels of one image, all three channels.  It stages the photograph and
// the composite of the tile plus a 5-pixel halo in LDS (2 x 3 planes of 26 x 42 f32), writes the composite of its own pixels,
// and per channel filters the five maps X, Y, XX, YY, XY down the columns into LDS (5 x 16 x 42) and along the rows into
// registers: the five blurred maps never reach HBM.  The SSIM map exists at the pixels whose whole window lies inside the
// image (5 <= r < H-5, 5 <= c < W-5: the (H-10) x (W-10) 'valid' positions, indexed here by their CENTRE pixel).  Each lane adds
// its map values, squared differences and mask values in f64; the workgroup reduces them with the fixed-order block sum
// (gcfr_reduce.hpp, BlockSum) into five doubles of the caller's workspace.  Two small kernels add the tiles of each image and then
// the images, again in a fixed order: no floating-point atomic anywhere, so two calls on the same inputs give the same bits.
// LDS: 2 x 3 x 1099 + 5 x 672 floats = 39.8 KB -> three workgroups per CU.  The planes' stride is 26 * 42 + 7 = 1099 floats
// (1099 mod 32 = 11): when the interleaved (NHWC) photograph is staged, consecutive lanes write channels 0, 1, 2 of one pixel
// into three planes, and with the unpadded stride (1092 mod 32 = 4) the three groups of ~11 consecutive banks would overlap.
// All other LDS traffic is 32 consecutive floats per half-wave: conflict-free at any row stride.
//
// Backward (gather form, 512 lanes, the same 16 x 32 tile, one channel after the other): the adjoints of the map with respect to
// blur(X), blur(XX), blur(XY) -- a, b, c -- are needed on the tile plus a 5-pixel halo, and each of them needs the five blurs,
// i.e. the inputs on a 10-pixel halo.  The workgroup recomputes them (inputs 36 x 52, maps 26 x 42), zeroes them outside the
// valid positions, applies the same symmetric window to them (the transpose of a valid correlation is the correlation of the
// zero-extended map) and writes
//   grad_rendered = m (g_composite + blurT(a) + 2 X blurT(b) + Y blurT(c)) + g_recon 2 m (rendered m - img m)
// once per pixel: no atomics, bit-reproducible.  LDS 2 x 1872 + 5 x 1352 + 3 x 1092 floats = 55.1 KB -> two workgroups
// (sixteen waves) per CU.
#include "gcfr_device.hpp"
#include "gcfr_reduce.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kWin = 11, kWinR = 5;
constexpr int kLossTileH = 16, kLossTileW = 32;                                       // the pixels a workgroup owns
constexpr int kFwdH = kLossTileH + 2 * kWinR, kFwdW = kLossTileW + 2 * kWinR;         // 26 x 42: tile + the window's halo
constexpr int kFwdPlane = kFwdH * kFwdW + 7;                                          // see the bank note above
constexpr int kBwdH = kLossTileH + 4 * kWinR, kBwdW = kLossTileW + 4 * kWinR;         // 36 x 52: + the halo of the adjoints
constexpr int kLossPartials = 5;                                                      // per tile: ssim sums of 3 channels, sq, mask

struct LossWindow {
    float w[kWin];
};

__device__ inline size_t photo_index(int layout, int b, int ch, int r, int c, int H, int W)
{
    return layout == 0 ? (((size_t)b * H + r) * W + c) * 3 + ch : (((size_t)b * 3 + ch) * H + r) * W + c;
}

// T8:619 / 641: the mask paste, bit-equal to the torch expression
__device__ inline float paste(float rv, float m, float y)
{
    const float t1 = rv * m;
    const float om = 1.0f - m;
    const float t3 = om * y;
    return t1 + t3;
}

// The SSIM arithmetic, stated once for the forward and for the backward's recomputation: the gradient belongs to its forward only
// while both run these very operations.  Every accumulator starts at 0.0f and adds w[t] * v, tap 0 to tap 10.
//
// Along H: the five maps X, Y, XX, YY, XY of the staged planes pX, pY (row stride ROW_W) at N consecutive positions, into the five
// planes of N floats of sMid.
template <int ROW_W, int N, int LANES>
__device__ inline void ssim_blur_columns(const float *pX, const float *pY, const LossWindow &win, float *sMid)
{
    for (int i = threadIdx.x; i < N; i += LANES) {
        float ax = 0.0f, ay = 0.0f, axx = 0.0f, ayy = 0.0f, axy = 0.0f;
#pragma unroll
        for (int t = 0; t < kWin; ++t) {
            const float x = pX[i + t * ROW_W], y = pY[i + t * ROW_W], w = win.w[t];
            ax += w * x;
            ay += w * y;
            axx += w * (x * x);
            ayy += w * (y * y);
            axy += w * (x * y);
        }
        sMid[0 * N + i] = ax;
        sMid[1 * N + i] = ay;
        sMid[2 * N + i] = axx;
        sMid[3 * N + i] = ayy;
        sMid[4 * N + i] = axy;
    }
}

// Along W at one map position (p = its first tap in plane 0 of sMid, planes N floats apart), then the two factors of the map:
// lum = (2 mu1 mu2 + C1) / B1, cs = (2 s12 + C2) / B2.
struct SsimPoint {
    float mu1, mu2, B1, B2, lum, cs;
};
template <int N>
__device__ inline SsimPoint ssim_point(const float *p, const LossWindow &win, float C1, float C2)
{
    float mu1 = 0.0f, mu2 = 0.0f, xx = 0.0f, yy = 0.0f, xy = 0.0f;
#pragma unroll
    for (int t = 0; t < kWin; ++t) {
        const float w = win.w[t];
        mu1 += w * p[0 * N + t];
        mu2 += w * p[1 * N + t];
        xx += w * p[2 * N + t];
        yy += w * p[3 * N + t];
        xy += w * p[4 * N + t];
    }
    const float s1 = xx - mu1 * mu1, s2 = yy - mu2 * mu2, s12 = xy - mu1 * mu2;
    const float B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s1 + s2 + C2;
    return {mu1, mu2, B1, B2, (2.0f * mu1 * mu2 + C1) / B1, (2.0f * s12 + C2) / B2};
}

__global__ __launch_bounds__(256) void image_losses_fwd_kernel(const float *__restrict__ rendered, const float *__restrict__ img,
                                                               const float *__restrict__ mask, int layout, int H, int W, int tiles_x,
                                                               LossWindow win, float C1, float C2, float *__restrict__ composite,
                                                               double *__restrict__ partials)
{
    __shared__ float sX[3 * kFwdPlane], sY[3 * kFwdPlane];
    __shared__ float sMid[5 * kLossTileH * kFwdW];
    __shared__ BlockSum<kLossPartials> red;
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int r0 = (tile / tiles_x) * kLossTileH, c0 = (tile % tiles_x) * kLossTileW;
    constexpr int kItems = 3 * kFwdH * kFwdW;

    // the photograph, in its own order (NHWC: a row of the region is 126 consecutive floats)
    for (int i = tid; i < kItems; i += 256) {
        int ch, rr, cc;
        if (layout == 0) {
            rr = i / (kFwdW * 3);
            const int k = i - rr * (kFwdW * 3);
            cc = k / 3;
            ch = k - cc * 3;
        } else {
            ch = i / (kFwdH * kFwdW);
            const int k = i - ch * (kFwdH * kFwdW);
            rr = k / kFwdW;
            cc = k - rr * kFwdW;
        }
        const int r = r0 - kWinR + rr, c = c0 - kWinR + cc;
        float y = 0.0f;
        if (r >= 0 && r < H && c >= 0 && c < W)
            y = img[photo_index(layout, b, ch, r, c, H, W)];
        sY[ch * kFwdPlane + rr * kFwdW + cc] = y;
    }
    __syncthreads();

    // the composite, plane by plane; the tile's own pixels are written out and enter the reconstruction sums
    double acc_sq = 0.0, acc_m = 0.0;
    for (int i = tid; i < kItems; i += 256) {
        const int ch = i / (kFwdH * kFwdW);
        const int k = i - ch * (kFwdH * kFwdW);
        const int rr = k / kFwdW, cc = k - rr * kFwdW;
        const int r = r0 - kWinR + rr, c = c0 - kWinR + cc;
        float x = 0.0f;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            const size_t q = (((size_t)b * 3 + ch) * H + r) * W + c;
            const float rv = rendered[q];
            const float m = mask ? mask[((size_t)b * H + r) * W + c] : 1.0f;
            const float y = sY[ch * kFwdPlane + k];
            x = paste(rv, m, y);
            if (rr >= kWinR && rr < kWinR + kLossTileH && cc >= kWinR && cc < kWinR + kLossTileW) {
                composite[q] = x;
                const float d = rv * m - y * m;                               // T8:633
                acc_sq += (double)(d * d);
                acc_m += (double)m;
            }
        }
        sX[ch * kFwdPlane + k] = x;
    }
    __syncthreads();

    double acc_s[3] = {0.0, 0.0, 0.0};
    constexpr int kMid = kLossTileH * kFwdW;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        ssim_blur_columns<kFwdW, kMid, 256>(sX + ch * kFwdPlane, sY + ch * kFwdPlane, win, sMid);
        __syncthreads();
        for (int i = tid; i < kLossTileH * kLossTileW; i += 256) {            // along W, then the map
            const int r = i / kLossTileW, c = i - r * kLossTileW;
            const int pr = r0 + r, pc = c0 + c;
            if (pr >= kWinR && pr < H - kWinR && pc >= kWinR && pc < W - kWinR) {
                const SsimPoint s = ssim_point<kMid>(sMid + r * kFwdW + c, win, C1, C2);
                acc_s[ch] += (double)(s.lum * s.cs);
            }
        }
        __syncthreads();
    }

    const double vals[kLossPartials] = {acc_s[0], acc_s[1], acc_s[2], acc_sq, acc_m};
    red.reduce(vals);
    if (tid < kLossPartials)
        partials[((size_t)b * gridDim.x + tile) * kLossPartials + tid] = red.total(tid);
}

// the tiles of one image, lane t taking tiles t, t + 256, ... in order, then the same block sum
__global__ __launch_bounds__(256) void image_losses_finish_image_kernel(const double *__restrict__ partials, int tiles, double n_valid,
                                                                        float *__restrict__ ssim_out, double *__restrict__ per_image)
{
    __shared__ BlockSum<kLossPartials> red;
    const int b = blockIdx.x, tid = threadIdx.x;
    double acc[kLossPartials] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = tid; t < tiles; t += 256) {
        const double *p = partials + ((size_t)b * tiles + t) * kLossPartials;
#pragma unroll
        for (int k = 0; k < kLossPartials; ++k)
            acc[k] += p[k];
    }
    red.reduce(acc);
    if (tid < kLossPartials) {
        const double s = red.total(tid);
        if (tid < 3)
            ssim_out[3 * (size_t)b + tid] = (float)(s / n_valid);
        else
            per_image[2 * (size_t)b + (tid - 3)] = s;
    }
}

// the images of the batch: one wave
__global__ __launch_bounds__(64) void image_losses_finish_batch_kernel(const double *__restrict__ per_image, int B, double *__restrict__ sums)
{
    double sq = 0.0, m = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) {
        sq += per_image[2 * (size_t)b];
        m += per_image[2 * (size_t)b + 1];
    }
    sq = wave_sum_f64(sq);
    m = wave_sum_f64(m);
    if (threadIdx.x == 0) {
        sums[0] = sq;
        sums[1] = m;
    }
}

__global__ __launch_bounds__(512) void image_losses_bwd_kernel(const float *__restrict__ rendered, const float *__restrict__ img,
                                                               const float *__restrict__ mask, int layout, int H, int W, int tiles_x,
                                                               LossWindow win, float C1, float C2, float n_valid,
                                                               const float *__restrict__ g_composite, const float *__restrict__ g_ssim,
                                                               const float *__restrict__ g_recon, float *__restrict__ grad_rendered)
{
    constexpr int kMapH = kFwdH, kMapW = kFwdW;                                // the adjoints: tile + 5
    constexpr int kMid = kMapH * kBwdW, kMap = kMapH * kMapW, kCol = kLossTileH * kMapW;
    __shared__ float sX[kBwdH * kBwdW], sY[kBwdH * kBwdW];
    __shared__ float sMid[5 * kMid];
    __shared__ float sAbc[3 * kMap];
    float *sCol = sMid;                                                        // 3 x 16 x 42, once sMid has been consumed
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int r0 = (tile / tiles_x) * kLossTileH, c0 = (tile % tiles_x) * kLossTileW;
    const float grec = g_recon ? g_recon[0] : 0.0f;

    // the tile's own pixel of this lane (16 x 32 = 512 lanes)
    const int tr = tid / kLossTileW, tc = tid - tr * kLossTileW;
    const int pr = r0 + tr, pc = c0 + tc;
    const bool own = pr < H && pc < W;
    const float m_own = (own && mask) ? mask[((size_t)b * H + pr) * W + pc] : 1.0f;

#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        float gx = 0.0f;
        if (g_ssim) {                                                          // (uniform)
            const float u = g_ssim[3 * (size_t)b + ch] / n_valid;               // the mean's backward
            for (int i = tid; i < kBwdH * kBwdW; i += 512) {
                const int rr = i / kBwdW, cc = i - rr * kBwdW;
                const int r = r0 - 2 * kWinR + rr, c = c0 - 2 * kWinR + cc;
                float x = 0.0f, y = 0.0f;
                if (r >= 0 && r < H && c >= 0 && c < W) {
                    y = img[photo_index(layout, b, ch, r, c, H, W)];
                    const float rv = rendered[(((size_t)b * 3 + ch) * H + r) * W + c];
                    const float m = mask ? mask[((size_t)b * H + r) * W + c] : 1.0f;
                    x = paste(rv, m, y);
                }
                sX[i] = x;
                sY[i] = y;
            }
            __syncthreads();
            ssim_blur_columns<kBwdW, kMid, 512>(sX, sY, win, sMid);            // map rows r0-5 ..., all 52 columns
            __syncthreads();
            for (int i = tid; i < kMap; i += 512) {                            // along W, then the map's adjoints
                const int mr = i / kMapW, mc = i - mr * kMapW;
                const int qr = r0 - kWinR + mr, qc = c0 - kWinR + mc;          // the map position's centre pixel
                float a = 0.0f, bb = 0.0f, c_ = 0.0f;
                if (qr >= kWinR && qr < H - kWinR && qc >= kWinR && qc < W - kWinR) {
                    const SsimPoint s = ssim_point<kMid>(sMid + mr * kBwdW + mc, win, C1, C2);
                    // d map / d blur(X), d blur(XX), d blur(XY)
                    const float d_mu1 = 2.0f * s.cs * (s.mu2 - s.lum * s.mu1) / s.B1 + 2.0f * s.lum * (s.cs * s.mu1 - s.mu2) / s.B2;
                    const float d_xx = -(s.lum * s.cs) / s.B2;
                    const float d_xy = 2.0f * s.lum / s.B2;
                    a = u * d_mu1;
                    bb = u * d_xx;
                    c_ = u * d_xy;
                }
                sAbc[0 * kMap + i] = a;
                sAbc[1 * kMap + i] = bb;
                sAbc[2 * kMap + i] = c_;
            }
            __syncthreads();
            for (int i = tid; i < kCol; i += 512) {                            // blurT along H (sMid is free: every lane passed the barrier)
                float va = 0.0f, vb = 0.0f, vc = 0.0f;
#pragma unroll
                for (int t = 0; t < kWin; ++t) {
                    const float w = win.w[t];
                    va += w * sAbc[0 * kMap + i + t * kMapW];
                    vb += w * sAbc[1 * kMap + i + t * kMapW];
                    vc += w * sAbc[2 * kMap + i + t * kMapW];
                }
                sCol[0 * kCol + i] = va;
                sCol[1 * kCol + i] = vb;
                sCol[2 * kCol + i] = vc;
            }
            __syncthreads();
            {                                                                  // blurT along W at the lane's own pixel
                const float *p = sCol + tr * kMapW + tc;
                float ta = 0.0f, tb = 0.0f, tcc = 0.0f;
#pragma unroll
                for (int t = 0; t < kWin; ++t) {
                    const float w = win.w[t];
                    ta += w * p[0 * kCol + t];
                    tb += w * p[1 * kCol + t];
                    tcc += w * p[2 * kCol + t];
                }
                const int o = (tr + 2 * kWinR) * kBwdW + tc + 2 * kWinR;
                gx = ta + 2.0f * sX[o] * tb + sY[o] * tcc;
            }
            __syncthreads();                                                   // sX / sY / sCol are rewritten by the next channel
        }
        if (own) {
            const size_t q = (((size_t)b * 3 + ch) * H + pr) * W + pc;
            const float g = (g_composite ? g_composite[q] : 0.0f) + gx;
            float out = m_own * g;
            if (g_recon) {
                const float rv = rendered[q];
                const float y = img[photo_index(layout, b, ch, pr, pc, H, W)];
                out += grec * (2.0f * m_own * (rv * m_own - y * m_own));
            }
            grad_rendered[q] = out;
        }
    }
}

inline bool loss_shape_ok(int32_t B, int32_t H, int32_t W)
{
    return B >= 1 && B <= 65535 && H >= kWin && H <= 4096 && W >= kWin && W <= 4096;
}
inline int loss_tiles_x(int32_t W) { return (W + kLossTileW - 1) / kLossTileW; }
inline int loss_tiles_y(int32_t H) { return (H + kLossTileH - 1) / kLossTileH; }

inline bool loss_consts(const float *window, double data_range, LossWindow *win, float *C1, float *C2)
{
    if (!window || !(data_range > 0.0) || !(data_range < 1e30))
        return false;
    for (int i = 0; i < kWin; ++i)
        win->w[i] = window[i];
    *C1 = (float)((0.01 * data_range) * (0.01 * data_range));
    *C2 = (float)((0.03 * data_range) * (0.03 * data_range));
    return true;
}

}  // namespace gcfr

using namespace gcfr;

extern "C" size_t gcfr_image_losses_workspace_bytes(int32_t B, int32_t H, int32_t W)
{
    if (!loss_shape_ok(B, H, W))
        return 0;
    const size_t tiles = (size_t)loss_tiles_x(W) * loss_tiles_y(H);
    return ((size_t)B * tiles * kLossPartials + 2 * (size_t)B) * sizeof(double);
}

extern "C" int gcfr_image_losses_fwd(const float *rendered, const float *images, const float *mask, int32_t images_layout,
                                     int32_t B, int32_t H, int32_t W, const float *window, double data_range, float *composite,
                                     float *ssim, double *sums, void *workspace, size_t workspace_bytes, void *stream)
{
    LossWindow win;
    float C1, C2;
    if (!rendered || !images || !composite || !ssim || !sums || !loss_shape_ok(B, H, W) ||
        (images_layout != GCFR_IMAGES_NHWC && images_layout != GCFR_IMAGES_NCHW) || !loss_consts(window, data_range, &win, &C1, &C2) ||
        !workspace || ((uintptr_t)workspace & 7u) || workspace_bytes < gcfr_image_losses_workspace_bytes(B, H, W))
        return GCFR_ERR_INVALID_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    const int tx = loss_tiles_x(W), tiles = tx * loss_tiles_y(H);
    double *partials = (double *)workspace;
    double *per_image = partials + (size_t)B * tiles * kLossPartials;
    hipLaunchKernelGGL(image_losses_fwd_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, st, rendered, images, mask,
                       images_layout, H, W, tx, win, C1, C2, composite, partials);
    hipLaunchKernelGGL(image_losses_finish_image_kernel, dim3((unsigned)B), dim3(256), 0, st, partials, tiles,
                       (double)(H - 2 * kWinR) * (double)(W - 2 * kWinR), ssim, per_image);
    hipLaunchKernelGGL(image_losses_finish_batch_kernel, dim3(1), dim3(64), 0, st, per_image, B, sums);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}

extern "C" int gcfr_image_losses_bwd(const float *rendered, const float *images, const float *mask, int32_t images_layout,
                                     int32_t B, int32_t H, int32_t W, const float *window, double data_range,
                                     const float *g_composite, const float *g_ssim, const float *g_recon, float *grad_rendered,
                                     void *stream)
{
    LossWindow win;
    float C1, C2;
    if (!rendered || !images || !grad_rendered || !loss_shape_ok(B, H, W) ||
        (images_layout != GCFR_IMAGES_NHWC && images_layout != GCFR_IMAGES_NCHW) || !loss_consts(window, data_range, &win, &C1, &C2))
        return GCFR_ERR_INVALID_ARGUMENT;
    const int tx = loss_tiles_x(W), tiles = tx * loss_tiles_y(H);
    hipLaunchKernelGGL(image_losses_bwd_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(512), 0, (hipStream_t)stream, rendered,
                       images, mask, images_layout, H, W, tx, win, C1, C2, (float)(H - 2 * kWinR) * (float)(W - 2 * kWinR),
                       g_composite, g_ssim, g_recon, grad_rendered);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
