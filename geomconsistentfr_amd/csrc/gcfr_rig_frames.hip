// Rig frames, gfx950: F light rigs per face combined with the per-light shadings of ONE many-lights pass and pasted into the
// photograph, straight to the uint8 frames (B,F,H,W,3) -- an animated rig (a key fading into a fill, a colour sweep, a turntable
// of an environment map) in ONE launch.  Frame [b,f] is, byte for byte, gcfr_light_rig_fwd with rgb[.,f] followed by
// gcfr_inference_images_u8 at L = 1; the f32 `rendered` of that path never reaches memory here.
//
// Arithmetic (the library is built with -ffp-contract=off: every product and sum is one separately rounded IEEE f32 operation).
// Per pixel p, frame f and channel c, the rig stage's chain (gcfr_light_rig.hip):
//   acc = rgb[f,0,c] final[0];  acc = acc + rgb[f,l,c] final[l] for l = 1 .. L-1 ascending;  rendered = albedo[c] acc
// then the image kernel's composite (gcfr_composite.hpp, the same functions the image kernel calls):
//   m = mask_f32 ? (double)((float)mk / 255.0f) : (double)mk / 255.0
//   byte = quantise_u8(m > 0 ? (double)(255.0f rendered) m : (double)input 255.0)
// Nothing is clamped before the quantisation; a NaN gives byte 0.
//
// Work split: a workgroup of 256 lanes owns kQuadChunk = 1024 consecutive pixels of ONE face (four per lane, gcfr_reduce.hpp) and
// ONE tile of kFrameTile consecutive frames; a lane keeps kFrameTile x 3 x 4 f32 accumulators and walks the L lights once, so a
// plane of `final` is read ceil(F / kFrameTile) times, not F times.  The face and the frame tile are the same for the whole
// workgroup: the 3 kFrameTile rig values of a light are read through wave-uniform addresses (scalar loads) and every multiply takes
// one scalar operand.  Albedo, photograph and mask are loaded after the light loop, once per pixel and frame tile.  The last tile
// of F % kFrameTile frames computes on a copy of the last frame (a valid address) and stores only its own frames.
// VEC (H W a multiple of four, final / albedo / photograph 16-byte aligned, mask and frames 4-byte aligned): lane t owns pixels
// 4 t .. 4 t + 3, every f32 plane moves in 16-byte accesses, the photograph's 12 floats in three, the mask's four bytes in one,
// and a frame's 12 consecutive bytes leave as three dwords.  Otherwise lane t owns pixels t, t + 256, t + 512, t + 768 and the
// photograph, the mask and the frames move one element at a time.
// Bytes per pixel: ceil(F / kFrameTile) (4 L + 12 + 12 + 1) read, 3 F written.
#include "gcfr_composite.hpp"
#include "gcfr_device.hpp"
#include "gcfr_reduce.hpp"

#include "../../include/gcfr.h"

namespace gcfr {

constexpr int kFrameTile = 4;                 // frames per workgroup (lighting.RIG_FRAMES_TILE)
constexpr int kFramesMaxLights = 4096;        // the rig stage's limit
constexpr int kFramesMaxFrames = 4096;

template <bool VEC>
__global__ __launch_bounds__(kQuadLanes) void light_rig_frames_kernel(
    const float *__restrict__ final_shading, const float *__restrict__ albedo, const float *__restrict__ input_hwc,
    const uint8_t *__restrict__ mask, uint32_t mask_stride, int mask_f32, const float *__restrict__ rgb, uint32_t rgb_stride,
    uint32_t L, uint32_t F, uint32_t HW, uint32_t chunks, uint8_t *__restrict__ frames)
{
    const uint32_t b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;          // (uniform)
    const uint32_t f0 = blockIdx.y * (uint32_t)kFrameTile;                         // (uniform; f0 < F by the grid)
    const uint32_t q = quad_first<VEC>(ch * (uint32_t)kQuadChunk);
    const float *fb = final_shading + (size_t)b * L * HW;
    const float *rig[kFrameTile];
#pragma unroll
    for (int j = 0; j < kFrameTile; ++j) {                                         // a frame past the last one: the last one again
        const uint32_t f = f0 + (uint32_t)j < F ? f0 + (uint32_t)j : F - 1u;
        rig[j] = rgb + (size_t)b * rgb_stride + (size_t)f * 3u * L;
    }
    float f[4], acc[kFrameTile][3][4];
    quad_load<VEC>(fb, q, HW, f);
#pragma unroll
    for (int j = 0; j < kFrameTile; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = rig[j][c];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                acc[j][c][k] = r * f[k];
        }
#pragma unroll 2
    for (uint32_t l = 1; l < L; ++l) {
        quad_load<VEC>(fb + (size_t)l * HW, q, HW, f);
#pragma unroll
        for (int j = 0; j < kFrameTile; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r = rig[j][3u * l + c];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    acc[j][c][k] = acc[j][c][k] + r * f[k];
            }
    }
    // rendered = albedo * acc, in place
    const size_t plane3 = (size_t)b * 3u * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float al[4];
        quad_load<VEC>(albedo + plane3 + (size_t)c * HW, q, HW, al);
#pragma unroll
        for (int j = 0; j < kFrameTile; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                acc[j][c][k] = al[k] * acc[j][c][k];
    }
    // the photograph and the mask of the lane's four pixels
    const float *in_b = input_hwc + (size_t)b * 3u * HW;
    const uint8_t *mk_b = mask + (size_t)b * mask_stride;
    float in[4][3];
    uint8_t mk[4];
    if (VEC) {
        float4 t[3];
        uint32_t w = 0;
        if (q < HW) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                t[i] = *reinterpret_cast<const float4 *>(in_b + 3u * (size_t)q + 4 * i);
            w = *reinterpret_cast<const uint32_t *>(mk_b + q);
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                t[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        const float flat[12] = {t[0].x, t[0].y, t[0].z, t[0].w, t[1].x, t[1].y, t[1].z, t[1].w, t[2].x, t[2].y, t[2].z, t[2].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                in[k][c] = flat[3 * k + c];
            mk[k] = (uint8_t)(w >> (8 * k));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t p = quad_pixel<false>(q, k);
            const bool ok = p < HW;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                in[k][c] = ok ? in_b[3u * (size_t)p + c] : 0.0f;
            mk[k] = ok ? mk_b[p] : (uint8_t)0;
        }
    }
    double m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        m[k] = mask3_value(mk[k], mask_quotient_f32(mk[k]), mask_f32);
#pragma unroll
    for (int j = 0; j < kFrameTile; ++j) {
        if (f0 + (uint32_t)j >= F)                                                 // (uniform)
            break;
        uint8_t *out = frames + ((size_t)b * F + f0 + (uint32_t)j) * 3u * HW;
        if (VEC) {
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int i = 3 * k + c;
                    w[i / 4] |= (uint32_t)composite_u8(in[k][c], acc[j][c][k], m[k]) << (8 * (i % 4));
                }
            if (q < HW) {
                uint32_t *o = reinterpret_cast<uint32_t *>(out + 3u * (size_t)q);
                o[0] = w[0], o[1] = w[1], o[2] = w[2];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t p = quad_pixel<false>(q, k);
                if (p < HW) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        out[3u * (size_t)p + c] = composite_u8(in[k][c], acc[j][c][k], m[k]);
                }
            }
        }
    }
}

}  // namespace gcfr

using namespace gcfr;

extern "C" int gcfr_light_rig_frames_u8(const float *final_shading, const float *albedo, const float *input_hwc, const uint8_t *mask,
                                        int32_t mask_batch, int32_t mask_f32, const float *rgb, int32_t rgb_batch, int32_t B,
                                        int32_t L, int32_t F, int32_t H, int32_t W, uint8_t *frames, void *stream)
{
    if (!final_shading || !albedo || !input_hwc || !mask || !rgb || !frames || B < 1 || L < 1 || L > kFramesMaxLights || F < 1 ||
        F > kFramesMaxFrames || H < 1 || W < 1 || (mask_batch != 1 && mask_batch != B) || (rgb_batch != 1 && rgb_batch != B) ||
        (mask_f32 != 0 && mask_f32 != 1))
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint64_t HW64 = (uint64_t)H * (uint64_t)W;
    if (HW64 > 0x7fffffffull || (uint64_t)B * ((HW64 + kQuadChunk - 1) / kQuadChunk) > 0x7fffffffull)   // one workgroup per face and chunk
        return GCFR_ERR_INVALID_ARGUMENT;
    const uint32_t HW = (uint32_t)HW64, chunks = (HW + kQuadChunk - 1) / kQuadChunk;
    const uint32_t rgb_stride = rgb_batch == 1 ? 0u : 3u * (uint32_t)F * (uint32_t)L;
    const uint32_t mask_stride = mask_batch == 1 ? 0u : HW;
    const bool vec = quad_vec_ok(HW, final_shading, albedo, input_hwc) && aligned4(mask) && aligned4(frames);
    const dim3 grid((uint32_t)B * chunks, ((uint32_t)F + kFrameTile - 1) / kFrameTile), block(kQuadLanes);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(light_rig_frames_kernel<true>, grid, block, 0, st, final_shading, albedo, input_hwc, mask, mask_stride,
                           mask_f32, rgb, rgb_stride, (uint32_t)L, (uint32_t)F, HW, chunks, frames);
    else
        hipLaunchKernelGGL(light_rig_frames_kernel<false>, grid, block, 0, st, final_shading, albedo, input_hwc, mask, mask_stride,
                           mask_f32, rgb, rgb_stride, (uint32_t)L, (uint32_t)F, HW, chunks, frames);
    return hipGetLastError() == hipSuccess ? GCFR_OK : GCFR_ERR_LAUNCH;
}
