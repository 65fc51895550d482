// The composite byte of the inference scripts (S1:601-620, S8:596-602, SLT:567-572), shared by the image kernel
// (gcfr_postprocess.hip) and the rig-frames kernel (gcfr_rig_frames.hip) so that the two cannot drift: the mask's value, the
// paste / keep expression and the quantisation.  The dtypes are the reference's (gcfr_postprocess.hip's header states them).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gcfr {

__device__ inline uint8_t quantise_u8(double v)
{
    const double r = __builtin_rint(v);  // cvRound: round half to even
    return (uint8_t)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));  // NaN -> 0 (saturate_cast of INT_MIN)
}

// the u8 mask / 255.0 in f32                                              SLT:540 (torch: u8 -> f32, IEEE division)
__device__ inline float mask_quotient_f32(uint8_t mk) { return (float)mk / 255.0f; }

// value of mask_3_channels (an f64 array): mask_f32 = 0 the f64 quotient (S1:580), 1 the f32 quotient `mf`, widened
__device__ inline double mask3_value(uint8_t mk, float mf, int mask_f32) { return mask_f32 ? (double)mf : (double)mk / 255.0; }

// input_image = training_images*255.0; rendered_image = 255.0*rendered*mask; input[mask > 0] = rendered[mask > 0]
__device__ inline uint8_t composite_u8(float input, float rendered, double m)
{
    const double keep = (double)input * 255.0;
    const double paste = (double)(255.0f * rendered) * m;
    return quantise_u8(m > 0.0 ? paste : keep);
}

}  // namespace gcfr
