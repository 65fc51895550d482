"""The rig-frames kernel's contract (csrc/gcfr_rig_frames.hip, include/gcfr.h), stated in numpy (helper module, no tests): frame
[b,f] is the rig stage's restatement (tests/light_rig_emulation.py `forward`) with rig f, pasted into the photograph and quantised
by the statements of the reference's scripts (oracle/postprocess_statements.py `composite_into_input`, `to_uint8`) -- three
functions that exist already, composed per frame and per face.  It shares no code with either kernel.

Arrays in the C ABI's layouts: final (B,L,H,W) f32, albedo (B,3,H,W) f32, images (B,H,W,3) f32, mask (MB,H,W) u8 with MB in {1, B},
rgb (RB,F,L,3) f32 with RB in {1, B}; -> frames (B,F,H,W,3) u8."""
import os
import sys

import numpy as np

import light_rig_emulation as rig

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import postprocess_statements as pps  # noqa: E402  (checker only)


def mask_value(mask_u8, mask_f32):
    """the mask the scripts hold, f64: the u8 mask / 255.0 in f64 (S1:580), or with mask_f32 the f32 quotient, widened (SLT:540)"""
    assert mask_u8.dtype == np.uint8
    if mask_f32:
        return (mask_u8.astype(np.float32) / np.float32(255.0)).astype(np.float64)
    return mask_u8.astype(np.float64) / 255.0


def frame(final, albedo, images, mask_u8, rgb_f, mask_f32=False):
    """ONE frame: rgb_f (RB,L,3) -> (B,H,W,3) u8"""
    B = final.shape[0]
    rendered, _ = rig.forward(final, albedo, rgb_f)
    m = mask_value(mask_u8, mask_f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([pps.to_uint8(pps.composite_into_input(images[b], rendered[b], m[b if m.shape[0] > 1 else 0]))
                         for b in range(B)])


def frames(final, albedo, images, mask_u8, rgb, mask_f32=False):
    """-> (B,F,H,W,3) u8"""
    B, L, H, W = final.shape
    assert images.shape == (B, H, W, 3) and images.dtype == np.float32
    assert mask_u8.shape[1:] == (H, W) and mask_u8.shape[0] in (1, B)
    assert rgb.ndim == 4 and rgb.shape[2:] == (L, 3) and rgb.shape[0] in (1, B) and rgb.dtype == np.float32
    return np.stack([frame(final, albedo, images, mask_u8, np.ascontiguousarray(rgb[:, f]), mask_f32) for f in range(rgb.shape[1])],
                    axis=1)
