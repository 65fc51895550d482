"""The light-rig stage's operation order (csrc/gcfr_light_rig.hip, include/gcfr.h), restated in numpy: every f32 operation of the
kernels as one numpy float32 operation in the same order, the rig's gradient summed in f64.  tests/test_gpu_light_rig.py holds
the kernels to it -- rendered, shading_rgb, g_final and g_albedo bit for bit, g_rgb within one f32 rounding of the f64 sum -- and
tests/test_light_rig_host.py holds it to f64 torch autograd of the plain expression, so that it is a checked statement and not
a second opinion.

Arrays are float32 in the C ABI's layouts: final (B,L,H,W), albedo (B,3,H,W), rgb (B,L,3) or (1,L,3); the upstream gradients
g_rendered / g_shading (B,3,H,W) or None each."""
import numpy as np

from f32_bits import F32, _f, bit_equal  # noqa: F401  (bit_equal: for the tests)


def _shapes(final, albedo, rgb):
    _f(final), _f(albedo), _f(rgb)
    B, L, H, W = final.shape
    assert albedo.shape == (B, 3, H, W) and rgb.shape[1:] == (L, 3) and rgb.shape[0] in (1, B)
    return B, L, H, W


def _rig(rgb, B):
    """(B,L,3): the shared rig repeated per face"""
    return np.broadcast_to(rgb, (B,) + rgb.shape[1:])


def shading(final, albedo, rgb):
    """shading_rgb (B,3,H,W): acc = rgb[0,c] final[0]; acc = acc + rgb[l,c] final[l], l ascending; no add to zero"""
    B, L, H, W = _shapes(final, albedo, rgb)
    r = _rig(rgb, B)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = _f(r[:, 0, :, None, None] * final[:, 0, None])
        for l in range(1, L):
            acc = _f(acc + _f(r[:, l, :, None, None] * final[:, l, None]))
    return acc


def forward(final, albedo, rgb):
    """-> rendered (B,3,H,W), shading_rgb (B,3,H,W); the albedo product comes last"""
    sh = shading(final, albedo, rgb)
    with np.errstate(invalid="ignore", over="ignore"):
        return _f(albedo * sh), sh


def upstream(albedo, g_rendered, g_shading):
    """u = g_shading + g_rendered albedo; an absent term is not formed"""
    assert g_rendered is not None or g_shading is not None
    with np.errstate(invalid="ignore", over="ignore"):
        if g_rendered is None:
            return _f(g_shading)
        t = _f(_f(g_rendered) * albedo)
        return t if g_shading is None else _f(_f(g_shading) + t)


def backward(final, albedo, rgb, g_rendered, g_shading):
    """-> dict: g_final (B,L,H,W) f32, g_albedo (B,3,H,W) f32, g_rgb (rgb's shape) f32 = the f64 sum rounded once,
    g_rgb_f64 the sum itself, g_rgb_bound = 2^-23 sum_p |final u| per entry (one f32 rounding of a sum whose order is free)"""
    B, L, H, W = _shapes(final, albedo, rgb)
    r = _rig(rgb, B)
    u = upstream(albedo, g_rendered, g_shading)
    with np.errstate(invalid="ignore", over="ignore"):
        g_final = np.empty((B, L, H, W), F32)
        for l in range(L):
            g = _f(r[:, l, 0, None, None] * u[:, 0])
            g = _f(g + _f(r[:, l, 1, None, None] * u[:, 1]))
            g_final[:, l] = _f(g + _f(r[:, l, 2, None, None] * u[:, 2]))
        if g_rendered is None:
            g_albedo = np.zeros(albedo.shape, F32)
        else:
            g_albedo = _f(_f(g_rendered) * shading(final, albedo, rgb))
        prod = final.astype(np.float64)[:, :, None] * u.astype(np.float64)[:, None]          # (B,L,3,H,W), exact in f64
        s, a = prod.sum(axis=(3, 4)), np.abs(prod).sum(axis=(3, 4))
        if rgb.shape[0] == 1:
            s, a = s.sum(axis=0, keepdims=True), a.sum(axis=0, keepdims=True)
    return {"g_final": g_final, "g_albedo": g_albedo, "g_rgb": s.astype(F32), "g_rgb_f64": s, "g_rgb_bound": a * 2.0 ** -23}
