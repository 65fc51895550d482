"""Light rigs: L weighted, coloured directional lights combined into ONE relit image per face (csrc/gcfr_light_rig.hip).

The many-lights form of the block returns L separate images, each under one white light.  A rig -- an area light as a cone of
directions, a coloured key / fill / rim set, an environment sampled into a few dozen directions -- is their weighted sum:

    shading_rgb[b,c] = sum_l light_rgb[b,l,c] * final_shading[b,l]          rendered[b,c] = albedo[b,c] * shading_rgb[b,c]

`light_rgb` is colour x weight per light and weights the whole per-light shading, its ambient term included: weights that sum
to 1 count the ambient once.  One fused HIP launch forward and one backward; the order of operations is part of the contract
(include/gcfr.h), so that one light of colour 1 is the block's own composite bit for bit.  There is no CPU path.

    combine_lights          the operation, differentiable with respect to final_shading, albedo and light_rgb
    render_rig_from_depth   block.render_from_depth in its many-lights form + combine_lights on its final_shading
    area_light              n directions on a spherical cap (a deterministic Fibonacci spiral) and their weights, on the host
"""
import math

import numpy as np
import torch

from . import _lib
from .block import RenderParams, render_from_depth

MAX_LIGHTS = 4096      # include/gcfr.h: 1 <= L <= 4096


def _launch_fwd(final, albedo, rgb, rendered, shading):
    B, L, H, W = final.shape
    dev = final.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gcfr_light_rig_fwd(final.data_ptr(), albedo.data_ptr(), rgb.data_ptr(), rgb.shape[0], B, L, H, W,
                                                  rendered.data_ptr(), shading.data_ptr(), _lib.stream_ptr(dev)),
                   "gcfr_light_rig_fwd")


def _launch_bwd(final, albedo, rgb, g_rendered, g_shading, g_final, g_albedo, g_rgb):
    B, L, H, W = final.shape
    dev = final.device
    ptr = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gcfr_light_rig_bwd(final.data_ptr(), albedo.data_ptr(), rgb.data_ptr(), rgb.shape[0], B, L, H, W,
                                                  ptr(g_rendered), ptr(g_shading), ptr(g_final), ptr(g_albedo), ptr(g_rgb),
                                                  _lib.stream_ptr(dev)), "gcfr_light_rig_bwd")


class _CombineLightsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, final, albedo, rgb):
        rendered, shading = torch.empty_like(albedo), torch.empty_like(albedo)
        _launch_fwd(final, albedo, rgb, rendered, shading)
        ctx.save_for_backward(final, albedo, rgb)
        ctx.set_materialize_grads(False)          # an unused output's gradient arrives as None -> NULL, not as a tensor of zeros
        return rendered, shading

    @staticmethod
    def backward(ctx, g_rendered, g_shading):
        final, albedo, rgb = ctx.saved_tensors
        if g_rendered is None and g_shading is None:
            return None, None, None
        want_final, want_albedo, want_rgb = ctx.needs_input_grad
        if not (want_final or want_albedo or want_rgb):
            return None, None, None
        g_final = torch.empty_like(final) if want_final else None
        g_albedo = torch.empty_like(albedo) if want_albedo else None
        g_rgb = torch.zeros(rgb.shape, dtype=torch.float64, device=rgb.device) if want_rgb else None      # accumulated in f64
        _launch_bwd(final, albedo, rgb, _lib.f32c(g_rendered), _lib.f32c(g_shading), g_final, g_albedo, g_rgb)
        return g_final, g_albedo, (g_rgb.float() if want_rgb else None)


def _check_combine(final_shading, albedo, light_rgb):
    """Every shape, dtype and device BEFORE anything is launched or loaded: a mismatch never reaches the kernel."""
    names = ("final_shading", "albedo", "light_rgb")
    tensors = (final_shading, albedo, light_rgb)
    for n, t in zip(names, tensors):
        if not torch.is_tensor(t):
            raise _lib.GcfrError("combine_lights: %s must be a tensor, got %s" % (n, type(t).__name__))
    for n, t in zip(names, tensors):
        if t.dtype != torch.float32:
            raise _lib.GcfrError("combine_lights: %s must be float32, got %s" % (n, t.dtype))
    if any(t.device != final_shading.device for t in tensors):
        raise _lib.GcfrError("combine_lights: tensors on one device; got %s" % ", ".join(str(t.device) for t in tensors))
    if final_shading.dim() != 4:
        raise _lib.GcfrError("final_shading must be (B,L,H,W) -- the many-lights form, with its light axis; got %s"
                             % (tuple(final_shading.shape),))
    B, L, H, W = final_shading.shape
    if B < 1 or H < 1 or W < 1 or not 1 <= L <= MAX_LIGHTS:
        raise _lib.GcfrError("final_shading (B,L,H,W) = %s: B, H, W >= 1 and 1 <= L <= %d" % (tuple(final_shading.shape), MAX_LIGHTS))
    if tuple(albedo.shape) != (B, 3, H, W):
        raise _lib.GcfrError("albedo must be %s (per face, no light axis) for final_shading %s; got %s"
                             % ((B, 3, H, W), tuple(final_shading.shape), tuple(albedo.shape)))
    if light_rgb.dim() != 3 or tuple(light_rgb.shape[1:]) != (L, 3) or light_rgb.shape[0] not in (1, B):
        raise _lib.GcfrError("light_rgb must be (%d,%d,3) or (1,%d,3) for final_shading %s; got %s"
                             % (B, L, L, tuple(final_shading.shape), tuple(light_rgb.shape)))
    _lib.require_device(final_shading)


def combine_lights(final_shading: torch.Tensor, albedo: torch.Tensor, light_rgb: torch.Tensor):
    """(rendered (B,3,H,W), shading_rgb (B,3,H,W)) of the many-lights `final_shading` (B,L,H,W), `albedo` (B,3,H,W) and the rig
    `light_rgb` (B,L,3), or (1,L,3) for one rig shared by all faces: colour x weight per light.  All f32 on one ROCm device.
    shading_rgb[b,c] = sum_l light_rgb[b,l,c] final_shading[b,l] in ascending l, each product and sum rounded separately, the
    first product initialising; rendered = albedo * shading_rgb.  Nothing is clamped: zero and negative weights are legal and
    non-finite values propagate.  Differentiable with respect to all three inputs (the gradient of a shared rig is summed over
    the faces).  A malformed input raises GcfrError before any launch."""
    _check_combine(final_shading, albedo, light_rgb)
    return _CombineLightsFunction.apply(final_shading.contiguous(), albedo.contiguous(), light_rgb.contiguous())


def render_rig_from_depth(depth, albedo, light, ambient, light_rgb, camera_matrix, z_offset, mask,
                          params: RenderParams = RenderParams(), prepared=None):
    """`block.render_from_depth` in its many-lights form (light (B,L,3), ambient (B,L)) followed by `combine_lights` on its
    final_shading with the rig `light_rgb` (B,L,3) | (1,L,3).  Returns that call's dict (every per-light tensor with its light
    axis, unchanged) plus `rig_rendered_images` (B,3,H,W) and `rig_shading` (B,3,H,W).  Gradients reach depth, albedo, light,
    ambient and light_rgb: the rig stage's gradient enters the block's fused backward through final_shading, summed by autograd
    with whatever the caller puts on the per-light outputs."""
    B = depth.shape[0]
    if light.dim() != 3 or light.shape[0] != B or light.shape[2] != 3:
        raise _lib.GcfrError("render_rig_from_depth needs the many-lights form: light (B,L,3), ambient (B,L); got light %s"
                             % (tuple(light.shape),))
    r = render_from_depth(depth, albedo, light, ambient, camera_matrix, z_offset, mask, params, prepared=prepared)
    rendered, shading = combine_lights(r["final_shading"], albedo.to(torch.float32), light_rgb)
    r["rig_rendered_images"], r["rig_shading"] = rendered, shading
    return r


def _spiral_cap(axis, e1, e2, radius, n):
    """n unit vectors (f64) on the cap of `radius` radians around `axis`: point i at cos(theta_i) = 1 - (1 - cos radius)(i + 1/2) / n
    (equal areas per point, all strictly inside the cap) and at azimuth i times the golden angle, then rotated as a rigid set
    so that their mean points along `axis` exactly (a rotation is linear: the rotated mean is the mean's rotation)."""
    i = np.arange(n, dtype=np.float64)
    cos_t = 1.0 - (1.0 - math.cos(radius)) * (i + 0.5) / n
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    pts = cos_t[:, None] * axis + (sin_t * np.cos(phi))[:, None] * e1 + (sin_t * np.sin(phi))[:, None] * e2
    m = pts.mean(axis=0)
    m /= np.linalg.norm(m)
    v, c = np.cross(m, axis), float(np.dot(m, axis))                     # Rodrigues: the rotation that takes m to axis
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    rot = np.eye(3) + vx + vx @ vx / (1.0 + c)
    pts = pts @ rot.T
    return pts / np.linalg.norm(pts, axis=1, keepdims=True)


def area_light(direction, angular_radius_deg: float, n: int, colour=(1.0, 1.0, 1.0)):
    """An area light as n directional lights: (lights (n,3) f32 unit directions, light_rgb (n,3) f32 = colour / n each).
    The directions are a Fibonacci spiral on the spherical cap of `angular_radius_deg` (0 .. 90) around `direction`
    (`_spiral_cap`): equal areas per point, every point inside the cap, and the set's mean direction is `direction` itself,
    so the rig lights the face from where the one light would.  n = 1, or a radius of 0, gives `direction` (normalised).
    Deterministic (no random numbers), computed on the host in f64 and rounded to f32 once."""
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    norm = float(np.linalg.norm(d))
    if not (norm > 0.0 and math.isfinite(norm)):
        raise ValueError("area_light: direction must be a finite, non-zero 3-vector; got %r" % (direction,))
    n = int(n)
    if n < 1:
        raise ValueError("area_light: n >= 1; got %d" % n)
    if not 0.0 <= float(angular_radius_deg) <= 90.0:
        raise ValueError("area_light: angular_radius_deg in [0, 90]; got %r" % (angular_radius_deg,))
    axis = d / norm
    colour = np.asarray(colour, dtype=np.float64).reshape(3)
    rgb = np.broadcast_to((colour / n).astype(np.float32), (n, 3)).copy()
    radius = math.radians(float(angular_radius_deg))
    if n == 1 or radius == 0.0:
        return np.broadcast_to(axis.astype(np.float32), (n, 3)).copy(), rgb
    # an orthonormal frame (e1, e2, axis): e1 from the coordinate axis least aligned with `axis`
    helper = np.zeros(3)
    helper[int(np.argmin(np.abs(axis)))] = 1.0
    e1 = np.cross(helper, axis)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(axis, e1)
    # centring the mean tilts the spiral by the (small) angle between its mean and the axis, which can push its outermost point
    # past the rim: the spiral is then drawn on a proportionally smaller cap (a few iterations of a contraction, fixed count)
    r = radius
    for _ in range(8):
        pts = _spiral_cap(axis, e1, e2, r, n)
        worst = float(np.arccos(np.clip(pts @ axis, -1.0, 1.0)).max())
        if worst <= radius:
            break
        r *= (radius / worst) * (1.0 - 1e-9)
    else:
        raise ValueError("area_light: no spiral of %d points fits the cap of %r degrees" % (n, angular_radius_deg))
    return pts.astype(np.float32), rgb
