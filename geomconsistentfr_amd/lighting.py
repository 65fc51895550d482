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

Environment maps (csrc/gcfr_environment.hip): a lat-long radiance map becomes the `light_rgb` of a rig of L fixed directions -- every
texel belongs to the direction nearest to it, a light's rgb is the solid-angle-weighted sum of its texels.  Rotating the map changes
`light_rgb` only, so a turntable needs one network pass and L marches in total.

    environment_tables             the map's trigonometry and solid-angle weights, on the host (no kernel evaluates a sine)
    sphere_directions              n directions on the part of the sphere the block can light from (a deterministic Fibonacci spiral)
    environment_lights             the stage: map + directions (+ rotation) -> light_rgb, differentiable with respect to the map
    render_environment_from_depth  render_rig_from_depth with light_rgb taken from the stage

Rig frames (csrc/gcfr_rig_frames.hip): F rigs per face -- an animated rig, a turntable of an environment map -- from ONE many-lights
pass, straight to uint8 frames in one launch.

    rig_frames_u8                  final_shading + albedo + photographs + mask + light_rgb_frames (B|1,F,L,3) -> (B,F,H,W,3) uint8
    environment_lights_frames      environment_lights for F rotations at once -> light_rgb_frames (E,F,L,3): two launches

Rig capture (csrc/gcfr_light_fit.hip), the inverse of the rig stage: the `light_rgb` under which the per-light shadings come closest
to a photograph, a weighted least-squares problem per face and channel -- "light this face like that photograph".

    light_normal_equations         the weighted Gram matrix and right-hand side over all pixels, f64 in a fixed order
    fit_light_rgb                  the normal equations + a Cholesky solve with a relative ridge -> light_rgb (not differentiable);
                                   `nonnegative=True`: the same system under light_rgb >= 0, by an active-set method
"""
import math

import numpy as np
import torch

from . import _lib
from .block import RenderParams, render_from_depth

MAX_LIGHTS = 4096      # include/gcfr.h: 1 <= L <= 4096


class _CombineLightsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, final, albedo, rgb):
        rendered, shading = torch.empty_like(albedo), torch.empty_like(albedo)
        B, L, H, W = final.shape
        _lib.launch("gcfr_light_rig_fwd", final.device, final, albedo, rgb, rgb.shape[0], B, L, H, W, rendered, shading, _lib.STREAM)
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
        B, L, H, W = final.shape
        _lib.launch("gcfr_light_rig_bwd", final.device, final, albedo, rgb, rgb.shape[0], B, L, H, W, _lib.f32c(g_rendered),
                    _lib.f32c(g_shading), g_final, g_albedo, g_rgb, _lib.STREAM)
        return g_final, g_albedo, (g_rgb.float() if want_rgb else None)


def _many_lights(final_shading, max_lights):
    """-> (B, L, H, W) of a many-lights `final_shading`, each at least 1 and L at the most `max_lights`"""
    if final_shading.dim() != 4:
        raise _lib.GcfrError("final_shading must be (B,L,H,W) -- the many-lights form, with its light axis; got %s"
                             % (tuple(final_shading.shape),))
    B, L, H, W = final_shading.shape
    if B < 1 or H < 1 or W < 1 or not 1 <= L <= max_lights:
        raise _lib.GcfrError("final_shading (B,L,H,W) = %s: B, H, W >= 1 and 1 <= L <= %d" % (tuple(final_shading.shape), max_lights))
    return B, L, H, W


def _check_combine(final_shading, albedo, light_rgb):
    """Every shape, dtype and device BEFORE anything is launched or loaded: a mismatch never reaches the kernel."""
    tensors = _lib.check_tensors("combine_lights", [("final_shading", final_shading), ("albedo", albedo), ("light_rgb", light_rgb)])
    B, L, H, W = _many_lights(final_shading, MAX_LIGHTS)
    _lib.check_shape("albedo", albedo, (B, 3, H, W), why=" (per face, no light axis) for final_shading %s" % (tuple(final_shading.shape),))
    _lib.check_shape("light_rgb", light_rgb, (B, L, 3), (1, L, 3), why=" for final_shading %s" % (tuple(final_shading.shape),))
    _lib.require_device(*tensors)


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


# ------------------------------------------------------------------------------------------------------------------------------
# environment maps
# ------------------------------------------------------------------------------------------------------------------------------
MAX_TEXELS = 1 << 24   # include/gcfr.h: He We <= 2^24


def environment_tables(He: int, We: int):
    """The tables the environment kernels read instead of evaluating trigonometry, for a lat-long map of He rows and We columns:
    (rows (He,2) f32 = sin, cos theta_r; row_w (He,) f64; cols (We,2) f32 = sin, cos phi_c), computed on the host in f64 and
    rounded once.  Texel (r, c) looks along omega = (sin theta sin phi, cos theta, sin theta cos phi) in the block's frame, the
    one light directions are given in: +x towards the image's right (increasing column), +y UP in the image (towards row 0 of the
    photograph: `LIGHT_DIRECTIONS["top_A00E45"]` has y > 0), +z from the face towards the camera.
    theta_r = pi (r + 1/2) / He is measured from +y: row 0 of the map is the sky above the head, the last row the ground.
    phi_c = 2 pi (c + 1/2) / We - pi: the map's centre column faces +z, the side the camera and the front lights are on; columns
    right of the centre have omega_x > 0, and the two outer columns meet behind the head.
    row_w[r] = (cos theta_top - cos theta_bottom) / (2 We) with theta_top = pi r / He, theta_bottom = pi (r + 1) / He: the band's
    exact solid angle per texel over 4 pi, so the weights of all He We texels sum to 1 and a constant map of radiance 1 gives
    weights that count the rig stage's ambient term once."""
    He, We = int(He), int(We)
    if He < 1 or We < 1 or He * We > MAX_TEXELS:
        raise ValueError("environment_tables: He, We >= 1 and He We <= 2^24; got %d x %d" % (He, We))
    theta = math.pi * (np.arange(He, dtype=np.float64) + 0.5) / He
    edge = np.cos(math.pi * np.arange(He + 1, dtype=np.float64) / He)
    edge[0], edge[-1] = 1.0, -1.0
    phi = 2.0 * math.pi * (np.arange(We, dtype=np.float64) + 0.5) / We - math.pi
    rows = np.stack([np.sin(theta), np.cos(theta)], axis=1).astype(np.float32)
    cols = np.stack([np.sin(phi), np.cos(phi)], axis=1).astype(np.float32)
    return rows, (edge[:-1] - edge[1:]) / (2.0 * We), cols


def sphere_directions(n: int, min_z: float = 0.2) -> np.ndarray:
    """n unit directions (n,3) f32 on the part z >= min_z of the sphere, an equal-area Fibonacci spiral: point i at
    z_i = 1 - (1 - min_z)(i + 1/2) / n (every point strictly inside the cap) and at azimuth i times the golden angle.
    Deterministic, computed on the host in f64 and rounded once.  The default keeps clear of the lighting-transfer model's clamp
    of a light's z (`clamp_min` 0.16), so that the block lights the face from where the map's cell is; min_z = -1 gives the whole
    sphere (lights behind the face shade nothing but still take their share of the map)."""
    n, min_z = int(n), float(min_z)
    if not 1 <= n <= MAX_LIGHTS:
        raise ValueError("sphere_directions: 1 <= n <= %d; got %d" % (MAX_LIGHTS, n))
    if not -1.0 <= min_z < 1.0:
        raise ValueError("sphere_directions: min_z in [-1, 1); got %r" % (min_z,))
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (1.0 - min_z) * (i + 0.5) / n
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1).astype(np.float32)


_ENV_TABLES = {}       # (He, We, device) -> (rows, row_w, cols) on the device: uploaded once, never written, never evicted


def _device_tables(He, We, device):
    """the tables of a (He, We) map on `device`.  The FIRST call per (He, We, device) builds them on the host and uploads them (a
    pageable host-to-device copy: not for a stream that is being captured); every later call only looks them up"""
    key = (He, We, str(device))
    if key not in _ENV_TABLES:
        _ENV_TABLES[key] = tuple(torch.from_numpy(a).to(device) for a in environment_tables(He, We))
    return _ENV_TABLES[key]


class _EnvironmentLightsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, env, dirs_map, min_cos, out):
        E, He, We, _ = env.shape
        L = dirs_map.shape[0]
        rows, row_w, cols = _device_tables(He, We, env.device)
        cell = torch.empty((He, We), dtype=torch.int32, device=env.device)
        rgb = torch.empty((E, L, 3), dtype=torch.float32, device=env.device) if out is None else out
        _lib.launch("gcfr_environment_cells", env.device, rows, cols, dirs_map, He, We, L, float(min_cos), cell, _lib.STREAM)
        _lib.launch("gcfr_environment_fwd", env.device, env, E, He, We, row_w, cell, L, rgb, _lib.STREAM)
        ctx.save_for_backward(row_w, cell)
        ctx.env_shape = tuple(env.shape)
        if out is not None:
            ctx.mark_dirty(out)
        return rgb

    @staticmethod
    def backward(ctx, g_rgb):
        row_w, cell = ctx.saved_tensors
        if g_rgb is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        g_env = torch.empty(ctx.env_shape, dtype=torch.float32, device=cell.device)
        E, He, We, _ = ctx.env_shape
        g_rgb = _lib.f32c(g_rgb)
        _lib.launch("gcfr_environment_bwd", cell.device, g_rgb, row_w, cell, E, He, We, g_rgb.shape[1], g_env, _lib.STREAM)
        return g_env, None, None, None          # (no gradient to the directions: the cell map is piecewise constant in them)


def _check_environment(env, directions, rotation, out, faces=None, frames=None):
    """Every shape, dtype and device BEFORE anything is launched or loaded: a mismatch never reaches the kernels.  `faces`: the
    batch the maps are for (E must be 1 or that).  `frames`: `out` is the frames form's, (E,frames,L,3).  `rotation` may be a
    host tensor (it is uploaded), so it is held to no device."""
    _lib.check_tensors("environment_lights", [("env", env), ("directions", directions), ("out", out)])
    _lib.check_tensors("environment_lights", [("rotation", rotation)])
    if env.dim() != 4 or env.shape[3] != 3:
        raise _lib.GcfrError("env must be (E,He,We,3) -- a lat-long map per face, or E = 1 for one map; got %s" % (tuple(env.shape),))
    E, He, We, _ = env.shape
    if E < 1 or He < 1 or We < 1 or He * We > MAX_TEXELS:
        raise _lib.GcfrError("env (E,He,We,3) = %s: E, He, We >= 1 and He We <= 2^24" % (tuple(env.shape),))
    if faces is not None and E not in (1, faces):
        raise _lib.GcfrError("env must be (1,He,We,3) or (%d,He,We,3) for %d faces; got %s" % (faces, faces, tuple(env.shape)))
    if directions.dim() != 2 or directions.shape[1] != 3 or not 1 <= directions.shape[0] <= MAX_LIGHTS:
        raise _lib.GcfrError("directions must be (L,3) with 1 <= L <= %d; got %s" % (MAX_LIGHTS, tuple(directions.shape)))
    if rotation is not None:
        _lib.check_shape("rotation", rotation, (3, 3))
    L = directions.shape[0]
    _lib.check_out(out, (E, L, 3) if frames is None else (E, frames, L, 3))
    _lib.require_device(env, directions, out)


def environment_lights(env: torch.Tensor, directions: torch.Tensor, rotation=None, min_cos: float = -2.0, out=None):
    """`light_rgb` (E,L,3) of the lat-long radiance map(s) `env` (E,He,We,3) for the rig of `directions` (L,3): every texel
    belongs to the direction nearest to it (largest dot product; a tie goes to the lowest index) and a light's rgb is the sum of
    its texels' radiance times their solid angle over 4 pi (`environment_tables`).  E = 1 is one map for all faces, E = B one per
    face -- what `combine_lights` takes.  All f32 tensors on one ROCm device.  Nothing is clamped: negative radiance is legal, a
    non-finite texel reaches its own light's entry only.
    `rotation` (3,3), a device or host tensor: the rig is looked up in the map at `directions @ rotation`.  With R = rotation
    as a matrix acting on column vectors, what the map shows in direction m lights the face from R m: R = I leaves the map's
    centre column in front of the face, a rotation about +y by an angle a turns the environment around the head by a.  The
    product is torch's, on the device; a host `rotation` is uploaded first (pass a device tensor to keep the call asynchronous).
    `min_cos`: a texel whose best dot product is below it belongs to no light (the default drops nothing); its radiance is
    then not counted, so the weights no longer sum to 1.
    `out`: a contiguous (E,L,3) f32 buffer the result is written into and which is returned -- `RelightSession.light_rgb`
    between two replays, for example: no output is allocated and the host never waits.
    The tables of a map size are uploaded by the first call for that (He, We, device) and kept for the life of the process
    (three small tensors per size).  Make that first call OUTSIDE a stream capture -- a warm-up call on the same map size does
    it -- since the upload is a pageable host-to-device copy; every later call launches the two kernels and nothing else.
    Differentiable with respect to `env` (a gather of the upstream gradient); the directions and the rotation receive no
    gradient, the cell assignment being piecewise constant in them.  Two launches forward, one backward; the order of the
    f64 sum is fixed (include/gcfr.h), so equal inputs give equal bits.  A malformed input raises GcfrError before any launch."""
    _check_environment(env, directions, rotation, out)
    dirs_map = directions.detach()
    if rotation is not None:
        dirs_map = dirs_map @ rotation.detach().to(env.device)
    return _environment_lights(env, dirs_map, min_cos, out)


def _environment_lights(env, dirs_map, min_cos, out):
    """environment_lights behind its checks, on directions already in the map's frame"""
    return _EnvironmentLightsFunction.apply(env.contiguous(), dirs_map.contiguous(), float(min_cos), out)


def render_environment_from_depth(depth, albedo, directions, ambient, env, camera_matrix, z_offset, mask,
                                  params: RenderParams = RenderParams(), prepared=None, rotation=None, min_cos: float = -2.0):
    """`render_rig_from_depth` with the rig's `light_rgb` taken from `environment_lights(env, directions, rotation, min_cos)`:
    every face is lit from the L `directions` (L,3) (ambient (B,L), the many-lights form) and the per-light shadings are combined
    with the map's colour x weight per light.  `env` (1,He,We,3) is one map for all faces, (B,He,We,3) one per face.  Returns
    that call's dict plus `light_rgb` (E,L,3).  Gradients reach depth, albedo, ambient and `env`."""
    B = depth.shape[0]
    _check_environment(env, directions, rotation, None, faces=B)
    light_rgb = environment_lights(env, directions, rotation, min_cos)
    light = directions.detach()[None].expand(B, -1, -1).contiguous()
    r = render_rig_from_depth(depth, albedo, light, ambient, light_rgb, camera_matrix, z_offset, mask, params, prepared=prepared)
    r["light_rgb"] = light_rgb
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# rig frames: F rigs per face, one launch, uint8 frames
# ------------------------------------------------------------------------------------------------------------------------------
MAX_FRAMES = 4096          # include/gcfr.h: 1 <= F <= 4096
RIG_FRAMES_TILE = 4        # csrc/gcfr_rig_frames.hip kFrameTile: frames per workgroup; final_shading is read ceil(F / 4) times


def _check_rig_frames(final_shading, albedo, images, mask_u8, light_rgb_frames, out):
    """Every tensor that is passed by pointer -- shape, dtype, device -- BEFORE anything is launched or loaded."""
    tensors = _lib.check_tensors("rig_frames_u8", [("final_shading", final_shading), ("albedo", albedo), ("images", images),
                                                   ("mask_u8", mask_u8), ("light_rgb_frames", light_rgb_frames), ("out", out)],
                                 mask_u8=torch.uint8, out=torch.uint8)
    B, L, H, W = _many_lights(final_shading, MAX_LIGHTS)
    of = " for final_shading %s" % (tuple(final_shading.shape),)
    if H * W >= 2 ** 31 or B * ((H * W + 1023) // 1024) >= 2 ** 31:
        raise _lib.GcfrError("final_shading (B,L,H,W) = %s: H W < 2^31 and B ceil(H W / 1024) < 2^31" % (tuple(final_shading.shape),))
    _lib.check_shape("albedo", albedo, (B, 3, H, W), why=of)
    _lib.check_shape("images", images, (B, H, W, 3), why=" (the photographs, HWC)" + of)
    _lib.check_shape("mask_u8", mask_u8, (B, H, W), (1, H, W), (H, W))
    r = light_rgb_frames
    if r.dim() not in (3, 4) or tuple(r.shape[-2:]) != (L, 3) or (r.dim() == 4 and r.shape[0] not in (1, B)):
        raise _lib.GcfrError("light_rgb_frames must be (F,%d,3), (1,F,%d,3) or (%d,F,%d,3)%s; got %s" % (L, L, B, L, of, tuple(r.shape)))
    F = r.shape[-3]
    if not 1 <= F <= MAX_FRAMES:
        raise _lib.GcfrError("light_rgb_frames %s: 1 <= F <= %d frames" % (tuple(r.shape), MAX_FRAMES))
    _lib.check_out(out, (B, F, H, W, 3))
    _lib.require_device(*tensors)
    return B, L, F, H, W


def rig_frames_u8(final_shading: torch.Tensor, albedo: torch.Tensor, images: torch.Tensor, mask_u8: torch.Tensor,
                  light_rgb_frames: torch.Tensor, mask_f32: bool = False, out=None) -> torch.Tensor:
    """(B,F,H,W,3) uint8 frames (RGB, HWC, on the device): every face of the many-lights `final_shading` (B,L,H,W) and `albedo`
    (B,3,H,W) under each of the F rigs `light_rgb_frames` -- (F,L,3) or (1,F,L,3), the same rigs for all faces, or (B,F,L,3) --
    pasted into the photographs `images` (B,H,W,3) f32 through the compositing mask `mask_u8` ((B,H,W), or (1,H,W) / (H,W) shared;
    uint8 as stored on disk).  ONE launch; frame [b,f] equals, byte for byte, `combine_lights(final_shading, albedo,
    light_rgb_frames[:,f])` followed by `postprocess.inference_images_device(images, rendered, mask_u8, mask_f32=...)`: the same
    f32 chain in ascending l and the image kernel's own composite function (include/gcfr.h).  `mask_f32`: the mask's quotient in
    f32 (the lighting-transfer script), else f64.  Nothing is clamped before the quantisation; a NaN gives byte 0.
    `out`: a contiguous (B,F,H,W,3) uint8 buffer the frames are written into and which is returned.  NOT DIFFERENTIABLE: inputs are
    detached.  No host synchronisation; a malformed input (rank, shape, dtype, device, L or F out of range) raises GcfrError before
    anything is loaded or launched, host tensors too.  There is no CPU path."""
    B, L, F, H, W = _check_rig_frames(final_shading, albedo, images, mask_u8, light_rgb_frames, out)
    dev = final_shading.device
    final, alb, x = final_shading.detach().contiguous(), albedo.detach().contiguous(), images.detach().contiguous()
    m = mask_u8.contiguous().reshape(-1, H, W)
    rgb = light_rgb_frames.detach().contiguous().reshape(-1, F, L, 3)
    frames = torch.empty((B, F, H, W, 3), dtype=torch.uint8, device=dev) if out is None else out
    _lib.launch("gcfr_light_rig_frames_u8", dev, final, alb, x, m, m.shape[0], int(bool(mask_f32)), rgb, rgb.shape[0], B, L, F, H, W,
                frames, _lib.STREAM)
    return frames


def _check_rotations(rotations):
    _lib.check_tensors("environment_lights_frames", [("rotations", rotations)])
    if rotations.dim() != 3 or tuple(rotations.shape[1:]) != (3, 3) or not 1 <= rotations.shape[0] <= MAX_FRAMES:
        raise _lib.GcfrError("rotations must be (F,3,3) with 1 <= F <= %d; got %s" % (MAX_FRAMES, tuple(rotations.shape)))


def environment_lights_frames(env: torch.Tensor, directions: torch.Tensor, rotations: torch.Tensor, min_cos: float = -2.0,
                              out=None) -> torch.Tensor:
    """`light_rgb_frames` (E,F,L,3) -- what `rig_frames_u8` takes -- of the lat-long radiance map(s) `env` (E,He,We,3) for the rig
    of `directions` (L,3) under each of the F `rotations` (F,3,3; a device or host tensor): entry [:,f] equals
    `environment_lights(env, directions, rotation=rotations[f], min_cos=min_cos)` bit for bit.  The F rotated direction sets are
    that call's own F small products `directions @ rotations[f]`, stacked afterwards (a batched product could round differently
    and move a cell border); then ONE launch builds the F cell maps and ONE integrates them, both running the single call's
    device code per frame (include/gcfr.h).  `out`: a contiguous (E,F,L,3) f32 buffer the result is written into and which is
    returned.  The tables of a map size are uploaded by the first call for that (He, We, device), as in `environment_lights`: make
    that call outside a stream capture.  NOT DIFFERENTIABLE in this form.  A malformed input raises GcfrError before any launch,
    host `env` / `directions` too."""
    _check_rotations(rotations)
    _check_environment(env, directions, None, out, frames=rotations.shape[0])
    E, He, We, _ = env.shape
    L, F = directions.shape[0], rotations.shape[0]
    if E * F * L >= 2 ** 31:
        raise _lib.GcfrError("environment_lights_frames: E F L < 2^31 (one workgroup per map, frame and light); got %d x %d x %d" % (E, F, L))
    dev = env.device
    d, rots = directions.detach(), rotations.detach().to(dev)
    dirs_map = torch.stack([d @ rots[f] for f in range(F)])                        # (F,L,3): the single call's products, stacked
    rows, row_w, cols = _device_tables(He, We, dev)
    cell = torch.empty((F, He, We), dtype=torch.int32, device=dev)
    rgb = torch.empty((E, F, L, 3), dtype=torch.float32, device=dev) if out is None else out
    _lib.launch("gcfr_environment_cells_frames", dev, rows, cols, dirs_map, F, He, We, L, float(min_cos), cell, _lib.STREAM)
    _lib.launch("gcfr_environment_fwd_frames", dev, env.detach().contiguous(), E, He, We, row_w, cell, F, L, rgb, _lib.STREAM)
    return rgb


# ------------------------------------------------------------------------------------------------------------------------------
# rig capture: light_rgb fitted to a photograph
# ------------------------------------------------------------------------------------------------------------------------------
MAX_FIT_LIGHTS = 64            # include/gcfr.h: 1 <= L <= 64 for the fit
LIGHT_FIT_CHUNK = 64           # csrc/gcfr_light_fit.hip kFitChunk: pixels per chunk
LIGHT_FIT_MAX_GROUPS = 512     # ... kFitMaxGroups: workgroups per launch at the most


def light_fit_geometry(B: int, H: int, W: int):
    """(chunk, groups) of gcfr_light_fit_normal for B faces of H x W: the face's pixels are cut into chunks of `chunk` consecutive
    pixels and workgroup g of the face's `groups` sums the chunks g, g + groups, ... (include/gcfr.h).  The restatement
    (tests/light_fit_emulation.py) takes the two as parameters; the host test holds them to gcfr_light_fit_workspace_bytes."""
    chunks = (int(H) * int(W) + LIGHT_FIT_CHUNK - 1) // LIGHT_FIT_CHUNK
    return LIGHT_FIT_CHUNK, min(chunks, max(1, LIGHT_FIT_MAX_GROUPS // int(B)))


def _check_fit(final_shading, albedo, image, weight, image_layout, out=None, shared=False, ridge=0.0, max_solves=0):
    """Every shape, dtype, device and range BEFORE anything is launched or loaded: a mismatch never reaches the kernels."""
    tensors = _lib.check_tensors("fit_light_rgb", [("final_shading", final_shading), ("albedo", albedo), ("image", image),
                                                   ("weight", weight), ("out", out)], weight=(torch.float32, torch.uint8))
    if image_layout not in ("nhwc", "nchw"):
        raise _lib.GcfrError("image_layout must be 'nhwc' or 'nchw'; got %r" % (image_layout,))
    B, L, H, W = _many_lights(final_shading, MAX_FIT_LIGHTS)
    of = " for final_shading %s" % (tuple(final_shading.shape),)
    if B > 65535 or H * W >= 2 ** 31 - LIGHT_FIT_CHUNK:
        raise _lib.GcfrError("final_shading (B,L,H,W) = %s: B <= 65535 and H W < 2^31 - %d" % (tuple(final_shading.shape), LIGHT_FIT_CHUNK))
    _lib.check_shape("albedo", albedo, (B, 3, H, W), why=of)
    _lib.check_shape("image", image, (B, H, W, 3) if image_layout == "nhwc" else (B, 3, H, W), why=" (image_layout=%r)" % image_layout + of)
    if weight is not None:
        _lib.check_shape("weight", weight, (B, H, W), (1, H, W), (H, W))
    if not (isinstance(ridge, (int, float)) and math.isfinite(ridge) and ridge >= 0.0):
        raise _lib.GcfrError("ridge must be a finite number >= 0; got %r" % (ridge,))
    if isinstance(max_solves, bool) or not isinstance(max_solves, int) or not 0 <= max_solves < 2 ** 31:
        raise _lib.GcfrError("max_solves must be an int >= 0 (0: the default cap, 3 L); got %r" % (max_solves,))
    _lib.check_out(out, (1 if shared else B, L, 3))
    _lib.require_device(*tensors)


def _fit_weight(weight):
    """the weight as the kernel reads it: f32, contiguous, (1|B,H,W); a u8 mask is divided by 255 in f32"""
    if weight is None:
        return None
    w = weight.detach()
    if w.dtype == torch.uint8:       # an IEEE f32 division: by a device tensor (torch turns a division by a Python scalar into a product)
        w = w.to(torch.float32) / torch.full((1,), 255.0, dtype=torch.float32, device=w.device)
    return (w[None] if w.dim() == 2 else w).contiguous()


def _normal_equations(final_shading, albedo, image, weight, image_layout):
    """light_normal_equations behind its checks"""
    B, L, H, W = final_shading.shape
    dev = final_shading.device
    gram = torch.empty((B, 3, L, L), dtype=torch.float64, device=dev)
    rhs = torch.empty((B, 3, L), dtype=torch.float64, device=dev)
    final, alb, img, w = final_shading.detach().contiguous(), albedo.detach().contiguous(), image.detach().contiguous(), _fit_weight(weight)
    ws = torch.empty(max(8, int(_lib.load().gcfr_light_fit_workspace_bytes(B, L, H, W))) // 8, dtype=torch.float64, device=dev)
    _lib.launch("gcfr_light_fit_normal", dev, final, alb, img, 1 if image_layout == "nhwc" else 0, w, 1 if w is None else w.shape[0],
                B, L, H, W, ws, gram, rhs, _lib.STREAM)
    return gram, rhs


def light_normal_equations(final_shading: torch.Tensor, albedo: torch.Tensor, image: torch.Tensor, weight=None,
                           image_layout: str = "nhwc"):
    """(gram (B,3,L,L) f64, rhs (B,3,L) f64): the normal equations of `fit_light_rgb`, per face b and channel c
    gram[b,c,l,l'] = sum_p w a_c^2 f_l f_l', rhs[b,c,l] = sum_p w a_c I_c f_l, over the pixels p of `final_shading` (B,L,H,W),
    `albedo` (B,3,H,W), the photograph `image` ((B,H,W,3) for image_layout "nhwc", (B,3,H,W) for "nchw") and `weight`
    ((B,H,W), or (1,H,W) / (H,W) shared; f32, or u8 divided by 255 in f32; None: ones).  f64 sums in a fixed order
    (include/gcfr.h): equal inputs give equal bits; gram is exactly symmetric.  Nothing is clamped; a non-finite value reaches the
    entries it enters, also under a weight of 0.  1 <= L <= 64.  Not differentiable (inputs are detached); no host
    synchronisation; a malformed input raises GcfrError before any launch.  There is no CPU path."""
    _check_fit(final_shading, albedo, image, weight, image_layout)
    return _normal_equations(final_shading, albedo, image, weight, image_layout)


def fit_light_rgb(final_shading: torch.Tensor, albedo: torch.Tensor, image: torch.Tensor, weight=None, ridge: float = 1e-3,
                  shared: bool = False, image_layout: str = "nhwc", out=None, return_info: bool = False, nonnegative: bool = False,
                  max_solves: int = 0):
    """The rig `light_rgb` (B,L,3) -- (1,L,3) with `shared=True`, one rig fitted to all faces -- under which `combine_lights`
    followed by the mask paste comes closest to the photograph `image`: per face and channel the weighted least-squares problem
        minimise  sum_p w (image_c - albedo_c sum_l x[l,c] final_shading[l])^2  +  ridge (trace(G_c) / L) |x[:,c]|^2
    with G_c the Gram matrix of `light_normal_equations` (arguments as there).  The ridge is relative to the problem's own scale;
    `ridge=0` is plain least squares.  Two launches form the normal equations, one solves them by Cholesky factorisation in f64
    and rounds once to f32; every operation's order is fixed (include/gcfr.h): equal inputs give equal bits.
    The default `ridge` is a convenience, not a gate: lights close to each other have nearly parallel shadings and make G
    ill-conditioned, the fit then trades large weights of opposite sign against each other, and the result MAY CONTAIN NEGATIVE
    ENTRIES.  The rig stage allows them, but such a rig reproduces its photograph only through cancellation, which does not survive
    another face or a turned environment.
    `nonnegative=True` solves the SAME system under light_rgb >= 0 (Lawson and Hanson's active-set method on the normal equations,
    one launch in place of the Cholesky solve; order in include/gcfr.h): every entry is >= 0 (an excluded light is exactly +0), and
    wherever the unconstrained solution is positive in every entry the two return the same bits.  It factorises once per step, at
    the most `max_solves` times per rig and channel (0: the default cap, 3 L); `return_info=True` then returns
    (light_rgb, info, solves), both (B|1,3) i32 on the device: info 0, or -1 where the cap was reached (the result is the current
    iterate, still >= 0), or k + 1 where the pivot of light k was not a positive finite number (NaN entries); solves the number of
    factorisations.  `max_solves` is not read without `nonnegative`, but is checked.
    `out`: a contiguous f32 buffer of the result's shape that the result is written into and which is returned --
    `RelightSession.light_rgb` between two replays, for example: a captured session is re-lit from a photograph without recapture.
    `return_info=True` returns (light_rgb, info): info (B|1,3) i32 ON THE DEVICE, 0 where the channel was solved, k + 1 where pivot k
    of the factorisation was not a positive finite number (a singular system: that channel's L entries are NaN).  The function
    never synchronises with the host, so it cannot raise on a failed solve: look at `info`, or at the NaNs.
    NOT DIFFERENTIABLE: the inputs are detached and the result carries no graph.  A malformed input (rank, shape, dtype, device,
    L outside 1 .. 64, layout, `out`) raises GcfrError before anything is loaded or launched; host tensors raise too."""
    _check_fit(final_shading, albedo, image, weight, image_layout, out, shared, ridge, max_solves)
    B, L, _, _ = final_shading.shape
    dev = final_shading.device
    gram, rhs = _normal_equations(final_shading, albedo, image, weight, image_layout)
    rigs = 1 if shared else B
    rgb = torch.empty((rigs, L, 3), dtype=torch.float32, device=dev) if out is None else out
    info = torch.empty((rigs, 3), dtype=torch.int32, device=dev)
    if nonnegative:
        solves = torch.empty((rigs, 3), dtype=torch.int32, device=dev)
        _lib.launch("gcfr_light_fit_solve_nonneg", dev, gram, rhs, B, L, float(ridge), rigs, max_solves, rgb, info, solves, _lib.STREAM)
        return (rgb, info, solves) if return_info else rgb
    _lib.launch("gcfr_light_fit_solve", dev, gram, rhs, B, L, float(ridge), rigs, rgb, info, _lib.STREAM)
    return (rgb, info) if return_info else rgb
