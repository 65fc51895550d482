"""GPU: environment-map lighting (csrc/gcfr_environment.hip; lighting.environment_lights / render_environment_from_depth;
inference.relight_environment / relight_environment_frames) against its numpy restatement (tests/environment_emulation.py,
itself held to an f64 brute-force search and to f64 autograd by tests/test_environment_host.py) and against the rig paths that
are already pinned.

  kernels      cell and g_env: BIT-EQUAL to the restatement.  rgb: within the restatement's bound (2^-23 sum |env w|, one f32
               rounding) of its f64 sum, and bit-equal to it as well, the restatement adding in BlockSum's order.  Two calls
               return the same bits.
  inputs       duplicate directions, min_cos above every score, a NaN texel, a NaN direction, negative radiance, base pointers
               4 bytes past a 16-byte boundary, a side stream, `out=`.
  orientation  a map bright on one side lights the half of a synthetic face whose normals point to that side; a constant white
               map under four mirror-image lights gives each a quarter and reproduces the mean of the per-light composites.
  bytes        relight_environment == relight_rig with the stage's light_rgb; a frame of relight_environment_frames == the single
               call with that rotation; a captured RelightSession(light_rgb=...) whose light_rgb buffer is refilled through `out=`
               between replays == the eager call, byte for byte on fixed head outputs."""
import numpy as np
import pytest
import torch

import environment_emulation as emu
from f32_bits import bit_equal_any_nan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _tables(He, We):
    from geomconsistentfr_amd.lighting import environment_tables
    return environment_tables(He, We)


def _directions(L, min_z=-1.0):
    from geomconsistentfr_amd.lighting import sphere_directions
    return sphere_directions(L, min_z)


def _inputs(seed, E, He, We, L):
    rng = np.random.default_rng(seed)
    env = (3.0 * rng.standard_normal((E, He, We, 3))).astype(np.float32)          # signed radiance: nothing is clamped
    g_rgb = rng.standard_normal((E, L, 3)).astype(np.float32)
    return env, g_rgb


def _dev(a, misalign=False):
    """a device tensor of `a`; misalign: its first element sits 4 bytes past a 16-byte boundary"""
    if not misalign:
        return torch.from_numpy(a).to(DEV)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _gpu_cells(dirs, He, We, min_cos):
    from geomconsistentfr_amd import _lib, lighting
    rows, _w, cols = lighting._device_tables(He, We, DEV)
    cell = torch.full((He, We), -7, dtype=torch.int32, device=DEV)
    _lib.launch("gcfr_environment_cells", DEV, rows, cols, _dev(dirs), He, We, dirs.shape[0], float(min_cos), cell, _lib.STREAM)
    return cell.cpu().numpy()


def _gpu(env, dirs, min_cos, g_rgb):
    """the public entry and its autograd.  The entry does not return its cell map, so `cell` is RECOMPUTED by a launch of its own
    through the launcher the entry uses (the entry's own map is held through the bit-equal `rgb` and `g_env`)"""
    from geomconsistentfr_amd import environment_lights
    E, He, We, _ = env.shape
    te = _dev(env).requires_grad_()
    rgb = environment_lights(te, _dev(dirs), min_cos=min_cos)
    (rgb * _dev(g_rgb)).sum().backward()
    return {"cell": _gpu_cells(dirs, He, We, min_cos), "rgb": rgb.detach().cpu().numpy(), "g_env": te.grad.cpu().numpy()}


def _check(label, got, env, dirs, min_cos, g_rgb):
    E, He, We, _ = env.shape
    L = dirs.shape[0]
    rows, row_w, cols = _tables(He, We)
    cell = emu.cells(rows, cols, dirs, min_cos)
    fw = emu.forward(env, row_w, cell, L)
    g_env = emu.backward(g_rgb, row_w, cell)
    ok = ~np.isnan(fw["rgb_f64"])
    err = np.abs(got["rgb"].astype(np.float64) - fw["rgb_f64"])
    ratio = float((err[ok] / np.maximum(fw["bound"][ok], 1e-300)).max()) if ok.any() else 0.0
    same = lambda a, b: int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())
    print("%s: cells that differ %d, g_env elements that differ %d, rgb entries that differ %d; rgb largest |error| = %.3f of its bound"
          % (label, int((got["cell"] != cell).sum()), same(got["g_env"], g_env), same(got["rgb"], fw["rgb"]), ratio))
    assert got["cell"].dtype == np.int32 and np.array_equal(got["cell"], cell), label
    assert got["rgb"].shape == (E, L, 3) and got["rgb"].dtype == np.float32
    assert np.array_equal(np.isnan(got["rgb"]), ~ok), label
    assert (err[ok] <= fw["bound"][ok]).all(), (label, ratio)
    assert bit_equal_any_nan(got["rgb"], fw["rgb"]), label
    assert got["g_env"].shape == env.shape and bit_equal_any_nan(got["g_env"], g_env), label
    return cell, fw


SHAPES = [  # (E, He, We, L)
    (1, 1, 1, 1), (1, 2, 4, 3), (1, 5, 7, 4),
    (1, 1, 255, 5), (1, 1, 256, 5), (1, 1, 257, 5),                               # around the 256-lane stride
    (1, 16, 32, 256), (3, 16, 32, 256),                                           # one map for all faces; a map per face
    (1, 64, 128, 64),                                                             # the usual size
    (1, 8, 16, 4096),                                                             # the most lights: most cells are empty
]


@pytest.mark.parametrize("E,He,We,L", SHAPES)
def test_kernels_equal_the_restatement(E, He, We, L):
    env, g_rgb = _inputs(5 * L + We, E, He, We, L)
    dirs = _directions(L)
    got = _gpu(env, dirs, -2.0, g_rgb)
    cell, _fw = _check("(%d,%d,%d) %d lights" % (E, He, We, L), got, env, dirs, -2.0, g_rgb)
    empty = np.setdiff1d(np.arange(L), cell.reshape(-1))
    assert (got["rgb"][:, empty] == 0).all() and not np.signbit(got["rgb"][:, empty]).any()      # an empty cell: exactly +0
    if L == 4096:
        assert len(empty) >= L - He * We
    again = _gpu(env, dirs, -2.0, g_rgb)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32 if got[k].dtype == np.float32 else np.int32),
                              again[k].view(np.uint32 if again[k].dtype == np.float32 else np.int32)), k


def test_duplicate_directions_the_lower_index_takes_the_cell():
    E, He, We = 2, 6, 9
    base = _directions(5)
    dirs = np.concatenate([base, base[1:3]])                                      # lights 5, 6 repeat 1, 2
    env, g_rgb = _inputs(1, E, He, We, 7)
    got = _gpu(env, dirs, -2.0, g_rgb)
    cell, _ = _check("duplicates", got, env, dirs, -2.0, g_rgb)
    assert (cell < 5).all() and (cell == 1).any() and (cell == 2).any()
    assert (got["rgb"][:, 5:] == 0).all() and not np.signbit(got["rgb"][:, 5:]).any()
    assert np.abs(got["rgb"][:, 1:3]).min() > 0


def test_min_cos_above_every_score_drops_everything():
    E, He, We, L = 2, 5, 7, 4
    env, g_rgb = _inputs(2, E, He, We, L)
    got = _gpu(env, _directions(L), 2.0, g_rgb)
    _check("min_cos = 2", got, env, _directions(L), 2.0, g_rgb)
    assert (got["cell"] == -1).all()
    for k in ("rgb", "g_env"):
        assert (got[k] == 0).all() and not np.signbit(got[k]).any(), k
    # a cap in between: some texels belong to no light, and their gradient is exactly +0
    front = _directions(L, 0.2)
    got = _gpu(env, front, 0.5, g_rgb)
    cell, _ = _check("min_cos = 0.5", got, env, front, 0.5, g_rgb)
    assert (cell == -1).any() and (cell >= 0).any()
    assert (got["g_env"][:, cell == -1] == 0).all() and np.abs(got["g_env"][:, cell >= 0]).min() > 0


def test_a_nan_texel_poisons_its_own_cell_and_map_only():
    E, He, We, L = 3, 16, 32, 12
    env, g_rgb = _inputs(3, E, He, We, L)
    dirs = _directions(L)
    e, r, c = 1, 9, 20
    env[e, r, c] = np.nan
    got = _gpu(env, dirs, -2.0, g_rgb)
    cell, _ = _check("NaN texel", got, env, dirs, -2.0, g_rgb)
    where = np.zeros((E, L, 3), bool)
    where[e, cell[r, c]] = True
    assert np.array_equal(np.isnan(got["rgb"]), where)
    assert not np.isnan(got["g_env"]).any()                                      # the gather does not read the map


def test_a_nan_direction_never_owns_a_texel():
    E, He, We, L = 1, 16, 32, 12
    env, g_rgb = _inputs(4, E, He, We, L)
    dirs = _directions(L)
    dirs[3] = np.nan
    dirs[7, 1] = np.nan
    got = _gpu(env, dirs, -2.0, g_rgb)
    cell, _ = _check("NaN directions", got, env, dirs, -2.0, g_rgb)
    assert (cell != 3).all() and (cell != 7).all() and (cell >= 0).all()
    assert (got["rgb"][:, [3, 7]] == 0).all() and not np.isnan(got["rgb"]).any()
    nothing = np.full((2, 3), np.nan, np.float32)                                # no finite score at all: no cell at all
    assert (_gpu_cells(nothing, He, We, -2.0) == -1).all()


def test_negative_radiance_is_not_clamped():
    E, He, We, L = 1, 16, 32, 12
    env, g_rgb = _inputs(6, E, He, We, L)
    env = -np.abs(env) - np.float32(0.5)
    got = _gpu(env, _directions(L), -2.0, g_rgb)
    _check("negative radiance", got, env, _directions(L), -2.0, g_rgb)
    assert (got["rgb"] < 0).all()


@pytest.mark.parametrize("E,He,We,L", [(2, 5, 7, 4), (1, 16, 32, 12)])
def test_misaligned_base_pointers(E, He, We, L):
    """every f32 and i32 tensor 4 bytes past a 16-byte boundary (the f64 table stays 8-byte aligned, as the entries require)"""
    from geomconsistentfr_amd import _lib
    env, g_rgb = _inputs(7, E, He, We, L)
    dirs = _directions(L)
    rows, row_w, cols = _tables(He, We)
    cell = _dev(np.full((He, We), -7, np.int32), True)
    rgb = _dev(np.full((E, L, 3), np.nan, np.float32), True)
    g_env = _dev(np.full((E, He, We, 3), np.nan, np.float32), True)
    w_d = _dev(row_w)
    _lib.launch("gcfr_environment_cells", DEV, _dev(rows, True), _dev(cols, True), _dev(dirs, True), He, We, L, -2.0, cell, _lib.STREAM)
    _lib.launch("gcfr_environment_fwd", DEV, _dev(env, True), E, He, We, w_d, cell, L, rgb, _lib.STREAM)
    _lib.launch("gcfr_environment_bwd", DEV, _dev(g_rgb, True), w_d, cell, E, He, We, L, g_env, _lib.STREAM)
    got = {"cell": cell.cpu().numpy(), "rgb": rgb.cpu().numpy(), "g_env": g_env.cpu().numpy()}
    _check("misaligned (%d,%d,%d)" % (E, He, We), got, env, dirs, -2.0, g_rgb)


def test_a_side_stream():
    from geomconsistentfr_amd import environment_lights
    E, He, We, L = 2, 16, 32, 12
    env, g_rgb = _inputs(8, E, He, We, L)
    dirs = _directions(L)
    te, td, tg = _dev(env).requires_grad_(), _dev(dirs), _dev(g_rgb)
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        rgb = environment_lights(te, td)
        (rgb * tg).sum().backward()
    side.synchronize()
    got = {"cell": _gpu_cells(dirs, He, We, -2.0), "rgb": rgb.detach().cpu().numpy(), "g_env": te.grad.cpu().numpy()}
    _check("side stream", got, env, dirs, -2.0, g_rgb)


def _rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float32)


def test_out_writes_in_place_and_a_rotation_is_the_callers_matmul():
    from geomconsistentfr_amd import environment_lights
    E, He, We, L = 1, 16, 32, 12
    env, _g = _inputs(9, E, He, We, L)
    dirs = _directions(L)
    te, td = _dev(env), _dev(dirs)
    R = _rotation_y(0.7)
    buf = torch.full((E, L, 3), float("nan"), device=DEV)
    ptr = buf.data_ptr()
    ret = environment_lights(te, td, rotation=torch.from_numpy(R).to(DEV), out=buf)
    assert ret.data_ptr() == ptr and buf.data_ptr() == ptr and tuple(ret.shape) == (E, L, 3)
    fresh = environment_lights(te, td, rotation=torch.from_numpy(R))             # a host rotation: uploaded, the same product
    assert fresh.data_ptr() != ptr and torch.equal(fresh, buf) and not torch.isnan(buf).any()
    # the stage on `directions @ rotation`, the product taken by torch on the device
    rotated = (td @ torch.from_numpy(R).to(DEV)).cpu().numpy()
    rows, row_w, cols = _tables(He, We)
    want = emu.forward(env, row_w, emu.cells(rows, cols, rotated, -2.0), L)["rgb"]
    assert bit_equal_any_nan(buf.cpu().numpy(), want)
    assert not torch.equal(environment_lights(te, td), buf)                      # ... and the rotation matters
    # the sense of the rotation: what the map shows in direction m lights the face from R m
    spot = np.zeros((1, He, We, 3), np.float32)
    spot[0, 5, 22] = 1.0
    m = emu.omega(rows, cols)[5, 22].astype(np.float64)
    many = _directions(256)
    rgb = environment_lights(_dev(spot), _dev(many), rotation=torch.from_numpy(R)).cpu().numpy()
    lit = int(np.argmax(rgb[0, :, 0]))
    assert (rgb[0, :, 0] > 0).sum() == 1
    assert many[lit].astype(np.float64) @ (R.astype(np.float64) @ m) > 0.98      # 256 lights: a cell is ~7 degrees across


# ------------------------------------------------------------------------------------------------------------------------------
# the block + the stage: orientation and normalisation
# ------------------------------------------------------------------------------------------------------------------------------
S = 48


def _scene(B, L):
    import scenes
    depth, mask, albedo, _n, _l, amb = scenes.synth_faces_sized(B, 21, S, L)
    return torch.from_numpy(depth[:, None]).to(DEV), torch.from_numpy(mask).to(DEV), torch.from_numpy(albedo).to(DEV), \
        torch.from_numpy(amb).to(DEV)


def _camera():
    from geomconsistentfr_amd.inference import camera_matrix
    return camera_matrix(700.0, S, S)


def _params():
    from geomconsistentfr_amd import RenderParams
    return RenderParams(n_samples=40, dt=0.02)


def test_a_half_bright_map_lights_the_half_of_the_face_that_looks_at_it_and_env_receives_its_gradient():
    from geomconsistentfr_amd import render_environment_from_depth
    B, L, He, We = 1, 32, 16, 32
    depth, mask, albedo, amb = _scene(B, L)
    dirs = _directions(L, 0.2)
    rows, row_w, cols = _tables(He, We)
    o = emu.omega(rows, cols)
    for axis, name in ((1, "y"), (0, "x")):
        means = {}
        for sign in (1.0, -1.0):
            env = np.repeat(((sign * o[..., axis]) > 0).astype(np.float32)[None, :, :, None], 3, axis=3)
            te = _dev(env).requires_grad_()
            r = render_environment_from_depth(depth, albedo, _dev(dirs), amb, te, _camera(), 500.0, mask, _params())
            assert tuple(r["rig_shading"].shape) == (B, 3, S, S) and tuple(r["light_rgb"].shape) == (1, L, 3)
            n = r["surface_normals"][0, axis]
            inside = mask[0] > 0
            sh = r["rig_shading"][0, 0].detach()
            pos, neg = float(sh[inside & (n > 0.15)].mean()), float(sh[inside & (n < -0.15)].mean())
            print("bright for omega_%s %s 0: mean shading where n_%s > 0.15: %.4f, where n_%s < -0.15: %.4f"
                  % (name, ">" if sign > 0 else "<", name, pos, name, neg))
            means[sign] = (pos, neg)
            # the lights on the bright side carry the weight
            w = r["light_rgb"][0, :, 0].detach().cpu().numpy()
            side = sign * dirs[:, axis]
            assert w[side > 0.2].sum() > 4 * w[side < -0.2].sum()
        assert means[1.0][0] > means[1.0][1] and means[-1.0][1] > means[-1.0][0], (name, means)
    # the frame the docstring states: n_y > 0 is the upper half of the image, n_x > 0 the right half
    rr, cc = torch.meshgrid(torch.arange(S, device=DEV), torch.arange(S, device=DEV), indexing="ij")
    ny, nx = r["surface_normals"][0, 1], r["surface_normals"][0, 0]
    assert float(rr[inside & (ny > 0.15)].float().mean()) < float(rr[inside & (ny < -0.15)].float().mean())
    assert float(cc[inside & (nx > 0.15)].float().mean()) > float(cc[inside & (nx < -0.15)].float().mean())
    # gradients reach env: the stage's backward on the rig stage's g_rgb, bit for bit
    r["light_rgb"].retain_grad()
    r["rig_rendered_images"].sum().backward()
    cell = emu.cells(rows, cols, dirs, -2.0)
    want = emu.backward(r["light_rgb"].grad.cpu().numpy(), row_w, cell)
    assert bit_equal_any_nan(te.grad.cpu().numpy(), want) and np.abs(want).max() > 0


def test_a_constant_white_map_reproduces_the_mean_of_the_per_light_composites():
    """Four lights that are mirror images of each other in x and in y under a map with an even number of rows and columns: the
    texel grid has the same two symmetries and no texel centre lies on a mirror plane, so each light owns a quarter of the
    texels and a quarter of the weight, within its bound (one f32 rounding of 1/4).  The rig image is then the mean of the four
    per-light composites; gate per pixel: sum_l bound_l |composite_l| for the weights plus L 2^-23 sum_l |composite_l / 4| for the
    rig stage's own L products and L - 1 sums in f32 (the gate of tests/test_light_rig_host.py)."""
    from geomconsistentfr_amd import render_environment_from_depth
    B, L, He, We = 2, 4, 16, 32
    depth, mask, albedo, amb = _scene(B, L)
    d = np.array([[0.4, 0.3, 0.0], [-0.4, 0.3, 0.0], [0.4, -0.3, 0.0], [-0.4, -0.3, 0.0]])
    d[:, 2] = np.sqrt(1.0 - 0.25)
    dirs = d.astype(np.float32)
    env = np.ones((1, He, We, 3), np.float32)
    with torch.no_grad():
        r = render_environment_from_depth(depth, albedo, _dev(dirs), amb, _dev(env), _camera(), 500.0, mask, _params())
    rows, row_w, cols = _tables(He, We)
    fw = emu.forward(env, row_w, emu.cells(rows, cols, dirs, -2.0), L)
    rgb = r["light_rgb"].cpu().numpy()
    print("weights - 1/4:", (rgb[0, :, 0].astype(np.float64) - 0.25).tolist(), "bound", fw["bound"][0, :, 0].tolist())
    assert (np.abs(rgb.astype(np.float64) - 0.25) <= fw["bound"]).all()
    assert abs(float(rgb[0, :, 0].astype(np.float64).sum()) - 1.0) <= fw["bound"][0, :, 0].sum()
    per_light = r["rendered_images"].cpu().numpy().astype(np.float64)            # (B,L,3,H,W)
    got = r["rig_rendered_images"].cpu().numpy().astype(np.float64)
    gate = (fw["bound"][0, :, 0][None, :, None, None, None] * np.abs(per_light)).sum(1) + L * 2.0 ** -23 * np.abs(per_light / 4).sum(1)
    err = np.abs(got - per_light.mean(axis=1))
    print("largest |rig image - mean of the per-light composites| / gate = %.3f" % float((err / np.maximum(gate, 1e-300)).max()))
    assert (err <= gate).all() and per_light.std() > 0.01


# ------------------------------------------------------------------------------------------------------------------------------
# bytes
# ------------------------------------------------------------------------------------------------------------------------------
def _serving_case(seed):
    from test_gpu_light_rig import _fixed_net
    B, size = 2, 64
    net, mask_u8 = _fixed_net(B, size)
    rng = np.random.default_rng(seed)
    images = rng.random((B, size, size, 3), dtype=np.float32)
    env = (2.0 * rng.random((8, 16, 3))).astype(np.float32)
    env[:, 8:] *= np.float32(4.0)                                                 # one side of the world is brighter
    rotations = np.stack([_rotation_y(a) for a in (0.0, 2.1, 4.2)])
    return B, size, net, mask_u8, images, env, rotations


def test_relight_environment_bytes():
    from geomconsistentfr_amd import environment_lights
    from geomconsistentfr_amd import inference as inf
    B, size, net, mask_u8, images, env, rotations = _serving_case(12)
    n = 6
    dirs = _directions(n, 0.2)
    for fix in (False, True):
        got = inf.relight_environment_device(net, images, mask_u8, env, n_lights=n, rotation=rotations[1], device=DEV, fix_border=fix)
        assert tuple(got.shape) == (B, size, size, 3) and got.dtype == torch.uint8
        rgb = environment_lights(_dev(env[None]), _dev(dirs), rotation=_dev(rotations[1]))
        want = inf.relight_rig_device(net, images, mask_u8, dirs, rgb, device=DEV, fix_border=fix)
        assert torch.equal(got, want)
    host = inf.relight_environment(net, images, mask_u8, env, n_lights=n, rotation=rotations[1], device=DEV, fix_border=True)
    np.testing.assert_array_equal(host, got.cpu().numpy())
    assert host.std() > 10
    # a map per face: face 1 under a darker world
    both = np.stack([env, np.float32(0.25) * env])
    per_face = inf.relight_environment_device(net, images, mask_u8, both, n_lights=n, rotation=rotations[1], device=DEV)
    shared = inf.relight_environment_device(net, images, mask_u8, env, n_lights=n, rotation=rotations[1], device=DEV)
    assert torch.equal(per_face[0], shared[0]) and not torch.equal(per_face[1], shared[1])


def test_a_frame_of_the_turntable_is_the_single_call_with_that_rotation():
    from geomconsistentfr_amd import inference as inf
    B, size, net, mask_u8, images, env, rotations = _serving_case(13)
    frames = inf.relight_environment_frames(net, images, mask_u8, env, rotations, n_lights=6, device=DEV)
    assert tuple(frames.shape) == (B, 3, size, size, 3) and frames.dtype == torch.uint8
    for f in range(3):
        one = inf.relight_environment_device(net, images, mask_u8, env, n_lights=6, rotation=rotations[f], device=DEV)
        assert torch.equal(frames[:, f], one), f
    assert not torch.equal(frames[:, 0], frames[:, 1])
    fixed = inf.relight_environment_frames(net, images, mask_u8, env, rotations[:1], n_lights=6, device=DEV, fix_border=True)
    assert torch.equal(fixed[:, 0], inf.relight_environment_device(net, images, mask_u8, env, n_lights=6, rotation=rotations[0],
                                                                   device=DEV, fix_border=True))


def test_a_session_whose_light_rgb_is_refilled_between_replays_returns_the_eager_result():
    """B = 2, 64 x 64, six lights, captured once; between two replays only the session's light_rgb buffer changes, through
    `out=`.  The captured pass is a single-stream chain; the machine's default number of hardware queues."""
    from geomconsistentfr_amd import environment_lights
    from geomconsistentfr_amd import inference as inf
    B, size, net, mask_u8, images, env, rotations = _serving_case(14)
    n = 6
    dirs = _directions(n, 0.2)
    env_d, dirs_d = _dev(env[None]), _dev(dirs)
    sess = inf.RelightSession(net, B, mask_u8, dirs, device=DEV, H=size, W=size, light_rgb=torch.zeros(1, n, 3, device=DEV))
    assert sess.graph is not None and tuple(sess.light_rgb.shape) == (1, n, 3)
    ptr = sess.light_rgb.data_ptr()
    seen = []
    for f in (1, 2):
        ret = environment_lights(env_d, dirs_d, rotation=_dev(rotations[f]), out=sess.light_rgb)
        assert ret.data_ptr() == ptr and sess.light_rgb.data_ptr() == ptr
        got = sess.run(torch.from_numpy(images))
        assert tuple(got.shape) == (B, size, size, 3) and got.dtype == torch.uint8
        want = inf.relight_environment_device(net, images, mask_u8, env, n_lights=n, rotation=rotations[f], device=DEV)
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        seen.append(got.cpu().numpy())
    assert np.abs(seen[0].astype(int) - seen[1].astype(int)).max() > 0
