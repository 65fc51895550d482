"""CPU: the environment stage's host side (geomconsistentfr_amd/lighting.py) and its numpy restatement
(tests/environment_emulation.py), which tests/test_gpu_environment.py holds the kernels to bit for bit.

1. environment_tables / sphere_directions: the properties they promise.
2. The restatement's cell map against an f64 brute-force search over the SAME f32 tables and directions.  A score is five f32
   operations on values of magnitude <= 1 behind two rounded products for omega: its error is below 2e-7, so the f32 and the
   f64 winner can differ only where the f64 margin between the best and the second best score is below 4e-7.  Texels under
   that margin are excluded (at most 1 % of a map); on every other texel the two must agree.
3. The restatement's sums against the plain f64 sum, within its own bound (2^-23 sum |env w|: one f32 rounding of an f64 sum),
   and its backward against f64 torch autograd of the index_add formulation.
4. The C entries and the Python entries refuse malformed input before a launch, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import environment_emulation as emu

CASES = [(64, 128, 64), (64, 128, 256), (16, 32, 256), (8, 16, 4096), (5, 7, 4)]      # (He, We, L)


def _tables(He, We):
    from geomconsistentfr_amd.lighting import environment_tables
    return environment_tables(He, We)


def _directions(L, min_z=-1.0):
    from geomconsistentfr_amd.lighting import sphere_directions
    return sphere_directions(L, min_z)


@pytest.mark.parametrize("He,We", [(1, 1), (2, 4), (5, 7), (64, 128), (512, 1024)])
def test_table_weights_sum_to_one_and_the_frame_is_the_documented_one(He, We):
    rows, row_w, cols = _tables(He, We)
    assert rows.shape == (He, 2) and cols.shape == (We, 2) and row_w.shape == (He,)
    assert rows.dtype == cols.dtype == np.float32 and row_w.dtype == np.float64
    total = float(row_w.sum() * We)
    print("%d x %d: sum of the texel weights - 1 = %.3e" % (He, We, total - 1.0))
    assert abs(total - 1.0) <= 1e-14 and (row_w > 0).all()
    theta = np.pi * (np.arange(He) + 0.5) / He
    phi = 2 * np.pi * (np.arange(We) + 0.5) / We - np.pi
    np.testing.assert_array_equal(rows, np.stack([np.sin(theta), np.cos(theta)], 1).astype(np.float32))
    np.testing.assert_array_equal(cols, np.stack([np.sin(phi), np.cos(phi)], 1).astype(np.float32))
    o = emu.omega(rows, cols).astype(np.float64)
    assert np.abs(np.linalg.norm(o, axis=-1) - 1.0).max() <= 4e-7
    if He >= 2 and We >= 4:
        assert o[0, :, 1].min() > 0 > o[-1, :, 1].max()                          # row 0 is +y, the last row -y
        assert o[He // 2, We // 2, 2] > 0 and o[He // 2, 0, 2] < 0                # the centre column faces +z, the edge -z
        assert o[He // 2, We - 1 - We // 4, 0] > 0 > o[He // 2, We // 4, 0]      # right of the centre is +x


@pytest.mark.parametrize("n", [1, 2, 7, 64, 4096])
@pytest.mark.parametrize("min_z", [0.2, -1.0, 0.0, 0.9])
def test_sphere_directions(n, min_z):
    d = _directions(n, min_z)
    assert d.shape == (n, 3) and d.dtype == np.float32
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert (d[:, 2] >= min_z).all()
    assert np.array_equal(d, _directions(n, min_z))
    assert len({tuple(v) for v in d.tolist()}) == n
    if n >= 64:                                                                  # equal areas: z is uniform on [min_z, 1]
        assert abs(float(d[:, 2].astype(np.float64).mean()) - (1.0 + min_z) / 2.0) <= 1e-6
    from geomconsistentfr_amd.lighting import sphere_directions
    assert sphere_directions(4).shape == (4, 3) and (sphere_directions(4)[:, 2] >= 0.2).all()      # the default cap
    for bad in [(0, 0.2), (4097, 0.2), (4, 1.0), (4, -1.5)]:
        with pytest.raises(ValueError):
            sphere_directions(*bad)


@pytest.mark.parametrize("He,We,L", CASES)
def test_restated_cells_equal_an_f64_brute_force_search(He, We, L):
    rows, _w, cols = _tables(He, We)
    dirs = _directions(L)
    cell = emu.cells(rows, cols, dirs, -2.0)
    o = emu.omega(rows, cols).astype(np.float64).reshape(-1, 3)                   # (the f32 omega, exactly, as f64)
    s = o @ dirs.astype(np.float64).T                                            # (T,L)
    order = np.argsort(-s, axis=1, kind="stable")
    best = order[:, 0]
    if L > 1:
        margin = s[np.arange(len(s)), best] - s[np.arange(len(s)), order[:, 1]]
    else:
        margin = np.full(len(s), np.inf)
    keep = margin > 4e-7
    differ = int((cell.reshape(-1) != best).sum())
    print("%d x %d, %d lights: %d texels excluded, smallest margin %.2e, f32 / f64 winners differ on %d texels"
          % (He, We, L, int((~keep).sum()), float(margin.min()), differ))
    assert (~keep).sum() <= 0.01 * len(s)
    assert np.array_equal(cell.reshape(-1)[keep], best[keep].astype(np.int32))
    assert cell.min() >= 0 and cell.dtype == np.int32


def test_restated_cells_ties_nan_directions_and_min_cos():
    rows, _w, cols = _tables(6, 9)
    dirs = _directions(5)
    dup = np.concatenate([dirs, dirs[1:3]])                                      # lights 5, 6 repeat 1, 2
    np.testing.assert_array_equal(emu.cells(rows, cols, dup, -2.0), emu.cells(rows, cols, dirs, -2.0))
    bad = dirs.copy()
    bad[2] = np.nan
    cell = emu.cells(rows, cols, bad, -2.0)
    assert (cell != 2).all() and (cell >= 0).all()
    assert (emu.cells(rows, cols, np.full((3, 3), np.nan, np.float32), -2.0) == -1).all()
    assert (emu.cells(rows, cols, dirs, 2.0) == -1).all()
    front = emu.cells(rows, cols, _directions(5, 0.2), 0.5)                      # a cap: texels far from every light drop out
    assert (front == -1).any() and (front >= 0).any()


@pytest.mark.parametrize("He,We,L", CASES)
@pytest.mark.parametrize("E", [1, 2])
def test_restated_sums_equal_the_plain_f64_sum_within_the_bound(He, We, L, E):
    rows, row_w, cols = _tables(He, We)
    cell = emu.cells(rows, cols, _directions(L), -2.0)
    rng = np.random.default_rng(He + L + E)
    env = rng.standard_normal((E, He, We, 3)).astype(np.float32) * np.float32(3.0)   # signed: cancellation inside a cell
    out = emu.forward(env, row_w, cell, L)
    prod = env.astype(np.float64) * row_w[None, :, None, None]
    plain = np.zeros((E, L, 3))
    np.add.at(plain, (slice(None), cell.reshape(-1)), prod.reshape(E, -1, 3))
    err = np.abs(out["rgb_f64"] - plain)
    # the two f64 sums differ in order only: far inside one f32 rounding of the sum
    assert (err <= 1e-3 * out["bound"] + 1e-300).all()
    assert (np.abs(out["rgb"].astype(np.float64) - out["rgb_f64"]) <= out["bound"]).all()
    # all lights together: the whole map's weighted sum
    whole = prod.reshape(E, -1, 3).sum(axis=1)
    assert (np.abs(out["rgb"].astype(np.float64).sum(axis=1) - whole) <= out["bound"].sum(axis=1) + 1e-300).all()
    empty = np.setdiff1d(np.arange(L), cell.reshape(-1))
    assert (out["rgb"][:, empty] == 0).all() and not np.signbit(out["rgb"][:, empty]).any()
    # a constant map of radiance 1: the weights sum to 1
    ones = emu.forward(np.ones((1, He, We, 3), np.float32), row_w, cell, L)
    assert np.abs(ones["rgb_f64"].sum(axis=1) - 1.0).max() <= 1e-13
    assert (np.abs(ones["rgb"].astype(np.float64).sum(axis=1) - 1.0) <= ones["bound"].sum(axis=1)).all()


@pytest.mark.parametrize("He,We,L", [(16, 32, 256), (8, 16, 4096), (5, 7, 4)])
def test_restated_backward_equals_f64_autograd_of_index_add(He, We, L):
    rows, row_w, cols = _tables(He, We)
    cell = emu.cells(rows, cols, _directions(L, 0.2), 0.3)                       # some texels without a cell
    assert (cell == -1).any()
    E = 2
    rng = np.random.default_rng(L)
    g_rgb = rng.standard_normal((E, L, 3)).astype(np.float32)
    w32 = row_w.astype(np.float32).astype(np.float64)                            # the backward's weight is the f32 rounding of row_w
    env = torch.zeros(E, He * We, 3, dtype=torch.float64, requires_grad=True)
    has = torch.from_numpy(cell.reshape(-1) >= 0)
    idx = torch.from_numpy(cell.reshape(-1).astype(np.int64))[has]
    w = torch.from_numpy(np.repeat(w32, We))
    rgb = torch.zeros(E, L, 3, dtype=torch.float64).index_add(1, idx, (env * w[None, :, None])[:, has])
    (rgb * torch.from_numpy(g_rgb.astype(np.float64))).sum().backward()
    got = emu.backward(g_rgb, row_w, cell)
    assert got.dtype == np.float32 and got.shape == (E, He, We, 3)
    want = env.grad.numpy().reshape(E, He, We, 3)
    # autograd's value is the product of two f32 numbers, exact in f64; the restatement's is that product as ONE f32 operation,
    # i.e. the exact value rounded to the output's format: compared after that rounding, to 1e-12
    diff = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    print("%d x %d, %d lights: largest |restatement - f32(f64 autograd)| = %.3e" % (He, We, L, float(diff.max())))
    assert (diff <= 1e-12).all() and np.abs(want).max() > 1e-3
    assert (got[:, cell == -1] == 0).all() and not np.signbit(got[:, cell == -1]).any()


def test_library_refuses_bad_environment_arguments_before_a_launch():
    """the three C entries validate on the host (no GPU needed): NULLs, sizes out of range, a misaligned f64 table"""
    from geomconsistentfr_amd import _lib
    L_ = _lib.load()
    p = ctypes.c_void_p(4096)
    assert L_.gcfr_environment_cells(p, p, p, 0, 4, 3, -2.0, p, None) == -1
    for k in range(4):
        ptrs = [p, p, p, p]
        ptrs[k] = None
        assert L_.gcfr_environment_cells(ptrs[0], ptrs[1], ptrs[2], 4, 8, 3, -2.0, ptrs[3], None) == -1, k
        assert L_.gcfr_environment_fwd(ptrs[0], 1, 4, 8, ptrs[1], ptrs[2], 3, ptrs[3], None) == -1, k
        assert L_.gcfr_environment_bwd(ptrs[0], ptrs[1], ptrs[2], 1, 4, 8, 3, ptrs[3], None) == -1, k
    for E, He, We, L in [(0, 4, 8, 3), (65536, 4, 8, 3), (1, 0, 8, 3), (1, 4, 0, 3), (1, 4, 8, 0), (1, 4, 8, 4097),
                         (1, 4097, 4096, 3), (1, 65536, 65536, 3), (-1, 4, 8, 3), (1, -4, -8, 3)]:
        if E == 1:
            assert L_.gcfr_environment_cells(p, p, p, He, We, L, -2.0, p, None) == -1, (He, We, L)
        assert L_.gcfr_environment_fwd(p, E, He, We, p, p, L, p, None) == -1, (E, He, We, L)
        assert L_.gcfr_environment_bwd(p, p, p, E, He, We, L, p, None) == -1, (E, He, We, L)
    odd = ctypes.c_void_p(4100)                                                   # row_w is f64: 8-byte aligned
    assert L_.gcfr_environment_fwd(p, 1, 4, 8, odd, p, 3, p, None) == -1
    assert L_.gcfr_environment_bwd(p, odd, p, 1, 4, 8, 3, p, None) == -1


def test_python_entries_refuse_malformed_inputs_before_any_launch(monkeypatch):
    from geomconsistentfr_amd import _lib, environment_lights, lighting, render_environment_from_depth

    def reached(*a, **k):
        raise AssertionError("a malformed input reached the launch")
    monkeypatch.setattr(_lib, "launch", reached)
    monkeypatch.setattr(_lib, "load", reached)
    E, He, We, L = 2, 4, 8, 5
    z = lambda *s, **k: torch.zeros(*s, dtype=k.get("dtype", torch.float32), device=k.get("device", "cpu"))
    env, dirs = z(E, He, We, 3), z(L, 3)
    bad = {
        "env without the map axis": dict(env=z(He, We, 3), directions=dirs),
        "env with four channels": dict(env=z(E, He, We, 4), directions=dirs),
        "env planar": dict(env=z(E, 3, He, We), directions=dirs),
        "no rows": dict(env=z(E, 0, We, 3), directions=dirs),
        "too many texels": dict(env=z(1, 4097, 4096, 3, device="meta"), directions=z(L, 3, device="meta")),
        "f64 env": dict(env=z(E, He, We, 3, dtype=torch.float64), directions=dirs),
        "f16 directions": dict(env=env, directions=z(L, 3, dtype=torch.float16)),
        "directions with a batch axis": dict(env=env, directions=z(1, L, 3)),
        "directions with four components": dict(env=env, directions=z(L, 4)),
        "no lights": dict(env=env, directions=z(0, 3)),
        "too many lights": dict(env=env, directions=z(4097, 3)),
        "mixed devices": dict(env=env, directions=z(L, 3, device="meta")),
        "rotation not 3 x 3": dict(env=env, directions=dirs, rotation=z(3, 4)),
        "f64 rotation": dict(env=env, directions=dirs, rotation=z(3, 3, dtype=torch.float64)),
        "out of another shape": dict(env=env, directions=dirs, out=z(E, L + 1, 3)),
        "out without the map axis": dict(env=env, directions=dirs, out=z(L, 3)),
        "f64 out": dict(env=env, directions=dirs, out=z(E, L, 3, dtype=torch.float64)),
        "out that is not contiguous": dict(env=env, directions=dirs, out=z(E, L, 6)[:, :, ::2]),
        "out on another device": dict(env=env, directions=dirs, out=z(E, L, 3, device="meta")),
        "out that requires a gradient": dict(env=env, directions=dirs, out=z(E, L, 3).requires_grad_()),
        "not a tensor": dict(env=np.zeros((E, He, We, 3), np.float32), directions=dirs),
    }
    for why, kw in bad.items():
        with pytest.raises(_lib.GcfrError):
            environment_lights(**kw)
            pytest.fail(why)
    # well-formed but on the host: refused as well (there is no CPU path), still before the launch
    with pytest.raises(_lib.GcfrError, match="no CPU path"):
        environment_lights(env, dirs)
    with pytest.raises(_lib.GcfrError, match="no CPU path"):
        environment_lights(env, dirs, rotation=torch.eye(3), out=z(E, L, 3))
    B = 3
    with pytest.raises(_lib.GcfrError, match="for 3 faces"):                       # E neither 1 nor B: a shape error, found first
        render_environment_from_depth(z(B, 1, 8, 8), z(B, 3, 8, 8), dirs, z(B, L), env, None, 500.0, z(B, 8, 8))
    with pytest.raises(_lib.GcfrError, match="no CPU path"):
        render_environment_from_depth(z(E, 1, 8, 8), z(E, 3, 8, 8), dirs, z(E, L), env, None, 500.0, z(E, 8, 8))


def test_inference_signatures():
    import inspect
    from geomconsistentfr_amd import inference as inf
    for name in ("relight_environment", "relight_environment_device"):
        sig = inspect.signature(getattr(inf, name))
        assert list(sig.parameters)[:6] == ["model", "images", "mask_u8", "env", "n_lights", "rotation"]
        assert sig.parameters["n_lights"].default == 64 and sig.parameters["rotation"].default is None
    assert list(inspect.signature(inf.relight_environment_frames).parameters)[:5] == ["model", "images", "mask_u8", "env", "rotations"]


def test_inference_entries_reject_a_malformed_map_before_the_network_pass():
    """a map whose E is neither 1 nor the number of faces, and rotations that are not (F,3,3): GcfrError before the model is
    called at all (the model here would raise AttributeError if it were)"""
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import inference as inf
    B, He, We = 3, 4, 8
    images, mask = np.zeros((B, 8, 8, 3), np.float32), np.zeros((8, 8), np.uint8)
    bad_env, env = np.zeros((2, He, We, 3), np.float32), np.zeros((He, We, 3), np.float32)
    rots = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    with pytest.raises(_lib.GcfrError, match="for 3 faces"):
        inf.relight_environment_device(None, images, mask, bad_env, n_lights=4, device="cpu")
    with pytest.raises(_lib.GcfrError, match="for 3 faces"):
        inf.relight_environment_frames(None, images, mask, bad_env, rots, n_lights=4, device="cpu")
    with pytest.raises(_lib.GcfrError, match="rotation must be"):
        inf.relight_environment_device(None, images, mask, env, n_lights=4, rotation=np.eye(4, dtype=np.float32), device="cpu")
    with pytest.raises(_lib.GcfrError, match="rotations must be"):
        inf.relight_environment_frames(None, images, mask, env, np.eye(3, dtype=np.float32), n_lights=4, device="cpu")
