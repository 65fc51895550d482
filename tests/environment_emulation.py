"""The environment kernels' operation order (csrc/gcfr_environment.hip, include/gcfr.h), restated in numpy (helper module, no
tests): the cell scores in f32, operation by operation; the integration's products and sums in f64 in the kernel's own order
(256 lanes, lane i taking texels i, i + 256, ... ascending from +0; each wave's xor-shuffle tree, offsets 32 .. 1; the four waves as
(w0 + w1) + (w2 + w3)); the backward product in f32.  tests/test_gpu_environment.py holds the kernels to it bit for bit and
tests/test_environment_host.py holds it to an f64 brute-force search and to f64 torch autograd, so that it is a checked statement
and not a second opinion.

Arrays in the C ABI's layouts: env (E,He,We,3) f32, rows (He,2) f32, row_w (He,) f64, cols (We,2) f32, dirs_map (L,3) f32,
cell (He,We) i32, rgb and g_rgb (E,L,3) f32."""
import numpy as np

from f32_bits import F32, _f, bit_equal  # noqa: F401  (bit_equal: for the tests)

LANES = 256


def omega(rows, cols):
    """(He,We,3) f32: the texels' directions, (sin_t sin_p, cos_t, sin_t cos_p), each product one f32 operation"""
    _f(rows), _f(cols)
    He, We = rows.shape[0], cols.shape[0]
    ox = _f(rows[:, None, 0] * cols[None, :, 0])
    oy = _f(np.broadcast_to(rows[:, None, 1], (He, We)))
    oz = _f(rows[:, None, 0] * cols[None, :, 1])
    return np.stack([ox, oy, oz], axis=-1)


def cells(rows, cols, dirs_map, min_cos):
    """(He,We) i32: best = -inf, cell = -1; l ascending, s = (ox dx + oy dy) + oz dz in f32; s > best takes the cell (a tie keeps
    the lowest index, a NaN never wins); afterwards a best that is not >= min_cos gives -1"""
    _f(dirs_map)
    o = omega(rows, cols)
    ox, oy, oz = o[..., 0], o[..., 1], o[..., 2]
    best = np.full(ox.shape, -np.inf, F32)
    cell = np.full(ox.shape, -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(dirs_map.shape[0]):
            dx, dy, dz = dirs_map[l]
            s = _f(_f(_f(ox * dx) + _f(oy * dy)) + _f(oz * dz))
            win = s > best
            best = np.where(win, s, best)
            cell = np.where(win, np.int32(l), cell)
        cell = np.where(best >= F32(min_cos), cell, np.int32(-1))
    return cell.astype(np.int32)


def _block_sum(lane_sums):
    """(..., 256) f64 -> (...): BlockSum's order (gcfr_reduce.hpp)"""
    v = lane_sums.reshape(lane_sums.shape[:-1] + (4, 64))
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off]
    w = v[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def forward(env, row_w, cell, L):
    """-> dict: rgb (E,L,3) f32 = the f64 sum in the kernel's order rounded once, rgb_f64 that sum, bound (E,L,3) =
    2^-23 sum |env w| over the cell (one f32 rounding of an f64 sum, the form light_rig_emulation uses for g_rgb)"""
    _f(env)
    assert row_w.dtype == np.float64 and cell.dtype == np.int32
    E, He, We, _ = env.shape
    T = He * We
    w = np.repeat(row_w, We)                                                        # (T,)
    flat = cell.reshape(T)
    n_steps = (T + LANES - 1) // LANES
    pad = n_steps * LANES - T
    rgb64 = np.zeros((E, L, 3), np.float64)
    bound = np.zeros((E, L, 3), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = env.reshape(E, T, 3).astype(np.float64) * w[None, :, None]            # one f64 product per term
        for l in np.unique(flat[(flat >= 0) & (flat < L)]):
            own = flat == l
            mine = np.where(own[None, :, None], prod, 0.0)                          # the texels of other cells are not added at all:
            mine = np.concatenate([mine, np.zeros((E, pad, 3))], axis=1).reshape(E, n_steps, LANES, 3)
            member = np.concatenate([own, np.zeros(pad, bool)]).reshape(n_steps, LANES)
            acc = np.zeros((E, LANES, 3), np.float64)
            for k in range(n_steps):                                                # ... a skipped step leaves the lane's sum as it is
                acc = np.where(member[k][None, :, None], acc + mine[:, k], acc)
            rgb64[:, l] = _block_sum(np.moveaxis(acc, 1, -1))
            bound[:, l] = np.abs(np.where(own[None, :, None], prod, 0.0)).sum(axis=1) * 2.0 ** -23
    return {"rgb": rgb64.astype(F32), "rgb_f64": rgb64, "bound": bound}


def backward(g_rgb, row_w, cell):
    """g_env (E,He,We,3) f32 = (float)row_w[row] * g_rgb[e,cell,c], one f32 product; +0 where the texel has no cell"""
    _f(g_rgb)
    E, L, _ = g_rgb.shape
    He, We = cell.shape
    w32 = row_w.astype(F32)
    has = (cell >= 0) & (cell < L)
    with np.errstate(invalid="ignore", over="ignore"):
        g = _f(w32[None, :, None, None] * g_rgb[:, np.where(has, cell, 0)])         # (E,He,We,3)
    return np.where(has[None, :, :, None], g, F32(0.0)).astype(F32)
