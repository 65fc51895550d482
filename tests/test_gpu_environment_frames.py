"""GPU: the environment stage with a frame axis (csrc/gcfr_environment.hip gcfr_environment_cells_frames /
gcfr_environment_fwd_frames; lighting.environment_lights_frames) against the single-rotation entry it must equal bit for bit, and
its cell maps against the numpy restatement (tests/environment_emulation.py)."""
import numpy as np
import pytest
import torch

import environment_emulation as emu
from test_gpu_environment import _dev, _directions, _inputs, _rotation_y, _tables

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rotations(F):
    return np.stack([_rotation_y(0.3 + 2.0 * np.pi * f / F) for f in range(F)])


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("E,He,We,L,F", [(1, 5, 7, 4, 1), (2, 5, 7, 4, 3), (1, 16, 32, 12, 5)])
def test_frames_equal_the_stack_of_single_rotations_and_the_cell_maps_the_restatement(E, He, We, L, F):
    from geomconsistentfr_amd import _lib, environment_lights, environment_lights_frames, lighting
    env, _g = _inputs(F + L, E, He, We, L)
    dirs, rots = _directions(L), _rotations(F)
    te, td, tr = _dev(env), _dev(dirs), _dev(rots)
    got = environment_lights_frames(te, td, tr)
    assert tuple(got.shape) == (E, F, L, 3) and got.dtype == torch.float32
    want = torch.stack([environment_lights(te, td, rotation=tr[f]) for f in range(F)], dim=1)
    print("(%d,%d,%d) %d lights %d frames: entries whose bits differ from the single calls' %d"
          % (E, He, We, L, F, int((_bits(got) != _bits(want)).sum())))
    assert np.array_equal(_bits(got), _bits(want))
    host = environment_lights_frames(te, td, torch.from_numpy(rots))            # host rotations: uploaded, the same products
    assert np.array_equal(_bits(host), _bits(got))
    if F > 1:
        assert not torch.equal(got[:, 0], got[:, 1])
    # the cell maps: one launch for all frames, on the direction sets the entry forms (the single call's products, stacked)
    dirs_map = torch.stack([td @ tr[f] for f in range(F)])
    rows_d, _w, cols_d = lighting._device_tables(He, We, DEV)
    cell = torch.full((F, He, We), -7, dtype=torch.int32, device=DEV)
    _lib.launch("gcfr_environment_cells_frames", DEV, rows_d, cols_d, dirs_map, F, He, We, L, -2.0, cell, _lib.STREAM)
    rows, row_w, cols = _tables(He, We)
    for f in range(F):
        c = emu.cells(rows, cols, dirs_map[f].cpu().numpy(), -2.0)
        assert np.array_equal(cell[f].cpu().numpy(), c), f
        assert np.array_equal(_bits(got[:, f]), emu.forward(env, row_w, c, L)["rgb"].view(np.uint32)), f
    # a cap on the angle reaches every frame
    capped = environment_lights_frames(te, td, tr, min_cos=0.9)
    want = torch.stack([environment_lights(te, td, rotation=tr[f], min_cos=0.9) for f in range(F)], dim=1)
    assert np.array_equal(_bits(capped), _bits(want))


def test_a_nan_direction_in_one_frame_affects_that_frame_only():
    """the frame's direction sets are given to the launchers directly: a NaN in frame 1's light 2"""
    from geomconsistentfr_amd import _lib, lighting
    E, He, We, L, F = 2, 16, 32, 12, 3
    env, _g = _inputs(3, E, He, We, L)
    td, tr = _dev(_directions(L)), _dev(_rotations(F))
    dirs_map = torch.stack([td @ tr[f] for f in range(F)])
    rows_d, w_d, cols_d = lighting._device_tables(He, We, DEV)

    def run(d):
        cell = torch.empty((F, He, We), dtype=torch.int32, device=DEV)
        rgb = torch.empty((E, F, L, 3), dtype=torch.float32, device=DEV)
        _lib.launch("gcfr_environment_cells_frames", DEV, rows_d, cols_d, d, F, He, We, L, -2.0, cell, _lib.STREAM)
        _lib.launch("gcfr_environment_fwd_frames", DEV, _dev(env), E, He, We, w_d, cell, F, L, rgb, _lib.STREAM)
        return cell.cpu().numpy(), rgb.cpu().numpy()

    cell0, rgb0 = run(dirs_map)
    poisoned = dirs_map.clone()
    poisoned[1, 2, 1] = float("nan")
    cell1, rgb1 = run(poisoned)
    rows, row_w, cols = _tables(He, We)
    for f in range(F):
        assert np.array_equal(cell1[f], emu.cells(rows, cols, poisoned[f].cpu().numpy(), -2.0)), f
    for f in (0, 2):
        assert np.array_equal(cell1[f], cell0[f]) and np.array_equal(rgb1[:, f].view(np.uint32), rgb0[:, f].view(np.uint32)), f
    assert (cell0[1] == 2).any() and (cell1[1] != 2).all() and (cell1[1] >= 0).all()          # the NaN light owns no texel ...
    assert (rgb1[:, 1, 2] == 0).all() and not np.isnan(rgb1).any()                            # ... and carries no weight
    assert not np.array_equal(rgb1[:, 1], rgb0[:, 1])


def test_out_writes_in_place():
    from geomconsistentfr_amd import environment_lights_frames
    E, He, We, L, F = 2, 5, 7, 4, 3
    env, _g = _inputs(4, E, He, We, L)
    te, td, tr = _dev(env), _dev(_directions(L)), _dev(_rotations(F))
    buf = torch.full((E, F, L, 3), float("nan"), device=DEV)
    ptr = buf.data_ptr()
    ret = environment_lights_frames(te, td, tr, out=buf)
    assert ret.data_ptr() == ptr and buf.data_ptr() == ptr and not torch.isnan(buf).any()
    fresh = environment_lights_frames(te, td, tr)
    assert fresh.data_ptr() != ptr and np.array_equal(_bits(fresh), _bits(buf))
    assert not ret.requires_grad
