"""Scenes shared by tests/test_shade_backward_restatement_host.py and tests/test_gpu_shade_backward_pixels.py: the bump of
tests/march_scenes.py at any size, three lights of which the first is the low one whose terminator crosses the bump, random
albedo / ambient, SYNTHETIC minimum distances with planted special values, and a few planted zero-vector normals.  Everything
is generated from seeds."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import materialised as M  # noqa: E402

# the smallest shapes at which each mechanism exists (even: the fused entries)
FUSED_SHAPES = [(2, 2), (8, 32), (10, 34), (18, 66)]
ODD_SHAPES = [(3, 5), (9, 33)]
CAMERA = (600.0, 900.0)               # focal length, z offset (tests/march_scenes.py's camera)
PRODUCT_CAMERA = (1570.0, 1610.0)
LIGHTS = [(0.6, -0.7, 0.05), (0.3, 0.5, 0.8), (-0.9, 0.001, 0.2)]     # [0]: the low light (terminator)
INTENSITY = 0.5
BEYOND_UNDERFLOW = 200.0              # exp(-200) is 0 in f32


def params():
    return M.BlockParams()


def depth(H, W, seed=1, noise=1.0):
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:H, 0:W]
    bump = 0.3 * H * np.exp(-(((c - 0.45 * W) / (0.2 * W)) ** 2 + ((r - 0.48 * H) / (0.2 * H)) ** 2))
    return (bump + noise * rng.random((H, W))).astype(np.float32)


def light_points(L):
    """(L,3) f32 light points, the oracle's (T8:357-362)."""
    return M.light_points(torch.tensor(LIGHTS[:L], dtype=torch.float32), params())[1]


def planted(H, W):
    """flat pixel indices: (d = 0, d beyond the underflow, d of a pixel without a sample, zero-vector normals) -- none where a
    single pixel is more than the 1 % the exclusions may take."""
    P = H * W
    if P < 256:
        return [], [], [], []
    return [5], [P // 3], [P // 2 + 3], [(7 * P) // 10 + 400 * j for j in range(max(1, P // 400)) if (7 * P) // 10 + 400 * j < P]


def inputs(H, W, L, no_sample_value, seed=7):
    """-> albedo (3,H,W), ambient (L,), minimum distance (L,H,W): f32 torch.  Distances uniform in [0.05, 8] plus the planted
    values (every light)."""
    rng = np.random.default_rng(seed + 1000 * L + H * W)
    albedo = torch.from_numpy(rng.random((3, H, W), dtype=np.float32))
    amb = torch.from_numpy((0.3 + 0.4 * rng.random(L)).astype(np.float32))
    md = torch.from_numpy((0.05 + 7.95 * rng.random((L, H * W))).astype(np.float32))
    zero, under, nosample, _ = planted(H, W)
    md[:, zero], md[:, under], md[:, nosample] = 0.0, BEYOND_UNDERFLOW, float(no_sample_value)
    return albedo, amb, md.reshape(L, H, W)


def plant_zero_normals(normals, H, W):
    """normals (3,H,W) -> a copy with the planted pixels' normal the zero vector."""
    n = normals.clone().reshape(3, H * W)
    n[:, planted(H, W)[3]] = 0.0
    return n.reshape(3, H, W)


def cotangents(H, W, L, seed=13):
    """dense g_w, g_full, g_final (L,H,W), g_rendered (L,3,H,W), g_normals_out (3,H,W): f32, none of them zero anywhere."""
    rng = np.random.default_rng(seed + 1000 * L + H * W)
    g = lambda *s: torch.from_numpy((rng.standard_normal(s) + np.sign(rng.standard_normal(s)) * 0.1).astype(np.float32))
    return dict(g_w=g(L, H, W), g_full=g(L, H, W), g_final=g(L, H, W), g_rendered=g(L, 3, H, W), g_normals_out=g(3, H, W))
