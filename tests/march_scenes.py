"""Scenes shared by tests/test_march_backward_restatement_host.py and tests/test_gpu_march_backward_pixels.py: two small
even sizes, ten lights that between them reach every mechanism of the march's backward (all three end-point kinds, both
choices of the corner cases, clamped end points, wrapped columns and rows), a smooth and a rough depth, a 10 % mask."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import materialised as M  # noqa: E402

SIZES = [(40, 48, 33), (48, 72, 40)]          # H, W, N
LIGHTS = [(0.004, -0.003, 1.0), (0.002, 0.9, 0.3), (-0.003, -0.9, 0.3), (-0.9, 0.001, 0.2), (0.9, -0.002, 0.2),
          (0.3, 0.5, 0.8), (-0.5, 0.4, 0.3), (0.6, -0.7, 0.05), (-0.4, -0.6, 0.5), (-0.95, 0.02, 0.3)]
DEPTHS = {"smooth": 1.0, "rough": 4.0}       # amplitude of the uniform noise on top of the bump


def params(N):
    return M.BlockParams(n_samples=N, t0=0.02, dt=0.8 / N)


def scene(H, W, kind, seed=1):
    """-> depth (H,W) f32, mask (H,W) u8, both numpy."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:H, 0:W]
    bump = 0.3 * H * np.exp(-(((c - 0.45 * W) / (0.2 * W)) ** 2 + ((r - 0.48 * H) / (0.2 * H)) ** 2))
    depth = (bump + DEPTHS[kind] * rng.random((H, W))).astype(np.float32)
    mask = (rng.random((H, W)) > 0.1).astype(np.uint8)
    return depth, mask


def light_points(lights, p):
    """(n,3) raw lights -> (n,3) f32 light points, the oracle's."""
    return M.light_points(torch.tensor(lights, dtype=torch.float32), p)[1]


def light_name(light):
    return "light (%g, %g, %g)" % tuple(light)


def describe_term(name, cls_names, light):
    return "%s pixels of %s, term: %s" % (" / ".join(cls_names) if cls_names else "unclassified", light_name(light), name)
