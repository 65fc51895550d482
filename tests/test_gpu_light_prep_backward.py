"""gcfr_light_prep_bwd against f64 autograd of oracle/materialised.light_points, in the three configurations the ABI documents:
clamp_z = 1 with clamp_min 0 (T8:357-363) and 0.16 (SLT:332), clamp_z = 0 (S1:332-336); lights with z below and above the
clamp (not on it: torch.maximum splits the gradient there); grad_unit and grad_light_pt given separately and together.
Gate: the output is the f64 result rounded to f32 once, 2^-24 relative per component; 4 * 2^-24 of the largest component."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

LIGHTS = np.array([[0.3, 0.5, 0.8], [-0.9, 0.1, 0.2], [0.004, -0.003, 1.0], [0.7, -0.7, 0.05], [0.5, -0.8, -0.3],
                   [-0.2, 0.6, 0.159], [-0.2, 0.6, 0.161], [0.6, 0.2, -1e-3], [0.6, 0.2, 1e-3], [-3.0, 2.0, 0.5],
                   [0.01, 0.02, -0.9]], np.float32)


@pytest.mark.parametrize("which", ["unit", "light_pt", "both"])
@pytest.mark.parametrize("clamp", [0.0, 0.16, None], ids=["T8_clamp_0", "SLT_clamp_0.16", "S1_no_clamp"])
def test_light_prep_backward_matches_f64_autograd(clamp, which):
    import materialised as M
    from geomconsistentfr_amd import _lib
    d = torch.device("cuda:0")
    n = len(LIGHTS)
    assert clamp is None or (np.any(LIGHTS[:, 2] < clamp) and np.any(LIGHTS[:, 2] > clamp) and not np.any(LIGHTS[:, 2] == np.float32(clamp)))
    rng = np.random.default_rng(7)
    g_unit = rng.standard_normal((n, 3)).astype(np.float32)
    g_pt = rng.standard_normal((n, 3)) * 1e-3
    p = M.BlockParams(clamp_light_z_min=clamp)
    leaf = torch.from_numpy(LIGHTS).double().requires_grad_()
    unit, pt = M.light_points(leaf, p)
    loss = 0.0
    if which in ("unit", "both"):
        loss = loss + (unit * torch.from_numpy(g_unit).double()).sum()
    if which in ("light_pt", "both"):
        loss = loss + (pt * torch.from_numpy(g_pt)).sum()
    loss.backward()
    ref = leaf.grad.numpy()

    raw = torch.from_numpy(LIGHTS).to(d)
    gu = torch.from_numpy(g_unit).to(d) if which in ("unit", "both") else None
    gp = torch.from_numpy(g_pt).to(d) if which in ("light_pt", "both") else None
    out = torch.full((n, 3), float("nan"), dtype=torch.float32, device=d)
    _lib.check(_lib.load().gcfr_light_prep_bwd(raw.data_ptr(), n, int(clamp is not None), float(clamp or 0.0), float(p.light_distance),
                                               _lib.ptr(gu), _lib.ptr(gp), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "gcfr_light_prep_bwd")
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print("clamp %s, %s: max |difference| %.3e, largest component %.3e, ratio to the gate %.3f" %
          (clamp, which, err, np.abs(ref).max(), err / (4 * 2.0 ** -24 * np.abs(ref).max())))
    assert err <= 4 * 2.0 ** -24 * np.abs(ref).max(), (err, np.abs(ref).max())
    if clamp is not None:       # below the clamp z carries no gradient at all
        assert np.all(got[LIGHTS[:, 2] < clamp, 2] == 0.0) and np.all(ref[LIGHTS[:, 2] < clamp, 2] == 0.0)
