"""CPU: what the LDS annex of the six-wave fused inference grid march may cost, read from the code objects inside libgcfr_hip.so
(the metadata the loader uses, as in tests/test_kernel_resources.py).

The kernels that park their sample positions in LDS (csrc/gcfr_march.hpp: PARK -- fused, groups of 4 and 2, even W/2 and H/2)
  * still fit six waves per SIMD: at most 80 VGPRs, and no scratch;
  * hold ONE annex of 16 KiB whatever the number of tile-function instantiations inside them, and never more than the 26 KiB
    that six workgroups per CU leave each (160 KiB / 6);
and every other march kernel keeps the LDS it had: none in the grid kernels (training, march-only, groups of one, odd
half-parity), the 4,352 B of the combine step in the k-split kernels."""
import os
import re

import pytest

from test_kernel_resources import LLVM, _kernel_metadata

LDS_BUDGET = (160 * 1024) // 6          # six workgroups per CU
ANNEX = 4 * 4 * 64 * 16                 # waves x slots x lanes x (sx, sy) f64
KSPLIT_LDS = 4 * 64 * (4 * 4 + 1)       # the k-split combine: four f32 / i32 planes and one of bytes


def _parks(name):
    """shadow_fwd_quad_kernel<TILE_W, EVEN_HALF, DEPTH, FUSE_SHADE, SCHED>: fused, even half-parity, groups of 4 or 2"""
    m = re.match(r"shadow_fwd_quad_kernel<(\d+), (true|false), (\d+), (true|false), 0>$", name)
    return bool(m) and m.group(2) == "true" and m.group(4) == "true" and int(m.group(3)) >= 2


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_annex_fits_six_waves_and_six_workgroups_and_nothing_else_changes_its_lds(tmp_path):
    k = _kernel_metadata(tmp_path)
    inference = {n: v for n, v in k.items() if n.startswith("shadow_fwd_quad_kernel<")}
    training = {n: v for n, v in k.items() if n.startswith(("shadow_fwd_quad_argmin_kernel<", "shadow_fwd_quad_argmin_own_kernel<"))}
    ksplit = {n: v for n, v in k.items() if n.startswith("shadow_fwd_quad_ksplit_kernel<")}
    parked = {n: v for n, v in inference.items() if _parks(n)}
    # twelve units: 48 inference grid kernels, of which the fused even ones with groups of 4 and 2 park: 4 tile widths x 2 groups
    assert len(inference) == 48 and len(parked) == 8 and len(training) == 96 and len(ksplit) == 96, (len(inference), len(parked), len(training), len(ksplit))
    for n, v in inference.items():
        assert v["vgpr"] <= 80, (n, v)                        # six waves per SIMD
        assert v["scratch"] == 0, (n, v)                      # (the parent: none in any of the 48)
        assert v["lds"] == (ANNEX if n in parked else 0), (n, v)
    assert ANNEX <= LDS_BUDGET
    # both half-parities of the default unit, by name
    for even in ("true", "false"):
        v = inference["shadow_fwd_quad_kernel<16, %s, 4, true, 0>" % even]
        assert v["vgpr"] <= 80 and v["scratch"] == 0 and v["lds"] <= LDS_BUDGET, (even, v)
    for n, v in training.items():
        assert v["lds"] == 0 and v["vgpr"] <= 96, (n, v)
    for n, v in ksplit.items():
        assert v["lds"] == KSPLIT_LDS, (n, v)
