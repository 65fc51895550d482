"""CPU: what GCFR_VISIT_TRIM (csrc/gcfr_march.hpp) may cost in registers, read from the code objects inside
libgcfr_hip.so (the metadata the loader uses, as in tests/test_kernel_resources.py) and, for the default unit, from the compiler's
own resource remarks through tools/resusage.py (the occupancy is only there).

  * all 48 inference grid kernels of the twelve units: at most 80 VGPRs, no scratch -- six waves per SIMD --, and the LDS they had
    (the 16 KiB annex in the eight kernels that park, none elsewhere);
  * the 24 fused ones are the only kernels the switch changes; the march-only inference kernels, the 96 training kernels and the 96
    k-split kernels hold exactly the parent's registers, scratch and LDS (tests/golden/visit_trim_parent_march_resources.json:
    the table of the library built with -DGCFR_VISIT_TRIM=0, which is the parent kernel for kernel --
    profiles/visit_trim_device_code.txt);
  * the default unit through tools/resusage.py: both fused inference kernels at six waves, at most 80 VGPRs, no scratch, and the
    training kernels at five."""
import json
import os
import re
import subprocess
import sys

import pytest

from test_kernel_resources import LLVM, _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANNEX = 4 * 4 * 64 * 16                 # waves x slots x lanes x (sx, sy) f64
PARENT = os.path.join(ROOT, "tests", "golden", "visit_trim_parent_march_resources.json")   # name -> [vgpr, sgpr, scratch, lds]


def _fused(name):
    return re.match(r"shadow_fwd_quad_kernel<\d+, (true|false), \d+, true, 0>$", name) is not None


def _parks(name):
    m = re.match(r"shadow_fwd_quad_kernel<(\d+), (true|false), (\d+), (true|false), 0>$", name)
    return bool(m) and m.group(2) == "true" and m.group(4) == "true" and int(m.group(3)) >= 2


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_inference_kernels_keep_six_waves_and_every_other_march_kernel_is_untouched(tmp_path):
    k = _kernel_metadata(tmp_path)
    with open(PARENT) as f:
        parent = json.load(f)
    march = {n: v for n, v in k.items() if n.startswith("shadow_fwd_quad_")}
    assert sorted(march) == sorted(parent)   # the same 240 kernels
    inference = {n: v for n, v in march.items() if n.startswith("shadow_fwd_quad_kernel<")}
    assert len(inference) == 48 and sum(_fused(n) for n in inference) == 24
    for n, v in inference.items():
        assert v["vgpr"] <= 80 and v["scratch"] == 0, (n, v)                  # six waves per SIMD, nothing spilled
        assert v["lds"] == (ANNEX if _parks(n) else 0) == parent[n][3], (n, v)   # LDS as before
    others = {n: v for n, v in march.items() if not _fused(n)}
    assert len(others) == 240 - 24
    for n, v in others.items():   # march-only inference, training (argmin, argmin_own), k-split: the parent's numbers exactly
        assert [v["vgpr"], v["sgpr"], v["scratch"], v["lds"]] == parent[n], (n, v, parent[n])
    for n in (m for m in inference if _fused(m)):   # the changed kernels: no more vector registers than the parent's, no scratch either side
        assert march[n]["vgpr"] <= parent[n][0] and parent[n][2] == 0, (n, march[n], parent[n])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_default_unit_through_resusage():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resusage.py"), "--all"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(\S.*?)\s+sgpr\s+(\d+) vgpr\s+(\d+) scratch\s+(\d+) occ (\d+) lds (\d+)", line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("sgpr", "vgpr", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    inference = {n: v for n, v in rows.items() if n.startswith("shadow_fwd_quad_kernel<")}
    training = {n: v for n, v in rows.items() if n.startswith("shadow_fwd_quad_argmin")}
    assert len(inference) == 4 and len(training) == 8, sorted(rows)
    for n, v in inference.items():
        assert v["occ"] == 6 and v["vgpr"] <= 80 and v["scratch"] == 0, (n, v)
    assert inference["shadow_fwd_quad_kernel<16, true, 4, true, 0>"]["lds"] == ANNEX
    for n, v in training.items():
        assert v["occ"] == 5 and v["scratch"] == 0 and v["lds"] == 0, (n, v)
