"""GPU: bilinear_weights() (csrc/gcfr_device.hpp) -- the bilinear weights of the bounds variant of the grid march as two
v_fract_f64 per axis -- against the reference's floor / ceil / two subtractions, bit for bit, on the device
(tests/c/fract_weights_check.hip, built here with hipcc; the product helper is included, not restated):
  * every binade 2^-70 ... 2^12, both signs: the first 2^20 doubles and 2^20 random mantissas of each;
  * the 2^12 doubles either side of every integer -2 ... 1100, +0 and -0;
  * the positions round u = 0 that images of every even size 6 ... 2048 can produce, through the march's own expressions.
No mismatch outside 0 < |u| <= 2^-54; inside it EVERY position mismatches (the instruction clamps to 1 - 2^-53 where IEEE rounds
1 - |u| to 1.0: the clamp is what tests/test_fract_weights_host.py assumes), and no reachable position lies inside it.  What the
helper returns for +-0, +-inf and NaN is printed (DESIGN.md 4.1h records it; the march's positions are finite by construction)."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fract_weights_equal_the_reference_weights_outside_the_unreachable_window(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not on this box")
    exe = str(tmp_path / "fract_weights_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    os.path.join(ROOT, "tests", "c", "fract_weights_check.hip"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"total +mismatches outside the window (\d+), inside (\d+) of (\d+), reachable positions in the window (\d+)", r.stdout)
    assert m, r.stdout
    outside, inside, seen, reachable = map(int, m.groups())
    assert outside == 0 and reachable == 0, r.stdout
    assert inside == seen > 0, r.stdout                # the clamp, everywhere in the window
    checked = {k: int(v) for k, v in re.findall(r"^(\w+) +checked +(\d+)", r.stdout, re.M)}
    assert checked["binades"] == 83 * 2 * 2 ** 21, r.stdout
    assert checked["integers"] == 1103 * (2 ** 13 + 1) + 1, r.stdout
    assert checked["reachable"] == 1022 * 2 * (2 ** 12 + 1), r.stdout
    # +0 and -0: both weights zero, as the reference has them
    for name in (r"\+0", "-0"):
        assert re.search(r"u = %s +w0 = -?0 \(0x[08]0{15}\) +w1 = -?0 \(0x[08]0{15}\)" % name, r.stdout), r.stdout
