"""GPU: the arithmetic helpers every kernel of the render block goes through (csrc/gcfr_device.hpp) over their whole domains,
against f64 / IEEE references ON THE DEVICE: tests/c/device_primitives_check.hip, built here with the product's own flags
(geomconsistentfr_amd.build.FLAGS minus -shared / -fPIC; the product header is included, not restated), run ONCE as a child
process; one test per helper reads its line.  Every bound below is the issue's or derived in the test's docstring -- none is
what the helpers happened to deliver; the measured values are recorded in profiles/device_primitives.md."""
import os
import shutil
import subprocess

import pytest

import device_primitives_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not on this box")
    from geomconsistentfr_amd.build import FLAGS
    tmp = tmp_path_factory.mktemp("device_primitives")
    exe, dump = str(tmp / "device_primitives_check"), str(tmp / "f64_pairs.bin")
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tests", "c", "device_primitives_check.hip"), "-o", exe], check=True)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, dump], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode in (0, 1), "the check program did not finish (%d):\n%s" % (r.returncode, r.stdout + r.stderr)
    report = ref.check_report(ref.parse_report(r.stdout))
    return {"status": r.returncode, "report": report, "pairs": ref.read_dump(dump)}


def _line(run, name):
    print(name, run["report"][name])
    return run["report"][name]


def test_exp_neg(run):
    """e^-d for every float d of [0, 200], 4096 per binade above, +inf, NaN, against f64 exp: <= 2.0 ulp wherever the reference
    is a normal f32 (v_exp_f32's specified 1 ulp, half an ulp of the closing fma, the hi / lo split's second-order residue);
    below 2^-126 a flush to zero is allowed, so the absolute error is <= 2^-126 there.  exp_neg(0) == 1, exp_neg(+inf) == 0 and
    NaN -> NaN are among the facts."""
    a, sub = _line(run, "exp_neg"), _line(run, "exp_neg_below_normal")
    _line(run, "v_exp_f32")                                                                # the hardware alone: for the record
    assert int(a["bad"]) == 0 and float(a["max_ulp"]) <= 2.0, a
    assert int(sub["bad"]) == 0 and float(sub["max_abs"]) <= 2.0 ** -126, sub
    assert int(sub["count"]) > 0x43480000 - 0x42b00000                                     # every d from 88 to 200 is below normal
    assert int(_line(run, "facts")["failed"], 16) & 0b111 == 0


def test_shadow_transfer(run):
    """w = 1 - 4 e / (1 + e)^2 on the same sweep: <= 1e-6 from the oracle's chain in IEEE f32 on a correctly rounded e (the
    project's own contract); -1e-6 <= w <= 1 everywhere, w == 1 for every d >= 40; w(0) == 0, w(masked distance) == 1,
    w(+inf) == 1, NaN -> NaN.  The distance to tanh^2(d/2) in f64 is reported for helper and chain alike: the formula's own
    cancellation near 0, which both share."""
    b, rng = _line(run, "shadow_transfer"), _line(run, "shadow_transfer_range")
    _line(run, "shadow_transfer_tanh2")
    assert int(b["bad"]) == 0 and float(b["max_abs"]) <= 1e-6, b
    assert int(rng["bad"]) == 0 and int(rng["from40_bad"]) == 0, rng
    assert int(rng["from40_count"]) == 0x43480000 - 0x42200000 + 1 + 121 * 4096 + 1         # [40, 200], the binades above, +inf
    assert int(_line(run, "facts")["failed"], 16) & (0b1111 << 3) == 0


def test_inv_norm3_clamped(run):
    """1 / max(|v|, 1e-12) against f64 on the helper's own f32 |v|^2: relative error <= 3 2^-24.  After the Newton step the
    v_rsq_f32 seed's 1 ulp enters in second order (1.5 (2^-23)^2); what is left is one rounding each of -0.5 s2 r, of the fma
    (a result near 1) and of the final product: 2.5 2^-24.  (0, 0, c) for every positive float c whose square is finite, and
    2^24 hashed vectors of length 1e-13 ... 1e18.  Facts: the zero vector gives 1e12f; |v|^2 one float below, at and above
    1e-24f lands on its side of the clamp; a NaN component gives a NaN product; |v|^2 = +inf gives NaN as documented."""
    for name in ("inv_norm3_axis", "inv_norm3_hashed"):
        c = _line(run, name)
        assert int(c["bad"]) == 0 and float(c["max_rel"]) <= 3.0 * 2.0 ** -24, (name, c)
    assert int(_line(run, "facts")["failed"], 16) & (0b111111 << 7) == 0


def test_lambert_dot(run):
    """n_hat . l_hat against f64 (l formed in f32 as the forward forms it) on 2^24 cases in the shapes of the project's scenes,
    a quarter of them with the exact dot within 2e-4 of zero: absolute error <= 1e-6, and the SIGN agrees wherever
    |dot| >= 1e-4 -- what the backward kernels' kink rule rests on (they take the forward's side inside that window only).
    Bound, in units of 2^-24 (half an f32 ulp of 1): a unit vector's component is v r.  r is within 3 (relative) of
    1 / sqrt(s2) for ITS s2 (test_inv_norm3_clamped); s2 = |v|^2 carries three roundings of non-negative terms, <= 3 relative,
    which the square root halves: 1.5; the product v r rounds once more: 1.  So <= 5.5 relative per component and 11 for a
    product n_i u_i of two of them; the three products' sizes sum to <= 1 (Cauchy-Schwarz), so that is <= 11 absolute.  Then
    three roundings of the products (sizes summing to <= 1: <= 1 together) and two of the sums (each <= 1 in size: 1 each).
    Together <= 14 2^-24 = 8.4e-7 < 1e-6; with a factor of a hundred to the 1e-4 window of the kink rule."""
    d, s = _line(run, "lambert_dot"), _line(run, "lambert_dot_sign")
    assert int(d["bad"]) == 0 and float(d["max_abs"]) <= 1e-6, d
    assert int(s["bad"]) == 0, s
    assert int(s["near_kink_count"]) == 1 << 22 and int(s["near_kink_bad"]) == 0, s          # the construction put them there
    assert int(s["count"]) >= 3 << 22, s             # the sign is checked on all but the near cases inside the window


@pytest.mark.parametrize("name,kind,device_bound", [("fast_rcp64", "rcp", 1), ("fast_sqrt64", "sqrt", 1), ("fast_rsqrt64", "rsqrt", 2)])
def test_fast_f64(run, name, kind, device_bound):
    """401 binades x 2^14 mantissas (structured ones included) and the callers' floors, on the device against the IEEE
    operation (correctly rounded, so the difference is the error to within half an ulp; 1 / sqrt is two rounded operations:
    2), and 64 pairs per binade exactly, in integers.  The exact statement is the device's own, without the device: rcp and
    sqrt lie at most ONE double from the correctly rounded value (|error| <= 1.5 ulp: what '<= 1 ulp difference from IEEE'
    says); rsqrt, which has no IEEE operation to differ from, lies within 1 ulp of the TRUE value (the bracket with k = 1).
    How many rcp / sqrt pairs are beyond 1 ulp of the true value is printed for the record."""
    e = _line(run, name)
    assert int(e["bad"]) == 0 and float(e["max_ulp"]) <= device_bound and int(e["ulp3plus"]) == 0, e
    if device_bound == 1:
        assert int(e["ulp2"]) == 0, e
    assert int(e["ulp0"]) + int(e["ulp1"]) + int(e["ulp2"]) + int(e["ulp3plus"]) == int(e["count"])
    pairs = run["pairs"]
    assert len(pairs) == ref.DUMP_RECORDS
    column = {"rcp": 1, "sqrt": 2, "rsqrt": 3}[kind]
    worst, beyond = 0, []
    for rec in pairs:
        x, y = rec[0], rec[column]
        assert x > 0.0
        if not ref.within_ulps(kind, x, y, 2):
            beyond.append((x.hex(), y.hex()))
        worst = max(worst, ref.rounded_distance(kind, x, y, limit=8))
    print("%s: exact check of %d pairs, farthest from the correctly rounded value %d ulp, beyond 1 ulp of the true value %d"
          % (name, len(pairs), worst, len(beyond)))
    if kind == "rsqrt":
        assert not beyond, beyond[:8]
    else:
        assert worst <= 1


def test_every_check_is_inside_its_bound(run):
    assert run["status"] == 0 and _line(run, "facts") == {"count": str(ref.FACTS), "failed": "0x0"}
