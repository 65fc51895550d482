"""No GPU: the pieces the device-primitives checks stand on (tests/device_primitives_reference.py).
  * tests/c/device_primitives_check.hip compiles for gfx950 against the product headers, so a header change that breaks the
    check program is seen on a box without a GPU;
  * the exact integer bracket reports a planted distance of 0, 1, 2 and 3 ulp from a correctly rounded value as exactly that;
  * the byte lattice has teeth: recomputed the way a wrong kernel would (the f32 mask as a multiplication by 1/255.0f; 255.0f r
    widened before the product), the expected bytes change;
  * the report parser rejects a missing check and a short sweep."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import device_primitives_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_program_compiles_for_gfx950(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not on this box")
    from geomconsistentfr_amd.build import FLAGS
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["-c", os.path.join(ROOT, "tests", "c", "device_primitives_check.hip"), "-o",
                                          str(tmp_path / "device_primitives_check.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _isqrt_round(n):
    """round-half-up of sqrt(n) for an integer n (ties cannot occur for the n used here)"""
    import math
    r = math.isqrt(n)
    return r + 1 if (2 * r + 1) ** 2 < 4 * n else r


def _correctly_rounded(kind, x):
    """f(x) rounded to the nearest double, from integers alone"""
    fx = Fraction(x)
    scale = 1 << 400
    if kind == "rcp":
        big = (scale * fx.denominator * 2 + fx.numerator) // (2 * fx.numerator)            # round(scale / x)
    elif kind == "sqrt":
        big = _isqrt_round(scale * scale * fx.numerator // fx.denominator)                # x is dyadic: the division is exact
    else:
        big = _isqrt_round(scale * scale * fx.denominator // fx.numerator)
    # big / scale carries ~400 bits; round it to 53
    drop = big.bit_length() - 53
    m = (big + (1 << (drop - 1))) >> drop
    return float(Fraction(m << drop, scale))


XS = [1.0 + 2.0 ** -30, 3.0, 1e-24, 1e-12, 1e-4, 0.7071067811865476, 1.7e+55, 5.5e-61, 2.0 - 2.0 ** -52, 123456.789]


@pytest.mark.parametrize("kind", ["rcp", "sqrt", "rsqrt"])
def test_bracket_reports_planted_distances_exactly(kind):
    import math
    for x in XS:
        y0 = _correctly_rounded(kind, x)
        assert ref.within_ulps(kind, x, y0, 1)                                            # within half an ulp: correctly rounded
        lib = {"rcp": 1.0 / x, "sqrt": math.sqrt(x), "rsqrt": 1.0 / math.sqrt(x)}[kind]
        assert abs(lib - y0) <= 2 * math.ulp(y0)                                          # (the integer route found the right number)
        for d in (0, 1, 2, 3):
            for sign in (1, -1):
                y = y0
                for _ in range(d):
                    y = math.nextafter(y, sign * math.inf)
                if math.frexp(y)[1] != math.frexp(y0)[1]:
                    continue                                                               # stepped into another binade: another ulp
                assert ref.rounded_distance(kind, x, y) == d, (kind, x, d, sign)
                if d == 0:
                    assert ref.within_ulps(kind, x, y, 2)
                if d >= 2:
                    assert not ref.within_ulps(kind, x, y, 2), (kind, x, d)              # the k = 1 bracket the GPU test asserts


def test_bracket_on_exact_results():
    assert ref.rounded_distance("sqrt", 4.0, 2.0) == 0 and ref.within_ulps("sqrt", 4.0, 2.0, 0)
    assert ref.rounded_distance("rcp", 4.0, 0.25) == 0 and ref.within_ulps("rcp", 4.0, 0.25, 0)
    assert ref.rounded_distance("rsqrt", 4.0, 0.5) == 0 and ref.within_ulps("rsqrt", 4.0, 0.5, 0)
    assert not ref.within_ulps("rsqrt", 4.0, np.nextafter(0.5, 1.0), 0)


def test_lattice_covers_every_mask_byte_and_changes_under_the_mutants():
    total = 0
    for mask_f32 in (False, True):
        lat = ref.byte_lattice(mask_f32)
        assert lat["mask_u8"].shape == (256, 256) and (lat["mask_u8"][:, 7] == np.arange(256)).all()
        for p in ref.PLANES:                                                               # every mask byte has kept cases in every plane
            rows = lat["kept"][p].reshape(256, -1).any(axis=1)
            assert rows[1:].all() and (rows[0] or p != "rendered_image"), p
        plain = ref.lattice_expected(lat, mask_f32)
        cases = ref.lattice_cases(lat)
        total += cases
        # planted ties are decisive: both parities of the target appear in every plane
        for p in ref.PLANES:
            assert len(np.unique(plain[p][lat["kept"][p]])) >= 80, p
        if mask_f32:
            changed = ref.lattice_differences(lat, plain, ref.lattice_expected(lat, True, mutant_mask=True))
            print("f32 mode: %d of %d cases change under the reciprocal-multiply mask" % (changed, cases))
            assert changed >= 0.05 * cases                                                 # a floor on the test's power, not a tolerance
        widened = ref.lattice_differences(lat, plain, ref.lattice_expected(lat, mask_f32, widen_rendered=True))
        print("mask_f32=%s: %d of %d cases change when 255.0f r is widened first" % (mask_f32, widened, cases))
        assert widened >= 1
    print("cases over both modes: %d" % total)
    assert total > 200000


def test_lattice_extra_pixels():
    lat = ref.byte_lattice(False)
    assert lat["mask_u8"][255, 253] == 255 and np.isnan(lat["rendered"][0, 255, 253]) and np.isposinf(lat["rendered"][0, 255, 254])
    assert lat["rendered"][0, 255, 255] < 0
    exp = ref.lattice_expected(lat, False)["rendered_image"]
    assert list(exp[255, 253:, 0]) == [0, 255, 0]


def _report():
    lines = []
    for name, count in ref.COUNTS.items():
        lines.append("%s count=%d max_ulp=0.5 worst=0x00000000 bad=0" % (name, count if count is not None else 1))
    return "\n".join(lines) + "\n"


def test_parser_accepts_a_whole_report_and_rejects_a_missing_check_and_a_short_count():
    text = _report()
    rep = ref.check_report(ref.parse_report(text))
    assert rep["exp_neg"]["worst"] == "0x00000000" and float(rep["fast_rcp64"]["max_ulp"]) == 0.5
    for name, count in ref.COUNTS.items():
        missing = "\n".join(l for l in text.splitlines() if not l.startswith(name + " "))
        with pytest.raises(AssertionError, match=name):
            ref.check_report(ref.parse_report(missing))
        if count is not None:
            short = text.replace("%s count=%d " % (name, count), "%s count=%d " % (name, count - 1))
            with pytest.raises(AssertionError, match=name):
                ref.check_report(ref.parse_report(short))
    with pytest.raises(AssertionError):
        ref.check_report(ref.parse_report("hipErrorNoDevice\n"))
