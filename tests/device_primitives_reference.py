"""Helper module (no tests, no GPU) of tests/test_gpu_device_primitives.py, tests/test_device_primitives_host.py and the byte
lattices of tests/test_gpu_postprocess.py / tests/test_gpu_rig_frames.py:

  parse_report / check_report   the lines of tests/c/device_primitives_check.hip: every check present, no sweep shorter than stated
  within_ulps / rounded_distance   exact brackets in Python integers for the f64 helpers' dumped (x, result) pairs
  byte_lattice / lattice_expected  one 256 x 256 image per plane whose values sit ON the half-way points of the scripts' byte
                                   expressions (oracle/postprocess_statements.py) for every mask byte, and the bytes expected there
"""
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import postprocess_statements as st  # noqa: E402  (checker only)

# ---------------------------------------------------------------------------------------------------------------------
# the check program's report
# ---------------------------------------------------------------------------------------------------------------------
EXP_SWEEP = 0x43480000 + 1 + 121 * 4096 + 2          # every float of [0, 200]; 4096 per binade above, (200, 256) included; +inf; a NaN
F64_GRID = 401 * (1 << 14) + 3                       # binades 2^-200 ... 2^200 with 2^14 mantissas each; the three floors
DUMP_RECORDS = 401 * 64 + 3
FACTS = 13
# name of the line -> the pattern count it must state (a sweep that shrinks fails)
COUNTS = {
    "exp_neg": EXP_SWEEP,
    "v_exp_f32": None,                                # report only: the inputs whose 2^t is a normal f32
    "exp_neg_below_normal": None,                     # part of exp_neg's count
    "shadow_transfer": EXP_SWEEP,
    "shadow_transfer_tanh2": EXP_SWEEP - 1,           # (not the NaN)
    "shadow_transfer_range": EXP_SWEEP - 1,
    "inv_norm3_axis": 0x5f7fffff,                     # every positive float whose square is finite
    "inv_norm3_hashed": 1 << 24,
    "lambert_dot": 1 << 24,
    "lambert_dot_sign": None,                         # the cases with |dot| >= 1e-4: bounded below in the test
    "fast_rcp64": 2 * F64_GRID,                       # both signs
    "fast_sqrt64": F64_GRID,
    "fast_rsqrt64": F64_GRID,
    "facts": FACTS,
}


def parse_report(text):
    """-> {name: {key: value string}} of the `name key=value ...` lines"""
    out = {}
    for line in text.splitlines():
        parts = line.split()
        if len(parts) >= 2 and all("=" in p for p in parts[1:]):
            out[parts[0]] = dict(p.split("=", 1) for p in parts[1:])
    return out


def check_report(report):
    """every check's line is there and states its whole sweep; raises AssertionError naming the first that does not"""
    for name, count in COUNTS.items():
        assert name in report, "the check program printed no line for %s" % name
        assert "count" in report[name], "%s states no pattern count" % name
        if count is not None:
            assert int(report[name]["count"]) == count, "%s checked %s patterns, not %d" % (name, report[name]["count"], count)
    return report


# ---------------------------------------------------------------------------------------------------------------------
# exact brackets for 1/x, sqrt(x), 1/sqrt(x) of f64: integers only, nothing is rounded
# ---------------------------------------------------------------------------------------------------------------------
def _split(x):
    """a finite positive double as (integer mantissa, exponent): x == m 2^e exactly, m < 2^53"""
    assert x > 0.0 and math.isfinite(x)
    m, e = math.frexp(x)
    return int(m * (1 << 53)), e - 53


def _ulp_exponent(y):
    """spacing of the doubles at y is 2^this (y normal)"""
    return math.frexp(y)[1] - 53


def _cmp_scaled(a, ea, b, eb):
    """sign of a 2^ea - b 2^eb for integers a, b"""
    e = min(ea, eb)
    l, r = a << (ea - e), b << (eb - e)
    return (l > r) - (l < r)


def within_ulps(kind, x, y, half_ulps):
    """True iff |y - f(x)| <= (half_ulps / 2) ulp(y), f = 1/x ("rcp"), sqrt ("sqrt") or 1/sqrt ("rsqrt"), x, y > 0.
    For rsqrt with k = half_ulps / 2: (y - k ulp)^2 x <= 1 <= (y + k ulp)^2 x; the others alike.  y and ulp are taken in
    units of ulp / 2, so that k = 1/2 -- 'y is the correctly rounded value' -- is an integer statement too."""
    mx, ex = _split(x)
    my, ey = _split(y)
    shift = ey - _ulp_exponent(y) + 1                 # y = Y 2^u with u = ulp exponent - 1
    Y, u = my << shift, _ulp_exponent(y) - 1
    lo, hi = Y - half_ulps, Y + half_ulps
    if kind == "rcp":                                 # lo 2^u x <= 1 <= hi 2^u x
        return _cmp_scaled(lo * mx, u + ex, 1, 0) <= 0 <= _cmp_scaled(hi * mx, u + ex, 1, 0)
    if kind == "sqrt":                                # lo^2 2^2u <= x <= hi^2 2^2u
        low_ok = lo <= 0 or _cmp_scaled(lo * lo, 2 * u, mx, ex) <= 0
        return low_ok and _cmp_scaled(hi * hi, 2 * u, mx, ex) >= 0
    if kind == "rsqrt":                               # lo^2 2^2u x <= 1 <= hi^2 2^2u x
        low_ok = lo <= 0 or _cmp_scaled(lo * lo * mx, 2 * u + ex, 1, 0) <= 0
        return low_ok and _cmp_scaled(hi * hi * mx, 2 * u + ex, 1, 0) >= 0
    raise ValueError(kind)


def rounded_distance(kind, x, y, limit=64):
    """how many doubles y lies from the correctly rounded f(x): the least d with |y - f(x)| <= (d + 1/2) ulp(y)"""
    for d in range(limit):
        if within_ulps(kind, x, y, 2 * d + 1):
            return d
    return limit


def read_dump(path):
    """the check program's file: records of (x, fast_rcp64, fast_sqrt64, fast_rsqrt64) as raw f64"""
    raw = open(path, "rb").read()
    assert len(raw) % 32 == 0
    return [struct.unpack_from("<4d", raw, o) for o in range(0, len(raw), 32)]


# ---------------------------------------------------------------------------------------------------------------------
# the byte lattice
# ---------------------------------------------------------------------------------------------------------------------
SIDE = 256
LIMIT = 1.2                                            # values beyond it are dropped (their pixels carry 0 and are not counted)
PLANES = ("rendered_image", "shadow_mask", "albedo", "depth", "shading", "surface_normals")


def mask_value(mask_u8, mask_f32, mutant=False):
    """the mask as the script holds it (f64 array / 255.0, or torch's f32 quotient); mutant: the f32 quotient formed by a
    multiplication with the rounded reciprocal -- what a kernel must NOT do"""
    if mutant:
        return mask_u8.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    return (mask_u8.astype(np.float32) / np.float32(255.0)) if mask_f32 else mask_u8 / 255.0


def _near_half_way(mask_f32, which):
    """(256,256) f32 and the kept pixels: row i under mask byte i; column j: target byte k = j // 3, and (j + which) % 3 picks the
    f32 nearest to t = (k + 0.5) / (255 m), the float below it or the float above it"""
    i, j = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    m = mask_value(i.astype(np.uint8), mask_f32).astype(np.float64)
    with np.errstate(divide="ignore"):
        t = ((j // 3) + 0.5) / (255.0 * m)
    kept = np.isfinite(t) & (t <= LIMIT)
    v = np.where(kept, t, 0.0).astype(np.float32)
    pick = (j + which) % 3
    v = np.where(pick == 1, np.nextafter(v, np.float32(-np.inf)), np.where(pick == 2, np.nextafter(v, np.float32(np.inf)), v))
    return np.where(kept, v, np.float32(0.0)).astype(np.float32), kept


def byte_lattice(mask_f32):
    """-> dict: mask_u8 (256,256); input (256,256,3); rendered, albedo, normals (3,256,256); depth (1,256,256); shadow, shading
    (256,256), all f32; kept: {plane: bool array in the plane's output layout}.
    Each plane's expression comes to k + 0.5, or one f32 step of its operand beside it, wherever `kept`:
      rendered, albedo (255.0f v) m;  shadow (255.0f v) m in the mask's dtype;  shading (255.0 v) m in f64;
      normals (255.0 (n + 1.0) / 2.0) m with n = 2 v - 1;  depth 255.0f d m with d = v after the min-max step (planted 0 and 1
      make that step the identity; v <= 1 there);  under mask 0 the composite keeps the photograph: input 255.0, input = (k + 0.5) / 255.
    Row 255 carries a NaN, a +inf and a negative rendered value in its last three columns (channel 0)."""
    mask_u8 = np.repeat(np.arange(SIDE, dtype=np.uint8)[:, None], SIDE, axis=1)
    chans = [_near_half_way(mask_f32, c) for c in range(3)]
    rendered = np.stack([c[0] for c in chans])
    kept3 = np.stack([c[1] for c in chans], axis=2)                                # HWC, as the outputs are
    albedo = np.stack([chans[(c + 1) % 3][0] for c in range(3)])
    kept_albedo = np.stack([chans[(c + 1) % 3][1] for c in range(3)], axis=2)
    normals = (2.0 * np.stack([chans[(c + 2) % 3][0] for c in range(3)]).astype(np.float64) - 1.0).astype(np.float32)
    kept_normals = np.stack([chans[(c + 2) % 3][1] for c in range(3)], axis=2)
    shadow, kept1 = _near_half_way(mask_f32, 1)
    shading, _ = _near_half_way(mask_f32, 2)
    d, kept_d = _near_half_way(mask_f32, 0)
    kept_d &= d <= 1.0
    d = np.where(kept_d, d, np.float32(0.0))
    d[0, 0], d[0, 1] = 0.0, 1.0                                                     # the batch's range: -depth in [0, 1] exactly
    depth = (-d)[None].astype(np.float32)
    # the photograph: half-way points of input 255.0 in every row, decisive where the mask is 0
    j = np.arange(SIDE)
    photo = np.float32(((j // 3) * 3 + 0.5) / 255.0)                               # bytes 0, 3, ... 255
    photo = np.where(j % 3 == 1, np.nextafter(photo, np.float32(-1)), np.where(j % 3 == 2, np.nextafter(photo, np.float32(2)), photo))
    inp = np.repeat(np.repeat(photo[None, :, None], SIDE, axis=0), 3, axis=2).astype(np.float32)
    rendered[0, 255, 253:] = [np.nan, np.inf, -0.25]
    kept_r = kept3.copy()
    kept_r[0, :, :] = True                                                          # mask 0: the photograph's lattice
    return {"mask_u8": mask_u8, "input": inp, "rendered": rendered, "albedo": albedo, "normals": normals, "depth": depth,
            "shadow": shadow, "shading": shading,
            "kept": {"rendered_image": kept_r, "shadow_mask": kept1, "albedo": kept_albedo, "depth": kept_d, "shading": kept1.copy(),
                     "surface_normals": kept_normals}}


def lattice_expected(lat, mask_f32, mutant_mask=False, widen_rendered=False):
    """{plane: u8} from the scripts' statements; the two flags recompute them as a wrong kernel would (the host tests measure
    how many bytes that changes: the lattice's power)"""
    m01 = mask_value(lat["mask_u8"], mask_f32, mutant=mutant_mask)
    ren = lat["rendered"].astype(np.float64) if widen_rendered else lat["rendered"]
    with np.errstate(invalid="ignore", over="ignore"):
        exp = st.diagnostic_images(lat["input"].astype(np.float64), lat["albedo"], lat["depth"][None], 0, lat["shadow"], ren,
                                   lat["shading"].astype(np.float64), lat["normals"].astype(np.float64), m01)
        return {k: st.to_uint8(v) for k, v in exp.items()}


def lattice_cases(lat):
    return int(sum(k.sum() for k in lat["kept"].values()))


def lattice_differences(lat, a, b):
    """kept cases at which two sets of expected bytes differ"""
    return int(sum(((a[p] != b[p]) & lat["kept"][p]).sum() for p in PLANES))
