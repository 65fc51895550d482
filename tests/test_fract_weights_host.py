"""CPU: the bilinear weights of the bounds variant of the grid march as two v_fract_f64 per axis (csrc/gcfr_device.hpp:
bilinear_weights, csrc/gcfr_march.hpp: FRACT) -- the argument that they are the reference's weights bit for bit
on every position a marched image can produce, in exact rational arithmetic (`fractions`; rn() = correct rounding to double).

Both forms restated:
  parent   w0 = rn(ceil(u) - u),  w1 = rn(u - floor(u))                      (T8:492-494; floor, ceil, two subtractions)
  new      w1 = fract(u),  w0 = fract(-u),  fract(v) = min(rn(v - floor(v)), 1 - 2^-53)     (what v_fract_f64 computes: the
           instruction itself is pinned on the device by tests/test_gpu_fract_weights.py)
They agree on integers (0 and 0), on (-1, 0) (the wrap column / row), on large |u| and on every binade from 2^-53 up; they differ
exactly where rn(1 - |u|) = 1.0, which the instruction clamps: 0 < |u| <= 2^-54 (at |u| = 2^-54 itself the tie goes to the even
neighbour, 1.0, so the end point belongs to the window; the bound below is therefore asserted STRICTLY).

Reachability.  ux = (sx + W/2) - 0.0001 and uy = (H/2 - sy) - 0.0001 (csrc/gcfr_march.hpp).  Near u = 0 the sum a = sx + W/2 is
about 1e-4, |sx| about W/2 - 1e-4: sx and W/2 have opposite signs and magnitudes within a factor of two, so a is exact (Sterbenz)
and, as sx and the integer W/2 are both multiples of ulp(sx), a multiple g ulp(sx).  a and the double c = 0.0001 are again within
a factor of two where u is small, so u = a - c exactly: the smallest non-zero |u| is the distance of c to the grid of multiples
of ulp(sx) (the grid's own spacing if c lies on it).  For every even size from 6 up that distance exceeds 2^-54; for half-sizes
1 and 2 (|s| in [0.5, 1) and [1, 2)) it does not, which is why images of fewer than six rows or columns never march in the
bounds variant (use_zb in march_tile).  (The sign of a zero weight is not modelled here: the device test compares bit patterns.)"""
import math
import random
from fractions import Fraction

ONE_MINUS = Fraction(2 ** 53 - 1, 2 ** 53)   # 1 - 2^-53, the largest double below 1
WINDOW = Fraction(1, 2 ** 54)                # the forms differ for 0 < |u| <= WINDOW
C = 0.0001                                   # the double the kernels subtract (T8:483)


def rn(q):
    """correct rounding of a rational to double (CPython's int / int true division is correctly rounded)"""
    return float(q)


def parent(u):
    q = Fraction(u)
    return rn(math.ceil(q) - q), rn(q - math.floor(q))


def fract(q):
    return min(Fraction(rn(q - math.floor(q))), ONE_MINUS)


def new(u):
    q = Fraction(u)
    return float(fract(-q)), float(fract(q))


def in_window(u):
    return 0 < abs(Fraction(u)) <= WINDOW


def check(u):
    """the forms agree outside the window and differ inside it"""
    same = parent(u) == new(u)
    assert same != in_window(u), (u.hex(), parent(u), new(u))
    return same


def test_equal_on_integers_zeros_the_wrap_interval_and_large_positions():
    for i in range(-4, 1101):
        assert parent(float(i)) == new(float(i)) == (0.0, 0.0)
    assert parent(-0.0) == new(-0.0) == (0.0, 0.0)
    rng = random.Random(1)
    for _ in range(1000):                    # (-1, 0): floor = -1, the texel column / row that wraps
        u = -rng.random() or -0.5
        assert check(u) and new(u) == (-u, rn(Fraction(u) + 1))
    assert new(-0.0001) == parent(-0.0001) and abs(new(-0.0001)[1] - 0.9999) < 1e-15
    for e in range(13, 60):                  # large |u|: beyond 2^52 every double is integral
        for _ in range(40):
            u = math.ldexp(1.0 + rng.random(), e) * rng.choice((-1.0, 1.0))
            assert check(u)
    for u in (2.0 ** 52 + 1, -(2.0 ** 52 + 1), 2.0 ** 53, 1e300, -1e300, math.nextafter(4.0, 0.0), math.nextafter(-4.0, 0.0)):
        assert check(u)


def test_they_differ_only_inside_the_window():
    rng = random.Random(2)
    n_in = n_out = 0
    for e in range(-70, 13):                 # every binade [2^e, 2^(e+1)) from 2^-70 to 2^12, both signs
        lo = math.ldexp(1.0, e)
        us = [lo, math.nextafter(lo, math.inf), math.nextafter(2 * lo, 0.0)] + [math.ldexp(1.0 + rng.random(), e) for _ in range(80)]
        for u in us:
            for v in (u, -u):
                if check(v):
                    n_out += 1
                else:
                    n_in += 1
    assert n_in > 0 and n_out > 0
    # the window's end points and its neighbours: 2^-54 (tie to even: 1.0) is inside, the next double up is outside
    w = math.ldexp(1.0, -54)
    for s in (1.0, -1.0):
        assert not check(s * w) and not check(s * math.nextafter(w, 0.0)) and check(s * math.nextafter(w, 1.0))
        assert not check(s * 5e-324)         # the smallest denormal
    # inside the window the difference is the clamp and nothing else: the parent has the weight 1.0, the instruction 1 - 2^-53
    assert parent(1e-17) == (1.0, 1e-17) and new(1e-17) == (float(ONE_MINUS), 1e-17)
    assert parent(-1e-17) == (1e-17, 1.0) and new(-1e-17) == (1e-17, float(ONE_MINUS))


def smallest_nonzero_u(half):
    """the smallest non-zero |u| = |g ulp - c| an image of half-size `half` can produce near u = 0 (see the module's docstring)"""
    c = Fraction(C)
    s_lo, s_hi = half - 2 * C, half - C / 2            # |s| where a = half - |s| lies within a factor of two of c
    e = math.frexp(s_lo)[1] - 1                        # 2^e <= |s| < 2^(e+1)
    assert math.frexp(s_hi)[1] - 1 == e, half          # one binade
    ulp = Fraction(2) ** (e - 52)
    g = math.floor(c / ulp)
    best = min(d for d in (abs(g * ulp - c), abs((g + 1) * ulp - c), ulp) if d != 0)
    # (u = a - c is exact there: a and c are multiples of ulp(c) = 2^-66 within a factor of two of each other)
    assert rn(best) == best
    return best


def test_no_position_of_an_image_of_six_or_more_rows_and_columns_reaches_the_window():
    worst = {}
    for size in range(6, 4097, 2):           # W and H alike: uy = (H/2 - sy) - 0.0001 has the structure of ux
        d = smallest_nonzero_u(size // 2)
        assert d > WINDOW, (size, float(d))
        e = math.frexp(size // 2 - C)[1] - 1
        worst[e] = min(worst.get(e, d), d)
    # the figures of DESIGN.md 4.1h, per binade of |s|
    assert 2.0e-16 < float(worst[1]) < 2.2e-16         # [2, 4)
    assert all(2.2e-16 < float(worst[e]) < 2.4e-16 for e in (2, 3, 4))      # [4, 32)
    assert all(float(worst[e]) > 3.2e-15 for e in (6, 7, 8))                # [64, 512)


def test_half_sizes_one_and_two_do_reach_it():
    for half in (1, 2):                      # images of 2 or 4 rows / columns: the guard in march_tile
        d = smallest_nonzero_u(half)
        assert 0 < d < WINDOW, (half, float(d))
        assert 1.0e-17 < float(d) < 1.2e-17
