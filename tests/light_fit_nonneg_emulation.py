"""The non-negative solve's operation order (gcfr_light_fit_solve_nonneg: csrc/gcfr_light_fit.hip, include/gcfr.h), restated in
numpy f64 (helper module, no tests): Lawson and Hanson's active-set method on the normal equations, step for step as the header
numbers them.  tests/test_gpu_light_fit_nonneg.py holds the kernel to it bit for bit; tests/test_light_fit_nonneg_host.py holds it
to statements that do not share its algorithm (a KKT certificate, a brute force over all supports, scipy's nnls on the explicit
design matrix), so that it is a checked statement and not a second opinion.

Nothing of the unconstrained solve is written a second time: every factorisation is `light_fit_emulation.solve` itself on the
rows and columns of the passive set (ridge 0 there adds an exact +0 to an already shifted diagonal), and the summed, ridged system
is taken from the same function's order -- `system()` below states the sum over the faces and the ridge once more only because
`solve` does not return them, and the host test holds it to `solve` bit for bit where the passive set ends as all lights.  The
domain is a FINITE gram (a non-finite one would make `solve`'s zero ridge a NaN); rhs may hold anything.

Arrays in the C ABI's layouts: gram (B,3,L,L) f64, rhs (B,3,L) f64, rgb (1|B,L,3) f32, info and solves (1|B,3) i32."""
import functools

import numpy as np

import light_fit_emulation as lfe
from f32_bits import F32

# Gates, each FOUR TIMES the largest figure measured on the CPU by tests/test_light_fit_nonneg_host.py (the restatement against the
# independent statements named there; distances relative to the largest entry of the reference):
GATE_KKT_STATIONARITY = 4 * 5.24e-16   # max |g_l| / max|r| over x_l > 0, g = A x - r on the test's own A, r  (at (1,63,33,47), ridge 0)
GATE_BRUTE_FORCE = 4 * 2.23e-15        # against the best feasible support of all 2^L, L <= 8                 (at (2,5,21,37), ridge 1e-3)
GATE_NNLS = 4 * 2.21e-14               # against scipy.optimize.nnls on the explicit design matrix            (at (1,64,33,47), ridge 1e-3)
# ... and the round trip of a known rig with exact zeros through the rig stage: the image is the rig stage's own (f32 products and
# sums over the lights, light_rig_emulation.forward = combine_lights bit for bit), |x - x_true| / max|x_true| of the f32 solution:
# 4.80e-7 at L = 64, 33 x 47 (90 of 192 entries of x_true are zero), 1.57e-8 at (2,5,21,37)
GATE_RECOVERY = 4 * 4.80e-7


# the shapes of light_fit_emulation.SHAPES the solve is held to FROM PIXELS (the last: one weight and one rig shared by three faces)
PIXEL_SHAPES = [s for s in lfe.SHAPES if s[:4] in ((1, 1, 1, 1), (1, 3, 7, 5), (2, 5, 21, 37), (1, 63, 33, 47), (1, 64, 33, 47), (3, 4, 9, 11))]
GRAM_LIGHTS = (1, 2, 5, 64)            # ... and from Gram matrices handed straight to the C entry: two faces of 13 x 11 pixels
RIDGES = (0.0, 1e-3)


def _geometry(B, H, W):
    from geomconsistentfr_amd.lighting import light_fit_geometry
    return light_fit_geometry(B, H, W)


@functools.lru_cache(maxsize=None)
def pixel_case(B, L, H, W, shared_w):
    """-> (final, albedo, image, weight, gram, rhs): planes and photograph uniform as light_fit_emulation.make_inputs draws them (the
    unconstrained fit of such a photograph has negative entries), a {0,1} weight; computed once, shared by the tests, never modified"""
    final, albedo, image, w = lfe.make_inputs(900 + 7 * L + W, B, L, H, W, "ones" if H * W == 1 else "mask", shared_weight=shared_w)
    chunk, groups = _geometry(B, H, W)
    return (final, albedo, image, w) + lfe.normal_equations(final, albedo, image, w, True, chunk, groups)


@functools.lru_cache(maxsize=None)
def gram_case(L, B=2, H=13, W=11):
    """-> (final, albedo, image, gram, rhs) of the mixed-sign family: the photograph synthesised from mixed_sign_rig, no weight"""
    final, albedo, image, _w = lfe.make_inputs(700 + L, B, L, H, W, None, x_true=mixed_sign_rig(70 + L, B, L))
    chunk, groups = _geometry(B, H, W)
    return (final, albedo, image) + lfe.normal_equations(final, albedo, image, None, True, chunk, groups)


@functools.lru_cache(maxsize=None)
def solved(kind, key, ridge, max_solves=0):
    """solve() of pixel_case(*key) (kind "pixels"; a shared weight also shares the rig) or gram_case(key) (kind "gram"), once"""
    if kind == "pixels":
        c = pixel_case(*key)
        return solve(c[4], c[5], ridge, key[4], max_solves)
    c = gram_case(key)
    return solve(c[3], c[4], ridge, False, max_solves)


def all_negative_rhs():
    """(gram, rhs) with every entry of rhs negative: x = 0 after 0 factorisations"""
    c = gram_case(5)
    return c[3], -np.abs(c[4])


def one_nan_in_rhs():
    """(gram, rhs) with rhs[0, 1, 2] a NaN: that light is never admitted, the others are fitted without it"""
    c = gram_case(5)
    rhs = c[4].copy()
    rhs[0, 1, 2] = np.nan
    return c[3], rhs


def mixed_sign_rig(seed, B, L):
    """x_true (B,L,3) uniform in [-0.5, 1.5]: the family whose unconstrained fit has negative entries"""
    return np.random.default_rng(seed).uniform(-0.5, 1.5, (B, L, 3))


def sparse_rig(seed, B, L):
    """x_true (B,L,3) f32: about 40 % exact zeros, the rest uniform in [0.2, 1] -- a rig a non-negative fit can return"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.2, 1.0, (B, L, 3))
    x[rng.random((B, L, 3)) < 0.4] = 0.0
    return x.astype(F32)


def system(gram, rhs, ridge, shared, rig, c):
    """(A (L,L) full symmetric, r (L,)) of one (rig, channel) in `light_fit_emulation.solve`'s order: the faces added in ascending
    b, the trace in ascending l, A[l,l] = G[l,l] + ridge * (trace / L).  Only the lower triangle of gram is read."""
    B, _, L, _ = gram.shape
    A, r = gram[rig, c].copy(), rhs[rig, c].copy()
    if shared:
        for b in range(1, B):
            A, r = A + gram[b, c], r + rhs[b, c]
    A = np.where(np.tril(np.ones((L, L), bool)), A, A.T)
    trace = 0.0
    for l in range(L):
        trace = trace + A[l, l]
    shift = np.float64(ridge) * (trace / np.float64(L))
    for l in range(L):
        A[l, l] = A[l, l] + shift
    return A, r


def _solve_on(A, r, P):
    """A_PP s_P = r_P by light_fit_emulation.solve -> (s (len(P),) f64, 0 | index into P of the bad pivot + 1).  `solve` takes three
    channels: the system is channel 0, the other two are zero matrices, which it leaves at their first pivot."""
    gram, rhs = np.zeros((1, 3, P.size, P.size)), np.zeros((1, 3, P.size))
    gram[0, 0], rhs[0, 0] = A[np.ix_(P, P)], r[P]
    _rgb, info, s = lfe.solve(gram, rhs, 0.0, False)
    return s[0, :, 0], int(info[0, 0])


def solve_one(A, r, max_solves=0):
    """one (rig, channel): -> (x (L,) f64, info, solves, counters); the numbers are the header's steps"""
    L = r.shape[0]
    cap = int(max_solves) if max_solves else 3 * L
    counters = {"step_removals": 0}                                                   # lights the step rule took out of P
    x = np.zeros(L)
    inP = np.zeros(L, bool)
    n = 0
    largest = np.fmax.reduce(np.abs(r), initial=0.0)                                  # 1. (a NaN never enters)
    tol = 2.0 ** -40 * largest
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        while True:
            w = r.copy()                                                              # 2.
            for j in np.flatnonzero(inP):
                w = w - A[:, j] * x[j]
            enter, best = -1, tol
            for l in np.flatnonzero(~inP):
                if w[l] > best:
                    enter, best = int(l), w[l]
            if enter < 0:
                return x, 0, n, counters
            inP[enter] = True
            while True:                                                               # 3.
                if n == cap:
                    return x, -1, n, counters
                n += 1
                P = np.flatnonzero(inP)
                s = np.zeros(L)
                if P.size:
                    s[P], bad = _solve_on(A, r, P)
                    if bad:
                        return np.full(L, np.nan), int(P[bad - 1]) + 1, n, counters
                blocked = [int(l) for l in P if not s[l] > 0.0]
                if not blocked:
                    x[P] = s[P]
                    break
                at = blocked[0]
                alpha = x[at] / (x[at] - s[at])
                for l in blocked[1:]:
                    q = x[l] / (x[l] - s[l])
                    if q < alpha:
                        alpha, at = q, l
                d = s[P] - x[P]
                m = alpha * d
                x[P] = x[P] + m
                x[at] = 0.0
                leave = [int(l) for l in P if not x[l] > 0.0]
                x[leave] = 0.0
                inP[leave] = False
                counters["step_removals"] += len(leave)


def solve(gram, rhs, ridge, shared, max_solves=0):
    """-> (rgb (1|B,L,3) f32, info (1|B,3) i32, solves (1|B,3) i32, x (1|B,L,3) f64 before the rounding, counters summed over the
    (rig, channel) systems) in the kernel's order"""
    B, _, L, _ = gram.shape
    assert np.isfinite(gram).all(), "the restatement's domain is a finite gram"
    rigs = 1 if shared else B
    x = np.zeros((rigs, L, 3))
    info = np.zeros((rigs, 3), np.int32)
    solves = np.zeros((rigs, 3), np.int32)
    total = {}
    for rig in range(rigs):
        for c in range(3):
            A, r = system(gram, rhs, ridge, shared, rig, c)
            x[rig, :, c], info[rig, c], solves[rig, c], counters = solve_one(A, r, max_solves)
            for k, v in counters.items():
                total[k] = total.get(k, 0) + v
    return x.astype(F32), info, solves, x, total
