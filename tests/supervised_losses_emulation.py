"""The supervised-loss head's operation order (csrc/gcfr_supervised_losses.hip, include/gcfr.h), restated in numpy: every f32
operation of the kernels as one numpy float32 operation in the same order, the sums in f64, the scalar formulas in f32, and the
gradient expressions.  tests/test_gpu_supervised_losses.py holds the kernels to it -- gradients bit for bit, the five terms to one
f32 ulp (the association of the f64 sums is the only freedom) -- and tests/test_supervised_losses_host.py holds it to the f64 torch
restatement of `train.generator_losses`, so that it is a checked statement and not a second opinion.

Arrays are float32 in the C ABI's layouts: depth, gt_depth, mask, gt_albedo, mask_fill (B,H,W); albedo (B,3,H,W); unit_light (B,3);
ambient (B,); lightings (B,4); logits any shape or None."""
import numpy as np

from f32_bits import F32, _f, bit_equal, ulps  # noqa: F401  (bit_equal, ulps: for the tests)

THIRD = F32(1.0) / F32(3.0)
TERMS = ("depth", "ambient", "lighting", "albedo", "generator")


def sgn(d):
    """sign(0) = 0 and sign(NaN) = 0, as +0.0"""
    _f(d)
    return np.where(d > 0, F32(1.0), np.where(d < 0, F32(-1.0), F32(0.0))).astype(F32)


def exp_plain(x):
    """the kernel's e^x: clamp to [-87, 88], n = rint(x log2 e), r = (x - n ln2_hi) - n ln2_lo, Cephes' polynomial, ldexp"""
    x = _f(np.asarray(x))
    x = np.where(x < F32(-87.0), F32(-87.0), x)
    x = np.where(x > F32(88.0), F32(88.0), x)
    n = np.rint(_f(x * F32(1.44269504)))
    r = _f(_f(x - _f(n * F32(0.693359375))) - _f(n * F32(-2.12194440e-4)))
    p = np.full(x.shape, F32(1.9875691500e-4), F32)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = _f(_f(p * r) + F32(c))
    y = _f(_f(_f(p * _f(r * r)) + r) + F32(1.0))
    return _f(np.ldexp(y, n.astype(np.int32)).astype(F32))


def _diffs(depth, gt_depth, mask, albedo, gt_albedo, mask_fill):
    for a in (depth, gt_depth, mask, albedo, gt_albedo, mask_fill):
        _f(a)
    assert depth.ndim == 3 and albedo.shape == (depth.shape[0], 3) + depth.shape[1:]
    assert gt_depth.shape == mask.shape == gt_albedo.shape == mask_fill.shape == depth.shape
    dd = _f(_f(depth * mask) - _f(gt_depth * mask))                                   # T8:634
    grey = _f(_f(_f(albedo[:, 0] + albedo[:, 1]) + albedo[:, 2]) * THIRD)              # T8:638
    da = _f(_f(grey * mask_fill) - _f(gt_albedo * mask_fill))                          # T8:639
    return dd, da


def softplus_neg_f64(logits):
    x = _f(np.asarray(logits)).astype(np.float64)
    return np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))                          # -log sigmoid(x)


def forward(depth, gt_depth, mask, albedo, gt_albedo, mask_fill, unit_light, ambient, lightings, logits=None):
    """-> terms (5,) f32 in TERMS' order, sums (4,) f64 = S_depth, M, S_albedo, M_fill"""
    dd, da = _diffs(depth, gt_depth, mask, albedo, gt_albedo, mask_fill)
    u, amb, l = _f(unit_light), _f(ambient), _f(lightings)
    B = depth.shape[0]
    assert u.shape == (B, 3) and amb.shape == (B,) and l.shape == (B, 4)
    f64sum = lambda a: np.float64(a.astype(np.float64).sum())
    S, M, Sa, Mf = f64sum(np.abs(dd)), f64sum(mask), f64sum(np.abs(da)), f64sum(mask_fill)
    A = f64sum(np.abs(_f(amb - l[:, 0])))                                              # T8:635
    dot = _f(_f(_f(u[:, 0] * l[:, 1]) + _f(u[:, 1] * l[:, 2])) + _f(u[:, 2] * l[:, 3]))  # T8:636
    Lt = f64sum(_f(F32(1.0) - dot))
    fB = F32(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = [F32(S) / F32(M), F32(2.5) * (F32(A) / fB), F32(Lt) / fB, F32(5.0) * (F32(Sa) / F32(Mf))]
    if logits is None:
        terms.append(F32(0.0))
    else:
        n = int(np.asarray(logits).size)
        terms.append(F32(0.01) * (F32(np.float64(softplus_neg_f64(logits).sum())) / F32(n)))     # T8:642
    return _f(np.array(terms, F32)), np.array([S, M, Sa, Mf], np.float64)


def backward(depth, gt_depth, mask, albedo, gt_albedo, mask_fill, ambient, lightings, logits, sums, g):
    """`g`: five float32 scalars or None each (None: zeros for that term) -> dict of float32 gradients"""
    dd, da = _diffs(depth, gt_depth, mask, albedo, gt_albedo, mask_fill)
    amb, l = _f(ambient), _f(lightings)
    B = depth.shape[0]
    for v in g:
        assert v is None or (isinstance(v, np.generic) and v.dtype == np.float32)
    g_d, g_amb, g_l, g_a, g_g = g
    M, Mf, fB = F32(sums[1]), F32(sums[3]), F32(B)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if g_d is None:
            out["depth"] = np.zeros(depth.shape, F32)
        else:
            out["depth"] = _f(_f((g_d / M) * sgn(dd)) * mask)
        if g_a is None:
            ga = np.zeros(depth.shape, F32)
        else:
            ga = _f(_f(_f(((g_a * F32(5.0)) / Mf) * sgn(da)) * mask_fill) * THIRD)
        out["albedo"] = np.ascontiguousarray(np.broadcast_to(ga[:, None], albedo.shape))
        out["ambient"] = np.zeros(B, F32) if g_amb is None else _f(((g_amb * F32(2.5)) / fB) * sgn(_f(amb - l[:, 0])))
        out["unit_light"] = np.zeros((B, 3), F32) if g_l is None else _f((-(g_l / fB)) * l[:, 1:4])
        if logits is not None:
            x = _f(np.asarray(logits))
            if g_g is None:
                out["logits"] = np.zeros(x.shape, F32)
            else:
                s = (g_g * F32(0.01)) / F32(x.size)
                out["logits"] = _f(s * -(F32(1.0) / _f(F32(1.0) + exp_plain(x))))
    return {k: _f(np.ascontiguousarray(v)) for k, v in out.items()}
