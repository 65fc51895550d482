"""The masked metrics' contract (csrc/gcfr_dataset.hip `gcfr_masked_metrics_u8`, include/gcfr.h), stated in numpy at a precision
above the kernels' (helper module, no tests).  Written from the two MATLAB lines and the kernel file's header comment; it does NOT
import oracle/postprocess_statements.py, so that statement is a second opinion (tests/test_masked_metrics_host.py), not this one.

  MSE_MP.m:24          sum |r m - g m|^2 / (3 sum m)                               r, g, m = uint8 / 255.0
  DSSIM_MP_RGB.m:24-26 (1 - sum(ssimmap .* m3) / sum(m3)) / 2, ssimmap of MATLAB's ssim(A, ref) on the M x N x 3 VOLUME with its
                       documented defaults: Gaussian sigma 1.5, radius ceil(3 sigma) = 5 (11 taps), replicate padding on all three
                       axes -- the channel axis included --, K = (0.01, 0.03), dynamic range 1 for double images.
                       PARITY UNPINNED: MATLAB is not available; nothing here replaces it.

`mse_exact` has no rounding of its own (Python integers, one final rounding to float).  `ssim_map` / `dssim` run in
`dtype`: np.longdouble (x86 extended, eps 1.08e-19: the expected values of the GPU tests) or np.float64 (what a careful double
implementation can reach: the yardstick beside the kernels' deviation in profiles/dataset_metrics_pins.md).

`wrong=` selects a deliberately WRONG variant.  They exist only so that tests/test_masked_metrics_host.py can show that the inputs
of the GPU tests tell each of them from the statement; no kernel is ever compared with one.
  "channel_unfiltered"  (a) the Gaussian runs over rows and columns only
  "reflect"             (b) reflect padding (np.pad "reflect") instead of replicate
  "zero"                (c) zero padding
  "radius4"             (d) 9 taps instead of 11 (sigma stays 1.5)
  "clamp_low_only"      (e) the index is clamped at 0 but not at n - 1: taps beyond the high edge read nothing (zero)
  "weight_m"            (f) MSE weighted by m instead of m^2
  "no_three"            (g) MSE divided by sum m instead of 3 sum m
  "mask_face0"          (h) a per-face mask (B,H,W) read as if it were shared: every face gets face 0's

The inputs of the GPU tests are defined here as well (`cases`, `masks`, `one_hot`, the shape lists), so that the host test can
show on the CPU that these very inputs discriminate."""
from fractions import Fraction

import numpy as np

WRONG_SSIM = ("channel_unfiltered", "reflect", "zero", "radius4", "clamp_low_only")
WRONG_MSE = ("weight_m", "no_three")
WRONG_BATCH = ("mask_face0",)

DSSIM_GATE = dict(rtol=1e-9, atol=1e-12)      # the project's gate for this quantity (tests/test_gpu_dataset.py)
MSE_GATE = dict(rtol=1e-12, atol=0.0)

SEED = 5                                                               # of `cases` and `masks`, in the host and the GPU tests alike
PER_PIXEL_SHAPE = (13, 11)                                             # both axes > 2 radius + 1: an interior pixel clamps nowhere
CLAMP_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 3), (5, 5), (6, 11))       # an axis < 6: one pixel clamps on both sides
WHOLE_SHAPES = ((16, 16), (15, 17), (1, 257))                          # P = 256, 255, and one row over two blocks


# ----------------------------------------------------------------------------------------------------------------------------
# MSE_MP.m:24
# ----------------------------------------------------------------------------------------------------------------------------
def mse_exact(recon, gt, mask, wrong=None):
    """sum (a - g)^2 m^2 / (255^3 * 3 * sum m) over the bytes a, g (H,W,3) and m (H,W): the exact rational, as the nearest float.
    (r m - g m)^2 = (a - g)^2 m^2 / 255^4 and 3 sum m / 255 below it.  An all-zero mask is 0/0: NaN, as in MATLAB."""
    assert recon.dtype == gt.dtype == mask.dtype == np.uint8 and recon.shape == gt.shape == mask.shape + (3,)
    assert wrong is None or wrong in WRONG_MSE
    d2 = ((recon.astype(np.int64) - gt.astype(np.int64)) ** 2).sum(axis=-1)
    m = mask.astype(np.int64)
    sm = int(m.sum())
    if sm == 0:
        return float("nan")
    if wrong == "weight_m":                    # |r - g|^2 m: (a - g)^2 m / 255^3 over 3 sum m / 255
        return float(Fraction(int((d2 * m).sum()), 255 ** 2 * 3 * sm))
    num = int((d2 * m * m).sum())
    return float(Fraction(num, 255 ** 3 * (1 if wrong == "no_three" else 3) * sm))


# ----------------------------------------------------------------------------------------------------------------------------
# DSSIM_MP_RGB.m:24-26
# ----------------------------------------------------------------------------------------------------------------------------
def gauss_taps(dtype=np.longdouble, radius=5):
    d = np.arange(-radius, radius + 1).astype(dtype)
    k = np.exp(-(d * d) / (dtype(2) * dtype(1.5) * dtype(1.5)))
    return k / k.sum()


def _padded(x, axis, r, pad):
    width = [(0, 0)] * x.ndim
    width[axis] = (r, r)
    if pad == "replicate":
        return np.pad(x, width, mode="edge")
    if pad == "reflect":
        return np.pad(x, width, mode="reflect")
    if pad == "zero":
        return np.pad(x, width, mode="constant")
    assert pad == "clamp_low_only"
    width[axis] = (r, 0)
    low = np.pad(x, width, mode="edge")
    width[axis] = (0, r)
    return np.pad(low, width, mode="constant")


def _filtered(x, k, axis, pad):
    r, n = len(k) // 2, x.shape[axis]
    p = _padded(x, axis, r, pad)
    out = np.zeros_like(x)
    for t in range(len(k)):
        out = out + k[t] * np.take(p, np.arange(t, t + n), axis=axis)
    return out


def ssim_map(recon, gt, dtype=np.longdouble, wrong=None):
    """-> the (H,W,3) SSIM map of MATLAB's ssim(recon / 255, gt / 255) on the M x N x 3 volume, in `dtype`"""
    assert recon.dtype == gt.dtype == np.uint8 and recon.shape == gt.shape and recon.ndim == 3 and recon.shape[2] == 3
    assert wrong is None or wrong in WRONG_SSIM
    k = gauss_taps(dtype, 4 if wrong == "radius4" else 5)
    pad = wrong if wrong in ("reflect", "zero", "clamp_low_only") else "replicate"
    axes = (0, 1) if wrong == "channel_unfiltered" else (0, 1, 2)

    def g(x):
        for ax in axes:
            x = _filtered(x, k, ax, pad)
        return x
    A, R = recon.astype(dtype) / dtype(255), gt.astype(dtype) / dtype(255)
    C1, C2 = (dtype(1) / dtype(100)) ** 2, (dtype(3) / dtype(100)) ** 2
    mux, muy = g(A), g(R)
    sx, sy, sxy = g(A * A) - mux * mux, g(R * R) - muy * muy, g(A * R) - mux * muy
    return ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sx + sy + C2))


def dssim_map(recon, gt, dtype=np.longdouble, wrong=None):
    """-> (H,W): (1 - mean over the channels of ssim[p]) / 2, what DSSIM_MP_RGB.m gives under a mask that is non-zero at p alone
    (the mask's value cancels)"""
    s = ssim_map(recon, gt, dtype, wrong)
    return (1 - (s[..., 0] + s[..., 1] + s[..., 2]) / 3) / 2


def dssim(recon, gt, mask, dtype=np.longdouble, wrong=None):
    """(1 - sum(ssimmap .* m3) / sum(m3)) / 2 in `dtype`; an all-zero mask is 0/0: NaN"""
    assert mask.dtype == np.uint8 and mask.shape == recon.shape[:2]
    s = ssim_map(recon, gt, dtype, wrong)
    m = mask.astype(dtype) / dtype(255)
    with np.errstate(invalid="ignore"):
        return (1 - (s * m[..., None]).sum() / (3 * m.sum())) / 2


def batch(recon, gt, mask, dtype=np.longdouble, wrong=None):
    """recon, gt (B,H,W,3), mask (H,W), (1,H,W) or (B,H,W) -> (mse (B,) float64, dssim (B,) `dtype`), as `masked_metrics` takes and
    returns them"""
    B, H, W, _ = recon.shape
    m = mask.reshape(-1, H, W)
    assert m.shape[0] in (1, B)
    pick = (lambda b: 0) if (m.shape[0] == 1 or wrong == "mask_face0") else (lambda b: b)
    w = None if wrong in WRONG_BATCH else wrong
    mse = np.array([mse_exact(recon[b], gt[b], m[pick(b)], w if w in WRONG_MSE else None) for b in range(B)])
    ds = np.array([dssim(recon[b], gt[b], m[pick(b)], dtype, w if w in WRONG_SSIM else None) for b in range(B)], dtype=dtype)
    return mse, ds


# ----------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests
# ----------------------------------------------------------------------------------------------------------------------------
def _ramp(H, W):
    r, c = np.mgrid[0:H, 0:W]
    return np.stack([10 + (200 * c) // max(W - 1, 1),
                     30 + (180 * r) // max(H - 1, 1),
                     5 + (120 * r) // max(H - 1, 1) + (120 * c) // max(W - 1, 1)], axis=-1).astype(np.uint8)       # <= 245: + 1 fits


def cases(H, W, seed):
    """name -> (recon, gt), uint8 (H,W,3): noise, smooth, constant, saturated -- where g(A^2) - mu^2 cancels and where relit faces live"""
    from geomconsistentfr_amd.train import synthetic_batch
    rng = np.random.default_rng(seed)
    full = lambda v: np.full((H, W, 3), v, np.uint8)
    out = {}
    gt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    out["noise"] = (np.clip(gt.astype(int) + rng.integers(-25, 26, gt.shape), 0, 255).astype(np.uint8), gt)
    ramp = _ramp(H, W)
    out["ramp"] = (ramp + np.uint8(1), ramp)
    out["black_black"] = (full(0), full(0))
    out["white_white"] = (full(255), full(255))
    out["black_white"] = (full(0), full(255))
    out["const200_201"] = (full(200), full(201))
    one = ramp.copy()
    one[H // 2, W // 2, 1] ^= 0x80                                  # one byte's top bit, at the centre
    out["one_pixel"] = (one, ramp)
    r, c = np.mgrid[0:H, 0:W]
    chk = np.repeat((((r + c) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    out["checker"] = (chk, 255 - chk)
    face = np.rint(synthetic_batch(1, 4242 + seed, H, W)["images"][0].numpy().astype(np.float64) * 255).astype(np.uint8)
    gain = 0.85 + 0.3 * (c / max(W - 1, 1))[..., None] * np.array([1.0, 0.8, 0.6])          # a smooth, coloured gain
    out["face"] = (np.clip(np.rint(face * gain), 0, 255).astype(np.uint8), face)
    return out


def masks(H, W, seed):
    """name -> (H,W) uint8: full; drawn from all 256 levels; zero on the border ring.  An axis of 1 or 2 pixels is all border: the
    ring is then taken off the other axis alone (and off neither at 2 x 2 and below), so that the mask is never all zero."""
    rng = np.random.default_rng(1000 + seed)
    ring = np.full((H, W), 255, np.uint8)
    if H > 2:
        ring[0], ring[-1] = 0, 0
    if W > 2:
        ring[:, 0], ring[:, -1] = 0, 0
    levels = rng.integers(0, 256, (H, W), dtype=np.uint8)
    levels.flat[0] = 77                                             # (never all zero, whatever the draw)
    return dict(full=np.full((H, W), 255, np.uint8), levels=levels, ring=ring)


CASE_NAMES = ("noise", "ramp", "black_black", "white_white", "black_white", "const200_201", "one_pixel", "checker", "face")


def three_faces(H, W, seed):
    """-> recon, gt (3,H,W,3), masks (3,H,W): three different pairs under three different masks (the mask-form tests' inputs)"""
    c, m = cases(H, W, seed), masks(H, W, seed)
    recon, gt = (np.stack([c[n][i] for n in ("noise", "ramp", "face")]) for i in (0, 1))
    return recon, gt, np.stack([m["full"], m["levels"], m["ring"]])


def one_hot(H, W, value=255):
    """(H W, H, W) uint8: mask p is `value` at pixel p and zero elsewhere"""
    m = np.zeros((H * W, H * W), np.uint8)
    m[np.arange(H * W), np.arange(H * W)] = value
    return m.reshape(H * W, H, W)


def gate(expected, rtol, atol):
    """numpy's allclose bound for `expected`"""
    return atol + rtol * np.abs(np.asarray(expected, dtype=np.float64))
