"""The rig-capture kernels' operation order (csrc/gcfr_light_fit.hip, include/gcfr.h), restated in numpy f64 (helper module, no
tests): the normal equations with every entry summed sequentially over a workgroup's pixels (`np.cumsum(..., axis=0)[-1]` is a
sequential sum) and the workgroups' partials added in ascending order, and the solve -- the faces' systems added in ascending b,
the relative ridge, a Cholesky factorisation whose every dot product runs in ascending m, forward and back substitution.
tests/test_gpu_light_fit.py holds the kernels to it bit for bit; tests/test_light_fit_host.py holds it to numpy's SVD least
squares on the explicit design matrix, so that it is a checked statement and not a second opinion.

The chunk and group geometry are PARAMETERS (`chunk`, `groups`): the tests take them from lighting.light_fit_geometry, the one
place that mirrors the kernel's constants.

Arrays in the C ABI's layouts: final (B,L,H,W) f32, albedo (B,3,H,W) f32, image (B,H,W,3) f32 with nhwc=True else (B,3,H,W),
weight (1|B,H,W) f32 or None, gram (B,3,L,L) f64, rhs (B,3,L) f64, rgb (1|B,L,3) f32, info (1|B,3) i32."""
import numpy as np

from f32_bits import F32, _f

# (B, L, H, W, one weight shared by the faces): the smallest shapes at which each mechanism of the kernels can go wrong
SHAPES = [
    (1, 1, 1, 1, False),                                       # one pixel, one light
    (1, 3, 7, 5, False),                                       # odd H W, misaligned planes
    (2, 5, 21, 37, False),                                     # two faces, several workgroups per face
    (1, 63, 33, 47, False), (1, 64, 33, 47, False),            # the most entries per lane
    (1, 5, 7, 9, False), (1, 5, 8, 8, False), (1, 5, 5, 13, False),      # chunk - 1, chunk, chunk + 1 pixels
    (1, 4, 256, 256, False),                                   # the grid cap binds (512 workgroups) and each walks two chunks
    (3, 4, 9, 11, True),                                       # a (1,H,W) weight shared by three faces
]

# Gates, each FOUR TIMES the largest figure measured on the CPU by tests/test_light_fit_host.py over SHAPES (the restatement
# against numpy's SVD least squares on the explicit design matrix; relative to the largest entry of the reference):
GATE_GRAM = 4 * 1.43e-15
GATE_RHS = 4 * 1.03e-14
GATE_SOLUTION = 4 * 2.06e-14
# ... and the recovery of a known rig from an image synthesised in f32, |x - x_true| / max|x_true| of the f32 solution: 2.36e-7
# at L = 64, 33 x 47, cond(G) = 495 (lstsq itself: 2.22e-7)
GATE_RECOVERY = 4 * 2.36e-7


def make_inputs(seed, B, L, H, W, weight="mask", shared_weight=False, x_true=None):
    """planes independent uniform in [0.05, 1]; weight: "mask" ({0,1}, 70 % ones), "u8" (k / 255 in f32, k uniform), "ones" or None.
    With x_true (B,L,3) the image is f32(a_c sum_l x_true f_l) in f64 rounded once, else uniform like the planes.  image is NHWC."""
    rng = np.random.default_rng(seed)
    u = lambda *s: (0.05 + 0.95 * rng.random(s)).astype(F32)
    final, albedo = u(B, L, H, W), u(B, 3, H, W)
    if x_true is None:
        image = u(B, H, W, 3)
    else:
        sh = np.einsum("blc,blhw->bchw", np.asarray(x_true, np.float64), final.astype(np.float64))
        image = np.ascontiguousarray((albedo.astype(np.float64) * sh).astype(F32).transpose(0, 2, 3, 1))
    Wb = 1 if shared_weight else B
    if weight == "mask":
        w = (rng.random((Wb, H, W)) < 0.7).astype(F32)
    elif weight == "u8":
        w = (rng.integers(0, 256, (Wb, H, W)).astype(F32) / F32(255.0)).astype(F32)
    elif weight == "ones":
        w = np.ones((Wb, H, W), F32)
    else:
        w = None
    return final, albedo, image, w


def _sequential(terms):
    """the sum of terms[0], terms[1], ... along axis 0, one after the other, starting from +0"""
    return np.cumsum(np.concatenate([np.zeros((1,) + terms.shape[1:]), terms], axis=0), axis=0)[-1]


def normal_equations(final, albedo, image, weight, nhwc, chunk, groups):
    """-> (gram (B,3,L,L) f64, rhs (B,3,L) f64) in the kernel's order"""
    _f(final), _f(albedo), _f(image)
    B, L, H, W = final.shape
    HW = H * W
    f = final.reshape(B, L, HW).astype(np.float64)
    a = albedo.reshape(B, 3, HW).astype(np.float64)
    im = (image.reshape(B, HW, 3).transpose(0, 2, 1) if nhwc else image.reshape(B, 3, HW)).astype(np.float64)
    if weight is None:
        w = np.ones((B, HW))
    else:
        w = np.broadcast_to(_f(weight).reshape(weight.shape[0], HW).astype(np.float64), (B, HW))
    n_chunks = (HW + chunk - 1) // chunk
    assert 1 <= groups <= n_chunks
    gram = np.zeros((B, 3, L, L))
    rhs = np.zeros((B, 3, L))
    lower = np.tril(np.ones((L, L), bool))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for c in range(3):
                s = w[b] * a[b, c]
                q, u = s * a[b, c], s * im[b, c]
                G = r = None
                for g in range(groups):
                    idx = np.concatenate([np.arange(j * chunk, min(HW, (j + 1) * chunk)) for j in range(g, n_chunks, groups)])
                    fp = f[b][:, idx].T                                                  # (P,L)
                    pg = _sequential((q[idx, None] * fp)[:, :, None] * fp[:, None, :])    # (q f_l) f_l'
                    pr = _sequential(u[idx, None] * fp)
                    G, r = (pg, pr) if g == 0 else (G + pg, r + pr)
                G = np.where(lower, G, G.T)                                               # the upper triangle: a copy
                gram[b, c], rhs[b, c] = G, r
    return gram, rhs


def solve(gram, rhs, ridge, shared):
    """-> (rgb (1|B,L,3) f32, info (1|B,3) i32, x (1|B,L,3) f64 before the rounding) in the kernel's order"""
    B, _, L, _ = gram.shape
    rigs = 1 if shared else B
    rgb64 = np.full((rigs, L, 3), np.nan)
    info = np.zeros((rigs, 3), np.int32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for rig in range(rigs):
            for c in range(3):
                A, y = gram[rig, c].copy(), rhs[rig, c].copy()
                if shared:
                    for b in range(1, B):
                        A, y = A + gram[b, c], y + rhs[b, c]
                trace = 0.0
                for l in range(L):
                    trace = trace + A[l, l]
                shift = np.float64(ridge) * (trace / np.float64(L))
                for l in range(L):
                    A[l, l] = A[l, l] + shift
                diag = np.zeros(L)
                for k in range(L):
                    s = A[k:, k].copy()
                    for m in range(k):
                        s = s - A[k:, m] * A[k, m]
                    if not (s[0] > 0.0 and s[0] < np.inf):
                        info[rig, c] = k + 1
                        break
                    diag[k] = np.sqrt(s[0])
                    A[k + 1:, k] = s[1:] / diag[k]
                if info[rig, c]:
                    continue
                z = np.zeros(L)
                for k in range(L):
                    z[k] = y[k] / diag[k]
                    y[k + 1:] = y[k + 1:] - A[k + 1:, k] * z[k]
                x = np.zeros(L)
                for k in range(L - 1, -1, -1):
                    x[k] = z[k] / diag[k]
                    z[:k] = z[:k] - A[k, :k] * x[k]
                rgb64[rig, :, c] = x
        return rgb64.astype(F32), info, rgb64


def design_lstsq(final, albedo, image, weight, nhwc, shared=False):
    """the INDEPENDENT statement: per (face | all faces, channel) numpy's SVD least squares on the explicit weighted design matrix,
    columns sqrt(w) a_c f_l, target sqrt(w) I_c.  -> (x (1|B,L,3) f64, gram (B,3,L,L) = D^T D, rhs (B,3,L) = D^T t, cond (1|B,3))"""
    B, L, H, W = final.shape
    HW = H * W
    f = final.reshape(B, L, HW).astype(np.float64)
    a = albedo.reshape(B, 3, HW).astype(np.float64)
    im = (image.reshape(B, HW, 3).transpose(0, 2, 1) if nhwc else image.reshape(B, 3, HW)).astype(np.float64)
    w = np.ones((B, HW)) if weight is None else np.broadcast_to(weight.reshape(weight.shape[0], HW).astype(np.float64), (B, HW))
    D = np.sqrt(w)[:, None, :, None] * a[:, :, :, None] * f.transpose(0, 2, 1)[:, None]          # (B,3,HW,L)
    t = np.sqrt(w)[:, None, :] * im                                                              # (B,3,HW)
    gram = np.einsum("bcpl,bcpm->bclm", D, D)
    rhs = np.einsum("bcpl,bcp->bcl", D, t)
    if shared:
        D, t = D.transpose(1, 0, 2, 3).reshape(1, 3, B * HW, L), t.transpose(1, 0, 2).reshape(1, 3, B * HW)
    x = np.zeros((D.shape[0], L, 3))
    cond = np.zeros((D.shape[0], 3))
    for r in range(D.shape[0]):
        for c in range(3):
            x[r, :, c], _res, _rank, sv = np.linalg.lstsq(D[r, c], t[r, c], rcond=None)
            cond[r, c] = (sv[0] / sv[-1]) ** 2 if sv[-1] > 0 else np.inf
    return x, gram, rhs, cond
