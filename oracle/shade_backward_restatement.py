"""TEST INFRASTRUCTURE -- per-pixel float64 restatement of the shading backward (T8:364-369, 517-522 under autograd) and of
the normals-stencil backward (T8:353-354 under autograd), torch on the CPU.  The companion of march_backward_restatement.py:
per-pixel leaves, so ONE autograd pass per cotangent kind yields per-pixel results and no chain rule is written by hand.

Inputs are the f32 tensors the kernels receive (depth, normals, albedo, light point, ambient, minimum distance); everything is
evaluated in f64 from them, with two exceptions the reference and the kernels share: e = exp(-d) is the F32 value (T8:517 is
evaluated in f32 by both; its derivative is -e), and depth + z_offset is the F32 sum (T8:353).

SHADING (restate_shading).  Per (light, pixel), linear in the cotangents g_w, g_full, g_final, g_rendered[3]:
    albedo[3], normal[3] (on the normal AS PASSED IN, i.e. through F.normalize and its 1e-12 clamp), min_dist, light[3],
    own_depth (= -light[2]: l = C - P), ambient
each as `val` and as `mag`, its MAGNITUDE: the sum of the absolute values of the addends before they cancel.  Addends are kept
apart by giving every USE of an input a leaf of its own and every cotangent kind a backward pass of its own:
  * v / |v| (both normalisations): the numerator and, per output component, the vector under the norm -- the projection
    v_j (v . dv) / |v|^3 is then three addends per component, not their (cancelling) sum;
  * w full = full - q full and (1 - w) amb = amb - w amb with q = 4e / (1 + e)^2 = 1 - w: f32 holds w and 1 - w with an
    ABSOLUTE error of an ulp of 1, so the magnitude of what passes through them counts the 1 and the q (the w) separately;
  * the minimum distance by use (in w full, in (1 - w) amb, in g_w w), the ambient by use (in full, in (1 - w) amb).
The Lambert side max(n.l, 0) is a frozen decision `lit` passed in (default: the f64 dot product's sign); a caller evaluates
the other side by passing the other decision.

STENCIL (restate_stencil).  Per pixel the Jacobian of the returned unit normal (y negated if `negate_y`) in the pixel's nine
replicate-padded neighbour depths, split by use (x, y, z coordinate of the point; d/du, d/dv).  StencilJ.terms(g) gives, for a
gradient g on the returned normal, the eight neighbour terms as (clamped texel index, value) -- offsets that replicate padding
folds onto one texel stay separate terms -- each term's magnitude, and |d term / d g_i|, which carries the f32 rounding of the
gradient the fused routes hand to the stencil.

GATES.  Every bound is a 2^-24 M with M the magnitude.  The f64 routes' multipliers are derived (f64_allowance); the f32 stage
of the fused kernels is gated at 4 x the reference's own f32 noise, measured on the host by
tests/test_shade_backward_restatement_host.py (F32_MEASURED, F32_GATE below).

Only tests/ may import this module.
"""
from dataclasses import dataclass
from typing import Dict, Optional

import torch

import materialised as M

U24 = 2.0 ** -24
KINDS = ("g_w", "g_full", "g_final", "g_r0", "g_r1", "g_r2")
OUTPUTS = ("albedo", "normal", "min_dist", "own_depth", "light", "ambient")
TILE_W, TILE_H = 32, 8                       # render_bwd_single_light_kernel's tile
KINK = 2e-4                                  # near the kink: |n.l| < KINK in f64
SMALL_1ME = 2.0 ** -10                       # pixels with 1 - e below this are left out of the grad_min_dist comparison

# The reference's own f32 autograd (the oracle port's shading lines with f32 per-pixel leaves) against this restatement, worst
# |difference| / (2^-24 magnitude) per output kind over the scenes of tests/shade_scenes.py, near-kink pixels excluded;
# min_dist relative to (1 + 1/(1 - e)) times its magnitude, on pixels with 1 - e >= 2^-10.  Measured on the host by
# tests/test_shade_backward_restatement_host.py::test_reference_f32_noise_fixes_the_gates, which prints them.
F32_MEASURED = {
    "albedo": 3.4,       # measured 3.32 (18 x 66, L = 3)
    "normal": 4.8,       # measured 4.79 (18 x 66, L = 3)
    "min_dist": 2.8,     # measured 2.74 (18 x 66, L = 1)
    "own_depth": 3.7,    # measured 3.69 (8 x 32, L = 1)
    "light": 4.8,        # measured 4.73 (18 x 66, L = 3)
    "ambient": 1.3,      # measured 1.21 (9 x 33, L = 3)
}
# The fused kernels' f32 stage is gated at 4 x the reference's noise: the margin covers another, equally valid f32 operation
# order, FMA contraction and divisions / expf within a couple of ulp of correctly rounded.
F32_GATE = {k: 4.0 * v for k, v in F32_MEASURED.items()}


def f64_allowance(kind: str, one_minus_e: Optional[torch.Tensor] = None):
    """Multiplier a of the f64 routes' bound a 2^-24 M (gcfr_shade_bwd), derived:
      the f32 store: 1 (the light and ambient sums stay f64: 0);
      e = expf(-d) is an f32 library value on both sides, within an ulp each: 2^-22 = 4 x 2^-24 on every term carrying e --
        albedo (through final), normal / light / own depth / ambient (through w);
      min_dist: its factor 4e(1-e)/(1+e)^3 carries e and 1 - e: 2^-22 (1 + 1/(1 - e)) on top, as the march test allows."""
    if kind == "min_dist":
        return 1.0 + 4.0 + 4.0 * (1.0 + 1.0 / one_minus_e)
    return {"albedo": 5.0, "normal": 5.0, "own_depth": 5.0, "light": 4.0, "ambient": 4.0}[kind]


# ---------------------------------------------------------------------------------------------------------------------
# pixel classes
# ---------------------------------------------------------------------------------------------------------------------
IMAGE_CLASSES = ("image corner", "top edge", "bottom edge", "left edge", "right edge", "image interior")
TILE_CLASSES = ("tile corner", "tile edge row", "tile edge column", "tile interior", "partial tile")
KINK_CLASSES = ("lit", "unlit", "near kink")


def pixel_classes(H: int, W: int) -> Dict[str, torch.Tensor]:
    """name -> (H,W) bool: position in the image and in the 32 x 8 tile grid of the single-light kernel."""
    r, c = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None].expand(H, W)
    top, bot, left, right = r == 0, r == H - 1, c == 0, c == W - 1
    corner = (top | bot) & (left | right)
    ty, tx = r % TILE_H, c % TILE_W
    ey, ex = (ty == 0) | (ty == TILE_H - 1), (tx == 0) | (tx == TILE_W - 1)
    partial = ((r // TILE_H) * TILE_H + TILE_H > H) | ((c // TILE_W) * TILE_W + TILE_W > W)
    return {"image corner": corner, "top edge": top & ~corner, "bottom edge": bot & ~corner, "left edge": left & ~corner,
            "right edge": right & ~corner, "image interior": ~(top | bot | left | right),
            "tile corner": ey & ex, "tile edge row": ey & ~ex, "tile edge column": ex & ~ey, "tile interior": ~ey & ~ex,
            "partial tile": partial}


def kink_classes(dot: torch.Tensor) -> Dict[str, torch.Tensor]:
    """dot (L,H,W) f64 -> lit / unlit / near kink, disjoint."""
    near = dot.abs() < KINK
    return {"lit": (dot > 0) & ~near, "unlit": ~(dot > 0) & ~near, "near kink": near}


# ---------------------------------------------------------------------------------------------------------------------
# shading
# ---------------------------------------------------------------------------------------------------------------------
class _Leaves:
    def __init__(self):
        self.items = []          # (output name, leaf, True if the leaf carries an extra per-output-component axis at -2)

    def new(self, out, value, per_component=False):
        t = value.detach().clone().requires_grad_()
        self.items.append((out, t, per_component))
        return t


def _unit(num, under):
    """num (...,3) / max(|under_i|, 1e-12) with under (...,3,3): component i has its own copy of the vector under the norm."""
    return num / torch.linalg.vector_norm(under, dim=-1).clamp_min(1e-12)


@dataclass
class Shaded:
    L: int
    H: int
    W: int
    val: Dict[str, torch.Tensor]        # albedo, normal, light (L,H,W,3); min_dist, own_depth, ambient (L,H,W); f64
    mag: Dict[str, torch.Tensor]        # same shapes: sum of |addend|
    dot: torch.Tensor                   # (L,H,W) f64  n_hat . l_hat
    lit: torch.Tensor                   # (L,H,W) bool the Lambert side used
    one_minus_e: torch.Tensor           # (L,H,W) f64  from the f32 e
    fin: torch.Tensor                   # (L,H,W) f64  final shading


def exp_neg_f32(md32):
    """e = exp(-d) as f32 evaluates it, in f64."""
    return torch.exp(-md32.float()).double()


def restate_shading(depth, normals, albedo, C, amb, md, intensity, cots, lit=None, exp_in_f32=True) -> Shaded:
    """depth (H,W), normals (3,H,W), albedo (3,H,W), C (L,3), amb (L,), md (L,H,W): f32.  cots: dict with any of g_w, g_full,
    g_final (L,H,W) and g_rendered (L,3,H,W), f32 or None.  lit (L,H,W) bool or None.  exp_in_f32=False: e = exp(-d) in f64 (the
    pure-f64 function dense f64 autograd differentiates; host validation only).  See the module docstring."""
    depth, normals, albedo, C, amb, md = [t.detach() for t in (depth, normals, albedo, C, amb, md)]     # (f64 inputs are taken as they are)
    H, W = depth.shape
    L = C.shape[0]
    xx, yy = M.pixel_grids(H, W)
    P = torch.stack([xx.double(), yy.double(), depth.double()], -1)                            # (H,W,3)  T8:356
    l64 = C.double()[:, None, None, :] - P[None]                             # (L,H,W,3)  T8:364
    n64 = normals.double().permute(1, 2, 0)[None].expand(L, H, W, 3)
    amb64 = amb.double()[:, None, None].expand(L, H, W)
    md64 = md.double()
    e_val = exp_neg_f32(md) if exp_in_f32 else torch.exp(-md64)             # the value of e; its derivative is -e_val
    I = float(intensity)
    dot0 = (_unit(n64, n64[..., None, :].expand(L, H, W, 3, 3)) * _unit(l64, l64[..., None, :].expand(L, H, W, 3, 3))).sum(-1)
    lit = (dot0 > 0) if lit is None else lit.bool()
    lv = _Leaves()

    def full():                                                              # T8:364-369, fresh leaves per use
        u = _unit(lv.new("light", l64), lv.new("light", l64[..., None, :].expand(L, H, W, 3, 3), True))
        n = _unit(lv.new("normal", n64), lv.new("normal", n64[..., None, :].expand(L, H, W, 3, 3), True))
        return lv.new("ambient", amb64) + I * torch.where(lit, (n * u).sum(-1), torch.zeros((), dtype=torch.float64))

    def q():                                                                 # 4e / (1 + e)^2 = 1 - w, e the f32 value (T8:517)
        e = e_val * torch.exp(-(lv.new("min_dist", md64) - md64))
        return 4.0 * e / (1.0 + e) ** 2

    full_1, full_q = full(), full()
    fin = (full_1 - q() * full_q) + (lv.new("ambient", amb64) - (1.0 - q()) * lv.new("ambient", amb64))     # T8:518
    w = 1.0 - q()
    alb = lv.new("albedo", albedo.double().permute(1, 2, 0)[None].expand(L, H, W, 3))
    rendered = alb * fin[..., None]                                          # T8:519-522
    get = lambda k: None if cots.get(k) is None else cots[k].detach().double()
    gr = get("g_rendered")
    losses = {"g_w": (get("g_w"), w), "g_full": (get("g_full"), full_1), "g_final": (get("g_final"), fin)}
    for ch in range(3):
        losses["g_r%d" % ch] = (None if gr is None else gr[:, ch], rendered[..., ch])
    shapes = {"albedo": (L, H, W, 3), "normal": (L, H, W, 3), "light": (L, H, W, 3), "min_dist": (L, H, W), "ambient": (L, H, W)}
    val = {k: torch.zeros(s, dtype=torch.float64) for k, s in shapes.items()}
    mag = {k: torch.zeros(s, dtype=torch.float64) for k, s in shapes.items()}
    leaves = [t for _, t, _ in lv.items]
    for kind in KINDS:
        g, out = losses[kind]
        if g is None:
            continue
        grads = torch.autograd.grad((g * out).sum(), leaves, retain_graph=True, allow_unused=True)
        for (name, _, per_component), gl in zip(lv.items, grads):
            if gl is None:
                continue
            val[name] += gl.sum(-2) if per_component else gl
            mag[name] += gl.abs().sum(-2) if per_component else gl.abs()
    val["own_depth"], mag["own_depth"] = -val["light"][..., 2], mag["light"][..., 2]
    return Shaded(L=L, H=H, W=W, val=val, mag=mag, dot=dot0.detach(), lit=lit, one_minus_e=1.0 - exp_neg_f32(md), fin=fin.detach())


# ---------------------------------------------------------------------------------------------------------------------
# normals stencil
# ---------------------------------------------------------------------------------------------------------------------
_KU = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=torch.float64) / 8.0
_KV = _KU.t().contiguous()
OFFSETS = [(dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0)]


@dataclass
class StencilTerms:
    idx: torch.Tensor        # (H,W,8) int64 clamped texel index r W + c, OFFSETS order
    val: torch.Tensor        # (H,W,8) f64
    mag: torch.Tensor        # (H,W,8) f64
    sens: torch.Tensor       # (3,H,W,8) f64  |d term / d g_i|


@dataclass
class StencilJ:
    H: int
    W: int
    idx: torch.Tensor        # (H,W,8)
    J: torch.Tensor          # (3,H,W,8) f64  d(returned normal component i) / d(neighbour depth), summed over its uses
    Jabs: torch.Tensor       # (3,H,W,8) f64  the same with |.| per use
    normal: torch.Tensor     # (H,W,3) f64   the returned unit normal

    def terms(self, g) -> StencilTerms:
        """g (H,W,3): gradient on the returned unit normal."""
        g = g.detach().double().permute(2, 0, 1)[..., None]                  # (3,H,W,1)
        return StencilTerms(idx=self.idx, val=(self.J * g).sum(0), mag=(self.Jabs * g.abs()).sum(0), sens=self.J.abs())


def restate_stencil(depth, fx, fy, cx, cy, z_offset, negate_y=True) -> StencilJ:
    """depth (H,W) f32.  kornia 0.4.1's depth_to_normals (oracle/normals_restatement.py) per pixel, on the pixel's own copy
    of its nine replicate-padded neighbours, each copied once more per use."""
    depth = depth.detach().float()
    H, W = depth.shape
    D = (depth + torch.tensor(z_offset, dtype=torch.float32)).double()       # depth + offset in f32 (T8:353)
    r, c = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None].expand(H, W)
    rr = torch.stack([(r + d).clamp(0, H - 1) for d in (-1, 0, 1)], -1)      # (H,W,3)
    cc = torch.stack([(c + d).clamp(0, W - 1) for d in (-1, 0, 1)], -1)
    nb = D[rr[..., :, None], cc[..., None, :]]                               # (H,W,3,3)
    leaf = nb[..., None, None].expand(H, W, 3, 3, 3, 2).clone().requires_grad_()      # ... x coordinate x (d/du, d/dv)
    ax = ((cc.double() - cx) / fx)[..., None, :].expand(H, W, 3, 3)
    ay = ((rr.double() - cy) / fy)[..., :, None].expand(H, W, 3, 3)
    coef = torch.stack([ax, ay, torch.ones_like(ax)], -1)                    # (H,W,3,3,3)   depth_to_3d
    Pn = coef[..., None] * leaf
    du = (Pn[..., 0] * _KU[..., None]).sum((2, 3))                           # (H,W,3)       spatial_gradient
    dv = (Pn[..., 1] * _KV[..., None]).sum((2, 3))
    n = torch.cross(du, dv, dim=-1)
    n = n / torch.linalg.vector_norm(n, dim=-1, keepdim=True).clamp_min(1e-12)
    out = n * torch.tensor([1.0, -1.0 if negate_y else 1.0, 1.0], dtype=torch.float64)
    keep = [3 * (dr + 1) + (dc + 1) for dr, dc in OFFSETS]
    J, Jabs = [], []
    for i in range(3):
        (g,) = torch.autograd.grad(out[..., i].sum(), leaf, retain_graph=True)
        g = g.reshape(H, W, 9, 6)[:, :, keep]
        J.append(g.sum(-1))
        Jabs.append(g.abs().sum(-1))
    idx = (rr[..., :, None] * W + cc[..., None, :]).reshape(H, W, 9)[:, :, keep]
    return StencilJ(H=H, W=W, idx=idx, J=torch.stack(J), Jabs=torch.stack(Jabs), normal=out.detach())


def scatter_terms(t: StencilTerms, H: int, W: int, delta=None):
    """The terms of every pixel summed per texel: (signed field, sum of |magnitude|, number of non-zero terms,
    sum of sens_i delta_i) each (H,W); delta (H,W,3) or None: the allowance on the gradient handed to the stencil."""
    idx = t.idx.reshape(-1)
    acc = lambda v: torch.zeros(H * W, dtype=torch.float64).index_add_(0, idx, v.reshape(-1)).reshape(H, W)
    prop = torch.zeros(H, W, dtype=torch.float64) if delta is None else acc((t.sens * delta.double().permute(2, 0, 1)[..., None]).sum(0))
    return acc(t.val), acc(t.mag), acc((t.val != 0).double()), prop
