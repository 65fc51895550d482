"""TEST INFRASTRUCTURE -- per-pixel float64 restatement of the ray march's backward, torch on the CPU.

What it is.  For ONE image and ONE light it evaluates T8:378-509 at a given sample k[r, c] of every pixel in float64 with
every DECISION frozen, and lets torch autograd differentiate that.  The decisions -- the nine-way end-point branch, the
arithmetic select of the corner cases, the clamp, floor / ceil, the -1 index wrap and the argmin k itself -- are
piecewise constant: they are computed from the float32 forward (the same separately-rounded f32 ops as
materialised._end_points) and enter the f64 graph as constants.

f32 values under f64 derivatives.  A pure-f64 forward is NOT the reference's function: its end point differs from the
f32 one by an ulp and floor / ceil then pick another texel (the distance is wrong by tens of per cent on such pixels).
Both the reference's autograd and the kernels linearise at the f32 forward's values.  So every intermediate the reference
holds in f32 enters the graph as  v64 + (v32.double() - v64).detach():  the value is the f32 one, the derivative is the
f64 expression's.  These are: C_x - x + 1e-4, the slope m, m + 1e-4, the intercept ic, both end-point candidates, the
end point E, E - start, the point A after .float(), BA and BC.  The two f32 divisions (m and the y candidate) are
differentiated in their divisor as -quotient / divisor with the F32 quotient, as torch's division backward and the kernels
both do (_Snap.div).

What stays in f64.  The cross product BA x BC, num, den and their quotient are evaluated in f64 FROM the f32 BA / BC:
that is the function the HIP kernels differentiate (gcfr_backward.hip, shadow_bwd_pixel).  The reference's own autograd
forms the cross product, the two sums of squares and the square roots in f32, so its forward value and its gradient differ
from this restatement where the distance is small (|BA x BC|^2 next to the 1e-4 under the root, cancellation in the
products): tests/test_march_backward_restatement_host.py measures by how much.

Not differentiated.  LX, LY of the light-inside-the-image case are Python floats in the reference (T8:380-381): no
gradient.  A clamped end-point coordinate (T8:462-465, masked assignment) carries none.

Leaves.  Pixels do not share any leaf, so ONE autograd pass gives per-pixel results:
  * the light point is a per-pixel leaf (H,W,3), with separate copies for its three uses -- in BC, in the slope
    (C_x - x + 1e-4 and m) and in the intercept ic = C_y - m C_x.  Their gradients sum to the pixel's gC; the sum of
    their absolute values is the pixel's light-gradient magnitude (what a rounding allowance scales with);
  * the four bilinear corner depths are a per-pixel leaf (H,W,4): d d/d corner = d d/d zA * wx * wy;
  * the pixel's own depth (B_z) is a separate per-pixel leaf.

Only tests/ may import this module.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

import materialised as M

CLASS_NAMES = ("kind0", "kind1", "kind2", "corner_chose_y", "corner_chose_x", "clamp_x", "clamp_y", "wrap_col",
               "wrap_row", "own_corner", "k_first", "k_last")
TERM_NAMES = ("corner UL", "corner UR", "corner LL", "corner LR", "own depth")
LIGHT_USES = ("BC", "slope m", "ic")


class _Snap:
    """v64 -> v64 + (v32 - v64).detach().  Records the offsets on the first pass; a replay (finite differences of the
    frozen forward) reuses them, so the replayed function is exactly the one autograd differentiated."""

    def __init__(self, offsets: Optional[List[torch.Tensor]] = None):
        self.record = offsets is None
        self.offsets = [] if offsets is None else offsets
        self.i = 0

    def __call__(self, v64, v32=None):
        if self.record:
            self.offsets.append((v32.double() - v64).detach())
        off = self.offsets[self.i]
        self.i += 1
        return v64 + off

    def freeze(self, v):
        """v as a constant: its own value on the first pass, that same value on a replay."""
        if self.record:
            self.offsets.append(v.detach())
        c = self.offsets[self.i]
        self.i += 1
        return c

    def div(self, a, b, q32):
        """a / b held in f32 (q32).  Its derivative in b is -q32 / b -- the f32 quotient over the divisor, which is what
        torch's division backward and the kernels both form -- not -a / b^2 from the unrounded quotient: written as
        (a - q32 (b - b0)) / b0 with b0 = b frozen, the same value and that derivative."""
        b0 = self.freeze(b)
        q = q32.double()
        return self((a - q * (b - b0)) / b0, q32)


@dataclass
class Restated:
    H: int
    W: int
    N: int
    live: torch.Tensor                  # (H,W) bool: k >= 0
    d: torch.Tensor                     # (H,W) f64, the restated distance at sample k
    gC: torch.Tensor                    # (H,W,3) f64, the pixel's light-point gradient (times g)
    gC_uses: torch.Tensor               # (3,H,W,3): by use, LIGHT_USES
    gC_mag: torch.Tensor                # (H,W,3): sum over the uses of |.|
    term_idx: torch.Tensor              # (H,W,5) int64 flat texel index r*W + c, TERM_NAMES
    term_val: torch.Tensor              # (H,W,5) f64 (times g)
    classes: Dict[str, torch.Tensor]    # name -> (H,W) bool, live pixels only
    frozen: dict = field(repr=False, default_factory=dict)

    def scatter(self, pixels: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None):
        """The five depth terms of the pixels in `pixels` ((H,W) bool, default: all live ones) summed per texel:
        (signed field, sum of |term| [* weight of the term's pixel], number of non-zero terms), each (H,W)."""
        sel = self.live if pixels is None else (pixels & self.live)
        idx = self.term_idx[sel].reshape(-1)
        val = self.term_val[sel].reshape(-1)
        w = torch.ones_like(self.d) if weight is None else weight.double()
        wv = w[sel][:, None].expand(-1, 5).reshape(-1)
        P = self.H * self.W
        signed = torch.zeros(P, dtype=torch.float64).index_add_(0, idx, val)
        absum = torch.zeros(P, dtype=torch.float64).index_add_(0, idx, val.abs() * wv)
        count = torch.zeros(P, dtype=torch.float64).index_add_(0, idx, (val != 0).double())
        return signed.reshape(self.H, self.W), absum.reshape(self.H, self.W), count.reshape(self.H, self.W)

    def times(self, g):
        """The same restatement under the upstream gradient g (H,W) instead of 1 (the results are linear in it)."""
        import dataclasses
        g = g.detach().double()
        return dataclasses.replace(self, gC=self.gC * g[..., None], gC_uses=self.gC_uses * g[None, ..., None],
                                   gC_mag=self.gC_mag * g.abs()[..., None], term_val=self.term_val * g[..., None])

    def light(self, pixels: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None):
        """(sum of gC (3,), sum of the light-gradient magnitudes [* weight] (3,)) over `pixels`."""
        sel = self.live if pixels is None else (pixels & self.live)
        w = torch.ones_like(self.d) if weight is None else weight.double()
        return self.gC[sel].sum(0), (self.gC_mag[sel] * w[sel][:, None]).sum(0)

    def forward(self, depth64: Optional[torch.Tensor] = None, C64: Optional[torch.Tensor] = None):
        """The frozen f64 forward at another depth image (H,W) f64 and / or light point (3,) f64: same decisions, same
        f32 offsets.  What central differences are taken of."""
        f = self.frozen
        Z = f["depth64"] if depth64 is None else depth64
        C = f["C64"] if C64 is None else C64
        Cp = C.expand(self.H, self.W, 3)
        Zc = Z.reshape(-1)[self.term_idx[..., :4]]
        return _forward(f, Zc, Z, Cp, Cp, Cp, _Snap(f["offsets"]))


def _decisions(C, k, p, H, W):
    """The f32 forward of T8:378-467 and everything piecewise constant at sample k."""
    xx, yy = M.pixel_grids(H, W)
    x_lo, x_hi = -(W / 2.0), (W - W / 2.0 - 1)
    y_lo, y_hi = 1 - (H / 2.0), H / 2.0
    pden32 = C[0] - xx + 0.0001
    m32 = (C[1] - yy) / pden32
    q32 = m32 + 0.0001
    ic32 = C[1] - m32 * C[0]
    LX, LY = float(C[0]), float(C[1])
    xin, yin = x_lo <= LX <= x_hi, y_lo <= LY <= y_hi
    one = torch.ones_like(xx)
    xb = x_lo if LX < x_lo else x_hi
    yb = y_lo if LY < y_lo else y_hi
    cand_x = (xb * one, m32 * (xb * one) + ic32)              # "try x = xb"
    cand_y = ((yb * one - ic32) / q32, yb * one)              # "try y = yb"
    corner = not xin and not yin
    if xin and yin:
        kind = torch.zeros_like(k)
    elif xin:
        kind = torch.full_like(k, 2)
    elif yin:
        kind = torch.full_like(k, 1)
    else:
        hit = (cand_y[0] >= x_lo) & (cand_y[0] <= x_hi)
        kind = torch.where(hit, 2, 1).to(k.dtype)
    inside = (LX * one, LY * one)
    raw = tuple(torch.where(kind == 0, i_, torch.where(kind == 1, a, b)) for i_, a, b in zip(inside, cand_x, cand_y))
    clamp_x = (raw[0] < x_lo) | (raw[0] > x_hi)
    clamp_y = (raw[1] < y_lo) | (raw[1] > y_hi)
    E32 = (raw[0].clamp(x_lo, x_hi), raw[1].clamp(y_lo, y_hi))
    dx32, dy32 = E32[0] - xx, E32[1] - yy
    t = torch.from_numpy(p.sample_table())[k.clamp(min=0)]
    px, py = xx.double() + t * dx32.double(), yy.double() + t * dy32.double()
    ux, uy = (px + W / 2.0) - 0.0001, (H / 2.0 - py) - 0.0001
    fx, gx, fy, gy = torch.floor(ux), torch.ceil(ux), torch.floor(uy), torch.ceil(uy)
    return dict(H=H, W=W, xx=xx, yy=yy, xb=xb, yb=yb, pden32=pden32, m32=m32, q32=q32, ic32=ic32, cand_x32=cand_x,
                cand_y32=cand_y, kind=kind, corner=corner, clamp_x=clamp_x, clamp_y=clamp_y, E32=E32, dx32=dx32, dy32=dy32,
                t=t, fx=fx, gx=gx, fy=fy, gy=gy)


def _forward(f, Zc, Zown, C_bc, C_m, C_ic, sn):
    """d (H,W) f64 at the frozen decisions `f`.  Zc (H,W,4) corner depths UL, UR, LL, LR; Zown (H,W); the light point's
    three copies (H,W,3) each; sn: the _Snap."""
    H, W = f["H"], f["W"]
    xx, yy = f["xx"].double(), f["yy"].double()
    pden = sn(C_m[..., 0] - xx + 0.0001, f["pden32"])                         # T8:378
    m = sn.div(C_m[..., 1] - yy, pden, f["m32"])
    ic = sn(C_ic[..., 1] - m * C_ic[..., 0], f["ic32"])                       # T8:379
    q = sn(m + 0.0001, f["q32"])
    cxy = sn(m * f["xb"] + ic, f["cand_x32"][1])                              # x candidate (xb, m xb + ic)
    cyx = sn.div(f["yb"] - ic, q, f["cand_y32"][0])                          # y candidate ((yb - ic)/(m + 1e-4), yb)
    kind = f["kind"]
    E32x, E32y = f["E32"][0].double(), f["E32"][1].double()
    Ex = torch.where((kind == 2) & ~f["clamp_x"], cyx, E32x)                  # constants: kind 0, kind 1's xb, the clamp
    Ey = torch.where((kind == 1) & ~f["clamp_y"], cxy, E32y)
    Ex, Ey = sn(Ex, f["E32"][0]), sn(Ey, f["E32"][1])
    dx, dy = sn(Ex - xx, f["dx32"]), sn(Ey - yy, f["dy32"])                   # T8:467
    px, py = xx + f["t"] * dx, yy + f["t"] * dy                               # f64 from here, T8:468-480
    ux, uy = (px + W / 2.0) - 0.0001, (H / 2.0 - py) - 0.0001
    wx0, wx1, wy0, wy1 = f["gx"] - ux, ux - f["fx"], f["gy"] - uy, uy - f["fy"]
    up = Zc[..., 0] * wx0 + Zc[..., 1] * wx1                                  # T8:492-494
    low = Zc[..., 2] * wx0 + Zc[..., 3] * wx1
    zA = up * wy0 + low * wy1
    A = [ux - W / 2.0, H / 2.0 - uy, zA]
    A = [sn(a, a.detach().float() if sn.record else None) for a in A]         # T8:497-502 .float()
    Bp = [xx, yy, Zown]
    B32 = f.get("B32")
    BA = [sn(a - b, (a.detach().float() - b32) if sn.record else None) for a, b, b32 in zip(A, Bp, B32)]
    BC = [sn(C_bc[..., i] - b, (f["C32"][i] - b32) if sn.record else None) for i, (b, b32) in enumerate(zip(Bp, B32))]
    X = [BA[1] * BC[2] - BA[2] * BC[1], BA[2] * BC[0] - BA[0] * BC[2], BA[0] * BC[1] - BA[1] * BC[0]]
    num = torch.sqrt(X[0] ** 2 + X[1] ** 2 + X[2] ** 2 + 1e-4)
    den = torch.sqrt(BC[0] ** 2 + BC[1] ** 2 + BC[2] ** 2 + 1e-4)
    if sn.record:
        f["BA"], f["BC"] = BA, BC
    return num / den


def cross_product_f32_bound(r: "Restated"):
    """(H,W) bound on the relative difference between the reference's f32 evaluation of T8:508-509 and the f64 one, both
    from the same f32 BA / BC (u = 2^-24):
      X_i = a b - c d in f32: two products and a difference, |dX_i| <= 2u (|a b| + |c d|) =: e_i to first order;
      S = sum X_i^2 + 1e-4: 2 |X_i| e_i absolute, plus three squares and three additions of positive terms: 4u relative;
      sqrt halves both and adds u:  rel(num) <= sum |X_i| e_i / S + 3u;  den likewise without the e_i: 3u;  the division u.
    Total  sum_i |X_i| e_i / S + 7u."""
    u = 2.0 ** -24
    BA, BC = [v.detach() for v in r.frozen["BA"]], [v.detach() for v in r.frozen["BC"]]
    tot, S = 0.0, 1e-4
    for a, b in ((1, 2), (2, 0), (0, 1)):
        X = BA[a] * BC[b] - BA[b] * BC[a]
        tot = tot + X.abs() * 2 * u * ((BA[a] * BC[b]).abs() + (BA[b] * BC[a]).abs())
        S = S + X * X
    return tot / S + 7 * u


def restate(depth, C, k, p: M.BlockParams, g=None, tail: str = "f64") -> Restated:
    """depth (H,W) f32, C (3,) f32 light point, k (H,W) integer sample index per pixel (< 0: no gradient),
    g (H,W) optional upstream gradient on the distance (any float dtype; default 1).  See the module docstring.
    tail="f32": the cross product, the sums of squares, the roots and the quotient (T8:508-509) are evaluated and
    differentiated in f32 torch ops as the reference does, everything in front of them as above -- the hybrid that tells
    how much of a difference to the reference's autograd is that f32 tail's."""
    depth, C = depth.detach().float(), C.detach().float()
    H, W = depth.shape
    k = k.long()
    live = k >= 0
    f = _decisions(C, k, p, H, W)
    f["C32"] = C
    f["B32"] = [f["xx"], f["yy"], depth]
    f["depth64"], f["C64"] = depth.double(), C.double()
    wrap = lambda v, n: torch.where(v < 0, v + n, v).long()
    fxl, gxl, fyl, gyl = wrap(f["fx"], W), f["gx"].long(), wrap(f["fy"], H), f["gy"].long()
    rows, cols = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None].expand(H, W)
    term_idx = torch.stack([fyl * W + fxl, fyl * W + gxl, gyl * W + fxl, gyl * W + gxl, rows * W + cols], -1)

    Zc = f["depth64"].reshape(-1)[term_idx[..., :4]].clone().requires_grad_()
    Zown = f["depth64"].clone().requires_grad_()
    Cs = [f["C64"].expand(H, W, 3).clone().requires_grad_() for _ in range(3)]
    sn = _Snap()
    d = _forward(f, Zc, Zown, Cs[0], Cs[1], Cs[2], sn)
    f["offsets"] = sn.offsets
    if tail == "f32":
        BA, BC = f["BA"], f["BC"]
        ba, bc = [torch.stack([v.detach().float() for v in vs]).requires_grad_() for vs in (BA, BC)]
        X = torch.cross(ba, bc, dim=0)
        d = torch.sqrt(torch.sum(X * X, dim=0) + 0.0001) / torch.sqrt(torch.sum(bc * bc, dim=0) + 0.0001)
        d.sum().backward()
        torch.autograd.backward(BA + BC, [v.double() for v in ba.grad] + [v.double() for v in bc.grad])
    else:
        d.sum().backward()
    gg = (torch.ones_like(d) if g is None else g.detach().double()) * live
    term_val = torch.cat([Zc.grad, Zown.grad[..., None]], -1) * gg[..., None]
    uses = torch.stack([c.grad for c in Cs]) * gg[None, ..., None]

    kind = f["kind"]
    own = (term_idx[..., :4] == term_idx[..., 4:]).any(-1)
    cls = dict(kind0=kind == 0, kind1=kind == 1, kind2=kind == 2,
               corner_chose_y=(kind == 2) if f["corner"] else torch.zeros_like(live),
               corner_chose_x=(kind == 1) if f["corner"] else torch.zeros_like(live),
               clamp_x=f["clamp_x"], clamp_y=f["clamp_y"], wrap_col=f["fx"] < 0, wrap_row=f["fy"] < 0, own_corner=own,
               k_first=k == 0, k_last=k == p.n_samples - 1)
    cls = {n: (v & live) for n, v in cls.items()}
    return Restated(H=H, W=W, N=p.n_samples, live=live, d=d.detach().double(), gC=uses.sum(0), gC_uses=uses, gC_mag=uses.abs().sum(0),
                    term_idx=term_idx, term_val=term_val, classes=cls, frozen=f)


def transfer_gradient(min_dist32, g_w):
    """dLoss/d minimum_distance from dLoss/d shadow weight, w = 1 - 4e/(1+e)^2, e = exp(-d) (T8:517), in f64 from the
    f32 minimum distance: g_w 4e(1-e)/(1+e)^3.  Returns (gradient, 1 - e)."""
    e = torch.exp(-min_dist32.double())
    return g_w.double() * 4.0 * e * (1.0 - e) / (1.0 + e) ** 3, 1.0 - e


def fused_route_pixels(one_minus_e, live, threshold=2.0 ** -10, cap=0.01):
    """The pixels the fused routes are compared on, and their extra relative allowance.  The fused kernels evaluate the
    transfer derivative in f32, where 1 - e carries an absolute error of an ulp of e (2^-24 next to 1): relative allowance
    2^-22 (1 + 1/(1 - e)).  Pixels with 1 - e < threshold are left out, but never more than `cap` of the live pixels: where
    more fall under the threshold (a first sample lies right beside its own pixel: d of 1e-5 ... 1e-3), the ones with
    the smallest 1 - e go and the others are compared under their -- correspondingly wide -- allowance.
    -> (keep (H,W) bool, allowance (H,W) f64, number of live pixels under the threshold)"""
    small = live & (one_minus_e < threshold)
    n_cap = int(cap * int(live.sum()))
    order = torch.argsort(torch.where(small, one_minus_e, torch.full_like(one_minus_e, float("inf"))).reshape(-1))[:n_cap]
    out = torch.zeros(live.numel(), dtype=torch.bool)
    out[order] = True
    out = out.reshape(live.shape) & small
    return live & ~out, 2.0 ** -22 * (1.0 + 1.0 / one_minus_e), int(small.sum())
