"""The shading backward and the normals-stencil backward pinned PER PIXEL and PER TEXEL to oracle/shade_backward_restatement.py,
the f64 restatement validated on the host by tests/test_shade_backward_restatement_host.py.  Scenes: tests/shade_scenes.py.
The C ABI is called directly; every buffer's shape, dtype and contiguity is checked first.

  (a) gcfr_shade_bwd (f64 chain rule): dense cotangents, L = 1 and 3, each upstream pointer alone and all four together; every
      per-pixel output under its own bound; per-pixel light / ambient gradients from a one-hot launch at the two smallest shapes;
  (b) gcfr_normals_bwd: B = H W one-hot planes, both negate_y: exactly zero outside the clamped 3 x 3 neighbourhood, every texel
      inside its bound;
  (c) gcfr_render_bwd with argmin = -1 everywhere (the march backward, which tests/test_gpu_march_backward_pixels.py owns,
      contributes nothing): one-hot planes through g_rendered + g_final + g_full and through g_normals_out alone, L = 1
      (render_bwd_single_light_kernel) and L = 2 (render_bwd_multi_light_kernel), normals given and NULL; dense cotangents with
      B = 2 at L = 1 and L = 3;
  (d) composition: 48 x 72 of tests/march_scenes.py with the real forward's argmin and minimum distance, every upstream gradient
      dense, L = 1 and L = 10: grad_depth per texel against the sum of the march restatement's field and this one's;
  (e) buffer contracts: "=" outputs are pre-filled with NaN in EVERY launch of this file (each element must be overwritten, the
      pixels of partial tiles and those without any upstream gradient included); "+=" outputs are pre-filled with an exactly
      representable pattern in a test of their own and the increment is compared.

Gates -- every bound is a 2^-24 M with M the restatement's magnitude (the sum of |addend| before cancellation):
  f64 routes: a = shade_backward_restatement.f64_allowance (derived: the f32 store, 2^-22 for the f32 library e = expf(-d), the
      march test's 2^-22 (1 + 1/(1 - e)) on the transfer derivative; pixels with 1 - e < 2^-10 are left out of grad_min_dist, at
      most 1 %, and the planted d = 0 must give exactly zero);
  atomics into grad_depth: (n + 4) 2^-23 S per texel, n terms of summed magnitude S landing there, as in the march test;
  f32 stage of the fused kernels: a = F32_GATE = 4 x the reference's own f32 noise measured on the host; the f32 sum over L
      lights adds (L - 1); the gradient handed to the stencil carries that allowance delta_i into every texel as
      sum_i |d term / d g_i| delta_i;
  near the kink of max(n.l, 0) (|n.l| < 2e-4 in f64) the forward's side is not observable: a pixel passes if it is inside the
      bound of EITHER side (one-hot launches), resp. the difference of the two sides is added to the bound (dense launches); at
      most 1 % of a scene's pixels are left to this rule (asserted here as on the host).

The worst error / bound per route and class on an MI355X is recorded in DESIGN.md ("How the shading and the stencil backward are
pinned")."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_backward_restatement as R  # noqa: E402
import shade_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

U24, U23 = 2.0 ** -24, 2.0 ** -23
ALL_SHAPES = S.FUSED_SHAPES + S.ODD_SHAPES
F32, F64 = torch.float32, torch.float64
_SCENES, _MISC = {}, {}


def dev():
    return torch.device("cuda:0")


def _checked(t, shape, dtype):
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == tuple(shape), (tuple(t.shape), shape, t.dtype)
    return t.data_ptr()


def _opt(t, shape, dtype=F32):
    return None if t is None else _checked(t, shape, dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _camera(cam, H, W):
    return (cam[0], cam[0], W / 2.0, H / 2.0, cam[1])


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def normals_fwd(depth, cam, negate_y=1):
    from geomconsistentfr_amd import _lib
    B, H, W = depth.shape
    out = torch.full((B, 3, H, W), float("nan"), dtype=F32, device=dev())
    k = _camera(cam, H, W)
    _lib.check(_lib.load().gcfr_normals_fwd(_checked(depth, (B, H, W), F32), B, H, W, k[0], k[1], k[2], k[3], k[4], negate_y,
                                            out.data_ptr(), _stream()), "gcfr_normals_fwd")
    return out


def normals_bwd(g, depth, cam, negate_y, gd=None):
    from geomconsistentfr_amd import _lib
    B, H, W = depth.shape
    gd = torch.zeros((B, H, W), dtype=F32, device=dev()) if gd is None else gd
    k = _camera(cam, H, W)
    _lib.check(_lib.load().gcfr_normals_bwd(_checked(g, (B, 3, H, W), F32), _checked(depth, (B, H, W), F32), B, H, W, k[0], k[1], k[2],
                                            k[3], k[4], negate_y, _checked(gd, (B, H, W), F32), _stream()), "gcfr_normals_bwd")
    return gd


def _outputs(B, L, H, W, fill):
    """grad buffers: '=' ones full of NaN, '+=' ones zero or the given exactly representable patterns"""
    nan = lambda *s: torch.full(s, float("nan"), dtype=F32, device=dev())
    o = dict(gn=nan(B, 3, H, W), ga=nan(B, 3, H, W), gmd=nan(B, L, H, W), gd=torch.zeros((B, H, W), dtype=F32, device=dev()),
             gp=torch.zeros((B, L, 3), dtype=F64, device=dev()), gamb=torch.zeros((B, L), dtype=F64, device=dev()))
    if fill is not None:
        for k in ("gd", "gp", "gamb"):
            o[k].copy_(fill[k])
    return o


def shade_bwd(normals, depth, albedo, light_pt, ambient, md, cots, fill=None):
    """gcfr_shade_bwd; cots: g_w, g_full, g_final (B,L,H,W), g_rendered (B,L,3,H,W) or None each"""
    from geomconsistentfr_amd import _lib
    B, L, H, W = md.shape
    o = _outputs(B, L, H, W, fill)
    _lib.check(_lib.load().gcfr_shade_bwd(
        _checked(normals, (B, 3, H, W), F32), _checked(depth, (B, H, W), F32), _checked(albedo, (B, 3, H, W), F32),
        _checked(light_pt, (B, L, 3), F32), _checked(ambient, (B, L), F32), _checked(md, (B, L, H, W), F32), B, L, H, W, S.INTENSITY,
        _opt(cots.get("g_w"), (B, L, H, W)), _opt(cots.get("g_full"), (B, L, H, W)), _opt(cots.get("g_final"), (B, L, H, W)),
        _opt(cots.get("g_rendered"), (B, L, 3, H, W)), o["gn"].data_ptr(), o["ga"].data_ptr(), o["gd"].data_ptr(), o["gp"].data_ptr(),
        o["gamb"].data_ptr(), o["gmd"].data_ptr(), _stream()), "gcfr_shade_bwd")
    return o


def render_bwd(normals, depth, albedo, light_pt, ambient, md, cots, cam, negate_y=1, fill=None, argmin=None, tt=None):
    """gcfr_render_bwd, with argmin = -1 everywhere unless the forward's (argmin, sample table) are given; normals (B,3,H,W) or
    None; cots as above plus g_normals_out (B,3,H,W)"""
    from geomconsistentfr_amd import _lib
    B, L, H, W = md.shape
    o = _outputs(B, L, H, W, fill)
    if argmin is None:
        argmin = torch.full((B, L, H, W), -1, dtype=torch.int32, device=dev())
        tt = torch.linspace(0.02, 0.8, 4, dtype=F64, device=dev())
    N = tt.numel()
    k = _camera(cam, H, W)
    _lib.check(_lib.load().gcfr_render_bwd(
        _checked(depth, (B, H, W), F32), _checked(albedo, (B, 3, H, W), F32), _checked(light_pt, (B, L, 3), F32),
        _checked(ambient, (B, L), F32), _checked(md, (B, L, H, W), F32), _checked(argmin, (B, L, H, W), torch.int32),
        _opt(normals, (B, 3, H, W)), B, L, H, W, N, _checked(tt, (N,), F64), k[0], k[1], k[2], k[3], k[4], negate_y, S.INTENSITY,
        _opt(cots.get("g_w"), (B, L, H, W)), _opt(cots.get("g_full"), (B, L, H, W)), _opt(cots.get("g_final"), (B, L, H, W)),
        _opt(cots.get("g_rendered"), (B, L, 3, H, W)), _opt(cots.get("g_normals_out"), (B, 3, H, W)), o["ga"].data_ptr(),
        o["gd"].data_ptr(), o["gp"].data_ptr(), o["gamb"].data_ptr(), _stream()), "gcfr_render_bwd")
    return o


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def no_sample_value():
    """what the forward writes as minimum distance for a pixel without a sample, read from a forward run (mask all zero)"""
    if "no_sample" not in _MISC:
        from geomconsistentfr_amd import RenderParams
        from geomconsistentfr_amd import block as B_
        H, W = 8, 32
        z = torch.from_numpy(S.depth(H, W))[None].to(dev())
        o = B_.render_fwd(z, torch.zeros((1, H, W), dtype=torch.uint8, device=dev()), torch.tensor([[S.LIGHTS[0]]], dtype=F32, device=dev()),
                          torch.full((1, 1), 0.45, dtype=F32, device=dev()), None, torch.ones((1, 3, H, W), dtype=F32, device=dev()),
                          RenderParams(n_samples=8, t0=0.02, dt=0.1), want_argmin=True, camera=_camera(S.CAMERA, H, W))
        md = o["minimum_distance"].cpu()
        assert bool((o["argmin"] == -1).all()) and float(md.min()) == float(md.max())
        _MISC["no_sample"] = float(md.max())
        assert np.exp(-np.float32(_MISC["no_sample"])) == 0.0
    return _MISC["no_sample"]


def scene(H, W, L, cam=S.CAMERA, seed=1, zero_normals=False):
    """CPU tensors + the restatement of both Lambert sides.  The normals are the product's own (gcfr_normals_fwd)."""
    key = (H, W, L, cam, seed, zero_normals)
    if key in _SCENES:
        return _SCENES[key]
    depth = torch.from_numpy(S.depth(H, W, seed))
    albedo, amb, md = S.inputs(H, W, L, no_sample_value(), seed=7 * seed)
    normals = normals_fwd(depth[None].to(dev()), cam).cpu()[0]
    assert bool(torch.isfinite(normals).all())
    if zero_normals:
        normals = S.plant_zero_normals(normals, H, W)
    C = S.light_points(L)
    cots = S.cotangents(H, W, L, seed=13 * seed)
    sc = dict(H=H, W=W, L=L, cam=cam, depth=depth, albedo=albedo, amb=amb, md=md, normals=normals, C=C, cots=cots)
    _SCENES[key] = sc
    return sc


def restate(sc, names):
    """the restatement under the cotangents `names`, side A (the f64 dot product's sign) and side B (the near-kink pixels
    flipped; None without such pixels).  Asserts the 1 % cap on what is left to the either-side rule."""
    key = tuple(sorted(names))
    cache = sc.setdefault("restated", {})
    if key not in cache:
        cots = {k: sc["cots"][k] for k in names if k != "g_normals_out"}
        args = (sc["depth"], sc["normals"], sc["albedo"], sc["C"], sc["amb"], sc["md"], S.INTENSITY, cots)
        A = R.restate_shading(*args)
        near = R.kink_classes(A.dot)["near kink"]
        assert int(near.sum(dim=(1, 2)).max()) <= 0.01 * sc["H"] * sc["W"], "more than 1 % of the pixels near the kink"
        Bs = R.restate_shading(*args, lit=A.lit ^ near) if bool(near.any()) else None
        cache[key] = (A, Bs, near)
    return cache[key]


def d(t):
    return t.contiguous().to(dev())


def one_hot(c, H, W):
    """c (..., H, W) f32 on the host -> (P, ..., H, W) on the device: plane p holds c at pixel p alone"""
    P = H * W
    lead = tuple(c.shape[:-2])
    flat = c.reshape(-1, P).to(dev())
    out = torch.zeros((P, flat.shape[0], P), dtype=F32, device=dev())
    i = torch.arange(P, device=dev())
    out[i, :, i] = flat.t()
    return out.reshape((P,) + lead + (H, W)).contiguous()


def expand(t, B):
    return t[None].expand(B, *t.shape).contiguous().to(dev())


# ---------------------------------------------------------------------------------------------------------------------
# report
# ---------------------------------------------------------------------------------------------------------------------
class Report:
    """Worst error / bound per pixel class; a failure names the route, the shape, the class, the pixel and the term."""

    def __init__(self, route, H, W):
        self.route, self.H, self.W = route, H, W
        self.cls = {k: v.reshape(-1) for k, v in R.pixel_classes(H, W).items()}
        self.names = list(R.IMAGE_CLASSES + R.TILE_CLASSES + R.KINK_CLASSES)
        self.count, self.worst, self.where = {c: 0 for c in self.names}, {c: 0.0 for c in self.names}, {}
        self.terms = {}                                   # term name -> its worst error / bound over all pixels

    def add(self, ratios, kink=None, what=""):
        """ratios: term name -> (P,) error / bound of that term at (or for the plane of) each pixel; kink: class -> (P,) bool"""
        names = list(ratios)
        stack = torch.stack([ratios[k].reshape(-1).double().cpu() for k in names])
        ratio, arg = stack.max(0)
        for k, row in zip(names, stack):
            self.terms[k] = max(self.terms.get(k, 0.0), float(row.max()))
        cls = dict(self.cls)
        if kink is not None:
            cls.update({k: v.reshape(-1) for k, v in kink.items()})
        for c, m in cls.items():
            sel = m.nonzero().reshape(-1)
            self.count[c] += int(sel.numel())
            if sel.numel() and float(ratio[sel].max()) > self.worst[c]:
                p = int(sel[ratio[sel].argmax()])
                self.worst[c] = float(ratio[p])
                self.where[c] = "%s, %d x %d %s, %s pixels, pixel (%d, %d), term %s: %.3f of the bound" % (
                    self.route, self.H, self.W, what, c, p // self.W, p % self.W, names[int(arg[p])], self.worst[c])

    def check(self, need=()):
        print("route %s, %d x %d: worst error / bound per class" % (self.route, self.H, self.W))
        for c in self.names:
            print("    %-18s %6d pixels   %.3f   %s" % (c, self.count[c], self.worst[c], self.where.get(c, "")))
        print("    by term: " + ", ".join("%s %.3f" % kv for kv in self.terms.items()))
        empty = [c for c in need if self.count[c] == 0]
        assert not empty, "classes without a pixel: %s" % empty
        bad = [self.where[c] for c in self.names if self.worst[c] > 1.0]
        assert not bad, "\n".join(bad)


# class -> the shapes that must populate it (tests/test_shade_backward_restatement_host.py holds the same table on the host)
def needed_classes(H, W):
    n = {k: int(v.sum()) for k, v in R.pixel_classes(H, W).items()}
    need = [k for k, v in n.items() if v > 0]
    assert "image corner" in need and "tile corner" in need
    if (H, W) != (2, 2):
        assert all(k in need for k in R.IMAGE_CLASSES)
    if (H, W) in ((10, 34), (18, 66), (9, 33)):
        assert all(k in need for k in R.TILE_CLASSES)
    return need


def _ratio(err, bound):
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 2.0)


def _either(near, ra, rb):
    """error / bound under side A, or under the better of the two sides where the pixel is near the kink"""
    return ra if rb is None else torch.where(near, torch.minimum(ra, rb), ra)


# ---------------------------------------------------------------------------------------------------------------------
# (a) gcfr_shade_bwd
# ---------------------------------------------------------------------------------------------------------------------
SUBSETS = [("g_w",), ("g_full",), ("g_final",), ("g_rendered",), ("g_w", "g_full", "g_final", "g_rendered")]


def _per_pixel_f64(sh, got, keep_md):
    """error / bound of the per-pixel outputs of gcfr_shade_bwd under the restatement sh (one Lambert side):
    name -> (H,W); got: the kernel's outputs on the host as f64"""
    out = {}
    for k, name in (("albedo", "ga"), ("normal", "gn")):
        ref, mag = sh.val[k].sum(0).permute(2, 0, 1), sh.mag[k].sum(0).permute(2, 0, 1)
        out["grad_" + k] = _ratio((got[name] - ref).abs(), R.f64_allowance(k) * U24 * mag).max(0).values
    out["own depth"] = _ratio((got["gd"] - sh.val["own_depth"].sum(0)).abs(), R.f64_allowance("own_depth") * U24 * sh.mag["own_depth"].sum(0))
    a = R.f64_allowance("min_dist", sh.one_minus_e.clamp_min(R.SMALL_1ME))
    r = _ratio((got["gmd"] - sh.val["min_dist"]).abs(), a * U24 * sh.mag["min_dist"])
    out["grad_min_dist"] = torch.where(keep_md, r, torch.zeros((), dtype=F64)).max(0).values
    return out


@pytest.mark.parametrize("H,W,L,cam", [(H, W, L, S.CAMERA) for (H, W) in ALL_SHAPES for L in (1, 3)] + [(10, 34, 3, S.PRODUCT_CAMERA)])
def test_shade_bwd_every_pixel_under_its_own_bound(H, W, L, cam):
    sc = scene(H, W, L, cam, zero_normals=True)
    P = H * W
    rep = Report("gcfr_shade_bwd, dense, L = %d, f = %g" % (L, cam[0]), H, W)
    zero_d, _, _, zero_n = S.planted(H, W)
    base = [expand(sc[k], 1) for k in ("normals", "depth", "albedo", "C", "amb", "md")]
    for names in SUBSETS:
        A, Bs, near = restate(sc, names)
        cots = {k: expand(sc["cots"][k], 1) for k in names}
        o = shade_bwd(*base, cots)
        got = {k: v[0].cpu().double() for k, v in o.items()}
        for k in ("gn", "ga", "gmd"):
            assert bool(torch.isfinite(got[k]).all()), "%s: an element of %s was not written" % (names, k)
        keep_md = A.one_minus_e >= R.SMALL_1ME
        assert int((~keep_md).sum()) <= 0.01 * L * P
        for p in zero_d:                                   # planted d = 0: the transfer derivative is exactly zero
            assert float(got["gmd"].reshape(L, P)[:, p].abs().max()) == 0.0
        near_px = near.any(0)
        ra = _per_pixel_f64(A, got, keep_md)
        rb = None if Bs is None else _per_pixel_f64(Bs, got, keep_md)
        ratios = {k: _either(near_px, ra[k], None if rb is None else rb[k]) for k in ra}
        kink = {k: v.any(0) for k, v in R.kink_classes(A.dot).items()}
        rep.add(ratios, kink, what="upstream %s" % "+".join(names))
        # dense sums of the light and ambient gradients: the per-pixel bounds summed, plus the two sides' difference near the kink
        for k, name in (("light", "gp"), ("ambient", "gamb")):
            hull = 0.0 if Bs is None else (A.val[k] - Bs.val[k]).abs().sum((1, 2))
            bound = R.f64_allowance(k) * U24 * A.mag[k].sum((1, 2)) + hull
            r = _ratio((got[name] - A.val[k].sum((1, 2))).abs(), bound)
            assert float(r.max()) <= 1.0, "%s, %d x %d, upstream %s: dense %s gradient at %.3f of the bound" % (rep.route, H, W, names, k, float(r.max()))
        if zero_n and "g_rendered" in names:
            # planted zero-vector normals: n.l = 0 exactly, the unlit side -- no gradient on the normal; under the lit side it
            # would be dn / 1e-12 (the host test holds that value against autograd)
            assert float(got["gn"].reshape(3, P)[:, zero_n].abs().max()) == 0.0
    rep.check(needed_classes(H, W) + (["lit", "unlit"] if P >= 15 else []))


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5)])
@pytest.mark.parametrize("L", [1, 3])
def test_shade_bwd_light_and_ambient_gradient_of_every_pixel_alone(H, W, L):
    """B = H W planes, plane p carries the four cotangents at pixel p alone: grad_light_pt and grad_ambient of every (light,
    pixel); every other output is exactly zero off the pixel (written, not left as NaN)."""
    sc = scene(H, W, L, zero_normals=True)
    P = H * W
    names = SUBSETS[-1]
    A, Bs, near = restate(sc, names)
    o = shade_bwd(*[expand(sc[k], P) for k in ("normals", "depth", "albedo", "C", "amb", "md")], {k: one_hot(sc["cots"][k], H, W) for k in names})
    rep = Report("gcfr_shade_bwd, one pixel per plane, L = %d" % L, H, W)
    off = ~torch.eye(P, dtype=torch.bool, device=dev())
    for k, per in (("gn", 3), ("ga", 3), ("gmd", L), ("gd", 1)):
        assert bool((o[k].reshape(P, per, P).permute(1, 0, 2)[:, off] == 0).all()), "%s is not exactly zero off the plane's pixel" % k

    def ratios(sh):
        gp, gamb = o["gp"].cpu(), o["gamb"].cpu()                         # (P,L,3), (P,L)
        rl = _ratio((gp - sh.val["light"].reshape(L, P, 3).permute(1, 0, 2)).abs(), R.f64_allowance("light") * U24 * sh.mag["light"].reshape(L, P, 3).permute(1, 0, 2))
        ra = _ratio((gamb - sh.val["ambient"].reshape(L, P).t()).abs(), R.f64_allowance("ambient") * U24 * sh.mag["ambient"].reshape(L, P).t())
        return {"grad_light_pt": rl.reshape(P, -1).max(1).values, "grad_ambient": ra.max(1).values}

    ra, rb = ratios(A), (None if Bs is None else ratios(Bs))
    near_px = near.any(0).reshape(-1)
    rep.add({k: _either(near_px, ra[k], None if rb is None else rb[k]) for k in ra}, {k: v.any(0) for k, v in R.kink_classes(A.dot).items()})
    rep.check(needed_classes(H, W))


# ---------------------------------------------------------------------------------------------------------------------
# (b), (c): planes of grad_depth
# ---------------------------------------------------------------------------------------------------------------------
def plane_reference(t, own=None, delta=None):
    """Of a launch whose plane p carries a gradient at pixel p alone, on the device: expected grad_depth planes (P,P) f64, the
    bound per plane and texel, the number of terms.  t: StencilTerms of the per-pixel gradient; own: (value, magnitude,
    bound) (P,) each of the pixel's own-depth term; delta (P,3): the allowance on the gradient handed to the stencil."""
    P = t.idx.shape[0] * t.idx.shape[1]
    idx = t.idx.reshape(P, 8).to(dev())
    flat = (torch.arange(P, device=dev())[:, None] * P + idx).reshape(-1)
    acc = lambda v: torch.zeros(P * P, dtype=F64, device=dev()).index_add_(0, flat, v.reshape(-1).to(dev())).reshape(P, P)
    val, mag = t.val.reshape(P, 8), t.mag.reshape(P, 8)
    ref, S_, n = acc(val), acc(mag), acc((val != 0).double())
    extra = torch.zeros((P, P), dtype=F64, device=dev())
    if delta is not None:
        extra = acc((t.sens.reshape(3, P, 8) * delta.t()[..., None]).sum(0))
    if own is not None:
        i = torch.arange(P, device=dev())
        ref[i, i] += own[0].to(dev())
        S_[i, i] += own[1].to(dev())
        n[i, i] += (own[0] != 0).double().to(dev())
        extra[i, i] += own[2].to(dev())
    return ref, (n + 4) * U23 * S_ + extra, n


def plane_ratio(got, ref, bound, n):
    """(P,) worst error / bound of each plane; a non-zero value where no term lands counts as 2"""
    stray = ((got != 0) & (n == 0)).any(1)
    return torch.maximum(_ratio((got - ref).abs(), bound).max(1).values, stray.double() * 2.0).cpu(), stray.cpu()


@pytest.mark.parametrize("negate_y", [1, 0])
@pytest.mark.parametrize("H,W,cam", [(H, W, S.CAMERA) for (H, W) in ALL_SHAPES] + [(10, 34, S.PRODUCT_CAMERA)])
def test_normals_bwd_every_pixel_alone(H, W, cam, negate_y):
    P = H * W
    depth = torch.from_numpy(S.depth(H, W))
    g = S.cotangents(H, W, 1, seed=17 + negate_y)["g_normals_out"]                     # (3,H,W)
    k = _camera(cam, H, W)
    J = R.restate_stencil(depth, k[0], k[1], k[2], k[3], k[4], bool(negate_y))
    t = J.terms(g.permute(1, 2, 0))
    gd = normals_bwd(one_hot(g, H, W), expand(depth, P), cam, negate_y)
    ref, bound, n = plane_reference(t)
    r, stray = plane_ratio(gd.reshape(P, P).double(), ref, bound, n)
    assert not bool(stray.any()), "gcfr_normals_bwd, %d x %d: gradient outside the clamped 3 x 3 neighbourhood of pixel %d" % (H, W, int(stray.nonzero()[0]))
    rep = Report("gcfr_normals_bwd, one pixel per plane, negate_y = %d, f = %g" % (negate_y, cam[0]), H, W)
    rep.add({"stencil terms": r})
    rep.check(needed_classes(H, W))


def _fused_allowances(sh, L):
    """of the f32 shading stage, per pixel (flat P): delta (P,3) on the gradient handed to the stencil, the own-depth term
    (value, magnitude, bound), and the bounds of grad_albedo (P,3), light (P,L,3), ambient (P,L)."""
    P = sh.H * sh.W
    more = float(L - 1)                                   # the f32 (f64: nothing) sums over the lights
    mh = sh.mag["normal"].sum(0).reshape(P, 3)
    delta = (R.F32_GATE["normal"] + more) * U24 * mh
    own = (sh.val["own_depth"].sum(0).reshape(P), sh.mag["own_depth"].sum(0).reshape(P),
           R.F32_GATE["own_depth"] * U24 * sh.mag["own_depth"].sum(0).reshape(P))
    b_alb = (R.F32_GATE["albedo"] + more) * U24 * sh.mag["albedo"].sum(0).reshape(P, 3)
    b_light = R.F32_GATE["light"] * U24 * sh.mag["light"].reshape(L, P, 3).permute(1, 0, 2)
    b_amb = R.F32_GATE["ambient"] * U24 * sh.mag["ambient"].reshape(L, P).t()
    return delta, own, b_alb, b_light, b_amb


SHADING = ("g_full", "g_final", "g_rendered")


@pytest.mark.parametrize("H,W,L,cam", [(H, W, L, S.CAMERA) for (H, W) in S.FUSED_SHAPES for L in (1, 2)] + [(10, 34, 1, S.PRODUCT_CAMERA)])
def test_render_bwd_every_pixel_alone(H, W, L, cam):
    """gcfr_render_bwd, B = H W planes, argmin = -1: through g_rendered + g_final + g_full (the f32 shading stage feeds the
    stencil) and through g_normals_out alone (the shading stage idle: the gather / scatter split of the stencil in
    isolation), the forward's normals given and NULL."""
    sc = scene(H, W, L, cam)
    P = H * W
    k = _camera(cam, H, W)
    J = R.restate_stencil(sc["depth"], k[0], k[1], k[2], k[3], k[4], True)
    A, Bs, near = restate(sc, SHADING)
    near_px = near.any(0).reshape(-1)
    kink = {kk: v.any(0) for kk, v in R.kink_classes(A.dot).items()}
    base = {kk: expand(sc[kk], P) for kk in ("depth", "albedo", "C", "amb", "md")}
    gno = sc["cots"]["g_normals_out"]
    hot = {kk: one_hot(sc["cots"][kk], H, W) for kk in SHADING}
    hot_gno = one_hot(gno, H, W)
    eye = torch.eye(P, dtype=torch.bool, device=dev())

    def side(sh, o):
        delta, own, b_alb, b_light, b_amb = _fused_allowances(sh, L)
        t = J.terms(sh.val["normal"].sum(0))
        ref, bound, n = plane_reference(t, own, delta)
        rd, _ = plane_ratio(o["gd"].reshape(P, P).double(), ref, bound, n)
        ga = o["ga"].reshape(P, 3, P)
        ga_own = ga.permute(1, 0, 2)[:, eye].t().cpu().double()                          # (P,3): plane p, pixel p
        stray = (ga.permute(1, 0, 2)[:, ~eye] != 0).any().cpu()
        ralb = _ratio((ga_own - sh.val["albedo"].sum(0).reshape(P, 3)).abs(), b_alb).max(1).values + 2.0 * float(stray)
        rl = _ratio((o["gp"].cpu() - sh.val["light"].reshape(L, P, 3).permute(1, 0, 2)).abs(), b_light).reshape(P, -1).max(1).values
        ra = _ratio((o["gamb"].cpu() - sh.val["ambient"].reshape(L, P).t()).abs(), b_amb).max(1).values
        return {"grad_depth (stencil terms + own depth)": rd, "grad_albedo": ralb, "grad_light_pt": rl, "grad_ambient": ra}

    for nrm_name, nrm in (("given", expand(sc["normals"], P)), ("NULL", None)):
        rep = Report("gcfr_render_bwd, one pixel per plane, L = %d, normals %s, f = %g" % (L, nrm_name, cam[0]), H, W)
        o = render_bwd(nrm, base["depth"], base["albedo"], base["C"], base["amb"], base["md"], hot, cam)
        assert bool(torch.isfinite(o["ga"]).all()), "an element of grad_albedo was not written"
        ra, rb = side(A, o), (None if Bs is None else side(Bs, o))
        rep.add({kk: _either(near_px, ra[kk], None if rb is None else rb[kk]) for kk in ra}, kink, what="upstream g_rendered+g_final+g_full")
        # g_normals_out alone: no f32 stage, the f64 stencil's own bound; albedo, light and ambient gradients exactly zero
        o = render_bwd(nrm, base["depth"], base["albedo"], base["C"], base["amb"], base["md"], {"g_normals_out": hot_gno}, cam)
        assert float(o["ga"].abs().max()) == 0.0 and float(o["gp"].abs().max()) == 0.0 and float(o["gamb"].abs().max()) == 0.0
        ref, bound, n = plane_reference(J.terms(gno.permute(1, 2, 0)))
        rd, stray = plane_ratio(o["gd"].reshape(P, P).double(), ref, bound, n)
        assert not bool(stray.any()), "%s: gradient outside the clamped 3 x 3 neighbourhood of pixel %d" % (rep.route, int(stray.nonzero()[0]))
        rep.add({"grad_depth (stencil terms)": rd}, what="upstream g_normals_out")
        rep.check(needed_classes(H, W) + (["lit", "unlit"] if P >= 15 else []))


ALL_FUSED = ("g_w", "g_full", "g_final", "g_rendered", "g_normals_out")


@pytest.mark.parametrize("H,W", S.FUSED_SHAPES)
@pytest.mark.parametrize("L", [1, 3])
def test_render_bwd_dense_per_texel(H, W, L):
    """gcfr_render_bwd, B = 2 (two depth maps), every upstream gradient dense, argmin = -1: at L = 1 one tile per workgroup.
    grad_depth per texel, grad_albedo per pixel, light and ambient per (image, light)."""
    scs = [scene(H, W, L, seed=s) for s in (1, 2)]
    P = H * W
    st = lambda key: torch.stack([sc[key] for sc in scs]).contiguous().to(dev())
    cots = {kk: torch.stack([sc["cots"][kk] for sc in scs]).contiguous().to(dev()) for kk in ALL_FUSED}
    k = _camera(S.CAMERA, H, W)
    for nrm in (st("normals"), None):
        o = render_bwd(nrm, st("depth"), st("albedo"), st("C"), st("amb"), st("md"), cots, S.CAMERA)
        assert bool(torch.isfinite(o["ga"]).all()), "an element of grad_albedo was not written"
        rep = Report("gcfr_render_bwd, dense, B = 2, L = %d, normals %s" % (L, "given" if nrm is not None else "NULL"), H, W)
        for b, sc in enumerate(scs):
            A, Bs, near = restate(sc, ALL_FUSED)
            delta, own, b_alb, b_light, b_amb = _fused_allowances(A, L)
            hull = lambda key: 0.0 if Bs is None else (A.val[key] - Bs.val[key]).abs()
            if Bs is not None:                               # near the kink: the two sides' difference joins the bound
                delta = delta + hull("normal").sum(0).reshape(P, 3)
                own = (own[0], own[1], own[2] + hull("own_depth").sum(0).reshape(P))
                b_alb = b_alb + hull("albedo").sum(0).reshape(P, 3)
                b_light = b_light + hull("light").reshape(L, P, 3).permute(1, 0, 2)
                b_amb = b_amb + hull("ambient").reshape(L, P).t()
            J = R.restate_stencil(sc["depth"], k[0], k[1], k[2], k[3], k[4], True)
            g = A.val["normal"].sum(0) + sc["cots"]["g_normals_out"].double().permute(1, 2, 0)
            field, S_, n, prop = R.scatter_terms(J.terms(g), H, W, delta.reshape(H, W, 3))
            field = field + own[0].reshape(H, W)
            S_, n = S_ + own[1].reshape(H, W), n + (own[0] != 0).double().reshape(H, W)
            bound = (n + 4) * U23 * S_ + prop + own[2].reshape(H, W)
            rd = _ratio((o["gd"][b].cpu().double() - field).abs(), bound)
            ralb = _ratio((o["ga"][b].cpu().double().reshape(3, P).t() - A.val["albedo"].sum(0).reshape(P, 3)).abs(), b_alb).max(1).values
            rep.add({"grad_depth (texel)": rd, "grad_albedo": ralb}, {kk: v.any(0) for kk, v in R.kink_classes(A.dot).items()}, what="image %d" % b)
            rl = _ratio((o["gp"][b].cpu() - A.val["light"].sum((1, 2))).abs(), b_light.sum(0))
            ra = _ratio((o["gamb"][b].cpu() - A.val["ambient"].sum((1, 2))).abs(), b_amb.sum(0))
            assert float(rl.max()) <= 1.0 and float(ra.max()) <= 1.0, "%s, %d x %d, image %d: light / ambient sums at %.3f / %.3f of the bound" % (
                rep.route, H, W, b, float(rl.max()), float(ra.max()))
        rep.check(needed_classes(H, W))


# ---------------------------------------------------------------------------------------------------------------------
# (d) composition with the march backward: the fused backward as training runs it
# ---------------------------------------------------------------------------------------------------------------------
def _march_forward(H, W, N, kind):
    """tests/test_gpu_march_backward_pixels.py's cached forward of a tests/march_scenes.py scene (argmin and minimum distance
    checked against the C oracle bit for bit) and its unit-cotangent march restatements per light"""
    import test_gpu_march_backward_pixels as MT
    return MT.forward(H, W, N, kind)


def _composition_scene(f, ls, seed):
    """the shading scene of the lights `ls` of a march forward `f`: the REAL minimum distances; every upstream gradient dense,
    except on the (at most 1 % of the live) pixels whose 1 - e is under 2^-10, where all of them are zero (the fused routes'
    exclusion of the march test, march_backward_restatement.fused_route_pixels)"""
    import march_backward_restatement as MR
    H, W, L = f["H"], f["W"], len(ls)
    md = f["md_cpu"][ls]
    cots = S.cotangents(H, W, L, seed=seed)
    for j, l in enumerate(ls):
        live = f["live"][l]
        ome = 1.0 - R.exp_neg_f32(torch.where(live, md[j], torch.ones(())))
        keep, _, _ = MR.fused_route_pixels(ome, live)
        assert int((live & ~keep).sum()) <= 0.01 * int(live.sum())
        for kk in ("g_w", "g_full", "g_final"):
            cots[kk][j][live & ~keep] = 0.0
        cots["g_rendered"][j][:, live & ~keep] = 0.0
    return dict(H=H, W=W, L=L, cam=S.CAMERA, depth=f["depth"].cpu(), albedo=f["albedo"].cpu(), amb=torch.full((L,), 0.45, dtype=F32), md=md,
                normals=f["normals"].cpu(), C=f["light_pt"].cpu()[ls], cots=cots)


def _composed_reference(f, ls, sc):
    """per texel: the march restatement's field plus the shading / stencil restatement's field, and the sum of their bounds;
    per pixel grad_albedo; per light the light-point and ambient sums.  The march takes the restated gradient on the minimum
    distance; the f32 stage's allowance on it (F32_GATE["min_dist"], with the 1 + 1/(1 - e) of the transfer derivative) and the
    two Lambert sides' difference near the kink travel through the march's terms, which are linear in it."""
    H, W, L = sc["H"], sc["W"], sc["L"]
    P = H * W
    A, Bs, near = restate(sc, ALL_FUSED)
    hull = lambda key: torch.zeros_like(A.val[key]) if Bs is None else (A.val[key] - Bs.val[key]).abs()
    delta, own, b_alb, b_light, b_amb = _fused_allowances(A, L)
    delta = delta + hull("normal").sum(0).reshape(P, 3)
    own = (own[0], own[1], own[2] + hull("own_depth").sum(0).reshape(P))
    b_alb = b_alb + hull("albedo").sum(0).reshape(P, 3)
    b_light = (b_light + hull("light").reshape(L, P, 3).permute(1, 0, 2)).sum(0)              # (L,3)
    b_amb = (b_amb + hull("ambient").reshape(L, P).t()).sum(0)
    k = _camera(S.CAMERA, H, W)
    J = R.restate_stencil(sc["depth"], k[0], k[1], k[2], k[3], k[4], True)
    g = A.val["normal"].sum(0) + sc["cots"]["g_normals_out"].double().permute(1, 2, 0)
    field, S_, n, extra = R.scatter_terms(J.terms(g), H, W, delta.reshape(H, W, 3))
    field, S_, n, extra = field + own[0].reshape(H, W), S_ + own[1].reshape(H, W), n + (own[0] != 0).double().reshape(H, W), extra + own[2].reshape(H, W)
    light = A.val["light"].sum((1, 2)).clone()
    for j, l in enumerate(ls):
        live = f["live"][l]
        gmd = A.val["min_dist"][j] * live
        dg = (R.F32_GATE["min_dist"] * U24 * (1.0 + 1.0 / A.one_minus_e[j].clamp_min(R.SMALL_1ME)) * A.mag["min_dist"][j] + hull("min_dist")[j]) * live
        rg, rd = f["r"][l].times(gmd), f["r"][l].times(dg)
        sg, ab, cn = rg.scatter()
        field, S_, n, extra = field + sg, S_ + ab, n + cn, extra + rd.scatter()[1]
        gc, mag = rg.light()
        light[j] += gc
        b_light[j] += 2.0 ** -22 * mag + rd.light()[1]
    return A, field, (n + 4) * U23 * S_ + extra, light, b_light, b_amb, b_alb


@pytest.mark.parametrize("route", ["L = 1", "L = 10"])
def test_fused_backward_as_training_runs_it_per_texel(route):
    """48 x 72 of tests/march_scenes.py, smooth and rough, the real forward's argmin and minimum distance, every upstream gradient
    dense: grad_depth per texel against the SUM of the march restatement's field and this file's, under the sum of their
    bounds ((n + 4) 2^-23 S over all terms landing on the texel, plus the propagated f32 allowances); grad_albedo per pixel,
    light and ambient per (image, light).  L = 1: every (depth, light) an image of its own."""
    import march_scenes as MS
    H, W, N = MS.SIZES[1]
    P = H * W
    nl = len(MS.LIGHTS)
    for b, kind in enumerate(MS.DEPTHS):
        f = _march_forward(H, W, N, kind)
        groups = [[l] for l in range(nl)] if route == "L = 1" else [list(range(nl))]
        scs = [_composition_scene(f, ls, seed=50 + b) for ls in groups]
        L = len(groups[0])
        st = lambda key: torch.stack([sc[key] for sc in scs]).contiguous().to(dev())
        cots = {kk: torch.stack([sc["cots"][kk] for sc in scs]).contiguous().to(dev()) for kk in ALL_FUSED}
        am = torch.stack([f["am"][ls] for ls in groups]).contiguous()
        o = render_bwd(st("normals"), st("depth"), st("albedo"), st("C"), st("amb"), st("md"), cots, S.CAMERA, argmin=am, tt=f["tt"])
        assert bool(torch.isfinite(o["ga"]).all())
        rep = Report("gcfr_render_bwd with the march, dense, %s, %s depth" % (route, kind), H, W)
        for i, (ls, sc) in enumerate(zip(groups, scs)):
            A, field, bound, light, b_light, b_amb, b_alb = _composed_reference(f, ls, sc)
            rd = _ratio((o["gd"][i].cpu().double() - field).abs(), bound)
            ralb = _ratio((o["ga"][i].cpu().double().reshape(3, P).t() - A.val["albedo"].sum(0).reshape(P, 3)).abs(), b_alb).max(1).values
            rep.add({"grad_depth (texel)": rd, "grad_albedo": ralb}, {kk: v.any(0) for kk, v in R.kink_classes(A.dot).items()}, what="lights %s" % ls)
            rl = _ratio((o["gp"][i].cpu() - light).abs(), b_light)
            ra = _ratio((o["gamb"][i].cpu() - A.val["ambient"].sum((1, 2))).abs(), b_amb)
            assert float(rl.max()) <= 1.0 and float(ra.max()) <= 1.0, "%s, lights %s: light / ambient sums at %.3f / %.3f of the bound" % (
                rep.route, ls, float(rl.max()), float(ra.max()))
        rep.check(needed_classes(H, W))


# ---------------------------------------------------------------------------------------------------------------------
# (e) "+=" buffers
# ---------------------------------------------------------------------------------------------------------------------
def test_accumulated_buffers_add_to_what_they_hold():
    """grad_depth, grad_light_pt and grad_ambient are "+=": pre-filled with an exactly representable pattern, the increment
    equals the zero-filled launch's result up to the roundings of the additions themselves -- f32: (n + 4) 2^-23 (|pattern| +
    S) per texel, f64: 2^-50 (|pattern| + the summed magnitudes).  Both entries, 10 x 34 (partial tiles), L = 1 and 3."""
    H, W = 10, 34
    P = H * W
    for L in (1, 3):
        sc = scene(H, W, L)
        A, _, _ = restate(sc, ALL_FUSED)
        pat = lambda n, s: ((torch.arange(n, dtype=F64) % 7) - 3.0) * s
        fill = dict(gd=pat(P, 2.0 ** -20).reshape(1, H, W).float().to(dev()), gp=pat(3 * L, 0.25).reshape(1, L, 3).to(dev()),
                    gamb=pat(L, 0.5).reshape(1, L).to(dev()) + 8.0)
        k = _camera(S.CAMERA, H, W)
        J = R.restate_stencil(sc["depth"], k[0], k[1], k[2], k[3], k[4], True)
        g = A.val["normal"].sum(0) + sc["cots"]["g_normals_out"].double().permute(1, 2, 0)
        _, S_, n, _ = R.scatter_terms(J.terms(g), H, W)
        S_, n = S_ + A.mag["own_depth"].sum(0), n + 1
        base = [expand(sc[kk], 1) for kk in ("depth", "albedo", "C", "amb", "md")]
        cots = {kk: expand(sc["cots"][kk], 1) for kk in ALL_FUSED}
        shade_cots = {kk: v for kk, v in cots.items() if kk != "g_normals_out"}
        nrm = expand(sc["normals"], 1)
        for name, run in (("gcfr_render_bwd", lambda f: render_bwd(nrm, *base, cots, S.CAMERA, fill=f)),
                          ("gcfr_shade_bwd", lambda f: shade_bwd(nrm, *base, shade_cots, fill=f))):
            zero, filled = run(None), run(fill)
            inc = filled["gd"].double() - fill["gd"].double()
            bound = ((n + 4) * U23 * (fill["gd"].cpu().double().abs()[0] + S_)).to(dev())
            assert bool(((inc[0] - zero["gd"][0].double()).abs() <= bound).all()), "%s, L = %d: grad_depth is not accumulated into" % (name, L)
            for kk, m in (("gp", A.mag["light"].sum((1, 2))), ("gamb", A.mag["ambient"].sum((1, 2)))):
                inc = (filled[kk] - fill[kk]).cpu()[0]
                assert bool(((inc - zero[kk].cpu()[0]).abs() <= 2.0 ** -50 * (fill[kk].cpu()[0].abs() + m)).all()), "%s, L = %d: %s is not accumulated into" % (name, L, kk)
            assert float((filled["gd"] - fill["gd"]).abs().max()) > 0 and float((filled["gp"] - fill["gp"]).abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# one-pixel-wide images are refused by both normals entries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 6), (6, 1)])
def test_normals_entries_refuse_one_pixel_wide_images(H, W):
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd.normals import depth_to_normals
    K = torch.tensor([[[600.0, 0.0, W / 2.0], [0.0, 600.0, H / 2.0], [0.0, 0.0, 1.0]]], dtype=F64, device=dev())
    depth = torch.rand((2, 1, H, W), dtype=F32, device=dev())
    with pytest.raises(_lib.GcfrError, match="GCFR_ERR_INVALID_ARGUMENT"):
        depth_to_normals(depth, K, z_offset=900.0)
    # the C ABI, forward and backward: refused before a launch, the output buffers untouched
    lib = _lib.load()
    out = torch.full((2, 3, H, W), 7.0, dtype=F32, device=dev())
    gd = torch.full((2, H, W), 7.0, dtype=F32, device=dev())
    z = depth[:, 0].contiguous()
    assert lib.gcfr_normals_fwd(z.data_ptr(), 2, H, W, 600.0, 600.0, W / 2.0, H / 2.0, 900.0, 1, out.data_ptr(), _stream()) == -1
    assert lib.gcfr_normals_bwd(out.data_ptr(), z.data_ptr(), 2, H, W, 600.0, 600.0, W / 2.0, H / 2.0, 900.0, 1, gd.data_ptr(), _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((gd == 7.0).all())
