"""The march's backward (gcfr_backward.hip: shadow_bwd_pixel and its three launch routes) pinned PER PIXEL and PER TEXEL
to oracle/march_backward_restatement.py, the frozen-decision f64 restatement validated on the host by
tests/test_march_backward_restatement_host.py.  Scenes: tests/march_scenes.py.

The forward runs through render_fwd(..., want_argmin=True); argmin and minimum_distance are asserted equal to the C
oracle's bit for bit before use, and the restatement takes the PRODUCT's argmin, so no near-tie can make a test flaky.

Gates (derived, not picked):
  depth, per texel:   |got - ref| <= (n + 4) 2^-23 S
      n = number of terms landing on the texel, S = sum of their absolute values, both from the restatement.  Each term is
      computed in f64 and cast to f32 (2^-24 of the term); each f32 atomic or LDS add rounds a partial sum no larger than S
      (2^-24 S, n of them); the factor 2 covers f32-rounded operands in derivative-only positions.
  light, per plane or per (image, light), per component:   |got - ref| <= 2^-22 (sum of the pixels' light-gradient magnitudes)
      the block sums are f64; the allowance is dominated by the upstream gradient being f32.
  fused routes: the kernels evaluate the transfer derivative 4e(1-e)/(1+e)^3, e = exp(-d), in f32, and 1 - e cancels at small
      d: every pixel's terms get the extra relative allowance 2^-22 (1 + 1/(1 - e)); pixels with 1 - e < 2^-10 are left
      out of the fused-route comparisons, at most 1 % of the live pixels (march_backward_restatement.fused_route_pixels:
      3 ... 6 % of these scenes' live pixels lie under that threshold, so the cap binds and the rest is compared).

Every class of tests/march_scenes.py must be populated and inside the gate; a failure names the class, the light and the
term.  The worst observed error / bound ratios per route and class are recorded in DESIGN.md ("How the backward is pinned").
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import march_backward_restatement as R  # noqa: E402
import march_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

U23, U22 = 2.0 ** -23, 2.0 ** -22
CAM = (600.0, 600.0, None, None, 900.0)      # fx, fy, (cx, cy = W/2, H/2), z_offset
_FWD = {}


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _params(N):
    from geomconsistentfr_amd import RenderParams
    return RenderParams(n_samples=N, t0=0.02, dt=0.8 / N)


def forward(H, W, N, kind):
    """One forward per scene, all ten lights: the product's argmin / minimum distance / light points (checked against the C
    oracle bit for bit) and the unit-cotangent restatement per light.  Computed once and shared."""
    key = (H, W, N, kind)
    if key in _FWD:
        return _FWD[key]
    import c_oracle
    from geomconsistentfr_amd import block as B_
    depth_np, mask_np = S.scene(H, W, kind)
    prm = _params(N)
    L = len(S.LIGHTS)
    rng = np.random.default_rng(11)
    albedo = rng.random((1, 3, H, W), dtype=np.float32)
    cam = (CAM[0], CAM[1], W / 2.0, H / 2.0, CAM[4])
    o = B_.render_fwd(to_dev(depth_np[None]), to_dev(mask_np[None]), to_dev(np.asarray(S.LIGHTS, np.float32)[None]),
                      to_dev(np.full((1, L), 0.45, np.float32)), None, to_dev(albedo), prm, want_argmin=True, camera=cam)
    tt = B_.sample_table(prm, dev())
    assert np.array_equal(tt.cpu().numpy(), S.params(N).sample_table())
    pt = o["light_pt"].cpu().numpy().reshape(L, 3)
    _, pt_o = c_oracle.light_prep(np.asarray(S.LIGHTS, np.float32), clamp_z_min=0.0)
    np.testing.assert_array_equal(pt, pt_o)
    md, am = o["minimum_distance"].cpu().numpy()[0], o["argmin"].cpu().numpy()[0]
    md_o, am_o = c_oracle.shadow_min_distance(depth_np[None], mask_np[None], pt[None], tt.cpu().numpy())
    lit = md_o[0] < 1e5
    np.testing.assert_array_equal(md, md_o[0])
    assert np.all(am[~lit] == -1)
    np.testing.assert_array_equal(am[lit], am_o[0][lit])
    depth = torch.from_numpy(depth_np)
    rs = [R.restate(depth, torch.from_numpy(pt[l]), torch.from_numpy(am[l].astype(np.int64)), S.params(N)) for l in range(L)]
    f = dict(H=H, W=W, N=N, depth=to_dev(depth_np), albedo=to_dev(albedo[0]), light_pt=to_dev(pt), md=to_dev(md), am=to_dev(am),
             normals=o["surface_normals"][0].contiguous(), tt=tt, cam=cam, r=rs, md_cpu=torch.from_numpy(md), live=torch.from_numpy(am >= 0))
    _FWD[key] = f
    return f


def _checked(t, shape, dtype):
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == tuple(shape), (tuple(t.shape), shape, t.dtype)
    return t.data_ptr()


def shadow_bwd(g_md, depth, light_pt, argmin, N, tt):
    """gcfr_shadow_bwd with every buffer's shape, dtype and contiguity checked against (B,L,H,W) first."""
    from geomconsistentfr_amd import _lib
    B, L, H, W = g_md.shape
    assert B * L <= 65535 and tt.numel() == N and tt.dtype == torch.float64 and tt.is_cuda
    gd = torch.zeros((B, H, W), dtype=torch.float32, device=dev())
    gp = torch.zeros((B, L, 3), dtype=torch.float64, device=dev())
    _lib.check(_lib.load().gcfr_shadow_bwd(_checked(g_md, (B, L, H, W), torch.float32), _checked(depth, (B, H, W), torch.float32),
                                           _checked(light_pt, (B, L, 3), torch.float32), _checked(argmin, (B, L, H, W), torch.int32),
                                           B, L, H, W, N, tt.data_ptr(), gd.data_ptr(), gp.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "gcfr_shadow_bwd")
    return gd, gp


def render_bwd(g_w, depth, albedo, light_pt, ambient, md, argmin, normals, N, tt, cam):
    """gcfr_render_bwd with g_shadow_w as the ONLY upstream gradient: nothing but the march backward then contributes to
    the depth and light gradients, and the ambient gradient is zero.  Buffers checked as above."""
    from geomconsistentfr_amd import _lib
    B, L, H, W = g_w.shape
    assert B <= 65535 and tt.numel() == N and tt.dtype == torch.float64 and tt.is_cuda
    ga = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev())
    gd = torch.zeros((B, H, W), dtype=torch.float32, device=dev())
    gp = torch.zeros((B, L, 3), dtype=torch.float64, device=dev())
    gamb = torch.zeros((B, L), dtype=torch.float64, device=dev())
    _lib.check(_lib.load().gcfr_render_bwd(
        _checked(depth, (B, H, W), torch.float32), _checked(albedo, (B, 3, H, W), torch.float32),
        _checked(light_pt, (B, L, 3), torch.float32), _checked(ambient, (B, L), torch.float32),
        _checked(md, (B, L, H, W), torch.float32), _checked(argmin, (B, L, H, W), torch.int32),
        None if normals is None else _checked(normals, (B, 3, H, W), torch.float32), B, L, H, W, N, tt.data_ptr(),
        cam[0], cam[1], cam[2], cam[3], cam[4], 1, 0.5, _checked(g_w, (B, L, H, W), torch.float32), None, None, None, None, ga.data_ptr(), gd.data_ptr(),
        gp.data_ptr(), gamb.data_ptr(), torch.cuda.current_stream().cuda_stream), "gcfr_render_bwd")
    assert float(gamb.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0
    return gd, gp


def _expand(t, B):
    return t[None].expand(B, *t.shape).contiguous()


class Report:
    """Worst error / bound ratio per class; a failure names the class, the light and the term."""

    def __init__(self, route):
        self.route, self.count, self.worst, self.where = route, {c: 0 for c in R.CLASS_NAMES}, {c: 0.0 for c in R.CLASS_NAMES}, {}

    def add(self, r, light, ratio_depth, ratio_light, worst_texel, planes):
        """ratio_* (P,) per one-hot plane (pixel); worst_texel (P,) the texel of each plane's worst depth ratio, to name the
        term; planes (P,) bool: the planes compared."""
        ratio = torch.maximum(ratio_depth, ratio_light) * planes
        for c in R.CLASS_NAMES:
            sel = (r.classes[c].reshape(-1) & planes).nonzero().reshape(-1)
            self.count[c] += int(sel.numel())
            if sel.numel() and float(ratio[sel].max()) > self.worst[c]:
                p = int(sel[ratio[sel].argmax()])
                self.worst[c] = float(ratio[p])
                rr, cc = divmod(p, r.W)
                if ratio_depth[p] >= ratio_light[p]:
                    tx = int(worst_texel[p])
                    names = ([R.TERM_NAMES[j] for j in range(5) if int(r.term_idx[rr, cc, j]) == tx]
                             or ["a texel outside this light's five (the plane's other light, if it has one)"])
                    term = "depth, " + " + ".join(names)
                else:
                    term = "light point via " + R.LIGHT_USES[int(r.gC_uses[:, rr, cc].abs().sum(-1).argmax())]
                self.where[c] = "%s, pixel (%d, %d): %.3f of the bound" % (S.describe_term(term, [c], light), rr, cc, self.worst[c])

    def check(self, need=R.CLASS_NAMES):
        print("route %s: worst error / bound per class" % self.route)
        for c in R.CLASS_NAMES:
            print("    %-16s %6d pixels   %.3f   %s" % (c, self.count[c], self.worst[c], self.where.get(c, "")))
        empty = [c for c in need if self.count[c] == 0]
        assert not empty, "classes without a pixel: %s" % empty
        bad = [self.where[c] for c in R.CLASS_NAMES if self.worst[c] > 1.0]
        assert not bad, "\n".join(bad)


def _one_hot_reference(r, g, extra=None):
    """Of the launch whose plane p holds g[p] at pixel p alone, on the device: the expected grad_depth planes (P,P) f64, the sum
    of |term| and the number of terms per plane and texel, the per-plane extra relative allowance of the fused routes (P,);
    on the host: the light gradients (P,3) and their bounds."""
    P = r.H * r.W
    rg = r.times(g)
    val, idx = rg.term_val.reshape(P, 5).to(dev()), r.term_idx.reshape(P, 5).to(dev())
    flat = (torch.arange(P, device=dev())[:, None] * P + idx).reshape(-1)
    acc = lambda v: torch.zeros(P * P, dtype=torch.float64, device=dev()).index_add_(0, flat, v.reshape(-1)).reshape(P, P)
    x = torch.zeros(P, dtype=torch.float64) if extra is None else extra.reshape(P).double()
    return acc(val), acc(val.abs()), acc((val != 0).double()), x.to(dev()), rg.gC.reshape(P, 3), rg.gC_mag.reshape(P, 3) * (U22 + x[:, None])


def _ratio(err, bound):
    return torch.where(bound > 0, err / bound, (err > 0).double() * 2.0)


def _compare_one_hot(rep, r, light, g, gd, gp, planes, extra=None):
    """gd (P,H,W) f32, gp (P,3) f64 from a launch with one-hot upstream planes; planes (P,) bool: the planes compared (a
    plane whose pixel has no sample is compared too: it must be zero everywhere)."""
    P = r.H * r.W
    ref, S_, n, x, lref, lbound = _one_hot_reference(r, g, extra)
    got = gd.reshape(P, P).double()
    assert bool(((got == 0) | (n > 0))[planes.to(dev())].all()), "%s: gradient outside the pixel's five texels" % S.light_name(light)
    rd = _ratio((got - ref).abs(), (n + 4) * U23 * S_ + S_ * x[:, None])
    rl = _ratio((gp.reshape(P, 3).cpu() - lref).abs(), lbound).max(1).values
    rep.add(r, light, rd.max(1).values.cpu(), rl, rd.argmax(1).cpu(), planes)


def _one_hot(P, g):
    m = torch.zeros((P, P), dtype=torch.float32, device=dev())
    m.diagonal().copy_(g.reshape(P).to(dev()))
    return m


@pytest.mark.parametrize("H,W,N,kind", [(H, W, N, k) for (H, W, N) in S.SIZES for k in S.DEPTHS])
def test_every_pixel_alone_three_kernel_route(H, W, N, kind):
    """gcfr_shadow_bwd, B = H W planes, L = 1: plane p carries a random g at pixel p alone, so ONE launch returns every
    pixel's own grad_light_pt (f64) and its own grad_depth plane."""
    f = forward(H, W, N, kind)
    P = H * W
    rng = np.random.default_rng(21)
    rep = Report("gcfr_shadow_bwd, one pixel per plane, %d x %d %s" % (H, W, kind))
    depth, am_all = _expand(f["depth"], P), f["am"]
    for l, light in enumerate(S.LIGHTS):
        g = torch.from_numpy((rng.standard_normal((H, W)) + np.sign(rng.standard_normal((H, W))) * 0.1).astype(np.float32))
        gd, gp = shadow_bwd(_one_hot(P, g).reshape(P, 1, H, W), depth, _expand(f["light_pt"][l:l + 1], P),
                            _expand(am_all[l:l + 1], P), N, f["tt"])
        _compare_one_hot(rep, f["r"][l], light, g, gd, gp.reshape(P, 3), torch.ones(P, dtype=torch.bool))
    rep.check()


def _fused_cotangent(f, l, rng):
    """Random g_w, the restatement's gradient on the distance g_w 4e(1-e)/(1+e)^3 in f64 from the product's f32 minimum
    distance, the fused routes' extra allowance 2^-22 (1 + 1/(1 - e)) and the pixels compared (fused_route_pixels)."""
    H, W = f["H"], f["W"]
    g_w = torch.from_numpy((rng.standard_normal((H, W)) + np.sign(rng.standard_normal((H, W))) * 0.1).astype(np.float32))
    live = f["live"][l]
    g, ome = R.transfer_gradient(torch.where(live, f["md_cpu"][l], torch.ones(())), g_w)
    keep, extra, _ = R.fused_route_pixels(ome, live)
    assert int((live & ~keep).sum()) <= 0.01 * int(live.sum())
    assert float(f["md_cpu"][l][live].max()) < 80.0          # exp(-d) stays a normal f32
    return g_w, g * live, extra, keep


@pytest.mark.parametrize("normals", ["given", "recomputed"])
@pytest.mark.parametrize("L", [1, 2])
def test_every_pixel_alone_fused_routes(L, normals):
    """gcfr_render_bwd at 40 x 48, one pixel per plane through g_shadow_w: L = 1 (render_bwd_single_light_kernel) and L = 2
    with two different lights in each plane (render_bwd_multi_light_kernel), the forward's normals given or NULL."""
    H, W, N = S.SIZES[0]
    kind = "smooth"
    f = forward(H, W, N, kind)
    P = H * W
    rng = np.random.default_rng(31 + L)
    rep = Report("gcfr_render_bwd, one pixel per plane, L = %d, normals %s" % (L, normals))
    depth, albedo = _expand(f["depth"], P), _expand(f["albedo"], P)
    nrm = _expand(f["normals"], P) if normals == "given" else None
    amb = torch.full((P, L), 0.45, dtype=torch.float32, device=dev())
    for l0 in range(0, len(S.LIGHTS), L):
        ls = list(range(l0, l0 + L))
        cots = [_fused_cotangent(f, l, rng) for l in ls]
        g_w = torch.stack([_one_hot(P, c[0]) for c in cots], 1).reshape(P, L, H, W).contiguous()
        sl = slice(l0, l0 + L)
        gd, gp = render_bwd(g_w, depth, albedo, _expand(f["light_pt"][sl], P), amb, _expand(f["md"][sl], P),
                            _expand(f["am"][sl], P), nrm, N, f["tt"], f["cam"])
        comp = [c[3] | ~f["live"][l] for l, c in zip(ls, cots)]          # pixels compared: kept, or without a sample
        if L == 1:
            _compare_one_hot(rep, f["r"][l0], S.LIGHTS[l0], cots[0][1], gd, gp.reshape(P, 3), comp[0].reshape(-1).clone(), cots[0][2])
            continue
        # two lights in a plane: the depth plane is the sum of both lights' terms -- bound (n0 + n1 + 4) 2^-23 (S0 + S1) plus each
        # light's own extra allowance -- and each light point has its own gradient
        refs = [_one_hot_reference(f["r"][l], c[1], c[2]) for l, c in zip(ls, cots)]
        planes = (comp[0] & comp[1]).reshape(-1).clone()
        n = refs[0][2] + refs[1][2]
        got = gd.reshape(P, P).double()
        assert bool(((got == 0) | (n > 0))[planes.to(dev())].all())
        bound = (n + 4) * U23 * (refs[0][1] + refs[1][1]) + refs[0][1] * refs[0][3][:, None] + refs[1][1] * refs[1][3][:, None]
        rd = _ratio((got - (refs[0][0] + refs[1][0])).abs(), bound)
        rd_max, rd_arg = rd.max(1).values.cpu(), rd.argmax(1).cpu()
        for j, l in enumerate(ls):
            rl = _ratio((gp[:, j].cpu() - refs[j][4]).abs(), refs[j][5]).max(1).values
            rep.add(f["r"][l], S.LIGHTS[l], rd_max, rl, rd_arg, planes)
    rep.check()


def _window_census(rs, gs, H, W):
    """Which 32 x 8 tiles of render_bwd_single_light_kernel fit their corners into the 64 x 48 LDS window and which fall
    back to the register run-merge: the box of the corner rows / columns (after the -1 wrap) of the tile's pixels with a
    sample and a non-zero upstream gradient."""
    fit = fall = 0
    for r, g in zip(rs, gs):
        rows = torch.div(r.term_idx[..., :4], W, rounding_mode="floor")
        cols = r.term_idx[..., :4] % W
        have = r.live & (g != 0)
        for r0 in range(0, H, 8):
            for c0 in range(0, W, 32):
                h = have[r0:r0 + 8, c0:c0 + 32]
                if not bool(h.any()):
                    continue
                rr, cc = rows[r0:r0 + 8, c0:c0 + 32][h], cols[r0:r0 + 8, c0:c0 + 32][h]
                if int(rr.max() - rr.min()) < 48 and int(cc.max() - cc.min()) < 64:
                    fit += 1
                else:
                    fall += 1
    return fit, fall


@pytest.mark.parametrize("H,W,N", S.SIZES)
def test_dense_fields_all_three_routes(H, W, N):
    """B = 2 (the smooth and the rough depth), a dense random cotangent, per TEXEL: gcfr_shadow_bwd with all ten lights
    per image, gcfr_render_bwd with L = 1 (ten launches' worth of images in one: B = 20) and with L = 10.  At W = 72 the
    single-light kernel's corner window and its run-merge fallback are both taken (72 % 16 = 8: the run key's old failure);
    at W = 48 every tile fits the window."""
    fs = [forward(H, W, N, kind) for kind in S.DEPTHS]
    L, P = len(S.LIGHTS), H * W
    rng = np.random.default_rng(41)
    cots = [[_fused_cotangent(f, l, rng) for l in range(L)] for f in fs]
    depth = torch.stack([f["depth"] for f in fs])
    pt = torch.stack([f["light_pt"] for f in fs])
    am = torch.stack([f["am"] for f in fs]).contiguous()
    md = torch.stack([f["md"] for f in fs]).contiguous()
    tt = fs[0]["tt"]

    def reference(b, ls, fused):
        """signed field, bound and light references of image b over the lights ls"""
        ref, S_, n, xs = 0.0, 0.0, 0.0, 0.0
        lref, lbound = [], []
        for l in ls:
            g_w, g, extra, keep = cots[b][l]
            gg = g * keep if fused else g_w.double() * fs[b]["live"][l]
            rg = fs[b]["r"][l].times(gg)
            sg, ab, cn = rg.scatter()
            ref, S_, n = ref + sg, S_ + ab, n + cn
            if fused:
                xs = xs + rg.scatter(weight=extra)[1]
            gc, mag = rg.light()
            lref.append(gc)
            lbound.append(U22 * mag + (rg.light(weight=extra)[1] if fused else 0.0))
        return ref, (n + 4) * U23 * S_ + xs, n, torch.stack(lref), torch.stack(lbound)

    def check(route, gd, gp, b, ls, fused):
        ref, bound, n, lref, lbound = reference(b, ls, fused)
        got = gd.cpu().double()
        assert bool(((got == 0) | (n > 0)).all()), route
        err = (got - ref).abs()
        ratio = torch.where(bound > 0, err / bound, (err > 0).double() * 2.0)
        rl = torch.where(lbound > 0, (gp.cpu() - lref).abs() / lbound, torch.zeros(()))
        worst.setdefault(route, [0.0, 0.0])
        worst[route] = [max(worst[route][0], float(ratio.max())), max(worst[route][1], float(rl.max()))]
        tx = int(ratio.argmax())
        assert float(ratio.max()) <= 1.0, "%s, %s depth, lights %s: texel (%d, %d) at %.3f of the bound (%d terms)" % (
            route, list(S.DEPTHS)[b], ls, tx // W, tx % W, float(ratio.max()), int(n.reshape(-1)[tx]))
        assert float(rl.max()) <= 1.0, "%s, %s depth: light gradient at %.3f of the bound, %s" % (
            route, list(S.DEPTHS)[b], float(rl.max()), S.light_name(S.LIGHTS[ls[int(rl.max(1).values.argmax())]]))

    worst = {}
    # three-kernel route: the dense upstream gradient on the distance itself
    g_md = torch.stack([torch.stack([c[0] for c in cb]) for cb in cots]).to(dev()).contiguous()
    gd, gp = shadow_bwd(g_md, depth.contiguous(), pt.contiguous(), am, N, tt)
    for b in range(2):
        check("gcfr_shadow_bwd", gd[b], gp[b], b, list(range(L)), False)
    # fused routes: the upstream gradient on the shadow weight, zero on the pixels left out
    g_w = torch.stack([torch.stack([c[0] * c[3] for c in cb]) for cb in cots]).to(dev()).contiguous()
    albedo = torch.stack([f["albedo"] for f in fs]).contiguous()
    for nrm in (torch.stack([f["normals"] for f in fs]).contiguous(), None):
        amb = torch.full((2, L), 0.45, dtype=torch.float32, device=dev())
        gd, gp = render_bwd(g_w, depth.contiguous(), albedo, pt.contiguous(), amb, md, am, nrm, N, tt, fs[0]["cam"])
        for b in range(2):
            check("gcfr_render_bwd L = %d" % L, gd[b], gp[b], b, list(range(L)), True)
    # single-light kernel: every (image, light) as an image of its own
    rep = lambda t: t[:, None].expand(2, L, *t.shape[1:]).reshape(2 * L, *t.shape[1:]).contiguous()
    gd, gp = render_bwd(g_w.reshape(2 * L, 1, H, W), rep(depth), rep(albedo), pt.reshape(2 * L, 1, 3).contiguous(),
                        torch.full((2 * L, 1), 0.45, dtype=torch.float32, device=dev()), md.reshape(2 * L, 1, H, W),
                        am.reshape(2 * L, 1, H, W), rep(torch.stack([f["normals"] for f in fs])), N, tt, fs[0]["cam"])
    for b in range(2):
        for l in range(L):
            check("gcfr_render_bwd L = 1", gd[b * L + l], gp[b * L + l], b, [l], True)
    fit, fall = _window_census([f["r"][l] for f in fs for l in range(L)], [(c[0] * c[3]) for cb in cots for c in cb], H, W)
    print("%d x %d: worst error / bound (depth per texel, light)" % (H, W), worst, "; single-light tiles in the window / fallback:", fit, fall)
    assert fit > 0 and (fall > 0 if W > 64 else fall == 0), (fit, fall)
