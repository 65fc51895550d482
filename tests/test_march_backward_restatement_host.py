"""Host validation of oracle/march_backward_restatement.py, the per-pixel f64 restatement the GPU test
tests/test_gpu_march_backward_pixels.py pins the march's backward kernels to.  Everything here runs on the CPU.

  1. the scenes of tests/march_scenes.py populate every mechanism class (conditions, not figures);
  2. the restated distance equals the oracle's d[k] up to the f32 rounding of the reference's cross product and roots;
  3. the restatement's autograd equals central differences of its own frozen f64 forward (leaves and scatter wired right);
  4. against autograd through oracle/materialised.py under a dense cotangent: reference against reference, MEASURED and
     gated at twice the measured worst (table below);
  5. the same comparison on the four smallest cases of tools/soak_backward.py --oracle's seed-0 sequence whose light
     gradient differs by more than 1e-3 -- where the soak's 2e-2 light gate comes from.

Measured, restatement against the oracle's autograd (worst over the ten lights; depth: max |difference| of the gradient
field / its max; light: max |difference| of the light-point gradient / its largest component):

    scene             depth      light
    40 x 48 smooth    3.6e-4     7.2e-5
    40 x 48 rough     1.6e-4     2.9e-4
    48 x 72 smooth    1.1e-4     4.7e-4
    48 x 72 rough     9.3e-5     1.0e-4

With the f32 tail (restate(..., tail="f32"): cross product, sums of squares, roots and quotient evaluated and
differentiated in f32 as the reference does) the same differences are listed by test_f32_tail_explains_the_difference.
"""
import importlib.util
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
import materialised as M  # noqa: E402

# twice the worst of the table above
GATE_DEPTH = 2 * 3.7e-4
GATE_LIGHT = 2 * 4.8e-4

_CACHE = {}


def scene_runs(H, W, N, kind):
    """Per light: the oracle's minimum distance, argmin, all distances, its autograd gradients under a dense random
    cotangent, and the restatement at the oracle's own argmin under the same cotangent.  Computed once per scene."""
    key = (H, W, N, kind)
    if key in _CACHE:
        return _CACHE[key]
    p = S.params(N)
    Cs = S.light_points(S.LIGHTS, p)
    depth_np, mask_np = S.scene(H, W, kind)
    depth, mask = torch.from_numpy(depth_np), torch.from_numpy(mask_np)
    rng = np.random.default_rng(5)
    runs = []
    for light, C in zip(S.LIGHTS, Cs):
        dl, Cl = depth.clone().requires_grad_(), C.clone().requires_grad_()
        v, idx, dall = M.min_distance_one(dl, mask, Cl, p, return_all=True)
        live = v.detach() < 1e5
        g = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32))
        (v * g * live).sum().backward()
        k = torch.where(live, idx, torch.full_like(idx, -1))
        runs.append(dict(light=light, C=C, k=k, live=live, g=g, d_oracle=dall.detach().gather(0, idx[None])[0],
                         grad_depth=dl.grad, grad_C=Cl.grad, r=R.restate(depth, C, k, p, g), depth=depth, p=p))
    _CACHE[key] = runs
    return runs


SCENES = [(H, W, N, kind) for (H, W, N) in S.SIZES for kind in S.DEPTHS]


@pytest.mark.parametrize("H,W,N", S.SIZES)
def test_every_mechanism_class_is_populated(H, W, N):
    for kind in S.DEPTHS:
        runs = scene_runs(H, W, N, kind)
        n = {c: sum(int(x["r"].classes[c].sum()) for x in runs) for c in R.CLASS_NAMES}
        live = sum(int(x["live"].sum()) for x in runs)
        k1 = sum(int((x["k"] >= 1).sum()) for x in runs)
        assert k1 >= 0.2 * live, (kind, k1, live)
        if kind != "smooth":
            continue
        for c in ("kind0", "kind1", "kind2", "corner_chose_y", "corner_chose_x"):
            assert n[c] >= 100, (c, n)
        assert n["wrap_col"] >= 30 and n["wrap_row"] >= 30, n
        assert n["clamp_x"] >= 1 and n["clamp_y"] >= 5, n
        assert n["own_corner"] >= 100 and n["k_first"] >= 100 and n["k_last"] >= 10, n


@pytest.mark.parametrize("H,W,N,kind", SCENES)
def test_frozen_f32_forward_is_the_oracles(H, W, N, kind):
    """The decisions are frozen from an f32 forward that must be the oracle's, bit for bit."""
    for x in scene_runs(H, W, N, kind):
        E = M._end_points(*M.pixel_grids(H, W), x["C"], H, W)
        assert torch.equal(E[0], x["r"].frozen["E32"][0]) and torch.equal(E[1], x["r"].frozen["E32"][1]), x["light"]


@pytest.mark.parametrize("H,W,N,kind", SCENES)
def test_restated_distance_matches_the_oracle(H, W, N, kind):
    """The restatement forms BA x BC, the sums of squares, the roots and the quotient in f64 from the f32 BA / BC; the
    oracle (and the reference) in f32 from the same BA / BC.  Nothing else differs, so the relative difference of d[k]
    is bounded per pixel by that f32 tail's rounding -- derivation in cross_product_f32_bound: sum_i |X_i| e_i / S + 7u
    with e_i = 2u (|a b| + |c d|) the rounding of one cross-product component; plus one u for d itself being f32."""
    worst = 0.0
    for x in scene_runs(H, W, N, kind):
        r, live = x["r"], x["live"]
        bound = R.cross_product_f32_bound(r) + 2.0 ** -24
        rel = (r.d - x["d_oracle"].double()).abs() / r.d
        ratio = (rel / bound)[live].max().item()
        worst = max(worst, ratio)
        print("%s: worst relative difference %.2e, worst difference / bound %.3f" % (S.light_name(x["light"]), rel[live].max().item(), ratio))
        assert ratio <= 1.0, (x["light"], ratio)
    assert worst > 0


@pytest.mark.parametrize("H,W,N,kind", SCENES)
def test_fused_route_exclusion_stays_under_its_cap(H, W, N, kind):
    """The fused routes leave out pixels with 1 - exp(-d) < 2^-10, at most 1 % of the live ones.  On these scenes 3 ... 6 %
    of the live pixels of every light but the overhead one lie under that threshold (first samples right beside their
    own pixel), so the cap binds: exactly the 1 % with the smallest 1 - e are left out.  Also: exp(-d) stays a normal f32."""
    for x in scene_runs(H, W, N, kind):
        d = torch.where(x["live"], x["d_oracle"], torch.ones(()))
        keep, extra, n_small = R.fused_route_pixels(R.transfer_gradient(d, torch.ones_like(d))[1], x["live"])
        live = int(x["live"].sum())
        print("%s: %d of %d live pixels under the threshold, %d left out" % (S.light_name(x["light"]), n_small, live, live - int(keep.sum())))
        assert live - int(keep.sum()) <= 0.01 * live and n_small <= 0.08 * live
        assert not bool((keep & ~x["live"]).any()) and bool(torch.isfinite(extra[x["live"]]).all())
        assert float(d[x["live"]].max()) < 80.0


def _pick_pixels(runs, per_class, rng):
    """(run index, row, col) drawn from every class over the lights that have it."""
    picks = []
    for c in R.CLASS_NAMES:
        pool = [(i, int(rr), int(cc)) for i, x in enumerate(runs) for rr, cc in torch.nonzero(x["r"].classes[c]).tolist()]
        for j in rng.permutation(len(pool))[:per_class]:
            picks.append(pool[j] + (c,))
    return picks


@pytest.mark.parametrize("H,W,N", S.SIZES)
def test_autograd_equals_central_differences_of_the_frozen_forward(H, W, N):
    """64 (light, pixel) pairs drawn from every class (smooth and rough depth alternating): central differences of
    Restated.forward -- the frozen f64 function itself, same decisions and same f32 offsets -- in each depth texel the
    pixel touches (through the depth IMAGE, so coincident texels and the scatter's indices are exercised) and in the
    light point.  Step: 1e-3 of the pixel's own curvature scale num / (|BA|_1 + |BC|_1) (a depth texel moves BA_z and
    BC_z, so X moves by up to h (|BA|_1 + |BC|_1) against |X| <= num) resp. num / |BA|_1 for the light, at most 1e-3.
    Tolerance: truncation (relative step)^2 = 1e-6 of the term magnitudes, times 10;  rounding 2^-53 R / h with
    R = (H + W + max depth) |BC|_1 / den, times 4: the coordinates and depths that BA is the difference of carry
    2^-53 of THEIR magnitude (at most H + W + max depth together), and the cross product multiplies that by |BC|."""
    rng = np.random.default_rng(3)
    picks = []
    for kind, n in (("smooth", 3), ("rough", 3)):
        picks += [(kind,) + q for q in _pick_pixels(scene_runs(H, W, N, kind), n, rng)]
    picks = picks[:64] if len(picks) > 64 else picks
    assert len(picks) >= 60 and {q[4] for q in picks} == set(R.CLASS_NAMES)
    worst = 0.0
    for kind, i, rr, cc, cname in picks:
        x = scene_runs(H, W, N, kind)[i]
        r1 = _unit(x)
        f = r1.frozen
        BA1 = sum(v.detach()[rr, cc].abs() for v in f["BA"]).item()
        BC1 = sum(v.detach()[rr, cc].abs() for v in f["BC"]).item()
        den = float(torch.sqrt(sum(v.detach()[rr, cc] ** 2 for v in f["BC"]) + 1e-4))
        num = r1.d[rr, cc].item() * den
        Rr = (H + W + float(f["depth64"].max())) * BC1 / den
        one = torch.zeros(H, W, dtype=torch.bool)
        one[rr, cc] = True
        sg, ab, _ = r1.scatter(one)
        h = min(1e-3, 1e-3 * num / (BA1 + BC1))
        for tx in sorted(set(r1.term_idx[rr, cc].tolist())):
            Z = f["depth64"].clone().reshape(-1)
            Z[tx] += h
            a = r1.forward(depth64=Z.reshape(H, W))[rr, cc]
            Z[tx] -= 2 * h
            b = r1.forward(depth64=Z.reshape(H, W))[rr, cc]
            fd, ad = ((a - b) / (2 * h)).item(), sg.reshape(-1)[tx].item()
            tol = 1e-5 * ab.reshape(-1)[tx].item() + 4 * 2.0 ** -53 * Rr / h
            worst = max(worst, abs(fd - ad) / tol)
            assert abs(fd - ad) <= tol, (S.describe_term("depth texel %d" % tx, [cname], x["light"]), (rr, cc), fd, ad, tol)
        h = min(1e-3, 1e-3 * num / BA1)
        for j in range(3):
            e = torch.zeros(3, dtype=torch.float64)
            e[j] = h
            fd = ((r1.forward(C64=f["C64"] + e)[rr, cc] - r1.forward(C64=f["C64"] - e)[rr, cc]) / (2 * h)).item()
            ad = r1.gC[rr, cc, j].item()
            tol = 1e-5 * r1.gC_mag[rr, cc, j].item() + 4 * 2.0 ** -53 * Rr / h
            worst = max(worst, abs(fd - ad) / tol)
            assert abs(fd - ad) <= tol, (S.describe_term("light point component %d" % j, [cname], x["light"]), (rr, cc), fd, ad, tol)
    print("worst |central difference - autograd| / tolerance: %.3f" % worst)


def _unit(x):
    """The run's restatement under a unit cotangent (cached on the run)."""
    if "r1" not in x:
        x["r1"] = R.restate(x["depth"], x["C"], x["k"], x["p"])
    return x["r1"]


def _against_oracle(x, r):
    gd, gC = x["grad_depth"].double(), x["grad_C"].double()
    e_depth = ((r.scatter()[0] - gd).abs().max() / gd.abs().max()).item()
    e_light = ((r.light()[0] - gC).abs().max() / gC.abs().max()).item()
    return e_depth, e_light


@pytest.mark.parametrize("H,W,N,kind", SCENES)
def test_gradients_against_the_oracles_autograd(H, W, N, kind):
    """Reference against reference: the oracle's autograd forms the tail in f32, the restatement in f64.  Measured (module
    docstring), gated at twice the measured worst."""
    worst_d = worst_l = 0.0
    for x in scene_runs(H, W, N, kind):
        e_depth, e_light = _against_oracle(x, x["r"])
        print("%s: depth %.2e light %.2e" % (S.light_name(x["light"]), e_depth, e_light))
        worst_d, worst_l = max(worst_d, e_depth), max(worst_l, e_light)
    print("%d x %d %s: worst depth %.2e, worst light %.2e" % (H, W, kind, worst_d, worst_l))
    assert worst_d <= GATE_DEPTH and worst_l <= GATE_LIGHT, (worst_d, worst_l)


def test_f32_tail_explains_the_difference():
    """The restatement with the reference's f32 tail (everything in front of BA / BC unchanged) on the worst scene of each
    quantity.  DEPTH: the whole difference is that f32 tail -- 3.6e-4 with the f64 tail, 1.4e-7 with the f32 one (asserted:
    a hundred times better).  LIGHT: about half -- 2.9e-4 against 1.5e-4; the rest is the slope / intercept chain, which
    the reference's autograd evaluates in f32 too (test_soak_light_gate_cases); asserted only not to get worse."""
    H, W, N = S.SIZES[0]
    for kind, li, what in (("smooth", 6, 0), ("rough", 9, 1)):      # the worst depth resp. light rows of 40 x 48
        x = scene_runs(H, W, N, kind)[li]
        e64 = _against_oracle(x, x["r"])[what]
        e32 = _against_oracle(x, R.restate(x["depth"], x["C"], x["k"], x["p"], x["g"], tail="f32"))[what]
        print("%s %s, %s gradient: f64 tail %.2e, f32 tail %.2e" % (kind, S.light_name(x["light"]), ("depth", "light")[what], e64, e32))
        assert e32 <= (0.01 if what == 0 else 1.0) * e64, (e64, e32)


# ---------------------------------------------------------------------------------------------------------------------
# tools/soak_backward.py --oracle, seed 0: where its light gate comes from
# ---------------------------------------------------------------------------------------------------------------------
def _soak_module():
    spec = importlib.util.spec_from_file_location("soak_backward", os.path.join(ROOT, "tools", "soak_backward.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def soak_oracle_sequence(seed, n):
    """The inputs of `tools/soak_backward.py --oracle n --seed seed`, case by case: the same draws in the same order."""
    soak = _soak_module()
    rng = np.random.default_rng(seed)
    for it in range(n):
        B = int(rng.integers(1, 3))
        H, W = 2 * int(rng.integers(8, 25)), 2 * int(rng.integers(8, 25))
        N = int(rng.integers(8, 41))
        depth, mask, albedo = soak.random_inputs(rng, B, H, W)
        f, zoff = float(rng.uniform(300, 2000)), float(rng.uniform(100, 2000))
        light = rng.standard_normal((B, 3)).astype(np.float32)
        light[:, 2] = np.abs(light[:, 2]) + 0.05
        amb = (0.3 + 0.4 * rng.random(B)).astype(np.float32)
        G = {k: rng.standard_normal(s_).astype(np.float32) for k, s_ in
             [("shadow_mask_weights", (B, H, W)), ("final_shading", (B, H, W)), ("rendered_images", (B, 3, H, W))]}
        yield dict(case=it, B=B, H=H, W=W, N=N, depth=depth, mask=mask, albedo=albedo, f=f, zoff=zoff, light=light, amb=amb, G=G,
                   K=soak.camera(f, H, W, "cpu"))


def soak_light_difference(c, tail="f64", details=False):
    """The soak's light figure for one case with the RESTATEMENT in the kernels' place: the oracle's autograd of the whole
    block gives dLoss/d minimum_distance and the total raw-light gradient; the march's share of it is replaced by the
    restatement's (through the f64 Jacobian of the light preparation), and the difference is measured as the soak does,
    max |difference| / (max |oracle| + 2e-4 B H W).  Only the march's backward differs between the two."""
    from normals_restatement import depth_to_normals as oracle_normals
    B, H, W, N = c["B"], c["H"], c["W"], c["N"]
    p = M.BlockParams(n_samples=N, t0=0.025, dt=0.8 / N)
    cl = [torch.from_numpy(x).clone().requires_grad_() for x in (c["depth"][:, None], c["albedo"], c["light"], c["amb"])]
    n = oracle_normals(cl[0] + c["zoff"], c["K"])
    n = torch.cat([n[:, 0:1], -n[:, 1:2], n[:, 2:3]], 1)
    mask = torch.from_numpy(c["mask"])
    o = M.render_block(cl[0], cl[1], cl[2], cl[3], n, mask, p)
    o["minimum_distance"].retain_grad()
    sum((o[k].reshape(g.shape) * torch.from_numpy(g)).sum() for k, g in c["G"].items()).backward()
    g_md = o["minimum_distance"].grad
    light64 = torch.from_numpy(c["light"]).double().requires_grad_()
    C64 = M.light_points(light64, p)[1]
    C32 = M.light_points(torch.from_numpy(c["light"]), p)[1]
    dC, rows = [], []
    for i in range(B):
        Cl = C32[i].clone().requires_grad_()
        v, idx = M.min_distance_one(torch.from_numpy(c["depth"][i]), mask[i], Cl, p)
        (v * g_md[i]).sum().backward()
        k = torch.where(v.detach() < 1e5, idx, torch.full_like(idx, -1))
        r = R.restate(torch.from_numpy(c["depth"][i]), C32[i], k, p, g_md[i], tail=tail)
        dC.append(r.light()[0] - Cl.grad.double())
        if details:
            # per-pixel light-point gradients of the ORACLE (one batched autograd pass), to see which pixels differ
            Cp = C32[i].clone().requires_grad_()
            vp, _ = M.min_distance_one(torch.from_numpy(c["depth"][i]), mask[i], Cp, p)
            (J,) = torch.autograd.grad(vp.reshape(-1), Cp, torch.eye(vp.numel()), is_grads_batched=True)
            J = J.reshape(H, W, 3).double() * g_md[i].double()[..., None]
            r32 = R.restate(torch.from_numpy(c["depth"][i]), C32[i], k, p, g_md[i], tail="f32")
            per_pixel = ((r.gC - J).abs() * r.live[..., None]).sum(-1)
            for t in torch.argsort(per_pixel.reshape(-1), descending=True)[:3].tolist():
                rr, cc = divmod(t, W)
                rows.append(dict(image=i, pixel=(rr, cc), kind=int(r.frozen["kind"][rr, cc]), d=float(r.d[rr, cc]),
                                 slope=float(r.frozen["m32"][rr, cc]), pden=float(r.frozen["pden32"][rr, cc]),
                                 difference=float(per_pixel[rr, cc]), share_of_image=float(per_pixel[rr, cc] / per_pixel.sum()),
                                 of_which_f32_tail=float((r.gC - r32.gC)[rr, cc].abs().sum())))
    (dlight,) = torch.autograd.grad(C64, light64, torch.stack(dC))
    e = float(dlight.abs().max()) / (float(cl[2].grad.abs().max()) + 2e-4 * B * H * W)
    return (e, rows) if details else e


# Cases of the seed-0 sequence.  NONE of its first 1000 cases needs a light gate above 1e-3 by this measure: the worst is
# 8.7e-4 (case 163), and 53 cases exceed 1e-4.  These are the four largest.
SOAK_CASES = {163: 8.7e-4, 565: 4.8e-4, 353: 4.6e-4, 649: 4.3e-4}


def test_soak_light_gate_cases():
    """Verdict on the comment in tools/soak_backward.py ("near-vertical rays ... which the reference's autograd evaluates in
    f32 and the kernels' chain rule in f64"): CONFIRMED for the largest case, and the f32 cross product is ruled out for
    all four.  The light figure is unchanged to three digits when the restatement takes the reference's f32 tail (that
    tail explains the DEPTH difference instead, test_f32_tail_explains_the_difference); per pixel the tail's share of
    the difference is below 1 %.  Case 163 (8.7e-4): the light's projection lies 0.055 px from pixel column 4 of its
    second image, slopes of -7.2e4, end point through the y candidate; three pixels of that column carry 31 %, 31 % and
    11 % of the image's difference, all of it in the x component, which passes through m and ic alone.  Cases 353, 565,
    649 (4e-4 ... 5e-4): no ill-conditioned pixel (|C_x - x| of 1e3, slopes below 2); differences of 1e-8 per pixel
    spread over the image, against a light gradient whose sum nearly cancels (the soak's floor 2e-4 B H W is most of
    the denominator) -- the f32 evaluation of the same slope / intercept chain, without the amplification."""
    for c in soak_oracle_sequence(0, max(SOAK_CASES) + 1):
        if c["case"] not in SOAK_CASES:
            continue
        e64, rows = soak_light_difference(c, "f64", details=True)
        e32 = soak_light_difference(c, "f32")
        print("case %d (B %d, %d x %d, N %d): light figure %.2e with the f64 tail, %.2e with the reference's f32 tail" %
              (c["case"], c["B"], c["H"], c["W"], c["N"], e64, e32))
        for row in rows:
            print("   ", row)
        # (the recorded figure moves with the last bit of the oracle's f32 sums: the claims are "above 1e-4, not above 1e-3, near
        # the recorded value" and "the f32 tail does not change it")
        assert 1e-4 < e64 <= 1e-3 and 0.5 * SOAK_CASES[c["case"]] <= e64 <= 1.5 * SOAK_CASES[c["case"]], e64
        assert abs(e32 - e64) <= 0.05 * e64, (e64, e32)
        top = max(rows, key=lambda q: q["difference"])
        assert top["of_which_f32_tail"] <= 0.01 * top["difference"], top
        if c["case"] == 163:
            assert abs(top["pden"]) < 1.0 and abs(top["slope"]) > 1e4 and top["share_of_image"] > 0.25, top
