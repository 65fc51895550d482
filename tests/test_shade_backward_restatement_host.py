"""Host validation of oracle/shade_backward_restatement.py, the per-pixel f64 restatement that
tests/test_gpu_shade_backward_pixels.py pins the shading and normals-stencil backward kernels to.  CPU only.

  1. the restatement's per-pixel terms, summed per texel and per light, against DENSE f64 autograd through
     materialised.render_block and normals_restatement.depth_to_normals (the march replaced by the synthetic minimum distances):
     1e-12 relative to the magnitudes; central differences of the frozen f64 function on pixels of every class;
  2. every pixel class is populated at the shape that is supposed to populate it; near-kink pixels are at most 1 % of each
     scene, lit and unlit at least 5 % each under the low light;
  3. the measurement that fixes the fused kernels' f32 gates: the reference's own f32 autograd (the oracle port's shading lines,
     T8:364-369 and 517-522 op for op, with f32 per-pixel leaves -- checked against materialised.render_block's dense f32
     autograd first) against the restatement, per output kind, as a ratio to 2^-24 magnitude.  Printed; the gate constants
     derived from it are shade_backward_restatement.F32_MEASURED / F32_GATE.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import materialised as M  # noqa: E402
import normals_restatement as NR  # noqa: E402
import shade_backward_restatement as R  # noqa: E402
import shade_scenes as S  # noqa: E402

ALL_SHAPES = S.FUSED_SHAPES + S.ODD_SHAPES
NO_SAMPLE = 1000000.0          # T8:512 (the GPU test reads the product's value from a forward run)
_CACHE = {}


def camera(f, H, W, dtype=torch.float64):
    K = torch.zeros(1, 3, 3, dtype=dtype)
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 2, 2] = 1.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    return K


def host_normals(depth, f, off, H, W):
    """the f64 restatement's normals, y negated, rounded to f32: (3,H,W)"""
    n = NR.depth_to_normals((depth + torch.tensor(off, dtype=torch.float32)).double()[None, None], camera(f, H, W))[0]
    return torch.stack([n[0], -n[1], n[2]]).float()


def scene(H, W, L, cam=S.CAMERA):
    key = (H, W, L, cam)
    if key not in _CACHE:
        depth = torch.from_numpy(S.depth(H, W))
        albedo, amb, md = S.inputs(H, W, L, NO_SAMPLE)
        normals = S.plant_zero_normals(host_normals(depth, cam[0], cam[1], H, W), H, W)
        _CACHE[key] = dict(H=H, W=W, L=L, depth=depth, albedo=albedo, amb=amb, md=md, normals=normals, C=S.light_points(L),
                           cots=S.cotangents(H, W, L), cam=cam)
    return _CACHE[key]


def restated(sc, **kw):
    return R.restate_shading(sc["depth"], sc["normals"], sc["albedo"], sc["C"], sc["amb"], sc["md"], S.INTENSITY, sc["cots"], **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. against dense f64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def dense_autograd(sc, dtype, monkeypatch, normals_from_depth):
    """Autograd through materialised.render_block, one image per light, with the march replaced by the scene's synthetic
    minimum distances and the light point a leaf.  normals_from_depth: the normals come from normals_restatement (their
    gradient reaches the depth, and g_normals_out acts on them); otherwise the scene's normals are a leaf.
    -> dict of gradients: depth (H,W), normals (3,H,W), albedo (3,H,W), C (L,3), amb (L,), md (L,H,W)."""
    H, W, L = sc["H"], sc["W"], sc["L"]
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    depth, albedo, C, amb, md = [leaf(sc[k]) for k in ("depth", "albedo", "C", "amb", "md")]
    if normals_from_depth:
        f, off = sc["cam"]
        D = (sc["depth"] + torch.tensor(off, dtype=torch.float32)).to(dtype) + (depth - depth.detach())     # the f32 sum, slope 1
        n = NR.depth_to_normals(D[None, None], camera(f, H, W, dtype))[0]
        normals = torch.stack([n[0], -n[1], n[2]])
        loss = (normals * sc["cots"]["g_normals_out"].to(dtype)).sum()
    else:
        normals = leaf(sc["normals"])
        loss = 0.0
    state = {"l": 0}
    monkeypatch.setattr(M, "light_points", lambda light, p: (F.normalize(light, dim=1), C[state["l"]][None]))
    monkeypatch.setattr(M, "min_distance_one", lambda d, mk, Cl, p: (md[state["l"]], None))
    prm = M.BlockParams(directional_intensity=S.INTENSITY)
    for l in range(L):
        state["l"] = l
        o = M.render_block(depth[None, None], albedo[None], torch.ones(1, 3, dtype=dtype), amb[l:l + 1], normals[None],
                           torch.ones(1, H, W), prm)
        c = sc["cots"]
        loss = loss + (o["shadow_mask_weights"][0] * c["g_w"][l].to(dtype)).sum() + (o["full_shading"][0] * c["g_full"][l].to(dtype)).sum() \
            + (o["final_shading"][0] * c["g_final"][l].to(dtype)).sum() + (o["rendered_images"][0] * c["g_rendered"][l].to(dtype)).sum()
    loss.backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(depth=z(depth), normals=None if normals_from_depth else z(normals), albedo=z(albedo), C=z(C), amb=z(amb), md=z(md))


def composed_depth_field(sc, sh, negate_y=True):
    """grad_depth of the whole shading + stencil backward from the restatement: own-depth terms plus the stencil's terms under
    the gradient on the normal (all lights) + g_normals_out.  -> (field (H,W), magnitude (H,W))"""
    H, W = sc["H"], sc["W"]
    f, off = sc["cam"]
    J = R.restate_stencil(sc["depth"], f, f, W / 2.0, H / 2.0, off, negate_y)
    g = sh.val["normal"].sum(0) + sc["cots"]["g_normals_out"].double().permute(1, 2, 0)
    gm = sh.mag["normal"].sum(0) + sc["cots"]["g_normals_out"].double().abs().permute(1, 2, 0)
    t = J.terms(g)
    field, _, _, _ = R.scatter_terms(t, H, W)
    magf = torch.zeros(H * W, dtype=torch.float64).index_add_(0, t.idx.reshape(-1), (J.Jabs * gm.permute(2, 0, 1)[..., None]).sum(0).reshape(-1))
    return field + sh.val["own_depth"].sum(0), magf.reshape(H, W) + sh.mag["own_depth"].sum(0)


@pytest.mark.parametrize("H,W", ALL_SHAPES)
@pytest.mark.parametrize("L", [1, 3])
def test_per_pixel_terms_sum_to_dense_f64_autograd(H, W, L, monkeypatch):
    sc = scene(H, W, L)
    sh = restated(sc, exp_in_f32=False)
    worst = {}

    def cmp(name, got, mag, ref):
        err = (got - ref.double()).abs()
        assert bool((err <= 1e-12 * mag).all()), (name, float((err / mag.clamp_min(1e-300)).max()))
        worst[name] = float((err / mag.clamp_min(1e-300)).max())

    a = dense_autograd(sc, torch.float64, monkeypatch, normals_from_depth=False)
    cmp("albedo", sh.val["albedo"].sum(0).permute(2, 0, 1), sh.mag["albedo"].sum(0).permute(2, 0, 1), a["albedo"])
    # a planted zero-vector normal has n.l = 0 exactly: torch.maximum's backward splits a tie in halves, so dense autograd returns
    # HALF of the lit side's gradient there, (dn / 1e-12) / 2 -- neither frozen side.  Those pixels are compared with that.
    tie = (sh.dot == 0).any(0)
    assert int(tie.sum()) == len(S.planted(H, W)[3])
    lit_side = restated(sc, exp_in_f32=False, lit=sh.lit | (sh.dot == 0))
    n_val = torch.where(tie[..., None], 0.5 * lit_side.val["normal"].sum(0), sh.val["normal"].sum(0))
    n_mag = torch.where(tie[..., None], lit_side.mag["normal"].sum(0), sh.mag["normal"].sum(0))
    if bool(tie.any()):
        assert float(n_val[tie].abs().max()) > 1e9         # the 1e-12 clamp: dn / 1e-12
    cmp("normal", n_val.permute(2, 0, 1), n_mag.permute(2, 0, 1), a["normals"])
    cmp("min_dist", sh.val["min_dist"], sh.mag["min_dist"], a["md"])
    cmp("own depth", sh.val["own_depth"].sum(0), sh.mag["own_depth"].sum(0), a["depth"])
    cmp("light", sh.val["light"].sum((1, 2)), sh.mag["light"].sum((1, 2)), a["C"])
    cmp("ambient", sh.val["ambient"].sum((1, 2)), sh.mag["ambient"].sum((1, 2)), a["amb"])
    # the whole chain through the stencil: zero-vector normals cannot be planted when the normals come from the depth
    sc2 = dict(sc, normals=host_normals(sc["depth"], sc["cam"][0], sc["cam"][1], H, W))
    # (the dense graph's normals are f64: the restatement is evaluated at those, not at their f32 rounding)
    n64 = NR.depth_to_normals((sc["depth"] + torch.tensor(sc["cam"][1], dtype=torch.float32)).double()[None, None], camera(sc["cam"][0], H, W))[0]
    sh2 = restated(dict(sc2, normals=torch.stack([n64[0], -n64[1], n64[2]])), exp_in_f32=False)
    b = dense_autograd(sc2, torch.float64, monkeypatch, normals_from_depth=True)
    field, mag = composed_depth_field(sc2, sh2)
    cmp("depth through the stencil", field, mag, b["depth"])
    print("%d x %d, L = %d: worst |restatement - dense f64 autograd| / magnitude" % (H, W, L), {k: "%.1e" % v for k, v in worst.items()})


@pytest.mark.parametrize("H,W", [(3, 5), (10, 34)])
def test_autograd_equals_central_differences_of_the_frozen_function(H, W):
    """A handful of pixels of every class: central differences of the frozen f64 function (Lambert side frozen, e in f64) in
    every input of the pixel -- normal, albedo, minimum distance, ambient, light point, own depth -- and, for the stencil, in
    every depth texel of the pixel's neighbourhood.  Step 1e-6 of the input's scale (1e-2 for the light point and the own depth,
    which move a vector 4e3 long); tolerance 1e-7 of the magnitude (truncation) plus 8 x 2^-53 x 10 / h (the loss's rounding)."""
    L = 3
    sc = scene(H, W, L)
    sh = restated(sc, exp_in_f32=False)
    cls = R.pixel_classes(H, W)
    rng = np.random.default_rng(2)
    picks = set()
    for name, m in cls.items():
        pool = torch.nonzero(m).tolist()
        for j in rng.permutation(len(pool))[:2]:
            picks.add(tuple(pool[j]))
    xx, yy = M.pixel_grids(H, W)
    c = sc["cots"]

    def loss(l, r, cc, n, alb, d, amb, C, zb):
        P = torch.stack([xx[r, cc].double(), yy[r, cc].double(), zb])
        u, nh = F.normalize(C - P, dim=0), n / n.norm().clamp_min(1e-12)
        dot = (u * nh).sum()
        full = amb + S.INTENSITY * (dot if bool(sh.lit[l, r, cc]) else 0.0)
        e = torch.exp(-d)
        w = 1 - 4 * e / (1 + e) ** 2
        fin = w * full + (1 - w) * amb
        return (c["g_w"][l, r, cc] * w + c["g_full"][l, r, cc] * full + c["g_final"][l, r, cc] * fin
                + (c["g_rendered"][l, :, r, cc].double() * alb * fin).sum())

    worst = 0.0
    for (r, cc) in sorted(picks):
        for l in range(L):
            if float(sc["normals"][:, r, cc].abs().max()) == 0.0 or float(sc["md"][l, r, cc]) > 100:
                continue
            x0 = [sc["normals"][:, r, cc].double(), sc["albedo"][:, r, cc].double(), sc["md"][l, r, cc].double(), sc["amb"][l].double(),
                  sc["C"][l].double(), sc["depth"][r, cc].double()]
            ref = [(sh.val["normal"][l, r, cc], sh.mag["normal"][l, r, cc]), (sh.val["albedo"][l, r, cc], sh.mag["albedo"][l, r, cc]),
                   (sh.val["min_dist"][l, r, cc], sh.mag["min_dist"][l, r, cc]), (sh.val["ambient"][l, r, cc], sh.mag["ambient"][l, r, cc]),
                   (sh.val["light"][l, r, cc], sh.mag["light"][l, r, cc]), (sh.val["own_depth"][l, r, cc], sh.mag["own_depth"][l, r, cc])]
            for i, (x, (val, mag)) in enumerate(zip(x0, ref)):
                flat = x.reshape(-1)
                for j in range(flat.numel()):
                    h = 1e-2 if i >= 4 else 1e-6 * max(1.0, float(flat.abs().max()))     # light point, own depth: |l| is 4e3
                    rnd = 8 * 2.0 ** -53 * 10.0 / h                                      # the loss is a sum of six terms of O(1)
                    ev = lambda s: loss(l, r, cc, *[(xi if k != i else (flat + s * h * torch.eye(flat.numel(), dtype=torch.float64)[j]).reshape(x.shape))
                                                    for k, xi in enumerate(x0)])
                    fd = float((ev(1.0) - ev(-1.0)) / (2 * h))
                    ad, mg = float(val.reshape(-1)[j]), float(mag.reshape(-1)[j])
                    worst = max(worst, abs(fd - ad) / (1e-7 * mg + rnd))
                    assert abs(fd - ad) <= 1e-7 * mg + rnd, ((r, cc), l, i, j, fd, ad, mg)
    # stencil: d(sum_i g_i n_i at the pixel) / d(depth texel), through the dense f64 normals
    f, off = sc["cam"]
    for negate_y in (True, False):
        J = R.restate_stencil(sc["depth"], f, f, W / 2.0, H / 2.0, off, negate_y)
        g = c["g_normals_out"].permute(1, 2, 0)
        t = J.terms(g)
        D0 = (sc["depth"] + torch.tensor(off, dtype=torch.float32)).double()

        def nrm(D, r, cc):
            n = NR.depth_to_normals(D[None, None], camera(f, H, W))[0, :, r, cc]
            return float((n * torch.tensor([1.0, -1.0 if negate_y else 1.0, 1.0], dtype=torch.float64) * g[r, cc].double()).sum())

        for (r, cc) in sorted(picks):
            for tx in sorted(set(t.idx[r, cc].tolist())):
                sel = t.idx[r, cc] == tx
                ad, mg = float(t.val[r, cc][sel].sum()), float(t.mag[r, cc][sel].sum())
                h = 1e-4
                Dp, Dm = D0.clone().reshape(-1), D0.clone().reshape(-1)
                Dp[tx] += h
                Dm[tx] -= h
                fd = (nrm(Dp.reshape(H, W), r, cc) - nrm(Dm.reshape(H, W), r, cc)) / (2 * h)
                worst = max(worst, abs(fd - ad) / (1e-6 * mg))
                assert abs(fd - ad) <= 1e-6 * mg, ("stencil", negate_y, (r, cc), tx, fd, ad, mg)
    print("%d x %d: %d pixels, worst |central difference - autograd| / tolerance %.3f" % (H, W, len(picks), worst))


# ---------------------------------------------------------------------------------------------------------------------
# 2. classes and kink shares
# ---------------------------------------------------------------------------------------------------------------------
# class -> the smallest shapes that must populate it
POPULATED_AT = {
    "image corner": ALL_SHAPES, "top edge": ALL_SHAPES[1:], "bottom edge": ALL_SHAPES[1:], "left edge": ALL_SHAPES[1:],
    "right edge": ALL_SHAPES[1:], "image interior": ALL_SHAPES[1:],
    "tile corner": ALL_SHAPES, "tile edge row": ALL_SHAPES, "tile edge column": [(8, 32), (10, 34), (18, 66), (9, 33)],
    "tile interior": [(8, 32), (10, 34), (18, 66), (3, 5), (9, 33)], "partial tile": [(2, 2), (10, 34), (18, 66), (3, 5), (9, 33)],
}


@pytest.mark.parametrize("H,W", ALL_SHAPES)
def test_every_class_is_populated_where_it_should_be(H, W):
    cls = R.pixel_classes(H, W)
    n = {k: int(v.sum()) for k, v in cls.items()}
    print("%d x %d:" % (H, W), n)
    for k, shapes in POPULATED_AT.items():
        if (H, W) in shapes:
            assert n[k] > 0, (k, n)
    assert sum(n[k] for k in R.IMAGE_CLASSES) == H * W and sum(n[k] for k in R.TILE_CLASSES[:4]) == H * W
    if (H, W) == (2, 2):
        assert n["image corner"] == 4
    if (H, W) == (8, 32):
        assert n["partial tile"] == 0
    if (H, W) == (18, 66):      # a 3 x 3 tile grid with one whole interior tile
        whole = ~cls["partial tile"]
        assert int(whole[8:16, 32:64].sum()) == 256 and n["partial tile"] == H * W - 2 * 2 * 256


@pytest.mark.parametrize("H,W,cam", [(H, W, S.CAMERA) for (H, W) in ALL_SHAPES] + [(10, 34, S.PRODUCT_CAMERA)])
def test_kink_shares(H, W, cam):
    """near-kink pixels at most 1 % of each scene (planted zero-vector normals included: their dot product is 0); under the low
    light lit and unlit are at least 5 % each wherever the image has an interior."""
    sc = scene(H, W, 3, cam)
    sh = restated(sc)
    k = R.kink_classes(sh.dot)
    n = {name: [int(v[l].sum()) for l in range(3)] for name, v in k.items()}
    print("%d x %d, f = %g: per light" % (H, W, cam[0]), n)
    P = H * W
    for l in range(3):
        assert n["near kink"][l] <= 0.01 * P, n
    assert n["near kink"][0] >= len(S.planted(H, W)[3])
    if P >= 15:
        assert n["lit"][0] >= 0.05 * P and n["unlit"][0] >= 0.05 * P, n
    one_minus_e = sh.one_minus_e
    assert int((one_minus_e < R.SMALL_1ME).sum()) <= 0.01 * 3 * P


# ---------------------------------------------------------------------------------------------------------------------
# 3. the reference's f32 noise
# ---------------------------------------------------------------------------------------------------------------------
def port_f32_per_pixel(sc):
    """The oracle port's shading lines (materialised.render_block, T8:364-369, 517-522) op for op in f32 on per-(light, pixel)
    leaves: every (light, pixel) is a batch element of its own.  -> gradients with the restatement's shapes."""
    H, W, L = sc["H"], sc["W"], sc["L"]
    xx, yy = M.pixel_grids(H, W)
    ex = lambda t: t[None].expand(L, *t.shape).reshape(L * H * W, -1)
    pts = torch.stack([xx, yy, sc["depth"]], -1)                                                  # T8:356
    leaf = lambda t: t.detach().clone().contiguous().requires_grad_()
    pts_l = leaf(ex(pts))
    Cmap = leaf(sc["C"][:, None, :].expand(L, H * W, 3).reshape(-1, 3))
    normals = leaf(ex(sc["normals"].permute(1, 2, 0)))
    albedo = leaf(ex(sc["albedo"].permute(1, 2, 0)))
    amb = leaf(sc["amb"][:, None].expand(L, H * W).reshape(-1))
    md = leaf(sc["md"].reshape(-1))
    inc = F.normalize(Cmap - pts_l, p=2, dim=1)                                                   # T8:364
    nrm = F.normalize(normals, p=2, dim=1)                                                        # T8:365
    directional = S.INTENSITY * torch.maximum(torch.sum(nrm * inc, dim=1), torch.tensor([0.0]))
    full = amb + directional                                                                      # T8:369
    w = M.shadow_transfer(md)                                                                     # T8:517
    final = w * full + (1 - w) * amb                                                              # T8:518
    rendered = albedo * final[:, None]                                                            # T8:519-522
    c = sc["cots"]
    (w * c["g_w"].reshape(-1) + full * c["g_full"].reshape(-1) + final * c["g_final"].reshape(-1)
     + (rendered * c["g_rendered"].permute(0, 2, 3, 1).reshape(-1, 3)).sum(1)).sum().backward()
    sh3, sh1 = (L, H, W, 3), (L, H, W)
    return dict(albedo=albedo.grad.reshape(sh3), normal=normals.grad.reshape(sh3), light=Cmap.grad.reshape(sh3), min_dist=md.grad.reshape(sh1),
                ambient=amb.grad.reshape(sh1), own_depth=pts_l.grad[:, 2].reshape(sh1), own_depth_from_light=-Cmap.grad[:, 2].reshape(sh1))


def reference_f32_ratios(sc):
    """worst |reference f32 autograd - restatement| / (2^-24 magnitude) per output kind; near-kink pixels excluded."""
    sh = restated(sc)
    g32 = port_f32_per_pixel(sc)
    ok = ~R.kink_classes(sh.dot)["near kink"]
    out = {}
    for k in R.OUTPUTS:
        err, mag = (g32[k].double() - sh.val[k]).abs(), sh.mag[k]
        sel = ok
        if k == "min_dist":
            sel = ok & (sh.one_minus_e >= R.SMALL_1ME)
            mag = mag * (1.0 + 1.0 / sh.one_minus_e.clamp_min(R.SMALL_1ME))
        sel = sel[..., None].expand_as(err) if err.dim() == 4 else sel
        assert bool((err[sel & (mag == 0)] == 0).all()), k
        r = torch.where(sel & (mag > 0), err / (R.U24 * mag.clamp_min(1e-300)), torch.zeros(()).double())
        out[k] = float(r.max())
    return out


def test_the_per_pixel_f32_port_is_the_oracle_ports_autograd(monkeypatch):
    """the per-pixel f32 lines above against materialised.render_block's own dense f32 autograd: the per-pixel outputs bit for
    bit, the light and ambient sums to f32 summation noise."""
    sc = scene(10, 34, 3)
    g = port_f32_per_pixel(sc)
    a = dense_autograd(sc, torch.float32, monkeypatch, normals_from_depth=False)
    assert torch.equal(g["min_dist"], a["md"])
    for l_sum, dense in ((g["albedo"].sum(0).permute(2, 0, 1), a["albedo"]), (g["normal"].sum(0).permute(2, 0, 1), a["normals"])):
        assert float((l_sum - dense).abs().max()) <= 4 * 2.0 ** -24 * float(dense.abs().max())
    assert float((g["light"].double().sum((1, 2)) - a["C"].double()).abs().max()) <= 1e-5 * float(a["C"].abs().max())
    assert float((g["ambient"].double().sum((1, 2)) - a["amb"].double()).abs().max()) <= 1e-5 * float(a["amb"].abs().max())
    assert torch.equal(g["own_depth"], g["own_depth_from_light"])


def test_reference_f32_noise_fixes_the_gates():
    """Prints the worst ratios over every scene; asserts they are finite and positive and that the module's constants are these
    measurements (F32_MEASURED is the worst over the scenes, rounded up to two digits; F32_GATE four times that)."""
    worst = {k: 0.0 for k in R.OUTPUTS}
    for (H, W) in ALL_SHAPES:
        for L in (1, 3):
            for cam in ([S.CAMERA, S.PRODUCT_CAMERA] if (H, W) == (10, 34) else [S.CAMERA]):
                r = reference_f32_ratios(scene(H, W, L, cam))
                print("%2d x %2d, L = %d, f = %4g: " % (H, W, L, cam[0]) + "  ".join("%s %.2f" % kv for kv in r.items()))
                worst = {k: max(worst[k], r[k]) for k in worst}
    print("worst reference f32 noise / (2^-24 magnitude):", {k: round(v, 3) for k, v in worst.items()})
    print("gates of the fused kernels' f32 stage (4 x F32_MEASURED):", R.F32_GATE)
    for k, v in worst.items():
        assert np.isfinite(v) and v > 0, (k, v)
        assert v <= R.F32_MEASURED[k] <= 1.25 * v + 0.05, (k, v, R.F32_MEASURED[k])
        assert R.F32_GATE[k] == 4.0 * R.F32_MEASURED[k]


# ---------------------------------------------------------------------------------------------------------------------
# the one-pixel-wide normals shapes are refused (C ABI, on the host: the refusal comes before any launch)
# ---------------------------------------------------------------------------------------------------------------------
def test_normals_entries_refuse_one_pixel_wide_images_on_the_host():
    import ctypes
    from geomconsistentfr_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    for H, W in ((1, 5), (5, 1), (1, 1), (0, 4), (4, -1)):
        assert lib.gcfr_normals_fwd(p, 1, H, W, 600.0, 600.0, 2.0, 2.0, 900.0, 1, p, None) == -1, (H, W)
        assert lib.gcfr_normals_bwd(p, p, 1, H, W, 600.0, 600.0, 2.0, 2.0, 900.0, 1, p, None) == -1, (H, W)
    text = open(os.path.join(ROOT, "include", "gcfr.h")).read()
    assert "H >= 2 and W >= 2" in text[text.index("Surface normals from depth"):text.index("int gcfr_normals_fwd")]
