"""GPU: the fused image-loss head (losses.image_losses, csrc/gcfr_losses.hip) outside the white-noise regime of
tests/test_gpu_image_losses.py -- smooth and flat images (where the SSIM's cancelling terms xx - mu1*mu1, xy - mu1*mu2,
mu2 - lum*mu1, cs*mu1 - mu2 decide the result), the shapes at which the finishing kernels loop or a tile row / column owns pixels but
(almost) no valid position, and the arguments no GPU test passed yet.

(a) The operation-order pin.  tests/image_losses_emulation.py restates the kernel in numpy f32 operation by operation (and
    tests/test_image_losses_host.py holds that restatement to the f64 one).  Against it:
      composite, grad_rendered (each upstream gradient alone, and all together)   the same bits
      ssim, recon_sq_sum, mask_sum                                                 equal or one f32 ulp apart
    The only freedom is the association of an f64 sum of at most 1.7e7 f32 terms: its error is below 1e-9 of the sum of magnitudes,
    far below half an f32 ulp of the result, so the two roundings to f32 differ only at a tie boundary.  Where the mean of the map
    is below 1e-2 in magnitude (values of both signs cancelling) the absolute difference is gated at one f32 ulp of 1e-2 instead.
(b) Accuracy against f64 (`train.ssim` and the torch expressions of `generator_losses` in f64 on the f32 inputs), measured per input
    family as ABSOLUTE error of ssim (1 - ssim is meaningless relatively where the images are nearly equal) and as gradient error over
    the gradient's largest entry, for the head and for the project's three torch f32 forms of the same expressions on the same input:
    train.ssim on the CPU, and on the GPU with blur_kernels "miopen" and "aten".  A family's figure at a shape is the largest over its
    mask kinds and layouts; the head's gate is twice the worst of the three forms' figures, floored at 2e-6 / 2e-5: all four are the
    same f32 products in another association, so none should be systematically worse (`_hold_accuracy` says what happens where
    the head is outside it).
    (The torch forms see every (image, channel) plane as an image of two identical channels: the mean of two equal values and the sum
    of two equal gradient halves are exact, and with more than one group the GPU forms take the depthwise kernels they take in
    training.)  rendered == images under a {0,1} mask or none, and all-zero inputs: ssim is exactly 1.0f.
(c) Shapes, (d) arguments, (e) the pin's teeth: see the tests.
Every measured figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import image_losses_emulation as E
import test_gpu_image_losses as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")

MASKS = ["face", "fractional", "none"]
LAYOUTS = ["nhwc", "nchw"]
IMPULSES = dict(impulse_tile_tl=(16, 32), impulse_tile_tr=(16, 63), impulse_tile_bl=(31, 32), impulse_tile_br=(31, 63),
                impulse_origin=(0, 0), impulse_5_5=(5, 5), impulse_last_valid=(-6, -6))
FAMILIES = ["white", "smooth", "flat_1e-2", "flat_1e-3", "face_paste", "equal", "zero"] + list(IMPULSES) + ["synthetic"]
FAMILY_SHAPE = (2, 128, 128)
BIG_SHAPES = [(1, 512, 512), (1, 272, 1000), (1, 11, 11), (2, 11, 4096), (65, 11, 11), (130, 12, 43)]
EDGE_SHAPES = [(1, H, W) for H in (17, 21, 22, 27) for W in (33, 37, 38, 43)]
_ids = lambda s: "x".join(map(str, s))


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _smooth(B, H, W):
    b, ch, r, c = np.meshgrid(np.arange(B), np.arange(3), np.arange(H), np.arange(W), indexing="ij")
    return (0.5 + 0.35 * np.sin(c / 11.0 + b) * np.cos(r / 13.0 + ch)).astype(np.float32)


def _family(name, B, H, W, seed=0):
    """rendered X and photograph Y, (B,3,H,W) f32; `seed` draws another noise of the same family"""
    rng = np.random.default_rng(21 + seed)
    noisy = lambda Y, s: np.clip(Y + np.float32(s) * rng.standard_normal(Y.shape).astype(np.float32), 0, 1).astype(np.float32)
    if name == "white":
        return G._pair(B, H, W, seed=seed)
    if name == "smooth":
        Y = _smooth(B, H, W)
        return noisy(Y, 1e-2), Y
    if name.startswith("flat_"):
        Y = np.full((B, 3, H, W), 0.9, np.float32)
        return noisy(Y, float(name[5:])), Y
    if name == "face_paste":            # what the step feeds the head: equal to the photograph, bit for bit, outside the face
        Y = _smooth(B, H, W)
        mf = G._mask("face", B, H, W)[:, None]
        return (noisy(Y, 1e-2) * mf + (1 - mf) * Y).astype(np.float32), Y
    if name == "equal":
        Y = _smooth(B, H, W)
        return Y.copy(), Y
    if name == "zero":
        return np.zeros((B, 3, H, W), np.float32), np.zeros((B, 3, H, W), np.float32)
    if name in IMPULSES:
        Y = _smooth(B, H, W)
        X = Y.copy()
        r, c = IMPULSES[name]
        X[0, 1, r, c] += np.float32(0.25)
        return X, Y
    if name == "synthetic":
        from geomconsistentfr_amd.train import synthetic_batch
        Y = np.ascontiguousarray(synthetic_batch(B, 0, H, W)["images"].permute(0, 3, 1, 2).numpy())
        return noisy(np.float32(0.95) * Y + np.float32(0.02), 5e-3), Y
    raise KeyError(name)


class _Case(dict):
    """the emulation's results are computed when a test asks for them (the accuracy tests do not)"""

    def __missing__(self, key):
        assert key == "emu"
        self["emu"] = _emulate(self["X"], self["Y"], self["M"], self["ups"], self["data_range"])
        return self["emu"]


@functools.lru_cache(maxsize=4)
def _case(family, shape, mask, data_range=1.0, seed=0):
    """inputs and the f64 reference's results (and, on demand, the emulation's): computed once for both layouts"""
    B, H, W = shape
    X, Y = _family(family, B, H, W, seed)
    if data_range != 1.0:
        X, Y = X * np.float32(data_range), Y * np.float32(data_range)
    M, ups = G._mask(mask, B, H, W), G._upstreams(B, H, W)
    ref = _torch_form(X, Y, M, ups, "f64", data_range)
    x32, y32 = torch.from_numpy(X), torch.from_numpy(Y)
    m32 = torch.ones_like(y32) if M is None else torch.from_numpy(M)[:, None].expand(-1, 3, -1, -1)
    ref["composite"] = (x32 * m32 + (1.0 - m32) * y32).numpy()          # the torch f32 expression (T8:619)
    return _Case(X=X, Y=Y, M=M, ups=ups, ref=ref, data_range=data_range)


def _emulate(X, Y, M, ups, data_range=1.0, window=None):
    win = E.gauss_window() if window is None else window
    comp, s, sq, msum, _ = E.forward(X, Y, M, win, data_range)
    return dict(composite=comp, ssim=s, sq=np.float32(sq), msum=np.float32(msum),
                grads=E.backward_selections(X, Y, M, win, data_range, *ups))


def _torch_form(X, Y, M, ups, form, data_range=1.0):
    """the torch expressions of the head: form "f64" (CPU, the reference), "cpu_f32", "gpu_miopen", "gpu_aten" """
    from geomconsistentfr_amd.train import ssim
    dev = DEV if form.startswith("gpu") else CPU
    dt = torch.float64 if form == "f64" else torch.float32
    kern = "miopen" if form == "gpu_miopen" else "aten"
    B, _, H, W = X.shape
    x = torch.from_numpy(X).to(dev, dt).requires_grad_()
    y = torch.from_numpy(Y).to(dev, dt)
    m3 = torch.ones_like(y) if M is None else torch.from_numpy(M).to(dev, dt)[:, None].expand(-1, 3, -1, -1)
    comp = x * m3 + (1.0 - m3) * y
    sq = ((x * m3 - y * m3) ** 2).sum()
    two = lambda t: t.reshape(B * 3, 1, H, W).expand(-1, 2, -1, -1)          # every plane as an image of two identical channels
    s = ssim(two(comp), two(y), data_range=data_range, size_average=False, nonnegative_ssim=False, blur_kernels=kern).reshape(B, 3)
    Gc, Gs, gq = (torch.from_numpy(np.asarray(u)).to(dev, dt) for u in ups)
    terms = dict(composite=(comp * Gc).sum(), ssim=(s * Gs).sum(), recon=gq * sq)
    grads = {k: torch.autograd.grad(v, x, retain_graph=True)[0].cpu().numpy() for k, v in terms.items()}
    grads["all"] = torch.autograd.grad(sum(terms.values()), x)[0].cpu().numpy()
    return dict(ssim=s.detach().cpu().numpy(), sq=float(sq.detach()), msum=float(m3.sum()), grads=grads,
                dssim=float(G._dssim(s.detach().double().cpu())), composite=comp.detach().cpu().numpy())


def _run_op(X, Y, M, ups, layout, data_range=1.0, mask_shape=None):
    from geomconsistentfr_amd.losses import image_losses
    x = torch.from_numpy(X).to(DEV).requires_grad_()
    y = torch.from_numpy(Y).to(DEV)
    if layout == "nhwc":
        y = y.permute(0, 2, 3, 1).contiguous()
    m = None if M is None else torch.from_numpy(M).to(DEV)
    if mask_shape is not None:
        m = m.reshape(mask_shape)
    return _collect(x, x, image_losses(x, y, m, images_layout=layout, data_range=data_range), ups)


def _collect(leaf, x, outs, ups):
    comp, sq, msum, s = outs
    Gc, Gs, gq = (torch.from_numpy(np.asarray(u)).to(DEV) for u in ups)
    terms = dict(composite=(comp * Gc).sum(), ssim=(s * Gs).sum(), recon=gq * sq)
    grads = {k: torch.autograd.grad(v, leaf, retain_graph=True)[0] for k, v in terms.items()}
    grads["all"] = torch.autograd.grad(sum(terms.values()), leaf)[0]
    for g in grads.values():
        assert g.shape == leaf.shape
    assert sq.dtype == msum.dtype == torch.float32
    return dict(composite=comp.detach().cpu().numpy(), sq=np.float32(sq.item()), msum=np.float32(msum.item()),
                ssim=s.detach().cpu().numpy(), dssim=float(G._dssim(s.detach().double())),
                grads={k: g.cpu().numpy() for k, g in grads.items()})


# ------------------------------------------------------------------------------------------------
# (a) the comparator of the operation-order pin
# ------------------------------------------------------------------------------------------------
SMALL_MEAN = np.float32(1e-2)


def pin_mismatches(got, emu):
    """what of the head's results is not the emulation's: [] = pinned"""
    bad = []
    if not E.bit_equal(got["composite"], emu["composite"]):
        bad.append("composite: %d elements differ" % int((got["composite"] != emu["composite"]).sum()))
    for k in ("composite", "ssim", "recon", "all"):
        if not E.bit_equal(got["grads"][k], emu["grads"][k]):
            d = got["grads"][k].astype(np.float64) - emu["grads"][k]
            bad.append("gradient (%s): %d elements differ, largest difference %.3g of %.3g" % (
                k, int((got["grads"][k] != emu["grads"][k]).sum()), np.nanmax(np.abs(d)), np.nanmax(np.abs(emu["grads"][k]))))
    gs, es = got["ssim"].ravel(), emu["ssim"].ravel()
    nan = np.isnan(es)
    if not np.array_equal(nan, np.isnan(gs)):
        bad.append("ssim: NaN in other rows")
    for i in np.flatnonzero(~nan):
        if abs(es[i]) < SMALL_MEAN:
            ok = abs(np.float64(gs[i]) - np.float64(es[i])) <= np.spacing(SMALL_MEAN)
        else:
            ok = E.ulps(gs[i], es[i]) <= 1
        if not ok:
            bad.append("ssim[%d]: %.9g against %.9g" % (i, gs[i], es[i]))
    for k in ("sq", "msum"):
        if np.isnan(emu[k]) or np.isnan(got[k]):
            if not (np.isnan(emu[k]) and np.isnan(got[k])):
                bad.append("%s: %r against %r" % (k, got[k], emu[k]))
        elif E.ulps(got[k], emu[k]) > 1:
            bad.append("%s: %.9g against %.9g" % (k, got[k], emu[k]))
    return bad


def _hold_pin(got, emu, tag):
    bad = pin_mismatches(got, emu)
    print("%s: pin: ssim ulps %s, sq %d, msum %d, %s" % (
        tag, int(E.ulps(got["ssim"], emu["ssim"]).max()) if np.isfinite(emu["ssim"]).all() else "nan",
        -1 if np.isnan(emu["sq"]) else int(E.ulps(got["sq"], emu["sq"])), int(E.ulps(got["msum"], emu["msum"])),
        "gradient and composite bit-equal" if not bad else bad))
    assert not bad, (tag, bad[:8])


# ------------------------------------------------------------------------------------------------
# (b) accuracy against f64, against the torch f32 forms'
# ------------------------------------------------------------------------------------------------
KEYS = ("value", "ssim", "all", "composite", "recon")
FLOOR = dict(value=2e-6, dssim=2e-6, ssim=2e-5, all=2e-5, composite=2e-5, recon=2e-5)
FORMS = ("cpu_f32", "gpu_miopen", "gpu_aten")
N_SEEDS = 8


def _residue_bound(c):
    """Where rendered == images in every window (the `equal` family, an impulse the mask removes) the SSIM's own gradient is zero in
    exact arithmetic: gX = blurT(a) + 2 X blurT(b) + Y blurT(c) with a = 0 and c = -2 b, two terms of magnitude
    T = 2 max|X| max|g_ssim| / (n_valid C2) at most (|b| <= |u| / B2, B2 >= C2, the window sums to 1) that cancel.  What any f32 form
    returns there is the rounding of those terms -- 22 taps and the final sum: within 16 f32 epsilons of T -- and what f64 returns is
    its own rounding, ~1e-9 of that; an error "relative to the gradient's largest entry" is then noise over noise."""
    _, _, H, W = c["X"].shape
    C2 = (0.03 * c["data_range"]) ** 2
    return 16 * float(np.finfo(np.float32).eps) * 2 * float(np.abs(c["ref"]["composite"]).max()) * float(np.abs(c["ups"][1]).max()) / ((H - 10) * (W - 10) * C2)


def _errors(res, c):
    """distances from the f64 reference: `value` = ssim, absolute; `dssim` relative; the gradient keys over the reference's largest
    entry -- except the SSIM's own gradient where the reference's is below `_residue_bound`: there it must be within that bound,
    absolutely, and counts as 0"""
    ref = c["ref"]
    e = dict(value=float(np.abs(res["ssim"].astype(np.float64) - ref["ssim"]).max()))
    dd = abs(res["dssim"] - ref["dssim"])
    e["dssim"] = (0.0 if dd == 0 else float("inf")) if ref["dssim"] == 0 else dd / abs(ref["dssim"])
    for k, r in ref["grads"].items():
        d, scale = float(np.abs(res["grads"][k].astype(np.float64) - r).max()), float(np.abs(r).max())
        if k == "ssim" and scale < _residue_bound(c):
            assert d <= _residue_bound(c), ("the SSIM's gradient where it is zero up to rounding", d, _residue_bound(c))
            e[k] = 0.0
        else:
            e[k] = (0.0 if d == 0 else float("inf")) if scale == 0 else d / scale      # a gradient that is exactly zero must be returned as such
    return e


@functools.lru_cache(maxsize=4)
def _torch_errors(family, shape, mask, data_range=1.0):
    c = _case(family, shape, mask, data_range)
    return {form: _errors(_torch_form(c["X"], c["Y"], c["M"], c["ups"], form, data_range), c) for form in FORMS}


def _reference_draws(family, shape, data_range, keys):
    """torch f32 on the CPU against f64 on N_SEEDS further noise draws of the family at this shape, per mask kind: what the
    reference's own error does from one input to the next"""
    draws = {mask: [] for mask in MASKS}
    for seed in range(1, N_SEEDS + 1):
        for mask in MASKS:
            c = _case(family, shape, mask, data_range, seed)
            e = _errors(_torch_form(c["X"], c["Y"], c["M"], c["ups"], "cpu_f32", data_range), c)
            draws[mask].append({k: e[k] for k in keys})
    return draws


def _hold_accuracy(family, shape, keys=KEYS, data_range=1.0):
    """(b) for one input family at one shape.  Every mask kind and both layouts are run and printed; the figure of the head and of
    each torch form is the largest over those cases; the head's must be within twice the worst of the three forms' on the same
    inputs, floored at 2e-6 (ssim absolute, DSSIM relative) / 2e-5 (gradient over its largest entry).
    The factor 2 presumes that a form's error on a family at a shape is a property of the form.  Where the head exceeds that gate,
    the test prints it as a FINDING and measures whether the presumption holds there: torch f32 on the CPU against f64 on N_SEEDS
    further noise draws of the same family, shape and masks.  Only if, under some mask kind, the reference's own error moves by more
    than 2x from one draw to another -- a shape of so few valid positions that nothing averages, so that one input cannot rank two
    forms -- the head is held to twice the worst the reference did on any draw instead; otherwise the test fails on the gate above."""
    seed0 = {}
    worst = {form: dict.fromkeys(keys, 0.0) for form in ("hip",) + FORMS}
    fmt = lambda e: " ".join("%s %.2e" % (k, e[k]) for k in keys)
    tag = "%s %s" % (_ids(shape), family) + ("" if data_range == 1.0 else " data_range %g" % data_range)
    for mask in MASKS:
        c = _case(family, shape, mask, data_range)
        cases = dict(_torch_errors(family, shape, mask, data_range))
        for layout in LAYOUTS:
            got = _run_op(c["X"], c["Y"], c["M"], c["ups"], layout, data_range=data_range)
            assert np.isfinite(got["ssim"]).all() and all(np.isfinite(g).all() for g in got["grads"].values())
            e = _errors(got, c)
            cases["hip"] = {k: max(e[k], cases.get("hip", e)[k]) for k in keys}
            print("FIG %s %s %s hip        %s" % (tag, mask, layout, fmt(e)))
        seed0[mask] = cases["cpu_f32"]
        for form in FORMS:
            print("FIG %s %s - %-10s %s" % (tag, mask, form, fmt(cases[form])))
        for form, e in cases.items():
            worst[form] = {k: max(worst[form][k], e[k]) for k in keys}
    print("FAMILY %s: value = ssim absolute, dssim relative, gradient keys / largest entry ('ssim' = the SSIM's upstream alone)" % tag)
    for form, e in worst.items():
        print("FAMILY %s %-10s %s" % (tag, form, fmt(e)))
    gate = {k: max(2 * max(worst[f][k] for f in FORMS), FLOOR[k]) for k in keys}
    over = [k for k in keys if worst["hip"][k] > gate[k]]
    if not over:
        return
    for k in over:
        print("FINDING %s: %s: the head %.3g, the torch forms on the same inputs %s, gate %.3g" % (
            tag, k, worst["hip"][k], " / ".join("%.3g" % worst[f][k] for f in FORMS), gate[k]))
    draws = _reference_draws(family, shape, data_range, over)
    for k in over:
        seen = {mask: [seed0[mask][k]] + [d[k] for d in draws[mask]] for mask in MASKS}
        spread = max(max(v) / min(v) if min(v) > 0 else float("inf") for v in seen.values())
        bound = max(2 * max([max(v) for v in seen.values()] + [worst[f][k] for f in FORMS]), FLOOR[k])
        for mask, v in seen.items():
            print("FINDING %s: %s: torch f32 on the CPU, %s mask, %d noise draws: %s" % (tag, k, mask, len(v), " ".join("%.3g" % x for x in v)))
        print("FINDING %s: %s: largest / smallest within a mask kind %.2f; twice the worst of the reference: %.3g" % (tag, k, spread, bound))
        assert spread > 2, (tag, k, "the head is outside twice the worst torch form and the reference is repeatable here", worst["hip"][k], gate[k], spread)
        assert worst["hip"][k] <= bound, (tag, k, "the head is outside twice the worst the reference did on any draw", worst["hip"][k], bound)


def _hold_white(got, ref, tag):
    """White noise, per case: the gates of tests/test_gpu_image_losses.py on composite (bit-equal to the torch f32 expression), ssim,
    recon_sq_sum and mask_sum (2e-6 relative) and the gradient (2e-5 of its largest entry, every selection of upstream gradients).
    The DSSIM formed from ssim is gated per shape by `_hold_accuracy`: at 2e-6 relative, or at twice the torch forms' where they
    are further than 1e-6 themselves."""
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))
    e_ssim, e_dssim = rel(got["ssim"], ref["ssim"]), rel(got["dssim"], ref["dssim"])
    e_sq, e_m = rel(got["sq"], ref["sq"]), rel(got["msum"], ref["msum"])
    e_g = {k: float(np.abs(got["grads"][k] - ref["grads"][k]).max() / np.abs(ref["grads"][k]).max()) for k in ref["grads"]}
    print("%s: f64 distance: ssim %.2e (dssim %.2e) sq %.2e msum %.2e grad %s" % (
        tag, e_ssim, e_dssim, e_sq, e_m, " ".join("%s %.2e" % kv for kv in sorted(e_g.items()))))
    assert np.array_equal(got["composite"], ref["composite"]), (tag, "composite is not bit-equal to the torch f32 expression")
    assert e_ssim <= 2e-6, (tag, e_ssim)
    assert e_sq <= 2e-6 and e_m <= 2e-6, (tag, e_sq, e_m)
    for k, e in e_g.items():
        assert np.abs(ref["grads"][k]).max() > 0
        assert e <= 2e-5, (tag, k, e)


# ------------------------------------------------------------------------------------------------
# the input families at (2,128,128)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("family", FAMILIES)
def test_family_is_pinned_to_the_op_order(family, mask, layout):
    c = _case(family, FAMILY_SHAPE, mask)
    tag = "%s %s %s" % (family, mask, layout)
    got = _run_op(c["X"], c["Y"], c["M"], c["ups"], layout)
    _hold_pin(got, c["emu"], tag)
    assert all(np.isfinite(g).all() for g in got["grads"].values())
    if family == "zero" or (family == "equal" and mask != "fractional"):
        # every pair of window sums is identical, so cs = lum = 1 exactly at every position (a fractional mask pastes
        # x*m + (1-m)*x, which is x only up to rounding)
        assert np.array_equal(got["composite"], c["Y"])
        assert (got["ssim"] == np.float32(1.0)).all(), got["ssim"]


@pytest.mark.parametrize("family", FAMILIES)
def test_family_is_as_close_to_f64_as_the_torch_f32_forms(family):
    _hold_accuracy(family, FAMILY_SHAPE)


# ------------------------------------------------------------------------------------------------
# (c) shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("family", ["white", "smooth"])
@pytest.mark.parametrize("shape", BIG_SHAPES + EDGE_SHAPES, ids=_ids)
def test_shapes_where_the_finishing_kernels_loop_and_tiles_are_ragged(shape, family, mask, layout):
    """(1,512,512): 512 tiles and (1,272,1000): 544 tiles -- finish_image's loop runs a second and a third time; (1,11,11): one valid
    position; (2,11,4096): the widest row; (65,11,11), (130,12,43): finish_batch's loop runs again; H in {17,21,22,27} x W in
    {33,37,38,43}: the last tile row / column owns pixels but zero or one valid position.  The pin at all of them; white noise under
    the gates of tests/test_gpu_image_losses.py here (its DSSIM gate per shape, below), smooth under (b)'s per shape, below."""
    c = _case(family, shape, mask)
    tag = "%s %s %s %s" % (_ids(shape), family, mask, layout)
    got = _run_op(c["X"], c["Y"], c["M"], c["ups"], layout)
    _hold_pin(got, c["emu"], tag)
    assert all(np.isfinite(g).all() for g in got["grads"].values())
    if family == "white":
        _hold_white(got, c["ref"], tag)


@pytest.mark.parametrize("shape", BIG_SHAPES + EDGE_SHAPES, ids=_ids)
def test_smooth_family_at_each_shape_is_as_close_to_f64_as_the_torch_f32_forms(shape):
    _hold_accuracy("smooth", shape)


@pytest.mark.parametrize("shape", BIG_SHAPES + EDGE_SHAPES, ids=_ids)
def test_white_noise_dssim_at_each_shape(shape):
    _hold_accuracy("white", shape, keys=("dssim",))


# ------------------------------------------------------------------------------------------------
# (d) arguments
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("family", ["white", "smooth"])
def test_data_range_255(family, mask, layout):
    """inputs scaled by 255 and data_range = 255 (C1 = 6.5025, C2 = 58.5225) against the emulation and against
    train.ssim(data_range=255) in f64: white noise under the gates of tests/test_gpu_image_losses.py, smooth measured and printed"""
    shape = (2, 64, 72)
    c = _case(family, shape, mask, 255.0)
    tag = "data_range 255 %s %s %s" % (family, mask, layout)
    got = _run_op(c["X"], c["Y"], c["M"], c["ups"], layout, data_range=255.0)
    _hold_pin(got, c["emu"], tag)
    e = _errors(got, c)
    print("%s: f64 distance ssim_abs %.2e grad %s" % (tag, e["value"], " ".join("%s %.2e" % (k, e[k]) for k in ("ssim", "all"))))
    if family == "white":
        _hold_white(got, c["ref"], tag)


def test_data_range_255_white_noise_dssim():
    _hold_accuracy("white", (2, 64, 72), keys=("dssim",), data_range=255.0)


@pytest.mark.parametrize("family", ["white", "face_paste"])
def test_mask_layouts_return_the_same_bits(family):
    B, H, W = shape = (2, 64, 72)
    c = _case(family, shape, "fractional")
    base = _run_op(c["X"], c["Y"], c["M"], c["ups"], "nhwc")
    _hold_pin(base, c["emu"], "mask (B,H,W) " + family)
    for ms in ((B, H, W, 1), (B, 1, H, W)):
        got = _run_op(c["X"], c["Y"], c["M"], c["ups"], "nhwc", mask_shape=ms)
        assert not pin_mismatches(got, base) and np.array_equal(got["ssim"], base["ssim"]) and got["sq"] == base["sq"], ms


def test_non_contiguous_rendered_returns_the_same_bits_and_a_gradient_of_its_own_shape():
    from geomconsistentfr_amd.losses import image_losses
    B, H, W = shape = (2, 64, 72)
    c = _case("smooth", shape, "fractional")
    base = _run_op(c["X"], c["Y"], c["M"], c["ups"], "nchw")
    _hold_pin(base, c["emu"], "contiguous")
    y, m = torch.from_numpy(c["Y"]).to(DEV), torch.from_numpy(c["M"]).to(DEV)
    same = lambda got: not pin_mismatches(got, base) and np.array_equal(got["ssim"], base["ssim"]) and got["sq"] == base["sq"]

    x = torch.from_numpy(c["X"]).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    assert not x.is_contiguous()
    assert same(_collect(x, x, image_losses(x, y, m, images_layout="nchw"), c["ups"]))

    big = torch.full((B, 3, H + 4, W + 6), 0.25, device=DEV)
    big[:, :, 2:H + 2, 3:W + 3] = torch.from_numpy(c["X"]).to(DEV)
    big.requires_grad_()
    x = big[:, :, 2:H + 2, 3:W + 3]
    assert not x.is_contiguous()
    got = _collect(big, x, image_losses(x, y, m, images_layout="nchw"), c["ups"])
    inner = {k: np.ascontiguousarray(g[:, :, 2:H + 2, 3:W + 3]) for k, g in got["grads"].items()}
    for k, g in got["grads"].items():
        assert g.shape == (B, 3, H + 4, W + 6)
        outer = g.copy()
        outer[:, :, 2:H + 2, 3:W + 3] = 0
        assert not outer.any(), k
    assert same(dict(got, grads=inner))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", ["white", "smooth"])
def test_mask_values_outside_the_unit_interval(family, layout):
    B, H, W = 2, 64, 72
    X, Y = _family(family, B, H, W)
    M = (np.random.default_rng(8).random((B, H, W), dtype=np.float32) * np.float32(2.0) - np.float32(0.5)).astype(np.float32)
    assert M.min() < -0.4 and M.max() > 1.4
    ups = G._upstreams(B, H, W)
    _hold_pin(_run_op(X, Y, M, ups, layout), _emulate(X, Y, M, ups), "mask in [-0.5, 1.5] %s %s" % (family, layout))


def test_a_side_stream_returns_the_same_bits():
    c = _case("smooth", (2, 64, 72), "face")
    base = _run_op(c["X"], c["Y"], c["M"], c["ups"], "nhwc")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = _run_op(c["X"], c["Y"], c["M"], c["ups"], "nhwc")
    side.synchronize()
    _hold_pin(got, c["emu"], "side stream")
    assert not pin_mismatches(got, base) and np.array_equal(got["ssim"], base["ssim"]) and got["sq"] == base["sq"]


@pytest.mark.parametrize("where", ["rendered", "images"])
def test_a_nan_pixel_stays_inside_its_image(where):
    """Ordinary data: per-image partials must not mix.  One NaN pixel in image 0 of 3 (at a tile corner, under a mask value that is
    neither 0 nor 1)."""
    B, H, W = 3, 64, 72
    X, Y = _family("smooth", B, H, W)
    M, ups = G._mask("fractional", B, H, W), G._upstreams(B, H, W)
    clean = _run_op(X, Y, M, ups, "nhwc")
    Xn, Yn = X.copy(), Y.copy()
    (Xn if where == "rendered" else Yn)[0, 1, 16, 32] = np.nan
    got = _run_op(Xn, Yn, M, ups, "nhwc")
    _hold_pin(got, _emulate(Xn, Yn, M, ups), "NaN in %s" % where)
    assert np.isnan(got["ssim"][0, 1]) and np.array_equal(got["ssim"][1:], clean["ssim"][1:])
    assert np.array_equal(got["composite"][1:], clean["composite"][1:]) and np.isnan(got["composite"][0, 1, 16, 32])
    assert int(np.isnan(got["composite"]).sum()) == 1
    assert np.isnan(got["sq"]) and got["msum"] == clean["msum"]
    for k, g in got["grads"].items():
        assert not np.isnan(g[1:]).any() and np.array_equal(g[1:], clean["grads"][k][1:]), k
        assert np.isnan(g[0]).any() == (k != "composite"), k          # (the composite's upstream alone passes through m only)


# ------------------------------------------------------------------------------------------------
# (e) the pin has teeth: perturbed arguments through the C ABI
# ------------------------------------------------------------------------------------------------
def _run_abi(X, Y, M, ups, window, data_range):
    """the head through gcfr_image_losses_fwd / _bwd directly, NCHW, with the caller's window and data_range"""
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    B, _, H, W = X.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x, y, m = t(X), t(Y), (None if M is None else t(M))
    Gc, Gs, gq = (t(np.asarray(u, np.float32).reshape(-1)) for u in ups)
    comp, s, sums = torch.empty_like(x), torch.empty((B, 3), device=DEV), torch.empty(2, dtype=torch.float64, device=DEV)
    nbytes = int(L.gcfr_image_losses_workspace_bytes(B, H, W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    win = (ctypes.c_float * 11)(*[float(v) for v in window])
    wp = ctypes.cast(win, ctypes.c_void_p)
    st = torch.cuda.current_stream(DEV).cuda_stream
    ptr = lambda v: None if v is None else v.data_ptr()
    _lib.check(L.gcfr_image_losses_fwd(x.data_ptr(), y.data_ptr(), ptr(m), 1, B, H, W, wp, float(data_range), comp.data_ptr(),
                                       s.data_ptr(), sums.data_ptr(), ws.data_ptr(), nbytes, st), "gcfr_image_losses_fwd")
    grads = {}
    for k, (a, b, c) in dict(composite=(Gc, None, None), ssim=(None, Gs, None), recon=(None, None, gq), all=(Gc, Gs, gq)).items():
        g = torch.empty_like(x)
        _lib.check(L.gcfr_image_losses_bwd(x.data_ptr(), y.data_ptr(), ptr(m), 1, B, H, W, wp, float(data_range), ptr(a), ptr(b), ptr(c),
                                           g.data_ptr(), st), "gcfr_image_losses_bwd")
        grads[k] = g.cpu().numpy()
    torch.cuda.synchronize(DEV)
    return dict(composite=comp.cpu().numpy(), ssim=s.cpu().numpy(), sq=np.float32(sums[0].float().item()),
                msum=np.float32(sums[1].float().item()), grads=grads)


@pytest.mark.parametrize("family", ["white", "flat_1e-2"])
def test_the_pin_reports_a_window_tap_or_a_data_range_off_by_one_part_in_a_million(family):
    """The comparator of (a), fed the TRUE window and data_range, must report each of: tap 3 moved by one f32 ulp; taps 0 and 10
    made unequal by one ulp; data_range = 1 + 2^-20 -- all of which a 2e-6 gate lets through -- and must pass the true arguments."""
    c = _case(family, FAMILY_SHAPE, "fractional")
    win = E.gauss_window()
    assert not pin_mismatches(_run_abi(c["X"], c["Y"], c["M"], c["ups"], win, 1.0), c["emu"])
    tap3, ends = win.copy(), win.copy()
    tap3[3] = np.nextafter(win[3], np.float32(1.0))
    ends[10] = np.nextafter(win[10], np.float32(1.0))
    for what, w, dr in (("tap 3 + 1 ulp", tap3, 1.0), ("tap 10 + 1 ulp", ends, 1.0), ("data_range 1 + 2^-20", win, 1.0 + 2.0 ** -20)):
        got = _run_abi(c["X"], c["Y"], c["M"], c["ups"], w, dr)
        bad = pin_mismatches(got, c["emu"])
        e = _errors(dict(got, dssim=c["ref"]["dssim"]), c)
        print("%s, %s: f64 distance ssim %.2e gradient %.2e (inside the 2e-6 / 2e-5 gates: %s); the pin reports %s" % (
            family, what, e["value"], e["all"], e["value"] <= 2e-6 and e["all"] <= 2e-5, bad[:3]))
        assert any(b.startswith("ssim") or b.startswith("gradient") for b in bad), what
        assert not pin_mismatches(got, _emulate(c["X"], c["Y"], c["M"], c["ups"], dr, w)), what      # and the emulation follows the arguments
