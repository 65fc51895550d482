"""CPU: the supervised-loss head's plumbing (csrc/gcfr_supervised_losses.hip, include/gcfr.h, losses.supervised_losses,
TrainConfig.supervised_losses) -- the three symbols are declared, bound and exported and the ABI revision is unchanged; the
workspace follows its documented formula; arguments are validated on the host before any GPU call; the switch validates its value;
there is no CPU path; `generator_losses(supervised_terms=...)` fed the torch-made five terms reproduces the plain call; the kernels
are the stated set and spill-free.  And the numpy-f32 restatement of the head's operation order
(tests/supervised_losses_emulation.py), which tests/test_gpu_supervised_losses.py holds the kernels to, is itself held to the f64
torch restatement of `generator_losses` here: terms 2e-6 relative (the lighting term, which can cancel, 2e-6 of
sum_b |1 - cos_b| / B), gradients 2e-6 of each plane's largest entry."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_abi import declared_symbols
from test_kernel_resources import LLVM, _kernel_metadata

SYMBOLS = ("gcfr_supervised_losses_workspace_bytes", "gcfr_supervised_losses_fwd", "gcfr_supervised_losses_bwd")
KEYS = ("depth", "ambient", "lighting", "albedo", "generator")


def test_the_three_symbols_are_declared_bound_and_exported():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    for s in SYMBOLS:
        assert s in declared_symbols(), s
        assert s in _lib.exported_symbols(), s
        assert hasattr(L, s), s
    assert L.gcfr_abi_version() == 6 and _lib.ABI_VERSION == 6          # no existing entry point or struct changed


def test_workspace_bytes_is_the_documented_formula():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    for B, H, W in ((1, 1, 1), (1, 1, 1023), (1, 32, 32), (1, 25, 41), (3, 21, 37), (4, 256, 256), (32, 256, 256), (127, 4096, 4096)):
        assert L.gcfr_supervised_losses_workspace_bytes(B, H, W) == 8 * 5 * -(-(B * H * W) // 1024), (B, H, W)
    for B, H, W in ((0, 64, 64), (1, 0, 64), (1, 64, 0), (1, 4097, 64), (1, 64, 4097), (65536, 1, 1), (128, 4096, 4096)):
        assert L.gcfr_supervised_losses_workspace_bytes(B, H, W) == 0, (B, H, W)     # (the last: B H W = 2^31)


def test_invalid_arguments_are_rejected_before_any_launch():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = ctypes.c_void_p(4096)                                   # a dummy non-null, aligned "device" pointer: never dereferenced
    big = 1 << 30
    fwd_args = dict(depth=p, gt_depth=p, mask=p, albedo=p, gt_albedo=p, mask_fill=p, unit_light=p, ambient=p, lightings=p, logits=p,
                    n_logits=900, B=2, H=64, W=40, terms=p, sums=p, ws=p, ws_bytes=big, stream=None)
    bwd_args = dict(depth=p, gt_depth=p, mask=p, albedo=p, gt_albedo=p, mask_fill=p, ambient=p, lightings=p, logits=p, n_logits=900,
                    B=2, H=64, W=40, sums=p, g_depth=p, g_ambient=p, g_lighting=p, g_albedo=p, g_generator=p, grad_depth=p,
                    grad_albedo=p, grad_unit_light=p, grad_ambient=p, grad_logits=p, stream=None)
    fwd = lambda **kw: L.gcfr_supervised_losses_fwd(*{**fwd_args, **kw}.values())      # (dicts keep the argument order)
    bwd = lambda **kw: L.gcfr_supervised_losses_bwd(*{**bwd_args, **kw}.values())
    for name in ("depth", "gt_depth", "mask", "albedo", "gt_albedo", "mask_fill", "unit_light", "ambient", "lightings", "terms", "sums", "ws"):
        assert fwd(**{name: None}) == -1, name
    for name in ("depth", "gt_depth", "mask", "albedo", "gt_albedo", "mask_fill", "ambient", "lightings", "sums", "grad_depth",
                 "grad_albedo", "grad_unit_light", "grad_ambient", "grad_logits"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1            # zero sizes
        assert call(B=65536) == -1 and call(H=4097) == -1 and call(W=4097) == -1
        assert call(B=128, H=4096, W=4096) == -1                                   # B H W = 2^31
        assert call(n_logits=0) == -1 and call(n_logits=-1) == -1 and call(n_logits=1 << 31) == -1
    need = L.gcfr_supervised_losses_workspace_bytes(2, 64, 40)
    assert need > 0 and fwd(ws_bytes=need - 1) == -1 and fwd(ws_bytes=0) == -1     # a short workspace
    assert fwd(ws=ctypes.c_void_p(4100)) == -1 and fwd(sums=ctypes.c_void_p(4100)) == -1      # not 8-byte aligned
    assert bwd(sums=ctypes.c_void_p(4100)) == -1


def test_trainconfig_switch_validates_its_value():
    from geomconsistentfr_amd.train import TrainConfig
    assert TrainConfig().supervised_losses == "torch"           # the default does not change
    assert TrainConfig(supervised_losses="hip").supervised_losses == "hip"
    assert TrainConfig(supervised_losses="hip").image_losses == "torch" and TrainConfig(image_losses="hip").supervised_losses == "torch"
    with pytest.raises(ValueError, match="supervised_losses"):
        TrainConfig(supervised_losses="cuda")


def _cpu_out_and_batch(B=2, H=32, W=24, seed=3):
    from geomconsistentfr_amd.train import synthetic_batch
    g = torch.Generator().manual_seed(seed)
    batch = synthetic_batch(B, 7, H, W)
    batch["masks"] = (torch.rand(B, H, W, 1, generator=g) * 255).round() / 255        # different from masks_fill
    rnd = lambda *s: torch.rand(*s, generator=g)
    unit = F.normalize(torch.randn(B, 3, 1, 1, generator=g), dim=1)
    out = (rnd(B, 3, H, W).requires_grad_(), (80 * rnd(B, 1, H, W)).requires_grad_(), None, None, None, rnd(B, 3, H, W), unit.requires_grad_(),
           rnd(B, 1, 1).requires_grad_())
    return out, batch, (3 * torch.randn(B, 1, 6, 6, generator=g)).requires_grad_()


def test_supervised_losses_has_no_cpu_path_and_refuses_other_dtypes_and_shapes():
    from geomconsistentfr_amd._lib import GcfrError
    from geomconsistentfr_amd.losses import supervised_losses
    out, batch, logits = _cpu_out_and_batch()
    with pytest.raises(GcfrError, match="no CPU path"):
        supervised_losses(out[1], out[0], out[6], out[7], batch, logits)
    with pytest.raises(GcfrError, match="no CPU path"):
        supervised_losses(out[1], out[0], out[6], out[7], batch)


def test_generator_losses_with_torch_made_supervised_terms_gives_the_same_terms_and_gradients():
    """`supervised_terms` carries (depth, ambient, lighting, albedo, generator); made with torch on the CPU they must reproduce the
    built-in path: same keys, same order, the same sum for `total`."""
    from geomconsistentfr_amd.train import generator_losses
    out, batch, logits = _cpu_out_and_batch()
    albedo, depth, unit_light, ambient_values = out[0], out[1], out[6], out[7]
    B = depth.shape[0]
    ref = generator_losses(out, batch, logits)
    wrt = [depth, albedo, unit_light, ambient_values, logits]
    g_ref = torch.autograd.grad(ref["total"], wrt)
    grey = albedo.mean(1).reshape(B, albedo.shape[2], albedo.shape[3], 1)
    terms = torch.stack([
        F.l1_loss(depth.permute(0, 2, 3, 1) * batch["masks"], batch["depths"] * batch["masks"], reduction="sum") / batch["masks"].sum(),
        2.5 * F.l1_loss(ambient_values, batch["lightings"][:, 0].reshape(B, 1, 1)),
        torch.sum(1 - torch.sum(unit_light * batch["lightings"][:, 1:4].reshape(B, 3, 1, 1), dim=1)) / B,
        5.0 * F.l1_loss(grey * batch["masks_fill"], batch["albedo"] * batch["masks_fill"], reduction="sum") / batch["masks_fill"].sum(),
        0.01 * F.binary_cross_entropy_with_logits(logits, torch.ones_like(logits))])
    got = generator_losses(out, batch, None, supervised_terms=terms)
    assert list(got) == list(ref) == ["recon", "depth", "ambient", "lighting", "albedo", "generator", "DSSIM", "total"]
    for k in ref:
        np.testing.assert_allclose(float(got[k].detach()), float(ref[k].detach()), rtol=1e-6, err_msg=k)
    assert float(got["total"].detach()) == float(sum(v for k, v in got.items() if k != "total").detach())
    for a, b in zip(torch.autograd.grad(got["total"], wrt), g_ref):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_new_kernels_are_the_stated_set_and_use_no_scratch(tmp_path):
    k = _kernel_metadata(tmp_path)
    mine = {n: v for n, v in k.items() if n.startswith("supervised_losses_")}
    assert set(mine) == {"supervised_losses_fwd_kernel", "supervised_losses_finish_kernel", "supervised_losses_bwd_kernel"}, sorted(mine)
    for n, v in mine.items():
        assert v["scratch"] == 0, (n, v)
        assert v["vgpr"] <= 128 and v["lds"] <= 1024, (n, v)       # bandwidth-bound kernels: four waves per SIMD or more, LDS for the tree only


# ------------------------------------------------------------------------------------------------
# the operation-order restatement (tests/supervised_losses_emulation.py) against the f64 torch one
# ------------------------------------------------------------------------------------------------
def make_case(B, H, W, mask="face", inputs="random", seed=0):
    """numpy f32 inputs in the C ABI's layouts (shared with tests/test_gpu_supervised_losses.py).
    mask: face ({0,1} ellipses, `masks` and `masks_fill` different), fractional (k / 255), outside (values in [-0.5, 1.5]), ones.
    inputs: random; equal (depth == gt_depth on half the pixels); nan (one NaN depth pixel); pm50 (logits at +-50 among the others)."""
    rng = np.random.default_rng(seed + 1000 * B + 10 * H + W)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    r, c = np.mgrid[0:H, 0:W]
    ell = lambda s, i: (((c - W / 2.0 - i) / (s * 0.36 * W + 0.5)) ** 2 + ((r - H / 2.0 + i) / (s * 0.42 * H + 0.5)) ** 2) < 1
    if mask == "face":
        m, mf = (f(np.stack([ell(s, i) for i in range(B)])) for s in (1.0, 0.8))
        if B * H * W < 16:                                       # too few pixels for an ellipse: keep the masks' sums away from zero
            m, mf = np.ones((B, H, W), np.float32), np.ones((B, H, W), np.float32)
    elif mask == "fractional":
        m, mf = (f(rng.integers(0, 256, (B, H, W)) / 255.0) for _ in range(2))
    elif mask == "outside":
        m, mf = (f(rng.random((B, H, W)) * 2.0 - 0.5) for _ in range(2))
    else:
        m, mf = np.ones((B, H, W), np.float32), np.ones((B, H, W), np.float32)
    gt_depth = f(80.0 * rng.random((B, H, W)))
    depth = f(gt_depth + 5.0 * rng.standard_normal((B, H, W)))
    if inputs == "equal":
        keep = rng.random((B, H, W)) < 0.5
        depth = np.where(keep, gt_depth, depth)
    if inputs == "nan":
        depth.reshape(-1)[(B * H * W) // 2] = np.nan
        m.reshape(-1)[(B * H * W) // 2] = 1.0
    gt_albedo = f(0.05 + 0.9 * rng.random((B, H, W)))
    albedo = f(np.clip(gt_albedo[:, None] + 0.1 * rng.standard_normal((B, 3, H, W)), 0, 1))
    u = rng.standard_normal((B, 3))
    u = f(u / np.linalg.norm(u, axis=1, keepdims=True))
    l = rng.standard_normal((B, 3))                              # independent of u, as synthetic_batch draws it: 1 - cos is of order 1.
    # (The lighting term's gate is 2e-6 of mean |1 - cos|.  Any f32 evaluation of 1 - (u . l) carries ~1e-7 ABSOLUTE -- three
    #  products and two sums near 1, half an ulp of 1 each -- so for lights within ~18 degrees of the target (1 - cos < 0.05) that gate
    #  measures the number format, torch's own f32 included, not the kernel.)
    lightings = f(np.concatenate([0.4 + 0.2 * rng.random((B, 1)), l / np.linalg.norm(l, axis=1, keepdims=True)], axis=1))
    ambient = f(0.3 + 0.4 * rng.random(B))
    logits = f(3.0 * rng.standard_normal((B, 1, 5, 7)))
    if inputs == "pm50":
        logits.reshape(-1)[::3] = 50.0
        logits.reshape(-1)[1::3] = -50.0
    return dict(depth=depth, gt_depth=gt_depth, mask=m, albedo=albedo, gt_albedo=gt_albedo, mask_fill=mf, unit_light=u, ambient=ambient,
                lightings=lightings, logits=logits)


UPSTREAM = np.array([0.7, -1.3, 0.4, 1.1, -0.6], np.float32)


def torch_terms_and_grads(case, dtype, device, upstream=UPSTREAM, with_logits=True):
    """`train.generator_losses` and its autograd on the case's tensors in `dtype` on `device`: the five terms, the gradients of
    sum_k upstream[k] term[k], and sum_b |1 - cos_b| / B (the lighting term's scale).  The image terms are handed in, so that the
    function does not touch `rendered` and shapes below the SSIM's window can be used."""
    from geomconsistentfr_amd.train import generator_losses
    t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)
    B, H, W = case["depth"].shape
    depth, albedo = t(case["depth"]).reshape(B, 1, H, W).requires_grad_(), t(case["albedo"]).requires_grad_()
    unit, amb = t(case["unit_light"]).reshape(B, 3, 1, 1).requires_grad_(), t(case["ambient"]).reshape(B, 1, 1).requires_grad_()
    logits = t(case["logits"]).requires_grad_()
    batch = dict(images=torch.zeros(B, H, W, 3, dtype=dtype, device=device), depths=t(case["gt_depth"]).reshape(B, H, W, 1),
                 masks=t(case["mask"]).reshape(B, H, W, 1), albedo=t(case["gt_albedo"]).reshape(B, H, W, 1),
                 masks_fill=t(case["mask_fill"]).reshape(B, H, W, 1), lightings=t(case["lightings"]))
    one = torch.ones((), dtype=dtype, device=device)
    out = (albedo, depth, None, None, None, torch.zeros(B, 1, dtype=dtype, device=device), unit, amb)
    L = generator_losses(out, batch, logits if with_logits else torch.zeros(1, dtype=dtype, device=device),
                         image_terms=(None, 0 * one, one, torch.ones(B, 3, dtype=dtype, device=device)))
    wrt = dict(depth=depth, albedo=albedo, unit_light=unit, ambient=amb)
    keys = KEYS if with_logits else KEYS[:4]
    if with_logits:
        wrt["logits"] = logits
    total = sum(float(upstream[i]) * L[k] for i, k in enumerate(keys))
    grads = torch.autograd.grad(total, list(wrt.values()), allow_unused=True)
    cos = (unit.detach() * batch["lightings"][:, 1:4].reshape(B, 3, 1, 1)).sum(1).reshape(B)
    return dict(terms={k: float(L[k].detach()) for k in keys},
                grads={k: (torch.zeros_like(w) if g is None else g).detach().cpu().numpy().reshape(case_shape(case, k))
                       for (k, w), g in zip(wrt.items(), grads)},
                lighting_scale=float((1 - cos).abs().double().sum() / B))


def case_shape(case, k):
    B, H, W = case["depth"].shape
    return dict(depth=(B, H, W), albedo=(B, 3, H, W), unit_light=(B, 3), ambient=(B,), logits=case["logits"].shape)[k]


def emulate(case, upstream=UPSTREAM, with_logits=True):
    import supervised_losses_emulation as E
    c = case
    lg = c["logits"] if with_logits else None
    terms, sums = E.forward(c["depth"], c["gt_depth"], c["mask"], c["albedo"], c["gt_albedo"], c["mask_fill"], c["unit_light"],
                            c["ambient"], c["lightings"], lg)
    g = [None if u is None else np.float32(u) for u in upstream]
    grads = E.backward(c["depth"], c["gt_depth"], c["mask"], c["albedo"], c["gt_albedo"], c["mask_fill"], c["ambient"], c["lightings"],
                       lg, sums, g)
    return terms, sums, grads


def hold_to_torch(terms, grads, ref, tag, tol=2e-6):
    """the issue's gates against the code the head replaces; prints every figure before it asserts; returns the figures"""
    fig = {}
    for i, k in enumerate(KEYS[:len(ref["terms"])]):
        scale = ref["lighting_scale"] if k == "lighting" else abs(ref["terms"][k])
        both_nan = np.isnan(float(terms[i])) and np.isnan(ref["terms"][k])          # (a NaN input: the term is NaN on both sides)
        fig["term_" + k] = 0.0 if both_nan else abs(float(terms[i]) - ref["terms"][k]) / scale
    for k, g in ref["grads"].items():
        planes = [(grads[k][:, ch], g[:, ch]) for ch in range(3)] if k == "albedo" else [(grads[k], g)]
        fig["grad_" + k] = max(float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()) for a, b in planes)
    print("%s: %s" % (tag, " ".join("%s %.2e" % kv for kv in fig.items())))
    for k, v in fig.items():
        assert v <= tol, (tag, k, v)
    return fig


@pytest.mark.parametrize("mask,inputs", [("face", "random"), ("fractional", "equal"), ("outside", "pm50"), ("ones", "random")])
@pytest.mark.parametrize("shape", [(2, 32, 24), (3, 21, 37), (1, 1, 7)], ids=lambda s: "x".join(map(str, s)))
def test_the_emulation_is_within_2e6_of_the_f64_torch_restatement(shape, mask, inputs):
    case = make_case(*shape, mask=mask, inputs=inputs)
    terms, sums, grads = emulate(case)
    assert terms.dtype == np.float32 and terms.shape == (5,) and sums.dtype == np.float64
    assert all(g.dtype == np.float32 for g in grads.values())
    hold_to_torch(terms, grads, torch_terms_and_grads(case, torch.float64, "cpu"), "%s %s %s" % (shape, mask, inputs))
    if inputs == "equal":
        same = case["depth"] == case["gt_depth"]
        assert same.any() and (grads["depth"][same] == 0).all()


def test_the_emulation_without_logits_and_with_absent_upstreams():
    import supervised_losses_emulation as E
    case = make_case(2, 8, 12)
    terms, _, grads = emulate(case, with_logits=False)
    assert terms[4] == 0 and "logits" not in grads
    ref = torch_terms_and_grads(case, torch.float64, "cpu", with_logits=False)
    hold_to_torch(terms, grads, ref, "no logits")
    _, _, none = emulate(case, upstream=[None] * 5)
    assert all(not g.any() for g in none.values())
    # e^x: the plain-f32 form against numpy's, over the clamp's whole range and beyond it
    x = np.linspace(-100, 100, 20001).astype(np.float32)
    want = np.exp(np.clip(x.astype(np.float64), -87, 88))
    assert np.abs(E.exp_plain(x) / want - 1).max() <= 3e-7
    assert E.ulps(np.float32(1), np.nextafter(np.float32(1), np.float32(2))) == 1 and E.ulps(np.float32(0.0), np.float32(-0.0)) == 0
    assert not E.bit_equal(np.float32([0.0]), np.float32([-0.0])) and E.bit_equal(np.float32([np.nan]), np.float32([np.nan]))
