"""GPU: the fused supervised-loss head (losses.supervised_losses, csrc/gcfr_supervised_losses.hip).

Held to the numpy-f32 restatement of its operation order (tests/supervised_losses_emulation.py, itself held to f64 torch by
tests/test_supervised_losses_host.py): the four gradient planes (depth, the three albedo channels) and the three small gradients
(unit_light, ambient_values, logits) bit for bit; the five terms within one f32 ulp (the association of the f64 sums).
Held to the code it replaces -- `train.generator_losses` and its autograd on the same device tensors, in f32: terms within 2e-6
relative (the lighting term, which can cancel, within 2e-6 of sum_b |1 - cos_b| / B), gradients within 2e-6 of each plane's largest
entry.  Every case prints its figures before it asserts.

Shapes (B,H,W): (1,1,1); (1,1,7) shorter than a vector; (3,21,37) H W odd, the albedo planes misaligned; (2,64,40); 1023, 1024 and
1025 pixels around the 1024 a workgroup owns (1024 = 32 x 32 takes the vector path); B = 65 and 130 at 11 x 11 (more images than a
wave of the finishing launch) and B = 300 (more than its 256 lanes); (4,256,256) once.  Masks: {0,1} ellipses, k / 255, values in
[-0.5, 1.5], all ones, `masks` always different from `masks_fill`.  Inputs: random; depth == gt_depth on half the pixels; a NaN
pixel; logits at +-50.

Measured on an MI355X, largest over the cases below: every gradient bit-equal to the restatement, the terms 0 ulp from it; against
`generator_losses` in f32: terms depth 1.1e-7, ambient 0, lighting 1.1e-7, albedo 1.4e-7, generator 8.8e-8; gradients depth 8.5e-8,
albedo 1.3e-7, unit_light 8.8e-8, ambient 0, logits 2.0e-7; each upstream gradient alone 1.7e-7 (the logits'), 0 for the others."""
import numpy as np
import pytest
import torch

import supervised_losses_emulation as E
from test_supervised_losses_host import KEYS, UPSTREAM, case_shape, emulate, hold_to_torch, make_case, torch_terms_and_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = [((1, 1, 1), "ones", "random"), ((1, 1, 7), "fractional", "random"), ((3, 21, 37), "face", "random"),
         ((3, 21, 37), "outside", "equal"), ((2, 64, 40), "face", "equal"), ((2, 64, 40), "fractional", "nan"),
         ((2, 64, 40), "ones", "pm50"), ((1, 1, 1023), "fractional", "random"), ((1, 32, 32), "outside", "random"),
         ((1, 25, 41), "face", "pm50"), ((65, 11, 11), "face", "random"), ((130, 11, 11), "fractional", "pm50"),
         ((300, 2, 3), "ones", "random"), ((4, 256, 256), "face", "random")]


def _device_inputs(case, with_logits=True):
    B, H, W = case["depth"].shape
    t = lambda a: torch.from_numpy(a).to(DEV)
    wrt = dict(depth=t(case["depth"]).reshape(B, 1, H, W).requires_grad_(), albedo=t(case["albedo"]).requires_grad_(),
               unit_light=t(case["unit_light"]).reshape(B, 3, 1, 1).requires_grad_(), ambient=t(case["ambient"]).reshape(B, 1, 1).requires_grad_())
    if with_logits:
        wrt["logits"] = t(case["logits"]).requires_grad_()
    batch = dict(depths=t(case["gt_depth"]).reshape(B, H, W, 1), masks=t(case["mask"]).reshape(B, H, W, 1),
                 albedo=t(case["gt_albedo"]).reshape(B, H, W, 1), masks_fill=t(case["mask_fill"]).reshape(B, H, W, 1),
                 lightings=t(case["lightings"]))
    return wrt, batch


def _run_op(case, upstream=UPSTREAM, with_logits=True):
    """-> terms (5,) f32, {name: gradient of sum_k upstream[k] terms[k]} as numpy"""
    from geomconsistentfr_amd.losses import supervised_losses
    wrt, batch = _device_inputs(case, with_logits)
    terms = supervised_losses(wrt["depth"], wrt["albedo"], wrt["unit_light"], wrt["ambient"], batch, wrt.get("logits"))
    assert terms.shape == (5,) and terms.dtype == torch.float32
    grads = torch.autograd.grad((terms * torch.from_numpy(np.asarray(upstream, np.float32)).to(DEV)).sum(), list(wrt.values()))
    return terms.detach().cpu().numpy(), {k: g.cpu().numpy().reshape(case_shape(case, k)) for k, g in zip(wrt, grads)}


def _hold_to_emulation(terms, grads, e_terms, e_grads, tag):
    u = E.ulps(terms, e_terms)
    u = np.where(np.isnan(terms) & np.isnan(e_terms), 0, u)
    print("%s: terms' ulps from the restatement %s" % (tag, u.tolist()))
    assert (u <= 1).all(), (tag, terms, e_terms)
    assert set(grads) == set(e_grads)
    for k in grads:
        assert E.bit_equal(grads[k], e_grads[k]), (tag, k, int((grads[k].view(np.uint32) != e_grads[k].view(np.uint32)).sum()))


@pytest.mark.parametrize("shape,mask,inputs", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_terms_and_gradients_against_the_restatement_and_against_generator_losses(shape, mask, inputs):
    case = make_case(*shape, mask=mask, inputs=inputs)
    tag = "%s %s %s" % (shape, mask, inputs)
    terms, grads = _run_op(case)
    e_terms, _, e_grads = emulate(case)
    _hold_to_emulation(terms, grads, e_terms, e_grads, tag)
    hold_to_torch(terms, grads, torch_terms_and_grads(case, torch.float32, DEV), tag)
    if inputs == "equal":                                        # exact zeros give a zero gradient
        same = case["depth"] == case["gt_depth"]
        assert same.sum() > same.size // 4 and (grads["depth"][same] == 0).all()
    if inputs == "nan":                                          # the NaN stays in its own term
        assert np.isnan(terms[0]) and np.isfinite(terms[1:]).all()
        assert all(np.isfinite(g).all() for k, g in grads.items() if k != "depth")
    if inputs == "pm50":                                         # the stable softplus: finite, and its gradient in [-|g| / n, 0]
        n = case["logits"].size
        assert np.isfinite(terms[4]) and terms[4] > 0.01 * 50 / 3 * 0.99
        s = grads["logits"] / (UPSTREAM[4] * 0.01 / n)
        assert np.isfinite(s).all() and s.min() >= -1.000001 and s.max() <= 0.0 and s.min() < -0.999999


def test_an_all_zero_mask_gives_a_nan_term_and_no_fault():
    case = make_case(2, 16, 20, mask="fractional")
    case["mask"][:] = 0.0
    terms, grads = _run_op(case)
    torch.cuda.synchronize()
    e_terms, _, _ = emulate(case)
    assert np.isnan(terms[0]) and np.isnan(e_terms[0]) and np.isfinite(terms[1:]).all()
    assert (E.ulps(terms[1:], e_terms[1:]) <= 1).all()
    assert all(np.isfinite(g).all() for k, g in grads.items() if k != "depth")      # (the depth gradient under 0 / 0 is not pinned)


def test_two_calls_return_the_same_bits_and_a_side_stream_does_too():
    case = make_case(4, 64, 64, mask="fractional")
    first = _run_op(case)
    second = _run_op(case)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = _run_op(case)
    side.synchronize()
    for other in (second, third):
        assert E.bit_equal(first[0], other[0])
        for k in first[1]:
            assert E.bit_equal(first[1][k], other[1][k]), k


def test_without_logits_the_generator_slot_is_exactly_zero_and_has_no_gradient():
    from geomconsistentfr_amd.losses import supervised_losses
    case = make_case(3, 21, 37)
    terms, grads = _run_op(case, with_logits=False)
    e_terms, _, e_grads = emulate(case, with_logits=False)
    assert terms[4] == 0.0 and not np.signbit(terms[4]) and "logits" not in grads
    _hold_to_emulation(terms, grads, e_terms, e_grads, "no logits")
    hold_to_torch(terms, grads, torch_terms_and_grads(case, torch.float32, DEV, with_logits=False), "no logits")
    wrt, batch = _device_inputs(case, with_logits=False)
    t = supervised_losses(wrt["depth"], wrt["albedo"], wrt["unit_light"], wrt["ambient"], batch, None)
    g = torch.autograd.grad(t[4], list(wrt.values()))          # the slot is part of the output, its gradient is all zeros
    assert all(not x.any() for x in g)


@pytest.mark.parametrize("k", range(5), ids=KEYS)
def test_each_upstream_gradient_alone_matches_autograd(k):
    case = make_case(2, 64, 40, mask="fractional", seed=5)
    one_hot = [0.0] * 5
    one_hot[k] = float(UPSTREAM[k])
    terms, grads = _run_op(case, upstream=one_hot)
    ref = torch_terms_and_grads(case, torch.float32, DEV, upstream=one_hot)
    own = dict(depth="depth", ambient="ambient", lighting="unit_light", albedo="albedo", generator="logits")[KEYS[k]]
    for name, g in grads.items():
        if name != own:
            assert not g.any() and not ref["grads"][name].any(), name
    assert grads[own].any()
    err = float(np.abs(grads[own].astype(np.float64) - ref["grads"][own]).max() / np.abs(ref["grads"][own]).max())
    print("%s alone: %.2e" % (KEYS[k], err))
    assert err <= 2e-6
    # through the C ABI the other four upstream gradients are NULL: the same bits, and exact zeros elsewhere
    e = emulate(case, upstream=[UPSTREAM[j] if j == k else None for j in range(5)])[2]
    got = _bwd_through_the_abi(case, k)
    for name in got:
        assert E.bit_equal(got[name], e[name]), name
        assert E.bit_equal(got[name], grads[name]) or name != own


def _bwd_through_the_abi(case, k):
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    B, H, W = case["depth"].shape
    d = {n: torch.from_numpy(a).to(DEV) for n, a in case.items()}
    terms, sums = torch.empty(5, device=DEV), torch.empty(4, dtype=torch.float64, device=DEV)
    nbytes = L.gcfr_supervised_losses_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    n = case["logits"].size
    st = torch.cuda.current_stream(DEV).cuda_stream
    p = lambda name: d[name].data_ptr()
    _lib.check(L.gcfr_supervised_losses_fwd(p("depth"), p("gt_depth"), p("mask"), p("albedo"), p("gt_albedo"), p("mask_fill"), p("unit_light"),
                                            p("ambient"), p("lightings"), p("logits"), n, B, H, W, terms.data_ptr(), sums.data_ptr(),
                                            ws.data_ptr(), nbytes, st), "fwd")
    g = torch.tensor([float(UPSTREAM[k])], device=DEV)
    gp = [g.data_ptr() if j == k else None for j in range(5)]
    out = dict(depth=torch.full((B, H, W), 7.0, device=DEV), albedo=torch.full((B, 3, H, W), 7.0, device=DEV),
               unit_light=torch.full((B, 3), 7.0, device=DEV), ambient=torch.full((B,), 7.0, device=DEV),
               logits=torch.full(case["logits"].shape, 7.0, device=DEV))
    _lib.check(L.gcfr_supervised_losses_bwd(p("depth"), p("gt_depth"), p("mask"), p("albedo"), p("gt_albedo"), p("mask_fill"), p("ambient"),
                                            p("lightings"), p("logits"), n, B, H, W, sums.data_ptr(), *gp, out["depth"].data_ptr(),
                                            out["albedo"].data_ptr(), out["unit_light"].data_ptr(), out["ambient"].data_ptr(),
                                            out["logits"].data_ptr(), st), "bwd")
    return {name: t.cpu().numpy() for name, t in out.items()}


def test_refusals_on_the_device():
    from geomconsistentfr_amd._lib import GcfrError
    from geomconsistentfr_amd.losses import supervised_losses
    case = make_case(2, 8, 12)
    wrt, batch = _device_inputs(case)
    args = lambda **kw: [{**wrt, **kw}[n] for n in ("depth", "albedo", "unit_light", "ambient")]
    with pytest.raises(GcfrError, match="f32"):
        supervised_losses(*args(depth=wrt["depth"].double()), batch, wrt["logits"])
    with pytest.raises(GcfrError, match="albedo must be"):
        supervised_losses(*args(albedo=wrt["albedo"][:, :2]), batch, wrt["logits"])
    with pytest.raises(GcfrError, match="depth must be"):
        supervised_losses(*args(depth=wrt["depth"][:, 0]), batch, wrt["logits"])
    with pytest.raises(GcfrError, match="masks"):
        supervised_losses(*args(), {**batch, "masks": batch["masks"][..., 0]}, wrt["logits"])
    with pytest.raises(GcfrError, match="must not require grad"):
        supervised_losses(*args(), {**batch, "depths": batch["depths"].clone().requires_grad_()}, wrt["logits"])
    with pytest.raises(GcfrError, match="no CPU path"):
        supervised_losses(*args(), {**batch, "lightings": batch["lightings"].cpu()}, wrt["logits"])
