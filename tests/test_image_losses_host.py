"""CPU: the image-loss head's plumbing (csrc/gcfr_losses.hip, include/gcfr.h, losses.py, TrainConfig.image_losses) -- the three
symbols are declared, bound and exported; argument validation happens on the host before any launch; the workspace formula is the
documented one; the switch validates its value; there is no CPU path; `generator_losses` without `image_terms` computes what it
always did, and with torch-made terms the same numbers; the new kernels are spill-free in the built library.
And the numpy-f32 restatement of the kernel's operation order (tests/image_losses_emulation.py), which
tests/test_gpu_image_losses_regimes.py holds the kernel to bit for bit, is itself held to the f64 restatement here, under the gates
of tests/test_gpu_image_losses.py, so that it is a checked statement and not a second opinion."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_abi import declared_symbols
from test_kernel_resources import LLVM, _kernel_metadata

SYMBOLS = ("gcfr_image_losses_workspace_bytes", "gcfr_image_losses_fwd", "gcfr_image_losses_bwd")


def test_the_three_symbols_are_declared_bound_and_exported():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    for s in SYMBOLS:
        assert s in declared_symbols(), s
        assert s in _lib.exported_symbols(), s
        assert hasattr(L, s), s
    assert L.gcfr_abi_version() == 6          # no existing entry point or struct changed


def test_workspace_bytes_is_the_documented_formula():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    for B, H, W in ((1, 11, 11), (4, 256, 256), (2, 64, 40), (1, 33, 47), (3, 21, 128), (32, 256, 256), (1, 4096, 4096)):
        tiles = -(-H // 16) * -(-W // 32)
        assert L.gcfr_image_losses_workspace_bytes(B, H, W) == 8 * (5 * B * tiles + 2 * B), (B, H, W)
    for B, H, W in ((0, 64, 64), (1, 10, 64), (1, 64, 10), (1, 4097, 64), (1, 64, 4097)):
        assert L.gcfr_image_losses_workspace_bytes(B, H, W) == 0, (B, H, W)


def test_invalid_arguments_are_rejected_before_any_launch():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = ctypes.c_void_p(4096)                                   # a dummy non-null, aligned "device" pointer: never dereferenced
    win = (ctypes.c_float * 11)(*([1.0 / 11] * 11))
    w = ctypes.cast(win, ctypes.c_void_p)
    big = 1 << 30
    fwd_args = dict(rendered=p, images=p, mask=p, layout=0, B=2, H=64, W=40, window=w, dr=1.0, composite=p, ssim=p, sums=p, ws=p,
                    ws_bytes=big, stream=None)
    bwd_args = dict(rendered=p, images=p, mask=p, layout=0, B=2, H=64, W=40, window=w, dr=1.0, g_composite=p, g_ssim=p, g_recon=p,
                    grad=p, stream=None)
    fwd = lambda **kw: L.gcfr_image_losses_fwd(*{**fwd_args, **kw}.values())      # (dicts keep the argument order)
    bwd = lambda **kw: L.gcfr_image_losses_bwd(*{**bwd_args, **kw}.values())
    for name in ("rendered", "images", "window", "composite", "ssim", "sums", "ws"):
        assert fwd(**{name: None}) == -1, name
    for name in ("rendered", "images", "window", "grad"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        assert call(H=10) == -1 and call(W=10) == -1 and call(H=4097) == -1 and call(W=4097) == -1
        assert call(B=0) == -1 and call(B=65536) == -1
        assert call(layout=2) == -1 and call(layout=-1) == -1
        assert call(dr=0.0) == -1
    need = L.gcfr_image_losses_workspace_bytes(2, 64, 40)
    assert need > 0 and fwd(ws_bytes=need - 1) == -1 and fwd(ws_bytes=0) == -1
    assert fwd(ws=ctypes.c_void_p(4100)) == -1                  # not 8-byte aligned


def test_trainconfig_switch_validates_its_value():
    from geomconsistentfr_amd.train import TrainConfig
    assert TrainConfig().image_losses == "torch"                # the default does not change
    assert TrainConfig(image_losses="hip").image_losses == "hip"
    with pytest.raises(ValueError, match="image_losses"):
        TrainConfig(image_losses="cuda")


def test_image_losses_has_no_cpu_path_and_differentiates_rendered_only():
    from geomconsistentfr_amd._lib import GcfrError
    from geomconsistentfr_amd.losses import image_losses
    r, img, m = torch.rand(1, 3, 16, 16), torch.rand(1, 16, 16, 3), torch.ones(1, 16, 16, 1)
    with pytest.raises(GcfrError, match="no CPU path"):
        image_losses(r, img, m)
    with pytest.raises(GcfrError, match="no CPU path"):
        image_losses(r, img)
    with pytest.raises(ValueError):
        image_losses(r, img, m, images_layout="hwcn")


def _cpu_out_and_batch(B=2, H=32, W=24, seed=3):
    from geomconsistentfr_amd.train import synthetic_batch
    g = torch.Generator().manual_seed(seed)
    batch = synthetic_batch(B, 7, H, W)
    rnd = lambda *s: torch.rand(*s, generator=g)
    unit = F.normalize(torch.randn(B, 3, 1, 1, generator=g), dim=1)
    out = (rnd(B, 3, H, W), 80 * rnd(B, 1, H, W), None, None, None, rnd(B, 3, H, W).requires_grad_(), unit, rnd(B, 1, 1))
    return out, batch, torch.randn(B, 1, 6, 6, generator=g)


def test_generator_losses_without_image_terms_is_what_it_was():
    """The terms restated here are the expressions of the function before `image_terms` existed (T8:633-645)."""
    from geomconsistentfr_amd.train import generator_losses, ssim
    out, batch, logits = _cpu_out_and_batch()
    got = generator_losses(out, batch, logits, image_terms=None)
    assert {k: float(v.detach()) for k, v in generator_losses(out, batch, logits).items()} == {k: float(v.detach()) for k, v in got.items()}
    rendered = out[5]
    img = batch["images"].permute(0, 3, 1, 2)
    m3 = batch["masks_fill"].permute(0, 3, 1, 2).expand(-1, 3, -1, -1)
    recon = 20.0 * F.mse_loss(rendered * m3, img * m3, reduction="sum") / m3.sum()
    dssim = 8.0 * (1 - ssim(rendered * m3 + (1.0 - m3) * img, img, data_range=1.0, size_average=True, nonnegative_ssim=True)) / 2.0
    assert float(got["recon"].detach()) == float(recon.detach()) and float(got["DSSIM"].detach()) == float(dssim.detach())
    assert set(got) == {"recon", "depth", "ambient", "lighting", "albedo", "generator", "DSSIM", "total"}
    assert float(got["total"].detach()) == float(sum(v for k, v in got.items() if k != "total").detach())


def test_generator_losses_with_torch_made_image_terms_gives_the_same_terms_and_gradient():
    """`image_terms` carries (composite, recon_sq_sum, mask_sum, ssim (B,3) before the relu); made with torch on the CPU they must
    reproduce the built-in path: the scalar formulas on top are the same ones."""
    from geomconsistentfr_amd.train import _gauss_window, generator_losses
    out, batch, logits = _cpu_out_and_batch()
    ref = generator_losses(out, batch, logits)
    g_ref, = torch.autograd.grad(ref["total"], out[5])
    rendered = out[5]
    img = batch["images"].permute(0, 3, 1, 2)
    m3 = batch["masks_fill"].permute(0, 3, 1, 2).expand(-1, 3, -1, -1)
    composite = rendered * m3 + (1.0 - m3) * img
    gw = _gauss_window(11, 1.5, "cpu", torch.float32)
    blur = lambda t: F.conv2d(F.conv2d(t, gw.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3), gw.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)
    mu1, mu2, xx, yy, xy = blur(composite), blur(img), blur(composite * composite), blur(img * img), blur(composite * img)
    cs = (2 * (xy - mu1 * mu2) + 0.03 ** 2) / ((xx - mu1 * mu1) + (yy - mu2 * mu2) + 0.03 ** 2)
    ssim_bc = (((2 * mu1 * mu2 + 0.01 ** 2) / (mu1 * mu1 + mu2 * mu2 + 0.01 ** 2)) * cs).flatten(2).mean(-1)
    terms = (composite, ((rendered * m3 - img * m3) ** 2).sum(), m3.sum(), ssim_bc)
    got = generator_losses(out, batch, logits, image_terms=terms)
    for k in ref:
        np.testing.assert_allclose(float(got[k].detach()), float(ref[k].detach()), rtol=1e-6, err_msg=k)
    g_got, = torch.autograd.grad(got["total"], out[5])
    assert float((g_got - g_ref).abs().max()) <= 1e-5 * float(g_ref.abs().max())


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_new_kernels_use_no_scratch(tmp_path):
    k = _kernel_metadata(tmp_path)
    mine = {n: v for n, v in k.items() if n.startswith("image_losses_")}
    assert set(mine) == {"image_losses_fwd_kernel", "image_losses_finish_image_kernel", "image_losses_finish_batch_kernel",
                         "image_losses_bwd_kernel"}, sorted(mine)
    for n, v in mine.items():
        assert v["scratch"] == 0, (n, v)
    assert mine["image_losses_fwd_kernel"]["lds"] <= 160 * 1024 // 3        # three workgroups per CU
    assert mine["image_losses_bwd_kernel"]["lds"] <= 64 * 1024              # static LDS; two workgroups of 512 lanes per CU
    assert mine["image_losses_bwd_kernel"]["vgpr"] <= 128                   # 512 lanes per workgroup


# ------------------------------------------------------------------------------------------------
# the operation-order restatement (tests/image_losses_emulation.py) against the f64 one
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["face", "fractional", "none"])
@pytest.mark.parametrize("shape", [(2, 64, 40), (1, 33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_the_emulation_keeps_the_f64_gates_on_white_noise(shape, mask):
    """No library call: white-noise inputs, masks, upstream gradients, the f64 reference and the gates (composite bit-equal to the
    torch f32 expression; ssim / sq_sum / mask_sum 2e-6 relative; gradient 2e-5 of its largest entry for each upstream alone and for
    all together) are those of tests/test_gpu_image_losses.py."""
    import image_losses_emulation as E
    import test_gpu_image_losses as G
    B, H, W = shape
    X, Y = G._pair(B, H, W)
    M, ups = G._mask(mask, B, H, W), G._upstreams(B, H, W)
    ref = G._reference(X, Y, M, ups)
    win = E.gauss_window()
    comp, s, sq, msum, smap = E.forward(X, Y, M, win, 1.0)
    assert comp.dtype == s.dtype == smap.dtype == np.float32 and sq.dtype == msum.dtype == np.float64
    assert smap.shape == (B, 3, H - 10, W - 10) and s.shape == (B, 3)
    Gc, Gs, gq = ups
    sel = dict(composite=dict(g_composite=Gc), ssim=dict(g_ssim=Gs), recon=dict(g_recon=gq),
               all=dict(g_composite=Gc, g_ssim=Gs, g_recon=gq))
    grads = {k: E.backward(X, Y, M, win, 1.0, **kw) for k, kw in sel.items()}
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))
    e_s, e_sq, e_m = rel(s, ref["ssim"]), rel(sq, ref["sq"]), rel(msum, ref["msum"])
    e_g = {k: float(np.abs(g.astype(np.float64) - ref["grads"][k]).max() / np.abs(ref["grads"][k]).max()) for k, g in grads.items()}
    print("%s %s: ssim %.2e sq %.2e msum %.2e grad %s" % (shape, mask, e_s, e_sq, e_m, " ".join("%s %.2e" % kv for kv in sorted(e_g.items()))))
    assert E.bit_equal(comp, ref["composite"])
    assert e_s <= 2e-6 and e_sq <= 2e-6 and e_m <= 2e-6, (e_s, e_sq, e_m)
    for k, e in e_g.items():
        assert grads[k].dtype == np.float32 and np.abs(ref["grads"][k]).max() > 0
        assert e <= 2e-5, (k, e)


def test_the_emulation_refuses_anything_but_float32():
    import image_losses_emulation as E
    win = E.gauss_window()
    assert win.dtype == np.float32 and win.shape == (11,) and np.array_equal(win, win[::-1])      # symmetric: blurT reuses it unflipped
    X = np.full((1, 3, 11, 11), 0.5, np.float32)
    for bad in (dict(rendered=X.astype(np.float64)), dict(images_nchw=X.astype(np.float64)), dict(window=win.astype(np.float64)),
                dict(mask=np.ones((1, 11, 11)))):
        with pytest.raises(AssertionError):
            E.forward(**{**dict(rendered=X, images_nchw=X, mask=None, window=win), **bad})
    with pytest.raises(AssertionError):
        E.backward(X, X, None, win, g_ssim=np.ones((1, 3)))
    with pytest.raises(AssertionError):
        E.backward(X, X, None, win, g_recon=0.37)
    C1, C2 = E.consts(1.0)
    assert C1.dtype == C2.dtype == np.float32 and C1 == np.float32(1e-4) and C2 == np.float32(9e-4)


def test_the_emulations_ulp_distance_and_bit_comparison():
    import image_losses_emulation as E
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert E.ulps(one, one) == 0 and E.ulps(one, up) == 1 and E.ulps(-one, -up) == 1
    assert E.ulps(np.float32(0.0), np.float32(-0.0)) == 0
    assert E.ulps(np.nextafter(np.float32(0), one), -np.nextafter(np.float32(0), one)) == 2
    a = np.array([1.0, np.nan, 0.0], np.float32)
    assert E.bit_equal(a, a.copy())
    assert not E.bit_equal(a, np.array([up, np.nan, 0.0], np.float32))
    assert not E.bit_equal(a, np.array([1.0, 2.0, 0.0], np.float32))
    assert not E.bit_equal(a, np.array([1.0, np.nan, -0.0], np.float32))
