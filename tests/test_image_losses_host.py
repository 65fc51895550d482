"""CPU: the image-loss head's plumbing (csrc/gcfr_losses.hip, include/gcfr.h, losses.py, TrainConfig.image_losses) -- the three
symbols are declared, bound and exported; argument validation happens on the host before any launch; the workspace formula is the
documented one; the switch validates its value; there is no CPU path; `generator_losses` without `image_terms` computes what it
always did, and with torch-made terms the same numbers; the new kernels are spill-free in the built library."""
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
