"""The training step's image-loss head as one fused HIP forward and one fused HIP backward (csrc/gcfr_losses.hip).

`image_losses(rendered, images, masks_fill)` computes what `train.generator_losses` and `Trainer.step` compute from
`rendered_images` with a chain of ATen launches (T8:619, 633, 641, 643):

    composite    = rendered * m + (1 - m) * images            bit-equal to the torch expression
    recon_sq_sum = sum (rendered * m - images * m)^2           over (B,3,H,W)
    mask_sum     = sum m                                       over (B,3,H,W): the mask counted once per channel
    ssim         = the per-(image, channel) mean of the Gaussian-window SSIM map of (composite, images), before the relu

The scalar arithmetic on top stays in torch, in `generator_losses`' own formulas, so corner cases behave as there (an all-zero
mask gives 0 / 0):  recon = 20 * recon_sq_sum / mask_sum;  DSSIM = 8 * (1 - relu(ssim).mean(1).mean()) / 2.
The gradient is with respect to `rendered` only.  There is no CPU path.

`supervised_losses(depth, albedo, unit_light, ambient_values, batch, logits_fake)` is the second head
(csrc/gcfr_supervised_losses.hip): the five terms of `generator_losses` that do not read `rendered_images` -- depth, ambient,
lighting, albedo, generator (T8:634-642) -- as one (5,) tensor from one fused forward, with one fused backward.
"""
import ctypes

import torch

from . import _lib

WIN_SIZE, WIN_SIGMA = 11, 1.5          # pytorch_msssim.ssim's defaults, as T8:643 calls it
_LAYOUTS = {"nhwc": 0, "nchw": 1}      # include/gcfr.h GCFR_IMAGES_NHWC / GCFR_IMAGES_NCHW


_WINDOW = None


def _window():
    """the 11 f32 weights `train._gauss_window` produces, as a host array (made once: it is a constant)"""
    global _WINDOW
    if _WINDOW is None:
        from .train import _gauss_window
        g = _gauss_window(WIN_SIZE, WIN_SIGMA, "cpu", torch.float32)
        _WINDOW = (ctypes.c_float * WIN_SIZE)(*g.tolist())
    return _WINDOW


class _ImageLossesFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendered, images, mask, layout, data_range):
        L_ = _lib.load()
        B, _, H, W = rendered.shape
        dev = rendered.device
        composite = torch.empty_like(rendered)
        ssim = torch.empty((B, 3), dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        ws_bytes = int(L_.gcfr_image_losses_workspace_bytes(B, H, W))
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=dev)
        win = _window()
        _lib.launch("gcfr_image_losses_fwd", dev, rendered, images, mask, layout, B, H, W, ctypes.cast(win, ctypes.c_void_p),
                    data_range, composite, ssim, sums, ws, ws_bytes, _lib.STREAM)
        recon_sq_sum, mask_sum = sums[0].float(), sums[1].float()
        ctx.save_for_backward(rendered, images, mask)
        ctx.layout, ctx.data_range = layout, data_range
        ctx.set_materialize_grads(False)          # an unused output's gradient arrives as None -> NULL, not as a tensor of zeros
        ctx.mark_non_differentiable(mask_sum)
        return composite, recon_sq_sum, mask_sum, ssim

    @staticmethod
    def backward(ctx, g_composite, g_recon, _g_mask_sum, g_ssim):
        rendered, images, mask = ctx.saved_tensors
        B, _, H, W = rendered.shape
        dev = rendered.device
        g_composite, g_recon, g_ssim = _lib.f32c(g_composite), _lib.f32c(g_recon), _lib.f32c(g_ssim)
        grad = torch.empty_like(rendered)
        win = _window()
        _lib.launch("gcfr_image_losses_bwd", dev, rendered, images, mask, ctx.layout, B, H, W, ctypes.cast(win, ctypes.c_void_p),
                    ctx.data_range, g_composite, g_ssim, g_recon, grad, _lib.STREAM)
        return grad, None, None, None, None


def image_losses(rendered: torch.Tensor, images: torch.Tensor, masks_fill: torch.Tensor = None, *, images_layout: str = "nhwc",
                 data_range: float = 1.0):
    """(composite (B,3,H,W), recon_sq_sum (), mask_sum (), ssim (B,3)) of `rendered` (B,3,H,W) against the photograph `images`
    ((B,H,W,3) for images_layout="nhwc", as batch["images"] holds it, or (B,3,H,W) for "nchw") under `masks_fill` (B,H,W),
    (B,H,W,1) or (B,1,H,W), any values; None = no mask (composite = rendered, m = 1).  All f32 on one ROCm device.
    `composite` and `ssim` are differentiable with respect to `rendered`, as is `recon_sq_sum`; `images` and `masks_fill` must not
    require grad."""
    if images_layout not in _LAYOUTS:
        raise ValueError("images_layout must be 'nhwc' or 'nchw', got %r" % (images_layout,))
    tensors = [t for t in (rendered, images, masks_fill) if t is not None]
    _lib.require_device(*tensors)
    if any(t.dtype != torch.float32 or t.device != rendered.device for t in tensors):
        raise _lib.GcfrError("image_losses: f32 tensors on one device")
    if images.requires_grad or (masks_fill is not None and masks_fill.requires_grad):
        raise _lib.GcfrError("image_losses differentiates with respect to `rendered` only: images / masks_fill must not require grad")
    if rendered.dim() != 4 or rendered.shape[1] != 3:
        raise _lib.GcfrError("rendered must be (B,3,H,W); got %s" % (tuple(rendered.shape),))
    B, _, H, W = rendered.shape
    want = (B, H, W, 3) if images_layout == "nhwc" else (B, 3, H, W)
    if tuple(images.shape) != want:
        raise _lib.GcfrError("images must be %s for images_layout=%r; got %s" % (want, images_layout, tuple(images.shape)))
    if masks_fill is not None:
        if masks_fill.numel() != B * H * W or tuple(masks_fill.shape) not in ((B, H, W), (B, H, W, 1), (B, 1, H, W)):
            raise _lib.GcfrError("masks_fill must be (B,H,W), (B,H,W,1) or (B,1,H,W); got %s" % (tuple(masks_fill.shape),))
        masks_fill = masks_fill.contiguous().reshape(B, H, W)
    return _ImageLossesFunction.apply(rendered.contiguous(), images.contiguous(), masks_fill, _LAYOUTS[images_layout],
                                      float(data_range))


class _SupervisedLossesFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, albedo, unit_light, ambient_values, logits, gt_depth, mask, gt_albedo, mask_fill, lightings):
        L_ = _lib.load()
        B, _, H, W = depth.shape
        dev = depth.device
        terms = torch.empty(5, dtype=torch.float32, device=dev)
        sums = torch.empty(4, dtype=torch.float64, device=dev)
        ws_bytes = int(L_.gcfr_supervised_losses_workspace_bytes(B, H, W))
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=dev)
        _lib.launch("gcfr_supervised_losses_fwd", dev, depth, gt_depth, mask, albedo, gt_albedo, mask_fill, unit_light, ambient_values,
                    lightings, logits, logits.numel() if logits is not None else 0, B, H, W, terms, sums, ws, ws_bytes, _lib.STREAM)
        ctx.save_for_backward(depth, albedo, unit_light, ambient_values, logits, gt_depth, mask, gt_albedo, mask_fill, lightings, sums)
        return terms

    @staticmethod
    def backward(ctx, g_terms):
        depth, albedo, unit_light, ambient_values, logits, gt_depth, mask, gt_albedo, mask_fill, lightings, sums = ctx.saved_tensors
        B, _, H, W = depth.shape
        dev = depth.device
        g = g_terms.to(torch.float32).contiguous()                 # stays on the device: the kernel reads the five values there
        gp = [g.data_ptr() + 4 * k for k in range(5)]
        grad_depth, grad_albedo = torch.empty_like(depth), torch.empty_like(albedo)
        grad_unit_light, grad_ambient = torch.empty_like(unit_light), torch.empty_like(ambient_values)
        grad_logits = torch.empty_like(logits) if logits is not None else None
        _lib.launch("gcfr_supervised_losses_bwd", dev, depth, gt_depth, mask, albedo, gt_albedo, mask_fill, ambient_values, lightings,
                    logits, logits.numel() if logits is not None else 0, B, H, W, sums,
                    gp[0], gp[1], gp[2], gp[3], gp[4] if logits is not None else None,
                    grad_depth, grad_albedo, grad_unit_light, grad_ambient, grad_logits, _lib.STREAM)
        return grad_depth, grad_albedo, grad_unit_light, grad_ambient, grad_logits, None, None, None, None, None


_SUPERVISED_BATCH_KEYS = ("depths", "masks", "albedo", "masks_fill")


def supervised_losses(depth: torch.Tensor, albedo: torch.Tensor, unit_light: torch.Tensor, ambient_values: torch.Tensor, batch,
                      logits_fake: torch.Tensor = None) -> torch.Tensor:
    """The (5,) f32 tensor (depth, ambient, lighting, albedo, generator) of `train.generator_losses`' terms T8:634-642 for
    `depth` (B,1,H,W), `albedo` (B,3,H,W), `unit_light` (B,3,1,1), `ambient_values` (B,1,1) -- RelightNet.forward's out[1], out[0],
    out[6], out[7] -- against batch["depths"], ["masks"], ["albedo"], ["masks_fill"] (each (B,H,W,1)) and ["lightings"] (B,4), and
    PatchGAN's `logits_fake` for the composite (any shape; None: the generator slot is exactly 0 and has no gradient).  All f32 on
    one ROCm device.  Differentiable with respect to the four network outputs and the logits; the batch's tensors must not
    require grad."""
    gts = [batch[k] for k in _SUPERVISED_BATCH_KEYS] + [batch["lightings"]]
    tensors = [depth, albedo, unit_light, ambient_values] + gts + ([logits_fake] if logits_fake is not None else [])
    _lib.require_device(*tensors)
    if any(t.dtype != torch.float32 or t.device != depth.device for t in tensors):
        raise _lib.GcfrError("supervised_losses: f32 tensors on one device")
    if any(t.requires_grad for t in gts):
        raise _lib.GcfrError("supervised_losses differentiates with respect to the network's outputs and the logits only: the "
                             "batch's tensors must not require grad")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise _lib.GcfrError("depth must be (B,1,H,W); got %s" % (tuple(depth.shape),))
    B, _, H, W = depth.shape
    if tuple(albedo.shape) != (B, 3, H, W):
        raise _lib.GcfrError("albedo must be %s; got %s" % ((B, 3, H, W), tuple(albedo.shape)))
    if tuple(unit_light.shape) != (B, 3, 1, 1) or tuple(ambient_values.shape) != (B, 1, 1):
        raise _lib.GcfrError("unit_light must be %s and ambient_values %s; got %s and %s"
                             % ((B, 3, 1, 1), (B, 1, 1), tuple(unit_light.shape), tuple(ambient_values.shape)))
    for k in _SUPERVISED_BATCH_KEYS:
        if tuple(batch[k].shape) != (B, H, W, 1):
            raise _lib.GcfrError("batch[%r] must be %s; got %s" % (k, (B, H, W, 1), tuple(batch[k].shape)))
    if tuple(batch["lightings"].shape) != (B, 4):
        raise _lib.GcfrError("batch['lightings'] must be %s; got %s" % ((B, 4), tuple(batch["lightings"].shape)))
    if logits_fake is not None and logits_fake.numel() == 0:
        raise _lib.GcfrError("logits_fake must not be empty (pass None for no generator term)")
    c = lambda t: t.contiguous()
    return _SupervisedLossesFunction.apply(c(depth), c(albedo), c(unit_light), c(ambient_values),
                                           c(logits_fake) if logits_fake is not None else None,
                                           c(batch["depths"]), c(batch["masks"]), c(batch["albedo"]), c(batch["masks_fill"]),
                                           c(batch["lightings"]))
