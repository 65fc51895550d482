"""Callers of the render block on the inference side, as functions.

The reference's three test scripts are `main()` bodies with hard-coded paths; what they DO with the model is:

  relight_single_image    test_relight_single_image.py:569-620 (S1) -- one image, one target light, composite
  relight_batch           test_raytracing_relighting_CelebAHQ_DSSIM_8x.py:552-608 (S8) -- many (image, light) pairs
  lighting_transfer       test_relight_single_image_lighting_transfer.py:527-579 (SLT) -- two passes: estimate the
                          reference image's light, relight the input with it

The reference runs one image per forward (batch_size = 1 hard-coded); here a whole batch goes through one forward.
Light directions the reference ships in source (S1:519-562) are exposed as LIGHT_DIRECTIONS.
"""
from typing import Dict

import numpy as np
import torch

from . import postprocess as pp
from ._lib import GcfrError
from .lighting import (MAX_FIT_LIGHTS, _check_environment, _environment_lights, combine_lights, environment_lights,
                       environment_lights_frames, fit_light_rgb, rig_frames_u8, sphere_directions)
from .relightnet import RelightNetLightingTransfer, RelightNetSingleImage

# name -> (x, y, z), test_relight_single_image.py:519-562
LIGHT_DIRECTIONS: Dict[str, tuple] = {
    "multipie_04": (0.7518, 0.0, 0.6594),
    "multipie_14": (0.6893, 0.3991, 0.6047),
    "multipie_05": (0.5145, 0.0, 0.8575),
    "multipie_09": (-0.5843, 0.0, 0.8115),
    "multipie_10": (-0.7574, 0.0, 0.6529),
    "multipie_18": (-0.7076, 0.3892, 0.5897),
    "multipie_17": (-0.5151, 0.4722, 0.7154),
    "multipie_15": (0.4478, 0.4925, 0.7463),
    "top_A00E45": (0.0, 0.7071, 0.7071),
    "bottom_left_A60E-20": (-0.8138, -0.3420, 0.4698),
    "bottom_right_A-60E-20": (0.8138, -0.3420, 0.4698),
}


def camera_matrix(focal: float, H: int = 256, W: int = 256, device="cpu") -> torch.Tensor:
    """(1,3,3) float64 intrinsics as built at S1:566-572 (focal 1570) / SLT:528-534 (focal 700)."""
    K = torch.zeros(1, 3, 3, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = focal
    K[:, 2, 2] = 1.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    return K.to(device)


def _is_transfer(model) -> bool:
    return isinstance(model, RelightNetLightingTransfer)


def _default_focal(transfer: bool, focal):
    """the scripts' focal length for the model kind (S1:566: 1570; SLT:528: 700) unless the caller gives one"""
    return (700.0 if transfer else 1570.0) if focal is None else focal


def _as(a, device, dtype=torch.float32, single=None) -> torch.Tensor:
    """`a` (a tensor, an array, nested numbers) as a `dtype` tensor on `device` (None: where it is); one of rank `single` is a
    single item -- one photograph (H,W,3), one light (3,), one rig (L,3), one map (He,We,3) -- and gets a leading axis"""
    t = (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dtype)        # (converted where it is, then moved)
    t = t[None] if t.dim() == single else t
    return t if device is None else t.to(device)


@torch.no_grad()
def relight_batch(model, images, masks_u8, lights, ambient: float = 0.5,
                  focal: float = None, device="cuda", epoch: int = 200):
    """images (B,H,W,3) float [0,1]; masks_u8 (H,W) shared skin mask (the S1/S8 model takes ONE mask per
    forward, S1:488) ; lights (B,3) target directions.  RelightNetSingleImage: the lighting head's first output is the ambient
    the model uses (plus the model's ambient_offset); `ambient` only feeds the unused target argument, as in S1:588 (focal
    1570).  RelightNetLightingTransfer: `ambient` IS the target ambient (SLT:545; focal 700).
    Returns the model's 10- / 12-tuple (device tensors)."""
    x = _as(images, device, single=3)
    B, H, W, _ = x.shape
    mask = torch.as_tensor(np.asarray(masks_u8), dtype=torch.float64).reshape(H, W, 1) / 255.0     # S1:580
    tl = torch.as_tensor(np.asarray(lights), dtype=torch.float32).reshape(B, 3, 1, 1).to(device)
    ta = torch.full((B, 1, 1), float(ambient), dtype=torch.float32, device=device)
    # (the camera matrix stays a HOST tensor: block.camera_scalars reads it without a device round trip; a fresh device tensor
    #  per call -- what the scripts pass, S1:588 -- would cost a device-to-host synchronisation per pass)
    if _is_transfer(model):
        return model(x, epoch, camera_matrix(700.0 if focal is None else focal, H, W), mask.to(device), tl, ta)
    return model(x, epoch, camera_matrix(1570.0 if focal is None else focal, H, W), mask.to(device), tl, ta, mask[None].to(device))


@torch.no_grad()
def relight_single_image(model, image, mask_u8, light, ambient: float = 0.5,
                         focal: float = None, device="cuda", fix_border: bool = False,
                         composite_mask_u8=None) -> np.ndarray:
    """S1:569-620 for one image: returns the composite (H,W,3) uint8 RGB (rendered face pasted into the input),
    composited and quantised on the device (gcfr_inference_images_u8); `fix_border=True` also applies
    fix_border_artifacts_CVPR2022.m there.  `composite_mask_u8`: see relight_images."""
    return relight_images(model, image, mask_u8, np.asarray(light, np.float32)[None], ambient, focal, device,
                          fix_border=fix_border, composite_mask_u8=composite_mask_u8)[0]


@torch.no_grad()
def relight_images(model, images, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                   device="cuda", fix_border: bool = False, composite_mask_u8=None) -> np.ndarray:
    """Batch form of S1:569-620 (+ the MATLAB border fix): (B,H,W,3) uint8 RGB composites.  Forward, compositing,
    quantisation and the border fix all run on the device; one device-to-host copy of B*H*W*3 bytes at the end.
    The script feeds the MODEL `curr_mask` (S1:586-588) and composites with the fill-nose-and-mouth mask
    (`curr_mask_fill_nose_3_channels`, S1:606-618); both are read from the same file in the shipped script (S1:564-567), so
    `composite_mask_u8` defaults to `mask_u8` -- pass the second mask when they differ."""
    x = _as(images, device, single=3)
    out = relight_batch(model, x, mask_u8, lights, ambient, focal, device)
    mask = _as(mask_u8 if composite_mask_u8 is None else composite_mask_u8, device, torch.uint8)
    imgs = pp.inference_images_device(x, out[5], mask, mask_f32=_is_transfer(model))["rendered_image"]
    if fix_border:
        imgs = pp.fix_border_artifacts_device(imgs, mask)
    return imgs.cpu().numpy()


@torch.no_grad()
def relight_lights_device(model, images, mask_u8, lights, ambient: float = 0.5, focal: float = None, device="cuda",
                          fix_border: bool = False, composite_mask_u8=None, epoch: int = 200) -> torch.Tensor:
    """`relight_lights` up to the bytes ON THE DEVICE: (B,L,H,W,3) uint8 tensor, nothing copied back.  `images` / `mask_u8` /
    `lights` may already be device tensors (then nothing is uploaded either): what bench.py's `relight_e2e` leg times."""
    x = _as(images, device, single=3)
    out, cm, transfer = _lights_pass(model, x, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch)
    return _light_composites(x, out, cm, transfer, fix_border)


@torch.no_grad()
def relight_lights(model, images, mask_u8, lights, ambient: float = 0.5, focal: float = None, device="cuda",
                   fix_border: bool = False, composite_mask_u8=None, epoch: int = 200) -> np.ndarray:
    """Every face of `images` (B,H,W,3) under every one of `lights` (L,3) -- e.g. the eleven directions the reference ships
    (LIGHT_DIRECTIONS, S1:519-562) -- as (B,L,H,W,3) uint8 RGB composites.  ONE network pass, one prepass and one normals
    stage per face, L marches, one image-kernel launch over all B*L composites: the scripts run the whole model once per
    (face, light) (S1:582-620).  `model`: a RelightNetSingleImage (the lighting head's ambient + the model's offset, S1:342;
    focal 1570) or a RelightNetLightingTransfer (`ambient` is the target ambient, SLT:545; focal 700).  Composite [b, l]
    equals relight_images(model, images[b:b+1], mask_u8, lights[l:l+1]) given the same network outputs.  One device-to-host
    copy of B*L*H*W*3 bytes at the end (`relight_lights_device` stops before it)."""
    return relight_lights_device(model, images, mask_u8, lights, ambient, focal, device, fix_border, composite_mask_u8, epoch).cpu().numpy()


def _light_composites(x, out, cm, transfer: bool, fix_border: bool) -> torch.Tensor:
    """`forward_lights`' tuple -> (B,L,H,W,3) uint8: the image kernel on its rendered images (out[5]), one launch over all B L
    composites, and the optional border fix on the (B L,H,W,3) view"""
    imgs = pp.inference_images_device(x, out[5], cm, mask_f32=transfer)["rendered_image"]
    if fix_border:
        B, L, H, W, _ = imgs.shape
        imgs = pp.fix_border_artifacts_device(imgs.reshape(B * L, H, W, 3), cm).reshape(B, L, H, W, 3)
    return imgs


def _rig_composites(x, out, cm, light_rgb, transfer: bool, fix_border: bool) -> torch.Tensor:
    """`forward_lights`' tuple -> (B,H,W,3) uint8: the rig stage on its albedo (out[0]) and final shading (out[8]), then the image
    kernel at one image per photograph and the optional border fix"""
    rendered, _ = combine_lights(out[8], out[0], light_rgb)
    imgs = pp.inference_images_device(x, rendered, cm, mask_f32=transfer)["rendered_image"]
    return pp.fix_border_artifacts_device(imgs, cm) if fix_border else imgs


@torch.no_grad()
def relight_rig_device(model, images, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None, device="cuda",
                       fix_border: bool = False, composite_mask_u8=None, epoch: int = 200) -> torch.Tensor:
    """`relight_rig` up to the bytes ON THE DEVICE: (B,H,W,3) uint8 tensor, nothing copied back.  `images` / `mask_u8` / `lights` /
    `light_rgb` may already be device tensors."""
    x = _as(images, device, single=3)
    out, cm, transfer = _lights_pass(model, x, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch)
    return _rig_composites(x, out, cm, _as(light_rgb, x.device, single=2).contiguous(), transfer, fix_border)


@torch.no_grad()
def relight_rig(model, images, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None, device="cuda",
                fix_border: bool = False, composite_mask_u8=None, epoch: int = 200) -> np.ndarray:
    """Every face of `images` (B,H,W,3) under the RIG of `lights` (L,3) | (B,L,3) with colour x weight `light_rgb` (L,3) | (1,L,3)
    | (B,L,3) per light -- an area light (`lighting.area_light`), a coloured key / fill / rim set -- as ONE (B,H,W,3) uint8 RGB
    composite per face.  One network pass (`forward_lights`), then `lighting.combine_lights` on its albedo and final shading
    (the weights apply to the whole per-light shading, ambient included: weights that sum to 1 count the ambient once), the image
    kernel and the optional border fix.  `model` / `ambient` / `focal` as in `relight_lights`; with one light of colour 1 the
    composite equals `relight_lights(...)[:, 0]`.  One device-to-host copy of B*H*W*3 bytes at the end."""
    return relight_rig_device(model, images, mask_u8, lights, light_rgb, ambient, focal, device, fix_border, composite_mask_u8,
                              epoch).cpu().numpy()


def _as_photographs(photos_u8, device) -> torch.Tensor:
    """uint8 photographs (B,H,W,3) | (H,W,3) as a device tensor (B,H,W,3); another dtype is refused, never rescaled"""
    t = photos_u8 if torch.is_tensor(photos_u8) else torch.as_tensor(np.asarray(photos_u8))
    if t.dtype != torch.uint8:
        raise GcfrError("photographs must be uint8 (0..255), got %s" % t.dtype)
    return _as(t, device, torch.uint8, single=3)


def _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch, ingest, composite, light_rgb=None, rig=False):
    """Every full-resolution and in-photograph entry, on the device: `ingest(photos)` -> the network's input x, ONE `forward_lights`
    pass on it, for a `rig` `lighting.combine_lights`' one image per face under `light_rgb`, then `composite(photos, x, rendered, cm)`"""
    photos = _as_photographs(photos_u8, device)
    x = ingest(photos)
    out, cm, _transfer = _lights_pass(model, x, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch)
    return composite(photos, x, combine_lights(out[8], out[0], _as(light_rgb, x.device, single=2).contiguous())[0] if rig else out[5], cm)


@torch.no_grad()
def relight_lights_fullres_device(model, photos_u8, mask_u8, lights, scale: int, ambient: float = 0.5, focal: float = None,
                                  device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                  floor: float = 1.0, upsample: str = "bilinear", range_sigma: float = 20.0) -> torch.Tensor:
    """`relight_lights_fullres` up to the bytes ON THE DEVICE: (B,L,H,W,3) uint8 tensor, nothing copied back.  `photos_u8` /
    `mask_u8` / `lights` may already be device tensors."""
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_photographs_device(ph, scale),
                                lambda *a: pp.fullres_composites_device(*a, scale, detail_clamp, floor, upsample=upsample, range_sigma=range_sigma))


@torch.no_grad()
def relight_lights_fullres(model, photos_u8, mask_u8, lights, scale: int, ambient: float = 0.5, focal: float = None, device="cuda",
                           composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0, floor: float = 1.0,
                           upsample: str = "bilinear", range_sigma: float = 20.0) -> np.ndarray:
    """`relight_lights` on photographs LARGER than the network: photos_u8 (B, s h, s w, 3) uint8 with `scale` s = 1, 2, 4 or 8 and
    (h, w) the network's resolution -> (B,L, s h, s w, 3) uint8 RGB, every face under every one of `lights` (L,3) at the
    photograph's own size.  Three steps on the device: `postprocess.ingest_photographs_device` (block mean / 255: the network's
    input, without a host-side resize), ONE `forward_lights` pass on it, then ONE `postprocess.fullres_composites_device` launch
    for all L lights (quotient / detail transfer: see there for `detail_clamp` and `floor`).  `mask_u8` (and `composite_mask_u8`,
    as in `relight_lights`) stay at the network's resolution (h,w); the upsampled compositing mask blends the relit face into the
    photograph, and outside it the photograph's bytes are returned untouched.  `upsample="guided"` carries the relit image, the
    quotient and the mask up with the edge-aware joint-bilateral upsample guided by the photograph (`range_sigma` in grey levels,
    an argument and not a tuned value: see `postprocess.fullres_composites_device`); the default "bilinear" is unchanged.
    `model` / `ambient` / `focal` as in `relight_lights`; there is no border fix at full resolution.  One device-to-host copy of B*L*H*W*3 bytes at the end."""
    return relight_lights_fullres_device(model, photos_u8, mask_u8, lights, scale, ambient, focal, device, composite_mask_u8, epoch,
                                         detail_clamp, floor, upsample, range_sigma).cpu().numpy()


@torch.no_grad()
def relight_rig_fullres_device(model, photos_u8, mask_u8, lights, light_rgb, scale: int, ambient: float = 0.5, focal: float = None,
                               device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                               floor: float = 1.0, upsample: str = "bilinear", range_sigma: float = 20.0) -> torch.Tensor:
    """`relight_rig_fullres` up to the bytes ON THE DEVICE: (B,H,W,3) uint8 tensor, nothing copied back."""
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_photographs_device(ph, scale),
                                lambda *a: pp.fullres_composites_device(*a, scale, detail_clamp, floor, upsample=upsample, range_sigma=range_sigma),
                                light_rgb, rig=True)


@torch.no_grad()
def relight_rig_fullres(model, photos_u8, mask_u8, lights, light_rgb, scale: int, ambient: float = 0.5, focal: float = None,
                        device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                        floor: float = 1.0, upsample: str = "bilinear", range_sigma: float = 20.0) -> np.ndarray:
    """`relight_rig` on photographs larger than the network: ONE (B, s h, s w, 3) uint8 RGB composite per face under the rig of
    `lights` with colour x weight `light_rgb` (as in `relight_rig`).  `relight_lights_fullres`' three steps with
    `lighting.combine_lights`' `rendered` between the pass and the full-resolution launch (L = 1 there); with one light of colour 1
    the composite equals `relight_lights_fullres(...)[:, 0]`.  One device-to-host copy of B*H*W*3 bytes at the end."""
    return relight_rig_fullres_device(model, photos_u8, mask_u8, lights, light_rgb, scale, ambient, focal, device, composite_mask_u8,
                                      epoch, detail_clamp, floor, upsample, range_sigma).cpu().numpy()


def _network_size(mask_u8):
    """(h, w) of the network from the mask that goes with it: (h,w) or (1,h,w) uint8"""
    shape = tuple(mask_u8.shape) if torch.is_tensor(mask_u8) else np.asarray(mask_u8).shape
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[0] != 1) or min(shape) < 1:
        raise GcfrError("mask_u8 must be (h,w) or (1,h,w) at the network's resolution; got %s" % (shape,))
    return int(shape[-2]), int(shape[-1])


def _check_host_boxes(boxes):
    if torch.is_tensor(boxes) and boxes.is_cuda:
        raise GcfrError("boxes are HOST integers (x0, y0, bw, bh); got a tensor on %s" % boxes.device)


@torch.no_grad()
def relight_lights_in_photograph_device(model, photos_u8, boxes, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                                        device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                        floor: float = 1.0, paste: bool = True) -> torch.Tensor:
    """`relight_lights_in_photograph` up to the bytes ON THE DEVICE: (B,L,Hp,Wp,3) uint8 tensor (`paste=False`: (B,L,bh,bw,3)),
    nothing copied back.  `photos_u8` / `mask_u8` / `lights` may already be device tensors; `boxes` stay on the host."""
    _check_host_boxes(boxes)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_box_device(ph, boxes, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_box_composites_device(ph, boxes, *a, detail_clamp, floor, paste=paste))


@torch.no_grad()
def relight_lights_in_photograph(model, photos_u8, boxes, mask_u8, lights, ambient: float = 0.5, focal: float = None, device="cuda",
                                 composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0, floor: float = 1.0,
                                 paste: bool = True) -> np.ndarray:
    """`relight_lights` on a FACE BOX inside a larger photograph: photos_u8 (B,Hp,Wp,3) uint8 of any size, `boxes` host integers
    (x0, y0, bw, bh) in photograph pixels -- (4,) for every face or (B,4), whatever a detector reports, never smaller than the
    network's input -> (B,L,Hp,Wp,3) uint8 RGB: every photograph under every one of `lights` (L,3), relit inside its box and
    untouched outside it (`paste=False`: the boxes alone, (B,L,bh,bw,3), all of one size).  Three steps on the device:
    `postprocess.ingest_box_device` (the exact area mean of the box: the network's input, without a host-side crop and resize),
    ONE `forward_lights` pass on it, then ONE `postprocess.fullres_box_composites_device` launch for all L lights.  The network's
    size (h, w) is `mask_u8`'s; `mask_u8` and `composite_mask_u8` are in the box's frame.  `model` / `ambient` / `focal` as in
    `relight_lights`; `detail_clamp` / `floor` as in `relight_lights_fullres`, whose bytes these are when the box is the whole
    photograph at 1, 2, 4 or 8 times the network's side.  The edge-aware upsample over a box is
    `relight_lights_in_photograph_guided`.  One device-to-host copy of the result at the end."""
    return relight_lights_in_photograph_device(model, photos_u8, boxes, mask_u8, lights, ambient, focal, device, composite_mask_u8,
                                               epoch, detail_clamp, floor, paste).cpu().numpy()


@torch.no_grad()
def relight_rig_in_photograph_device(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None,
                                     device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                     floor: float = 1.0, paste: bool = True) -> torch.Tensor:
    """`relight_rig_in_photograph` up to the bytes ON THE DEVICE: (B,Hp,Wp,3) uint8 tensor (`paste=False`: (B,bh,bw,3)), nothing
    copied back."""
    _check_host_boxes(boxes)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_box_device(ph, boxes, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_box_composites_device(ph, boxes, *a, detail_clamp, floor, paste=paste),
                                light_rgb, rig=True)


@torch.no_grad()
def relight_rig_in_photograph(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None,
                              device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0, floor: float = 1.0,
                              paste: bool = True) -> np.ndarray:
    """`relight_rig` on a face box inside a larger photograph: ONE (B,Hp,Wp,3) uint8 RGB composite per photograph under the rig of
    `lights` with colour x weight `light_rgb` (as in `relight_rig`), relit inside its box.  `relight_lights_in_photograph`'s
    three steps with `lighting.combine_lights`' `rendered` between the pass and the box launch (L = 1 there); with one light of
    colour 1 the composite equals `relight_lights_in_photograph(...)[:, 0]`.  One device-to-host copy at the end."""
    return relight_rig_in_photograph_device(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient, focal, device,
                                            composite_mask_u8, epoch, detail_clamp, floor, paste).cpu().numpy()


@torch.no_grad()
def relight_lights_in_photograph_guided_device(model, photos_u8, boxes, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                                               device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                               floor: float = 1.0, paste: bool = True, range_sigma: float = 20.0) -> torch.Tensor:
    """`relight_lights_in_photograph_guided` up to the bytes ON THE DEVICE: (B,L,Hp,Wp,3) uint8 tensor (`paste=False`:
    (B,L,bh,bw,3)), nothing copied back."""
    _check_host_boxes(boxes)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_box_device(ph, boxes, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_box_composites_device(ph, boxes, *a, detail_clamp, floor, paste=paste,
                                                                                upsample="guided", range_sigma=range_sigma))


@torch.no_grad()
def relight_lights_in_photograph_guided(model, photos_u8, boxes, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                                        device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                        floor: float = 1.0, paste: bool = True, range_sigma: float = 20.0) -> np.ndarray:
    """`relight_lights_in_photograph` with the EDGE-AWARE upsample over the box: the relit image, the quotient and the mask are
    carried up by the joint-bilateral upsample guided by the photograph (`postprocess.fullres_box_composites_device(
    upsample="guided")`; `range_sigma` in grey levels, an argument and not a tuned value), so that neither the relighting gain nor
    the mask crosses an edge the network's resolution does not see.  Everything else is `relight_lights_in_photograph`'s; with the
    box the whole photograph at 1, 2, 4 or 8 times the network's side these are `relight_lights_fullres(upsample="guided")`'s
    bytes.  One device-to-host copy of the result at the end."""
    return relight_lights_in_photograph_guided_device(model, photos_u8, boxes, mask_u8, lights, ambient, focal, device, composite_mask_u8,
                                                      epoch, detail_clamp, floor, paste, range_sigma).cpu().numpy()


@torch.no_grad()
def relight_rig_in_photograph_guided_device(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None,
                                            device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                            floor: float = 1.0, paste: bool = True, range_sigma: float = 20.0) -> torch.Tensor:
    """`relight_rig_in_photograph_guided` up to the bytes ON THE DEVICE: (B,Hp,Wp,3) uint8 tensor (`paste=False`: (B,bh,bw,3)),
    nothing copied back."""
    _check_host_boxes(boxes)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_box_device(ph, boxes, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_box_composites_device(ph, boxes, *a, detail_clamp, floor, paste=paste,
                                                                                upsample="guided", range_sigma=range_sigma),
                                light_rgb, rig=True)


@torch.no_grad()
def relight_rig_in_photograph_guided(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None,
                                     device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                     floor: float = 1.0, paste: bool = True, range_sigma: float = 20.0) -> np.ndarray:
    """`relight_rig_in_photograph` with the edge-aware upsample over the box (`relight_lights_in_photograph_guided`): ONE
    (B,Hp,Wp,3) uint8 RGB composite per photograph under the rig; with one light of colour 1 it equals
    `relight_lights_in_photograph_guided(...)[:, 0]`.  One device-to-host copy at the end."""
    return relight_rig_in_photograph_guided_device(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient, focal, device,
                                                   composite_mask_u8, epoch, detail_clamp, floor, paste, range_sigma).cpu().numpy()


@torch.no_grad()
def relight_lights_in_photograph_anybox_device(model, photos_u8, boxes, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                                               device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                               floor: float = 1.0, paste: bool = True) -> torch.Tensor:
    """`relight_lights_in_photograph_anybox` up to the bytes ON THE DEVICE: (B,L,Hp,Wp,3) uint8 tensor (`paste=False`:
    (B,L,bh,bw,3)), nothing copied back."""
    _check_host_boxes(boxes)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_anybox_device(ph, boxes, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_anybox_composites_device(ph, boxes, *a, detail_clamp, floor, paste=paste))


@torch.no_grad()
def relight_lights_in_photograph_anybox(model, photos_u8, boxes, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                                        device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                        floor: float = 1.0, paste: bool = True) -> np.ndarray:
    """`relight_lights_in_photograph` for face boxes of ANY size: a box may be smaller than the network's input on either axis, down
    to an eighth of it (bw, bh >= 1, 8 bw >= w, 8 bh >= h) -- the face in a group photograph or a webcam frame.  The same three
    steps with `postprocess.ingest_anybox_device` (a short axis is magnified bilinearly, in integers) and ONE
    `postprocess.fullres_anybox_composites_device` launch per 32 faces (a short axis receives the exact area mean of the network
    pixels a box pixel covers); large, small and mixed boxes may share a call.  Everything else, `paste` included, is
    `relight_lights_in_photograph`'s, and so are the bytes when no box is smaller than the network's input.  One device-to-host
    copy of the result at the end."""
    return relight_lights_in_photograph_anybox_device(model, photos_u8, boxes, mask_u8, lights, ambient, focal, device, composite_mask_u8,
                                                      epoch, detail_clamp, floor, paste).cpu().numpy()


@torch.no_grad()
def relight_rig_in_photograph_anybox_device(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None,
                                            device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                            floor: float = 1.0, paste: bool = True) -> torch.Tensor:
    """`relight_rig_in_photograph_anybox` up to the bytes ON THE DEVICE: (B,Hp,Wp,3) uint8 tensor (`paste=False`: (B,bh,bw,3)),
    nothing copied back."""
    _check_host_boxes(boxes)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_anybox_device(ph, boxes, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_anybox_composites_device(ph, boxes, *a, detail_clamp, floor, paste=paste),
                                light_rgb, rig=True)


@torch.no_grad()
def relight_rig_in_photograph_anybox(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient: float = 0.5, focal: float = None,
                                     device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                     floor: float = 1.0, paste: bool = True) -> np.ndarray:
    """`relight_rig_in_photograph` for face boxes of any size (`relight_lights_in_photograph_anybox`): ONE (B,Hp,Wp,3) uint8 RGB
    composite per photograph under the rig; with one light of colour 1 it equals `relight_lights_in_photograph_anybox(...)[:, 0]`.
    One device-to-host copy at the end."""
    return relight_rig_in_photograph_anybox_device(model, photos_u8, boxes, mask_u8, lights, light_rgb, ambient, focal, device,
                                                   composite_mask_u8, epoch, detail_clamp, floor, paste).cpu().numpy()


LIGHT_FRAMES = ("face", "photograph")


def lights_in_face_frame(lights, photo_to_net, faces: int):
    """Light directions given in the PHOTOGRAPH'S frame (+x right, +y up, as everywhere) turned into each face's own frame by the
    rotation part of that face's map photograph -> network: `lights` (L,3) | (B,L,3) (an array or a tensor, on any device) and
    `photo_to_net` (2,3) | (B,2,3) host numbers (the I of `postprocess.quantise_affine`, integers or not: only ratios are read) ->
    (B,L,3) f32 where `lights` live.  The angle of face b is phi = atan2(I10 - I01, I00 + I11); in the lights' frame, whose y axis
    points up while the image's points down, x' = cos(phi) x + sin(phi) y and y' = -sin(phi) x + cos(phi) y; z is untouched."""
    I = np.asarray(photo_to_net.detach().numpy() if torch.is_tensor(photo_to_net) else photo_to_net, dtype=np.float64)
    if I.shape not in ((2, 3), (faces, 2, 3)):
        raise GcfrError("photo_to_net must be (2,3) or (%d,2,3); got %s" % (faces, I.shape))
    I = np.broadcast_to(I, (faces, 2, 3))
    up, along = I[:, 1, 0] - I[:, 0, 1], I[:, 0, 0] + I[:, 1, 1]                   # (sin phi, cos phi) times twice the scale
    length = np.hypot(up, along)
    if not np.isfinite(length).all() or (length == 0).any():
        raise GcfrError("photo_to_net has no rotation part to read an angle from (a mirror image, or not finite)")
    t = _as(lights, None, torch.float64, single=1)
    if t.dim() not in (2, 3) or t.shape[-1] != 3 or (t.dim() == 3 and t.shape[0] != faces):
        raise GcfrError("lights must be (L,3) or (%d,L,3); got %s" % (faces, tuple(t.shape)))
    t = t[None].expand(faces, -1, -1) if t.dim() == 2 else t
    # cos phi and sin phi as quotients (exact at whole quarter turns); the two products and the sum in f64, rounded once to f32
    co, si = (torch.from_numpy(v / length).to(t.device)[:, None] for v in (along, up))
    x, y = t[..., 0], t[..., 1]
    return torch.stack([co * x + si * y, co * y - si * x, t[..., 2]], -1).to(torch.float32).contiguous()


def _affine_entry(photos_u8, net_to_photo, lights, light_frame, device):
    """what the four affine entries do before the pass: the photographs on the device, the host map as `quantise_affine`'s integer
    pair (so that the ingest, the composite and the lights read the same integers), and the lights in the faces' frame"""
    if light_frame not in LIGHT_FRAMES:
        raise GcfrError("light_frame must be one of %s; got %r" % (LIGHT_FRAMES, light_frame))
    photos = _as_photographs(photos_u8, device)
    pair = pp._affine_integers(net_to_photo, int(photos.shape[0]), "relight_in_photograph_affine")
    if light_frame == "photograph":
        lights = lights_in_face_frame(lights, pair[1], int(photos.shape[0]))
    return photos, pair, lights


@torch.no_grad()
def relight_lights_in_photograph_affine_device(model, photos_u8, net_to_photo, mask_u8, lights, ambient: float = 0.5,
                                               focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                               detail_clamp: float = 4.0, floor: float = 1.0, light_frame: str = "face") -> torch.Tensor:
    """`relight_lights_in_photograph_affine` up to the bytes ON THE DEVICE: (B,L,Hp,Wp,3) uint8 tensor, nothing copied back.
    `photos_u8` / `mask_u8` / `lights` may already be device tensors; `net_to_photo` stays on the host."""
    photos, pair, lights = _affine_entry(photos_u8, net_to_photo, lights, light_frame, device)
    return _relight_photographs(model, photos, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_affine_device(ph, pair, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_affine_composites_device(ph, pair, *a, detail_clamp, floor))


@torch.no_grad()
def relight_lights_in_photograph_affine(model, photos_u8, net_to_photo, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                                        device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                        floor: float = 1.0, light_frame: str = "face") -> np.ndarray:
    """`relight_lights_in_photograph` for a ROTATED face: `net_to_photo` is the host 2 x 3 map from the network's coordinates to the
    photograph's -- (2,3) for every face or (B,2,3) f64, what a face aligner reports (eye line horizontal, fixed inter-ocular
    distance) or `postprocess.affine_from_rotated_box` builds; or `postprocess.quantise_affine`'s integer pair -> (B,L,Hp,Wp,3)
    uint8 RGB: every photograph under every one of `lights`, relit inside the tilted quad of its face and untouched outside it.
    The same three steps with `postprocess.ingest_affine_device` (the network sees an ALIGNED face, without a host-side warp) and
    ONE `postprocess.fullres_affine_composites_device` launch per 32 faces.  `mask_u8` / `composite_mask_u8` are in the network's
    frame.  `light_frame`: "face" (the default) takes `lights` (L,3) | (B,L,3) in the network's frame, as everywhere else;
    "photograph" takes them in the photograph's frame (+x right, +y up) and turns each face's copy into that face's frame by the
    rotation part of its map (`lights_in_face_frame`; (L,3) becomes (B,L,3)), so that "light from the photograph's left" comes from
    the photograph's left on a tilted face too.  There is always a pasted photograph: a rotated quad has no "box alone".  Everything
    else is `relight_lights_in_photograph`'s.  One device-to-host copy of the result at the end."""
    return relight_lights_in_photograph_affine_device(model, photos_u8, net_to_photo, mask_u8, lights, ambient, focal, device,
                                                      composite_mask_u8, epoch, detail_clamp, floor, light_frame).cpu().numpy()


@torch.no_grad()
def relight_rig_in_photograph_affine_device(model, photos_u8, net_to_photo, mask_u8, lights, light_rgb, ambient: float = 0.5,
                                            focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                            detail_clamp: float = 4.0, floor: float = 1.0, light_frame: str = "face") -> torch.Tensor:
    """`relight_rig_in_photograph_affine` up to the bytes ON THE DEVICE: (B,Hp,Wp,3) uint8 tensor, nothing copied back."""
    photos, pair, lights = _affine_entry(photos_u8, net_to_photo, lights, light_frame, device)
    return _relight_photographs(model, photos, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_affine_device(ph, pair, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_affine_composites_device(ph, pair, *a, detail_clamp, floor),
                                light_rgb, rig=True)


@torch.no_grad()
def relight_rig_in_photograph_affine(model, photos_u8, net_to_photo, mask_u8, lights, light_rgb, ambient: float = 0.5,
                                     focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                     detail_clamp: float = 4.0, floor: float = 1.0, light_frame: str = "face") -> np.ndarray:
    """`relight_rig_in_photograph` for a rotated face (`relight_lights_in_photograph_affine`, `light_frame` included): ONE
    (B,Hp,Wp,3) uint8 RGB composite per photograph under the rig; with one light of colour 1 it equals
    `relight_lights_in_photograph_affine(...)[:, 0]`.  One device-to-host copy at the end."""
    return relight_rig_in_photograph_affine_device(model, photos_u8, net_to_photo, mask_u8, lights, light_rgb, ambient, focal, device,
                                                   composite_mask_u8, epoch, detail_clamp, floor, light_frame).cpu().numpy()


def _check_host_photo_index(photo_index):
    if torch.is_tensor(photo_index) and photo_index.is_cuda:
        raise GcfrError("photo_index are HOST integers, one photograph per face; got a tensor on %s" % photo_index.device)


@torch.no_grad()
def relight_lights_in_group_photograph_device(model, photos_u8, boxes, photo_index, mask_u8, lights, ambient: float = 0.5,
                                              focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                              detail_clamp: float = 4.0, floor: float = 1.0) -> torch.Tensor:
    """`relight_lights_in_group_photograph` up to the bytes ON THE DEVICE: (P,L,Hp,Wp,3) uint8 tensor, nothing copied back.
    `photos_u8` / `mask_u8` / `lights` may already be device tensors; `boxes` and `photo_index` stay on the host."""
    _check_host_boxes(boxes)
    _check_host_photo_index(photo_index)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_group_device(ph, boxes, photo_index, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_group_composites_device(ph, boxes, photo_index, *a, detail_clamp, floor))


@torch.no_grad()
def relight_lights_in_group_photograph(model, photos_u8, boxes, photo_index, mask_u8, lights, ambient: float = 0.5, focal: float = None,
                                       device="cuda", composite_mask_u8=None, epoch: int = 200, detail_clamp: float = 4.0,
                                       floor: float = 1.0) -> np.ndarray:
    """EVERY face of a GROUP PHOTOGRAPH relit: photos_u8 (P,Hp,Wp,3) uint8 (or one (Hp,Wp,3)), B faces with host `boxes` (B,4) of
    any size (`relight_lights_in_photograph_anybox`'s rules) and host `photo_index` (B,) naming each face's photograph (any order; a
    photograph may have no face, one or many; None: all faces in the one photograph) -> (P,L,Hp,Wp,3) uint8 RGB: every photograph
    under every one of `lights` (L,3) with ALL of its faces relit.  Three steps on the device:
    `postprocess.ingest_group_device` (the photographs are not copied per face), ONE `forward_lights` pass on all B faces, then
    `postprocess.fullres_group_composites_device`: one pass over each photograph's bytes, per photograph the chain of
    `relight_lights_in_photograph_anybox`'s composite over its faces in ascending face index (see there for overlapping faces).
    `mask_u8` / `composite_mask_u8` are in the boxes' frame and shared by the faces.  Everything else is
    `relight_lights_in_photograph_anybox`'s; there is no `paste=False`.  One device-to-host copy of the result at the end."""
    return relight_lights_in_group_photograph_device(model, photos_u8, boxes, photo_index, mask_u8, lights, ambient, focal, device,
                                                     composite_mask_u8, epoch, detail_clamp, floor).cpu().numpy()


@torch.no_grad()
def relight_rig_in_group_photograph_device(model, photos_u8, boxes, photo_index, mask_u8, lights, light_rgb, ambient: float = 0.5,
                                           focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                           detail_clamp: float = 4.0, floor: float = 1.0) -> torch.Tensor:
    """`relight_rig_in_group_photograph` up to the bytes ON THE DEVICE: (P,Hp,Wp,3) uint8 tensor, nothing copied back."""
    _check_host_boxes(boxes)
    _check_host_photo_index(photo_index)
    return _relight_photographs(model, photos_u8, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_group_device(ph, boxes, photo_index, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_group_composites_device(ph, boxes, photo_index, *a, detail_clamp, floor),
                                light_rgb, rig=True)


@torch.no_grad()
def relight_rig_in_group_photograph(model, photos_u8, boxes, photo_index, mask_u8, lights, light_rgb, ambient: float = 0.5,
                                    focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                    detail_clamp: float = 4.0, floor: float = 1.0) -> np.ndarray:
    """`relight_rig` on every face of a group photograph (`relight_lights_in_group_photograph`): ONE (P,Hp,Wp,3) uint8 RGB composite
    per photograph under the rig of `lights` with colour x weight `light_rgb`, all of its faces relit; with one light of colour 1 it
    equals `relight_lights_in_group_photograph(...)[:, 0]`.  One device-to-host copy at the end."""
    return relight_rig_in_group_photograph_device(model, photos_u8, boxes, photo_index, mask_u8, lights, light_rgb, ambient, focal, device,
                                                  composite_mask_u8, epoch, detail_clamp, floor).cpu().numpy()


def _group_affine_entry(photos_u8, net_to_photo, photo_index, lights, light_frame, device):
    """what the four group-affine entries do before the pass: the photographs on the device, the host indices checked, the host map
    as `quantise_affine`'s integer pair, quantised ONCE for the ingest, the composite and the lights, and the lights in the faces'
    frame"""
    if light_frame not in LIGHT_FRAMES:
        raise GcfrError("light_frame must be one of %s; got %r" % (LIGHT_FRAMES, light_frame))
    _check_host_photo_index(photo_index)
    photos = _as_photographs(photos_u8, device)
    what = "relight_in_group_photograph_affine"
    pi = pp._check_photo_index(photo_index, photos, what, faces=pp._faces_of_map(net_to_photo) if photo_index is None else None)
    pair = pp._affine_integers(net_to_photo, int(pi.shape[0]), what)
    if light_frame == "photograph":
        lights = lights_in_face_frame(lights, pair[1], int(pi.shape[0]))
    return photos, pair, pi, lights


@torch.no_grad()
def relight_lights_in_group_photograph_affine_device(model, photos_u8, net_to_photo, photo_index, mask_u8, lights, ambient: float = 0.5,
                                                     focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                                     detail_clamp: float = 4.0, floor: float = 1.0,
                                                     light_frame: str = "face") -> torch.Tensor:
    """`relight_lights_in_group_photograph_affine` up to the bytes ON THE DEVICE: (P,L,Hp,Wp,3) uint8 tensor, nothing copied back.
    `photos_u8` / `mask_u8` / `lights` may already be device tensors; `net_to_photo` and `photo_index` stay on the host."""
    photos, pair, pi, lights = _group_affine_entry(photos_u8, net_to_photo, photo_index, lights, light_frame, device)
    return _relight_photographs(model, photos, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_group_affine_device(ph, pair, pi, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_group_affine_composites_device(ph, pair, pi, *a, detail_clamp, floor))


@torch.no_grad()
def relight_lights_in_group_photograph_affine(model, photos_u8, net_to_photo, photo_index, mask_u8, lights, ambient: float = 0.5,
                                              focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                              detail_clamp: float = 4.0, floor: float = 1.0, light_frame: str = "face") -> np.ndarray:
    """EVERY TILTED face of a GROUP PHOTOGRAPH relit: photos_u8 (P,Hp,Wp,3) uint8 (or one (Hp,Wp,3)), B faces with the host map
    `net_to_photo` (B,2,3) f64 -- what a face aligner reports per head; (2,3) for every face; or `postprocess.quantise_affine`'s
    integer pair (`relight_lights_in_photograph_affine`'s rules) -- and host `photo_index` (B,) naming each face's photograph (any
    order; a photograph may have no face, one or many; None: all faces in the one photograph) -> (P,L,Hp,Wp,3) uint8 RGB: every
    photograph under every one of `lights` with ALL of its faces relit inside their tilted quads.  Three steps on the device:
    `postprocess.ingest_group_affine_device` (the photographs are not copied per face), ONE `forward_lights` pass on all B faces,
    then `postprocess.fullres_group_affine_composites_device`: one pass over each photograph's bytes, per photograph the chain of
    `relight_lights_in_photograph_affine`'s composite over its faces in ascending face index (see
    `relight_lights_in_group_photograph` for overlapping faces).  The matrix is quantised once per call.  `mask_u8` /
    `composite_mask_u8` are in the network's frame and shared by the faces.  `light_frame` as in
    `relight_lights_in_photograph_affine`: "photograph" turns each FACE's copy of the lights by its own map, which is what makes
    "light from the photograph's left" mean the same thing on every head of the group.  One device-to-host copy of the result at the
    end."""
    return relight_lights_in_group_photograph_affine_device(model, photos_u8, net_to_photo, photo_index, mask_u8, lights, ambient, focal,
                                                            device, composite_mask_u8, epoch, detail_clamp, floor,
                                                            light_frame).cpu().numpy()


@torch.no_grad()
def relight_rig_in_group_photograph_affine_device(model, photos_u8, net_to_photo, photo_index, mask_u8, lights, light_rgb,
                                                  ambient: float = 0.5, focal: float = None, device="cuda", composite_mask_u8=None,
                                                  epoch: int = 200, detail_clamp: float = 4.0, floor: float = 1.0,
                                                  light_frame: str = "face") -> torch.Tensor:
    """`relight_rig_in_group_photograph_affine` up to the bytes ON THE DEVICE: (P,Hp,Wp,3) uint8 tensor, nothing copied back."""
    photos, pair, pi, lights = _group_affine_entry(photos_u8, net_to_photo, photo_index, lights, light_frame, device)
    return _relight_photographs(model, photos, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch,
                                lambda ph: pp.ingest_group_affine_device(ph, pair, pi, _network_size(mask_u8)),
                                lambda ph, *a: pp.fullres_group_affine_composites_device(ph, pair, pi, *a, detail_clamp, floor),
                                light_rgb, rig=True)


@torch.no_grad()
def relight_rig_in_group_photograph_affine(model, photos_u8, net_to_photo, photo_index, mask_u8, lights, light_rgb, ambient: float = 0.5,
                                           focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200,
                                           detail_clamp: float = 4.0, floor: float = 1.0, light_frame: str = "face") -> np.ndarray:
    """`relight_rig` on every tilted face of a group photograph (`relight_lights_in_group_photograph_affine`, `light_frame`
    included): ONE (P,Hp,Wp,3) uint8 RGB composite per photograph under the rig of `lights` with colour x weight `light_rgb`, all of
    its faces relit; with one light of colour 1 it equals `relight_lights_in_group_photograph_affine(...)[:, 0]`.  One device-to-host
    copy at the end."""
    return relight_rig_in_group_photograph_affine_device(model, photos_u8, net_to_photo, photo_index, mask_u8, lights, light_rgb, ambient,
                                                         focal, device, composite_mask_u8, epoch, detail_clamp, floor,
                                                         light_frame).cpu().numpy()


def _rig_frames(x, out, cm, light_rgb_frames, transfer: bool, fix_border: bool) -> torch.Tensor:
    """`forward_lights`' tuple -> (B,F,H,W,3) uint8: ONE rig-frames launch on its albedo (out[0]) and final shading (out[8]), and
    the optional border fix on the (B F,H,W,3) view"""
    frames = rig_frames_u8(out[8], out[0], x, cm, light_rgb_frames, mask_f32=transfer)
    if fix_border:
        B, F, H, W, _ = frames.shape
        frames = pp.fix_border_artifacts_device(frames.reshape(B * F, H, W, 3), cm).reshape(B, F, H, W, 3)
    return frames


@torch.no_grad()
def relight_rig_frames_device(model, images, mask_u8, lights, light_rgb_frames, ambient: float = 0.5, focal: float = None,
                              device="cuda", fix_border: bool = False, composite_mask_u8=None, epoch: int = 200) -> torch.Tensor:
    """`relight_rig_frames` up to the bytes ON THE DEVICE: (B,F,H,W,3) uint8 tensor, nothing copied back.  `images` / `mask_u8` /
    `lights` / `light_rgb_frames` may already be device tensors."""
    x = _as(images, device, single=3)
    out, cm, transfer = _lights_pass(model, x, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch)
    return _rig_frames(x, out, cm, _as(light_rgb_frames, x.device, single=3).contiguous(), transfer, fix_border)


@torch.no_grad()
def relight_rig_frames(model, images, mask_u8, lights, light_rgb_frames, ambient: float = 0.5, focal: float = None, device="cuda",
                       fix_border: bool = False, composite_mask_u8=None, epoch: int = 200) -> np.ndarray:
    """An ANIMATED rig: every face of `images` (B,H,W,3) under each of the F rigs `light_rgb_frames` (F,L,3) | (1,F,L,3) | (B,F,L,3)
    of the fixed `lights` (L,3) | (B,L,3) -- a key fading into a fill, a colour sweep, a captured rig cross-faded into another -- as
    (B,F,H,W,3) uint8 RGB composites.  ONE network pass (`forward_lights`) and L marches in total, then ONE launch
    (`lighting.rig_frames_u8`) for all F frames, and one more with `fix_border`.  Frame f equals
    `relight_rig(model, images, mask_u8, lights, light_rgb_frames[:, f], ...)` byte for byte, given the same network outputs.
    `model` / `ambient` / `focal` as in `relight_lights`.  One device-to-host copy of B*F*H*W*3 bytes at the end."""
    return relight_rig_frames_device(model, images, mask_u8, lights, light_rgb_frames, ambient, focal, device, fix_border,
                                     composite_mask_u8, epoch).cpu().numpy()


def _environment_directions(n_lights, min_z, device) -> torch.Tensor:
    return torch.from_numpy(sphere_directions(n_lights, min_z)).to(device)


def _lights_pass(model, x, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch):
    """ONE `forward_lights` pass of `x` (B,H,W,3, on the device) under `lights` (L,3) | (B,L,3): the pass of every `relight_*` /
    `capture_rig` entry (the environment and rig-capture entries are held byte for byte to `relight_rig_device`).  Returns three values:
    `out`, the tuple `model.forward_lights` returned; `cm`, the compositing mask as a uint8 device tensor (`composite_mask_u8`, or
    `mask_u8` where that is None); `transfer`, True if `model` is a RelightNetLightingTransfer."""
    B, H, W, _ = x.shape
    transfer = _is_transfer(model)
    K = camera_matrix(_default_focal(transfer, focal), H, W)                                                     # host: read without a sync
    m_u8 = _as(mask_u8, device, torch.uint8)
    mask = (m_u8.to(torch.float64).reshape(H, W, 1) / 255.0)                                                     # S1:580 / SLT:540
    out = _forward_lights(model, x, epoch, K, mask, _as(lights, device, single=1), float(ambient))
    return out, (m_u8 if composite_mask_u8 is None else _as(composite_mask_u8, device, torch.uint8)), transfer


def _forward_lights(model, x, epoch, K, mask, lights, ambient, hoist=None):
    """`model.forward_lights` on operands that are already built (`_lights_pass` builds them per call, `RelightSession` once);
    `ambient` reaches a RelightNetLightingTransfer only -- a RelightNetSingleImage reads its own (S1:342)"""
    if _is_transfer(model):
        return model.forward_lights(x, epoch, K, mask, lights, ambient, hoist=hoist)
    return model.forward_lights(x, epoch, K, mask, lights, hoist=hoist)


@torch.no_grad()
def relight_environment_device(model, images, mask_u8, env, n_lights: int = 64, rotation=None, min_cos: float = -2.0,
                               min_z: float = 0.2, ambient: float = 0.5, focal: float = None, device="cuda",
                               fix_border: bool = False, composite_mask_u8=None, epoch: int = 200) -> torch.Tensor:
    """`relight_environment` up to the bytes ON THE DEVICE: (B,H,W,3) uint8 tensor, nothing copied back.  `images` / `mask_u8` /
    `env` / `rotation` may already be device tensors."""
    x = _as(images, device, single=3)
    directions = _environment_directions(n_lights, min_z, x.device)
    env_d = _as(env, x.device, single=3).contiguous()
    rot = None if rotation is None else torch.as_tensor(rotation, dtype=torch.float32)
    _check_environment(env_d, directions, rot, None, faces=x.shape[0])                # a malformed map fails before the network pass
    out, cm, transfer = _lights_pass(model, x, mask_u8, directions, ambient, focal, device, composite_mask_u8, epoch)
    return _rig_composites(x, out, cm, environment_lights(env_d, directions, rot, min_cos), transfer, fix_border)


@torch.no_grad()
def relight_environment(model, images, mask_u8, env, n_lights: int = 64, rotation=None, min_cos: float = -2.0,
                        min_z: float = 0.2, ambient: float = 0.5, focal: float = None, device="cuda", fix_border: bool = False,
                        composite_mask_u8=None, epoch: int = 200) -> np.ndarray:
    """Every face of `images` (B,H,W,3) under the lat-long radiance map `env` (He,We,3) | (1,He,We,3) | (B,He,We,3) as ONE
    (B,H,W,3) uint8 RGB composite per face.  The map is integrated into a rig of `n_lights` fixed directions
    (`lighting.sphere_directions(n_lights, min_z)`, the part of the sphere in front of the face) by `lighting.environment_lights`:
    one network pass (`forward_lights`) over those directions, the stage, then `relight_rig`'s combine, image kernel and optional
    border fix.  `rotation` (3,3) turns the environment around the face (`environment_lights` states its sense), `min_cos` as
    there.  The map's frame and layout: `lighting.environment_tables`.  The weights of the whole sphere sum to 1, so a constant
    map of radiance 1 counts the ambient term once.  `model` / `ambient` / `focal` as in `relight_lights`.  One device-to-host
    copy of B*H*W*3 bytes at the end."""
    return relight_environment_device(model, images, mask_u8, env, n_lights, rotation, min_cos, min_z, ambient, focal, device,
                                      fix_border, composite_mask_u8, epoch).cpu().numpy()


@torch.no_grad()
def relight_environment_frames(model, images, mask_u8, env, rotations, n_lights: int = 64, min_cos: float = -2.0,
                               min_z: float = 0.2, ambient: float = 0.5, focal: float = None, device="cuda",
                               fix_border: bool = False, composite_mask_u8=None, epoch: int = 200, fused: bool = False) -> torch.Tensor:
    """A turntable: every face of `images` under `env` rotated by each of `rotations` (F,3,3), as a (B,F,H,W,3) uint8 DEVICE
    tensor; frame f equals `relight_environment_device(..., rotation=rotations[f])` byte for byte, given the same network outputs.
    The rig's directions are fixed in the face's frame and a rotation changes `light_rgb` only, so the whole turntable is ONE
    network pass and L marches.  The F rotated direction sets are F small matmuls issued before the frames (the single call's own
    `directions @ rotation`, so that the cell maps cannot differ from its in a last bit).  Per frame four launches -- the cell
    map, the integration, the rig combine, the image kernel -- and a fifth with `fix_border`; one more in total stacks the
    frames.
    `fused=True`: the same bytes from the same pass and the same F matmuls, then one stack, ONE cell-map launch and ONE
    integration launch for all frames (`lighting.environment_lights_frames`), ONE rig-frames launch (`lighting.rig_frames_u8`),
    and one more with `fix_border` -- no per-frame launch and no f32 image per frame."""
    x = _as(images, device, single=3)
    directions = _environment_directions(n_lights, min_z, x.device)
    rots = torch.as_tensor(rotations, dtype=torch.float32).to(x.device)
    if rots.dim() != 3 or tuple(rots.shape[1:]) != (3, 3) or rots.shape[0] < 1:
        raise GcfrError("rotations must be (F,3,3) with F >= 1; got %s" % (tuple(rots.shape),))
    env_d = _as(env, x.device, single=3).contiguous()
    _check_environment(env_d, directions, None, None, faces=x.shape[0])               # a malformed map fails before the network pass
    out, cm, transfer = _lights_pass(model, x, mask_u8, directions, ambient, focal, device, composite_mask_u8, epoch)
    if fused:
        return _rig_frames(x, out, cm, environment_lights_frames(env_d, directions, rots, min_cos), transfer, fix_border)
    dirs_map = [directions @ rots[f] for f in range(rots.shape[0])]
    frames = [_rig_composites(x, out, cm, _environment_lights(env_d, d, min_cos, None), transfer, fix_border) for d in dirs_map]
    return torch.stack(frames, dim=1)


@torch.no_grad()
def capture_rig(model, reference_images, mask_u8, lights, ridge: float = 1e-3, shared: bool = False, ambient: float = 0.5,
                focal: float = None, device="cuda", composite_mask_u8=None, epoch: int = 200, nonnegative: bool = False) -> torch.Tensor:
    """The rig `light_rgb` (B,L,3) -- (1,L,3) with `shared=True` -- of the photographs `reference_images` (B,H,W,3): the colour x
    weight of each of `lights` (L,3) | (B,L,3), 1 <= L <= 64, under which the model's own albedo and per-light shadings of a
    photograph come closest to that photograph inside the compositing mask.  ONE network pass (`forward_lights`) on the reference
    photographs, then `lighting.fit_light_rgb` on its albedo and final shading against the photographs themselves, weighted by the
    compositing mask (`composite_mask_u8`, or `mask_u8` where that is None; u8 / 255).  A device tensor, not differentiable, no
    host synchronisation; it is what `relight_rig(_device)` and `RelightSession(light_rgb=...)` take.  `ridge` / `shared`: see
    `fit_light_rgb`, which also says why entries may be negative; `nonnegative=True` fits under light_rgb >= 0 instead (see there).
    `model` / `ambient` / `focal` as in `relight_lights`."""
    x = _as(reference_images, device, single=3)
    n = (lights.shape if torch.is_tensor(lights) else np.asarray(lights).shape)
    L = n[-2] if len(n) >= 2 else 1
    if not 1 <= L <= MAX_FIT_LIGHTS:                                                  # a rig too large fails before the network pass
        raise GcfrError("capture_rig: 1 <= L <= %d lights; got %d" % (MAX_FIT_LIGHTS, L))
    out, cm, _transfer = _lights_pass(model, x, mask_u8, lights, ambient, focal, device, composite_mask_u8, epoch)
    return fit_light_rgb(out[8], out[0], x, weight=cm.reshape(x.shape[1], x.shape[2]), ridge=ridge, shared=shared,
                         nonnegative=nonnegative)


@torch.no_grad()
def rig_lighting_transfer(model, input_images, reference_images, mask_u8, lights, ridge: float = 1e-3, shared: bool = False,
                          ambient: float = 0.5, focal: float = None, device="cuda", fix_border: bool = False,
                          composite_mask_u8=None, epoch: int = 200, nonnegative: bool = False) -> torch.Tensor:
    """"Light this face like that photograph", at the level of a rig: `capture_rig` on `reference_images[b]`, then
    `relight_rig_device` on `input_images[b]` with the captured rig -- (B,H,W,3) uint8 DEVICE composites, equal byte for byte to
    `relight_rig_device(model, input_images, mask_u8, lights, capture_rig(model, reference_images, mask_u8, lights, ...), ...)`
    given the same network outputs.  The counterpart of `lighting_transfer`, which reads ONE white light and one ambient from the
    network's lighting head: here `lights` (L,3) | (B,L,3) are fixed directions (a key / fill / rim set, `lighting.sphere_directions`)
    and their colours x weights come from the photograph.  Two network passes, one per set of photographs; with `shared=True` one
    rig is fitted to all reference photographs and applied to every input.  `nonnegative` is `capture_rig`'s."""
    rgb = capture_rig(model, reference_images, mask_u8, lights, ridge, shared, ambient, focal, device, composite_mask_u8, epoch,
                      nonnegative)
    return relight_rig_device(model, input_images, mask_u8, lights, rgb, ambient, focal, device, fix_border, composite_mask_u8, epoch)


def fold_batchnorm(model):
    """An EVAL-mode copy of a RelightNet* model with every BatchNorm folded into the convolution in front of it.

    The hourglass applies `bn_X(conv_X(x))` / `bn_X(deconv_X(x))` everywhere (T8:199-350; `_Hourglass._cb`).  In eval mode a
    BatchNorm is the affine map `y = (x - mean) * gamma / sqrt(var + eps) + beta` with constants, so it folds into the
    convolution's weight (scaled per OUTPUT channel: dim 0 of a Conv2d weight, dim 1 of a ConvTranspose2d weight) and bias; the
    copy's `bn_X` modules become `nn.Identity` and 56 elementwise kernels per pass disappear (the convolutions stay MIOpen's).
    A deployment optimisation for inference only: the folded products are rounded once more than the reference's two-step
    evaluation (network outputs agree to ~1e-6 relative, the uint8 composites on >= 99.9 % of the bytes:
    tests/test_gpu_relight_lights.py); the copy's state_dict no longer has the reference's BatchNorm entries, so checkpoints are
    loaded into the ORIGINAL model and folded afterwards.  Raises if the model is in training mode (batch statistics do not fold)."""
    import copy
    import torch.nn as nn
    if model.training:
        raise ValueError("fold_batchnorm needs model.eval(): training-mode BatchNorm uses batch statistics")
    m = copy.deepcopy(model)
    with torch.no_grad():
        for name, bn in list(m.named_children()):
            if not name.startswith("bn_") or not isinstance(bn, nn.BatchNorm2d):
                continue
            base = name[3:]
            conv = getattr(m, "conv_" + base, None)
            kind = "conv"
            if conv is None:
                conv, kind = getattr(m, "deconv_" + base, None), "deconv"
            if conv is None:
                continue
            scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
            shift = bn.bias - bn.running_mean * scale
            if kind == "conv":
                conv.weight.mul_(scale.reshape(-1, 1, 1, 1))
            else:                                               # ConvTranspose2d: (in, out / groups, kH, kW)
                conv.weight.mul_(scale.reshape(1, -1, 1, 1))
            if conv.bias is None:
                conv.bias = nn.Parameter(shift.clone())
            else:
                conv.bias.mul_(scale).add_(shift)
            setattr(m, name, nn.Identity())
    return m.eval()


class RelightSession:
    """Steady-state serving form of `relight_lights_device` for a fixed shape: B photographs x L lights of H x W.

    The eager pass is host-bound -- ~350 kernel launches of the network's small convolutions, the block's two and the image
    kernel's one, issued one by one from Python (bench.py `relight_e2e`: 4.7 ms per pass of 8 faces of which the GPU is busy a
    fraction).  Here the WHOLE pass -- network forward (eval), render block, uint8 image kernel -- is captured ONCE into a
    hipGraph on static buffers; `run(images)` copies the new photographs into the static input and replays it: one launch per
    pass.  Nothing in the block allocates or synchronises (include/gcfr.h), MIOpen runs in immediate mode (no find pass inside
    the capture), the camera matrix is a host tensor.  The captured kernels are the eager pass's kernels with the eager pass's
    arguments: the composites equal `relight_lights_device` on the same inputs up to MIOpen's own run-to-run jitter
    (tests/test_gpu_relight_lights.py).  `graph=False` keeps the static buffers and runs eagerly (the A/B).
    `miopen_find=True`: the warm-up passes run with `torch.backends.cudnn.benchmark` on, so MIOpen SEARCHES the fastest solver
    for each of the network's convolutions at this batch size (once per process and shape: seconds to a minute or two of
    construction time on a cold kernel cache) and the capture then holds those solvers instead of the immediate-mode
    heuristic's picks; the flag is restored afterwards.
    `light_rgb` (L,3) | (1,L,3) | (B,L,3): the L lights are a RIG with this colour x weight per light (`relight_rig_device`): the
    captured pass ends in the rig stage (lighting.combine_lights) and `run()` returns ONE composite per face, (B,H,W,3).  None
    (the default): nothing changes."""

    def __init__(self, model, B: int, mask_u8, lights, ambient: float = 0.5, focal: float = None, device="cuda",
                 H: int = 256, W: int = 256, fix_border: bool = False, composite_mask_u8=None, graph: bool = True, epoch: int = 200,
                 miopen_find: bool = False, light_rgb=None):
        self.model, self.device, self.epoch, self.ambient, self.fix_border = model, torch.device(device), epoch, float(ambient), fix_border
        self.transfer = _is_transfer(model)
        self.K = camera_matrix(_default_focal(self.transfer, focal), H, W)                                   # host
        self.m_u8 = _as(mask_u8, self.device, torch.uint8).reshape(H, W)
        self.cm = self.m_u8 if composite_mask_u8 is None else _as(composite_mask_u8, self.device, torch.uint8).reshape(H, W)
        self.mask = (self.m_u8.to(torch.float64).reshape(H, W, 1) / 255.0)
        self.lights = _as(lights, self.device, single=1).contiguous()
        self.light_rgb = None if light_rgb is None else _as(light_rgb, self.device, single=2).contiguous()   # a rig: one composite per face
        self.x = torch.zeros((B, H, W, 3), dtype=torch.float32, device=self.device)
        self.ambient_dev = torch.full((1,), self.ambient, dtype=torch.float32, device=self.device)   # (no host-to-device copy inside the capture)
        self.out = None
        self.graph = None
        find_before = torch.backends.cudnn.benchmark
        if miopen_find:
            torch.backends.cudnn.benchmark = True
        try:
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):                     # warm-up outside the capture (allocator, MIOpen's solution look-up / search)
                for _ in range(2 if graph else (1 if miopen_find else 0)):
                    self._pass()
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            if graph:
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self.out = self._pass()
        finally:
            torch.backends.cudnn.benchmark = find_before

    @torch.no_grad()
    def _pass(self):
        # inside a graph there is no launch latency for a side stream to hide: no hoisted prepass there (None: the model's own choice)
        hoist = False if (self.graph is not None or torch.cuda.is_current_stream_capturing()) else None
        o = _forward_lights(self.model, self.x, self.epoch, self.K, self.mask, self.lights, self.ambient_dev, hoist=hoist)
        if self.light_rgb is not None:
            return _rig_composites(self.x, o, self.cm, self.light_rgb, self.transfer, self.fix_border)
        return _light_composites(self.x, o, self.cm, self.transfer, self.fix_border)

    @torch.no_grad()
    def run(self, images=None) -> torch.Tensor:
        """images (B,H,W,3) f32 in [0,1] (host or device; None = whatever the static input holds) -> (B,L,H,W,3) uint8 DEVICE
        tensor ((B,H,W,3) for a session built with `light_rgb`); with a graph it is overwritten by the next run."""
        if images is not None:
            self.x.copy_(_as(images, None, single=3), non_blocking=True)
        if self.graph is None:
            return self._pass()
        self.graph.replay()
        return self.out


@torch.no_grad()
def lighting_transfer(model: RelightNetLightingTransfer, input_image, reference_image, mask_u8,
                      focal: float = 700.0, device="cuda") -> Dict[str, np.ndarray]:
    """SLT:535-579: pass 1 on the reference image with a zero target light reads the estimated light and ambient
    (SLT:543); pass 2 relights the input image with them (SLT:545).  Returns the six images SLT:574-579 writes
    (uint8 RGB / single channel, composited and quantised on the device) plus the estimated light."""
    xin, xref = _as(input_image, device, single=3), _as(reference_image, device, single=3)
    _, H, W, _ = xin.shape
    K = camera_matrix(focal, H, W, device)
    mask = (torch.as_tensor(np.asarray(mask_u8), dtype=torch.float64).reshape(H, W, 1) / 255.0).to(device)
    zero_l = torch.zeros(1, 3, 1, 1, device=device)
    zero_a = torch.zeros(1, 1, 1, device=device)
    est = model(xref, 200, K, mask, zero_l, zero_a)
    est_light, est_amb = est[10], est[11]
    out = model(xin, 200, K, mask, est_light.reshape(1, 3, 1, 1).float(), est_amb.reshape(1, 1, 1).float())
    m_u8 = torch.as_tensor(np.asarray(mask_u8), dtype=torch.uint8, device=device)
    dev_imgs = pp.inference_images_device(xin, out[5], m_u8, albedo=out[0], depth=out[1], shadow_mask_weights=out[2],
                                          final_shading=out[8], surface_normals=out[9], mask_f32=True)      # SLT:540
    imgs = {k: v[0].cpu().numpy() for k, v in dev_imgs.items()}                # uint8, what SLT:574-579 writes
    imgs["estimated_light"] = est_light.reshape(3).cpu().numpy()
    imgs["estimated_ambient"] = est_amb.reshape(1).cpu().numpy()
    return imgs
