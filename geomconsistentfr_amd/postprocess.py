"""Callers and data formats either side of the render block -- device side and file formats.

Device path (HIP kernels of csrc/gcfr_postprocess.hip, no CPU fallback): `inference_images_device`,
`fix_border_artifacts_device` -- what the inference mirrors use, so a relit batch leaves the GPU as bytes:

  inference_images_device       S1:614-620 / S8:583-608 / SLT:547-579: composite + the five diagnostic maps, quantised
                                to the bytes cv2.imwrite stores
  fix_border_artifacts_device   fix_border_artifacts_CVPR2022.m:1-18
  ingest_photographs_device     the uint8 photograph at 1, 2, 4 or 8 times the network's side -> the network's f32 input
                                (S1:515/580 without the host-side cv2.resize), csrc/gcfr_fullres.hip
  fullres_composites_device     the relit low-resolution images carried back onto the photograph's own pixels, uint8
  ingest_box_device             a face box of any size and position inside a larger photograph -> the network's f32 input,
                                csrc/gcfr_fullres_box.hip
  fullres_box_composites_device the relit images carried back onto the box's pixels: the photograph relit inside the box, uint8;
                                upsample="guided": edge-aware, csrc/gcfr_fullres_box_guided.hip
  ingest_anybox_device          `ingest_box_device` for a box that may be SMALLER than the network's input on either axis,
                                csrc/gcfr_fullres_anybox.hip
  fullres_anybox_composites_device  `fullres_box_composites_device` for such a box
  ingest_group_device           `ingest_anybox_device` for B faces spread over P photographs (a group photograph),
                                csrc/gcfr_fullres_group.hip
  fullres_group_composites_device   every face of a photograph relit in ONE pass over it: one photograph per photograph out
  ingest_affine_device          a ROTATED face: the photograph sampled through a 2 x 3 affine map (what a face aligner reports) ->
                                the network's f32 input, csrc/gcfr_fullres_affine.hip
  fullres_affine_composites_device  the relit images carried back through the inverse map onto the photograph's pixels
  quantise_affine, affine_from_rotated_box   (host) the integer matrices those two read; the map of a rotated box
  ingest_group_affine_device    `ingest_affine_device` for B tilted faces spread over P photographs,
                                csrc/gcfr_fullres_group_affine.hip
  fullres_group_affine_composites_device   every tilted face of a photograph relit in ONE pass over it

Host side: the on-disk formats of load_data() (T8:545-556).  The numpy statements of the script lines these kernels
implement live in oracle/postprocess_statements.py (test infrastructure, pinned to the reference's own main() by
tests/golden/slt_main_*.npz); nothing here imports them.
"""
import numpy as np


# ------------------------------------------------------------------------------------------------
# device path (csrc/gcfr_postprocess.hip)
# ------------------------------------------------------------------------------------------------
def inference_images_device(input_images, rendered, mask_u8, albedo=None, depth=None, shadow_mask_weights=None,
                            final_shading=None, surface_normals=None, mask_f32=False):
    """The images S1:614-620 / S8:603-608 / SLT:574-579 write, as uint8 device tensors (RGB, HWC), straight from the
    forward's device outputs: `rendered_image` always, the five diagnostic maps for whichever inputs are given.
    input_images (B,H,W,3) f32 in [0,1]; rendered / albedo / surface_normals (B,3,H,W); depth (B,1,H,W) or (B,H,W);
    shadow_mask_weights / final_shading (B,H,W); mask_u8 (1|B,H,W) or (H,W) uint8 skin mask as stored on disk (the kernel
    forms the scripts' mask/255.0 itself: f64 as S1:580 / S8:569 hold it, or with mask_f32=True f32 as SLT:540 does).
    Many lights per face: rendered (B,L,3,H,W) (and shadow_mask_weights / final_shading (B,L,H,W)) give `rendered_image`
    (B,L,H,W,3) (`shadow_mask` / `shading` (B,L,H,W)) from ONE launch that reads each photograph once per light in place --
    no L-fold copy of the input; the per-photograph maps (albedo, depth, normals) keep their (B,...) shapes."""
    import torch
    from . import _lib
    what, x = "inference_images_device", input_images
    per_light = [("shadow_mask_weights", shadow_mask_weights), ("final_shading", final_shading)]
    per_face = [("albedo", albedo), ("surface_normals", surface_normals)]
    named = [("input_images", x), ("rendered", rendered)] + per_light + per_face + [("depth", depth)]
    tensors = _lib.check_tensors(what, named, **{n: _lib.FLOATS for n, _ in named})      # (whatever is not f32 is converted below)
    _lib.check_tensors(what, [("mask_u8", mask_u8)], mask_u8=torch.uint8)                 # (on any device: it is moved to the images')
    if x.dim() != 4 or x.shape[3] != 3:
        raise _lib.GcfrError("input_images must be (B,H,W,3); got %s" % (tuple(x.shape),))
    B, H, W, _ = x.shape
    multi = rendered.dim() == 5
    L = rendered.shape[1] if multi else 1
    lead = (B, L) if multi else (B,)
    of = " for rendered %s" % (tuple(rendered.shape),)
    _lib.check_shape("rendered", rendered, (B, 3, H, W), (B, L, 3, H, W), why=" for input images %s" % (tuple(x.shape),))
    for n, t in per_light:              # the kernel indexes these planes at (b L + l) H W, the per-face ones at b
        if t is not None:
            _lib.check_shape(n, t, lead + (H, W), why=of)
    for n, t in per_face:
        if t is not None:
            _lib.check_shape(n, t, (B, 3, H, W), why=" (per face, no light axis)" + of)
    if depth is not None:
        _lib.check_shape("depth", depth, (B, 1, H, W), (B, H, W), why=of)
    _lib.check_shape("mask_u8", mask_u8, (H, W), (1, H, W), (B, H, W), why=" (the uint8 skin mask, 0..255)")
    _lib.require_device(*tensors)
    f = _lib.f32c
    x, rendered = f(x), f(rendered)
    m = mask_u8.to(x.device).contiguous().reshape(-1, H, W)
    albedo, shadow_mask_weights, final_shading, surface_normals = f(albedo), f(shadow_mask_weights), f(final_shading), f(surface_normals)
    drange = None
    if depth is not None:
        depth = f(depth).reshape(B, H, W)
        neg = -depth
        drange = torch.stack([neg.amin(), neg.amax()]).contiguous()              # stays on the device: no sync
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=x.device)
    out = {"rendered_image": u8(*lead, H, W, 3)}
    if shadow_mask_weights is not None:
        out["shadow_mask"] = u8(*lead, H, W)
    if albedo is not None:
        out["albedo"] = u8(B, H, W, 3)
    if depth is not None:
        out["depth"] = u8(B, H, W)
    if final_shading is not None:
        out["shading"] = u8(*lead, H, W)
    if surface_normals is not None:
        out["surface_normals"] = u8(B, H, W, 3)
    _lib.launch("gcfr_inference_images_u8", x.device, x, rendered, albedo, depth, drange, shadow_mask_weights, final_shading,
                surface_normals, m, m.shape[0], B, L, H, W, out["rendered_image"], out.get("shadow_mask"), out.get("albedo"),
                out.get("depth"), out.get("shading"), out.get("surface_normals"), int(bool(mask_f32)), _lib.STREAM)
    return out


def fix_border_artifacts_device(img_u8, face_mask_u8):
    """fix_border_artifacts_CVPR2022.m on the device: img_u8 (B,H,W,3) uint8, face_mask_u8 (1|B,H,W) or (H,W) uint8
    skin mask as stored on disk.  Returns a new (B,H,W,3) uint8 tensor."""
    import torch
    from . import _lib
    what = "fix_border_artifacts_device"
    _lib.check_tensors(what, [("img_u8", img_u8)], img_u8=torch.uint8)
    _lib.check_tensors(what, [("face_mask_u8", face_mask_u8)], face_mask_u8=torch.uint8)  # (on any device: it is moved to the images')
    if img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise _lib.GcfrError("img_u8 must be (B,H,W,3); got %s" % (tuple(img_u8.shape),))
    B, H, W, _ = img_u8.shape
    _lib.check_shape("face_mask_u8", face_mask_u8, (H, W), (1, H, W), (B, H, W), why=" for img_u8 %s" % (tuple(img_u8.shape),))
    _lib.require_device(img_u8)
    img = img_u8.contiguous()
    mk = face_mask_u8.to(img.device).contiguous().reshape(-1, H, W)
    out = torch.empty_like(img)
    _lib.launch("gcfr_fix_border_u8", img.device, img, mk, mk.shape[0], B, H, W, out, _lib.STREAM)
    return out


FULLRES_SCALES = (1, 2, 4, 8)       # photograph side / network side (csrc/gcfr_fullres.hip)
FULLRES_MAX_LIGHTS = 4096


def _check_photographs(photo_u8, scale, what, boxed=False):
    """-> (B, h, w, s) of uint8 photographs (B, s h, s w, 3) within the kernels' 31-bit limits, or GcfrError (where they live is the
    caller's last check).  `boxed`: photographs (B,Hp,Wp,3) of any size but empty, as the box entries take them (at scale 1)."""
    import torch
    from . import _lib
    _lib.check_tensors(what, [("photographs", photo_u8)], photographs=torch.uint8)
    if photo_u8.dim() != 4 or photo_u8.shape[-1] != 3 or (boxed and min(photo_u8.shape) < 1):
        raise _lib.GcfrError("%s: photographs must be a uint8 tensor (B,%s,3); got %s" % (what, "Hp,Wp" if boxed else "H,W", tuple(photo_u8.shape)))
    if isinstance(scale, bool) or not isinstance(scale, int) or scale not in FULLRES_SCALES:
        raise _lib.GcfrError("%s: scale must be one of %s; got %r" % (what, FULLRES_SCALES, scale))
    B, H, W, _ = photo_u8.shape
    if B < 1 or H < 1 or W < 1 or H % scale or W % scale:
        raise _lib.GcfrError("%s: photographs %s are not (B, scale h, scale w, 3) for scale %d" % (what, tuple(photo_u8.shape), scale))
    if H * W > 0x7fffffff or B * ((H * W + 1023) // 1024) > 0x7fffffff:
        raise _lib.GcfrError("%s: %d photographs of %d x %d pixels do not fit the kernels' 31-bit pixel and chunk counts" % (what, B, H, W))
    return B, H // scale, W // scale, scale


def _check_composite_tensors(what, x_lo, rendered, mask_u8, out):
    """what both composites take beside the photographs is tensors of the right types: an entry's first look at them"""
    import torch
    from . import _lib
    _lib.check_tensors(what, [("x_lo", x_lo), ("rendered", rendered), ("mask_u8", mask_u8), ("out", out)], one_device=False,
                       rendered=_lib.FLOATS, mask_u8=torch.uint8, out=torch.uint8)


def _composite_operands(what, photo_u8, x_lo, rendered, mask_u8, out, detail_clamp, floor, B, h, w, window, frame="", images=None):
    """The operands both composites share, for B faces of a network of (h, w) and an output `window` (rows, columns), or GcfrError
    -> the photographs, x_lo, rendered and the mask as the kernels read them, L, and the result's shape.  `images`: the number of
    images that come back where it is not one per face (the group entry's P)."""
    import torch
    from . import _lib
    _lib.check_shape("x_lo", x_lo, (B, h, w, 3))
    L = rendered.shape[1] if rendered.dim() == 5 else 1
    n = B if images is None else images
    shape = ((n, L) if rendered.dim() == 5 else (n,)) + tuple(window) + (3,)
    _lib.check_shape("rendered", rendered, (B, 3, h, w), (B, L, 3, h, w))
    if not 1 <= L <= FULLRES_MAX_LIGHTS:
        raise _lib.GcfrError("%s: rendered %s: 1 <= L <= %d" % (what, tuple(rendered.shape), FULLRES_MAX_LIGHTS))
    _lib.check_shape("mask_u8", mask_u8, (h, w), (1, h, w), (B, h, w), why=" (the uint8 skin mask at the network's resolution%s)" % frame)
    if not float(detail_clamp) >= 1.0 or not float(floor) > 0.0:
        raise _lib.GcfrError("%s: detail_clamp >= 1 and floor > 0; got %r, %r" % (what, detail_clamp, floor))
    _lib.check_out(out, shape)
    _lib.require_device(photo_u8, x_lo, rendered, mask_u8, out)
    return (photo_u8.detach().contiguous(), x_lo.detach().contiguous(), rendered.detach().to(torch.float32).contiguous(),
            mask_u8.contiguous().reshape(-1, h, w), L, shape)


def ingest_photographs_device(photo_u8, scale):
    """The network's input from the photographs, on the device: photo_u8 (B, s h, s w, 3) uint8 -> (B,h,w,3) f32 in [0,1], the
    mean of every s x s block of bytes over 255 (the integer sum, one f64 division, one rounding to f32: csrc/gcfr_fullres.hip).
    `scale` s is 1, 2, 4 or 8; at 1 the result has the bits of np.float32(img / 255.0), what the scripts feed the network
    (S1:515/580).  Replaces the scripts' host-side cv2.resize and the upload of an f32 image.  One launch, no host
    synchronisation; a malformed input raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    B, h, w, s = _check_photographs(photo_u8, scale, "ingest_photographs_device")
    _lib.require_device(photo_u8)
    photo = photo_u8.detach().contiguous()
    x_lo = torch.empty((B, h, w, 3), dtype=torch.float32, device=photo.device)
    _lib.launch("gcfr_ingest_photographs_u8", photo.device, photo, B, h, w, s, x_lo, _lib.STREAM)
    return x_lo


FULLRES_UPSAMPLES = ("bilinear", "guided")


def _check_upsample(what, upsample, range_sigma):
    """the two keywords of both composite entries, or GcfrError: an entry's first check, with either upsample"""
    from . import _lib
    if upsample not in FULLRES_UPSAMPLES:
        raise _lib.GcfrError("%s: upsample must be one of %s; got %r" % (what, FULLRES_UPSAMPLES, upsample))
    if isinstance(range_sigma, bool) or not isinstance(range_sigma, (int, float)) or not float(range_sigma) > 0.0:
        raise _lib.GcfrError("%s: range_sigma > 0 (grey levels); got %r" % (what, range_sigma))


def fullres_composites_device(photo_u8, x_lo, rendered, mask_u8, scale, detail_clamp=4.0, floor=1.0, out=None, upsample="bilinear",
                              range_sigma=20.0):
    """The relit low-resolution `rendered` of ONE pass carried back onto the photographs' own pixels, as uint8 on the device:
    photo_u8 (B, s h, s w, 3) uint8; x_lo (B,h,w,3) f32, the network's input (`ingest_photographs_device`); rendered (B,L,3,h,w)
    -> (B,L,H,W,3), or (B,3,h,w) -> (B,H,W,3); mask_u8 (1|B,h,w) or (h,w) uint8, the compositing mask AT THE NETWORK'S RESOLUTION
    as stored on disk.  Quotient / detail transfer (include/gcfr.h states every operation): the photograph's detail relative to
    its own low-resolution version, d = clamp(photo / max(255 Up(x_lo), floor), 1 / detail_clamp, detail_clamp), multiplies the
    bilinearly upsampled relit image, and the upsampled mask m BLENDS it with the photograph, v = p + m (255 Up(rendered) d - p);
    where m is 0 the photograph's byte is kept, whatever `rendered` holds there.  `floor` is in grey levels.  ONE launch for all L
    lights: the photograph, x_lo and the mask are read once per pixel.  `rendered` is the only operand that may be non-f32 on
    entry.  `out`: a contiguous uint8 buffer of the result's shape that is written and returned (not the photographs).
    `upsample`: "bilinear" (the default) is the launch described above; "guided" replaces Up in all three places by the
    EDGE-AWARE joint-bilateral upsample of csrc/gcfr_fullres_guided.hip (include/gcfr.h states it): a 4 x 4 tent of low-resolution
    taps whose weights fall off with the squared distance, in grey levels, between the photograph's pixel and 255 x_lo at the tap,
    k = 1 / (1 + d2 / range_sigma^2), so that neither the relighting gain nor the mask crosses an edge the network's resolution
    does not see.  `range_sigma` > 0 (grey levels; +inf: the spatial tent alone) is used by "guided" only; its default of 20 is an
    argument, NOT a tuned value.  NOT DIFFERENTIABLE.  No host synchronisation; a malformed input raises GcfrError before anything
    is loaded or launched."""
    import torch
    from . import _lib
    what = "fullres_composites_device"
    _check_upsample(what, upsample, range_sigma)
    B, h, w, s = _check_photographs(photo_u8, scale, what)
    _check_composite_tensors(what, x_lo, rendered, mask_u8, out)
    photo, x, ren, m, L, shape = _composite_operands(what, photo_u8, x_lo, rendered, mask_u8, out, detail_clamp, floor, B, h, w, (s * h, s * w))
    if out is not None and out.data_ptr() == photo.data_ptr():
        raise _lib.GcfrError("%s: out must not be the photographs" % what)
    res = torch.empty(shape, dtype=torch.uint8, device=photo.device) if out is None else out
    if upsample == "guided":
        _lib.launch("gcfr_fullres_composites_guided_u8", photo.device, photo, x, ren, m, m.shape[0], B, L, h, w, s, float(floor),
                    float(detail_clamp), float(range_sigma), res, _lib.STREAM)
    else:
        _lib.launch("gcfr_fullres_composites_u8", photo.device, photo, x, ren, m, m.shape[0], B, L, h, w, s, float(floor),
                    float(detail_clamp), res, _lib.STREAM)
    return res


def _check_boxes(boxes, photo_u8, h, w, what, same_size=False, any_size=False, faces=None):
    """-> a contiguous (B,4) int32 numpy array of HOST boxes (x0, y0, bw, bh) that satisfy include/gcfr.h's box rules for the uint8
    photographs (B,Hp,Wp,3) and a network of (h, w), or GcfrError.  `boxes`: (4,) broadcast over the faces or (B,4); a list, a numpy
    array or a CPU tensor of integers.  `any_size`: the relaxed rules of the anybox entries, bw, bh >= 1 with 8 bw >= w and
    8 bh >= h, in the place of bw >= w and bh >= h.  `faces`: B faces over the P photographs (P,Hp,Wp,3) of the group entries, in
    the place of one face per photograph."""
    import torch
    from . import _lib
    B, Hp, Wp, _ = _check_photographs(photo_u8, 1, what, boxed=True)
    if faces is not None:
        B = faces
    if any(isinstance(n, bool) or not isinstance(n, int) or n < 1 for n in (h, w)):
        raise _lib.GcfrError("%s: the network's size (h, w) must be positive integers; got %r" % (what, (h, w)))
    if torch.is_tensor(boxes):
        if boxes.is_cuda:
            raise _lib.GcfrError("%s: boxes are HOST integers (the entry bakes them into its launches); got a tensor on %s" % (what, boxes.device))
        boxes = boxes.detach().numpy()
    try:
        a = np.asarray(boxes)
    except Exception as e:
        raise _lib.GcfrError("%s: boxes must be integers (4,) or (B,4): %s" % (what, e))
    if a.dtype.kind not in "iu":
        raise _lib.GcfrError("%s: boxes must be integers, got %s" % (what, a.dtype))
    if a.shape not in ((4,), (B, 4)):
        raise _lib.GcfrError("%s: boxes must be (4,) or (%d,4) (x0, y0, bw, bh); got %s" % (what, B, a.shape))
    a = np.broadcast_to(a.astype(np.int64), (B, 4))
    for b, (x0, y0, bw, bh) in enumerate(a.tolist()):
        if x0 < 0 or y0 < 0 or x0 + bw > Wp or y0 + bh > Hp:
            raise _lib.GcfrError("%s: box %d (x0 %d, y0 %d, bw %d, bh %d) does not lie inside the %d x %d photograph" % (what, b, x0, y0, bw, bh, Wp, Hp))
        if any_size and (bw < 1 or bh < 1 or 8 * bw < w or 8 * bh < h):
            raise _lib.GcfrError("%s: box %d (%d x %d) is empty or under an eighth of the network's input (%d x %d) on an axis" % (what, b, bw, bh, w, h))
        if not any_size and (bw < w or bh < h):
            raise _lib.GcfrError("%s: box %d (%d x %d) is smaller than the network's input (%d x %d)" % (what, b, bw, bh, w, h))
        if 2 * bh * h > 0x7fffffff or 2 * bw * w > 0x7fffffff:
            raise _lib.GcfrError("%s: box %d: 2 bh h and 2 bw w must fit 31 bits" % (what, b))
        if same_size and (bw, bh) != (int(a[0, 2]), int(a[0, 3])):
            raise _lib.GcfrError("%s: with paste=False all boxes share one (bw, bh); box %d is %d x %d, box 0 is %d x %d"
                                 % (what, b, bw, bh, int(a[0, 2]), int(a[0, 3])))
    return np.ascontiguousarray(a, dtype=np.int32)


def _host_pointer(a):
    """a contiguous numpy array's address for a HOST pointer parameter; the caller keeps `a` alive over the call"""
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p)


def ingest_box_device(photo_u8, boxes, size):
    """The network's input from a FACE BOX inside each photograph, on the device: photo_u8 (B,Hp,Wp,3) uint8 of any size, `boxes`
    host integers (x0, y0, bw, bh) in photograph pixels -- (4,) for every face or (B,4); a list, a numpy array or a CPU tensor --
    and `size` the network's (h, w) (an int: square) -> (B,h,w,3) f32 in [0,1].  The exact area mean of the box over each
    low-resolution cell, over 255 (integer overlap weights, a 64-bit sum, one f64 division, one rounding to f32: include/gcfr.h
    states it; csrc/gcfr_fullres_box.hip).  bw >= w and bh >= h; the two ratios are independent and need not be integers.  With
    the box the whole photograph at 1, 2, 4 or 8 times the network's side these are `ingest_photographs_device`'s bits.  One
    launch per 32 faces, no host synchronisation; a malformed input raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    what = "ingest_box_device"
    h, w = (size, size) if isinstance(size, int) else (tuple(size) if isinstance(size, (tuple, list)) and len(size) == 2 else (None, None))
    bx = _check_boxes(boxes, photo_u8, h, w, what)
    _lib.require_device(photo_u8)
    photo = photo_u8.detach().contiguous()
    B, Hp, Wp, _ = photo.shape
    x_lo = torch.empty((B, h, w, 3), dtype=torch.float32, device=photo.device)
    _lib.launch("gcfr_ingest_box_u8", photo.device, photo, B, Hp, Wp, _host_pointer(bx), h, w, x_lo, _lib.STREAM)
    return x_lo


def fullres_box_composites_device(photo_u8, boxes, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, paste=True, out=None,
                                  upsample="bilinear", range_sigma=20.0):
    """`fullres_composites_device` for a FACE BOX inside each photograph: photo_u8 (B,Hp,Wp,3) uint8 of any size; `boxes` host
    integers (x0, y0, bw, bh) as in `ingest_box_device`; x_lo (B,h,w,3) f32, the network's input (`ingest_box_device`); rendered
    (B,L,3,h,w) or (B,3,h,w); mask_u8 (1|B,h,w) or (h,w) uint8, the compositing mask at the network's resolution IN THE BOX'S
    FRAME.  `paste=True` -> (B,L,Hp,Wp,3) (or (B,Hp,Wp,3)): the photograph, relit inside the box and untouched outside it;
    `paste=False` -> (B,L,bh,bw,3): the box alone, all faces then sharing one (bw, bh).  Inside the box the quotient / detail
    transfer of `fullres_composites_device` with the bilinear Up taken over the box (include/gcfr.h states every operation); with
    the box the whole photograph at 1, 2, 4 or 8 times the network's side, that entry's bytes.  ONE launch per 32 faces for all L
    lights; the boxes travel in the launch's arguments, nothing is uploaded.  `rendered` is the only operand that may be non-f32
    on entry.  `out`: a contiguous uint8 buffer of the result's shape that is written and returned; it must not overlap the
    photographs.  `upsample` / `range_sigma` as in `fullres_composites_device`: "bilinear" (the default) is the launch described
    above; "guided" replaces Up in all three places by the edge-aware joint-bilateral upsample taken over the box
    (csrc/gcfr_fullres_box_guided.hip; include/gcfr.h states it), with that entry's bytes when the box is the whole photograph at
    1, 2, 4 or 8 times the network's side.  NOT DIFFERENTIABLE.  No host synchronisation; a malformed input raises GcfrError before
    anything is loaded or launched."""
    import torch
    from . import _lib
    what = "fullres_box_composites_device"
    _check_upsample(what, upsample, range_sigma)
    if not isinstance(paste, (bool, int)) or paste not in (0, 1):
        raise _lib.GcfrError("%s: paste must be True or False; got %r" % (what, paste))
    _check_composite_tensors(what, x_lo, rendered, mask_u8, out)
    if x_lo.dim() != 4 or x_lo.shape[-1] != 3 or min(x_lo.shape) < 1:
        raise _lib.GcfrError("%s: x_lo must be (B,h,w,3); got %s" % (what, tuple(x_lo.shape)))
    h, w = int(x_lo.shape[1]), int(x_lo.shape[2])
    bx = _check_boxes(boxes, photo_u8, h, w, what, same_size=not paste)
    B, Hp, Wp, _ = photo_u8.shape
    window = (Hp, Wp) if paste else (int(bx[0, 3]), int(bx[0, 2]))
    photo, x, ren, m, L, shape = _composite_operands(what, photo_u8, x_lo, rendered, mask_u8, out, detail_clamp, floor, B, h, w, window,
                                                     frame=", in the box's frame")
    if out is not None and out.data_ptr() < photo.data_ptr() + photo.numel() and photo.data_ptr() < out.data_ptr() + out.numel():
        raise _lib.GcfrError("%s: out must not overlap the photographs" % what)
    res = torch.empty(shape, dtype=torch.uint8, device=photo.device) if out is None else out
    if upsample == "guided":
        _lib.launch("gcfr_fullres_composites_box_guided_u8", photo.device, photo, x, ren, m, m.shape[0], B, L, Hp, Wp, _host_pointer(bx),
                    h, w, int(bool(paste)), float(floor), float(detail_clamp), float(range_sigma), res, _lib.STREAM)
    else:
        _lib.launch("gcfr_fullres_composites_box_u8", photo.device, photo, x, ren, m, m.shape[0], B, L, Hp, Wp, _host_pointer(bx), h, w,
                    int(bool(paste)), float(floor), float(detail_clamp), res, _lib.STREAM)
    return res


def ingest_anybox_device(photo_u8, boxes, size):
    """`ingest_box_device` for a face box that may be SMALLER than the network's input, on either axis or on both: bw, bh >= 1 with
    8 bw >= w and 8 bh >= h -> (B,h,w,3) f32 in [0,1].  Each axis on its own: an axis at least as long as the network's is
    `ingest_box_device`'s exact area mean; a shorter one is magnified by the half-pixel-centre bilinear rule written in integers
    (two taps of weights 2n - rem and rem over 2n).  One exact 64-bit integer, one f64 division, one rounding to f32 for all four
    combinations (include/gcfr.h states it; csrc/gcfr_fullres_anybox.hip); with bw >= w and bh >= h, `ingest_box_device`'s bits
    from this entry's own kernel.  One launch per 32 faces, no host synchronisation; a malformed input raises GcfrError before
    anything is loaded or launched."""
    import torch
    from . import _lib
    what = "ingest_anybox_device"
    h, w = (size, size) if isinstance(size, int) else (tuple(size) if isinstance(size, (tuple, list)) and len(size) == 2 else (None, None))
    bx = _check_boxes(boxes, photo_u8, h, w, what, any_size=True)
    _lib.require_device(photo_u8)
    photo = photo_u8.detach().contiguous()
    B, Hp, Wp, _ = photo.shape
    x_lo = torch.empty((B, h, w, 3), dtype=torch.float32, device=photo.device)
    _lib.launch("gcfr_ingest_anybox_u8", photo.device, photo, B, Hp, Wp, _host_pointer(bx), h, w, x_lo, _lib.STREAM)
    return x_lo


def fullres_anybox_composites_device(photo_u8, boxes, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, paste=True, out=None):
    """`fullres_box_composites_device` for a face box that may be SMALLER than the network's input on either axis (the box rules of
    `ingest_anybox_device`); operands, `paste` and `out` as there.  The relit image, x_lo and the mask are carried to the box per
    axis: an axis at least as long as the network's by that entry's two taps and one lerp, a shorter one by the exact-footprint
    area mean of the at most nine network pixels a box pixel covers (f64 sum of integer weight times value, one division by n, one
    rounding; include/gcfr.h states every operation; csrc/gcfr_fullres_anybox.hip).  Horizontal first, then vertical.  With
    bw >= w and bh >= h these are `fullres_box_composites_device`'s bytes, from this entry's own kernel: there is no dispatch
    between the two.  There is no guided upsample here.  ONE launch per 32 faces for all L lights; large, small and mixed boxes
    may share a launch.  NOT DIFFERENTIABLE.  No host synchronisation; a malformed input raises GcfrError before anything is
    loaded or launched."""
    import torch
    from . import _lib
    what = "fullres_anybox_composites_device"
    if not isinstance(paste, (bool, int)) or paste not in (0, 1):
        raise _lib.GcfrError("%s: paste must be True or False; got %r" % (what, paste))
    _check_composite_tensors(what, x_lo, rendered, mask_u8, out)
    if x_lo.dim() != 4 or x_lo.shape[-1] != 3 or min(x_lo.shape) < 1:
        raise _lib.GcfrError("%s: x_lo must be (B,h,w,3); got %s" % (what, tuple(x_lo.shape)))
    h, w = int(x_lo.shape[1]), int(x_lo.shape[2])
    bx = _check_boxes(boxes, photo_u8, h, w, what, same_size=not paste, any_size=True)
    B, Hp, Wp, _ = photo_u8.shape
    window = (Hp, Wp) if paste else (int(bx[0, 3]), int(bx[0, 2]))
    photo, x, ren, m, L, shape = _composite_operands(what, photo_u8, x_lo, rendered, mask_u8, out, detail_clamp, floor, B, h, w, window,
                                                     frame=", in the box's frame")
    if out is not None and out.data_ptr() < photo.data_ptr() + photo.numel() and photo.data_ptr() < out.data_ptr() + out.numel():
        raise _lib.GcfrError("%s: out must not overlap the photographs" % what)
    res = torch.empty(shape, dtype=torch.uint8, device=photo.device) if out is None else out
    _lib.launch("gcfr_fullres_composites_anybox_u8", photo.device, photo, x, ren, m, m.shape[0], B, L, Hp, Wp, _host_pointer(bx), h, w,
                int(bool(paste)), float(floor), float(detail_clamp), res, _lib.STREAM)
    return res


def _check_photo_index(photo_index, photo_u8, what, faces=None, boxes=None):
    """-> a contiguous (B,) int32 numpy array of HOST indices: the photograph of each of the B faces of the group entries, every one in
    [0, P) for the uint8 photographs (P,Hp,Wp,3), or GcfrError.  `photo_index`: a list, a numpy array or a CPU tensor of integers
    (B,); None: all zeros, which needs P == 1.  B is `faces` where the caller knows it (x_lo's), else photo_index's length, else the
    number of rows of `boxes`."""
    import torch
    from . import _lib
    P = _check_photographs(photo_u8, 1, what, boxed=True)[0]
    if photo_index is None:
        if P != 1:
            raise _lib.GcfrError("%s: photo_index=None means one photograph for every face; got %d photographs" % (what, P))
        if faces is None:
            shape = tuple(boxes.shape) if torch.is_tensor(boxes) else np.shape(boxes) if isinstance(boxes, (list, tuple, np.ndarray)) else ()
            faces = int(shape[0]) if len(shape) == 2 else 1
        return np.zeros((faces,), np.int32)
    if torch.is_tensor(photo_index):
        if photo_index.is_cuda:
            raise _lib.GcfrError("%s: photo_index are HOST integers (the entry bakes them into its launches); got a tensor on %s"
                                 % (what, photo_index.device))
        photo_index = photo_index.detach().numpy()
    try:
        a = np.asarray(photo_index)
    except Exception as e:
        raise _lib.GcfrError("%s: photo_index must be integers (B,): %s" % (what, e))
    if a.dtype.kind not in "iu":
        raise _lib.GcfrError("%s: photo_index must be integers, got %s" % (what, a.dtype))
    if a.ndim != 1 or a.shape[0] < 1 or (faces is not None and a.shape[0] != faces):
        raise _lib.GcfrError("%s: photo_index must be (%s,), one photograph per face; got %s" % (what, "B" if faces is None else faces, a.shape))
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= P:
        raise _lib.GcfrError("%s: photo_index must lie in [0, %d) for %d photographs; got %d .. %d" % (what, P, P, a.min(), a.max()))
    return np.ascontiguousarray(a, dtype=np.int32)


def ingest_group_device(photo_u8, boxes, photo_index, size):
    """`ingest_anybox_device` for a GROUP PHOTOGRAPH: photo_u8 (P,Hp,Wp,3) uint8, B faces with host `boxes` (B,4) (or (4,) for every
    face) under that entry's rules and host `photo_index` (B,) naming each face's photograph -- a list, a numpy array or a CPU
    tensor of integers in [0, P), in any order; a photograph may have no face, one or many; None: every face in the one photograph
    (P == 1) -> (B,h,w,3) f32 in [0,1].  The bits are `ingest_anybox_device(photo_u8[photo_index], boxes, size)`'s, and the
    photographs are neither gathered nor copied (include/gcfr.h states it; csrc/gcfr_fullres_group.hip).  One launch per 32 faces,
    no host synchronisation; a malformed input raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    what = "ingest_group_device"
    h, w = (size, size) if isinstance(size, int) else (tuple(size) if isinstance(size, (tuple, list)) and len(size) == 2 else (None, None))
    pi = _check_photo_index(photo_index, photo_u8, what, boxes=boxes)
    B = int(pi.shape[0])
    bx = _check_boxes(boxes, photo_u8, h, w, what, any_size=True, faces=B)
    _lib.require_device(photo_u8)
    photo = photo_u8.detach().contiguous()
    P, Hp, Wp, _ = photo.shape
    x_lo = torch.empty((B, h, w, 3), dtype=torch.float32, device=photo.device)
    _lib.launch("gcfr_ingest_group_u8", photo.device, photo, P, Hp, Wp, _host_pointer(bx), _host_pointer(pi), B, h, w, x_lo, _lib.STREAM)
    return x_lo


def fullres_group_composites_device(photo_u8, boxes, photo_index, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, out=None):
    """EVERY face of a photograph relit in one pass over the photograph: photo_u8 (P,Hp,Wp,3) uint8; `boxes` and `photo_index` as in
    `ingest_group_device`; x_lo (B,h,w,3) f32, the network's input (`ingest_group_device`); rendered (B,L,3,h,w) -> (P,L,Hp,Wp,3), or
    (B,3,h,w) -> (P,Hp,Wp,3); mask_u8 (1|B,h,w) or (h,w) uint8, per FACE and in the box's frame, exactly as
    `fullres_anybox_composites_device` takes them.  Per photograph and light the result is the CHAIN of that entry's pasted
    composite over the photograph's faces in ascending face index, byte for byte: the running image starts as the photograph; a
    face relights it inside its box where its carried mask is positive, reading the running bytes where that entry reads the
    photograph's, and every step rounds to a byte (include/gcfr.h states it; csrc/gcfr_fullres_group.hip).  Where at most one face
    relights a pixel the byte is that entry's; where two carried masks are positive the second face's gain multiplies the first's
    result, so order matters there and nowhere else.  A photograph without faces comes back as it is for every light; all faces of a
    photograph share the light index.  With `photo_index = arange(B)` and P = B these are `fullres_anybox_composites_device`'s
    bytes.  ONE launch per 32 faces, whole photographs per launch; a photograph with more than 32 faces is continued by further
    launches on the same stream.  There is no `paste=False`, no guided upsample.  `out`: a contiguous uint8 buffer of the result's
    shape that is written and returned; it must not overlap the photographs.  NOT DIFFERENTIABLE.  No host synchronisation; a
    malformed input raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    what = "fullres_group_composites_device"
    _check_composite_tensors(what, x_lo, rendered, mask_u8, out)
    if x_lo.dim() != 4 or x_lo.shape[-1] != 3 or min(x_lo.shape) < 1:
        raise _lib.GcfrError("%s: x_lo must be (B,h,w,3); got %s" % (what, tuple(x_lo.shape)))
    B, h, w = int(x_lo.shape[0]), int(x_lo.shape[1]), int(x_lo.shape[2])
    pi = _check_photo_index(photo_index, photo_u8, what, faces=B)
    bx = _check_boxes(boxes, photo_u8, h, w, what, any_size=True, faces=B)
    P, Hp, Wp, _ = photo_u8.shape
    # (a photograph that is not contiguous is copied below and cannot overlap anything; where the tensors live is the last check)
    if (out is not None and photo_u8.is_contiguous() and out.data_ptr() < photo_u8.data_ptr() + photo_u8.numel()
            and photo_u8.data_ptr() < out.data_ptr() + out.numel()):
        raise _lib.GcfrError("%s: out must not overlap the photographs" % what)
    photo, x, ren, m, L, shape = _composite_operands(what, photo_u8, x_lo, rendered, mask_u8, out, detail_clamp, floor, B, h, w, (Hp, Wp),
                                                     frame=", in the box's frame", images=P)
    res = torch.empty(shape, dtype=torch.uint8, device=photo.device) if out is None else out
    _lib.launch("gcfr_fullres_composites_group_u8", photo.device, photo, x, ren, m, m.shape[0], P, B, L, Hp, Wp, _host_pointer(bx),
                _host_pointer(pi), h, w, float(floor), float(detail_clamp), res, _lib.STREAM)
    return res


AFFINE_ONE = 1 << 14            # the fixed point of the affine entries: a matrix entry is an integer number of 2^-14 (include/gcfr.h)
AFFINE_MAX_NORM = 8             # the longest column an affine entry takes: K(M) is 1, 2, 4 or 8
AFFINE_MAX_SHIFT = 1 << 40      # the largest |M02|, |M12|


def affine_sub_samples(M):
    """K(M) of include/gcfr.h for one (2,3) integer matrix: the smallest of 1, 2, 4, 8 with K^2 ONE^2 >= the longer column's
    squared length, in exact integers; None for a column longer than 8"""
    m = [[int(v) for v in row] for row in M]
    n2 = max(m[0][0] ** 2 + m[1][0] ** 2, m[0][1] ** 2 + m[1][1] ** 2)
    return next((K for K in (1, 2, 4, 8) if (K * AFFINE_ONE) ** 2 >= n2), None)


def _check_affine_integers(M, what, name, face):
    """one (2,3) integer matrix under include/gcfr.h's rules, or GcfrError"""
    from . import _lib
    m = [[int(v) for v in row] for row in M]
    if m[0][0] * m[1][1] - m[0][1] * m[1][0] <= 0:
        raise _lib.GcfrError("%s: %s of face %d has a determinant <= 0: a mirror image (which would need a mirrored light) or no map at all"
                             % (what, name, face))
    if affine_sub_samples(m) is None:
        raise _lib.GcfrError("%s: %s of face %d has a column longer than %d: a step of one pixel crosses more than %d pixels"
                             % (what, name, face, AFFINE_MAX_NORM, AFFINE_MAX_NORM))
    if max(abs(m[0][2]), abs(m[1][2])) > AFFINE_MAX_SHIFT:
        raise _lib.GcfrError("%s: %s of face %d has a translation beyond 2^26 pixels" % (what, name, face))


def quantise_affine(net_to_photo):
    """The integer pair the affine entries read, from one f64 matrix, on the host: `net_to_photo` (2,3) or (B,2,3), the map
    (X, Y) = A (u, v, 1) from the network's continuous coordinates to the photograph's (pixel k covers [k, k+1) on both sides) ->
    (F, I), int64 numpy arrays of that shape in units of 2^-14: F = rint(A 2^14), network -> photograph, and
    I = rint(inverse(F / 2^14) 2^14), photograph -> network, the inverse of the QUANTISED F written out in f64 (det = a d - b c; the
    linear part (d, -b; -c, a) / det; the translation -(linear part) t).  Refused with GcfrError: entries that are not finite, a
    determinant <= 0 (a mirror image), a column of either matrix longer than 8, a translation beyond 2^26 pixels."""
    from . import _lib
    what = "quantise_affine"
    try:
        A = np.array(net_to_photo, dtype=np.float64)
    except Exception as e:
        raise _lib.GcfrError("%s: net_to_photo must be numbers (2,3) or (B,2,3): %s" % (what, e))
    if A.shape[-2:] != (2, 3) or A.ndim not in (2, 3) or (A.ndim == 3 and A.shape[0] < 1):
        raise _lib.GcfrError("%s: net_to_photo must be (2,3) or (B,2,3); got %s" % (what, A.shape))
    if not np.isfinite(A).all() or np.abs(A).max() > 2.0 ** 27:
        raise _lib.GcfrError("%s: net_to_photo must be finite, with no entry beyond 2^27" % what)
    Fq = np.rint(A * AFFINE_ONE).astype(np.int64)
    for b, m in enumerate(Fq.reshape(-1, 2, 3)):
        _check_affine_integers(m, what, "F (network -> photograph)", b)
    f = Fq.astype(np.float64) / AFFINE_ONE
    a, b_, tx, c, d, ty = f[..., 0, 0], f[..., 0, 1], f[..., 0, 2], f[..., 1, 0], f[..., 1, 1], f[..., 1, 2]
    det = a * d - b_ * c
    i00, i01, i10, i11 = d / det, -b_ / det, -c / det, a / det
    inv = np.stack([np.stack([i00, i01, -(i00 * tx + i01 * ty)], -1), np.stack([i10, i11, -(i10 * tx + i11 * ty)], -1)], -2)
    if not np.isfinite(inv).all() or np.abs(inv).max() > 2.0 ** 27:
        raise _lib.GcfrError("%s: the inverse map has an entry beyond 2^27" % what)
    Iq = np.rint(inv * AFFINE_ONE).astype(np.int64)
    for b, m in enumerate(Iq.reshape(-1, 2, 3)):
        _check_affine_integers(m, what, "I (photograph -> network)", b)
    return Fq, Iq


def affine_from_rotated_box(cx, cy, bw, bh, angle_degrees, size):
    """The map network -> photograph of a ROTATED face box, (2,3) f64 for `quantise_affine` and the affine entries: a box of
    bw x bh photograph pixels centred at (cx, cy) and turned by `angle_degrees` about its centre, clockwise as the photograph is
    displayed (+x right, +y down), over a network of `size` (h, w) (an int: square).  With angle 0 and (cx, cy) the centre of the box
    (x0, y0, bw, bh) it is that box's axis-aligned map, (bw / w, 0, x0; 0, bh / h, y0)."""
    from . import _lib
    h, w = (size, size) if isinstance(size, int) else (tuple(size) if isinstance(size, (tuple, list)) and len(size) == 2 else (None, None))
    if any(isinstance(n, bool) or not isinstance(n, int) or n < 1 for n in (h, w)):
        raise _lib.GcfrError("affine_from_rotated_box: size must be the network's (h, w), positive integers; got %r" % (size,))
    vals = np.array([cx, cy, bw, bh, angle_degrees], dtype=np.float64)
    if vals.shape != (5,) or not np.isfinite(vals).all() or not (vals[2] > 0 and vals[3] > 0):
        raise _lib.GcfrError("affine_from_rotated_box: cx, cy, bw > 0, bh > 0 and the angle must be finite numbers")
    cx, cy, bw, bh, ang = vals.tolist()
    quarter = ang / 90.0
    if quarter == np.floor(quarter):                   # whole quarter turns: exact sines
        co, si = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter) % 4]
    else:
        co, si = float(np.cos(np.radians(ang))), float(np.sin(np.radians(ang)))
    sx, sy = bw / w, bh / h
    A = np.array([[co * sx, -si * sy, 0.0], [si * sx, co * sy, 0.0]], np.float64)
    A[:, 2] = np.array([cx, cy]) - A[:, :2] @ np.array([w / 2.0, h / 2.0])
    return A


def _affine_integers(net_to_photo, B, what):
    """-> (F, I), contiguous (B,2,3) int64 numpy arrays under include/gcfr.h's rules, from what the affine entries take as the map:
    an f64 matrix (2,3) | (B,2,3) network -> photograph (a list, a numpy array or a CPU tensor), which goes through
    `quantise_affine`, or the INTEGER pair (F, I) of `quantise_affine`, each (2,3) | (B,2,3), which is taken unchanged"""
    import torch
    from . import _lib
    host = lambda a: a.detach().numpy() if torch.is_tensor(a) else a
    # (a pair: a tuple of two matrices; a tuple of two ROWS of numbers is one matrix)
    is_pair = isinstance(net_to_photo, tuple) and len(net_to_photo) == 2 and all(torch.is_tensor(a) or np.ndim(a) >= 2 for a in net_to_photo)
    parts = net_to_photo if is_pair else (net_to_photo,)
    if any(torch.is_tensor(a) and a.is_cuda for a in parts):
        raise _lib.GcfrError("%s: the map is HOST numbers (the entry bakes them into its launches); got a tensor on %s"
                             % (what, next(a.device for a in parts if torch.is_tensor(a) and a.is_cuda)))
    if is_pair:
        pair = []
        for name, a in zip(("F (network -> photograph)", "I (photograph -> network)"), net_to_photo):
            try:
                a = np.asarray(host(a))
            except Exception as e:
                raise _lib.GcfrError("%s: %s must be integers (2,3) or (B,2,3): %s" % (what, name, e))
            if a.dtype.kind not in "iu":
                raise _lib.GcfrError("%s: %s of a pair must be integers (quantise_affine's), got %s" % (what, name, a.dtype))
            if a.shape not in ((2, 3), (B, 2, 3)):
                raise _lib.GcfrError("%s: %s must be (2,3) or (%d,2,3); got %s" % (what, name, B, a.shape))
            a = np.ascontiguousarray(np.broadcast_to(a.astype(np.int64), (B, 2, 3)))
            for b, m in enumerate(a):
                _check_affine_integers(m, what, name, b)
            pair.append(a)
        return tuple(pair)
    try:
        A = np.asarray(host(net_to_photo), dtype=np.float64)
    except Exception as e:
        raise _lib.GcfrError("%s: the map must be numbers (2,3) or (B,2,3): %s" % (what, e))
    if A.shape not in ((2, 3), (B, 2, 3)):
        raise _lib.GcfrError("%s: the map must be (2,3) or (%d,2,3) (network -> photograph); got %s" % (what, B, A.shape))
    Fq, Iq = quantise_affine(A)
    return tuple(np.ascontiguousarray(np.broadcast_to(a, (B, 2, 3))) for a in (Fq, Iq))


def ingest_affine_device(photo_u8, net_to_photo, size):
    """The network's input from a ROTATED face in each photograph, on the device: photo_u8 (B,Hp,Wp,3) uint8 of any size,
    `net_to_photo` the HOST map from the network's coordinates to the photograph's -- an f64 matrix (2,3) for every face or (B,2,3)
    (a list, a numpy array or a CPU tensor; `affine_from_rotated_box` builds one, a face aligner reports one), or the integer pair
    (F, I) of `quantise_affine`, taken unchanged -- and `size` the network's (h, w) (an int: square) -> (B,h,w,3) f32 in [0,1].
    Every network pixel samples the photograph bilinearly through the map at its centre, or at K x K sub-sample centres where a
    step of one network pixel crosses more than one photograph pixel (K = 2, 4, 8), all in integers with 14 fractional bits: one
    exact 64-bit sum, one f64 division, one rounding to f32 (include/gcfr.h states it; csrc/gcfr_fullres_affine.hip).  Taps beyond
    the photograph's edge replicate it, so a face may hang over the edge.  For the axis-aligned map of a box at 1, 2, 4 or 8 times
    the network's side these are `ingest_box_device`'s bits.  One launch per 32 faces, no host synchronisation; a malformed input
    raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    what = "ingest_affine_device"
    h, w = (size, size) if isinstance(size, int) else (tuple(size) if isinstance(size, (tuple, list)) and len(size) == 2 else (None, None))
    B, Hp, Wp, _ = _check_photographs(photo_u8, 1, what, boxed=True)
    if any(isinstance(n, bool) or not isinstance(n, int) or n < 1 for n in (h, w)) or h * w > 0x7fffffff:
        raise _lib.GcfrError("%s: the network's size (h, w) must be positive integers with h w < 2^31; got %r" % (what, (h, w)))
    Fq, _ = _affine_integers(net_to_photo, B, what)
    _lib.require_device(photo_u8)
    photo = photo_u8.detach().contiguous()
    x_lo = torch.empty((B, h, w, 3), dtype=torch.float32, device=photo.device)
    _lib.launch("gcfr_ingest_affine_u8", photo.device, photo, B, Hp, Wp, _host_pointer(Fq), h, w, x_lo, _lib.STREAM)
    return x_lo


def fullres_affine_composites_device(photo_u8, net_to_photo, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0, out=None):
    """`fullres_box_composites_device` for a ROTATED face: photo_u8 (B,Hp,Wp,3) uint8 of any size; `net_to_photo` as in
    `ingest_affine_device`; x_lo (B,h,w,3) f32, the network's input (`ingest_affine_device`); rendered (B,L,3,h,w) -> (B,L,Hp,Wp,3),
    or (B,3,h,w) -> (B,Hp,Wp,3); mask_u8 (1|B,h,w) or (h,w) uint8, the compositing mask at the network's resolution IN THE NETWORK'S
    FRAME.  A photograph pixel belongs to the face where its centre lands in the network square under the inverse map; there the
    relit image, x_lo and the mask are carried to it bilinearly through that map (K x K sub-samples averaged where the face is
    smaller than the network, K = 2, 4, 8; integer taps and weights, include/gcfr.h states every operation;
    csrc/gcfr_fullres_affine.hip), and the quotient / detail transfer of `fullres_composites_device` follows.  Every other pixel is
    the photograph's byte for every light: the entry always pastes, a rotated quad has no rectangular "box alone".  For the
    axis-aligned map of a box at 1, 2 or 4 times the network's side these are `fullres_box_composites_device(paste=True)`'s bytes,
    from this entry's own kernel: there is no dispatch between the two.  ONE launch per 32 faces for all L lights; the matrices
    travel in the launch's arguments, nothing is uploaded.  `rendered` is the only operand that may be non-f32 on entry.  `out`: a
    contiguous uint8 buffer of the result's shape that is written and returned; it must not overlap the photographs.  NOT
    DIFFERENTIABLE.  No host synchronisation; a malformed input raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    what = "fullres_affine_composites_device"
    _check_composite_tensors(what, x_lo, rendered, mask_u8, out)
    if x_lo.dim() != 4 or x_lo.shape[-1] != 3 or min(x_lo.shape) < 1:
        raise _lib.GcfrError("%s: x_lo must be (B,h,w,3); got %s" % (what, tuple(x_lo.shape)))
    h, w = int(x_lo.shape[1]), int(x_lo.shape[2])
    B, Hp, Wp, _ = _check_photographs(photo_u8, 1, what, boxed=True)
    _, Iq = _affine_integers(net_to_photo, B, what)
    photo, x, ren, m, L, shape = _composite_operands(what, photo_u8, x_lo, rendered, mask_u8, out, detail_clamp, floor, B, h, w, (Hp, Wp),
                                                     frame=", in the network's frame")
    if out is not None and out.data_ptr() < photo.data_ptr() + photo.numel() and photo.data_ptr() < out.data_ptr() + out.numel():
        raise _lib.GcfrError("%s: out must not overlap the photographs" % what)
    res = torch.empty(shape, dtype=torch.uint8, device=photo.device) if out is None else out
    _lib.launch("gcfr_fullres_composites_affine_u8", photo.device, photo, x, ren, m, m.shape[0], B, L, Hp, Wp, _host_pointer(Iq), h, w,
                float(floor), float(detail_clamp), res, _lib.STREAM)
    return res


def _faces_of_map(net_to_photo):
    """how many faces the map of an affine entry names by itself: B of a (B,2,3) matrix (or of the F of an integer pair), else 1"""
    import torch
    a = net_to_photo
    if isinstance(a, tuple) and len(a) == 2 and all(torch.is_tensor(x) or np.ndim(x) >= 2 for x in a):
        a = a[0]
    try:
        shape = tuple(a.shape) if torch.is_tensor(a) else np.shape(a)
    except Exception:
        shape = ()
    return int(shape[0]) if len(shape) == 3 and shape[0] >= 1 else 1


def ingest_group_affine_device(photo_u8, net_to_photo, photo_index, size):
    """`ingest_affine_device` for a GROUP PHOTOGRAPH: photo_u8 (P,Hp,Wp,3) uint8, B tilted faces with the host map `net_to_photo` --
    (B,2,3) f64 (or (2,3) for every face), or `quantise_affine`'s integer pair, as that entry takes it -- and host `photo_index` (B,)
    naming each face's photograph, as `ingest_group_device` takes it (any order; a photograph may have no face, one or many; None:
    every face in the one photograph, P == 1) -> (B,h,w,3) f32 in [0,1].  The bits are
    `ingest_affine_device(photo_u8[photo_index], net_to_photo, size)`'s, and the photographs are neither gathered nor copied
    (include/gcfr.h states it; csrc/gcfr_fullres_group_affine.hip).  One launch per 32 faces, no host synchronisation; a malformed
    input raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    what = "ingest_group_affine_device"
    h, w = (size, size) if isinstance(size, int) else (tuple(size) if isinstance(size, (tuple, list)) and len(size) == 2 else (None, None))
    pi = _check_photo_index(photo_index, photo_u8, what, faces=_faces_of_map(net_to_photo) if photo_index is None else None)
    B = int(pi.shape[0])
    P, Hp, Wp, _ = _check_photographs(photo_u8, 1, what, boxed=True)
    if any(isinstance(n, bool) or not isinstance(n, int) or n < 1 for n in (h, w)) or h * w > 0x7fffffff:
        raise _lib.GcfrError("%s: the network's size (h, w) must be positive integers with h w < 2^31; got %r" % (what, (h, w)))
    Fq, _ = _affine_integers(net_to_photo, B, what)
    _lib.require_device(photo_u8)
    photo = photo_u8.detach().contiguous()
    x_lo = torch.empty((B, h, w, 3), dtype=torch.float32, device=photo.device)
    _lib.launch("gcfr_ingest_group_affine_u8", photo.device, photo, P, Hp, Wp, _host_pointer(Fq), _host_pointer(pi), B, h, w, x_lo,
                _lib.STREAM)
    return x_lo


def fullres_group_affine_composites_device(photo_u8, net_to_photo, photo_index, x_lo, rendered, mask_u8, detail_clamp=4.0, floor=1.0,
                                           out=None):
    """EVERY TILTED face of a photograph relit in one pass over the photograph: photo_u8 (P,Hp,Wp,3) uint8; `net_to_photo` and
    `photo_index` as in `ingest_group_affine_device`; x_lo (B,h,w,3) f32, the network's input (`ingest_group_affine_device`); rendered
    (B,L,3,h,w) -> (P,L,Hp,Wp,3), or (B,3,h,w) -> (P,Hp,Wp,3); mask_u8 (1|B,h,w) or (h,w) uint8, per FACE and in the network's frame,
    exactly as `fullres_affine_composites_device` takes them.  Per photograph and light the result is the CHAIN of that entry's
    composite over the photograph's faces in ascending face index, byte for byte: the running image starts as the photograph; a face
    relights it where a pixel's centre lands in the network square under its map and its carried mask is positive, reading the
    running bytes where that entry reads the photograph's, and every step rounds to a byte (include/gcfr.h states it;
    csrc/gcfr_fullres_group_affine.hip).  Where at most one face relights a pixel the byte is that entry's; where two do, the second
    face's gain multiplies the first's result, so order matters there and nowhere else.  A photograph without faces comes back as it
    is for every light; all faces of a photograph share the light index.  With `photo_index = arange(B)` and P = B these are
    `fullres_affine_composites_device`'s bytes; with axis-aligned maps at 1, 2 or 4 times the network's side they are
    `fullres_group_composites_device`'s on the same boxes.  ONE launch per 32 faces, whole photographs per launch; a photograph with
    more than 32 faces is continued by further launches on the same stream.  `out`: a contiguous uint8 buffer of the result's shape
    that is written and returned; it must not overlap the photographs.  NOT DIFFERENTIABLE.  No host synchronisation; a malformed
    input raises GcfrError before anything is loaded or launched."""
    import torch
    from . import _lib
    what = "fullres_group_affine_composites_device"
    _check_composite_tensors(what, x_lo, rendered, mask_u8, out)
    if x_lo.dim() != 4 or x_lo.shape[-1] != 3 or min(x_lo.shape) < 1:
        raise _lib.GcfrError("%s: x_lo must be (B,h,w,3); got %s" % (what, tuple(x_lo.shape)))
    B, h, w = int(x_lo.shape[0]), int(x_lo.shape[1]), int(x_lo.shape[2])
    pi = _check_photo_index(photo_index, photo_u8, what, faces=B)
    P, Hp, Wp, _ = photo_u8.shape
    _, Iq = _affine_integers(net_to_photo, B, what)
    # (a photograph that is not contiguous is copied below and cannot overlap anything; where the tensors live is the last check)
    if (out is not None and photo_u8.is_contiguous() and out.data_ptr() < photo_u8.data_ptr() + photo_u8.numel()
            and photo_u8.data_ptr() < out.data_ptr() + out.numel()):
        raise _lib.GcfrError("%s: out must not overlap the photographs" % what)
    photo, x, ren, m, L, shape = _composite_operands(what, photo_u8, x_lo, rendered, mask_u8, out, detail_clamp, floor, B, h, w, (Hp, Wp),
                                                     frame=", in the network's frame", images=P)
    res = torch.empty(shape, dtype=torch.uint8, device=photo.device) if out is None else out
    _lib.launch("gcfr_fullres_composites_group_affine_u8", photo.device, photo, x, ren, m, m.shape[0], P, B, L, Hp, Wp, _host_pointer(Iq),
                _host_pointer(pi), h, w, float(floor), float(detail_clamp), res, _lib.STREAM)
    return res


# ------------------------------------------------------------------------------------------------
# on-disk formats of load_data() (T8:527-558)
# ------------------------------------------------------------------------------------------------
def load_depth_mat(path: str) -> np.ndarray:
    """`.mat` with key 'depth_img' -> (256,256,1) float64 (T8:545)."""
    import scipy.io
    d = scipy.io.loadmat(path)["depth_img"]
    return np.reshape(np.asarray(d, dtype=np.float64), (d.shape[0], d.shape[1], 1))


def load_lighting_mat(path: str, ambient: float = 0.5) -> np.ndarray:
    """`.mat` with key 'lighting_direction' -> [ambient, lx, ly, lz] (T8:542, 549: ambient target fixed at 0.5)."""
    import scipy.io
    l = np.asarray(scipy.io.loadmat(path)["lighting_direction"], dtype=np.float64).reshape(3)
    return np.concatenate([[ambient], l])


def fill_nose_and_mouth_mask(face_mask_u8: np.ndarray, depth_mask_u8: np.ndarray) -> np.ndarray:
    """T8:552-556: element-wise max of the two masks, then > 128 -> 255, else 0.  Returns float64 (H,W,1)."""
    t = np.maximum(np.asarray(face_mask_u8, dtype=np.float64), np.asarray(depth_mask_u8, dtype=np.float64))
    t = np.where(t > 128, 255.0, 0.0)
    return t.reshape(t.shape[0], t.shape[1], 1)
