"""ctypes binding of libgcfr_hip.so (C ABI: include/gcfr.h).

There is NO fallback: if the HIP library is missing or a call fails, this module raises.  torch is
imported first on purpose -- it loads its bundled libamdhip64.so (SONAME libamdhip64.so.7), and the
dynamic loader then binds libgcfr_hip.so's DT_NEEDED libamdhip64.so.7 to that same, already loaded
runtime, so device pointers and streams are shared between torch and the kernels.
"""
import ctypes
import os

import torch  # (must be loaded before libgcfr_hip.so, see above)

from . import build as _build

_LIB = None

GCFR_OK = 0
ABI_VERSION = 6      # include/gcfr.h GCFR_ABI_VERSION this binding was written against
_ERRORS = {-1: "GCFR_ERR_INVALID_ARGUMENT", -2: "GCFR_ERR_LAUNCH"}

_p, _i, _f, _d = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_double

N_COUNTERS = 28      # GCFR_N_COUNTERS
COUNTER_NAMES = ("tiles", "groups_nominal", "groups_visited", "bound_tests", "bodies", "lane_samples", "early_exits",
                 "tie_remarches", "samples_in_range", "bounds_given_up", "visits_after_last_body", "visits_before_first_body",
                 "trail_enter", "trail_skips", "trail_leave", "rough_samples", "wave_samples", "wave_samples_taken", "lane_takes",
                 # the audit build (-DGCFR_AUDIT, csrc/gcfr_march.hpp): claims checked / contradicted; audit_max_use is a maximum (1/1000 of Kerr)
                 "audit_bound_checks", "audit_bound_violations", "audit_term_checks", "audit_term_violations",
                 "audit_masked_checks", "audit_masked_violations", "audit_safe_violations", "audit_max_use")


class Options(ctypes.Structure):
    """include/gcfr.h `gcfr_options`: per-call knobs and hooks of the forward entry points (none changes a result bit
    except `pixels`, see the header).  Build one with `options(...)`; pass it as `options=` to the block functions /
    RenderFwdPlan."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("tile_w", _i), ("group", _i), ("ksplit", _i),
                ("depth_bound_skip", _i), ("lds_stage", _i),
                ("event_start", _p), ("event_stop", _p), ("counters", _p), ("pixels", _i), ("phase", _i)]


def options(tile_w=0, group=0, ksplit=-1, depth_bound_skip=-1, event_start=None,
            event_stop=None, counters=None, lds_stage=-1, pixels=0, phase=0) -> Options:
    o = Options()
    load().gcfr_options_default(ctypes.byref(o))
    o.tile_w, o.group, o.ksplit, o.depth_bound_skip = tile_w, group, ksplit, depth_bound_skip
    o.lds_stage = lds_stage
    o.event_start, o.event_stop, o.counters = event_start, event_stop, counters
    o.pixels = pixels
    o.phase = phase
    return o


def _with(o, field: str, value: int) -> Options:
    """a copy of `o` (or the defaults) with one field set"""
    n = Options()
    if o is None:
        load().gcfr_options_default(ctypes.byref(n))
    else:
        ctypes.memmove(ctypes.byref(n), ctypes.byref(o), ctypes.sizeof(Options))
    setattr(n, field, value)
    return n


def with_phase(o, phase: int) -> Options:
    """a copy of `o` (or the defaults) with `phase` set: 1 = the prepass only, 2 = the march only (include/gcfr.h)"""
    return _with(o, "phase", phase)


def with_pixels(o, pixels: int) -> Options:
    """a copy of `o` (or the defaults) with `pixels` set -- RenderParams(pixels="mask") reaches the library this way"""
    return _with(o, "pixels", pixels)


def opt_ref(o):
    """ctypes argument for a `const gcfr_options *` parameter (None = library defaults)."""
    return ctypes.byref(o) if o is not None else None


_SIGNATURES = {
    "gcfr_version": (ctypes.c_char_p, []),
    "gcfr_abi_version": (_i, []),
    "gcfr_sample_table": (_i, [_d, _d, _i, _p]),
    "gcfr_light_prep": (_i, [_p, _i, _i, _f, _f, _p, _p, _p]),
    "gcfr_shadow_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "gcfr_options_default": (None, [_p]),
    "gcfr_render_from_depth_fwd": (_i, [_p, _i, _f, _f, _p, _p, _i, _d, _d, _d, _d, _f, _i, _p, _p, _i, _i, _i, _i, _i, _p,
                                        _f, _p, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, ctypes.c_size_t, _p, _p]),
    "gcfr_normals_fwd": (_i, [_p, _i, _i, _i, _d, _d, _d, _d, _f, _i, _p, _p]),
    "gcfr_normals_bwd": (_i, [_p, _p, _i, _i, _i, _d, _d, _d, _d, _f, _i, _p, _p]),
    "gcfr_render_fwd": (_i, [_p, _i, _f, _f, _p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p, _f, _p, _f,
                             _p, _p, _p, _p, _p, _p, _p, _p, _p, ctypes.c_size_t, _p, _p]),
    "gcfr_shadow_fwd": (_i, [_p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _f, _p, _p, _p, _p, ctypes.c_size_t, _p, _p]),
    "gcfr_shade_fwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p]),
    "gcfr_shadow_bwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "gcfr_shade_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "gcfr_render_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _d, _d, _d, _d, _f, _i, _f, _p, _p, _p, _p, _p,
                             _p, _p, _p, _p, _p]),
    "gcfr_light_prep_bwd": (_i, [_p, _i, _i, _f, _f, _p, _p, _p, _p]),
    "gcfr_inference_images_u8": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p]),
    "gcfr_fix_border_u8": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "gcfr_assemble_batch_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p]),
    "gcfr_masked_metrics_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "gcfr_masked_metrics_u8": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p, ctypes.c_size_t, _p]),
    "gcfr_image_losses_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "gcfr_image_losses_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _d, _p, _p, _p, _p, ctypes.c_size_t, _p]),
    "gcfr_image_losses_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _d, _p, _p, _p, _p, _p]),
    "gcfr_supervised_losses_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "gcfr_supervised_losses_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, ctypes.c_int64, _i, _i, _i, _p, _p, _p, ctypes.c_size_t, _p]),
    "gcfr_supervised_losses_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, ctypes.c_int64, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p,
                                        _p, _p, _p, _p]),
    "gcfr_light_rig_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p]),
    "gcfr_light_rig_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "gcfr_light_rig_frames_u8": (_i, [_p, _p, _p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    "gcfr_ingest_photographs_u8": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "gcfr_fullres_composites_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _p, _p]),
    "gcfr_fullres_composites_guided_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _f, _p, _p]),
    "gcfr_ingest_box_u8": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p]),
    "gcfr_fullres_composites_box_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _f, _f, _p, _p]),
    "gcfr_fullres_composites_box_guided_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _f, _f, _f, _p, _p]),
    "gcfr_ingest_anybox_u8": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p]),
    "gcfr_fullres_composites_anybox_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _f, _f, _p, _p]),
    "gcfr_ingest_group_u8": (_i, [_p, _i, _i, _i, _p, _p, _i, _i, _i, _p, _p]),
    "gcfr_fullres_composites_group_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _i, _f, _f, _p, _p]),
    "gcfr_ingest_affine_u8": (_i, [_p, _i, _i, _i, _p, _i, _i, _p, _p]),
    "gcfr_fullres_composites_affine_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _i, _f, _f, _p, _p]),
    "gcfr_ingest_group_affine_u8": (_i, [_p, _i, _i, _i, _p, _p, _i, _i, _i, _p, _p]),
    "gcfr_fullres_composites_group_affine_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _i, _f, _f, _p, _p]),
    "gcfr_environment_cells": (_i, [_p, _p, _p, _i, _i, _i, _f, _p, _p]),
    "gcfr_environment_fwd": (_i, [_p, _i, _i, _i, _p, _p, _i, _p, _p]),
    "gcfr_environment_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "gcfr_environment_cells_frames": (_i, [_p, _p, _p, _i, _i, _i, _i, _f, _p, _p]),
    "gcfr_environment_fwd_frames": (_i, [_p, _i, _i, _i, _p, _p, _i, _i, _p, _p]),
    "gcfr_light_fit_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "gcfr_light_fit_normal": (_i, [_p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "gcfr_light_fit_solve": (_i, [_p, _p, _i, _i, _d, _i, _p, _p, _p]),
    "gcfr_light_fit_solve_nonneg": (_i, [_p, _p, _i, _i, _d, _i, _i, _p, _p, _p, _p]),
    "gcfr_copy_probe": (_i, [_p, _p, ctypes.c_size_t, _p]),
}


class GcfrError(RuntimeError):
    pass


def lib_path() -> str:
    return _build.LIB_PATH


def load():
    """Load and type the library.  Without an override the in-tree library is (re)built first whenever it is
    missing or older than a source under csrc/ or include/gcfr.h and hipcc is available; a stale library on a
    host without hipcc (the GPU box ships the prebuilt .so) is loaded as it is.  `GCFR_HIP_LIB` selects another
    build of the same ABI (tools/ab.sh); a missing override is an error, never a silent fall-back."""
    global _LIB
    if _LIB is not None:
        return _LIB
    override = os.environ.get("GCFR_HIP_LIB")
    if override:
        if not os.path.exists(override):
            raise GcfrError("GCFR_HIP_LIB=%s does not exist" % override)
        path = override
    else:
        path = _build.LIB_PATH
        if _build.needs_build():
            try:
                _build.build()
            except Exception as e:  # no hipcc on this host
                if not os.path.exists(path):
                    raise GcfrError("libgcfr_hip.so is not built (%s) and there is no CPU fallback: run "
                                    "`python -c 'import __graft_entry__ as g; g.build()'`" % e)
                import warnings
                warnings.warn("libgcfr_hip.so is older than its sources and could not be rebuilt (%s): loading the stale "
                              "library (its ABI revision is checked below)" % e, RuntimeWarning)
    L = ctypes.CDLL(path)
    # ABI revision first: a stale library exports every symbol by name, and would be called with shifted arguments
    try:
        L.gcfr_abi_version.restype = _i
        L.gcfr_abi_version.argtypes = []
        have = int(L.gcfr_abi_version())
    except AttributeError:
        have = None
    if have != ABI_VERSION:
        raise GcfrError("%s implements ABI revision %s, this binding needs %d (include/gcfr.h GCFR_ABI_VERSION): rebuild "
                        "with `python -c 'import __graft_entry__ as g; g.build()'`" % (path, have, ABI_VERSION))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError here = the library does not export the declared ABI
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def exported_symbols():
    return sorted(_SIGNATURES)


def check(status: int, what: str):
    if status != GCFR_OK:
        raise GcfrError("%s failed: %s (%d)" % (what, _ERRORS.get(status, "unknown"), status))


NO_CPU_PATH = "geomconsistentfr_amd has no CPU path: tensors must be on a ROCm device"


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise GcfrError(NO_CPU_PATH)


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    """a tensor's device address for a pointer parameter; None stays None (NULL: the optional input or output is absent)"""
    return None if t is None else t.data_ptr()


def f32c(t):
    """a tensor (an input, an upstream gradient) as the kernels read it: detached, f32, contiguous; None stays None"""
    return None if t is None else t.detach().to(torch.float32).contiguous()


STREAM = object()      # stands at the stream parameter's position in `launch`'s arguments


def launch(name: str, device, *args):
    """THE way a kernel entry is called: `args` in the order of the prototype in include/gcfr.h, with `STREAM` where the stream goes.
    A tensor is passed as its address after it has been found on `device` (a ROCm device) and contiguous; None is NULL; ints,
    floats, ctypes objects and computed addresses go through as given.  The call runs with `device` current, on its current
    stream, and a status other than GCFR_OK raises.  Every refusal is a GcfrError naming the entry, before the entry is called:
    the entries are cdecl, so ctypes itself would pass a list that is too long."""
    want = _SIGNATURES[name][1]
    if len(args) != len(want):
        raise GcfrError("%s takes %d arguments (include/gcfr.h), got %d" % (name, len(want), len(args)))
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    call, at = list(args), None
    for i, a in enumerate(args):
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise GcfrError("%s, argument %d: %s" % (name, i, NO_CPU_PATH))
            if a.device != device:
                raise GcfrError("%s, argument %d: a tensor on %s in a launch on %s" % (name, i, a.device, device))
            if not a.is_contiguous():
                raise GcfrError("%s, argument %d: a tensor %s with strides %s is not contiguous"
                                % (name, i, tuple(a.shape), tuple(a.stride())))
            call[i] = a.data_ptr()
        elif a is STREAM:
            at = i
    fn = getattr(load(), name)
    with torch.cuda.device(device):
        if at is not None:
            call[at] = torch.cuda.current_stream(device).cuda_stream
        check(fn(*call), name)


# ----------------------------------------------------------------------------------------------------------------------------
# what the Python entries check BEFORE anything is loaded or launched, so that a mismatch never reaches a kernel
# ----------------------------------------------------------------------------------------------------------------------------
FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def check_tensors(what: str, named, one_device: bool = True, **dtypes):
    """the (name, value) pairs of `named` are tensors -- f32, or `name=dtype` / `name=(dtype, ...)` -- and, with `one_device`, all
    on the first one's device.  A value of None is an absent optional and is skipped.  Returns the tensors that are present."""
    named = [(n, t) for n, t in named if t is not None]
    for n, t in named:
        if not torch.is_tensor(t):
            raise GcfrError("%s: %s must be a tensor, got %s" % (what, n, type(t).__name__))
    for n, t in named:
        want = dtypes.get(n, torch.float32)
        if t.dtype not in (want if isinstance(want, tuple) else (want,)):
            names = " or ".join(str(d).replace("torch.", "") for d in (want if isinstance(want, tuple) else (want,)))
            raise GcfrError("%s: %s must be %s, got %s" % (what, n, names, t.dtype))
    if one_device and any(t.device != named[0][1].device for _, t in named):
        raise GcfrError("%s: tensors on one device; got %s" % (what, ", ".join("%s on %s" % (n, t.device) for n, t in named)))
    return [t for _, t in named]


def check_shape(name: str, t, *shapes, why: str = ""):
    """the shape of tensor `t` is one of `shapes`"""
    if tuple(t.shape) not in shapes:
        raise GcfrError("%s must be %s%s; got %s" % (name, " or ".join(str(tuple(s)).replace(" ", "") for s in shapes), why, tuple(t.shape)))


def check_out(out, shape):
    """`out` (None: absent) is a buffer the result can be written into: contiguous, of `shape`, and does not require a gradient
    (its dtype and device are `check_tensors`')"""
    if out is None:
        return
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise GcfrError("out must be a contiguous %s tensor; got %s with strides %s" % (tuple(shape), tuple(out.shape), tuple(out.stride())))
    if out.requires_grad:
        raise GcfrError("out must not require a gradient: it is a buffer the result is written into")
