"""Host: `_lib.launch`, the one way the package calls a kernel entry, and the checks in front of the two image entries that had none.

No GPU: the library loads on the CPU (as tests/test_abi.py does), every refusal here happens before an entry is reached, and the
entry under test is replaced by a function that fails the test if it is called."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "geomconsistentfr_amd")

# entries that run on the host and take no stream: called directly, not through launch
HOST_ONLY = {"gcfr_version", "gcfr_abi_version", "gcfr_sample_table", "gcfr_options_default", "gcfr_shadow_workspace_bytes",
             "gcfr_masked_metrics_workspace_bytes", "gcfr_image_losses_workspace_bytes", "gcfr_supervised_losses_workspace_bytes",
             "gcfr_light_fit_workspace_bytes"}


def _reached(*a, **k):
    raise AssertionError("a refused call reached the entry")


def test_launch_refuses_a_wrong_argument_count_and_host_tensors_before_the_entry_is_called(monkeypatch):
    from geomconsistentfr_amd import _lib
    name = "gcfr_light_rig_fwd"
    monkeypatch.setattr(_lib.load(), name, _reached)
    B, L, H, W = 2, 3, 4, 5
    z = lambda *s, **k: torch.zeros(*s, device=k.get("device", "cpu"))
    final, albedo, rgb, rendered, shading = z(B, L, H, W), z(B, 3, H, W), z(1, L, 3), z(B, 3, H, W), z(B, 3, H, W)
    good = (final, albedo, rgb, 1, B, L, H, W, rendered, shading, _lib.STREAM)
    assert len(good) == len(_lib._SIGNATURES[name][1])
    with pytest.raises(_lib.GcfrError, match=name + " takes 11 arguments"):
        _lib.launch(name, "cuda:0", *good, None)                                   # one too many: ctypes would pass it through
    with pytest.raises(_lib.GcfrError, match=name + " takes 11 arguments"):
        _lib.launch(name, "cuda:0", *good[:-1])                                    # one too few
    with pytest.raises(_lib.GcfrError, match="no CPU path") as e:
        _lib.launch(name, "cuda:0", *good)                                         # host tensors
    assert name in str(e.value)
    meta = (z(B, L, H, W, device="meta"),) + good[1:]
    with pytest.raises(_lib.GcfrError, match="no CPU path") as e:
        _lib.launch(name, "cuda:0", *meta)
    assert name in str(e.value)


def _calls_launch(node):
    f = node.func
    return (isinstance(f, ast.Name) and f.id == "launch") or (isinstance(f, ast.Attribute) and f.attr == "launch")


def test_every_kernel_entry_is_named_only_as_an_argument_of_launch_or_inside_forward():
    """what keeps the next feature from adding a hand-written launch site: in geomconsistentfr_amd/*.py an entry that takes a
    stream appears only as the first argument of `launch(...)`, or inside block._Forward (which binds its argument lists once);
    the binding module's own table of signatures is the one other place the names are written"""
    from geomconsistentfr_amd import _lib
    entries = set(_lib._SIGNATURES) - HOST_ONLY
    assert HOST_ONLY <= set(_lib._SIGNATURES)
    launched = set()
    for path in sorted(glob.glob(os.path.join(PACKAGE, "*.py"))):
        module = os.path.basename(path)
        tree = ast.parse(open(path).read())
        inside_forward, first_args = set(), set()
        for node in ast.walk(tree):
            if isinstance(node, ast.ClassDef) and node.name == "_Forward":
                inside_forward = {id(n) for n in ast.walk(node)}
            if isinstance(node, ast.Call) and _calls_launch(node) and module != "_lib.py":
                first = node.args[0] if node.args else None
                assert isinstance(first, ast.Constant) and first.value in _lib._SIGNATURES, \
                    "%s:%d: launch's entry must be a literal name of the ABI" % (module, node.lineno)
                assert first.value not in HOST_ONLY, "%s:%d: %s takes no stream" % (module, node.lineno, first.value)
                first_args.add(id(first))
                launched.add(first.value)
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and node.attr in entries:
                assert id(node) in inside_forward, "%s:%d: %s called by hand" % (module, node.lineno, node.attr)
                launched.add(node.attr)
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value in entries and module != "_lib.py":
                assert id(node) in first_args or id(node) in inside_forward, "%s:%d: %s named outside launch" % (module, node.lineno, node.value)
    # (gcfr_copy_probe is bench.py's and the tools'; the package launches every other entry)
    assert launched == entries - {"gcfr_copy_probe"}, sorted(entries - launched)


def _no_launch(monkeypatch):
    from geomconsistentfr_amd import _lib
    monkeypatch.setattr(_lib, "launch", _reached)
    monkeypatch.setattr(_lib, "load", _reached)


def test_inference_images_device_refuses_malformed_inputs_before_any_launch(monkeypatch):
    """a plane of the wrong rank used to be an out-of-bounds device read (the kernel indexes the per-light planes at (b L + l) H W)"""
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd.postprocess import inference_images_device
    _no_launch(monkeypatch)
    B, L, H, W = 2, 3, 4, 5
    z = lambda *s, **k: torch.zeros(*s, dtype=k.get("dtype", torch.float32), device=k.get("device", "cpu"))
    x, many, one, mask = z(B, H, W, 3), z(B, L, 3, H, W), z(B, 3, H, W), z(H, W, dtype=torch.uint8)
    bad = {
        "a (B,H,W) shadow plane beside a (B,L,3,H,W) rendered": dict(rendered=many, shadow_mask_weights=z(B, H, W)),
        "a (B,H,W) shading plane beside a (B,L,3,H,W) rendered": dict(rendered=many, final_shading=z(B, H, W)),
        "a (B,L,H,W) shading plane beside a (B,3,H,W) rendered": dict(rendered=one, final_shading=z(B, L, H, W)),
        "a shading plane of L + 1 lights": dict(rendered=many, final_shading=z(B, L + 1, H, W)),
        "albedo with an L axis": dict(rendered=many, albedo=z(B, L, 3, H, W)),
        "normals with an L axis": dict(rendered=many, surface_normals=z(B, L, 3, H, W)),
        "albedo of another size": dict(rendered=one, albedo=z(B, 3, H, W + 1)),
        "depth with an L axis": dict(rendered=many, depth=z(B, L, H, W)),
        "depth of another batch": dict(rendered=one, depth=z(B + 1, 1, H, W)),
        "rendered of another size": dict(rendered=z(B, 3, H, W + 1)),
        "rendered without channels": dict(rendered=z(B, H, W)),
        "rendered with four channels": dict(rendered=z(B, L, 4, H, W)),
        "images planar": dict(input_images=z(B, 3, H, W), rendered=one),
        "images without the batch axis": dict(input_images=z(H, W, 3), rendered=one),
        "mask of another size": dict(rendered=one, mask_u8=z(H, W + 1, dtype=torch.uint8)),
        "mask of another batch": dict(rendered=one, mask_u8=z(B + 1, H, W, dtype=torch.uint8)),
        "mask with a channel axis": dict(rendered=one, mask_u8=z(B, H, W, 1, dtype=torch.uint8)),
        "f32 mask": dict(rendered=one, mask_u8=z(H, W)),
        "integer rendered": dict(rendered=z(B, 3, H, W, dtype=torch.int32)),
        "integer shading plane": dict(rendered=one, final_shading=z(B, H, W, dtype=torch.int64)),
        "mixed devices": dict(rendered=one, albedo=z(B, 3, H, W, device="meta")),
        "rendered not a tensor": dict(rendered=np.zeros((B, 3, H, W), np.float32)),
        "mask not a tensor": dict(rendered=one, mask_u8=np.zeros((H, W), np.uint8)),
        "albedo not a tensor": dict(rendered=one, albedo=np.zeros((B, 3, H, W), np.float32)),
    }
    for why, kw in bad.items():
        args = dict(input_images=x, mask_u8=mask)
        args.update(kw)
        with pytest.raises(_lib.GcfrError) as e:
            inference_images_device(**args)
        assert "no CPU path" not in str(e.value), (why, str(e.value))              # refused for its shape, not for where it lives
    # well-formed but on the host, every optional plane given: refused last, still before the launch
    for rendered, lead in ((one, (B,)), (many, (B, L))):
        with pytest.raises(_lib.GcfrError, match="no CPU path"):
            inference_images_device(x, rendered, z(B, H, W, dtype=torch.uint8), albedo=z(B, 3, H, W), depth=z(B, H, W),
                                    shadow_mask_weights=z(*lead, H, W), final_shading=z(*lead, H, W, dtype=torch.float64),
                                    surface_normals=z(B, 3, H, W))


def test_fix_border_artifacts_device_refuses_malformed_inputs_before_any_launch(monkeypatch):
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd.postprocess import fix_border_artifacts_device
    _no_launch(monkeypatch)
    B, H, W = 2, 4, 5
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    img, mask = u8(B, H, W, 3), u8(H, W)
    bad = {
        "f32 images": (img.float(), mask),
        "images with four channels": (u8(B, H, W, 4), mask),
        "images planar": (u8(B, 3, H, W), mask),
        "one image without the batch axis": (u8(H, W, 3), mask),
        "mask of another size": (img, u8(H, W + 1)),
        "mask of another batch": (img, u8(B + 1, H, W)),
        "mask with a channel axis": (img, u8(B, H, W, 1)),
        "f32 mask": (img, mask.float()),
        "images not a tensor": (img.numpy(), mask),
        "mask not a tensor": (img, mask.numpy()),
    }
    for why, args in bad.items():
        with pytest.raises(_lib.GcfrError) as e:
            fix_border_artifacts_device(*args)
        assert "no CPU path" not in str(e.value), (why, str(e.value))
    for m in (mask, u8(1, H, W), u8(B, H, W)):
        with pytest.raises(_lib.GcfrError, match="no CPU path"):
            fix_border_artifacts_device(img, m)
