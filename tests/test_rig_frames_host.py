"""CPU: the rig-frames feature's host side (lighting.rig_frames_u8 / environment_lights_frames; csrc/gcfr_rig_frames.hip and the
frame forms of csrc/gcfr_environment.hip) without a GPU.

1. tests/rig_frames_emulation.py: F frames at once equal F single-frame statements written out here from the three functions it
   composes, for shared and per-face rigs and masks and both mask dtypes.
2. rig_frames_u8 and environment_lights_frames refuse host tensors and each malformed input before anything is launched (the
   launchers are monkeypatched to fail if reached); the C entries refuse NULL pointers and bad shapes on the host.
3. the binding's argument lists have the arity of the header's prototypes; lighting.RIG_FRAMES_TILE is the kernel's kFrameTile.
4. every kernel of the feature in the built library is free of scratch."""
import os
import re

import numpy as np
import pytest
import torch

import light_rig_emulation as rig
import rig_frames_emulation as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("gcfr_light_rig_frames_u8", "gcfr_environment_cells_frames", "gcfr_environment_fwd_frames")


def _case(seed, B, L, F, H, W, shared_rig, shared_mask):
    rng = np.random.default_rng(seed)
    final = (1.2 * rng.random((B, L, H, W))).astype(np.float32)
    albedo = (0.1 + 0.8 * rng.random((B, 3, H, W))).astype(np.float32)
    images = rng.random((B, H, W, 3), dtype=np.float32)
    mask = rng.choice(np.array([0, 1, 128, 255], np.uint8), size=(1 if shared_mask else B, H, W))
    rgb = (rng.standard_normal((1 if shared_rig else B, F, L, 3)) * 0.6).astype(np.float32)
    return final, albedo, images, mask, rgb


@pytest.mark.parametrize("mask_f32", [False, True])
@pytest.mark.parametrize("B,L,F,H,W,shared_rig,shared_mask", [(1, 1, 1, 1, 1, True, True), (2, 5, 3, 5, 7, False, True),
                                                              (3, 4, 6, 4, 4, True, False)])
def test_the_emulation_of_f_frames_is_f_single_frames(B, L, F, H, W, shared_rig, shared_mask, mask_f32):
    final, albedo, images, mask, rgb = _case(B + L + F, B, L, F, H, W, shared_rig, shared_mask)
    got = emu.frames(final, albedo, images, mask, rgb, mask_f32)
    assert got.shape == (B, F, H, W, 3) and got.dtype == np.uint8
    m = mask.astype(np.float32) / np.float32(255.0) if mask_f32 else mask.astype(np.float64) / 255.0
    for f in range(F):
        rendered, _ = rig.forward(final, albedo, np.ascontiguousarray(rgb[:, f]))
        for b in range(B):
            one = emu.pps.to_uint8(emu.pps.composite_into_input(images[b], rendered[b], m[0 if shared_mask else b].astype(np.float64)))
            np.testing.assert_array_equal(got[b, f], one)
        np.testing.assert_array_equal(got[:, f], emu.frame(final, albedo, images, mask, np.ascontiguousarray(rgb[:, f]), mask_f32))
    assert len(np.unique(got)) > 2 or got.size <= 3
    # where the mask is 0 the photograph is kept, whatever the rig
    keep = np.broadcast_to(mask[:, None, :, :, None] == 0, got.shape)
    want = np.broadcast_to(emu.pps.to_uint8(images.astype(np.float64) * 255.0)[:, None], got.shape)
    np.testing.assert_array_equal(got[keep], want[keep])


def _host(B=2, L=3, F=2, H=4, W=6):
    final, albedo, images, mask, rgb = _case(1, B, L, F, H, W, False, False)
    return [torch.from_numpy(a) for a in (final, albedo, images, mask, rgb)]


def _no_launch(monkeypatch):
    from geomconsistentfr_amd import _lib

    def fail(*a, **k):
        raise AssertionError("the library was loaded: a malformed input must be refused before that")
    monkeypatch.setattr(_lib, "load", fail)


def test_rig_frames_u8_refuses_host_tensors_and_malformed_inputs(monkeypatch):
    from geomconsistentfr_amd import rig_frames_u8
    from geomconsistentfr_amd._lib import GcfrError
    _no_launch(monkeypatch)
    final, albedo, images, mask, rgb = _host()
    with pytest.raises(GcfrError, match="no CPU path"):
        rig_frames_u8(final, albedo, images, mask, rgb)
    with pytest.raises(GcfrError, match="no CPU path"):
        rig_frames_u8(final, albedo, images, mask[0], rgb[0])                       # (H,W) mask, (F,L,3) rigs: well-formed, on the host
    bad = [
        ("wrong L between final and rig", dict(light_rgb_frames=rgb[:, :, :2])),
        ("RB not in {1,B}", dict(light_rgb_frames=torch.cat([rgb, rgb[:1]]))),
        ("mask not u8", dict(mask_u8=mask.to(torch.float32))),
        ("F = 0", dict(light_rgb_frames=rgb[:, :0])),
        ("rig rank", dict(light_rgb_frames=rgb[0, 0])),
        ("rig last axis", dict(light_rgb_frames=rgb[..., :2])),
        ("final rank", dict(final_shading=final[0])),
        ("final f64", dict(final_shading=final.double())),
        ("albedo shape", dict(albedo=albedo[:, :2])),
        ("images layout", dict(images=images.permute(0, 3, 1, 2))),
        ("images f64", dict(images=images.double())),
        ("mask batch", dict(mask_u8=torch.cat([mask, mask[:1]]))),
        ("mask size", dict(mask_u8=mask[:, :, :5])),
        ("rig f64", dict(light_rgb_frames=rgb.double())),
        ("out shape", dict(out=torch.empty(2, 2, 4, 6, 4, dtype=torch.uint8))),
        ("out dtype", dict(out=torch.empty(2, 2, 4, 6, 3, dtype=torch.float32))),
        ("out strided", dict(out=torch.empty(2, 2, 4, 6, 6, dtype=torch.uint8)[..., ::2])),
        ("not a tensor", dict(albedo=albedo.numpy())),
    ]
    for label, kw in bad:
        args = dict(final_shading=final, albedo=albedo, images=images, mask_u8=mask, light_rgb_frames=rgb)
        args.update(kw)
        with pytest.raises(GcfrError) as e:
            rig_frames_u8(**args)
        assert "no CPU path" not in str(e.value), (label, str(e.value))            # refused for its shape, not for where it lives
    too_many = torch.zeros(1, 4097, 3, 3)
    with pytest.raises(GcfrError, match="4096"):
        rig_frames_u8(final, albedo, images, mask, too_many)


def test_environment_lights_frames_refuses_host_tensors_and_malformed_inputs(monkeypatch):
    from geomconsistentfr_amd import environment_lights_frames
    from geomconsistentfr_amd._lib import GcfrError
    _no_launch(monkeypatch)
    env, dirs, rots = torch.rand(1, 4, 8, 3), torch.rand(5, 3), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(GcfrError, match="no CPU path"):
        environment_lights_frames(env, dirs, rots)
    bad = [
        ("F = 0", dict(rotations=rots[:0])),
        ("one rotation, no frame axis", dict(rotations=rots[0])),
        ("rotations (F,3,2)", dict(rotations=rots[:, :, :2])),
        ("rotations f64", dict(rotations=rots.double())),
        ("rotations not a tensor", dict(rotations=rots.numpy())),
        ("env rank", dict(env=env[0])),
        ("env f64", dict(env=env.double())),
        ("directions (L,2)", dict(directions=dirs[:, :2])),
        ("out of the single call's shape", dict(out=torch.empty(1, 5, 3))),
        ("out (E,L,F,3)", dict(out=torch.empty(1, 5, 2, 3))),
    ]
    for label, kw in bad:
        args = dict(env=env, directions=dirs, rotations=rots)
        args.update(kw)
        with pytest.raises(GcfrError) as e:
            environment_lights_frames(**args)
        assert "no CPU path" not in str(e.value), (label, str(e.value))
    with pytest.raises(GcfrError, match="4096"):
        environment_lights_frames(env, dirs, torch.eye(3).repeat(4097, 1, 1))


def test_the_c_entries_refuse_null_pointers_and_bad_shapes_without_a_gpu():
    import ctypes
    from geomconsistentfr_amd import _lib
    L_ = _lib.load()
    p = ctypes.c_void_p(64)
    ok = dict(final=p, albedo=p, x=p, mask=p, mb=1, mf=0, rgb=p, rb=1, B=2, L=3, F=4, H=5, W=6, frames=p)
    order = ("final", "albedo", "x", "mask", "mb", "mf", "rgb", "rb", "B", "L", "F", "H", "W", "frames")
    call = lambda **kw: L_.gcfr_light_rig_frames_u8(*[dict(ok, **kw)[k] for k in order], None)
    for k in ("final", "albedo", "x", "mask", "rgb", "frames"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(mb=3), dict(rb=3), dict(mf=2), dict(B=0), dict(L=0), dict(L=4097), dict(F=0), dict(F=4097), dict(H=0), dict(W=0),
               dict(H=65536, W=65536), dict(B=1 << 22, mb=1, H=1024, W=1024)):
        assert call(**kw) == -1, kw
    cells = lambda rows=p, cols=p, dirs=p, F=2, He=4, We=8, L=3, out=p: L_.gcfr_environment_cells_frames(rows, cols, dirs, F, He, We, L, -2.0, out, None)
    fwd = lambda env=p, E=1, He=4, We=8, w=p, cell=p, F=2, L=3, out=p: L_.gcfr_environment_fwd_frames(env, E, He, We, w, cell, F, L, out, None)
    for k in ("rows", "cols", "dirs", "out"):
        assert cells(**{k: None}) == -1, k
    for k in ("env", "w", "cell", "out"):
        assert fwd(**{k: None}) == -1, k
    for kw in (dict(F=0), dict(F=4097), dict(He=0), dict(We=0), dict(L=0), dict(L=4097), dict(He=4097, We=4097)):
        assert cells(**kw) == -1 and fwd(**kw) == -1, kw
    assert fwd(E=0) == -1 and fwd(E=65536) == -1 and fwd(w=ctypes.c_void_p(68)) == -1
    assert fwd(E=65535, F=4096, L=4096) == -1                                       # more workgroups than a grid holds


def _prototype_arity(name):
    text = open(os.path.join(ROOT, "include", "gcfr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_the_bindings_arity_is_the_headers_and_the_frame_tile_is_the_kernels():
    from geomconsistentfr_amd import _lib, lighting
    for name in NEW_ENTRIES:
        assert name in _lib._SIGNATURES, name
        assert len(_lib._SIGNATURES[name][1]) == _prototype_arity(name), name
    for name in ("gcfr_light_rig_fwd", "gcfr_environment_cells", "gcfr_environment_fwd", "gcfr_inference_images_u8"):
        assert len(_lib._SIGNATURES[name][1]) == _prototype_arity(name), name      # (the parser, on entries that exist already)
    src = open(os.path.join(ROOT, "geomconsistentfr_amd", "csrc", "gcfr_rig_frames.hip")).read()
    assert int(re.search(r"constexpr int kFrameTile = (\d+);", src).group(1)) == lighting.RIG_FRAMES_TILE
    assert int(re.search(r"constexpr int kFramesMaxFrames = (\d+);", src).group(1)) == lighting.MAX_FRAMES
    assert int(re.search(r"constexpr int kFramesMaxLights = (\d+);", src).group(1)) == lighting.MAX_LIGHTS
    from geomconsistentfr_amd import build
    assert "gcfr_rig_frames.hip" in build.SOURCES
    import geomconsistentfr_amd as pkg
    assert pkg.rig_frames_u8 is lighting.rig_frames_u8 and pkg.environment_lights_frames is lighting.environment_lights_frames


def test_the_frames_kernels_use_no_scratch(tmp_path):
    import test_kernel_resources as res
    if not os.path.exists(os.path.join(res.LLVM, "llvm-readelf")):
        pytest.skip("needs the ROCm LLVM tools")
    k = res._kernel_metadata(tmp_path)
    mine = {n: v for n, v in k.items() if n.startswith("light_rig_frames") or re.match(r"environment_\w+_frames", n)}
    print(mine)
    assert sum(n.startswith("light_rig_frames_kernel<") for n in mine) == 2, sorted(k)          # the vector and the element path
    assert any(n.startswith("environment_cells_frames") for n in mine) and any(n.startswith("environment_fwd_frames") for n in mine)
    for n, v in mine.items():
        assert v["scratch"] == 0, (n, v)
    # the image kernel, whose composite moved into the shared header, is as spill-free as before
    assert all(v["scratch"] == 0 for n, v in k.items() if n.startswith("inference_images_kernel"))
