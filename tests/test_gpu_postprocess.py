"""GPU: the inference-side byte kernels (csrc/gcfr_postprocess.hip)
  (1) against the bytes the reference's OWN main() produced (tests/golden/slt_main_*.npz, SLT:516-579 run unmodified by
      oracle/make_golden_slt_main.py): the kernel on the reference's model outputs, and the whole
      inference.lighting_transfer() with the shipped checkpoint;
  (2) against the oracle's numpy statements of the same script lines (oracle/postprocess_statements.py, themselves
      bit-equal to that main(): tests/test_oracle_postprocess.py), byte for byte -- half-way cases included -- at other
      shapes and in both mask modes, and against scipy for the MATLAB border fix."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import postprocess_statements as st  # noqa: E402  (checker only)

GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _inputs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.random(s, dtype=np.float32)
    x = f(B, H, W, 3)
    ren, alb = f(B, 3, H, W) * 1.2 - 0.1, f(B, 3, H, W)                       # a few values beyond [0, 1]: saturation
    depth = (60 * rng.standard_normal((B, 1, H, W))).astype(np.float32)
    w, fin = f(B, H, W), f(B, H, W) * 1.1
    nrm = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    mask_u8 = rng.choice([0, 64, 128, 192, 255], size=(H, W), p=[0.4, 0.1, 0.1, 0.1, 0.3]).astype(np.uint8)
    # plant exact half-way cases: 255*r*m == k + 0.5
    ren[0, 0, 0, :8] = np.float32((np.arange(8) + 0.5) / 255.0)
    mask_u8[0, :8] = 255
    return x, ren, alb, depth, w, fin, nrm, mask_u8


def rgb(a):
    if a.ndim == 3 and a.shape[2] == 3:
        return a[..., ::-1]
    return a[..., 0] if a.ndim == 3 else a


KEYS = ["rendered_image", "shadow_mask", "albedo", "depth", "shading", "surface_normals"]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_kernel_on_the_reference_model_outputs_gives_the_reference_main_bytes(tag):
    """The device kernel fed with what the reference's relighting pass returned (final_shading / normals rounded to the
    f32 the device holds) against the bytes of the six images the reference's main() wrote: every byte within 1 LSB,
    >= 99.99 % identical (the f32 rounding of the two f64 maps can move a value across a half-way point)."""
    from geomconsistentfr_amd import postprocess as pp
    z = np.load(os.path.join(GOLDEN, "slt_main_%s.npz" % tag))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    got = pp.inference_images_device(t((z["input_u8"] / 255.0).astype(np.float32)[None]), t(z["model_rendered_images"]),
                                     t(z["mask_u8"]), albedo=t(z["model_albedo"]), depth=t(z["model_depth"]),
                                     shadow_mask_weights=t(z["model_shadow_mask_weights"]),
                                     final_shading=t(z["model_final_shading"].astype(np.float32)),
                                     surface_normals=t(z["model_surface_normals"].astype(np.float32)), mask_f32=True)
    torch.cuda.synchronize()
    for k in KEYS:
        g, e = got[k][0].cpu().numpy().astype(int), rgb(z[k + "_u8"]).astype(int)
        assert np.abs(g - e).max() <= 1, k
        assert (g == e).mean() >= 0.9999, (k, (g == e).mean())
    for k in ("rendered_image", "shadow_mask", "albedo", "depth"):     # all-f32 inputs: nothing was rounded, so exact
        np.testing.assert_array_equal(got[k][0].cpu().numpy(), rgb(z[k + "_u8"]), err_msg=k)


def test_kernel_gives_the_single_image_scripts_bytes():
    """mask_f32 = 0 (the f64-mask flow of S1 / S8) against the bytes of the reference's own S1 main()
    (tests/golden/s1_main.npz): every input of the composite is f32 or uint8, so every byte is identical."""
    from geomconsistentfr_amd import postprocess as pp
    z = np.load(os.path.join(GOLDEN, "s1_main.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    got = pp.inference_images_device(t((z["input_u8"] / 255.0).astype(np.float32)[None]), t(z["model_rendered_images"]),
                                     t(z["mask_u8"]))
    np.testing.assert_array_equal(got["rendered_image"][0].cpu().numpy(), z["rendered_image_u8"][..., ::-1])


def _slt_model():
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "slt_checkpoint_epoch106.npz")).items()}
    m = RelightNetLightingTransfer()
    m.load_state_dict(sd, strict=True)
    return m.float().to(DEV).eval()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_lighting_transfer_end_to_end_against_the_reference_main(tag):
    """inference.lighting_transfer() -- both passes of the network (MIOpen), the HIP render block, the HIP image
    kernel -- with the reference's shipped checkpoint on the reference's inputs, against the six images its main()
    wrote.  The network runs on other convolution kernels than torch-CPU's, so: estimated light within 1e-4, every
    byte within 1 LSB except isolated pixels (a shadow decision can flip), >= 99.9 % of the bytes identical."""
    from geomconsistentfr_amd.inference import lighting_transfer
    z = np.load(os.path.join(GOLDEN, "slt_main_%s.npz" % tag))
    res = lighting_transfer(_slt_model(), z["input_u8"] / 255.0, z["reference_u8"] / 255.0, z["mask_u8"], device=DEV)
    np.testing.assert_allclose(res["estimated_light"], z["estimated_light"], atol=1e-4)
    np.testing.assert_allclose(res["estimated_ambient"], z["estimated_ambient"], atol=1e-4)
    for k in KEYS:
        g, e = res[k].astype(int), rgb(z[k + "_u8"]).astype(int)
        diff = np.abs(g - e)
        assert (diff <= 1).mean() >= 0.9999, (k, (diff <= 1).mean(), diff.max())
        assert (diff == 0).mean() >= 0.999, (k, (diff == 0).mean())


@pytest.mark.parametrize("mask_f32", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 256, 256), (3, 64, 96), (2, 37, 51)])
def test_inference_images_match_the_host_statement_byte_for_byte(B, H, W, mask_f32):
    from geomconsistentfr_amd import postprocess as pp
    x, ren, alb, depth, w, fin, nrm, mask_u8 = _inputs(B, H, W, B * 1000 + W)
    # the mask as the script holds it: S1:580 / S8:569 numpy f64 / 255.0; SLT:540 torch u8 / 255.0 -> f32
    m01 = (mask_u8.astype(np.float32) / np.float32(255.0)) if mask_f32 else mask_u8 / 255.0
    t = lambda a: torch.from_numpy(a).to(DEV)
    got = pp.inference_images_device(t(x), t(ren), t(mask_u8), albedo=t(alb), depth=t(depth), shadow_mask_weights=t(w),
                                     final_shading=t(fin), surface_normals=t(nrm), mask_f32=mask_f32)
    torch.cuda.synchronize()
    for b in range(B):
        # final_shading / normals are f64 in the reference: the kernel widens the device's f32 before the arithmetic
        exp = st.diagnostic_images(x[b].astype(np.float64), alb[b], depth, b, w[b], ren[b], fin[b].astype(np.float64),
                                   nrm[b].astype(np.float64), m01)
        for k, v in exp.items():
            np.testing.assert_array_equal(got[k][b].cpu().numpy(), st.to_uint8(v), err_msg="%s face %d" % (k, b))
    # only the composite, per-face masks
    masks = np.stack([np.roll(mask_u8, 3 * b, axis=1) for b in range(B)])
    only = pp.inference_images_device(t(x), t(ren), t(masks))
    assert set(only) == {"rendered_image"}
    for b in range(B):
        np.testing.assert_array_equal(only["rendered_image"][b].cpu().numpy(),
                                      st.to_uint8(st.composite_into_input(x[b].astype(np.float64), ren[b], masks[b] / 255.0)))


@pytest.mark.parametrize("B,H,W", [(1, 256, 256), (2, 40, 36), (2, 33, 70)])
def test_border_fix_matches_matlab_semantics(B, H, W):
    import scipy.ndimage as ndi
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = np.zeros((B, H, W), np.uint8)
    mask[:, H // 5:H - H // 4, W // 6:W - W // 5] = rng.choice([64, 127, 128, 255], size=(B, H - H // 4 - H // 5, W - W // 5 - W // 6))
    mask[0, :3, :] = 255                                                       # a mask touching the image border: zero padding
    got = pp.fix_border_artifacts_device(torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)).cpu().numpy()
    n_border = 0
    for b in range(B):
        np.testing.assert_array_equal(got[b], st.fix_border_artifacts(img[b], mask[b]))          # host statement
        m = np.floor(mask[b] / 255.0 + 0.5)                                                        # MATLAB uint8 division
        conv = ndi.correlate(m, np.ones((7, 7)), mode="constant", cval=0.0)
        border = (conv < 30) & (conv > 0)
        n_border += int(border.sum())
        for c in range(3):                                                                          # scipy, independently
            med = ndi.median_filter(img[b, ..., c], size=3, mode="constant", cval=0)
            np.testing.assert_array_equal(got[b, ..., c][border], med[border])
        np.testing.assert_array_equal(got[b][~border], img[b][~border])
    assert n_border > 0
    # one mask shared by the batch
    shared = pp.fix_border_artifacts_device(torch.from_numpy(img).to(DEV), torch.from_numpy(mask[B - 1]).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(shared[0], st.fix_border_artifacts(img[0], mask[B - 1]))


def test_device_functions_have_no_cpu_path():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    with pytest.raises(GcfrError):
        pp.inference_images_device(torch.zeros(1, 8, 8, 3), torch.zeros(1, 3, 8, 8), torch.ones(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(GcfrError):
        pp.fix_border_artifacts_device(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.ones(8, 8, dtype=torch.uint8))


@pytest.mark.parametrize("mask_f32", [False, True])
def test_byte_lattice_every_mask_byte_on_the_half_way_points(mask_f32):
    """Every one of the 256 mask bytes (a resized face mask takes them all), and under each the values at which every plane's
    expression comes to k + 0.5 or one f32 step beside it (tests/device_primitives_reference.py `byte_lattice`), plus a NaN, a
    +inf and a negative rendered value under mask 255: byte for byte the scripts' statements.  A mask formed as
    mk * (1 / 255.0f) changes 13 % of these bytes in the f32 mode (tests/test_device_primitives_host.py)."""
    import device_primitives_reference as ref
    from geomconsistentfr_amd import postprocess as pp
    lat = ref.byte_lattice(mask_f32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    got = pp.inference_images_device(t(lat["input"][None]), t(lat["rendered"][None]), t(lat["mask_u8"]), albedo=t(lat["albedo"][None]),
                                     depth=t(lat["depth"][None]), shadow_mask_weights=t(lat["shadow"][None]),
                                     final_shading=t(lat["shading"][None]), surface_normals=t(lat["normals"][None]), mask_f32=mask_f32)
    torch.cuda.synchronize()
    want = ref.lattice_expected(lat, mask_f32)
    assert set(got) == set(ref.PLANES) and ref.lattice_cases(lat) > 600000
    for k in ref.PLANES:
        g = got[k][0].cpu().numpy()
        print("%s: %d of %d lattice bytes differ" % (k, int(((g != want[k]) & lat["kept"][k]).sum()), int(lat["kept"][k].sum())))
    for k in ref.PLANES:
        np.testing.assert_array_equal(got[k][0].cpu().numpy(), want[k], err_msg=k)
    assert list(got["rendered_image"][0, 255, 253:, 0].cpu().numpy()) == [0, 255, 0]     # NaN, +inf, negative
