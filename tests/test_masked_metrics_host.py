"""CPU: what the GPU tests of the dataset kernels (tests/test_gpu_dataset.py) stand on.
  - the high-precision restatement of the two metrics (tests/masked_metrics_emulation.py) against three other opinions: itself in
    float64, the oracle's statement (oracle/postprocess_statements.py, written separately) and a NON-separable 11 x 11 x 11
    correlation (scipy.ndimage, mode="nearest");
  - the inputs of the GPU tests tell every deliberately wrong variant (a)-(h) from the statement, by more than 100 gates;
  - the 256-entry table of batch assembly: what a rewrite of the division would and would not change;
  - the Python entries refuse malformed operands before anything is loaded or launched."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import masked_metrics_emulation as emu  # noqa: E402
import postprocess_statements as st  # noqa: E402  (a second opinion; the emulation does not import it)

SEED = emu.SEED
HOST_SHAPES = ((13, 11), (6, 5))


def _nonseparable_dssim(recon, gt, mask):
    """the third opinion: one 3-D correlation with the outer product of the taps, replicate ("nearest") borders, float64"""
    from scipy import ndimage
    k = emu.gauss_taps(np.float64)
    K = k[:, None, None] * k[None, :, None] * k[None, None, :]
    g = lambda x: ndimage.correlate(x, K, mode="nearest")
    A, R = recon / 255.0, gt / 255.0
    mux, muy = g(A), g(R)
    sx, sy, sxy = g(A * A) - mux * mux, g(R * R) - muy * muy, g(A * R) - mux * muy
    s = ((2 * mux * muy + 1e-4) * (2 * sxy + 9e-4)) / ((mux * mux + muy * muy + 1e-4) * (sx + sy + 9e-4))
    m3 = np.repeat((mask / 255.0)[..., None], 3, axis=-1)
    return (1.0 - (s * m3).sum() / m3.sum()) / 2.0


@pytest.mark.parametrize("H,W", HOST_SHAPES)
def test_four_statements_of_the_metrics_agree(H, W):
    for name, (recon, gt) in emu.cases(H, W, SEED).items():
        for mname, mask in emu.masks(H, W, SEED).items():
            want = emu.dssim(recon, gt, mask, np.longdouble)
            opinions = dict(float64=emu.dssim(recon, gt, mask, np.float64), oracle=st.masked_dssim(recon, gt, mask),
                            nonseparable=_nonseparable_dssim(recon, gt, mask))
            for who, got in opinions.items():
                np.testing.assert_allclose(float(got), float(want), err_msg="%s, %s mask, %s" % (name, mname, who), **emu.DSSIM_GATE)
            np.testing.assert_allclose(st.masked_mse(recon, gt, mask), emu.mse_exact(recon, gt, mask), rtol=1e-12, err_msg=name)
        # per pixel as well: the float64 emulation's map against the long-double one
        np.testing.assert_allclose(emu.dssim_map(recon, gt, np.float64), emu.dssim_map(recon, gt, np.longdouble).astype(np.float64),
                                   err_msg=name, **emu.DSSIM_GATE)


def test_values_that_can_be_stated_by_hand():
    c = emu.cases(13, 11, SEED)
    full = emu.masks(13, 11, SEED)["full"]
    for dtype in (np.longdouble, np.float64):
        # constant images: every mean is the constant, every variance 0 -> ssim = C1 C2 / ((1 + C1) C2) = 1e-4 / 1.0001
        np.testing.assert_allclose(float(emu.dssim(*c["black_white"], full, dtype)), (1 - 1e-4 / 1.0001) / 2, rtol=1e-13)
        np.testing.assert_allclose(float(emu.dssim(*c["black_white"], full, dtype)), 0.4999500049995, rtol=1e-12)
        assert emu.dssim(*c["black_black"], full, dtype) == 0 and emu.dssim(*c["white_white"], full, dtype) == 0
    assert emu.mse_exact(*c["black_white"], full) == 1.0 and emu.mse_exact(*c["black_black"], full) == 0.0
    # one pixel, one-hot mask of value v: sum_ch (a - g)^2 v^2 / (255^3 3 v)
    recon, gt = c["noise"]
    d2 = int(((recon[4, 7].astype(int) - gt[4, 7].astype(int)) ** 2).sum())
    assert emu.mse_exact(recon, gt, emu.one_hot(13, 11, 64)[4 * 11 + 7]) == pytest.approx(d2 * 64 / (255.0 ** 3 * 3), rel=1e-15)
    zero = np.zeros((13, 11), np.uint8)
    assert np.isnan(emu.mse_exact(recon, gt, zero)) and np.isnan(emu.dssim(recon, gt, zero))


# ----------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests discriminate
# ----------------------------------------------------------------------------------------------------------------------------
def separations(seed=SEED):
    """variant -> (margin in gates, where): the widest margin by which the inputs of the GPU tests separate the wrong variant from
    the statement -- per pixel (one-hot masks) at the per-pixel and the both-clamps shapes, whole-image at the regime shapes"""
    best = {}

    def see(wrong, where, got, want, g):
        with np.errstate(invalid="ignore"):                # (an MSE of 0 on both sides: the gate is 0 wide there, 0/0 separates nothing)
            margin = np.nan_to_num(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / emu.gate(want, **g), nan=0.0)
        i = int(np.argmax(margin))
        if margin.flat[i] > best.get(wrong, (0.0, ""))[0]:
            best[wrong] = (float(margin.flat[i]), "%s, pixel %d" % (where, i) if margin.size > 1 else where)
    per_pixel = [(emu.PER_PIXEL_SHAPE, None)] + [(s, ("noise", "ramp")) for s in emu.CLAMP_SHAPES]
    for (H, W), names in per_pixel:
        for name, (recon, gt) in emu.cases(H, W, seed).items():
            if names is not None and name not in names:
                continue
            want = emu.dssim_map(recon, gt).ravel()
            for wrong in emu.WRONG_SSIM:
                see(wrong, "%s %dx%d one-hot" % (name, H, W), emu.dssim_map(recon, gt, wrong=wrong).ravel(), want, emu.DSSIM_GATE)
            hot = emu.one_hot(H, W, 64)
            want = [emu.mse_exact(recon, gt, m) for m in hot]
            for wrong in emu.WRONG_MSE:
                see(wrong, "%s %dx%d one-hot 64" % (name, H, W), [emu.mse_exact(recon, gt, m, wrong) for m in hot], want, emu.MSE_GATE)
    for H, W in emu.WHOLE_SHAPES:
        for name, (recon, gt) in emu.cases(H, W, seed).items():
            for mname, mask in emu.masks(H, W, seed).items():
                where = "%s %dx%d %s mask" % (name, H, W, mname)
                want = emu.dssim(recon, gt, mask)
                for wrong in emu.WRONG_SSIM:
                    see(wrong, where, emu.dssim(recon, gt, mask, wrong=wrong), want, emu.DSSIM_GATE)
                want = emu.mse_exact(recon, gt, mask)
                if want > 0:
                    for wrong in emu.WRONG_MSE:
                        see(wrong, where, emu.mse_exact(recon, gt, mask, wrong), want, emu.MSE_GATE)
    recon, gt, m3 = emu.three_faces(13, 11, seed)
    mse, ds = emu.batch(recon, gt, m3)
    wmse, wds = emu.batch(recon, gt, m3, wrong="mask_face0")
    see("mask_face0", "three faces 13x11, dssim of face", wds, ds, emu.DSSIM_GATE)
    see("mask_face0", "three faces 13x11, mse of face", wmse, mse, emu.MSE_GATE)
    return best


def test_the_gpu_tests_inputs_tell_every_wrong_variant_from_the_statement():
    best = separations()
    for wrong in emu.WRONG_SSIM + emu.WRONG_MSE + emu.WRONG_BATCH:
        margin, where = best.get(wrong, (0.0, "nowhere"))
        print("%-20s %.3g gates at %s" % (wrong, margin, where))
        assert margin > 100.0, (wrong, margin, where)


def test_both_sided_clamps_are_what_the_small_shapes_add():
    """(b) and (e) at a pixel that clamps on BOTH sides of one axis (an axis shorter than 6): separated there too, not only at the
    13 x 11 image's one-sided borders"""
    for H, W in ((1, 7), (7, 1), (2, 3), (5, 5)):
        recon, gt = emu.cases(H, W, SEED)["noise"]
        want = emu.dssim_map(recon, gt).astype(np.float64)
        for wrong in ("reflect", "clamp_low_only"):
            got = emu.dssim_map(recon, gt, wrong=wrong).astype(np.float64)
            assert (np.abs(got - want) / emu.gate(want, **emu.DSSIM_GATE)).max() > 100.0, (H, W, wrong)


# ----------------------------------------------------------------------------------------------------------------------------
# batch assembly: the table
# ----------------------------------------------------------------------------------------------------------------------------
def test_the_assembly_table_separates_a_reciprocal_but_not_the_f32_division():
    """`f32(f64(v) / 255.0)` (T8:550, 610-615 then .float()) is what the kernel computes.  Multiplying by an f32 reciprocal differs at
    126 of the 256 bytes, so the GPU tests' bit-equality over all 256 sees that rewrite.  The f32 DIVISION gives the same 256
    floats: the suite cannot tell it from the f64 one, and does not claim to."""
    v = np.arange(256)
    table = (v / 255.0).astype(np.float32)
    reciprocal = v.astype(np.float32) * np.float32(1.0 / 255.0)
    divided = v.astype(np.float32) / np.float32(255.0)
    assert reciprocal.dtype == divided.dtype == np.float32
    assert int((table != reciprocal).sum()) == 126
    assert int((table != divided).sum()) == 0
    assert table[0] == 0.0 and table[255] == 1.0 and np.all(np.diff(table) > 0)


# ----------------------------------------------------------------------------------------------------------------------------
# the Python entries refuse before anything is loaded or launched
# ----------------------------------------------------------------------------------------------------------------------------
def _reached(*a, **k):
    raise AssertionError("a refused call reached the library")


def _no_launch(monkeypatch):
    from geomconsistentfr_amd import _lib
    monkeypatch.setattr(_lib, "launch", _reached)
    monkeypatch.setattr(_lib, "load", _reached)


def _z(*shape, dtype=torch.uint8):
    return torch.zeros(shape, dtype=dtype)


def test_assemble_batch_refuses_malformed_operands_before_any_launch(monkeypatch):
    from geomconsistentfr_amd._lib import NO_CPU_PATH, GcfrError
    from geomconsistentfr_amd.dataset import assemble_batch
    _no_launch(monkeypatch)
    B, H, W = 2, 5, 7
    names = ("images_u8", "depth_mask_u8", "face_mask_u8", "albedo_u8")
    good = [_z(B, H, W, 3), _z(B, H, W), _z(B, H, W), _z(B, H, W)]
    wrong_planes = dict(shorter=_z(B, H - 1, W), fewer_faces=_z(B - 1, H, W), longer=_z(B, H, W + 1), transposed=_z(B, W, H),
                        flat=_z(B * H * W), scalar_axis=_z(B, H, W, 3))
    for i in (1, 2, 3):
        for how, t in wrong_planes.items():
            args = list(good)
            args[i] = t
            with pytest.raises(GcfrError, match=r"assemble_batch: %s must be \(2,5,7\)" % names[i]):
                assemble_batch(*args)
    for how, t in dict(no_channels=_z(B, H, W), four_channels=_z(B, H, W, 4), no_faces=_z(0, H, W, 3), no_rows=_z(B, 0, W, 3)).items():
        with pytest.raises(GcfrError, match=r"assemble_batch: images_u8 must be \(B,H,W,3\)"):
            assemble_batch(t, *good[1:])
    for i in range(4):                                       # dtypes first, and not a tensor at all
        args = list(good)
        args[i] = good[i].to(torch.float32)
        with pytest.raises(GcfrError, match="assemble_batch: %s must be uint8" % names[i]):
            assemble_batch(*args)
        args[i] = good[i].numpy()
        with pytest.raises(GcfrError, match="assemble_batch: %s must be a tensor" % names[i]):
            assemble_batch(*args)
    # a malformed CPU tensor gets the shape's message, a well-formed one "no CPU path"
    with pytest.raises(GcfrError, match="no CPU path") as e:
        assemble_batch(*good)
    assert str(e.value) == NO_CPU_PATH


def test_masked_metrics_refuses_malformed_operands_before_any_launch(monkeypatch):
    from geomconsistentfr_amd._lib import NO_CPU_PATH, GcfrError
    from geomconsistentfr_amd.dataset import MAX_METRIC_FACES, masked_metrics
    _no_launch(monkeypatch)
    B, H, W = 3, 5, 7
    recon, gt = _z(B, H, W, 3), _z(B, H, W, 3)
    for how, t in dict(fewer_faces=_z(B - 1, H, W, 3), shorter=_z(B, H - 1, W, 3), transposed=_z(B, W, H, 3), planes=_z(B, 3, H, W),
                       grey=_z(B, H, W)).items():
        with pytest.raises(GcfrError, match=r"masked_metrics: gt_u8 must be \(3,5,7,3\)"):
            masked_metrics(recon, t, _z(H, W))
    for how, t in dict(two_of_three=_z(2, H, W), too_many=_z(B + 1, H, W), transposed=_z(W, H), shorter=_z(B, H, W - 1),
                       channel_axis=_z(B, H, W, 1), flat=_z(H * W)).items():
        with pytest.raises(GcfrError, match=r"masked_metrics: mask_u8 must be \(5,7\) or \(1,5,7\) or \(3,5,7\)"):
            masked_metrics(recon, gt, t)
    for t in (_z(0, H, W, 3), _z(B, H, W), _z(B, H, W, 1), _z(B, H, 0, 3)):              # B = 0 among them
        with pytest.raises(GcfrError, match=r"masked_metrics: recon_u8 must be \(B,H,W,3\)"):
            masked_metrics(t, t, _z(H, W))
    many = _z(MAX_METRIC_FACES + 1, 1, 1, 3)
    with pytest.raises(GcfrError, match="masked_metrics: recon_u8 .* 1 <= B <= 65535"):
        masked_metrics(many, many, _z(1, 1))
    for i, name in enumerate(("recon_u8", "gt_u8", "mask_u8")):
        args = [recon, gt, _z(H, W)]
        args[i] = args[i].to(torch.float64)
        with pytest.raises(GcfrError, match="masked_metrics: %s must be uint8" % name):
            masked_metrics(*args)
    for mask in (_z(H, W), _z(1, H, W), _z(B, H, W)):
        with pytest.raises(GcfrError, match="no CPU path") as e:
            masked_metrics(recon, gt, mask)
        assert str(e.value) == NO_CPU_PATH
    one = _z(MAX_METRIC_FACES, 1, 1, 3)                                                   # the largest B is well-formed
    with pytest.raises(GcfrError, match="no CPU path"):
        masked_metrics(one, one, _z(1, 1))
