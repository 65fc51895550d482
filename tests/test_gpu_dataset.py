"""GPU: batch assembly from bytes (gcfr_assemble_batch_u8) against load_data()'s float64 arithmetic
(train_raytracing_relighting_CelebAHQ_DSSIM_8x.py:545-556, 607-615), the assembled batch through one Trainer.step, and the
device reductions of the MATLAB metrics (gcfr_masked_metrics_u8) against the oracle's numpy statements of MSE_MP.m:24 /
DSSIM_MP_RGB.m:24-26."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from make_dataset_fixture import write_dataset  # noqa: E402
from test_dataset_host import load_data_statement  # noqa: E402
import postprocess_statements as st  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_batch_from_bytes_equals_the_scripts_float64_batch(tmp_path):
    from geomconsistentfr_amd.dataset import RelightDataset
    write_dataset(str(tmp_path), 5)
    ds = RelightDataset(str(tmp_path))
    images, lightings, deps, msk, alb, fill = load_data_statement(str(tmp_path))
    idx = [3, 0, 4]
    b = ds.batch(idx, device=DEV)
    torch.cuda.synchronize()
    # T8:607-615: slices of the f64 arrays, /255.0 where load_data had not divided, then .float() at the call (T8:618)
    np.testing.assert_array_equal(b["images"].cpu().numpy(), images[idx].astype(np.float32))
    np.testing.assert_array_equal(b["masks"].cpu().numpy(), (msk[idx] / 255.0).astype(np.float32))
    np.testing.assert_array_equal(b["masks_fill"].cpu().numpy(), (fill[idx] / 255.0).astype(np.float32))
    np.testing.assert_array_equal(b["albedo"].cpu().numpy()[..., 0], (alb[idx] / 255.0).astype(np.float32))
    np.testing.assert_allclose(b["lightings"].cpu().numpy(), lightings[idx], rtol=1e-7)
    np.testing.assert_array_equal(b["depths"].cpu().numpy(), deps[idx].astype(np.float32))
    assert set(np.unique(b["masks_fill"].cpu().numpy())) <= {0.0, 1.0}


def test_assembled_batch_drives_a_training_step(tmp_path):
    from geomconsistentfr_amd.dataset import RelightDataset
    from geomconsistentfr_amd.train import TrainConfig, Trainer
    write_dataset(str(tmp_path), 3)
    ds = RelightDataset(str(tmp_path))
    torch.manual_seed(0)
    tr = Trainer(TrainConfig(miopen_find=False), device=DEV)
    logs = tr.step(ds.batch([0, 1, 2], device=DEV), 0, 0)                      # T8:617-656 on a batch of 3, epoch 0
    for k in ("recon", "depth", "ambient", "lighting", "albedo", "generator", "DSSIM", "total", "discriminator"):
        assert np.isfinite(logs[k]), (k, logs)


@pytest.mark.parametrize("B,H,W,shared", [(3, 64, 48, False), (2, 256, 256, True), (1, 37, 29, False)])
def test_masked_metrics_match_the_matlab_statements(B, H, W, shared):
    from geomconsistentfr_amd.dataset import masked_metrics
    rng = np.random.default_rng(H + B)
    gt = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    recon = np.clip(gt.astype(int) + rng.integers(-25, 26, gt.shape), 0, 255).astype(np.uint8)
    recon[0, : H // 3] = gt[0, : H // 3]                                            # an identical region
    mask = rng.choice([0, 64, 255], size=(1 if shared else B, H, W), p=[0.5, 0.1, 0.4]).astype(np.uint8)
    t = lambda a: torch.from_numpy(a).to(DEV)
    mse, dssim = masked_metrics(t(recon), t(gt), t(mask))
    mse, dssim = mse.cpu().numpy(), dssim.cpu().numpy()
    for b in range(B):
        m = mask[0 if shared else b]
        np.testing.assert_allclose(mse[b], st.masked_mse(recon[b], gt[b], m), rtol=1e-12)
        np.testing.assert_allclose(dssim[b], st.masked_dssim(recon[b], gt[b], m), rtol=1e-9, atol=1e-12)
    same, _ = masked_metrics(t(gt), t(gt), t(mask))
    assert float(same.abs().max()) == 0.0


# ============================================================================================================================
# The pins.  Batch assembly straight from bytes, bit for bit against numpy on bytes; the metrics per pixel and per regime against the
# long-double restatement and the exact rational MSE of tests/masked_metrics_emulation.py (no expected value comes from a kernel).
# tests/test_masked_metrics_host.py shows on the CPU that these inputs tell the wrong variants (a)-(h) from the statement.
# ============================================================================================================================
import masked_metrics_emulation as emu  # noqa: E402

SENTINEL = -7.5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assembly_statement(images, dmask, fmask, albedo):
    """T8:550-556, 610-615 and .float() (T8:618) on bytes"""
    f = lambda a: (a / 255.0).astype(np.float32)
    return dict(images=f(images), masks=f(dmask)[..., None], masks_fill=(np.maximum(fmask, dmask) > 128).astype(np.float32)[..., None],
                albedo=f(albedo)[..., None])


def _assert_bits(got, want, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def _random_bytes(seed, B, H, W):
    rng = np.random.default_rng(seed)
    u8 = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    dmask, fmask = u8(B, H, W), u8(B, H, W)
    fmask.flat[::5] = 128                                   # the threshold itself, on either side of the maximum
    dmask.flat[::7] = 128
    return u8(B, H, W, 3), dmask, fmask, u8(B, H, W)


def test_assembly_of_every_byte_and_every_pair_of_mask_bytes():
    from geomconsistentfr_amd.dataset import assemble_batch
    r, c = np.mgrid[0:256, 0:256]
    face, depth, albedo = (a.astype(np.uint8)[None] for a in (r, c, (r + c) & 255))
    images = np.stack([(r + 85 * ch + c) & 255 for ch in range(3)], axis=-1).astype(np.uint8)[None]
    assert all(len(np.unique(a)) == 256 for a in (depth, albedo, images[..., 0], images[..., 1], images[..., 2]))
    got = assemble_batch(_t(images), _t(depth), _t(face), _t(albedo))
    want = _assembly_statement(images, depth, face, albedo)
    for k in want:
        _assert_bits(got[k], want[k], k)
    fill = got["masks_fill"].cpu().numpy()[0, ..., 0]
    np.testing.assert_array_equal(fill, (np.maximum(r, c) > 128).astype(np.float32))         # all 65,536 pairs
    at_threshold = np.maximum(r, c) == 128
    assert int(at_threshold.sum()) == 257 and (fill[at_threshold] == 0.0).all()               # "> 128": 128 itself is not filled
    assert (fill[np.maximum(r, c) == 129] == 1.0).all()


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 5, 7), (3, 37, 29), (2, 16, 16), (1, 1, 257)])
def test_assembly_at_tails_and_odd_shapes(B, H, W):
    """B H W below, at and just over one 256-lane block, and H != W"""
    from geomconsistentfr_amd.dataset import assemble_batch
    arrays = _random_bytes(B * H * W, B, H, W)
    got = assemble_batch(*[_t(a) for a in arrays])
    want = _assembly_statement(*arrays)
    assert set(got) == set(want)
    for k in want:
        _assert_bits(got[k], want[k], k)


def _banded(n, shape, band=64):
    """-> (buffer, view): a contiguous f32 view of `shape` between two bands of SENTINEL"""
    buf = torch.full((band + n + band,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[band:band + n].view(shape)


@pytest.mark.parametrize("absent", ["none", "masks", "masks_fill", "albedo", "all"])
def test_assembly_with_absent_outputs_writes_only_its_own_bytes(absent):
    from geomconsistentfr_amd import _lib
    B, H, W = 3, 37, 29                                      # 3219 pixels: the last block is partial
    arrays = _random_bytes(11, B, H, W)
    images_u8, dmask, fmask, albedo_u8 = [_t(a) for a in arrays]
    want = _assembly_statement(*arrays)
    n = B * H * W
    out = dict(images=_banded(3 * n, (B, H, W, 3)), masks=_banded(n, (B, H, W, 1)), masks_fill=_banded(n, (B, H, W, 1)),
               albedo=_banded(n, (B, H, W, 1)))
    gone = {"none": (), "all": ("masks", "masks_fill", "albedo")}.get(absent, (absent,))
    arg = lambda k: None if k in gone else out[k][1]
    _lib.launch("gcfr_assemble_batch_u8", DEV, images_u8, dmask, None if "masks_fill" in gone else fmask,
                None if "albedo" in gone else albedo_u8, B, H, W, arg("images"), arg("masks"), arg("masks_fill"), arg("albedo"), _lib.STREAM)
    torch.cuda.synchronize(DEV)
    for k, (buf, view) in out.items():
        assert (buf[:64] == SENTINEL).all() and (buf[-64:] == SENTINEL).all(), k
        if k in gone:
            assert (buf == SENTINEL).all(), k
        else:
            _assert_bits(view, want[k], k)


@pytest.mark.parametrize("case", ["masks_fill without face_mask_u8", "albedo without albedo_u8", "B = 0"])
def test_assembly_entry_refuses_and_launches_nothing(case):
    from geomconsistentfr_amd import _lib
    B, H, W = 2, 5, 7
    images_u8, dmask, fmask, albedo_u8 = [_t(a) for a in _random_bytes(12, B, H, W)]
    outs = [torch.full(s, SENTINEL, dtype=torch.float32, device=DEV) for s in ((B, H, W, 3), (B, H, W, 1), (B, H, W, 1), (B, H, W, 1))]
    args = {"masks_fill without face_mask_u8": (images_u8, dmask, None, albedo_u8, B),
            "albedo without albedo_u8": (images_u8, dmask, fmask, None, B),
            "B = 0": (images_u8, dmask, fmask, albedo_u8, 0)}[case]
    with pytest.raises(_lib.GcfrError, match="gcfr_assemble_batch_u8 failed: GCFR_ERR_INVALID_ARGUMENT"):
        _lib.launch("gcfr_assemble_batch_u8", DEV, *args, H, W, *outs, _lib.STREAM)
    torch.cuda.synchronize(DEV)
    assert all(bool((o == SENTINEL).all()) for o in outs)


def test_assembly_of_non_contiguous_inputs_and_on_a_side_stream():
    from geomconsistentfr_amd.dataset import assemble_batch
    B, H, W = 3, 9, 13
    rng = np.random.default_rng(13)
    rgba = rng.integers(0, 256, (5, H, W, 4), dtype=np.uint8)
    wide = rng.integers(0, 256, (3, 5, H, 2 * W), dtype=np.uint8)
    idx = [3, 0, 4]
    images = _t(rgba)[idx][..., :3]                            # fancy-indexed, then channel-sliced: strides (4 H W, 4 W, 4, 1)
    planes = [_t(wide)[i][idx][..., ::2] for i in range(3)]    # every other column
    assert not images.is_contiguous() and not any(p.is_contiguous() for p in planes)
    want = _assembly_statement(rgba[idx][..., :3], *[wide[i][idx][..., ::2] for i in range(3)])
    got = assemble_batch(images, *planes)
    for k in want:
        _assert_bits(got[k], want[k], k)
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = assemble_batch(images, *planes)
    side.synchronize()
    for k in want:
        _assert_bits(got[k], want[k], "side stream, " + k)


def test_batch_from_bytes_at_another_size(tmp_path):
    """the reader and the kernel at 40 x 24: B H W = 1920 is no multiple of 256"""
    from geomconsistentfr_amd.dataset import RelightDataset
    H, W = 40, 24
    write_dataset(str(tmp_path), 3, H=H, W=W)
    ds = RelightDataset(str(tmp_path), H=H, W=W)
    images, lightings, deps, msk, alb, fill = load_data_statement(str(tmp_path), H, W)
    idx = [2, 0]
    b = ds.batch(idx, device=DEV)
    torch.cuda.synchronize()
    assert b["images"].shape == (2, H, W, 3) and b["masks"].shape == b["masks_fill"].shape == b["albedo"].shape == (2, H, W, 1)
    np.testing.assert_array_equal(b["images"].cpu().numpy(), images[idx].astype(np.float32))
    np.testing.assert_array_equal(b["masks"].cpu().numpy(), (msk[idx] / 255.0).astype(np.float32))
    np.testing.assert_array_equal(b["masks_fill"].cpu().numpy(), (fill[idx] / 255.0).astype(np.float32))
    np.testing.assert_array_equal(b["albedo"].cpu().numpy()[..., 0], (alb[idx] / 255.0).astype(np.float32))
    np.testing.assert_allclose(b["lightings"].cpu().numpy(), lightings[idx], rtol=1e-7)
    np.testing.assert_array_equal(b["depths"].cpu().numpy(), deps[idx].astype(np.float32))
    assert set(np.unique(b["masks_fill"].cpu().numpy())) <= {0.0, 1.0}


# ----------------------------------------------------------------------------------------------------------------------------
# masked metrics
# ----------------------------------------------------------------------------------------------------------------------------
def _metrics(recon, gt, mask):
    from geomconsistentfr_amd.dataset import masked_metrics
    mse, dssim = masked_metrics(_t(recon), _t(gt), _t(mask))
    assert mse.dtype == dssim.dtype == torch.float64 and mse.shape == dssim.shape == (recon.shape[0],)
    return mse.cpu().numpy(), dssim.cpu().numpy()


def _assert_metrics(got, want, what=""):
    """(mse, dssim) of the kernels against (the exact rational's float, the long-double value): the project's gates"""
    for name, g, w, gate_ in (("mse", got[0], want[0], emu.MSE_GATE), ("dssim", got[1], want[1], emu.DSSIM_GATE)):
        w = np.asarray(w).astype(np.float64)
        err = np.abs(g - w)
        i = int(np.nanargmax(err)) if err.size and not np.isnan(err).all() else 0
        print("%s %s: largest deviation %.3g (value %.6g) at %d" % (what, name, err.flat[i], w.flat[i], i))
        np.testing.assert_allclose(g, w, err_msg="%s %s" % (what, name), **gate_)


def _per_pixel(recon, gt, value):
    """every pixel's metrics from ONE call: the pair repeated H W times under the H W one-hot masks"""
    H, W, _ = recon.shape
    hot = emu.one_hot(H, W, value)
    rep = lambda a: np.repeat(a[None], H * W, axis=0)
    got = _metrics(rep(recon), rep(gt), hot)
    want = (np.array([emu.mse_exact(recon, gt, m) for m in hot]), emu.dssim_map(recon, gt).ravel())
    # MSE under a one-hot mask of value v, written out: sum_ch (a - g)^2 v^2 / (255^3 3 v)
    d2 = ((recon.astype(np.int64) - gt.astype(np.int64)) ** 2).sum(axis=-1).ravel()
    np.testing.assert_allclose(want[0], d2 * value / (255.0 ** 3 * 3.0), rtol=1e-15)
    return got, want


@pytest.mark.parametrize("name,value", [(n, 255) for n in emu.CASE_NAMES] + [("noise", 64), ("const200_201", 64)])
def test_metrics_per_pixel(name, value):
    """all 143 pixels of a 13 x 11 pair, each against the restatement's map: a mis-clamp at one border is not diluted by a mean;
    with the one-hot value 64 the mask must cancel out of the DSSIM"""
    H, W = emu.PER_PIXEL_SHAPE
    recon, gt = emu.cases(H, W, emu.SEED)[name]
    got, want = _per_pixel(recon, gt, value)
    _assert_metrics(got, want, "%s one-hot %d" % (name, value))


@pytest.mark.parametrize("H,W", emu.CLAMP_SHAPES)
@pytest.mark.parametrize("name", ["noise", "ramp"])
def test_metrics_per_pixel_where_both_clamps_act_on_one_pixel(name, H, W):
    recon, gt = emu.cases(H, W, emu.SEED)[name]
    got, want = _per_pixel(recon, gt, 255)
    _assert_metrics(got, want, "%s %dx%d" % (name, H, W))


@pytest.mark.parametrize("H,W", emu.WHOLE_SHAPES)
def test_metrics_of_whole_images_in_every_regime(H, W):
    """every named pair under three masks, as 27 faces of one call; then the same call again: one block per image (P <= 256) gives
    the same bits, more blocks meet in an f64 atomic whose order is not fixed -- agreement within the gate there, never bits"""
    c, m = emu.cases(H, W, emu.SEED), emu.masks(H, W, emu.SEED)
    keys = [(n, k) for n in emu.CASE_NAMES for k in ("full", "levels", "ring")]
    recon, gt = (np.stack([c[n][i] for n, _ in keys]) for i in (0, 1))
    mask = np.stack([m[k] for _, k in keys])
    want = emu.batch(recon, gt, mask)
    got = _metrics(recon, gt, mask)
    _assert_metrics(got, want, "%dx%d" % (H, W))
    for i, (n, k) in enumerate(keys):
        if n in ("black_black", "white_white"):
            assert got[0][i] == 0.0, (n, k)
    again = _metrics(recon, gt, mask)
    if H * W <= 256:
        np.testing.assert_array_equal(again[0], got[0])
        np.testing.assert_array_equal(again[1], got[1])
    else:
        print("%dx%d spread between two calls: mse %.3g, dssim %.3g" % (H, W, np.abs(again[0] - got[0]).max(), np.abs(again[1] - got[1]).max()))
        _assert_metrics(again, want, "%dx%d again" % (H, W))


def test_metrics_mask_forms():
    H, W = emu.PER_PIXEL_SHAPE
    recon, gt, m3 = emu.three_faces(H, W, emu.SEED)
    per_face = _metrics(recon, gt, m3)
    _assert_metrics(per_face, emu.batch(recon, gt, m3), "per-face masks")
    for b in range(3):                                         # the per-face result is three single calls (one block each: bits)
        for form in (m3[b], m3[b][None]):                      # (H,W) and (1,H,W) with B = 1
            single = _metrics(recon[b:b + 1], gt[b:b + 1], form)
            assert single[0][0] == per_face[0][b] and single[1][0] == per_face[1][b], (b, form.shape)
    levels = m3[1]
    want = emu.batch(recon, gt, levels)
    for form in (levels, levels[None], np.stack([levels] * 3)):    # one mask for B = 3, in all three forms
        _assert_metrics(_metrics(recon, gt, form), want, "shared mask %s" % (form.shape,))


def test_metrics_of_an_all_zero_mask_are_nan_for_that_face_alone():
    H, W = emu.PER_PIXEL_SHAPE
    recon, gt, m3 = emu.three_faces(H, W, emu.SEED)
    m3 = m3.copy()
    m3[1] = 0
    mse, dssim = _metrics(recon, gt, m3)
    assert np.isnan(mse[1]) and np.isnan(dssim[1])              # 0/0, as in MATLAB
    want = emu.batch(recon, gt, m3)
    assert np.isnan(want[0][1]) and np.isnan(want[1][1])
    keep = [0, 2]
    _assert_metrics((mse[keep], dssim[keep]), (want[0][keep], want[1][keep]), "beside an all-zero mask")


def _metrics_operands(H=15, W=17):
    from geomconsistentfr_amd import _lib
    recon, gt, m3 = emu.three_faces(H, W, emu.SEED)
    ws_bytes = int(_lib.load().gcfr_masked_metrics_workspace_bytes(3, H, W))
    assert ws_bytes == (3 * H * W * 15 + 4 * 3) * 8
    return recon, gt, m3, ws_bytes, emu.batch(recon, gt, m3)


def _banded_f64(n, band=16):
    buf = torch.full((band + n + band,), SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[band:band + n]


def test_metrics_with_an_absent_output():
    from geomconsistentfr_amd import _lib
    H, W = 15, 17
    recon, gt, m3, ws_bytes, want = _metrics_operands(H, W)
    r, g, m = _t(recon), _t(gt), _t(m3)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
    for present in ("mse", "dssim"):
        buf, both = _banded_f64(6)                              # [band | would-be mse | would-be dssim | band]
        mse, dssim = both[:3], both[3:]
        _lib.launch("gcfr_masked_metrics_u8", DEV, r, g, m, 3, 3, H, W, mse if present == "mse" else None,
                    dssim if present == "dssim" else None, ws, ws_bytes, _lib.STREAM)
        torch.cuda.synchronize(DEV)
        assert (buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all()
        if present == "mse":
            np.testing.assert_allclose(mse.cpu().numpy(), want[0], **emu.MSE_GATE)
            assert (dssim == SENTINEL).all()
        else:
            np.testing.assert_allclose(dssim.cpu().numpy(), want[1].astype(np.float64), **emu.DSSIM_GATE)
            assert (mse == SENTINEL).all()
    with pytest.raises(_lib.GcfrError, match="gcfr_masked_metrics_u8 failed: GCFR_ERR_INVALID_ARGUMENT"):
        _lib.launch("gcfr_masked_metrics_u8", DEV, r, g, m, 3, 3, H, W, None, None, ws, ws_bytes, _lib.STREAM)


def test_metrics_on_a_dirty_workspace_of_exactly_the_stated_size():
    """NaN everywhere in the workspace before the call: `fields` is fully written before it is read and `sums` is reset; the
    workspace's neighbours are untouched; a second call on the used workspace gives the first one's results (P = 255: one block)"""
    from geomconsistentfr_amd import _lib
    H, W = 15, 17
    recon, gt, m3, ws_bytes, want = _metrics_operands(H, W)
    r, g, m = _t(recon), _t(gt), _t(m3)
    buf, ws = _banded_f64(ws_bytes // 8)
    ws.fill_(float("nan"))
    results = []
    for _ in range(2):
        mse, dssim = (torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2))
        _lib.launch("gcfr_masked_metrics_u8", DEV, r, g, m, 3, 3, H, W, mse, dssim, ws, ws_bytes, _lib.STREAM)
        torch.cuda.synchronize(DEV)
        results.append((mse.cpu().numpy(), dssim.cpu().numpy()))
        _assert_metrics(results[-1], want, "dirty workspace")
        assert (buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all()
        assert not torch.isnan(ws).any()                        # every double of the stated size is the entry's own
    np.testing.assert_array_equal(results[0][0], results[1][0])
    np.testing.assert_array_equal(results[0][1], results[1][1])


@pytest.mark.parametrize("case", ["one byte short", "not a multiple of 8"])
def test_metrics_entry_refuses_a_workspace_it_cannot_use(case):
    from geomconsistentfr_amd import _lib
    H, W = 15, 17
    recon, gt, m3, ws_bytes, _ = _metrics_operands(H, W)
    buf, ws = _banded_f64(ws_bytes // 8)
    mse, dssim = (torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2))
    where, size = (ws, ws_bytes - 1) if case == "one byte short" else (ws.data_ptr() + 4, ws_bytes)     # (the band makes room)
    with pytest.raises(_lib.GcfrError, match="gcfr_masked_metrics_u8 failed: GCFR_ERR_INVALID_ARGUMENT"):
        _lib.launch("gcfr_masked_metrics_u8", DEV, _t(recon), _t(gt), _t(m3), 3, 3, H, W, mse, dssim, where, size, _lib.STREAM)
    torch.cuda.synchronize(DEV)
    assert (buf == SENTINEL).all() and (mse == SENTINEL).all() and (dssim == SENTINEL).all()
