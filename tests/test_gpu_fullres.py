"""GPU: the full-resolution kernels (csrc/gcfr_fullres.hip; postprocess.ingest_photographs_device / fullres_composites_device) byte
for byte against the numpy restatement (tests/fullres_emulation.py).

  shapes   (s, h, w): (1,7,9) and (2,5,3) take the element path (W no multiple of four); (4,3,5), (8,2,3) the vector path;
           (4,1,1) has every tap clamped to the one low-resolution pixel; (4,20,28) has more than one workgroup per face; (1,4,8)
           and (2,3,6) put s = 1 and s = 2 on the vector path as well (their column windows are the widest).
  inputs   B in {1, 2}, L in {1, 3, 5}; the mask shared or per face, with the shipped masks' grey levels {0, 64, 128, 255};
           `rendered` well outside [0, 1]; x_lo scaled away from the photograph's own means: both saturations and both sides of
           detail_clamp occur (asserted on the inputs); a NaN; every operand off its alignment; `out=` between guard bands; a side
           stream; `rendered` in f64.
  identity rendered == x_lo returns the photograph; s = 1 under a full mask is the image kernel's composite away from ties."""
import numpy as np
import pytest
import torch

import fullres_emulation as emu
from test_fullres_host import TIE, TIE_SHARE

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 7, 9), (2, 5, 3), (4, 3, 5), (8, 2, 3), (4, 1, 1), (4, 20, 28), (1, 4, 8), (2, 3, 6)]
LEVELS = np.array([255, 0, 64, 128], np.uint8)
NAMES = ("photo", "x_lo", "rendered", "mask")


def _inputs(seed, B, L, s, h, w, shared_mask):
    """photo (B,H,W,3) u8, x_lo (B,h,w,3) f32, rendered (B,L,3,h,w) f32, mask (1|B,h,w) u8"""
    rng = np.random.default_rng(seed)
    H, W = s * h, s * w
    photo = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    x_lo = (emu.ingest(photo, s) * (0.1 + 1.9 * rng.random((B, h, w, 3), dtype=np.float32))).astype(np.float32)
    rendered = (0.5 + 1.5 * rng.standard_normal((B, L, 3, h, w))).astype(np.float32)
    MB = 1 if shared_mask else B
    mask = np.stack([rng.permutation(m) for m in np.resize(LEVELS, MB * h * w).reshape(MB, h * w)]).reshape(MB, h, w)
    # hi-res pixels (0,0) and (0,1) read low-res pixel (0,0) alone, or (0,0) and (0,1) which are made equal: a quotient of
    # 255 / 40 above the clamp and one of 1 / 40 below it, a relit value below 0 and one above 255, all under a mask of 1
    photo[:, 0, 0, :], photo[:, 0, 1, :] = 255, 1
    x_lo[:, 0, :2, :] = np.float32(40.0 / 255.0)
    mask[:, 0, :2] = 255
    rendered[:, 0, 0, 0, :2], rendered[:, 0, 1, 0, :2] = -1.0, 5.0
    return photo, x_lo, rendered, mask


def _assert_regimes(arrays, s):
    photo, x_lo, rendered, mask = arrays
    q = emu.raw_quotient(photo, x_lo, s)
    v, m = emu.values(photo, x_lo, rendered, mask, s)
    inside = np.broadcast_to(m > 0, v.shape)
    assert (q > 4.0).any() and (q < 0.25).any(), "both sides of detail_clamp"
    assert (v[inside] < -0.5).any() and (v[inside] > 255.5).any(), "both saturations"


def _dev(a, misalign=False):
    """a device tensor of `a`; misalign: its first element sits one element past an aligned allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.to(DEV)
    buf = torch.empty(a.size + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(a.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _check(label, arrays, s, misalign=(), **kw):
    from geomconsistentfr_amd import postprocess as pp
    t = {n: _dev(a, n in misalign) for n, a in zip(NAMES, arrays)}
    got = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"], t["mask"], s, **kw)
    want = emu.composites(*arrays, s, **{k: v for k, v in kw.items() if k != "out"})
    g = got.cpu().numpy()
    print("%s: bytes that differ from the statement %d of %d" % (label, int((g != want).sum()), g.size))
    assert g.shape == want.shape and g.dtype == np.uint8
    np.testing.assert_array_equal(g, want, err_msg=label)
    return got, t


@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("s,h,w", SHAPES)
def test_composites_equal_the_statement(s, h, w, B, L):
    case = SHAPES.index((s, h, w))
    shared = (case + B + L) % 2 == 0
    arrays = _inputs(100 * case + 10 * B + L, B, L, s, h, w, shared)
    if h * w >= 12:                                                               # (two mask values are overwritten with 255)
        assert set(np.unique(arrays[3])) == set(LEVELS.tolist())
    _assert_regimes(arrays, s)
    got, _ = _check("(%d,%d,%d) B %d L %d" % (s, h, w, B, L), arrays, s)
    assert tuple(got.shape) == (B, L, s * h, s * w, 3)


@pytest.mark.parametrize("shared", [True, False])
def test_masks_shared_or_per_face_and_a_four_dimensional_rendered(shared):
    from geomconsistentfr_amd import postprocess as pp
    s, h, w, B = 4, 3, 5, 2
    arrays = _inputs(7, B, 1, s, h, w, shared)
    got, t = _check("mask shared %s" % shared, arrays, s)
    one = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"][:, 0], t["mask"][0] if shared else t["mask"], s)
    assert tuple(one.shape) == (B, s * h, s * w, 3) and torch.equal(one, got[:, 0])
    # `rendered` is the one operand that may arrive in another floating-point type
    again = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"].double(), t["mask"], s)
    assert torch.equal(again, got)
    # other arguments than the defaults
    _check("clamp 2, floor 8", arrays, s, detail_clamp=2.0, floor=8.0)


@pytest.mark.parametrize("s,h,w", SHAPES)
@pytest.mark.parametrize("B", [1, 2])
def test_ingest_bits(s, h, w, B):
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(s + h)
    photo = rng.integers(0, 256, (B, s * h, s * w, 3), dtype=np.uint8)
    want = emu.ingest(photo, s)
    for mis in (False, True):
        got = pp.ingest_photographs_device(_dev(photo, mis), s)
        assert tuple(got.shape) == (B, h, w, 3) and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if s == 1:
        np.testing.assert_array_equal(want.view(np.uint32), np.float32(photo / 255.0).view(np.uint32))


@pytest.mark.parametrize("s,h,w", [(4, 6, 8), (2, 6, 7), (1, 8, 8)])
def test_one_nan_gives_zero_where_its_taps_reach_inside_the_mask_and_nothing_under_a_zero_mask(s, h, w):
    B, L = 2, 3
    photo, x_lo, rendered, mask = _inputs(11, B, L, s, h, w, True)
    mask[:] = 255
    mask[0, :3, :3] = 0                                                           # every tap of low-res pixel (1,1) has mask 0
    clean, _ = _check("before the NaN", (photo, x_lo, rendered, mask), s)
    rendered[0, 0, 0, 1, 1] = np.nan                                              # under the zero mask
    (b, l, c), (yy, xx) = (1, 1, 2), (4, 5)
    rendered[b, l, c, yy, xx] = np.nan
    got, _ = _check("NaN", (photo, x_lo, rendered, mask), s)
    g, want = got.cpu().numpy(), clean.cpu().numpy().copy()
    rows, cols = emu.tap_footprint(s * h, s, h, yy), emu.tap_footprint(s * w, s, w, xx)
    m = emu.mask_up(mask, s)[0]
    assert (m[np.ix_(rows, cols)] > 0).all() and rows.size >= s and cols.size >= s
    assert (g[b, l][np.ix_(rows, cols)][..., c] == 0).all() and (want[b, l][np.ix_(rows, cols)][..., c] > 0).any()
    want[b, l, rows[:, None], cols[None, :], c] = 0
    np.testing.assert_array_equal(g, want)                                        # no other byte changed
    rz, cz = emu.tap_footprint(s * h, s, h, 1), emu.tap_footprint(s * w, s, w, 1)
    assert (m[np.ix_(rz, cz)] == 0).all()
    np.testing.assert_array_equal(g[0, 0][np.ix_(rz, cz)], photo[0][np.ix_(rz, cz)])


@pytest.mark.parametrize("which", ["photo", "x_lo", "rendered", "mask", "out", "all"])
@pytest.mark.parametrize("s,h,w", [(4, 3, 5), (1, 4, 8)])
def test_every_operand_off_its_alignment(s, h, w, which):
    """W is a multiple of four: aligned, these shapes take the vector path; with the photograph or the output one byte off, the
    element path must return the same bytes; the f32 operands and the mask need no alignment on either path"""
    B, L = 2, 3
    arrays = _inputs(12, B, L, s, h, w, False)
    mis = NAMES if which == "all" else (which,)
    kw = {}
    if which in ("out", "all"):
        buf = torch.full((B * L * s * h * s * w * 3 + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        kw["out"] = buf[1:].view(B, L, s * h, s * w, 3)
        assert kw["out"].data_ptr() % 4 == 1
    got, _ = _check("misaligned " + which, arrays, s, misalign=mis, **kw)
    if kw:
        assert got.data_ptr() == kw["out"].data_ptr() and int(buf[0]) == 0xAB


@pytest.mark.parametrize("s,h,w", [(2, 5, 3), (4, 3, 5), (4, 20, 28)])
def test_out_is_written_in_place_between_untouched_guard_bands(s, h, w):
    from geomconsistentfr_amd import postprocess as pp
    B, L = 2, 3
    arrays = _inputs(13, B, L, s, h, w, True)
    n = B * L * s * h * s * w * 3
    buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(B, L, s * h, s * w, 3)
    got, t = _check("out=", arrays, s, out=out)
    assert got.data_ptr() == out.data_ptr() and (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all()
    again = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"], t["mask"], s)              # two calls: the same bytes
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)


def test_a_side_stream():
    from geomconsistentfr_amd import postprocess as pp
    s, h, w = 4, 20, 28
    arrays = _inputs(14, 2, 3, s, h, w, False)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        x_dev = pp.ingest_photographs_device(photo, s)
        got = pp.fullres_composites_device(photo, x_lo, rendered, mask, s)
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), emu.composites(*arrays, s))
    np.testing.assert_array_equal(x_dev.cpu().numpy(), emu.ingest(arrays[0], s))


@pytest.mark.parametrize("s,h,w", SHAPES)
def test_identity_rendered_equal_to_x_lo_returns_the_photograph(s, h, w):
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(20 + s + w)
    B = 2
    photo = _dev(rng.integers(64, 225, (B, s * h, s * w, 3), dtype=np.uint8))
    mask = _dev(np.stack([rng.permutation(m) for m in np.resize(LEVELS, B * h * w).reshape(B, h * w)]).reshape(B, h, w))
    x_lo = pp.ingest_photographs_device(photo, s)
    got = pp.fullres_composites_device(photo, x_lo, x_lo.permute(0, 3, 1, 2).contiguous(), mask, s)
    assert tuple(got.shape) == (B, s * h, s * w, 3) and torch.equal(got, photo)


def test_scale_one_under_a_full_mask_is_the_image_kernels_composite():
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(5)
    B, L, h, w = 2, 3, 37, 44
    photo = _dev(rng.integers(64, 225, (B, h, w, 3), dtype=np.uint8))
    ren_np = (1.2 * rng.random((B, L, 3, h, w))).astype(np.float32)
    rendered = _dev(ren_np)
    mask = torch.full((1, h, w), 255, dtype=torch.uint8, device=DEV)
    x_lo = pp.ingest_photographs_device(photo, 1)
    got = pp.fullres_composites_device(photo, x_lo, rendered, mask, 1).cpu().numpy()
    want = pp.inference_images_device(x_lo, rendered, mask)["rendered_image"].cpu().numpy()
    value = np.transpose((np.float32(255.0) * ren_np).astype(np.float64), (0, 1, 3, 4, 2))       # what the image kernel quantises
    near_tie = np.abs(value - np.floor(value) - 0.5) <= TIE
    share = float(near_tie.mean())
    diff = (got != want) & ~near_tie
    print("s = 1: %d values, %d near a tie (%.4f %%), %d differ away from ties" % (got.size, int(near_tie.sum()), 100 * share, int(diff.sum())))
    assert share <= TIE_SHARE and not diff.any() and want.max() == 255
