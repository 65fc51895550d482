"""GPU: the guided full-resolution composite (csrc/gcfr_fullres_guided.hip; postprocess.fullres_composites_device(upsample="guided"))
byte for byte against the numpy restatement (tests/fullres_guided_emulation.py).

  shapes   (s, h, w): (1,7,9) and (2,5,3) take the element path (W no multiple of four); (4,3,5), (8,2,3), (1,8,12), (2,9,10) and
           (8,6,7) the vector path at every s (each s has its own window and its own left-border case); (4,1,1) has every tap
           clamped to the one low-resolution pixel; (4,20,28) has several workgroups per face.
  inputs   B in {1, 2}, L in {1, 3, 5}; the mask shared or per face with the shipped masks' grey levels, a zero block in its
           bottom-right corner and 255 in its top-left one; `rendered` well outside [0, 1]; x_lo scaled away from the
           photograph's own means.  Both saturations, both sides of detail_clamp and (for h, w >= 3) pixels with m > 0 and with
           m == 0 occur: asserted on the inputs, from the restatement.  range_sigma in {8, 20, inf}; a NaN in `rendered` and in
           x_lo; every operand off its alignment; `out=` between guard bands; a side stream; `rendered` in f64 and as (B,3,h,w).
  identity rendered == x_lo returns the photograph; upsample="bilinear" is the call without the keyword; the step edge of
           tests/test_fullres_guided_host.py does not leak through a one-sided mask."""
import numpy as np
import pytest
import torch

import fullres_guided_emulation as emu
from test_fullres_guided_host import offsets, step_edge

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 7, 9), (2, 5, 3), (4, 3, 5), (8, 2, 3), (1, 8, 12), (2, 9, 10), (8, 6, 7), (4, 1, 1), (4, 20, 28)]
LEVELS = np.array([255, 0, 64, 128], np.uint8)
SIGMAS = (8.0, 20.0, float("inf"))
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
    # the 4 x 4 footprint reaches a non-zero scattered mask value from every pixel: m == 0 needs a block of zeros.  The pixels of the
    # bottom-right corner read the last two rows and columns only
    mask[:, max(h - 3, 0):, max(w - 3, 0):] = 0
    # hi-res pixels (0,0) and (0,1) read the top-left 3 x 3 block alone (a fourth column, at s = 1, with weight 0), which is made
    # uniform: a quotient of 255 / 40 above the clamp and one of 1 / 40 below it, a relit value below 0 and one above 255, all under
    # a mask of 1
    mask[:, :3, :3] = 255
    photo[:, 0, 0, :], photo[:, 0, 1, :] = 255, 1
    x_lo[:, :3, :3, :] = np.float32(40.0 / 255.0)
    rendered[:, 0, 0, :3, :3], rendered[:, 0, 1, :3, :3] = -1.0, 5.0
    return photo, x_lo, rendered, mask


def _assert_regimes(arrays, s, **kw):
    photo, x_lo, rendered, mask = arrays
    _, raw, _, _, m1 = emu.parts(photo, x_lo, mask, s, **kw)
    v, m = emu.values(photo, x_lo, rendered, mask, s, **kw)
    inside = np.broadcast_to(m > 0, v.shape)
    clamp = kw.get("detail_clamp", 4.0)
    assert (raw > clamp).any() and (raw < 1.0 / clamp).any(), "both sides of detail_clamp"
    assert (v[inside] < -0.5).any() and (v[inside] > 255.5).any(), "both saturations"
    h, w = mask.shape[-2:]
    if h >= 3 and w >= 3:
        assert (m1 > 0).any() and (m1 == 0).any(), "pixels inside and outside the mask"


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
    got = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"], t["mask"], s, upsample="guided", **kw)
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
    sigma = SIGMAS[(case + B + L) % 3]
    arrays = _inputs(100 * case + 10 * B + L, B, L, s, h, w, shared)
    _assert_regimes(arrays, s, range_sigma=sigma)
    got, _ = _check("(%d,%d,%d) B %d L %d sigma %g" % (s, h, w, B, L, sigma), arrays, s, range_sigma=sigma)
    assert tuple(got.shape) == (B, L, s * h, s * w, 3)


@pytest.mark.parametrize("shared", [True, False])
def test_masks_shared_or_per_face_a_four_dimensional_rendered_and_other_arguments(shared):
    from geomconsistentfr_amd import postprocess as pp
    s, h, w, B = 4, 3, 5, 2
    arrays = _inputs(7, B, 1, s, h, w, shared)
    got, t = _check("mask shared %s" % shared, arrays, s)                          # the default range_sigma, 20
    one = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"][:, 0], t["mask"][0] if shared else t["mask"], s,
                                       upsample="guided")
    assert tuple(one.shape) == (B, s * h, s * w, 3) and torch.equal(one, got[:, 0])
    # `rendered` is the one operand that may arrive in another floating-point type
    again = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"].double(), t["mask"], s, upsample="guided")
    assert torch.equal(again, got)
    # other arguments than the defaults
    for sigma in SIGMAS:
        _assert_regimes(arrays, s, detail_clamp=2.0, floor=8.0, range_sigma=sigma)
        other, _ = _check("clamp 2, floor 8, sigma %g" % sigma, arrays, s, detail_clamp=2.0, floor=8.0, range_sigma=sigma)
        assert not torch.equal(other, got)


@pytest.mark.parametrize("s,h,w", [(4, 6, 8), (2, 6, 7), (1, 8, 8)])
def test_one_nan_in_rendered_gives_zero_and_one_in_x_lo_keeps_the_photograph(s, h, w):
    B, L = 2, 3
    photo, x_lo, rendered, mask = _inputs(11, B, L, s, h, w, True)
    mask[:] = 255
    clean, _ = _check("before the NaN", (photo, x_lo, rendered, mask), s)
    iy, _ = emu.taps(s * h, s, h)
    ix, _ = emu.taps(s * w, s, w)
    (b, l, c), (yy, xx) = (1, 1, 2), (4, 5)
    R, C = np.ix_(np.nonzero((iy == yy).any(axis=1))[0], np.nonzero((ix == xx).any(axis=1))[0])
    assert R.size >= s and C.size >= s
    ren = rendered.copy()
    ren[b, l, c, yy, xx] = np.nan
    got, _ = _check("NaN in rendered", (photo, x_lo, ren, mask), s)
    want = clean.cpu().numpy().copy()
    assert (want[b, l][R, C, c] > 0).any()
    want[b, l][R, C, c] = 0                                                       # (also through a tap of weight 0)
    np.testing.assert_array_equal(got.cpu().numpy(), want)                        # no other byte changed
    x = x_lo.copy()
    x[b, yy, xx, 0] = np.nan
    got, _ = _check("NaN in x_lo", (photo, x, rendered, mask), s)
    want = clean.cpu().numpy().copy()
    assert (want[b][:, R, C, :] != photo[b][R, C][None]).any()
    want[b][:, R, C, :] = photo[b][R, C][None]                                    # m is NaN there: every light keeps the photograph
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("which", ["photo", "x_lo", "rendered", "mask", "out", "all"])
@pytest.mark.parametrize("s,h,w", [(4, 3, 5), (1, 8, 12)])
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
    again = pp.fullres_composites_device(t["photo"], t["x_lo"], t["rendered"], t["mask"], s, upsample="guided")   # two calls: the same bytes
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)


def test_a_side_stream():
    from geomconsistentfr_amd import postprocess as pp
    s, h, w = 4, 20, 28
    arrays = _inputs(14, 2, 3, s, h, w, False)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = pp.fullres_composites_device(photo, x_lo, rendered, mask, s, upsample="guided", range_sigma=8.0)
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), emu.composites(*arrays, s, range_sigma=8.0))


@pytest.mark.parametrize("s,h,w", SHAPES)
def test_identity_rendered_equal_to_x_lo_returns_the_photograph(s, h, w):
    from geomconsistentfr_amd import postprocess as pp
    rng = np.random.default_rng(20 + s + w)
    B = 2
    photo = _dev(rng.integers(64, 225, (B, s * h, s * w, 3), dtype=np.uint8))
    mask = _dev(np.stack([rng.permutation(m) for m in np.resize(LEVELS, B * h * w).reshape(B, h * w)]).reshape(B, h, w))
    x_lo = pp.ingest_photographs_device(photo, s)
    got = pp.fullres_composites_device(photo, x_lo, x_lo.permute(0, 3, 1, 2).contiguous(), mask, s, upsample="guided")
    assert tuple(got.shape) == (B, s * h, s * w, 3) and torch.equal(got, photo)


def test_bilinear_through_the_keyword_is_the_call_without_it():
    from geomconsistentfr_amd import postprocess as pp
    s, h, w = 4, 20, 28
    arrays = _inputs(15, 2, 3, s, h, w, True)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    plain = pp.fullres_composites_device(photo, x_lo, rendered, mask, s)
    assert torch.equal(pp.fullres_composites_device(photo, x_lo, rendered, mask, s, upsample="bilinear"), plain)
    assert torch.equal(pp.fullres_composites_device(photo, x_lo, rendered, mask, s, upsample="bilinear", range_sigma=3.0), plain)
    assert not torch.equal(pp.fullres_composites_device(photo, x_lo, rendered, mask, s, upsample="guided"), plain)


def test_the_step_edge_does_not_leak_through_a_one_sided_mask():
    """condition (ii) of tests/test_fullres_guided_host.py at s = 4, through the kernel"""
    s = 4
    for off in offsets(s):
        photo, x_lo, rendered, e, half, _ = step_edge(s, off)
        mask = np.broadcast_to(np.where(half, 255, 0).astype(np.uint8)[None, None, :], (1, 12, 16)).copy()
        got, _ = _check("step edge, off %d" % off, (photo, x_lo, rendered, mask), s)
        g = got.cpu().numpy()
        moved = np.abs(g[0, 0].astype(np.int64) - photo[0].astype(np.int64))
        print("off %d: largest move right of the edge %d, left of it %d" % (off, int(moved[:, e:].max()), int(moved[:, :e].max())))
        assert moved[:, e:].max() == 0 and moved[:, :e].max() > 20
