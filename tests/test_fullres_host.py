"""CPU: the full-resolution feature's numpy restatement (tests/fullres_emulation.py) held to independent statements, and the host
side of the two entries (csrc/gcfr_fullres.hip, postprocess.ingest_photographs_device / fullres_composites_device): every refusal
is made before any launch, so it is exercised without a GPU.

  Up        within 2e-7 of torch's F.interpolate(bilinear, align_corners=False) evaluated in f64, s in {2, 4, 8}
  ingest    at s = 1 the bits of np.float32(img / 255.0); at s > 1 the f64 block mean / 255, rounded once
  identity  rendered == x_lo, photograph bytes in [64, 224], any mask: the output is the photograph
  s = 1     under an all-255 mask the bytes of the scripts' composite (oracle/postprocess_statements.py), away from rounding ties"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import fullres_emulation as emu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import postprocess_statements as pps  # noqa: E402  (checker only)

SHAPES = [(1, 7, 9), (2, 5, 3), (4, 3, 5), (8, 2, 3), (4, 20, 28), (4, 1, 1)]
# The s = 1 comparison with the scripts' composite excludes values close to a rounding tie k + 1/2 and caps their share at 0.1 %.
# The two expressions differ by at most 1.04e-4 grey levels for |r| <= 306: d = p / (f32(p / 255) 255) is within 3 roundings of 1
# (3 x 2^-24), r d rounds once more (306 x 4 x 2^-24 = 7.3e-5 in all), r d - p and p + (.) round to half an ulp of 306 each
# (2 x 1.5e-5).  A window of +-1e-3 would by itself cover 0.2 % of uniformly spread values -- above the cap -- so the window here is
# the NARROWER +-2.5e-4 (0.05 %): fewer values are excused, and the cap stands.
TIE = 2.5e-4
TIE_SHARE = 1e-3      # at most 0.1 % of the values may be excluded


def _mask(rng, MB, h, w):
    m = np.resize(np.array([255, 0, 64, 128, 191], np.uint8), MB * h * w)
    return np.stack([rng.permutation(x) for x in m.reshape(MB, h * w)]).reshape(MB, h, w)


@pytest.mark.parametrize("s", [2, 4, 8])
def test_up_is_torchs_bilinear_in_f64(s):
    import torch.nn.functional as Fn
    rng = np.random.default_rng(s)
    for h, w in [(5, 3), (3, 5), (1, 1), (2, 7), (20, 28)]:
        a = rng.random((2, 3, h, w), dtype=np.float32)
        want = Fn.interpolate(torch.from_numpy(a).to(torch.float64), scale_factor=s, mode="bilinear", align_corners=False).numpy()
        got = emu.up(a, s)
        assert got.shape == (2, 3, s * h, s * w) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("s %d (%d,%d): max |Up - interpolate_f64| %.3g" % (s, h, w, err))
        assert err <= 2e-7
    # a constant field is returned exactly, also one that is not a dyadic number
    c = np.full((1, 4, 6), np.float32(0.1))
    assert (emu.up(c, s) == np.float32(0.1)).all()


def test_up_at_scale_one_is_the_identity():
    a = np.random.default_rng(0).standard_normal((2, 7, 9)).astype(np.float32)
    np.testing.assert_array_equal(emu.up(a, 1), a)


def test_ingest_bits():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (2, 7, 9, 3), dtype=np.uint8)
    got = emu.ingest(img, 1)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), np.float32(img / 255.0).view(np.uint32))
    for s, h, w in SHAPES[1:]:
        img = rng.integers(0, 256, (2, s * h, s * w, 3), dtype=np.uint8)
        want = np.float32(img.reshape(2, h, s, w, s, 3).astype(np.float64).mean(axis=(2, 4)) / 255.0)
        got = emu.ingest(img, s)
        assert got.shape == (2, h, w, 3)
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24            # (mean / 255 rounds twice in f64: not the same bits)
        assert (emu.ingest(np.full_like(img, 255), s) == np.float32(1.0)).all()


@pytest.mark.parametrize("s,h,w", SHAPES)
def test_identity_rendered_equal_to_x_lo_returns_the_photograph(s, h, w):
    rng = np.random.default_rng(10 * s + h)
    for B, shared in ((1, True), (2, False)):
        photo = rng.integers(64, 225, (B, s * h, s * w, 3), dtype=np.uint8)
        x_lo = emu.ingest(photo, s)
        rendered = np.ascontiguousarray(np.transpose(x_lo, (0, 3, 1, 2)))[:, None]
        mask = _mask(rng, 1 if shared else B, h, w)
        d, _ = emu.detail(photo, x_lo, s)
        assert d.min() > 0.25 and d.max() < 4.0                                    # no pixel is clamped
        got = emu.composites(photo, x_lo, rendered, mask, s)
        assert got.shape == (B, 1, s * h, s * w, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got[:, 0], photo)


def test_scale_one_under_a_full_mask_is_the_scripts_composite():
    rng = np.random.default_rng(3)
    B, L, h, w = 2, 3, 37, 41
    photo = rng.integers(64, 225, (B, h, w, 3), dtype=np.uint8)
    x_lo = emu.ingest(photo, 1)
    rendered = (1.2 * rng.random((B, L, 3, h, w))).astype(np.float32)
    mask = np.full((1, h, w), 255, np.uint8)
    got = emu.composites(photo, x_lo, rendered, mask, 1)
    want64 = np.stack([[pps.composite_into_input(x_lo[b], rendered[b, l], mask[0].astype(np.float64) / 255.0) for l in range(L)]
                       for b in range(B)])
    near_tie = np.abs(want64 - np.floor(want64) - 0.5) <= TIE
    share = float(near_tie.mean())
    diff = (got != pps.to_uint8(want64)) & ~near_tie
    print("s = 1: %d values, %d near a tie (%.4f %%), %d differ away from ties" % (got.size, int(near_tie.sum()), 100 * share, int(diff.sum())))
    assert got.size >= 9000 and share <= TIE_SHARE
    assert not diff.any()
    assert got.min() == 0 or got.max() == 255                                     # rendered reaches past 1: the saturation is exercised


def test_outside_the_mask_nothing_reaches_the_photograph():
    rng = np.random.default_rng(4)
    s, h, w = 4, 3, 5
    photo = rng.integers(0, 256, (1, s * h, s * w, 3), dtype=np.uint8)
    x_lo = emu.ingest(photo, s)
    rendered = np.full((1, 2, 3, h, w), np.nan, np.float32)
    mask = np.zeros((1, h, w), np.uint8)
    mask[0, 1, 2] = 255
    got = emu.composites(photo, x_lo, rendered, mask, s)
    m = emu.mask_up(mask, s)[0]
    assert 0 < (m > 0).sum() < m.size
    np.testing.assert_array_equal(got[0, :, m == 0], np.broadcast_to(photo[0, m == 0][:, None], got[0, :, m == 0].shape))
    assert (got[0, :, m > 0] == 0).all()                                          # NaN -> 0 inside


# ------------------------------------------------------------------------------------------------
# the entries' host side
# ------------------------------------------------------------------------------------------------
def test_the_c_entries_refuse_before_any_launch():
    from geomconsistentfr_amd import _lib
    L = _lib.load()
    p = lambda v: ctypes.c_void_p(v)
    ok_c = dict(photo=p(64), x_lo=p(128), rendered=p(256), mask=p(512), mask_batch=1, B=2, L=3, h=5, w=3, s=2, floor=1.0, clamp=4.0,
                out=p(1024))

    def comp(**kw):
        a = dict(ok_c, **kw)
        return L.gcfr_fullres_composites_u8(a["photo"], a["x_lo"], a["rendered"], a["mask"], a["mask_batch"], a["B"], a["L"], a["h"],
                                            a["w"], a["s"], a["floor"], a["clamp"], a["out"], None)

    for name in ("photo", "x_lo", "rendered", "mask", "out"):
        assert comp(**{name: None}) == -1, name
    for s in (0, 3, 5, 6, 16, -2):
        assert comp(s=s) == -1, s
    assert comp(L=0) == -1 and comp(L=4097) == -1 and comp(L=-1) == -1
    assert comp(mask_batch=0) == -1 and comp(mask_batch=3) == -1
    assert comp(out=p(64)) == -1                                                  # out == photo
    assert comp(clamp=0.99) == -1 and comp(clamp=float("nan")) == -1
    assert comp(floor=0.0) == -1 and comp(floor=-1.0) == -1 and comp(floor=float("nan")) == -1
    assert comp(B=0) == -1 and comp(h=0) == -1 and comp(w=0) == -1
    # a per-face pixel count, or a chunk count, that does not fit 31 bits
    assert comp(B=1, h=1 << 15, w=1 << 15, s=2) == -1                              # H W = 2^32
    assert comp(B=1, h=1 << 14, w=1 << 14, s=8) == -1                              # H W = 2^34
    assert comp(B=1 << 12, h=1 << 14, w=1 << 14, s=2) == -1                        # H W = 2^30, B chunks = 2^32

    def ing(photo=p(64), B=2, h=5, w=3, s=2, out=p(128)):
        return L.gcfr_ingest_photographs_u8(photo, B, h, w, s, out, None)

    assert ing(photo=None) == -1 and ing(out=None) == -1
    for s in (0, 3, 16, -1):
        assert ing(s=s) == -1, s
    assert ing(B=0) == -1 and ing(h=0) == -1 and ing(w=-1) == -1
    assert ing(B=1, h=1 << 15, w=1 << 15, s=2) == -1
    assert ing(B=1 << 12, h=1 << 14, w=1 << 14, s=2) == -1


def test_the_python_entries_refuse_malformed_operands_without_a_gpu():
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd._lib import GcfrError
    B, L, h, w, s = 2, 3, 5, 3, 2
    photo = torch.zeros((B, s * h, s * w, 3), dtype=torch.uint8)
    x_lo = torch.zeros((B, h, w, 3))
    rendered = torch.zeros((B, L, 3, h, w))
    mask = torch.zeros((h, w), dtype=torch.uint8)
    bad = [
        dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(photo_u8=photo[:, :-1]), dict(photo_u8=photo.numpy()),
        dict(scale=3), dict(scale=0), dict(scale=2.0), dict(scale=True),
        dict(x_lo=x_lo[:1]), dict(x_lo=x_lo.double()), dict(x_lo=x_lo.permute(0, 3, 1, 2)),
        dict(rendered=rendered[:, :, :2]), dict(rendered=rendered[:1]), dict(rendered=rendered[0, 0]), dict(rendered=rendered.to(torch.int32)),
        dict(rendered=torch.zeros((B, 0, 3, h, w))), dict(rendered=torch.zeros((B, s * h, s * w, 3))),
        dict(mask_u8=mask.float()), dict(mask_u8=torch.zeros((s * h, s * w), dtype=torch.uint8)), dict(mask_u8=torch.zeros((3, h, w), dtype=torch.uint8)),
        dict(detail_clamp=0.5), dict(detail_clamp=float("nan")), dict(floor=0.0), dict(floor=-2.0),
        dict(out=torch.zeros((B, L, s * h, s * w, 3))), dict(out=torch.zeros((B, s * h, s * w, 3), dtype=torch.uint8)),
    ]
    for kw in bad:
        a = dict(photo_u8=photo, x_lo=x_lo, rendered=rendered, mask_u8=mask, scale=s)
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.fullres_composites_device(**a)
    # well-formed host tensors: there is no CPU path
    with pytest.raises(GcfrError, match="no CPU path"):
        pp.fullres_composites_device(photo, x_lo, rendered, mask, s)
    for kw in (dict(photo_u8=photo.float()), dict(photo_u8=photo[0]), dict(scale=3), dict(photo_u8=photo[:, :, :-1]), dict(scale="2")):
        a = dict(photo_u8=photo, scale=s)
        a.update(kw)
        with pytest.raises(GcfrError):
            pp.ingest_photographs_device(**a)
    with pytest.raises(GcfrError, match="no CPU path"):
        pp.ingest_photographs_device(photo, s)


def test_the_inference_entries_exist_and_refuse_other_dtypes():
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd._lib import GcfrError
    for name in ("relight_lights_fullres", "relight_lights_fullres_device", "relight_rig_fullres", "relight_rig_fullres_device"):
        assert callable(getattr(inf, name))
    with pytest.raises(GcfrError, match="uint8"):
        inf.relight_lights_fullres_device(None, np.zeros((1, 8, 8, 3), np.float32), None, None, 2, device="cpu")
