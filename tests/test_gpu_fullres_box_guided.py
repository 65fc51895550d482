"""GPU: the guided box kernel (csrc/gcfr_fullres_box_guided.hip; postprocess.fullres_box_composites_device(upsample="guided")) bit
for bit against the numpy restatement (tests/fullres_box_guided_emulation.py).

  networks (h, w) in {(5,7), (6,8), (4,8)}
  boxes    (bh, bw) per network, so that each axis sees a ratio of exactly 1, one in (1,2), one in (2,4), exactly 4 and one above
           4, the two axes not together; bw = 3 w and 3 w + 1, the two sides of the vector path's narrow column window; widths that
           are multiples of four (the vector path of paste=False) and not; touching the photograph's left, top, right and bottom
           border in turn, and in its interior; x0 odd and even
  photos   Wp a multiple of four (the vector path of paste=True) and not; the box starts at any column, so the vector path reads
           the photograph off its alignment
  calls    B in {1, 2, 33} (33 crosses the 32 faces of one launch), L in {1, 3}, paste both ways, the mask shared or per face,
           range_sigma in {20, 3, +inf}
  and      every operand off its alignment; `out=` between guard bands; a side stream; a NaN in `rendered` and one in x_lo; the
           anchor -- a whole-photograph power-of-two box returns the bytes of fullres_composites_device(upsample="guided"); the
           keyword's default is the bilinear box launch; the same box content at another origin in another photograph returns the
           same box bytes."""
import numpy as np
import pytest
import torch

import fullres_box_guided_emulation as emu
from test_gpu_fullres_box import LEVELS, NAMES, _dev, _inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NETS = [(5, 7), (6, 8), (4, 8)]
SIGMAS = [20.0, 3.0, float("inf")]


def _sizes(h, w):
    """(bh, bw): see the module's docstring"""
    return [(h, w), ((3 * h + 1) // 2, (3 * w + 1) // 2), (3 * h - 1, 3 * w + 1), (4 * h, 4 * w), (4 * h + 1, 5 * w + 2), (h, 4 * w + 4),
            (5 * h + 2, w + 1), (2 * h + 1, 3 * w)]


def _photo_size(h, w, aligned):
    return 5 * h + 5, 4 * ((6 * w + 3) // 4) + (0 if aligned else 1)


def _origins(Hp, Wp, bh, bw):
    """the box against the left, the top, the right and the bottom border, and an interior position"""
    xo, xe, ym = min(3, Wp - bw), min(6, Wp - bw), (Hp - bh + 1) // 2
    return [(0, ym), (xo, 0), (Wp - bw, min(1, Hp - bh)), (xe, Hp - bh), (xo, ym)]


def _check(label, arrays, boxes, misalign=(), **kw):
    from geomconsistentfr_amd import postprocess as pp
    t = {n: _dev(a, n in misalign) for n, a in zip(NAMES, arrays)}
    got = pp.fullres_box_composites_device(t["photo"], boxes, t["x_lo"], t["rendered"], t["mask"], upsample="guided", **kw)
    photo, x_lo, rendered, mask = arrays
    want = emu.composites(photo, boxes, x_lo, rendered, mask, **{k: v for k, v in kw.items() if k != "out"})
    g = got.cpu().numpy()
    print("%s: bytes that differ from the statement %d of %d" % (label, int((g != want).sum()), g.size))
    assert g.shape == want.shape and g.dtype == np.uint8
    np.testing.assert_array_equal(g, want, err_msg=label)
    return got, t


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("size", range(8))
@pytest.mark.parametrize("h,w", NETS)
def test_composites_equal_the_statement(h, w, size, aligned):
    bh, bw = _sizes(h, w)[size]
    Hp, Wp = _photo_size(h, w, aligned)
    assert h <= bh <= Hp and w <= bw <= Wp
    origins = _origins(Hp, Wp, bh, bw)
    case = 100 * NETS.index((h, w)) + 10 * size + aligned
    for i, (B, L) in enumerate([(1, 1), (2, 3), (1, 3), (2, 1)]):
        boxes = np.array([(x0, y0, bw, bh) for x0, y0 in (origins[i:] + origins)[:B]])
        shared = (case + i) % 2 == 0
        sigma = SIGMAS[(case // 10 + i) % 3]
        arrays = _inputs(1000 * case + i, B, L, h, w, Hp, Wp, boxes, shared)
        for paste in (True, False):
            got, _ = _check("(%d,%d) box %dx%d in %dx%d B %d L %d paste %s sigma %s" % (h, w, bh, bw, Hp, Wp, B, L, paste, sigma), arrays,
                            boxes, paste=paste, range_sigma=sigma)
            assert tuple(got.shape) == ((B, L, Hp, Wp, 3) if paste else (B, L, bh, bw, 3))
    # the interior box given once for every face, as a tuple
    one = tuple(int(v) for v in (origins[4] + (bw, bh)))
    _check("one box for both faces", _inputs(case, 2, 3, h, w, Hp, Wp, np.array(one), True), one)


def test_the_ratios_and_the_widths_the_docstring_promises():
    for h, w in NETS:
        for n, axis in ((h, 0), (w, 1)):
            r = [s[axis] / n for s in _sizes(h, w)]
            assert any(x == 1 for x in r) and any(1 < x < 2 for x in r) and any(2 < x < 4 for x in r) and any(x == 4 for x in r) \
                and any(x > 4 for x in r), (h, w, r)
        assert {s[1] % 4 == 0 for s in _sizes(h, w)} == {True, False}
    xs = {o[0] % 2 for h, w in NETS for s in _sizes(h, w) for o in _origins(*_photo_size(h, w, True), *s)}
    assert xs == {0, 1}


@pytest.mark.parametrize("s", [1, 2, 4, 8])
@pytest.mark.parametrize("h,w", [(4, 8), (5, 3), (20, 28)])
def test_a_whole_photograph_power_of_two_box_is_the_guided_entrys_bytes(h, w, s):
    from geomconsistentfr_amd import postprocess as pp
    B, L = 2, 3
    whole = (0, 0, s * w, s * h)
    arrays = _inputs(20 + s, B, L, h, w, s * h, s * w, np.array(whole), False)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    for sigma in (20.0, 3.0):
        want = pp.fullres_composites_device(photo, x_lo, rendered, mask, s, upsample="guided", range_sigma=sigma)
        for paste in (True, False):
            got = pp.fullres_box_composites_device(photo, whole, x_lo, rendered, mask, paste=paste, upsample="guided", range_sigma=sigma)
            assert got.shape == want.shape and torch.equal(got, want)
    assert (want.cpu().numpy() != arrays[0][:, None]).any()


@pytest.mark.parametrize("paste", [True, False])
def test_thirty_three_faces_cross_the_launch_limit(paste):
    from geomconsistentfr_amd import postprocess as pp
    h, w, B, L = 4, 8, 33, 3
    Hp, Wp = 23, 44
    rng = np.random.default_rng(33)
    if paste:                                                                      # every face its own size and origin
        bw, bh = rng.integers(w, Wp + 1, B), rng.integers(h, Hp + 1, B)
    else:                                                                          # one size, every face its own origin
        bw, bh = np.full(B, 20), np.full(B, 10)
    boxes = np.stack([rng.integers(0, Wp - bw + 1), rng.integers(0, Hp - bh + 1), bw, bh], axis=1)
    assert len({tuple(b) for b in boxes.tolist()}) >= 30
    arrays = _inputs(34, B, L, h, w, Hp, Wp, boxes, False)
    got, t = _check("B 33 paste %s" % paste, arrays, boxes, paste=paste)
    # a rendered without the light axis, in f64
    one = pp.fullres_box_composites_device(t["photo"], torch.from_numpy(boxes).to(torch.int16), t["x_lo"], t["rendered"][:, 1].double(),
                                           t["mask"], paste=paste, upsample="guided")
    assert one.dim() == 4 and torch.equal(one, got[:, 1])


@pytest.mark.parametrize("which", ["photo", "x_lo", "rendered", "mask", "out", "all"])
@pytest.mark.parametrize("paste", [True, False])
def test_every_operand_off_its_alignment(paste, which):
    """Wp and bw are multiples of four: aligned, both windows take the vector path; with the output one byte off, the element path
    must return the same bytes; the photograph, the f32 operands and the mask need no alignment on either path"""
    h, w, B, L = 4, 8, 2, 3
    Hp, Wp, bh, bw = 19, 68, 15, 36
    boxes = np.array([(5, 3, bw, bh), (31, 0, bw, bh)])
    arrays = _inputs(12, B, L, h, w, Hp, Wp, boxes, False)
    mis = NAMES if which == "all" else (which,)
    kw = {}
    shape = (B, L, Hp, Wp, 3) if paste else (B, L, bh, bw, 3)
    if which in ("out", "all"):
        buf = torch.full((int(np.prod(shape)) + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        kw["out"] = buf[1:].view(shape)
        assert kw["out"].data_ptr() % 4 == 1
    got, _ = _check("misaligned " + which, arrays, boxes, misalign=mis, paste=paste, **kw)
    if kw:
        assert got.data_ptr() == kw["out"].data_ptr() and int(buf[0]) == 0xAB


@pytest.mark.parametrize("paste", [True, False])
@pytest.mark.parametrize("Wp,bw", [(68, 36), (67, 35)])
def test_out_is_written_in_place_between_untouched_guard_bands(Wp, bw, paste):
    from geomconsistentfr_amd import postprocess as pp
    h, w, B, L = 4, 8, 2, 3
    Hp, bh = 40, 31                                                                # more than one workgroup per face
    boxes = np.array([(5, 3, bw, bh), (Wp - bw, Hp - bh, bw, bh)])
    arrays = _inputs(13, B, L, h, w, Hp, Wp, boxes, True)
    shape = (B, L, Hp, Wp, 3) if paste else (B, L, bh, bw, 3)
    n = int(np.prod(shape))
    assert n // (B * L * 3) > 1024
    buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(shape)
    got, t = _check("out=", arrays, boxes, paste=paste, out=out)
    assert got.data_ptr() == out.data_ptr() and (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all()
    again = pp.fullres_box_composites_device(t["photo"], boxes, t["x_lo"], t["rendered"], t["mask"], paste=paste, upsample="guided")
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)           # two calls: the same bytes
    np.testing.assert_array_equal(t["photo"].cpu().numpy(), arrays[0])


def test_a_side_stream():
    from geomconsistentfr_amd import postprocess as pp
    h, w = 20, 28
    Hp, Wp = 90, 124
    boxes = np.array([(7, 5, 101, 77), (20, 0, 100, 90)])
    arrays = _inputs(14, 2, 3, h, w, Hp, Wp, boxes, False)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, upsample="guided", range_sigma=8.0)
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), emu.composites(arrays[0], boxes, *arrays[1:], range_sigma=8.0))


def test_the_keywords_default_is_the_bilinear_box_launch():
    from geomconsistentfr_amd import postprocess as pp
    import fullres_box_emulation as bil
    h, w = 5, 7
    boxes = np.array([(3, 1, 22, 14), (10, 6, 22, 14)])
    arrays = _inputs(15, 2, 3, h, w, 23, 44, boxes, True)
    photo, x_lo, rendered, mask = [_dev(a) for a in arrays]
    for paste in (True, False):
        plain = pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, paste=paste)
        named = pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, paste=paste, upsample="bilinear", range_sigma=3.0)
        assert torch.equal(plain, named)
        np.testing.assert_array_equal(plain.cpu().numpy(), bil.composites(arrays[0], boxes, *arrays[1:], paste=paste))
        guided = pp.fullres_box_composites_device(photo, boxes, x_lo, rendered, mask, paste=paste, upsample="guided")
        assert guided.shape == plain.shape and not torch.equal(guided, plain)


def test_the_same_box_content_at_another_origin_in_another_photograph():
    from geomconsistentfr_amd import postprocess as pp
    h, w, L = 5, 7, 3
    bh, bw = 19, 28
    rng = np.random.default_rng(40)
    crop = rng.integers(0, 256, (bh, bw, 3), dtype=np.uint8)
    results = []
    for (Hp, Wp), (x0, y0) in (((23, 60), (0, 0)), ((23, 60), (31, 4)), ((40, 33), (5, 21)), ((19, 28), (0, 0))):
        photo = rng.integers(0, 256, (1, Hp, Wp, 3), dtype=np.uint8)
        photo[0, y0:y0 + bh, x0:x0 + bw] = crop
        b = (x0, y0, bw, bh)
        x = pp.ingest_box_device(_dev(photo), b, (h, w))
        if not results:
            rendered = _dev((0.5 + 0.5 * rng.standard_normal((1, L, 3, h, w))).astype(np.float32))
            mask = _dev(rng.choice(LEVELS, (1, h, w)))
        alone = pp.fullres_box_composites_device(_dev(photo), b, x, rendered, mask, paste=False, upsample="guided")
        pasted = pp.fullres_box_composites_device(_dev(photo), b, x, rendered, mask, upsample="guided")
        assert torch.equal(pasted[:, :, y0:y0 + bh, x0:x0 + bw], alone)
        results.append(alone)
    for alone in results[1:]:
        assert torch.equal(alone, results[0])
    assert (results[0].cpu().numpy() != crop).any()


def test_one_nan_in_rendered_and_one_in_x_lo_behave_as_on_the_host():
    h, w, B, L = 6, 8, 2, 3
    Hp, Wp, bh, bw = 31, 44, 23, 30
    boxes = np.array([(5, 3, bw, bh), (12, 8, bw, bh)])
    photo, x_lo, rendered, mask = _inputs(11, B, L, h, w, Hp, Wp, boxes, True)
    mask[:] = 255
    clean, _ = _check("before the NaN", (photo, x_lo, rendered, mask), boxes)
    want = clean.cpu().numpy().copy()
    (b, l, c), (yy, xx) = (1, 1, 2), (4, 5)
    rows, cols = emu.tap_footprint(bh, h, yy), emu.tap_footprint(bw, w, xx)
    R, C = rows + boxes[b, 1], cols + boxes[b, 0]
    # in `rendered`: byte 0 in that face, light and channel over the four-tap footprint, no other byte changes
    ren = rendered.copy()
    ren[b, l, c, yy, xx] = np.nan
    got, _ = _check("NaN in rendered", (photo, x_lo, ren, mask), boxes)
    g = got.cpu().numpy()
    assert (g[b, l][np.ix_(R, C)][..., c] == 0).all() and (want[b, l][np.ix_(R, C)][..., c] > 0).any()
    w1 = want.copy()
    w1[b, l, R[:, None], C[None, :], c] = 0
    np.testing.assert_array_equal(g, w1)
    # in x_lo: the weights, hence m, are NaN over the footprint: the photograph's bytes in every light, nothing else changes
    x = x_lo.copy()
    x[b, yy, xx, 0] = np.nan
    got, _ = _check("NaN in x_lo", (photo, x, rendered, mask), boxes)
    g = got.cpu().numpy()
    w2 = want.copy()
    w2[b][:, R[:, None], C[None, :], :] = photo[b][np.ix_(R, C)][None]
    np.testing.assert_array_equal(g, w2)
    assert (want[b][:, R[:, None], C[None, :], :] != photo[b][np.ix_(R, C)][None]).any()
    # a `rendered` of NaNs alone leaves every byte outside the boxes the photograph's
    got, _ = _check("all NaN", (photo, x_lo, np.full_like(rendered, np.nan), mask), boxes)
    outside = np.ones((B, Hp, Wp), bool)
    for i, (x0, y0, _, _) in enumerate(boxes):
        outside[i, y0:y0 + bh, x0:x0 + bw] = False
    g = got.cpu().numpy()
    for l in range(L):
        np.testing.assert_array_equal(g[:, l][outside], photo[outside])
