#!/usr/bin/env python
"""A/B of the affine kernels (csrc/gcfr_fullres_affine.hip; postprocess.ingest_affine_device / fullres_affine_composites_device) at
8 faces, 11 lights and a network of 256 x 256, in photographs of 3000 x 2000 (Wp x Hp).

  (a) the price of the affine map on the box kernel's ground   the 900 x 860 box of tools/fullres_box_ab.py:
             leg A   postprocess.fullres_box_composites_device(paste=True) on the box
             leg B   postprocess.fullres_affine_composites_device on the box's axis-aligned map.  The bytes are NOT expected to be
                     equal at this ratio (900 / 256 is not a power of two, so the inverse map is rounded to 2^-14): the number of
                     bytes that differ is reported, nothing is asserted
  (b) the same box turned by 20 degrees about its centre
  (c) a 180-pixel face turned by 20 degrees: smaller than the network, the composite takes 2 x 2 sub-samples per pixel
  (d) the ingests    ingest_box_device on the box against ingest_affine_device on its map (K = 4), and the ingests of (b) and (c)

Nothing is gated on speed: these are figures.  Each composite's achieved bytes per second over its byte floor (`floor_bytes`: per
pixel of the photograph 3 bytes read and 3 L written, the low-resolution planes once) stand beside the rate of the library's copy
probe (gcfr_copy_probe, read + write) measured in the same run.  The kernels' register counts are read from the library's code
objects where the LLVM tools are installed.

The protocol is tools/fullres_box_ab.py's: one process, one device, no profiler attached.  The legs of a case ALTERNATE (A, B, A, B,
...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after `--warmup` untimed calls per
leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and include what the
host does per call (checks, the quantisation of the matrix, launches).  Needs a GPU: there is no fallback.  Writes the table as
Markdown to `--out` (default profiles/fullres_affine_ab.md) and prints the numbers as JSON.

usage: tools/fullres_affine_ab.py [--repeats 7] [--iters 10] [--warmup 3] [--out PATH]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, H_LO, W_LO = 8, 11, 256, 256
HP, WP = 2000, 3000
LARGE = (1037, 571, 900, 860)                                 # x0, y0, bw, bh
SMALL_SIDE, ANGLE = 180, 20.0
LLVM = "/opt/rocm/lib/llvm/bin"


def floor_bytes(B, L, h, w, window_pixels):
    """what the fused launch has to move: per pixel of the output window the photograph's 3 bytes read and 3 L written; per low-res
    pixel x_lo (12), `rendered` (12 L) and the mask (1) once"""
    return B * window_pixels * (3 + 3 * L) + B * h * w * (12 + 12 * L) + h * w


def kernel_registers(lib_path):
    """{kernel: (vgpr, sgpr, scratch bytes)} of the affine kernels and the box kernels, from the code objects' notes; {} where the
    LLVM tools are missing"""
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        return {}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = shutil.copy(lib_path, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp)
        for f in sorted(os.listdir(tmp)):
            if not f.endswith("gfx950"):
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)], check=True, capture_output=True,
                                   text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)
                name = subprocess.run(["c++filt", get("name")], capture_output=True, text=True).stdout.strip()
                name = name.split("(")[0].replace("void ", "").replace("gcfr::", "")
                if name.startswith(("affine_", "fullres_composites_box_kernel", "ingest_box_kernel")):
                    out[name] = (int(get("vgpr_count")), int(get("sgpr_count")), int(get("private_segment_fixed_size")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullres_affine_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fullres_affine_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    from geomconsistentfr_amd import _lib, build
    from geomconsistentfr_amd import postprocess as pp
    dev = torch.device("cuda:0")
    h, w = H_LO, W_LO

    def timed(fn, n):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / n * 1e3                  # us per call

    def summary(v):
        return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}

    def alternate(legs):
        """the legs' times, interleaved"""
        for leg in legs:
            for _ in range(a.warmup):
                leg()
        t = [[] for _ in legs]
        for _ in range(a.repeats):
            for i, leg in enumerate(legs):
                t[i].append(timed(leg, a.iters))
        return [summary(v) for v in t]

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    L_ = _lib.load()
    lib = os.environ.get("GCFR_HIP_LIB") or _lib.lib_path()
    res = {"commit": commit, "library": os.path.relpath(lib, ROOT), "library_source_hash": build.source_hash()[:16],
           "device": torch.cuda.get_device_name(dev), "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup, "shape": [B, L, h, w],
           "registers": kernel_registers(lib)}

    # ---- the copy probe: what a plain device-to-device copy achieves in this run --------------------------------------------
    n_probe = 1 << 28                                         # 256 MiB read + 256 MiB written: past the Infinity Cache
    src, dst = torch.zeros(n_probe, dtype=torch.uint8, device=dev), torch.empty(n_probe, dtype=torch.uint8, device=dev)
    probe = lambda: _lib.check(L_.gcfr_copy_probe(src.data_ptr(), dst.data_ptr(), n_probe, _lib.stream_ptr(dev)), "gcfr_copy_probe")
    for _ in range(a.warmup):
        probe()
    tp = [timed(probe, a.iters) for _ in range(a.repeats)]
    res["copy_probe"] = dict(summary(tp), bytes=2 * n_probe, GBs=2 * n_probe / statistics.median(tp) / 1e3)
    del src, dst
    torch.cuda.empty_cache()

    # ---- inputs: smooth photographs with byte noise, a disc mask with the shipped grey levels on its rim ----------------------
    g = torch.Generator(device=dev).manual_seed(2)
    yy = torch.arange(HP, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(WP, device=dev, dtype=torch.float32)[None, :]
    base = 128 + 60 * torch.sin(xx / 97.0) * torch.cos(yy / 61.0)
    photo = torch.stack([(base[:, :, None] + 12 * torch.randn(HP, WP, 3, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
                         for _ in range(B)])
    rad = np.hypot(*(np.mgrid[0:h, 0:w] - np.array([h / 2, w / 2])[:, None, None]))
    mask = torch.from_numpy(np.select([rad < 90, rad < 94, rad < 98], [255, 128, 64], 0).astype(np.uint8)[None]).to(dev)

    def rendered_for(x_lo):
        gc = torch.Generator(device="cpu").manual_seed(L)
        return (x_lo.permute(0, 3, 1, 2)[:, None].cpu() * (0.4 + 1.2 * torch.rand(B, L, 3, h, w, generator=gc))).to(dev).contiguous()

    x0, y0, bw, bh = LARGE
    cx, cy = x0 + bw / 2.0, y0 + bh / 2.0
    maps = {"aligned": pp.affine_from_rotated_box(cx, cy, bw, bh, 0.0, (h, w)),
            "turned": pp.affine_from_rotated_box(cx, cy, bw, bh, ANGLE, (h, w)),
            "small_turned": pp.affine_from_rotated_box(cx, cy, SMALL_SIDE, SMALL_SIDE, ANGLE, (h, w))}
    out_a = torch.empty((B, L, HP, WP, 3), dtype=torch.uint8, device=dev)
    out_b = torch.empty((B, L, HP, WP, 3), dtype=torch.uint8, device=dev)
    n_full = floor_bytes(B, L, h, w, HP * WP)
    res["floor_bytes"], res["cases"], res["ingest"] = n_full, {}, {}
    with torch.no_grad():
        # (a) against the box kernel on its own ground, alternating
        x_box = pp.ingest_box_device(photo, LARGE, (h, w))
        rendered = rendered_for(x_box)
        box_leg = lambda: pp.fullres_box_composites_device(photo, LARGE, x_box, rendered, mask, paste=True, out=out_a)
        aff_leg = lambda: pp.fullres_affine_composites_device(photo, maps["aligned"], x_box, rendered, mask, out=out_b)
        differ = int((box_leg() != aff_leg()).sum())
        tb, ta = alternate([box_leg, aff_leg])
        Fq, Iq = pp.quantise_affine(maps["aligned"])
        res["cases"]["aligned"] = {"box": tb, "affine": ta, "bytes_that_differ": differ, "bytes": int(out_a.numel()),
                                   "K_in": pp.affine_sub_samples(Fq), "K_out": pp.affine_sub_samples(Iq)}
        x_aff = pp.ingest_affine_device(photo, maps["aligned"], (h, w))
        res["ingest"]["max_abs_difference_to_the_box_ingest"] = float((x_aff - x_box).abs().max())
        ib, ia = alternate([lambda: pp.ingest_box_device(photo, LARGE, (h, w)), lambda: pp.ingest_affine_device(photo, maps["aligned"], (h, w))])
        res["ingest"]["box"], res["ingest"]["aligned"] = ib, ia
        print("aligned done", file=sys.stderr, flush=True)
        # (b), (c) the turned faces
        for name in ("turned", "small_turned"):
            Fq, Iq = pp.quantise_affine(maps[name])
            x_lo = pp.ingest_affine_device(photo, maps[name], (h, w))
            rendered = rendered_for(x_lo)
            leg = lambda: pp.fullres_affine_composites_device(photo, maps[name], x_lo, rendered, mask, out=out_b)
            relit = int((leg() != photo[:, None]).any(dim=-1).sum())
            (t,) = alternate([leg])
            (ti,) = alternate([lambda: pp.ingest_affine_device(photo, maps[name], (h, w))])
            res["cases"][name] = {"affine": t, "K_in": pp.affine_sub_samples(Fq), "K_out": pp.affine_sub_samples(Iq), "pixels_relit": relit}
            res["ingest"][name] = ti
            print("%s done" % name, file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    Bf, Lf, h, w = res["shape"]
    cmd = "python tools/fullres_affine_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda v: "%.1f (%.1f .. %.1f)" % (v["median_us"], v["min_us"], v["max_us"])
    p = res["copy_probe"]
    n = res["floor_bytes"]
    rate = lambda v: "%.0f GB/s | %.1f %%" % (n / v["median_us"] / 1e3, 100.0 * n / v["median_us"] / 1e3 / p["GBs"])
    row = lambda label, v: "| %s | %s | %.1f MB | %s |" % (label, fmt(v), n / 1e6, rate(v))
    head = ["| leg | us per call | floor | achieved | of the copy probe |", "|---|---:|---:|---:|---:|"]
    x0, y0, bw, bh = LARGE
    c = res["cases"]
    lines = ["# Relighting a rotated face through an affine map: the affine kernels (one MI355X)", "",
             "`%s` (%slibrary `%s`, source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library"], res["library_source_hash"],
                                     res["device"]), "",
             "The legs of a case alternate A, B, A, B, ...: %d repeats of %d calls between two in-stream events behind a device "
             "synchronise, after %d untimed calls per leg.  Median and (min .. max) of the repeats, microseconds per CALL, including what "
             "the host does per call (checks, the quantisation of the matrix, launches; the outputs are written into one preallocated "
             "buffer per leg).  Kernel times were not traced separately.  Nothing here is a gate." % (a.repeats, a.iters, a.warmup), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call) in the same run: %s us per call, %.0f GB/s read + "
             "write." % (p["bytes"] // 2 >> 20, fmt(p), p["GBs"]), "",
             "%d faces, %d lights, the network at %d x %d, photographs of %d x %d; every leg writes the whole photograph for every light.  "
             "Smooth photographs with byte noise, a disc mask whose rim carries the shipped masks' grey levels, `rendered` = x_lo times a "
             "random factor in [0.4, 1.6).  `floor` is what a launch has to move (per pixel of the photograph 3 bytes read and 3 L "
             "written; per low-resolution pixel 12 + 12 L + 1 once); `achieved` is that over the median, and beside it its share of the "
             "copy probe's rate." % (Bf, Lf, h, w, WP, HP), "",
             "## (a) The price of the affine map on the box kernel's ground: the %d x %d box at (%d, %d)" % (bw, bh, x0, y0), "",
             "Leg A is `fullres_box_composites_device(paste=True)` on the box, leg B `fullres_affine_composites_device` on the box's "
             "axis-aligned map (K = %d on the way out).  At this ratio the inverse map is rounded to 2^-14, so the two need not agree: "
             "%d of %d bytes differ (reported, not asserted)." % (c["aligned"]["K_out"], c["aligned"]["bytes_that_differ"], c["aligned"]["bytes"]), ""]
    lines += head + [row("A: box kernel", c["aligned"]["box"]), row("B: affine kernel, angle 0", c["aligned"]["affine"]), "",
                     "B over A: %.3f." % (c["aligned"]["affine"]["median_us"] / c["aligned"]["box"]["median_us"]), "",
                     "## (b), (c) Turned by %g degrees" % ANGLE, ""] + head + [
                     row("(b) the %d x %d box turned (K = %d out; %d pixels changed over all faces and lights)" % (bw, bh, c["turned"]["K_out"], c["turned"]["pixels_relit"]),
                         c["turned"]["affine"]),
                     row("(c) a %d-pixel face turned (K = %d out; %d pixels changed over all faces and lights)" % (SMALL_SIDE, c["small_turned"]["K_out"],
                                                                                      c["small_turned"]["pixels_relit"]), c["small_turned"]["affine"]), "",
                     "(b) over (a) B: %.3f; (c) over (a) B: %.3f." % (c["turned"]["affine"]["median_us"] / c["aligned"]["affine"]["median_us"],
                                                                       c["small_turned"]["affine"]["median_us"] / c["aligned"]["affine"]["median_us"]), "",
                     "## (d) The ingests", "",
                     "On the axis-aligned map the affine ingest samples %d x %d sub-samples bilinearly where the box ingest takes the exact "
                     "area mean: the largest difference of the two inputs is %.3g." % (c["aligned"]["K_in"], c["aligned"]["K_in"],
                                                                                       res["ingest"]["max_abs_difference_to_the_box_ingest"]), "",
                     "| ingest | us per call |", "|---|---:|"]
    for label, key in (("`ingest_box_device`, the %d x %d box" % (bw, bh), "box"),
                       ("`ingest_affine_device`, its map (K = %d)" % c["aligned"]["K_in"], "aligned"),
                       ("`ingest_affine_device`, the box turned (K = %d)" % c["turned"]["K_in"], "turned"),
                       ("`ingest_affine_device`, the %d-pixel face turned (K = %d)" % (SMALL_SIDE, c["small_turned"]["K_in"]), "small_turned")):
        lines.append("| %s | %s |" % (label, fmt(res["ingest"][key])))
    lines += ["", "## Registers", ""]
    if res["registers"]:
        lines += ["Read from the library's code objects.", "", "| kernel | VGPRs | SGPRs | scratch bytes |", "|---|---:|---:|---:|"]
        lines += ["| `%s` | %d | %d | %d |" % ((k,) + tuple(v)) for k, v in sorted(res["registers"].items())]
    else:
        lines += ["The LLVM tools were not found: see `tests/test_fullres_affine_resources.py`, which prints the counts."]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
