#!/usr/bin/env python
"""A/B of the box kernels (csrc/gcfr_fullres_box.hip; postprocess.ingest_box_device / fullres_box_composites_device) at 8 faces,
11 lights and a network of 256 x 256.

  (a) the price of the general taps   the box is a whole 1024 x 1024 photograph:
             leg A   postprocess.fullres_composites_device at s = 4 (shifts, a shared column window, weights that are constants)
             leg B   postprocess.fullres_box_composites_device on the box (0, 0, 1024, 1024): the same bytes (checked) from integer
                     divisions, one f64 division per weight and each pixel's own taps
  (b) a detector's box   900 x 860 (bw x bh) at (1037, 571) in photographs of 3000 x 2000 (Wp x Hp), with paste=False (the box
             alone) and with paste=True (the whole photograph written for every light)
  (c) the two ingests   ingest_photographs_device at s = 4 against ingest_box_device on the same whole photograph (the same bits,
             checked), and ingest_box_device on the 900 x 860 box

Nothing is gated on speed: these are figures.  Each composite's achieved bytes per second over its byte floor (`floor_bytes`: per
pixel of the output window 3 bytes read and 3 L written, the low-resolution planes once) stand beside the rate of the library's
copy probe (gcfr_copy_probe, read + write) measured in the same run.  The kernels' register counts are read from the library's code
objects where the LLVM tools are installed.

The protocol is tools/fullres_ab.py's: one process, one device, no profiler attached.  The legs of a case ALTERNATE (A, B, A, B,
...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after `--warmup` untimed calls per
leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and include what the
host does per call (checks, allocation of outputs, launches).  Needs a GPU: there is no fallback.  Writes the table as Markdown to
`--out` (default profiles/fullres_box_ab.md) and prints the numbers as JSON.

usage: tools/fullres_box_ab.py [--repeats 7] [--iters 10] [--warmup 3] [--out PATH]"""
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

B, L, H_LO, W_LO, SCALE = 8, 11, 256, 256, 4
HP, WP = 2000, 3000
BOX = (1037, 571, 900, 860)                                   # x0, y0, bw, bh
LLVM = "/opt/rocm/lib/llvm/bin"


def floor_bytes(B, L, h, w, window_pixels):
    """what the fused launch has to move: per pixel of the output window the photograph's 3 bytes read and 3 L written; per low-res
    pixel x_lo (12), `rendered` (12 L) and the mask (1) once"""
    return B * window_pixels * (3 + 3 * L) + B * h * w * (12 + 12 * L) + h * w


def kernel_registers(lib_path):
    """{kernel: (vgpr, sgpr, scratch bytes)} of the box kernels and the power-of-two composite, from the code objects' notes; {} where
    the LLVM tools are missing"""
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
                if name.startswith(("fullres_composites_box_kernel", "ingest_box_kernel", "fullres_composites_kernel<4", "ingest_photographs_kernel<4")):
                    out[name] = (int(get("vgpr_count")), int(get("sgpr_count")), int(get("private_segment_fixed_size")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullres_box_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fullres_box_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    from geomconsistentfr_amd import _lib, build
    from geomconsistentfr_amd import postprocess as pp
    dev = torch.device("cuda:0")
    h, w, s = H_LO, W_LO, SCALE

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
    res = {"commit": commit, "library": os.path.relpath(os.environ.get("GCFR_HIP_LIB") or _lib.lib_path(), ROOT),
           "library_source_hash": build.source_hash()[:16], "device": torch.cuda.get_device_name(dev), "repeats": a.repeats,
           "iters": a.iters, "warmup": a.warmup, "shape": [B, L, h, w], "registers": kernel_registers(os.environ.get("GCFR_HIP_LIB") or _lib.lib_path())}

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
    def photographs(Hp, Wp, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        yy = torch.arange(Hp, device=dev, dtype=torch.float32)[:, None]
        xx = torch.arange(Wp, device=dev, dtype=torch.float32)[None, :]
        base = 128 + 60 * torch.sin(xx / 97.0) * torch.cos(yy / 61.0)
        return torch.stack([(base[:, :, None] + 12 * torch.randn(Hp, Wp, 3, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
                            for _ in range(B)])

    rad = np.hypot(*(np.mgrid[0:h, 0:w] - np.array([h / 2, w / 2])[:, None, None]))
    mask = torch.from_numpy(np.select([rad < 90, rad < 94, rad < 98], [255, 128, 64], 0).astype(np.uint8)[None]).to(dev)

    def rendered_for(x_lo):
        g = torch.Generator(device="cpu").manual_seed(L)
        return (x_lo.permute(0, 3, 1, 2)[:, None].cpu() * (0.4 + 1.2 * torch.rand(B, L, 3, h, w, generator=g))).to(dev).contiguous()

    with torch.no_grad():
        # ---- (a) and the first half of (c): the whole 1024 x 1024 photograph ----------------------------------------------------
        photo = photographs(s * h, s * w, 1)
        whole = (0, 0, s * w, s * h)
        x_lo = pp.ingest_photographs_device(photo, s)
        same_bits = bool(torch.equal(x_lo.view(torch.int32), pp.ingest_box_device(photo, whole, (h, w)).view(torch.int32)))
        rendered = rendered_for(x_lo)
        out = torch.empty((B, L, s * h, s * w, 3), dtype=torch.uint8, device=dev)
        leg_a = lambda: pp.fullres_composites_device(photo, x_lo, rendered, mask, s, out=out)
        leg_b = lambda: pp.fullres_box_composites_device(photo, whole, x_lo, rendered, mask, out=out)
        same_bytes = bool(torch.equal(leg_a().clone(), leg_b()))
        ta, tb = alternate([leg_a, leg_b])
        nb = floor_bytes(B, L, h, w, s * h * s * w)
        res["whole"] = {"power_of_two": ta, "box": tb, "floor_bytes": nb, "power_of_two_GBs": nb / ta["median_us"] / 1e3,
                        "box_GBs": nb / tb["median_us"] / 1e3, "same_bytes": same_bytes}
        print("(a) done", file=sys.stderr, flush=True)
        ia, ib = alternate([lambda: pp.ingest_photographs_device(photo, s), lambda: pp.ingest_box_device(photo, whole, (h, w))])
        ingest_bytes = B * s * h * s * w * 3 + B * h * w * 12
        res["ingest_whole"] = {"power_of_two": ia, "box": ib, "bytes": ingest_bytes, "same_bits": same_bits}
        del photo, out, rendered, x_lo
        torch.cuda.empty_cache()

        # ---- (b) and the second half of (c): a 900 x 860 box in 3000 x 2000 photographs -----------------------------------------
        photo = photographs(HP, WP, 2)
        x0, y0, bw, bh = BOX
        x_lo = pp.ingest_box_device(photo, BOX, (h, w))
        rendered = rendered_for(x_lo)
        out_box = torch.empty((B, L, bh, bw, 3), dtype=torch.uint8, device=dev)
        out_full = torch.empty((B, L, HP, WP, 3), dtype=torch.uint8, device=dev)
        alone = lambda: pp.fullres_box_composites_device(photo, BOX, x_lo, rendered, mask, paste=False, out=out_box)
        pasted = lambda: pp.fullres_box_composites_device(photo, BOX, x_lo, rendered, mask, paste=True, out=out_full)
        consistent = bool(torch.equal(alone(), pasted()[:, :, y0:y0 + bh, x0:x0 + bw]))
        t0, t1 = alternate([alone, pasted])
        n0, n1 = floor_bytes(B, L, h, w, bh * bw), floor_bytes(B, L, h, w, HP * WP)
        res["detector_box"] = {"alone": t0, "pasted": t1, "alone_floor_bytes": n0, "pasted_floor_bytes": n1,
                               "alone_GBs": n0 / t0["median_us"] / 1e3, "pasted_GBs": n1 / t1["median_us"] / 1e3,
                               "alone_is_the_pasted_box_region": consistent}
        print("(b) done", file=sys.stderr, flush=True)
        (ic,) = alternate([lambda: pp.ingest_box_device(photo, BOX, (h, w))])
        res["ingest_box"] = {"box": ic, "bytes": B * bh * bw * 3 + B * h * w * 12}
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    Bf, Lf, h, w = res["shape"]
    cmd = "python tools/fullres_box_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda v: "%.1f (%.1f .. %.1f)" % (v["median_us"], v["min_us"], v["max_us"])
    p, wh, db, iw, ibx = res["copy_probe"], res["whole"], res["detector_box"], res["ingest_whole"], res["ingest_box"]
    rate = lambda g: "%.0f GB/s | %.1f %%" % (g, 100.0 * g / p["GBs"])
    x0, y0, bw, bh = BOX
    lines = ["# Relighting a face box inside a larger photograph: the box kernels beside the power-of-two ones (one MI355X)", "",
             "`%s` (%slibrary `%s`, source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library"], res["library_source_hash"],
                                     res["device"]), "",
             "The legs of a case alternate A, B, A, B, ...: %d repeats of %d calls between two in-stream events behind a device "
             "synchronise, after %d untimed calls per leg.  Median and (min .. max) of the repeats, microseconds per CALL, including what "
             "the host does per call (checks, launches; the outputs are written into one preallocated buffer per leg).  Kernel times were "
             "not traced separately.  Nothing here is a gate." % (a.repeats, a.iters, a.warmup), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call) in the same run: %s us per call, %.0f GB/s read + "
             "write." % (p["bytes"] // 2 >> 20, fmt(p), p["GBs"]), "",
             "%d faces, %d lights, the network at %d x %d.  Smooth photographs with byte noise, a disc mask whose rim carries the shipped "
             "masks' grey levels, `rendered` = x_lo times a random factor in [0.4, 1.6).  `floor` is what a launch has to move (per pixel of "
             "the output window 3 bytes read and 3 L written; per low-resolution pixel 12 + 12 L + 1 once); `achieved` is that over the "
             "median, and beside it its share of the copy probe's rate." % (Bf, Lf, h, w), "",
             "## (a) The price of the general taps: the box is a whole %d x %d photograph" % (SCALE * w, SCALE * h), "",
             "Leg A is `fullres_composites_device` at s = %d, leg B `fullres_box_composites_device` on the box (0, 0, %d, %d).  The two "
             "return the same bytes: %s." % (SCALE, SCALE * w, SCALE * h, wh["same_bytes"]), "",
             "| leg | us per call | floor | achieved | of the copy probe |", "|---|---:|---:|---:|---:|",
             "| A: power-of-two kernel | %s | %.1f MB | %s |" % (fmt(wh["power_of_two"]), wh["floor_bytes"] / 1e6, rate(wh["power_of_two_GBs"])),
             "| B: box kernel | %s | %.1f MB | %s |" % (fmt(wh["box"]), wh["floor_bytes"] / 1e6, rate(wh["box_GBs"])),
             "", "B over A: %.3f." % (wh["box"]["median_us"] / wh["power_of_two"]["median_us"]), "",
             "## (b) A %d x %d box at (%d, %d) in photographs of %d x %d" % (bw, bh, x0, y0, WP, HP), "",
             "`paste=False` writes the box alone, `paste=True` the whole photograph for every light; outside the box a lane copies its "
             "three dwords per light.  The box alone is the pasted output's box region: %s." % db["alone_is_the_pasted_box_region"], "",
             "| leg | us per call | floor | achieved | of the copy probe |", "|---|---:|---:|---:|---:|",
             "| paste=False | %s | %.1f MB | %s |" % (fmt(db["alone"]), db["alone_floor_bytes"] / 1e6, rate(db["alone_GBs"])),
             "| paste=True | %s | %.1f MB | %s |" % (fmt(db["pasted"]), db["pasted_floor_bytes"] / 1e6, rate(db["pasted_GBs"])),
             "", "## (c) The two ingests", "",
             "On the whole %d x %d photograph `ingest_box_device` returns `ingest_photographs_device`'s bits: %s.  Bytes are the box's read "
             "plus the network's input written." % (SCALE * w, SCALE * h, iw["same_bits"]), "",
             "| ingest | us per call | bytes | achieved | of the copy probe |", "|---|---:|---:|---:|---:|",
             "| `ingest_photographs_device`, s = %d | %s | %.1f MB | %s |" % (SCALE, fmt(iw["power_of_two"]), iw["bytes"] / 1e6,
                                                                            rate(iw["bytes"] / iw["power_of_two"]["median_us"] / 1e3)),
             "| `ingest_box_device`, the same photograph | %s | %.1f MB | %s |" % (fmt(iw["box"]), iw["bytes"] / 1e6,
                                                                                  rate(iw["bytes"] / iw["box"]["median_us"] / 1e3)),
             "| `ingest_box_device`, the %d x %d box | %s | %.1f MB | %s |" % (bw, bh, fmt(ibx["box"]), ibx["bytes"] / 1e6,
                                                                             rate(ibx["bytes"] / ibx["box"]["median_us"] / 1e3)),
             "", "## Registers", ""]
    if res["registers"]:
        lines += ["Read from the library's code objects.", "", "| kernel | VGPRs | SGPRs | scratch bytes |", "|---|---:|---:|---:|"]
        lines += ["| `%s` | %d | %d | %d |" % ((n,) + tuple(v)) for n, v in sorted(res["registers"].items())]
    else:
        lines += ["The LLVM tools were not found: see `tests/test_fullres_box_resources.py`, which prints the counts."]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
