#!/usr/bin/env python
"""A/B of the any-size box kernels (csrc/gcfr_fullres_anybox.hip; postprocess.ingest_anybox_device /
fullres_anybox_composites_device) at 8 faces, 11 lights and a network of 256 x 256, in photographs of 3000 x 2000 (Wp x Hp).

  (a) a small face   a 180 x 170 box (bw x bh) at (1037, 571): both axes shorter than the network's, with paste=False (the box
             alone) and with paste=True (the whole photograph written for every light: nearly all of it the copy outside the box)
  (b) a mixed box    300 x 200 at the same origin: the columns are lerped, the rows averaged; paste both ways
  (c) the price of generality on the old ground   the 900 x 860 box of tools/fullres_box_ab.py:
             leg A   postprocess.fullres_box_composites_device
             leg B   postprocess.fullres_anybox_composites_device: the same bytes (checked) from the kernel that also branches on
                     the axis modes; paste both ways
  (d) the ingests    ingest_anybox_device on the three boxes and ingest_box_device on the 900 x 860 one (the same bits, checked)

Nothing is gated on speed: these are figures.  Each composite's achieved bytes per second over its byte floor (`floor_bytes`: per
pixel of the output window 3 bytes read and 3 L written, the low-resolution planes once) stand beside the rate of the library's
copy probe (gcfr_copy_probe, read + write) measured in the same run.  The kernels' register counts are read from the library's code
objects where the LLVM tools are installed.

The protocol is tools/fullres_box_ab.py's: one process, one device, no profiler attached.  The legs of a case ALTERNATE (A, B, A, B,
...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after `--warmup` untimed calls per
leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and include what the
host does per call (checks, launches).  Needs a GPU: there is no fallback.  Writes the table as Markdown to `--out` (default
profiles/fullres_anybox_ab.md) and prints the numbers as JSON.

usage: tools/fullres_anybox_ab.py [--repeats 7] [--iters 10] [--warmup 3] [--out PATH]"""
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
SMALL = (1037, 571, 180, 170)                                 # x0, y0, bw, bh
MIXED = (1037, 571, 300, 200)
LARGE = (1037, 571, 900, 860)
LLVM = "/opt/rocm/lib/llvm/bin"


def floor_bytes(B, L, h, w, window_pixels):
    """what the fused launch has to move: per pixel of the output window the photograph's 3 bytes read and 3 L written; per low-res
    pixel x_lo (12), `rendered` (12 L) and the mask (1) once"""
    return B * window_pixels * (3 + 3 * L) + B * h * w * (12 + 12 * L) + h * w


def kernel_registers(lib_path):
    """{kernel: (vgpr, sgpr, scratch bytes)} of the any-size box kernels and the box kernels, from the code objects' notes; {} where
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
                if name.startswith(("anybox_", "fullres_composites_box_kernel", "ingest_box_kernel")):
                    out[name] = (int(get("vgpr_count")), int(get("sgpr_count")), int(get("private_segment_fixed_size")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullres_anybox_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fullres_anybox_ab.py needs a GPU (a timing taken anywhere else says nothing)")
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

    out_full = torch.empty((B, L, HP, WP, 3), dtype=torch.uint8, device=dev)
    res["boxes"], res["ingest"] = {}, {}
    with torch.no_grad():
        for name, box in (("small", SMALL), ("mixed", MIXED), ("large", LARGE)):
            x0, y0, bw, bh = box
            x_lo = pp.ingest_anybox_device(photo, box, (h, w))
            rendered = rendered_for(x_lo)
            out_box = torch.empty((B, L, bh, bw, 3), dtype=torch.uint8, device=dev)
            alone = lambda: pp.fullres_anybox_composites_device(photo, box, x_lo, rendered, mask, paste=False, out=out_box)
            pasted = lambda: pp.fullres_anybox_composites_device(photo, box, x_lo, rendered, mask, paste=True, out=out_full)
            consistent = bool(torch.equal(alone(), pasted()[:, :, y0:y0 + bh, x0:x0 + bw]))
            n0, n1 = floor_bytes(B, L, h, w, bh * bw), floor_bytes(B, L, h, w, HP * WP)
            r = {"box": list(box), "alone_floor_bytes": n0, "pasted_floor_bytes": n1, "alone_is_the_pasted_box_region": consistent}
            if name == "large":                                # against the box entry, alternating
                old_alone = lambda: pp.fullres_box_composites_device(photo, box, x_lo, rendered, mask, paste=False, out=out_box)
                old_pasted = lambda: pp.fullres_box_composites_device(photo, box, x_lo, rendered, mask, paste=True, out=out_full)
                r["same_bytes"] = bool(torch.equal(old_alone().clone(), alone())) and bool(torch.equal(old_pasted().clone(), pasted()))
                r["box_alone"], r["alone"] = alternate([old_alone, alone])
                r["box_pasted"], r["pasted"] = alternate([old_pasted, pasted])
                xb = pp.ingest_box_device(photo, box, (h, w))
                same_bits = bool(torch.equal(xb.view(torch.int32), x_lo.view(torch.int32)))
                ib, ia = alternate([lambda: pp.ingest_box_device(photo, box, (h, w)), lambda: pp.ingest_anybox_device(photo, box, (h, w))])
                res["ingest"]["large_box_entry"] = {"t": ib, "bytes": B * bh * bw * 3 + B * h * w * 12, "same_bits": same_bits}
            else:
                r["alone"], r["pasted"] = alternate([alone, pasted])
                (ia,) = alternate([lambda: pp.ingest_anybox_device(photo, box, (h, w))])
            res["ingest"][name] = {"t": ia, "bytes": B * bh * bw * 3 + B * h * w * 12}
            res["boxes"][name] = r
            print("%s done" % name, file=sys.stderr, flush=True)
            del out_box, rendered, x_lo
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    Bf, Lf, h, w = res["shape"]
    cmd = "python tools/fullres_anybox_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda v: "%.1f (%.1f .. %.1f)" % (v["median_us"], v["min_us"], v["max_us"])
    p = res["copy_probe"]
    rate = lambda nbytes, v: "%.0f GB/s | %.1f %%" % (nbytes / v["median_us"] / 1e3, 100.0 * nbytes / v["median_us"] / 1e3 / p["GBs"])
    row = lambda label, v, nbytes: "| %s | %s | %.1f MB | %s |" % (label, fmt(v), nbytes / 1e6, rate(nbytes, v))
    head = ["| leg | us per call | floor | achieved | of the copy probe |", "|---|---:|---:|---:|---:|"]
    lines = ["# Relighting a face box of any size inside a larger photograph: the any-size box kernels (one MI355X)", "",
             "`%s` (%slibrary `%s`, source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library"], res["library_source_hash"],
                                     res["device"]), "",
             "The legs of a case alternate A, B, A, B, ...: %d repeats of %d calls between two in-stream events behind a device "
             "synchronise, after %d untimed calls per leg.  Median and (min .. max) of the repeats, microseconds per CALL, including what "
             "the host does per call (checks, launches; the outputs are written into one preallocated buffer per leg).  Kernel times were "
             "not traced separately.  Nothing here is a gate." % (a.repeats, a.iters, a.warmup), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call) in the same run: %s us per call, %.0f GB/s read + "
             "write." % (p["bytes"] // 2 >> 20, fmt(p), p["GBs"]), "",
             "%d faces, %d lights, the network at %d x %d, photographs of %d x %d.  Smooth photographs with byte noise, a disc mask whose "
             "rim carries the shipped masks' grey levels, `rendered` = x_lo times a random factor in [0.4, 1.6).  `floor` is what a launch "
             "has to move (per pixel of the output window 3 bytes read and 3 L written; per low-resolution pixel 12 + 12 L + 1 once); "
             "`achieved` is that over the median, and beside it its share of the copy probe's rate.  With a small box alone the floor is "
             "mostly the low-resolution planes, which every box pixel reads many times over: the share says little there."
             % (Bf, Lf, h, w, WP, HP), ""]
    for tag, name, what in (("(a)", "small", "both axes shorter than the network's"), ("(b)", "mixed", "the columns lerped, the rows averaged")):
        r = res["boxes"][name]
        x0, y0, bw, bh = r["box"]
        lines += ["## %s A %d x %d box at (%d, %d): %s" % (tag, bw, bh, x0, y0, what), "",
                  "The box alone is the pasted output's box region: %s." % r["alone_is_the_pasted_box_region"], ""] + head + [
                  row("paste=False", r["alone"], r["alone_floor_bytes"]), row("paste=True", r["pasted"], r["pasted_floor_bytes"]), ""]
    r = res["boxes"]["large"]
    x0, y0, bw, bh = r["box"]
    lines += ["## (c) The price of generality on the old ground: the %d x %d box" % (bw, bh), "",
              "Leg A is `fullres_box_composites_device`, leg B `fullres_anybox_composites_device`.  The two return the same bytes: %s."
              % r["same_bytes"], ""] + head + [
              row("A: box kernel, paste=False", r["box_alone"], r["alone_floor_bytes"]),
              row("B: any-size kernel, paste=False", r["alone"], r["alone_floor_bytes"]),
              row("A: box kernel, paste=True", r["box_pasted"], r["pasted_floor_bytes"]),
              row("B: any-size kernel, paste=True", r["pasted"], r["pasted_floor_bytes"]), "",
              "B over A: %.3f alone, %.3f pasted." % (r["alone"]["median_us"] / r["box_alone"]["median_us"],
                                                     r["pasted"]["median_us"] / r["box_pasted"]["median_us"]), "",
              "## (d) The ingests", "",
              "On the %d x %d box `ingest_anybox_device` returns `ingest_box_device`'s bits: %s.  Bytes are the box's read plus the "
              "network's input written." % (bw, bh, res["ingest"]["large_box_entry"]["same_bits"]), "",
              "| ingest | us per call | bytes | achieved | of the copy probe |", "|---|---:|---:|---:|---:|"]
    for label, key in (("`ingest_anybox_device`, 180 x 170", "small"), ("`ingest_anybox_device`, 300 x 200", "mixed"),
                       ("`ingest_anybox_device`, 900 x 860", "large"), ("`ingest_box_device`, 900 x 860", "large_box_entry")):
        v = res["ingest"][key]
        lines.append(row(label, v["t"], v["bytes"]))
    lines += ["", "## Registers", ""]
    if res["registers"]:
        lines += ["Read from the library's code objects.", "", "| kernel | VGPRs | SGPRs | scratch bytes |", "|---|---:|---:|---:|"]
        lines += ["| `%s` | %d | %d | %d |" % ((n,) + tuple(v)) for n, v in sorted(res["registers"].items())]
    else:
        lines += ["The LLVM tools were not found: see `tests/test_fullres_anybox_resources.py`, which prints the counts."]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
