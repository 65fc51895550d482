#!/usr/bin/env python
"""A/B of the guided box kernel (csrc/gcfr_fullres_box_guided.hip; postprocess.fullres_box_composites_device(upsample="guided")) at
8 faces, 11 lights and a network of 256 x 256.

  (a) the price of the general taps   the box is a whole 1024 x 1024 photograph:
             leg A   postprocess.fullres_composites_device(upsample="guided") at s = 4 (shifts, a shared column window per lane,
                     exact weights, the next light's window requested ahead)
             leg B   postprocess.fullres_box_composites_device(upsample="guided") on the box (0, 0, 1024, 1024): the same bytes
                     (checked) from integer divisions, one f64 division per weight and each pixel's own 16 taps
  (b) the price of the edge-aware upsample on a detector's box   900 x 860 (bw x bh) at (1037, 571) in photographs of 3000 x 2000
             (Wp x Hp), paste both ways: the bilinear box entry against the guided one
  (c) a sweep of the ratio   whole photographs of 2, 3, 3.5, 4 and 5 times the network's side, the bilinear box entry against the
             guided one: does the bilinear box kernel's step at a horizontal ratio of 4 show here too

Nothing is gated on speed: these are figures.  Each composite's achieved bytes per second over its byte floor (`floor_bytes`: per
pixel of the output window 3 bytes read and 3 L written, the low-resolution planes once) stand beside the rate of the library's
copy probe (gcfr_copy_probe, read + write) measured in the same run.  The kernels' register counts are read from the library's code
objects where the LLVM tools are installed.

The protocol is tools/fullres_box_ab.py's: one process, one device, no profiler attached.  The legs of a case ALTERNATE (A, B, A,
B, ...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after `--warmup` untimed calls
per leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and include what
the host does per call (checks, launches).  Needs a GPU: there is no fallback.  Writes the table as Markdown to `--out` (default
profiles/fullres_box_guided_ab.md) and prints the numbers as JSON.

usage: tools/fullres_box_guided_ab.py [--repeats 7] [--iters 10] [--warmup 3] [--out PATH]"""
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
SWEEP = (512, 768, 896, 1024, 1280)                           # the photograph's side: 2, 3, 3.5, 4, 5 times the network's
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("fullres_composites_box_guided_kernel", "fullres_composites_box_kernel", "fullres_composites_guided_kernel<4")


def floor_bytes(B, L, h, w, window_pixels):
    """what the fused launch has to move: per pixel of the output window the photograph's 3 bytes read and 3 L written; per low-res
    pixel x_lo (12), `rendered` (12 L) and the mask (1) once"""
    return B * window_pixels * (3 + 3 * L) + B * h * w * (12 + 12 * L) + h * w


def kernel_registers(lib_path):
    """{kernel: (vgpr, agpr, sgpr, scratch bytes, lds bytes)} of the guided box kernels and their two parents, from the code
    objects' notes; {} where the LLVM tools are missing"""
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
                if name.startswith(KERNELS):
                    out[name] = (int(get("vgpr_count")), int(blk.split()[0]), int(get("sgpr_count")), int(get("private_segment_fixed_size")),
                                 int(get("group_segment_fixed_size")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullres_box_guided_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fullres_box_guided_ab.py needs a GPU (a timing taken anywhere else says nothing)")
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

    box_entry = pp.fullres_box_composites_device
    with torch.no_grad():
        # ---- (a) and (c): whole photographs --------------------------------------------------------------------------------------
        res["sweep"] = []
        for side in SWEEP:
            photo = photographs(side, side, 1)
            whole = (0, 0, side, side)
            x_lo = pp.ingest_box_device(photo, whole, (h, w))
            rendered = rendered_for(x_lo)
            out = torch.empty((B, L, side, side, 3), dtype=torch.uint8, device=dev)
            bilinear = lambda: box_entry(photo, whole, x_lo, rendered, mask, out=out)
            guided = lambda: box_entry(photo, whole, x_lo, rendered, mask, out=out, upsample="guided")
            nb = floor_bytes(B, L, h, w, side * side)
            if side == s * w:
                leg_a = lambda: pp.fullres_composites_device(photo, x_lo, rendered, mask, s, out=out, upsample="guided")
                same_bytes = bool(torch.equal(leg_a().clone(), guided()))
                ta, tb = alternate([leg_a, guided])
                res["whole"] = {"power_of_two": ta, "box": tb, "floor_bytes": nb, "power_of_two_GBs": nb / ta["median_us"] / 1e3,
                                "box_GBs": nb / tb["median_us"] / 1e3, "same_bytes": same_bytes}
                print("(a) done", file=sys.stderr, flush=True)
            t0, t1 = alternate([bilinear, guided])
            res["sweep"].append({"side": side, "ratio": side / w, "bilinear": t0, "guided": t1, "floor_bytes": nb,
                                 "bilinear_GBs": nb / t0["median_us"] / 1e3, "guided_GBs": nb / t1["median_us"] / 1e3})
            print("(c) side %d done" % side, file=sys.stderr, flush=True)
            del photo, out, rendered, x_lo
            torch.cuda.empty_cache()

        # ---- (b): a 900 x 860 box in 3000 x 2000 photographs ---------------------------------------------------------------------
        photo = photographs(HP, WP, 2)
        x0, y0, bw, bh = BOX
        x_lo = pp.ingest_box_device(photo, BOX, (h, w))
        rendered = rendered_for(x_lo)
        out_box = torch.empty((B, L, bh, bw, 3), dtype=torch.uint8, device=dev)
        out_full = torch.empty((B, L, HP, WP, 3), dtype=torch.uint8, device=dev)
        legs = [lambda: box_entry(photo, BOX, x_lo, rendered, mask, paste=False, out=out_box),
                lambda: box_entry(photo, BOX, x_lo, rendered, mask, paste=False, out=out_box, upsample="guided"),
                lambda: box_entry(photo, BOX, x_lo, rendered, mask, paste=True, out=out_full),
                lambda: box_entry(photo, BOX, x_lo, rendered, mask, paste=True, out=out_full, upsample="guided")]
        consistent = bool(torch.equal(legs[1]().clone(), legs[3]()[:, :, y0:y0 + bh, x0:x0 + bw]))
        differs = int((legs[0]().clone() != legs[1]()).sum())
        t = alternate(legs)
        n0, n1 = floor_bytes(B, L, h, w, bh * bw), floor_bytes(B, L, h, w, HP * WP)
        res["detector_box"] = {"alone_bilinear": t[0], "alone_guided": t[1], "pasted_bilinear": t[2], "pasted_guided": t[3],
                               "alone_floor_bytes": n0, "pasted_floor_bytes": n1, "alone_is_the_pasted_box_region": consistent,
                               "bytes_that_differ_from_bilinear": differs, "box_bytes": out_box.numel()}
        print("(b) done", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    Bf, Lf, h, w = res["shape"]
    cmd = "python tools/fullres_box_guided_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda v: "%.1f (%.1f .. %.1f)" % (v["median_us"], v["min_us"], v["max_us"])
    p, wh, db = res["copy_probe"], res["whole"], res["detector_box"]
    rate = lambda nbytes, v: "%.0f GB/s | %.1f %%" % (nbytes / v["median_us"] / 1e3, 100.0 * nbytes / v["median_us"] / 1e3 / p["GBs"])
    x0, y0, bw, bh = BOX
    lines = ["# The edge-aware upsample over a face box: the guided box kernel beside its two parents (one MI355X)", "",
             "`%s` (%slibrary `%s`, source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library"], res["library_source_hash"],
                                     res["device"]), "",
             "The legs of a case alternate A, B, A, B, ...: %d repeats of %d calls between two in-stream events behind a device "
             "synchronise, after %d untimed calls per leg.  Median and (min .. max) of the repeats, microseconds per CALL, including what "
             "the host does per call (checks, launches; the outputs are written into one preallocated buffer per case).  Kernel times were "
             "not traced separately.  Nothing here is a gate." % (a.repeats, a.iters, a.warmup), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call) in the same run: %s us per call, %.0f GB/s read + "
             "write." % (p["bytes"] // 2 >> 20, fmt(p), p["GBs"]), "",
             "%d faces, %d lights, the network at %d x %d.  Smooth photographs with byte noise, a disc mask whose rim carries the shipped "
             "masks' grey levels, `rendered` = x_lo times a random factor in [0.4, 1.6), range_sigma = 20.  `floor` is what a launch has to "
             "move (per pixel of the output window 3 bytes read and 3 L written; per low-resolution pixel 12 + 12 L + 1 once); `achieved` "
             "is that over the median, and beside it its share of the copy probe's rate." % (Bf, Lf, h, w), "",
             "## (a) The price of the general taps: the box is a whole %d x %d photograph" % (SCALE * w, SCALE * h), "",
             "Leg A is `fullres_composites_device(upsample=\"guided\")` at s = %d, leg B `fullres_box_composites_device(upsample=\"guided\")` "
             "on the box (0, 0, %d, %d).  The two return the same bytes: %s." % (SCALE, SCALE * w, SCALE * h, wh["same_bytes"]), "",
             "| leg | us per call | floor | achieved | of the copy probe |", "|---|---:|---:|---:|---:|",
             "| A: power-of-two guided kernel | %s | %.1f MB | %s |" % (fmt(wh["power_of_two"]), wh["floor_bytes"] / 1e6, rate(wh["floor_bytes"], wh["power_of_two"])),
             "| B: guided box kernel | %s | %.1f MB | %s |" % (fmt(wh["box"]), wh["floor_bytes"] / 1e6, rate(wh["floor_bytes"], wh["box"])),
             "", "B over A: %.3f." % (wh["box"]["median_us"] / wh["power_of_two"]["median_us"]), "",
             "## (b) The price of the edge-aware upsample: a %d x %d box at (%d, %d) in photographs of %d x %d" % (bw, bh, x0, y0, WP, HP), "",
             "`paste=False` writes the box alone, `paste=True` the whole photograph for every light.  The guided box alone is the guided "
             "pasted output's box region: %s.  %d of the box's %d bytes differ between the two upsamples." %
             (db["alone_is_the_pasted_box_region"], db["bytes_that_differ_from_bilinear"], db["box_bytes"]), "",
             "| leg | us per call | floor | achieved | of the copy probe |", "|---|---:|---:|---:|---:|"]
    for key, label, nbytes in (("alone_bilinear", "paste=False, bilinear", db["alone_floor_bytes"]), ("alone_guided", "paste=False, guided", db["alone_floor_bytes"]),
                               ("pasted_bilinear", "paste=True, bilinear", db["pasted_floor_bytes"]), ("pasted_guided", "paste=True, guided", db["pasted_floor_bytes"])):
        lines.append("| %s | %s | %.1f MB | %s |" % (label, fmt(db[key]), nbytes / 1e6, rate(nbytes, db[key])))
    lines += ["", "Guided over bilinear: %.2f (paste=False), %.2f (paste=True)." %
              (db["alone_guided"]["median_us"] / db["alone_bilinear"]["median_us"], db["pasted_guided"]["median_us"] / db["pasted_bilinear"]["median_us"]), "",
              "## (c) Whole photographs of 2 to 5 times the network's side", "",
              "ns per pixel is the median over the output window's pixels of all %d faces (one pixel: %d lights)." % (Bf, Lf), "",
              "| side | ratio | bilinear box, us per call | ns per pixel | guided box, us per call | ns per pixel | achieved (guided) | of the copy probe |",
              "|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in res["sweep"]:
        px = Bf * r["side"] * r["side"]
        lines.append("| %d | %.1f | %s | %.3f | %s | %.3f | %s |" % (r["side"], r["ratio"], fmt(r["bilinear"]), 1e3 * r["bilinear"]["median_us"] / px,
                                                                   fmt(r["guided"]), 1e3 * r["guided"]["median_us"] / px, rate(r["floor_bytes"], r["guided"])))
    lines += ["", "## Registers", ""]
    if res["registers"]:
        lines += ["Read from the library's code objects.", "", "| kernel | VGPRs | of which AGPRs | SGPRs | scratch bytes | LDS bytes |", "|---|---:|---:|---:|---:|---:|"]
        lines += ["| `%s` | %d | %d | %d | %d | %d |" % ((n,) + tuple(v)) for n, v in sorted(res["registers"].items())]
    else:
        lines += ["The LLVM tools were not found: see `tests/test_fullres_box_guided_resources.py`, which prints the counts."]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
