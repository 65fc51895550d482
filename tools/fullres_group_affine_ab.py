#!/usr/bin/env python
"""A/B of the group-affine kernels (csrc/gcfr_fullres_group_affine.hip; postprocess.ingest_group_affine_device /
fullres_group_affine_composites_device) against the chain of affine calls they replace: photographs of 3000 x 2000 (Wp x Hp), a
network of 256 x 256, 11 lights and SIX tilted faces per photograph -- four of 180 x 170, one of 300 x 200 and one of 900 x 860, the
last 180 x 170 one inside the large one's relit part -- at P = 1 and at P = 8 photographs.

  composite  leg A   postprocess.fullres_group_affine_composites_device: ONE pass over each photograph's bytes
             leg B   the chain of six postprocess.fullres_affine_composites_device calls (the existing code, measured here): the first
                     face of every photograph with the photographs as its batch, which writes the (P,L,Hp,Wp,3) running images,
                     then one call per further face with the P L running images as its batch, between two buffers.  The operands of
                     the chain (maps, x_lo and `rendered` per call) are laid out before the clock starts.  The two legs return the
                     same bytes (checked).
             leg C   the same faces UPRIGHT (angle 0: axis-aligned boxes) through postprocess.fullres_group_composites_device, the
                     boxes' single pass: what the map costs over it
             leg D   the same upright faces as axis-aligned MAPS through leg A's entry
  ingest     leg A   postprocess.ingest_group_affine_device on the P photographs
             leg B   postprocess.ingest_affine_device on the gathered photo[photo_index], the gather included
             leg C   the same on photographs gathered before the clock starts

Nothing is gated on speed: these are figures.  Each leg's achieved bytes per second over the byte floor of the SINGLE pass
(`floor_bytes`: per photograph 3 Hp Wp read and 3 L Hp Wp written, the faces' low-resolution planes once) stand beside the rate of
the library's copy probe (gcfr_copy_probe, read + write) measured in the same run.  The kernels' register counts are read from the
library's code objects where the LLVM tools are installed.

The protocol is tools/fullres_group_ab.py's: one process, one device, no profiler attached.  The legs of a case ALTERNATE (A, B, C,
D, A, ...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after `--warmup` untimed calls
per leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL (leg B: per chain)
and include what the host does per call (checks, launches).  Needs a GPU: there is no fallback.  Writes the table as Markdown to
`--out` (default profiles/fullres_group_affine_ab.md) and prints the numbers as JSON.

usage: tools/fullres_group_affine_ab.py [--repeats 7] [--iters 5] [--warmup 2] [--out PATH]"""
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

L, H_LO, W_LO = 11, 256, 256
HP, WP = 2000, 3000
# x0, y0, bw, bh of the face upright (tools/fullres_group_ab.py's boxes) and its angle in degrees about the box's centre: four small
# faces, a mixed one, a large one; face 3 lies inside face 5's relit part
FACES = [(200, 300, 180, 170, 12.0), (700, 350, 180, 170, -25.0), (2200, 300, 180, 170, 33.0), (1400, 900, 180, 170, -8.0),
         (2400, 1200, 300, 200, 20.0), (1037, 571, 900, 860, -15.0)]
PHOTOS = (1, 8)
LLVM = "/opt/rocm/lib/llvm/bin"


def floor_bytes(P, B, L, h, w, Hp, Wp):
    """what the single pass has to move: per photograph its 3 Hp Wp bytes read and 3 L Hp Wp written; per face x_lo (12 per low-res
    pixel) and `rendered` (12 L) once; the shared mask once"""
    return P * Hp * Wp * (3 + 3 * L) + B * h * w * (12 + 12 * L) + h * w


def kernel_registers(lib_path):
    """{kernel: (vgpr, sgpr, scratch bytes)} of the group-affine kernels and their two parents', from the code objects' notes; {}
    where the LLVM tools are missing"""
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
                if name.startswith(("tilted_", "group_", "affine_")):
                    out[name] = (int(get("vgpr_count")), int(get("sgpr_count")), int(get("private_segment_fixed_size")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullres_group_affine_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fullres_group_affine_ab.py needs a GPU (a timing taken anywhere else says nothing)")
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
           "device": torch.cuda.get_device_name(dev), "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup,
           "shape": [len(FACES), L, h, w], "registers": kernel_registers(lib)}

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
    rad = np.hypot(*(np.mgrid[0:h, 0:w] - np.array([h / 2, w / 2])[:, None, None]))
    mask = torch.from_numpy(np.select([rad < 90, rad < 94, rad < 98], [255, 128, 64], 0).astype(np.uint8)[None]).to(dev)
    K = len(FACES)
    tilted_one = np.stack([pp.affine_from_rotated_box(x0 + bw / 2.0, y0 + bh / 2.0, bw, bh, deg, (h, w)) for x0, y0, bw, bh, deg in FACES])
    upright_one = np.stack([pp.affine_from_rotated_box(x0 + bw / 2.0, y0 + bh / 2.0, bw, bh, 0.0, (h, w)) for x0, y0, bw, bh, _ in FACES])
    res["sub_samples"] = [pp.affine_sub_samples(m) for m in pp.quantise_affine(tilted_one)[1]]
    res["cases"] = {}
    with torch.no_grad():
        for P in PHOTOS:
            photo = torch.stack([(base[:, :, None] + 12 * torch.randn(HP, WP, 3, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
                                 for _ in range(P)])
            B = P * K
            pidx = np.repeat(np.arange(P), K)                                      # face b = K q + k
            Fq, Iq = pp.quantise_affine(np.tile(tilted_one, (P, 1, 1)))
            pair = (Fq, Iq)
            up_pair = pp.quantise_affine(np.tile(upright_one, (P, 1, 1)))
            boxes = np.tile(np.array([f[:4] for f in FACES]), (P, 1))
            x_lo = pp.ingest_group_affine_device(photo, pair, pidx, (h, w))
            rendered = (x_lo.permute(0, 3, 1, 2)[:, None] * (0.4 + 1.2 * torch.rand(B, L, 3, h, w, device=dev, generator=g))).contiguous()
            out = torch.empty((P, L, HP, WP, 3), dtype=torch.uint8, device=dev)
            one = lambda: pp.fullres_group_affine_composites_device(photo, pair, pidx, x_lo, rendered, mask, out=out)
            # the chain's operands, laid out before the clock starts
            run = [torch.empty((P, L, HP, WP, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
            first = [K * q for q in range(P)]
            ops = [((Fq[first], Iq[first]), x_lo[first].contiguous(), rendered[first].contiguous())]
            for k in range(1, K):
                faces = [K * q + k for q in range(P)]
                ops.append(((np.repeat(Fq[faces], L, axis=0), np.repeat(Iq[faces], L, axis=0)),
                            x_lo[faces].repeat_interleave(L, dim=0).contiguous(), rendered[faces].reshape(P * L, 3, h, w).contiguous()))

            def chain():
                pp.fullres_affine_composites_device(photo, ops[0][0], ops[0][1], ops[0][2], mask, out=run[0])
                for k in range(1, K):
                    src_, dst_ = run[(k - 1) % 2], run[k % 2]
                    pp.fullres_affine_composites_device(src_.view(P * L, HP, WP, 3), ops[k][0], ops[k][1], ops[k][2], mask,
                                                        out=dst_.view(P * L, HP, WP, 3))
                return run[(K - 1) % 2]

            same = bool(torch.equal(one(), chain()))
            relit = int((out != photo[:, None]).any(dim=-1).sum().item())
            r = {"P": P, "B": B, "same_bytes": same, "pixels_relit": relit, "floor_bytes": floor_bytes(P, B, L, h, w, HP, WP)}
            # the same faces upright: the boxes' single pass, and the same boxes as maps through the new entry
            x_up = pp.ingest_group_device(photo, boxes, pidx, (h, w))
            out_up = run[0]
            boxed = lambda: pp.fullres_group_composites_device(photo, boxes, pidx, x_up, rendered, mask, out=out_up)
            mapped = lambda: pp.fullres_group_affine_composites_device(photo, up_pair, pidx, x_up, rendered, mask, out=out)
            r["tilted"], r["chain"], r["upright_boxes"], r["upright_maps"] = alternate([one, chain, boxed, mapped])
            print("P = %d composites done" % P, file=sys.stderr, flush=True)
            del run, ops, out_up, x_up
            torch.cuda.empty_cache()
            index = torch.from_numpy(pidx).to(dev)
            gathered = photo[index]
            xa = pp.ingest_affine_device(gathered, pair, (h, w))
            r["ingest_same_bits"] = bool(torch.equal(xa.view(torch.int32), x_lo.view(torch.int32)))
            r["ingest_bytes"] = int(sum(3 * bw * bh for _, _, bw, bh, _ in FACES)) * P + B * h * w * 12
            r["ingest_group"], r["ingest_gather"], r["ingest_gathered"] = alternate([
                lambda: pp.ingest_group_affine_device(photo, pair, pidx, (h, w)),
                lambda: pp.ingest_affine_device(photo[index], pair, (h, w)),
                lambda: pp.ingest_affine_device(gathered, pair, (h, w))])
            res["cases"][str(P)] = r
            print("P = %d ingests done" % P, file=sys.stderr, flush=True)
            del out, rendered, x_lo, photo, gathered, xa
            torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    K, Lf, h, w = res["shape"]
    cmd = "python tools/fullres_group_affine_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda v: "%.1f (%.1f .. %.1f)" % (v["median_us"], v["min_us"], v["max_us"])
    p = res["copy_probe"]
    rate = lambda nbytes, v: "%.0f GB/s | %.1f %%" % (nbytes / v["median_us"] / 1e3, 100.0 * nbytes / v["median_us"] / 1e3 / p["GBs"])
    row = lambda label, v, nbytes: "| %s | %s | %.1f MB | %s |" % (label, fmt(v), nbytes / 1e6, rate(nbytes, v))
    lines = ["# Rotated faces in group photographs: every tilted face of a photograph relit in one pass, against the chain of affine "
             "calls (one MI355X)", "",
             "`%s` (%slibrary `%s`, source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library"], res["library_source_hash"],
                                     res["device"]), "",
             "The legs of a case alternate A, B, C, D, A, ...: %d repeats of %d calls between two in-stream events behind a device "
             "synchronise, after %d untimed calls per leg.  Median and (min .. max) of the repeats, microseconds per CALL (the chain: per "
             "chain of %d calls), including what the host does per call (checks, launches; every output is written into a preallocated "
             "buffer).  Kernel times were not traced separately.  Nothing here is a gate." % (a.repeats, a.iters, a.warmup, K), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call) in the same run: %s us per call, %.0f GB/s read + "
             "write." % (p["bytes"] // 2 >> 20, fmt(p), p["GBs"]), "",
             "Photographs of %d x %d, %d lights, the network at %d x %d, %d faces per photograph (x0, y0, bw, bh of the face upright, "
             "degrees about its centre): %s; K on the way out %s.  Smooth photographs with byte noise, a disc mask whose rim carries the "
             "shipped masks' grey levels, `rendered` = x_lo times a random factor in [0.4, 1.6).  `floor` is what the SINGLE pass has to "
             "move (per photograph 3 Hp Wp bytes read and 3 L Hp Wp written; per face and low-resolution pixel 12 + 12 L; the mask once); "
             "`achieved` is that over a leg's median -- for the chain, too, so that the shares compare -- and beside it its share of the "
             "copy probe's rate.  Legs C and D relight the same faces UPRIGHT (angle 0), as boxes through the group entry and as "
             "axis-aligned maps through the new one; their bytes are not compared (a box of this size is not a whole multiple of the "
             "network's side)." % (WP, HP, Lf, h, w, K, ", ".join(str(f) for f in FACES), res["sub_samples"]), ""]
    for P in PHOTOS:
        r = res["cases"][str(P)]
        lines += ["## P = %d: %d faces" % (P, r["B"]), "",
                  "Legs A and B return the same bytes: %s (%d pixel-lights differ from the photograph)." % (r["same_bytes"], r["pixels_relit"]), "",
                  "| composite | us per call | floor | achieved | of the copy probe |", "|---|---:|---:|---:|---:|",
                  row("A: `fullres_group_affine_composites_device`", r["tilted"], r["floor_bytes"]),
                  row("B: the chain of %d `fullres_affine_composites_device` calls" % K, r["chain"], r["floor_bytes"]),
                  row("C: upright, `fullres_group_composites_device` on the boxes", r["upright_boxes"], r["floor_bytes"]),
                  row("D: upright, `fullres_group_affine_composites_device` on the boxes' maps", r["upright_maps"], r["floor_bytes"]), "",
                  "B over A: %.2f.  A over C: %.2f.  D over C: %.2f." % (r["chain"]["median_us"] / r["tilted"]["median_us"],
                                                                        r["tilted"]["median_us"] / r["upright_boxes"]["median_us"],
                                                                        r["upright_maps"]["median_us"] / r["upright_boxes"]["median_us"]), "",
                  "The ingests return the same bits: %s.  Bytes are the upright boxes' read plus the network's input written." % r["ingest_same_bits"], "",
                  "| ingest | us per call | bytes | achieved | of the copy probe |", "|---|---:|---:|---:|---:|",
                  row("A: `ingest_group_affine_device`", r["ingest_group"], r["ingest_bytes"]),
                  row("B: `ingest_affine_device(photo[photo_index])`, the gather included", r["ingest_gather"], r["ingest_bytes"]),
                  row("C: `ingest_affine_device` on photographs gathered beforehand", r["ingest_gathered"], r["ingest_bytes"]), ""]
    lines += ["## Registers", ""]
    if res["registers"]:
        lines += ["Read from the library's code objects.", "", "| kernel | VGPRs | SGPRs | scratch bytes |", "|---|---:|---:|---:|"]
        lines += ["| `%s` | %d | %d | %d |" % ((n,) + tuple(v)) for n, v in sorted(res["registers"].items())]
    else:
        lines += ["The LLVM tools were not found: see `tests/test_fullres_group_affine_resources.py`, which prints the counts."]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
