#!/usr/bin/env python
"""A/B of the two full-resolution composites of one library: the bilinear launch (csrc/gcfr_fullres.hip, unchanged) against the
guided launch (csrc/gcfr_fullres_guided.hip), postprocess.fullres_composites_device(upsample="bilinear" | "guided").

  leg A   upsample="bilinear"
  leg B   upsample="guided", range_sigma 20
  at B = 8 faces, s = 4, photographs of 256 x 256, 512 x 512 and 1024 x 1024 (the network at a quarter of that), for L in {1, 11}.

Both legs write the same bytes count; neither is the other's reference (the guided composite is held byte for byte to
tests/fullres_guided_emulation.py).  Reported per case: the two times, their ratio, and the achieved bytes per second of each leg
over its byte floor beside the rate of the library's copy probe (gcfr_copy_probe, read + write) measured in the same run.  The byte
floor is tools/fullres_ab.py's -- per hi-res pixel 3 bytes read and 3 L written, the low-resolution planes once from memory: the
guided kernel's wider footprint (16 taps instead of 4) re-reads the same low-resolution planes from cache and adds nothing that has
to come from memory.

The protocol is tools/fullres_ab.py's: one process, one device, no profiler attached.  Per case the two legs ALTERNATE (A, B, A,
B, ...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after `--warmup` untimed calls
per leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and include what
the host does per call (allocation of the output, the launch).  Needs a GPU: there is no fallback.  Writes the table as Markdown to
`--out` (default profiles/fullres_guided_ab.md) and prints the numbers as JSON.

usage: tools/fullres_guided_ab.py [--repeats 7] [--iters 20] [--warmup 5] [--out PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SCALE = 8, 4
SIDES = (256, 512, 1024)          # the photograph's side
LIGHTS = (1, 11)
RANGE_SIGMA = 20.0


def floor_bytes(B, L, h, w, s):
    """tools/fullres_ab.py's: per hi-res pixel the photograph's 3 bytes read and 3 L written; per low-res pixel x_lo (12),
    `rendered` (12 L) and the mask (1) once"""
    return B * (s * h) * (s * w) * (3 + 3 * L) + B * h * w * (12 + 12 * L) + h * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullres_guided_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fullres_guided_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    from geomconsistentfr_amd import _lib, build
    from geomconsistentfr_amd import postprocess as pp
    dev = torch.device("cuda:0")
    s = SCALE

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

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"commit": commit, "library_source_hash": build.source_hash()[:16], "device": torch.cuda.get_device_name(dev),
           "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup, "faces": B, "scale": s, "range_sigma": RANGE_SIGMA,
           "copy_probe": None, "cases": []}

    # ---- the copy probe: what a plain device-to-device copy achieves in this run --------------------------------------------
    n_probe = 1 << 28                                         # 256 MiB read + 256 MiB written: past the Infinity Cache
    src, dst = torch.zeros(n_probe, dtype=torch.uint8, device=dev), torch.empty(n_probe, dtype=torch.uint8, device=dev)
    L_ = _lib.load()
    probe = lambda: _lib.check(L_.gcfr_copy_probe(src.data_ptr(), dst.data_ptr(), n_probe, _lib.stream_ptr(dev)), "gcfr_copy_probe")
    for _ in range(a.warmup):
        probe()
    tp = [timed(probe, a.iters) for _ in range(a.repeats)]
    res["copy_probe"] = dict(summary(tp), bytes=2 * n_probe, GBs=2 * n_probe / statistics.median(tp) / 1e3)
    del src, dst
    torch.cuda.empty_cache()

    for side in SIDES:
        H = W = side
        h, w = H // s, W // s
        # smooth photographs with byte noise, a disc mask with the shipped grey levels on its rim (tools/fullres_ab.py's inputs)
        rng = np.random.default_rng(0)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        base = 128 + 60 * np.sin(xx / 97.0)[None, :, :, None] * np.cos(yy / 61.0)[None, :, :, None] * np.ones((B, 1, 1, 3), np.float32)
        photo = torch.from_numpy(np.clip(base + rng.normal(0, 12, (B, H, W, 3)), 0, 255).astype(np.uint8)).to(dev)
        rad = np.hypot(*(np.mgrid[0:h, 0:w] - np.array([h / 2, w / 2])[:, None, None]))
        k = h / 256.0
        mask = torch.from_numpy(np.select([rad < 90 * k, rad < 94 * k, rad < 98 * k], [255, 128, 64], 0).astype(np.uint8)[None]).to(dev)
        x_lo = pp.ingest_photographs_device(photo, s)
        for L in LIGHTS:
            g = torch.Generator(device="cpu").manual_seed(L)
            rendered = (x_lo.permute(0, 3, 1, 2)[:, None].cpu() * (0.4 + 1.2 * torch.rand(B, L, 3, h, w, generator=g))).to(dev).contiguous()
            leg_a = lambda: pp.fullres_composites_device(photo, x_lo, rendered, mask, s, upsample="bilinear")
            leg_b = lambda: pp.fullres_composites_device(photo, x_lo, rendered, mask, s, upsample="guided", range_sigma=RANGE_SIGMA)
            fa, fb = leg_a(), leg_b()
            differ, total = int((fa != fb).sum()), fa.numel()
            del fa, fb
            for leg in (leg_a, leg_b):
                for _ in range(a.warmup):
                    leg()
            ta, tb = [], []
            for _ in range(a.repeats):                        # interleaved
                ta.append(timed(leg_a, a.iters))
                tb.append(timed(leg_b, a.iters))
            nb = floor_bytes(B, L, h, w, s)
            res["cases"].append({"side": side, "lights": L, "bilinear": summary(ta), "guided": summary(tb), "floor_bytes": nb,
                                 "bilinear_GBs": nb / statistics.median(ta) / 1e3, "guided_GBs": nb / statistics.median(tb) / 1e3,
                                 "bytes_total": total, "bytes_that_differ_between_the_legs": differ})
            print("side %d L = %d done" % (side, L), file=sys.stderr, flush=True)
            del rendered
            torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    cmd = "python tools/fullres_guided_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda v: "%.1f (%.1f .. %.1f)" % (v["median_us"], v["min_us"], v["max_us"])
    p = res["copy_probe"]
    lines = ["# Full-resolution relighting: the guided (joint-bilateral) composite against the bilinear one (one MI355X)", "",
             "`%s` (%slibrary source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached.  Both legs are launches of the same library." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "",
                                                                                 res["library_source_hash"], res["device"]), "",
             "Per case the two legs alternate A, B, A, B, ...: %d repeats of %d calls between two in-stream events behind a device "
             "synchronise, behind %d untimed calls per leg.  Median and (min .. max) of the repeats, microseconds per CALL, including "
             "what the host does per call (output allocation, the launch); kernel times were not traced separately."
             % (a.repeats, a.iters, a.warmup), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call) in the same run: %s us per call, %.0f GB/s "
             "read + write." % (p["bytes"] // 2 >> 20, fmt(p), p["GBs"]), "",
             "%d faces, s = %d, `range_sigma` %g.  Smooth photographs with byte noise, a disc mask whose rim carries the shipped masks' "
             "grey levels, `rendered` = x_lo times a random factor in [0.4, 1.6)." % (res["faces"], res["scale"], res["range_sigma"]), "",
             "- Leg A: `fullres_composites_device(..., upsample=\"bilinear\")`, the launch of `csrc/gcfr_fullres.hip`.",
             "- Leg B: `fullres_composites_device(..., upsample=\"guided\")`, the launch of `csrc/gcfr_fullres_guided.hip`.",
             "- `floor` is what either launch has to move through memory (`floor_bytes`: per hi-res pixel 3 bytes read and 3 L written, "
             "per low-res pixel 12 + 12 L + 1 once; the guided footprint's further reads of the low-resolution planes come from cache); "
             "the rates are that over each leg's median, host work included, and the last column is the guided rate over the copy "
             "probe's.", "",
             "| photograph | lights | bilinear | guided | guided / bilinear | floor | bilinear achieved | guided achieved | guided, of the copy probe | bytes that differ between the legs |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for c in res["cases"]:
        lines.append("| %d x %d | %d | %s | %s | %.2fx | %.1f MB | %.0f GB/s | %.0f GB/s | %.1f %% | %d of %d |"
                     % (c["side"], c["side"], c["lights"], fmt(c["bilinear"]), fmt(c["guided"]),
                        c["guided"]["median_us"] / c["bilinear"]["median_us"], c["floor_bytes"] / 1e6, c["bilinear_GBs"], c["guided_GBs"],
                        100.0 * c["guided_GBs"] / p["GBs"], c["bytes_that_differ_between_the_legs"], c["bytes_total"]))
    lines += ["", "Nothing is gated on these times.  The two legs are different statements: the bytes that differ are the feature, not an "
              "error.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
