#!/usr/bin/env python
"""A/B of the full-resolution kernels (csrc/gcfr_fullres.hip; postprocess.ingest_photographs_device / fullres_composites_device).

  composite  leg A   the same statement written with torch ops on the device: F.interpolate (bilinear, align_corners=False) of
                     x_lo, the mask and `rendered`, the elementwise quotient / clamp / blend, round, clamp, to(uint8), where
             leg B   postprocess.fullres_composites_device: ONE launch for all L lights
             at B = 8 faces, h = w = 256, s = 4 (1024 x 1024 photographs) for L in {1, 11}.  The achieved bytes per second of leg B
             over the byte floor (`floor_bytes`: per hi-res pixel 3 read and 3 L written, the low-resolution planes once) are
             reported beside the rate of the library's copy probe (gcfr_copy_probe, read + write) measured in the same run.
  ingest     leg A   the host shrink (numpy block mean of the uint8 photographs, / 255 in f32) plus the upload of the f32 result
             leg B   the upload of the uint8 photographs plus postprocess.ingest_photographs_device
             and the ingest launch alone on photographs already on the device.  (cv2, whose resize the scripts call, is not a
             dependency of this project; the block mean is what the ingest computes.)

The protocol is tools/rig_frames_ab.py's: one process, one device, no profiler attached.  Per case the two legs ALTERNATE (A, B,
A, B, ...): every repeat is `--iters` calls between two in-stream events behind a device synchronise (the ingest legs, which
include host work and a copy, between two host clock readings around a synchronise), after `--warmup` untimed calls per leg;
reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and include what the host
does per call (allocation of outputs, launches).  Needs a GPU: there is no fallback.  Writes the table as Markdown to `--out`
(default profiles/fullres_ab.md) and prints the numbers as JSON.

usage: tools/fullres_ab.py [--repeats 7] [--iters 20] [--warmup 5] [--out PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H_LO, W_LO, SCALE = 8, 256, 256, 4
LIGHTS = (1, 11)


def floor_bytes(B, L, h, w, s):
    """what the fused launch has to move: per hi-res pixel the photograph's 3 bytes read and 3 L written; per low-res pixel x_lo
    (12), `rendered` (12 L) and the mask (1) once"""
    return B * (s * h) * (s * w) * (3 + 3 * L) + B * h * w * (12 + 12 * L) + h * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullres_ab.md"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as Fn
    if not torch.cuda.is_available():
        sys.exit("fullres_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    from geomconsistentfr_amd import _lib, build
    from geomconsistentfr_amd import postprocess as pp
    dev = torch.device("cuda:0")
    h, w, s = H_LO, W_LO, SCALE
    H, W = s * h, s * w

    def timed(fn, n):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / n * 1e3                  # us per call

    def timed_host(fn, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e6           # us per call

    def summary(v):
        return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"commit": commit, "library_source_hash": build.source_hash()[:16], "device": torch.cuda.get_device_name(dev),
           "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup, "shape": [B, h, w, s], "copy_probe": None, "composite": [],
           "ingest": None}

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

    # ---- inputs: smooth photographs with byte noise, a disc mask with the shipped grey levels on its rim ----------------------
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 128 + 60 * np.sin(xx / 97.0)[None, :, :, None] * np.cos(yy / 61.0)[None, :, :, None] * np.ones((B, 1, 1, 3), np.float32)
    photo_np = np.clip(base + rng.normal(0, 12, (B, H, W, 3)), 0, 255).astype(np.uint8)
    rad = np.hypot(*(np.mgrid[0:h, 0:w] - np.array([h / 2, w / 2])[:, None, None]))
    mask_np = np.select([rad < 90, rad < 94, rad < 98], [255, 128, 64], 0).astype(np.uint8)[None]
    photo = torch.from_numpy(photo_np).to(dev)
    mask = torch.from_numpy(mask_np).to(dev)
    x_lo = pp.ingest_photographs_device(photo, s)

    def torch_leg(rendered, clamp=4.0, floor=1.0):
        L = rendered.shape[1]
        up = lambda t: Fn.interpolate(t, scale_factor=s, mode="bilinear", align_corners=False)
        pc = photo.permute(0, 3, 1, 2)
        p = pc.to(torch.float32)
        d = (p / (up(x_lo.permute(0, 3, 1, 2)) * 255.0).clamp_min(floor)).clamp(1.0 / clamp, clamp)
        m = up((mask.to(torch.float32) / 255.0)[:, None])[:, None]                                   # (1,1,1,H,W)
        r = up(rendered.reshape(B * L, 3, h, w)).reshape(B, L, 3, H, W) * 255.0
        v = p[:, None] + m * (r * d[:, None] - p[:, None])
        q = v.round().clamp(0.0, 255.0).to(torch.uint8)
        return torch.where(m > 0, q, pc[:, None]).permute(0, 1, 3, 4, 2).contiguous()

    for L in LIGHTS:
        g = torch.Generator(device="cpu").manual_seed(L)
        rendered = (x_lo.permute(0, 3, 1, 2)[:, None].cpu() * (0.4 + 1.2 * torch.rand(B, L, 3, h, w, generator=g))).to(dev).contiguous()
        leg_a = lambda: torch_leg(rendered)
        leg_b = lambda: pp.fullres_composites_device(photo, x_lo, rendered, mask, s)
        with torch.no_grad():
            fa, fb = leg_a(), leg_b()
            differ, differ_gt1 = int((fa != fb).sum()), int(((fa.to(torch.int16) - fb.to(torch.int16)).abs() > 1).sum())
            total = fa.numel()
            del fa, fb
            for leg in (leg_a, leg_b):
                for _ in range(a.warmup):
                    leg()
            ta, tb = [], []
            for _ in range(a.repeats):                        # interleaved
                ta.append(timed(leg_a, a.iters))
                tb.append(timed(leg_b, a.iters))
        nb = floor_bytes(B, L, h, w, s)
        res["composite"].append({"lights": L, "torch_ops": summary(ta), "fused": summary(tb), "floor_bytes": nb,
                                 "fused_GBs": nb / statistics.median(tb) / 1e3, "bytes_total": total, "bytes_that_differ": differ,
                                 "bytes_that_differ_by_more_than_one": differ_gt1})
        print("composite L = %d done" % L, file=sys.stderr, flush=True)
        del rendered
        torch.cuda.empty_cache()

    # ---- the ingest against a host shrink plus upload -----------------------------------------------------------------------
    def host_shrink():
        x = photo_np.reshape(B, h, s, w, s, 3).mean(axis=(2, 4), dtype=np.float32) / np.float32(255.0)
        return torch.from_numpy(x).to(dev)

    dev_ingest = lambda: pp.ingest_photographs_device(torch.from_numpy(photo_np).to(dev), s)
    launch_only = lambda: pp.ingest_photographs_device(photo, s)
    err = float((host_shrink() - launch_only()).abs().max())
    for leg in (host_shrink, dev_ingest, launch_only):
        for _ in range(a.warmup):
            leg()
    th, td, tl = [], [], []
    n_host = max(1, a.iters // 4)
    for _ in range(a.repeats):
        th.append(timed_host(host_shrink, n_host))
        td.append(timed_host(dev_ingest, n_host))
        tl.append(timed(launch_only, a.iters))
    res["ingest"] = {"host_shrink_and_upload": summary(th), "upload_and_device_ingest": summary(td), "launch_alone": summary(tl),
                     "calls_per_repeat_host_legs": n_host, "bytes_read": B * H * W * 3, "bytes_written": B * h * w * 12,
                     "launch_GBs": (B * H * W * 3 + B * h * w * 12) / statistics.median(tl) / 1e3, "max_abs_difference": err}
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    Bf, h, w, s = res["shape"]
    cmd = "python tools/fullres_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda v, d=1.0: "%.1f (%.1f .. %.1f)" % (v["median_us"] / d, v["min_us"] / d, v["max_us"] / d)
    p = res["copy_probe"]
    lines = ["# Full-resolution relighting: the fused composite against torch ops, the device ingest against a host shrink (one MI355X)", "",
             "`%s` (%slibrary source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library_source_hash"], res["device"]), "",
             "Per case the two legs alternate A, B, A, B, ...: %d repeats behind %d untimed calls per leg.  Median and (min .. max) of "
             "the repeats.  The times are per CALL and include what the host does per call (output allocation, launches); kernel times "
             "were not traced separately." % (a.repeats, a.warmup), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call, %d calls per repeat) in the same run: %s us per "
             "call, %.0f GB/s read + write." % (p["bytes"] // 2 >> 20, a.iters, fmt(p), p["GBs"]), "",
             "## The composite: `fullres_composites_device` against the statement in torch ops", "",
             "%d faces, the network at %d x %d, s = %d: photographs of %d x %d.  Smooth photographs with byte noise, a disc mask whose rim "
             "carries the shipped masks' grey levels, `rendered` = x_lo times a random factor in [0.4, 1.6)." % (Bf, h, w, s, s * h, s * w), "",
             "- Leg A: `F.interpolate(bilinear, align_corners=False)` of x_lo, the mask and `rendered`, then the elementwise quotient, clamp "
             "and blend, `round`, `clamp`, `to(uint8)`, `where`, and the permute to HWC -- every intermediate an f32 tensor of the output's "
             "size through memory.",
             "- Leg B: ONE launch for all L lights.",
             "- %d calls per repeat between two in-stream events behind a device synchronise; microseconds per call.  `floor` is what the "
             "launch has to move (`floor_bytes`: per hi-res pixel 3 bytes read and 3 L written, per low-res pixel 12 + 12 L + 1 once); "
             "`achieved` is that over leg B's median, host work included; the last rate column is `achieved` over the copy probe's rate."
             % a.iters, "",
             "| lights | torch ops | fused launch | ratio | floor | achieved | of the copy probe | bytes that differ from leg A (by more than one level) |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for c in res["composite"]:
        lines.append("| %d | %s | %s | %.1fx | %.1f MB | %.0f GB/s | %.1f %% | %d of %d (%d) |"
                     % (c["lights"], fmt(c["torch_ops"]), fmt(c["fused"]), c["torch_ops"]["median_us"] / c["fused"]["median_us"],
                        c["floor_bytes"] / 1e6, c["fused_GBs"], 100.0 * c["fused_GBs"] / p["GBs"], c["bytes_that_differ"], c["bytes_total"],
                        c["bytes_that_differ_by_more_than_one"]))
    g = res["ingest"]
    lines += ["", "Leg A is not the kernel's restatement bit for bit (`F.interpolate` forms its weights and sums differently), so a byte may "
              "fall on the other side of a rounding tie; the kernel is held byte for byte to `tests/fullres_emulation.py`.", "",
              "## The ingest: `ingest_photographs_device` against a host shrink plus upload", "",
              "- Leg A: the numpy block mean of the uint8 photographs in f32, / 255, and the upload of the f32 (B,h,w,3) result.",
              "- Leg B: the upload of the uint8 photographs (pageable host memory) and the ingest launch.",
              "- %d calls per repeat between two host clock readings around a device synchronise; the launch alone (photographs already on "
              "the device) as the composite is timed.  Largest |A - B| of the network's input: %.3g." % (g["calls_per_repeat_host_legs"], g["max_abs_difference"]), "",
              "| | us per call |", "|---|---:|",
              "| host shrink + upload of f32 | %s |" % fmt(g["host_shrink_and_upload"]),
              "| upload of uint8 + device ingest | %s |" % fmt(g["upload_and_device_ingest"]),
              "| the ingest launch alone | %s |" % fmt(g["launch_alone"]),
              "", "The launch alone moves %.1f MB read and %.1f MB written: %.0f GB/s, host work per call included." %
              (g["bytes_read"] / 1e6, g["bytes_written"] / 1e6, g["launch_GBs"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
