#!/usr/bin/env python
"""A/B of rig frames (lighting.rig_frames_u8, csrc/gcfr_rig_frames.hip; inference.relight_environment_frames(fused=True)).

  stage      leg A (the baseline, the parent commit's code)   F x (lighting.combine_lights with rig f + postprocess.inference_images_device)
             leg B                                            lighting.rig_frames_u8: one launch for all F frames
             at 4 faces x 64 lights x 256^2 for F in {1, 4, 16} and at 8 faces x 18 lights x 512^2 x 16 frames.  The achieved bytes
             per second of leg B (the bytes the kernel has to move, `stage_bytes`) are reported beside the rate of the library's
             copy probe (gcfr_copy_probe, read + write) measured in the same run.
  turntable  leg A (the parent's code)   inference.relight_environment_frames(fused=False): the per-frame loop
             leg B                       the same call with fused=True
             for 4 faces of 256 x 256 under 64 lights, a 64 x 128 map and 16 rotations, the shipped lighting-transfer checkpoint on
             synthetic faces; one inference.relight_rig_device pass is timed in the same session, so that what the frames cost
             beyond the pass can be read off.

The protocol is tools/environment_ab.py's: one process, one device, no profiler attached.  Per case the two legs ALTERNATE (A, B,
A, B, ...): every repeat is `--iters` calls (stage) or one whole turntable between two in-stream events behind a device
synchronise, after `--warmup` untimed calls per leg; reported are the median over `--repeats` repeats and their spread
(min .. max).  The times are per CALL and include what the host does per call (allocation of outputs, launches).  Needs a GPU:
there is no fallback.  Writes the table as Markdown to `--out` (default profiles/rig_frames_ab.md) and prints the numbers as JSON.

usage: tools/rig_frames_ab.py [--repeats 7] [--iters 20] [--warmup 5] [--out PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGE_SHAPES = [(4, 64, 1, 256, 256), (4, 64, 4, 256, 256), (4, 64, 16, 256, 256), (8, 18, 16, 512, 512)]      # (B, L, F, H, W)


def stage_bytes(B, L, F, H, W, tile):
    """what the fused kernel has to move: per pixel and frame tile the L planes of final, albedo, photograph and mask once
    (4 L + 12 + 12 + 1 bytes), and 3 bytes per frame written; the rigs themselves are a few KB"""
    tiles = (F + tile - 1) // tile
    return B * H * W * (tiles * (4 * L + 25) + 3 * F) + 12 * F * L


def unfused_bytes(B, L, F, H, W):
    """the two-stage path's: per frame the rig stage reads 4 L + 12 and writes 24 (rendered and shading_rgb), the image kernel reads
    12 + 12 + 1 and writes 3"""
    return B * H * W * F * ((4 * L + 12 + 24) + (12 + 12 + 1 + 3))


def rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_frames_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rig_frames_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    import scenes
    from geomconsistentfr_amd import _lib, build, combine_lights, lighting, rig_frames_u8
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd import postprocess as pp
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    dev = torch.device("cuda:0")
    tile = lighting.RIG_FRAMES_TILE

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
           "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup, "frame_tile": tile, "copy_probe": None, "stage": [],
           "turntable": None}

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

    # ---- the stage against the two-stage path --------------------------------------------------------------------------------
    for B, L, F, H, W in STAGE_SHAPES:
        g = torch.Generator(device="cpu").manual_seed(L + F)
        final = (0.2 + torch.rand(B, L, H, W, generator=g)).to(dev)
        albedo = (0.1 + 0.8 * torch.rand(B, 3, H, W, generator=g)).to(dev)
        x = torch.rand(B, H, W, 3, generator=g).to(dev)
        mask = (255 * (torch.rand(1, H, W, generator=g) > 0.3)).to(torch.uint8).to(dev)
        rgb = (torch.randn(1, F, L, 3, generator=g) / L ** 0.5 + 1.0 / L).to(dev)
        rigs = [rgb[:, f].contiguous() for f in range(F)]     # (outside the timed region: the loop's callers hold a rig per frame)

        def leg_a():
            return [pp.inference_images_device(x, combine_lights(final, albedo, rigs[f])[0], mask)["rendered_image"] for f in range(F)]

        def leg_b():
            return rig_frames_u8(final, albedo, x, mask, rgb)

        with torch.no_grad():
            differ = int((torch.stack(leg_a(), dim=1) != leg_b()).sum())
            for leg in (leg_a, leg_b):
                for _ in range(a.warmup):
                    leg()
            ta, tb = [], []
            for _ in range(a.repeats):                        # interleaved
                ta.append(timed(leg_a, a.iters))
                tb.append(timed(leg_b, a.iters))
        nb = stage_bytes(B, L, F, H, W, tile)
        res["stage"].append({"shape": [B, L, F, H, W], "bytes_that_differ": differ, "two_stage": summary(ta), "fused": summary(tb),
                             "bytes": nb, "two_stage_bytes": unfused_bytes(B, L, F, H, W), "fused_GBs": nb / statistics.median(tb) / 1e3})
        print("stage %s done" % (res["stage"][-1]["shape"],), file=sys.stderr, flush=True)
        del final, albedo, x, mask, rgb, rigs
    torch.cuda.empty_cache()

    # ---- the turntable of DESIGN 4.8 ------------------------------------------------------------------------------------------
    B, F, L, He, We = 4, 16, 64, 64, 128
    sd = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests", "golden", "slt_checkpoint_epoch106.npz")).items()}
    net = RelightNetLightingTransfer()
    net.load_state_dict(sd, strict=True)
    net = net.float().to(dev).eval()
    depth, mask, albedo, _n, _l, _a = scenes.synth_faces(B, 0)
    shade = 0.45 + 0.55 * np.clip(depth / 80.0, 0, 1)
    x = torch.from_numpy((albedo * shade[:, None]).transpose(0, 2, 3, 1).astype(np.float32).copy()).to(dev)
    m_u8 = torch.from_numpy((mask[0] * 255).astype(np.uint8)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    env = (2.0 * torch.rand(1, He, We, 3, generator=g)).to(dev)
    env[:, :, We // 2:] *= 4.0
    rots = torch.from_numpy(np.stack([rotation_y(2.0 * np.pi * f / F) for f in range(F)])).to(dev)
    dirs = torch.from_numpy(lighting.sphere_directions(L, 0.2)).to(dev)
    with torch.no_grad():
        rgb0 = lighting.environment_lights(env, dirs, rotation=rots[0])

    def turn_a():
        return inf.relight_environment_frames(net, x, m_u8, env, rots, n_lights=L, device=dev)

    def turn_b():
        return inf.relight_environment_frames(net, x, m_u8, env, rots, n_lights=L, device=dev, fused=True)

    one_pass = lambda: inf.relight_rig_device(net, x, m_u8, dirs, rgb0, device=dev)
    fa, fb = turn_a(), turn_b()
    differ = int((fa != fb).sum())                            # (MIOpen's convolutions are not run-to-run reproducible: a count, not a gate)
    for leg in (turn_a, turn_b, one_pass):
        for _ in range(max(1, a.warmup // 2)):
            leg()
    ta, tb, tp = [], [], []
    for _ in range(a.repeats):
        ta.append(timed(turn_a, 1))
        tb.append(timed(turn_b, 1))
        tp.append(timed(one_pass, 4))
    res["turntable"] = {"faces": B, "frames": F, "lights": L, "map": [He, We], "bytes_that_differ": differ, "bytes_total": fa.numel(),
                        "loop": summary(ta), "fused": summary(tb), "one_rig_pass": summary(tp)}
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    t = res["turntable"]
    B, F, L = t["faces"], t["frames"], t["lights"]
    He, We = t["map"]
    cmd = "python tools/rig_frames_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda s, d=1.0: "%.1f (%.1f .. %.1f)" % (s["median_us"] / d, s["min_us"] / d, s["max_us"] / d)
    p = res["copy_probe"]
    lines = ["# Rig frames: one fused launch against F x (rig stage + image kernel), and the fused turntable against the loop (one MI355X)", "",
             "`%s` (%slibrary source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library_source_hash"], res["device"]), "",
             "Per case the two legs alternate A, B, A, B, ...: %d repeats behind %d untimed calls per leg, each repeat between two in-stream "
             "events behind a device synchronise.  Median and (min .. max) of the repeats.  The times are per CALL and include what the "
             "host does per call (output allocation, launches); kernel times were not traced separately." % (a.repeats, a.warmup), "",
             "The copy probe (`gcfr_copy_probe`, %d MiB read and as many written per call, %d calls per repeat) in the same run: %s us per "
             "call, %.0f GB/s read + write." % (p["bytes"] // 2 >> 20, a.iters, fmt(p), p["GBs"]), "",
             "## The stage: `rig_frames_u8` against F x (`combine_lights` + `inference_images_device`)", "",
             "- Leg A, the baseline (the parent commit's code): per frame the rig stage, then the image kernel at one image per "
             "photograph: 2 F launches, an f32 `rendered` and a `shading_rgb` per frame through memory.",
             "- Leg B: `lighting.rig_frames_u8`: one launch, frame tile %d." % res["frame_tile"],
             "- One shared rig set (1,F,L,3), one shared mask; %d calls per repeat; microseconds per call.  `bytes` is what the fused kernel "
             "has to move (`stage_bytes`: per pixel ceil(F / %d) (4 L + 25) read and 3 F written); `achieved` is that over leg B's median, "
             "host work included." % (a.iters, res["frame_tile"]), "",
             "| faces x lights x frames x pixels | two-stage path | `rig_frames_u8` | ratio | bytes (fused) | achieved | of the copy probe | bytes that differ |",
             "|---|---:|---:|---:|---:|---:|---:|---:|"]
    for s in res["stage"]:
        B_, L_, F_, H_, W_ = s["shape"]
        lines.append("| %d x %d x %d x %d^2 | %s | %s | %.2fx | %.1f MB | %.0f GB/s | %.1f %% | %d |"
                     % (B_, L_, F_, H_, fmt(s["two_stage"]), fmt(s["fused"]), s["two_stage"]["median_us"] / s["fused"]["median_us"],
                        s["bytes"] / 1e6, s["fused_GBs"], 100.0 * s["fused_GBs"] / p["GBs"], s["bytes_that_differ"]))
    per_frame = lambda s: (s["median_us"] - t["one_rig_pass"]["median_us"]) / 1e3 / F
    lines += ["", "## The turntable: %d faces of 256 x 256, %d lights, a %d x %d map, %d rotations" % (B, L, He, We, F), "",
              "- Leg A, the parent commit's code: `inference.relight_environment_frames(fused=False)`: one network pass, then per frame the "
              "cell map, the integration, the rig combine and the image kernel.",
              "- Leg B: the same call with `fused=True`: one network pass, then one cell-map launch, one integration launch and one "
              "rig-frames launch for all %d frames." % F,
              "- One whole turntable per repeat; milliseconds.", "",
              "| | whole turntable, ms | beyond one rig pass, per frame, ms |", "|---|---:|---:|",
              "| the loop (`fused=False`) | %s | %.3f |" % (fmt(t["loop"], 1e3), per_frame(t["loop"])),
              "| `fused=True` | %s | %.3f |" % (fmt(t["fused"], 1e3), per_frame(t["fused"])),
              "", "One `relight_rig_device` pass alone (network pass, %d marches per face, one rig combine, one image kernel), timed in the "
              "same session (4 calls per repeat): %s ms; the last column is (turntable - that pass) / %d.  Ratio of the two turntables: "
              "%.2fx; the loop's own spread is %.3f ms, the difference of the medians %.3f ms.  Bytes of the %d that differ between the "
              "two legs' frames: %d (the network's convolutions are MIOpen's and not run-to-run reproducible; on fixed head outputs the "
              "frames are byte-identical, `tests/test_gpu_rig_frames_inference.py`)."
              % (L, fmt(t["one_rig_pass"], 1e3), F, t["loop"]["median_us"] / t["fused"]["median_us"],
                 (t["loop"]["max_us"] - t["loop"]["min_us"]) / 1e3, (t["loop"]["median_us"] - t["fused"]["median_us"]) / 1e3,
                 t["bytes_total"], t["bytes_that_differ"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
