#!/usr/bin/env python
"""A/B of environment-map lighting (lighting.environment_lights, csrc/gcfr_environment.hip; inference.relight_environment_frames).

  stage      leg A (the baseline)   the torch composition over the SAME cell map: rgb.index_add_(1, cell, env * w) in f64, rounded
                                    to f32 (the map's products and the scatter; the cell map is given to it, not computed)
             leg B                  environment_lights(env, directions)      (the cell map + the integration: two launches)
             at 64 x 128 texels x 64 lights and 512 x 1024 texels x 256 lights, one map (E = 1) and eight (E = 8).
  turntable  leg A (the parent's way)   F calls of inference.relight_rig_device, one full pass (network + L marches + combine +
                                        image kernel) per frame, with the frame's light_rgb precomputed outside the timed region
             leg B                      inference.relight_environment_frames: ONE pass, then four launches per frame
             for B faces of 256 x 256 under 64 lights and F rotations, the shipped lighting-transfer checkpoint on synthetic faces.

One process, one device, no profiler attached.  Per case the two legs ALTERNATE (A, B, A, B, ...): every repeat is `--iters` calls
(stage) or one whole turntable (turntable) between two in-stream events behind a device synchronise, after `--warmup` untimed
calls per leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and
include what the host does per call (allocation of outputs, launches): at these sizes that is most of it.  Needs a GPU: there is
no fallback.  Writes the table as Markdown to `--out` (default profiles/environment_ab.md) and prints the same numbers as JSON.

usage: tools/environment_ab.py [--repeats 7] [--iters 50] [--warmup 5] [--faces 4] [--frames 16] [--out PATH]"""
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

STAGE_SHAPES = [(1, 64, 128, 64), (8, 64, 128, 64), (1, 512, 1024, 256), (8, 512, 1024, 256)]      # (E, He, We, L)


def stage_bytes(E, He, We, L):
    """what the two kernels have to move at the least: the cell map written once and read once per (e, l) workgroup (L2-resident
    at these sizes, counted once per launch here), every texel of radiance read once, the tables and the result"""
    T = He * We
    return (4 * T + 8 * (He + We) + 12 * L) + (4 * T + 12 * E * T + 8 * He + 12 * E * L)


def rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--faces", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "environment_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("environment_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    import scenes
    from geomconsistentfr_amd import _lib, build, environment_lights, lighting
    from geomconsistentfr_amd import inference as inf
    from geomconsistentfr_amd.relightnet import RelightNetLightingTransfer
    dev = torch.device("cuda:0")

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
           "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup, "stage": [], "turntable": None}

    # ---- the stage against the torch composition ---------------------------------------------------------------------------
    for E, He, We, L in STAGE_SHAPES:
        g = torch.Generator(device="cpu").manual_seed(L + E)
        env = (2.0 * torch.rand(E, He, We, 3, generator=g)).to(dev)
        dirs = torch.from_numpy(lighting.sphere_directions(L, 0.2)).to(dev)
        rows, row_w, cols = lighting._device_tables(He, We, dev)
        cell = torch.empty((He, We), dtype=torch.int32, device=dev)
        _lib.launch("gcfr_environment_cells", dev, rows, cols, dirs, He, We, L, -2.0, cell, _lib.STREAM)
        idx = cell.reshape(-1).to(torch.int64)
        w = row_w.repeat_interleave(We)[None, :, None]                                # (1,T,1) f64

        def leg_a():
            out = torch.zeros(E, L, 3, dtype=torch.float64, device=dev)
            out.index_add_(1, idx, env.reshape(E, -1, 3).to(torch.float64) * w)
            return out.float()

        def leg_b():
            return environment_lights(env, dirs)

        with torch.no_grad():
            diff = float((leg_a() - leg_b()).abs().max())
            for leg in (leg_a, leg_b):
                for _ in range(a.warmup):
                    leg()
            ta, tb = [], []
            for _ in range(a.repeats):                        # interleaved
                ta.append(timed(leg_a, a.iters))
                tb.append(timed(leg_b, a.iters))
        nb = stage_bytes(E, He, We, L)
        res["stage"].append({"shape": [E, He, We, L], "max_abs_diff": diff, "torch": summary(ta), "hip": summary(tb), "bytes": nb,
                             "hip_GBs": nb / statistics.median(tb) / 1e3})
        print("stage %s done" % (res["stage"][-1]["shape"],), file=sys.stderr, flush=True)
        del env, cell, idx, w
    torch.cuda.empty_cache()

    # ---- a turntable -------------------------------------------------------------------------------------------------------
    B, F, L, He, We = a.faces, a.frames, 64, 64, 128
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
        rgbs = [environment_lights(env, dirs, rotation=rots[f]) for f in range(F)]

    def turn_a():
        return [inf.relight_rig_device(net, x, m_u8, dirs, rgbs[f], device=dev) for f in range(F)]

    def turn_b():
        return inf.relight_environment_frames(net, x, m_u8, env, rots, n_lights=L, device=dev)

    one_pass = lambda: inf.relight_rig_device(net, x, m_u8, dirs, rgbs[0], device=dev)
    fa, fb = torch.stack(turn_a(), dim=1), turn_b()
    differ = int((fa != fb).sum())                            # (MIOpen's convolutions are not run-to-run reproducible: a count, not a gate)
    for leg in (turn_a, turn_b):
        for _ in range(max(1, a.warmup // 2)):
            leg()
    ta, tb, tp = [], [], []
    for _ in range(a.repeats):
        ta.append(timed(turn_a, 1))
        tb.append(timed(turn_b, 1))
        tp.append(timed(one_pass, 4))
    res["turntable"] = {"faces": B, "frames": F, "lights": L, "map": [He, We], "bytes_that_differ": differ, "bytes_total": fa.numel(),
                        "rig_pass_per_frame": summary(ta), "environment_frames": summary(tb), "one_rig_pass": summary(tp)}
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    B, F, L = res["turntable"]["faces"], res["turntable"]["frames"], res["turntable"]["lights"]
    He, We = res["turntable"]["map"]
    cmd = "python tools/environment_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup", "faces", "frames"))
    fmt = lambda s, d=1.0: "%.1f (%.1f .. %.1f)" % (s["median_us"] / d, s["min_us"] / d, s["max_us"] / d)
    t = res["turntable"]
    lines = ["# Environment-map lighting against the torch composition, and a turntable against a pass per frame (one MI355X)", "",
             "`%s` (%slibrary source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library_source_hash"], res["device"]), "",
             "Per case the two legs alternate A, B, A, B, ...: %d repeats behind %d untimed calls per leg, each repeat between two in-stream "
             "events behind a device synchronise.  Median and (min .. max) of the repeats.  The times are per CALL and include what the "
             "host does per call (output allocation, launches); kernel times were not traced separately." % (a.repeats, a.warmup), "",
             "## The stage: `environment_lights` against `index_add_` over the same cell map", "",
             "- Leg A, the baseline: `rgb.index_add_(1, cell, env * w)` in f64 and its rounding to f32, the cell map GIVEN (not computed).",
             "- Leg B: `lighting.environment_lights(env, directions)`: `gcfr_environment_cells` + `gcfr_environment_fwd`.",
             "- %d calls per repeat; microseconds per call." % a.iters, "",
             "| maps x texels x lights | torch composition | `environment_lights` | ratio | bytes the stage moves | achieved | largest difference |",
             "|---|---:|---:|---:|---:|---:|---:|"]
    for s in res["stage"]:
        E, He_, We_, L_ = s["shape"]
        lines.append("| %d x (%d x %d) x %d | %s | %s | %.2fx | %.2f MB | %.1f GB/s | %.1e |"
                     % (E, He_, We_, L_, fmt(s["torch"]), fmt(s["hip"]), s["torch"]["median_us"] / s["hip"]["median_us"], s["bytes"] / 1e6,
                        s["hip_GBs"], s["max_abs_diff"]))
    lines += ["", "## A turntable: %d faces of 256 x 256, %d lights, a %d x %d map, %d rotations" % (B, L, He, We, F), "",
              "- Leg A, the parent commit's way: %d calls of `inference.relight_rig_device`, a full pass per frame (the frame's `light_rgb` "
              "computed outside the timed region)." % F,
              "- Leg B: `inference.relight_environment_frames`: one network pass and %d marches per face in total, then per frame the cell "
              "map, the integration, the rig combine and the image kernel." % L,
              "- One whole turntable per repeat; milliseconds.", "",
              "| | whole turntable, ms | per frame, ms |", "|---|---:|---:|",
              "| a pass per frame (`relight_rig_device` x %d) | %s | %.3f |" % (F, fmt(t["rig_pass_per_frame"], 1e3), t["rig_pass_per_frame"]["median_us"] / 1e3 / F),
              "| `relight_environment_frames` | %s | %.3f |" % (fmt(t["environment_frames"], 1e3), t["environment_frames"]["median_us"] / 1e3 / F),
              "", "One `relight_rig_device` pass alone -- the per-frame pass as the parent commit has it, the function being unchanged -- "
              "timed in the same session (4 calls per repeat): %s ms.  Ratio of the two turntables: "
              "%.2fx.  Bytes of the %d that differ between the two legs' frames: %d (the network's convolutions are MIOpen's and not "
              "run-to-run reproducible; on fixed head outputs the frames are byte-identical, `tests/test_gpu_environment.py`)."
              % (fmt(t["one_rig_pass"], 1e3), t["rig_pass_per_frame"]["median_us"] / t["environment_frames"]["median_us"], t["bytes_total"],
                 t["bytes_that_differ"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
