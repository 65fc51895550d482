#!/usr/bin/env python3
"""Which job of the prepass kernel sets its duration?  (GPU)

    tools/prepass_jobs.py build            (CPU)  lib/prepass_jobs_<mask>.so for the masks below: -DGCFR_FAST_BUILD -DGCFR_PREPASS_JOBS=<mask>
    tools/prepass_jobs.py run [--faces 8]  (GPU)  per library: the prepass alone (gcfr_options.phase = 1) as a hipGraph, replayed one at a
                                                  time on one stream; fenced wall time per replay and the HIP-event time of 200 single
                                                  replays -> gpurun_out/prepass_jobs.json
                          [--prefix P]            the libraries lib/<P><mask>.so instead of lib/prepass_jobs_<mask>.so (another build of
                                                  the same masks, e.g. the parent commit's)
                          [--out FILE]            the JSON goes to FILE instead (so that two builds' results can lie side by side)
                          [--timeout S]           time limit of each library's child process (default 120 s)

`run` starts one child process per library, each under its own time limit, and STOPS at the first child that fails (a non-zero
status, a time-out or no result line): what has faulted the device once is not given the next library to fault it again.  Its exit
status is then 1 and the JSON names the failure.

build_quad_kernel's grid is [horizon tables | depth-bounds tiles | statistics chunks | repack]; -DGCFR_PREPASS_JOBS leaves the
grid as it is and makes the blocks of the jobs whose bit is clear return at once (1 horizon, 2 bounds, 4 statistics, 8 unused, 16 repack),
so a single job's time includes the dispatch of the other jobs' empty blocks -- which is what it would cost next to faster neighbours.
The workspace such a library leaves is garbage: only the prepass is timed."""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(REPO, "geomconsistentfr_amd", "lib")
MASKS = [("all", 31), ("none", 0), ("horizon", 1), ("bounds", 2), ("statistics", 4), ("repack", 16), ("all but horizon", 30),
         ("all but repack", 15), ("all but bounds", 29), ("all but statistics", 27)]


def lib_of(mask):
    return os.path.join(LIB_DIR, "prepass_jobs_%d.so" % mask)


def build():
    sys.path.insert(0, REPO)
    from geomconsistentfr_amd import build as b
    for _, m in MASKS:
        t = time.time()
        b.compile_and_link(lib_of(m), defines=["-DGCFR_FAST_BUILD", "-DGCFR_PREPASS_JOBS=%d" % m], jobs=8)
        print("prepass_jobs_%d.so  %.0f s" % (m, time.time() - t), flush=True)


def one(faces):
    """(in a subprocess with GCFR_HIP_LIB set)"""
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench

    class One:  # a minimal stand-in for bench.Ranks: one rank, fences = synchronize
        dev, rank, world = torch.device("cuda:0"), 0, 1

        def fence(self):
            torch.cuda.synchronize()

        def max_over_ranks(self, s):
            return s
    rig = bench.RenderRig(One(), faces, streams=1, from_depth=True)
    p0 = rig.plans[0]
    p0.capture_split(*rig.inputs[0])
    st = rig.streams[0]
    with torch.cuda.stream(st):
        for _ in range(200):
            p0.replay_prepass()
    torch.cuda.synchronize()
    walls = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            for _ in range(2000):
                p0.replay_prepass()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) / 2000)
    evs = []
    with torch.cuda.stream(st):
        for _ in range(200):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            p0.replay_prepass()
            e1.record(st)
            evs.append((e0, e1))
    torch.cuda.synchronize()
    ev_ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    print(json.dumps({"wall_us_per_replay_median": 1e6 * float(np.median(walls)), "wall_us_per_replay_min": 1e6 * min(walls),
                      "event_us_median": 1e3 * ev_ms[len(ev_ms) // 2], "event_us_min": 1e3 * ev_ms[0]}))


def run(faces, prefix=None, limit=120.0, out_file=None):
    out = {"faces": faces, "how": __doc__.split("\n\n")[1], "libraries": {}}
    failed = None
    for name, m in MASKS:
        lib = lib_of(m) if prefix is None else os.path.join(LIB_DIR, "%s%d.so" % (prefix, m))
        if not os.path.exists(lib):
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "one", str(faces)], env=dict(os.environ, GCFR_HIP_LIB=lib),
                               capture_output=True, text=True, timeout=limit)
            if r.returncode != 0:
                raise RuntimeError("exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-600:]))
            out["libraries"][name] = dict(json.loads(r.stdout.strip().splitlines()[-1]), mask=m)
        except subprocess.TimeoutExpired:
            failed = out["libraries"][name] = {"mask": m, "error": "no result within %.0f s" % limit}
        except Exception as e:
            failed = out["libraries"][name] = {"mask": m, "error": str(e)[-700:]}
        print(name, out["libraries"][name], flush=True)
        if failed:
            out["stopped_at"] = name   # the libraries behind it were not run
            break
    os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
    with open(os.path.join(REPO, "gpurun_out", "prepass_jobs.json"), "w") as f:
        json.dump(out, f, indent=1)
    if out_file:
        os.replace(f.name, out_file)
    return 1 if failed else 0


def _arg(flag, default, kind):
    return kind(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "build":
        build()
    elif what == "one":
        one(int(sys.argv[2]))
    elif what == "run":
        sys.exit(run(_arg("--faces", 8, int), _arg("--prefix", None, str), _arg("--timeout", 120.0, float), _arg("--out", None, str)))
    else:
        sys.exit(__doc__)
