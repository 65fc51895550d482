#!/usr/bin/env python
"""A/B of rig capture with and without the non-negative solve (lighting.fit_light_rgb(nonnegative=...), csrc/gcfr_light_fit.hip).

  leg A (the baseline)   fit_light_rgb(final, albedo, image, weight, ridge): the normal equations (two launches) + the Cholesky solve
  leg B                  fit_light_rgb(..., nonnegative=True): the same normal equations + gcfr_light_fit_solve_nonneg (one launch)
  at 8 faces x 11 lights x 256 x 256 and 8 x 64 x 256 x 256, a {0,1} weight of 70 % ones per face; at each shape one photograph
  synthesised from an ALL-POSITIVE rig (uniform in [0.2, 1]: every light is admitted, one factorisation per light) and one from the
  MIXED-SIGN family (uniform in [-0.5, 1.5]: the unconstrained fit has negative entries, lights enter and leave).

Protocol of tools/light_fit_ab.py: one process, one device, no profiler attached.  Per case the two legs ALTERNATE (A, B, A, B,
...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after `--warmup` untimed calls per
leg; reported are the median over `--repeats` repeats and their spread (min .. max).  The times are per CALL and include what the
host does per call (allocation of outputs and of the workspace, launches).  Beside the times: `solves`, the factorisations per (face,
channel) the non-negative solve reports (smallest .. largest and their mean over the 24 systems), how many entries the
unconstrained fit has below zero and the non-negative one at zero.  No speed is promised or gated.  Needs a GPU: there is no
fallback.  Writes the table as Markdown to `--out` (default profiles/light_fit_nonneg_ab.md) and prints the same numbers as JSON.

usage: tools/light_fit_nonneg_ab.py [--repeats 7] [--iters 10] [--warmup 3] [--out PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 11, 256, 256), (8, 64, 256, 256)]      # (B, L, H, W)
RIGS = [("all-positive", 0.2, 1.0), ("mixed-sign", -0.5, 1.5)]
RIDGE = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_fit_nonneg_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("light_fit_nonneg_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    from geomconsistentfr_amd import build, fit_light_rgb
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
           "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup, "ridge": RIDGE, "cases": []}
    for B, L, H, W in SHAPES:
        for name, lo, hi in RIGS:
            g = torch.Generator(device="cpu").manual_seed(L + B)
            u = lambda *s: (0.05 + 0.95 * torch.rand(*s, generator=g)).to(dev)
            final, albedo = u(B, L, H, W), u(B, 3, H, W)
            weight = (torch.rand(B, H, W, generator=g) < 0.7).float().to(dev)
            x_true = (lo + (hi - lo) * torch.rand(B, L, 3, generator=g, dtype=torch.float64)).to(dev)
            shading = torch.einsum("blc,blhw->bchw", x_true, final.to(torch.float64))
            image = (albedo.to(torch.float64) * shading).float().permute(0, 2, 3, 1).contiguous()      # (B,H,W,3), rounded once
            del shading

            def leg_a():
                return fit_light_rgb(final, albedo, image, weight, ridge=RIDGE)

            def leg_b():
                return fit_light_rgb(final, albedo, image, weight, ridge=RIDGE, nonnegative=True)

            with torch.no_grad():
                free = leg_a()
                rgb, info, solves = fit_light_rgb(final, albedo, image, weight, ridge=RIDGE, nonnegative=True, return_info=True)
                solves = solves.cpu().numpy()
                for leg in (leg_a, leg_b):
                    for _ in range(a.warmup):
                        leg()
                ta, tb = [], []
                for _ in range(a.repeats):                    # interleaved
                    ta.append(timed(leg_a, a.iters))
                    tb.append(timed(leg_b, a.iters))
            res["cases"].append({"shape": [B, L, H, W], "rig": name, "unconstrained": summary(ta), "nonnegative": summary(tb),
                                 "solves_min": int(solves.min()), "solves_max": int(solves.max()), "solves_mean": float(solves.mean()),
                                 "cap": 3 * L, "info_nonzero": int((info != 0).sum()), "entries": int(free.numel()),
                                 "unconstrained_negative": int((free < 0).sum()), "nonnegative_zero": int((rgb == 0).sum()),
                                 "nonnegative_below_zero": int((rgb < 0).sum()),
                                 "same_bits": bool(torch.equal(free.view(torch.int32), rgb.view(torch.int32)))})
            print("case %s %s done" % (res["cases"][-1]["shape"], name), file=sys.stderr, flush=True)
            del final, albedo, image, weight
            torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    cmd = "python tools/light_fit_nonneg_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda s: "%.1f (%.1f .. %.1f)" % (s["median_us"], s["min_us"], s["max_us"])
    lines = ["# Rig capture with and without the non-negative solve (`fit_light_rgb(nonnegative=...)`, one MI355X)", "",
             "`%s` (%slibrary source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library_source_hash"], res["device"]), "",
             "Per case the legs alternate A, B, A, B, ...: %d repeats behind %d untimed calls per leg, each repeat %d calls between two "
             "in-stream events behind a device synchronise.  Median and (min .. max) of the repeats, microseconds per CALL, including "
             "what the host does per call (allocation of outputs and workspace, launches); kernel times were not traced separately."
             % (a.repeats, a.warmup, a.iters), "",
             "- Leg A: `lighting.fit_light_rgb(final, albedo, image, weight, ridge=%g)`: `gcfr_light_fit_normal` (two launches) + "
             "`gcfr_light_fit_solve` (one)." % res["ridge"],
             "- Leg B: the same call with `nonnegative=True`: the same normal equations + `gcfr_light_fit_solve_nonneg` (one launch, "
             "one wave per face and channel, one factorisation per step).",
             "- The photograph is `albedo x sum_l x_true final_l` in f64, rounded once to f32, under a {0,1} weight of 70 % ones: "
             "`all-positive` draws x_true uniformly in [0.2, 1], `mixed-sign` in [-0.5, 1.5].",
             "- `solves`: factorisations per (face, channel) as the entry reports them, smallest .. largest (mean) over the 24 systems; "
             "the cap is 3 L.", "",
             "| faces x lights x pixels | rig | unconstrained, us | non-negative, us | difference, us | solves | cap | entries < 0 "
             "unconstrained | entries = 0 non-negative | same bits |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---|"]
    for c in res["cases"]:
        B, L, H, W = c["shape"]
        lines.append("| %d x %d x (%d x %d) | %s | %s | %s | %.1f | %d .. %d (%.1f) | %d | %d of %d | %d of %d | %s |"
                     % (B, L, H, W, c["rig"], fmt(c["unconstrained"]), fmt(c["nonnegative"]),
                        c["nonnegative"]["median_us"] - c["unconstrained"]["median_us"], c["solves_min"], c["solves_max"], c["solves_mean"],
                        c["cap"], c["unconstrained_negative"], c["entries"], c["nonnegative_zero"], c["entries"],
                        "yes" if c["same_bits"] else "no"))
    lines += ["", "Per factorisation, (non-negative - unconstrained) / mean solves: " + "; ".join(
        "%.1f us at %d lights, %s" % ((c["nonnegative"]["median_us"] - c["unconstrained"]["median_us"]) / max(c["solves_mean"], 1.0),
                                      c["shape"][1], c["rig"]) for c in res["cases"]) + " (the slowest of the 24 waves sets the time, "
              "so this is an upper estimate).", "",
              "**Would reusing the factor's leading columns between inner steps be worth building?**  No.  The factorisation runs in "
              "ascending LIGHT index -- that order is what makes the last factorisation the unconstrained solve's, bit for bit -- so a "
              "step keeps only the columns of the lights below the lowest index that entered or left.  Counted on the restatement's "
              "passive sets at 64 lights (33 x 47 pixels; a count, not a measurement of this tool), that shortens a lane's dependent "
              "multiply-subtract chain by 1.27x to 1.47x (all-positive rig, 64 factorisations: 43680 -> 31000 .. 33300; mixed-sign, 56 "
              "factorisations: 24372 -> 16631) and leaves the two substitutions and every barrier where they are.  A factor kept in "
              "ADMISSION order would append one column per step (L^2 / 2 instead of L^3 / 6 for an all-positive rig), but it gives up "
              "the bit equality with `gcfr_light_fit_solve` and needs a downdate for every removal; it is not built."]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
