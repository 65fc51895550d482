#!/usr/bin/env python
"""A/B of rig capture (lighting.fit_light_rgb, csrc/gcfr_light_fit.hip) against the torch composition a user would write.

  leg A (the baseline)   f64 einsum for G and r over the (B,3,P,L) weighted design, the relative ridge, torch.linalg.solve, rounded
                         to f32:    D = sqrt(w) a_c f_l;  G = D^T D;  r = D^T (sqrt(w) I_c);  x = solve(G + ridge tr(G) / L I, r)
  leg B                  fit_light_rgb(final, albedo, image, weight, ridge): the normal equations (two launches) + the solve (one)
  at 8 faces x 11 lights x 256 x 256 and 8 x 64 x 256 x 256, a {0,1} weight of 70 % ones per face.

One process, one device, no profiler attached.  Per case the two legs ALTERNATE (A, B, A, B, ...): every repeat is `--iters` calls
between two in-stream events behind a device synchronise, after `--warmup` untimed calls per leg; reported are the median over
`--repeats` repeats and their spread (min .. max).  The times are per CALL and include what the host does per call (allocation of
outputs and of the workspace, launches).  Beside the times, per pixel and face: the kernel's f64 operations (3 per entry: two
products and one sum; 2 more conversions f32 -> f64) and LDS reads (3 per entry), with 3 L (L + 3) / 2 entries -- arithmetic, not
counters.  Needs a GPU: there is no fallback.  Writes the table as Markdown to `--out` (default profiles/light_fit_ab.md) and
prints the same numbers as JSON.

usage: tools/light_fit_ab.py [--repeats 7] [--iters 10] [--warmup 3] [--out PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 11, 256, 256), (8, 64, 256, 256)]      # (B, L, H, W)
RIDGE = 1e-3


def counts(L):
    """per pixel and face: (entries, f64 products and sums, f32 -> f64 conversions, LDS reads, LDS bytes read)"""
    n = 3 * (L * (L + 3) // 2)
    return n, 3 * n, 2 * n, 3 * n, 16 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_fit_ab.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("light_fit_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    from geomconsistentfr_amd import build, fit_light_rgb, light_normal_equations
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
        g = torch.Generator(device="cpu").manual_seed(L + B)
        u = lambda *s: (0.05 + 0.95 * torch.rand(*s, generator=g)).to(dev)
        final, albedo, image = u(B, L, H, W), u(B, 3, H, W), u(B, H, W, 3)
        weight = (torch.rand(B, H, W, generator=g) < 0.7).float().to(dev)

        def leg_a():
            sw = weight.to(torch.float64).sqrt().reshape(B, 1, H * W)
            D = (sw * albedo.to(torch.float64).reshape(B, 3, H * W))[..., None] * final.to(torch.float64).reshape(B, 1, L, H * W).transpose(2, 3)
            t = sw * image.to(torch.float64).reshape(B, H * W, 3).transpose(1, 2)
            G = torch.einsum("bcpl,bcpm->bclm", D, D)
            r = torch.einsum("bcpl,bcp->bcl", D, t)
            A = G + (RIDGE / L) * torch.diagonal(G, dim1=2, dim2=3).sum(-1)[..., None, None] * torch.eye(L, dtype=torch.float64, device=dev)
            return torch.linalg.solve(A, r).transpose(1, 2).float()                   # (B,L,3)

        def leg_b():
            return fit_light_rgb(final, albedo, image, weight, ridge=RIDGE)

        def leg_n():
            return light_normal_equations(final, albedo, image, weight)

        with torch.no_grad():
            xa, xb = leg_a(), leg_b()
            diff = float((xa - xb).abs().max() / xa.abs().max())
            for leg in (leg_a, leg_b, leg_n):
                for _ in range(a.warmup):
                    leg()
            ta, tb, tn = [], [], []
            for _ in range(a.repeats):                        # interleaved
                ta.append(timed(leg_a, a.iters))
                tb.append(timed(leg_b, a.iters))
                tn.append(timed(leg_n, a.iters))
        n, flops, cvts, reads, lds_bytes = counts(L)
        res["cases"].append({"shape": [B, L, H, W], "rel_diff": diff, "torch": summary(ta), "hip": summary(tb), "hip_normal_only": summary(tn),
                             "entries": n, "f64_ops_per_pixel": flops, "cvt_per_pixel": cvts, "lds_reads_per_pixel": reads,
                             "f64_Gops": (flops + cvts) * B * H * W / statistics.median(tn) / 1e3,
                             "lds_TBs": lds_bytes * B * H * W / statistics.median(tn) / 1e6})
        print("case %s done" % (res["cases"][-1]["shape"],), file=sys.stderr, flush=True)
        del final, albedo, image, weight
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    write_table(res, a)


def write_table(res, a):
    cmd = "python tools/light_fit_ab.py" + "".join(" --%s %s" % (k, getattr(a, k)) for k in ("repeats", "iters", "warmup"))
    fmt = lambda s: "%.1f (%.1f .. %.1f)" % (s["median_us"], s["min_us"], s["max_us"])
    lines = ["# Rig capture (`fit_light_rgb`) against the torch composition (one MI355X)", "",
             "`%s` (%slibrary source hash `%s`, the first 16 digits of `build.source_hash()`; %s).  One process, one device, no "
             "profiler attached." % (cmd, "commit %s; " % res["commit"] if res["commit"] else "", res["library_source_hash"], res["device"]), "",
             "Per case the legs alternate A, B, A, B, ...: %d repeats behind %d untimed calls per leg, each repeat %d calls between two "
             "in-stream events behind a device synchronise.  Median and (min .. max) of the repeats, microseconds per CALL, including "
             "what the host does per call (allocation of outputs and workspace, launches); kernel times were not traced separately."
             % (a.repeats, a.warmup, a.iters), "",
             "- Leg A, the baseline: the f64 `einsum` for `G` and `r` over the (B,3,HW,L) weighted design, the relative ridge, "
             "`torch.linalg.solve`, rounded to f32.",
             "- Leg B: `lighting.fit_light_rgb(final, albedo, image, weight, ridge=%g)`: `gcfr_light_fit_normal` (two launches) + "
             "`gcfr_light_fit_solve` (one)." % res["ridge"],
             "- `normal equations alone`: `lighting.light_normal_equations` on the same inputs, timed in the same alternation.", "",
             "| faces x lights x pixels | torch composition | `fit_light_rgb` | ratio | normal equations alone | largest relative difference |",
             "|---|---:|---:|---:|---:|---:|"]
    for c in res["cases"]:
        B, L, H, W = c["shape"]
        lines.append("| %d x %d x (%d x %d) | %s | %s | %.2fx | %s | %.1e |"
                     % (B, L, H, W, fmt(c["torch"]), fmt(c["hip"]), c["torch"]["median_us"] / c["hip"]["median_us"], fmt(c["hip_normal_only"]),
                        c["rel_diff"]))
    lines += ["", "What the partials kernel does per pixel and face (ARITHMETIC from the kernel's loop, not counters), and the rates the "
              "measured time of the normal equations alone then implies:", "",
              "| lights | entries | f64 products + sums | f32 -> f64 conversions | LDS reads (8 + 4 + 4 bytes per entry) | implied f64-rate "
              "instructions | implied LDS read rate |", "|---:|---:|---:|---:|---:|---:|---:|"]
    for c in res["cases"]:
        lines.append("| %d | %d | %d | %d | %d | %.0f G/s | %.1f TB/s |" % (c["shape"][1], c["entries"], c["f64_ops_per_pixel"], c["cvt_per_pixel"],
                                                                          c["lds_reads_per_pixel"], c["f64_Gops"], c["lds_TBs"]))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
