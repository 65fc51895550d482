#!/usr/bin/env python3
"""DESIGN.md section 4's kernel table from the committed profiles, not by hand (CPU).

    tools/design_table.py [--tag r05] [--write]

Reads profiles/pmc_summary.json (tools/summarize_profile.py: per dominant kernel the duration under rocprofv3, the VALU mix by class,
the HBM bytes per launch) and profiles/<tag>_{fwd,bwd}_kernel_stats.csv (prepass and the small kernels), prices the VALU mix at the
guide's SPEC issue rates (bench.py SPEC_CYCLES) and prints the Markdown table; --write replaces the block between
`<!-- kernel-table:begin -->` and `<!-- kernel-table:end -->` in DESIGN.md.  VGPRs / waves per SIMD are the forced occupancies
(`amdgpu_waves_per_eu`, asserted by tests/test_kernel_resources.py); algorithmic bytes per launch are stated here with their
derivation."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = {"ADD_F32": 2, "MUL_F32": 2, "FMA_F32": 2, "INT32": 2, "OTHER": 2, "ADD_F64": 4, "MUL_F64": 4, "FMA_F64": 4, "CVT": 4, "INT64": 4,
        "TRANS_F32": 8, "TRANS_F64": 16}
CAP = 1024 * 2.4e9
# algorithmic (compulsory) HBM bytes per launch
PIX = 256 * 256
ALGO = {
    # forward from depth, 8 faces x 1 light: reads depth 4 + mask 1 + albedo 12, writes quad texels 16 (+ re-read 16: L2-resident, not counted),
    # min_dist 4 + w 4 + full 4 + final 4 + rendered 12 + normals 12  -> 73.25 B / pixel -> 38.4 MB
    "fwd": 8 * PIX * 73.25,
    "fwd_b128": 128 * PIX * 73.25,
    "fwd_training_march": 32 * PIX * 77.25,      # + argmin 4
    "bwd": 32 * PIX * 72.0,                      # bench.py run_train: 72 B per pixel
}
STATIC = {   # what the profiles do not carry
    "fwd": ("`shadow_fwd_quad_kernel<16,true,4,true,0>` (`gcfr_march.hpp`)", "T8:353-354 (fused stencil), 364-522: march + normals + shade, inference", "80 / 6"),
    "fwd_b128": ("the same, ONE launch of 128 faces", "(how busy the chip is when it is full)", "80 / 6"),
    "fwd_training_march": ("`shadow_fwd_quad_argmin_kernel` (B = 32, smooth faces + noise 2)", "the same with argmin (training forward)", "95 / 5"),
    "bwd": ("`render_bwd_single_light_kernel` (`gcfr_backward.hip`, B = 32, dense upstream gradient)", "autograd of T8:353-522, one light per face", "128 / 4"),
}


def spec_frac(e):
    cyc = sum(e["valu"]["by_class"].get(k, 0.0) * c for k, c in SPEC.items())
    ns = e.get("avg_launch_ns_under_rocprofv3") or 0.0
    return cyc, (cyc / (CAP * ns * 1e-9) if ns else float("nan"))


def small_kernels(tag):
    out = {}
    for leg in ("fwd", "bwd"):
        p = os.path.join(ROOT, "profiles", "%s_%s_kernel_stats.csv" % (tag, leg))
        if not os.path.exists(p):
            continue
        for r in csv.DictReader(open(p)):
            name = r["Name"].split("(")[0].replace("void ", "").replace("gcfr::", "")
            out.setdefault(name, (float(r["AverageNs"]) / 1e3, int(r["Calls"]), leg))
    return out


def prepass_row(tag, name, what, sk):
    """the prepass' row from the counters the fwd leg's PMC passes collected for it (profiles/<tag>_fwd_pmc.json), or None.
    60 VGPRs, eight waves per SIMD (tests/test_kernel_resources.py: no scratch); algorithmic bytes per launch of 8 faces: depth 4 +
    mask 1 read, texels 16 B x 257^2 / 256^2 written -> ~21.1 B / pixel."""
    p = os.path.join(ROOT, "profiles", "%s_fwd_pmc.json" % tag)
    if not os.path.exists(p) or name not in sk:
        return None
    c = next((v for k, v in json.load(open(p)).items() if name in k), None)
    if not c or "SQ_INSTS_VALU" not in c:
        return None
    by = {k: c.get("SQ_INSTS_VALU_" + k, 0.0) for k in SPEC if k != "OTHER"}
    by["OTHER"] = max(c["SQ_INSTS_VALU"] - sum(by.values()), 0.0)
    us = sk[name][0]
    frac = sum(by[k] * SPEC[k] for k in by) / (CAP * us * 1e-6)
    hbm = (2.0 * c.get("FETCH_SIZE", 0.0) + c.get("WRITE_SIZE", 0.0)) * 1024.0
    algo = 8 * (PIX * 5.0 + 257 * 257 * 16.0)
    return "| `%s` | %s | %.1f us (%s profile, %d calls) | 60 / 8 | %.2f M (+ %.2f M scalar, %d waves) | %.2f (launch-sized: ~10 us of it is the launch floor) | %.0f %% | %.1f / %.1f MB = %.2f |" % (
        name, what, us, sk[name][2], sk[name][1], c["SQ_INSTS_VALU"] / 1e6, c.get("SQ_INSTS_SALU", 0.0) / 1e6, c.get("SQ_WAVES", 0),
        frac, 100.0 * c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"], hbm / 1e6, algo / 1e6, hbm / algo)


def main():
    args = sys.argv[1:]
    tag = args[args.index("--tag") + 1] if "--tag" in args else "r05"
    pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json")))
    rows = ["| kernel | replaces | duration (rocprofv3) | VGPR / waves per SIMD | VALU wave-instructions per launch | frac (spec issue rates) | wait share of wave time | HBM traffic / algorithmic |",
            "|---|---|---|---|---|---|---|---|"]
    for key in ("fwd", "fwd_b128", "fwd_training_march", "bwd"):
        e = pm.get("kernels", {}).get(key)
        if not e:
            continue
        name, what, occ = STATIC[key]
        cyc, frac = spec_frac(e)
        wait = (e["wait_any_quad"] / e["wave_cycles_quad"]) if e.get("wait_any_quad") and e.get("wave_cycles_quad") else float("nan")
        hbm = e["hbm"]["bytes_per_launch"]
        rows.append("| %s | %s | %.1f us | %s | %.2f M | %.2f | %.0f %% | %.1f / %.1f MB = %.2f |" % (
            name, what, e["avg_launch_ns_under_rocprofv3"] / 1e3, occ, e["valu"]["insts_per_launch"] / 1e6, frac, 100 * wait, hbm / 1e6,
            ALGO[key] / 1e6, hbm / ALGO[key]))
    sk = small_kernels(tag)
    for name, what in (("build_quad_kernel", "prepass: repack, statistics, bounds tiles, horizon tables, light prep T8:357-363 (`gcfr_shadow.hip`); own enqueue since ABI 5 (`gcfr_options.phase`)"),
                       ("light_prep_bwd_kernel", "autograd of T8:357-363")):
        pre = prepass_row(tag, name, what, sk) if name == "build_quad_kernel" else None
        if pre:
            rows.append(pre)
        elif name in sk:
            rows.append("| `%s` | %s | %.1f us (%s profile, %d calls) | -- | -- | -- (latency) | -- | ~1.0 |" % (name, what, sk[name][0], sk[name][2], sk[name][1]))
    table = "\n".join(rows)
    note = ("\n\n(generated by `tools/design_table.py --tag %s --write` from `profiles/pmc_summary.json`, library hash `%s`, and "
            "`profiles/%s_*_kernel_stats.csv`; frac = sum over VALU classes of wave-instructions x SPEC issue cycles / (1024 SIMDs x 2.4 GHz x duration))"
            % (tag, (pm.get("library_srchash") or "?")[:12], tag))
    print(table + note)
    if "--write" in args:
        p = os.path.join(ROOT, "DESIGN.md")
        s = open(p).read()
        a, b = "<!-- kernel-table:begin -->", "<!-- kernel-table:end -->"
        i, j = s.index(a) + len(a), s.index(b)
        open(p, "w").write(s[:i].rstrip(" ") + "\n" + table + note + "\n\n" + s[j:].lstrip(" "))


if __name__ == "__main__":
    main()
