#!/usr/bin/env python3
"""Memory operations of a march kernel's epilogue, in program order, from the ISA (CPU; needs hipcc).

    tools/epilogue_memops.py [--kernel shadow_fwd_quad_kernelILi16ELb1ELi4ELb1ELi0E] [--csrc DIR] [--check] [-DMACRO ...]

Compiles csrc/gcfr_march_unit.hip (default shape, the flags of build.py) to gfx950 assembly and lists, for the LAST of the
kernel's epilogues in the text -- everything behind the last sample loop up to s_endpgm -- the scalar loads, vector loads,
vector stores, waits and branches in order, with the number of VALU / scalar ALU instructions between them
(profiles/epilogue_loads_ab.txt).  --csrc: another copy of csrc/ (an earlier commit's).
--check: every kernel of the unit; fails if a vector load can follow a vector store on a path that ends in s_endpgm without an
unconditional branch, or a wave-uniform branch to the kernel's exit, in between."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fno-fast-math", "-munsafe-fp-atomics"]
MEM = r"(global_|buffer_|flat_|scratch_|s_load|s_buffer_load|s_waitcnt|s_endpgm|s_cbranch|s_branch)"
VLOAD, VSTORE = r"\b(global|buffer|flat|scratch)_load", r"\b(global|buffer|flat|scratch)_store"


def assembly(csrc, defines):
    with tempfile.TemporaryDirectory(prefix="gcfr_memops_") as tmp:
        out = os.path.join(tmp, "march.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-DGCFR_UNIT_TILE_W=16", "-DGCFR_UNIT_GROUP=4"] + defines +
                       ["--cuda-device-only", "-S", os.path.join(csrc, "gcfr_march_unit.hip"), "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def kernels(lines):
    """[(name, first line, line of its last s_endpgm)]"""
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN4gcfr\w+:", l)]
    out = []
    for n, (i, name) in enumerate(starts):
        stop = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        ends = [j for j in range(i, stop) if lines[j].strip() == "s_endpgm"]
        out.append((name, i, ends[-1]))
    return out


def sequence(lines, first, end):
    in_loop = [i for i in range(first, end) if lines[i].startswith(".LBB") and "Loop" in lines[i]]
    start = next(i for i in range(in_loop[-1] + 1, end) if lines[i].startswith(".LBB") and "Loop" not in lines[i])
    valu = salu = 0
    rows = []

    def flush():
        nonlocal valu, salu
        if valu or salu:
            rows.append("        ... %d VALU, %d scalar ALU" % (valu, salu))
        valu = salu = 0
    for i in range(start, end + 1):
        t = lines[i].strip()
        if not t or t.startswith(";"):
            continue
        if re.match(MEM, t) or t.startswith(".LBB"):
            flush()
            rows.append("    " + re.sub(r"\s+", " ", t.split(";")[0]).strip())
        elif t.startswith("v_"):
            valu += 1
        elif t.startswith("s_"):
            salu += 1
    flush()
    return rows


def loads_behind_stores(lines, first, end):
    """(store line, load line) pairs: a vector load in the fall-through text of a vector store, before any unconditional branch"""
    bad = []
    for i in range(first, end):
        if re.search(VSTORE, lines[i]):
            for j in range(i + 1, end + 1):
                t = lines[j].strip()
                if re.match(r"(s_endpgm|s_branch|s_setpc)", t):
                    break
                if re.search(VLOAD, t):
                    bad.append((i + 1, j + 1))
                    break
    return bad


def main():
    args = sys.argv[1:]
    kernel, csrc, check, defines = "shadow_fwd_quad_kernelILi16ELb1ELi4ELb1ELi0E", os.path.join(ROOT, "geomconsistentfr_amd", "csrc"), False, []
    while args:
        a = args.pop(0)
        if a == "--kernel":
            kernel = args.pop(0)
        elif a == "--csrc":
            csrc = os.path.abspath(args.pop(0))
        elif a == "--check":
            check = True
        else:
            defines.append(a)
    lines = assembly(csrc, defines)
    ks = kernels(lines)
    if check:
        total = 0
        for name, first, end in ks:
            # A kernel's text continues, behind an epilogue's stores, with march_grid's wave-uniform tests (which instantiation runs,
            # `rough`) -- scalar branches to the kernel's exit, which a tile that has stored takes -- and then the next instantiation's
            # prologue: loads behind such a branch are not behind the store.
            label_at = {lines[i].split(":")[0]: i for i in range(first, end) if lines[i].startswith(".LBB")}

            def to_exit(label, depth=0):  # the text from `label` reaches s_endpgm with no vector load on the way
                for k in range(label_at.get(label, end), end + 1):
                    t = lines[k].strip()
                    if t == "s_endpgm":
                        return True
                    if re.search(VLOAD, t):
                        return False
                    m = re.match(r"s_branch\s+(\S+)", t)
                    if m:
                        return depth < 4 and to_exit(m.group(1), depth + 1)
                return False

            def leaves(k):
                m = re.match(r"s_cbranch_(scc[01]|vccn?z)\s+(\S+)", lines[k].strip())
                return bool(m) and to_exit(m.group(2))
            bad = [(s_, l) for s_, l in loads_behind_stores(lines, first, end) if not any(leaves(k) for k in range(s_, l))]
            total += len(bad)
            print("%-90s %d vector store(s) with a load behind them" % (name, len(bad)))
        sys.exit(1 if total else 0)
    hit = [k for k in ks if kernel in k[0]]
    if len(hit) != 1:
        sys.exit("kernel %r: %d matches" % (kernel, len(hit)))
    print("%s: the last epilogue, from the end of the last sample loop to s_endpgm" % hit[0][0])
    print("\n".join(sequence(lines, hit[0][1], hit[0][2])))


if __name__ == "__main__":
    main()
