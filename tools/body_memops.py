#!/usr/bin/env python3
"""Texel gathers, prefetch loads and vmcnt waits of the march kernels' executed group bodies, in program order, from the ISA
(CPU; needs hipcc).

    tools/body_memops.py [--kernel SUBSTRING] [--csrc DIR] [--check] [-DMACRO ...]

Compiles csrc/gcfr_march_unit.hip (default shape, the flags of build.py, -gline-tables-only: the line table says which source
line a load belongs to, debug info does not change code) to gfx950 assembly and lists, per kernel of the unit and per group
body in its text -- from the body's first texel gather to the wait that leaves none outstanding --, every vector load with its
kind (texel: the 16-B quad gather of a sample; mask / record: the next group's prefetch; other) and every `s_waitcnt vmcnt(n)`
with the number of texel gathers outstanding in front of it and behind it (vmcnt counts vector memory operations in issue
order; the listing follows the text, which is the executed order inside a body: its only branches skip masked lanes'
evaluations).  Between them the number of VALU / scalar instructions (profiles/body_pipeline_memops.txt).
--csrc: another copy of csrc/ (an earlier commit's).  --check: fails unless every body of the fused six-wave inference grid
kernels' main loops (the bodies with the prefetch inside) has two texel gathers outstanding at its first wait."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fno-fast-math", "-munsafe-fp-atomics"]


def assembly(csrc, defines):
    with tempfile.TemporaryDirectory(prefix="gcfr_bodyops_") as tmp:
        out = os.path.join(tmp, "march.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-DGCFR_UNIT_TILE_W=16", "-DGCFR_UNIT_GROUP=4"] + defines +
                       ["--cuda-device-only", "-gline-tables-only", "-S", os.path.join(csrc, "gcfr_march_unit.hip"), "-o", out],
                       check=True, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def load_lines(csrc):
    """source line -> kind, for the 16-byte buffer loads the march issues itself (gcfr_march.hpp)"""
    kinds = {}
    with open(os.path.join(csrc, "gcfr_march.hpp")) as f:
        for n, text in enumerate(f, 1):
            if "raw_buffer_load_b128(" in text:
                kinds[n] = "texel" if "(qr," in text else ("record" if "(zr, off" in text else "other")
    return kinds


def kernels(lines):
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN4gcfr\w+:", l)]
    out = []
    for n, (i, name) in enumerate(starts):
        stop = next((j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end")), len(lines))
        out.append((name, i, stop))
    return out


def bodies(lines, first, end, kinds, march_file):
    """[(label the body's first gather sits behind, rows, texels outstanding at the first wait, prefetch loads inside)]"""
    out = []
    i = first
    label, cur_line, cur_file = "", 0, 0
    while i < end:
        t = lines[i].strip()
        if lines[i].startswith(".LBB"):
            label = lines[i].split(":")[0]
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            cur_file, cur_line = int(m.group(1)), int(m.group(2))
        if t.startswith("buffer_load_dwordx4") and cur_file in march_file and kinds.get(cur_line) == "texel":
            rows, queue, valu, salu, texels, first_wait, prefetch = [], [], 0, 0, 0, None, 0

            def flush():
                nonlocal valu, salu
                if valu or salu:
                    rows.append("        ... %d VALU, %d scalar" % (valu, salu))
                valu = salu = 0
            j = i
            while j < end:
                u = lines[j].strip()
                m = re.match(r"\.loc\s+(\d+)\s+(\d+)", u)
                if m:
                    cur_file, cur_line = int(m.group(1)), int(m.group(2))
                elif lines[j].startswith(".LBB"):
                    flush()
                    rows.append("    " + lines[j].split(":")[0] + ":")
                elif re.match(r"(buffer|global|flat|scratch)_(load|store|atomic)", u):
                    flush()
                    if u.startswith("buffer_load_ubyte"):
                        kind = "mask"
                    elif u.startswith("buffer_load_dwordx4") and cur_file in march_file:
                        kind = kinds.get(cur_line, "other")
                    else:
                        kind = "other"
                    queue.append(kind)
                    texels += kind == "texel"
                    prefetch += kind in ("mask", "record")
                    rows.append("    %-28s %s" % (u.split()[0], kind))
                elif u.startswith("s_waitcnt") and "vmcnt" in u:
                    flush()
                    n = int(re.search(r"vmcnt\((\d+)\)", u).group(1))
                    before = queue.count("texel")
                    del queue[:max(0, len(queue) - n)]
                    rows.append("    %-28s texel gathers outstanding: %d in front, %d behind" % (re.sub(r"\s+", " ", u.split(";")[0]).strip(), before, queue.count("texel")))
                    if first_wait is None:
                        first_wait = before
                    if not queue.count("texel") and texels >= 1 and not re.match(r"buffer_load", lines[j + 1].strip()):
                        # (the next texel gather of the same body follows the evaluation behind this wait)
                        k = j + 1
                        more = False
                        while k < end and not re.match(r"s_(cbranch_(scc|vcc)|branch|endpgm)", lines[k].strip()):
                            if lines[k].strip().startswith("buffer_load_dwordx4"):
                                more = True
                                break
                            k += 1
                        if not more:
                            break
                elif re.match(r"s_(branch|endpgm|cbranch_(scc|vcc))", u):
                    flush()
                    rows.append("    " + re.sub(r"\s+", " ", u.split(";")[0]).strip())
                    if not queue.count("texel"):
                        break
                elif u.startswith("v_"):
                    valu += 1
                elif u.startswith("s_") and not u.startswith("s_nop"):
                    salu += 1
                j += 1
            flush()
            out.append((label, rows, first_wait, prefetch, texels))
            i = j
        i += 1
    return out


def main():
    args = sys.argv[1:]
    kernel, csrc, check, defines = "", os.path.join(ROOT, "geomconsistentfr_amd", "csrc"), False, []
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
    march_file = {int(m.group(1)) for l in lines for m in [re.match(r'\s*\.file\s+(\d+)\s+.*gcfr_march\.hpp"', l)] if m}
    kinds = load_lines(csrc)
    bad = 0
    for name, first, end in kernels(lines):
        if kernel not in name:
            continue
        found = bodies(lines, first, end, kinds, march_file)
        print("%s: %d group bodies" % (name, len(found)))
        for n, (label, rows, first_wait, prefetch, texels) in enumerate(found):
            print("  body %d (behind %s): %d texel gathers, %d prefetch loads inside, %s texel gathers outstanding at the first wait" %
                  (n, label, texels, prefetch, first_wait))
            if not check:
                print("\n".join(rows))
            if check and re.search(r"22shadow_fwd_quad_kernelILi\d+ELb[01]ELi[24]ELb1E", name) and prefetch and texels >= 2 and first_wait != 2:
                bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
