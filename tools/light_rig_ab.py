#!/usr/bin/env python
"""A/B of the light-rig stage (lighting.combine_lights, csrc/gcfr_light_rig.hip) against the torch composition it replaces.

  leg A (the baseline)   (final[:, :, None] * rgb[..., None, None]).sum(1) * albedo   and its autograd
  leg B                  combine_lights(final, albedo, rgb)

at 8 faces x 18 lights x 512^2 and 8 faces x 11 lights x 256^2, forward alone and forward + backward (a random gradient on
`rendered`, gradients with respect to final, albedo and the rig).  One process, one device; per shape and mode the two legs
ALTERNATE (A, B, A, B, ...): every repeat is `--iters` calls between two in-stream events behind a device synchronise, after
`--warmup` untimed calls per leg; reported are the median over `--repeats` repeats and their spread (min .. max).  Beside them the
bytes the kernel has to move (from the shapes) and the achieved rate against gcfr_copy_probe timed the same way in the same run.
Needs a GPU: there is no fallback.

usage: tools/light_rig_ab.py [--repeats 7] [--iters 20] [--warmup 5] [--json PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 18, 512, 512), (8, 11, 256, 256)]


def kernel_bytes(B, L, H, W, backward):
    """what the stage has to move: forward reads 4 L + 12 and writes 24 bytes per pixel (rendered + shading_rgb); the backward
    (g_rendered alone) reads 4 L + 24 (final, albedo, g_rendered) and writes 4 L + 12 (g_final, g_albedo)"""
    px = B * H * W
    fwd = px * (4 * L + 12 + 24)
    return fwd + (px * (4 * L + 24 + 4 * L + 12) if backward else 0)


def torch_bytes(B, L, H, W):
    """the forward of leg A at the least: the (B,L,3,H,W) product written and read back (24 L), its inputs, the sum written and read,
    the albedo product"""
    return B * H * W * (24 * L + 4 * L + 12 + 12 + 12 + 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("light_rig_ab.py needs a GPU (a timing taken anywhere else says nothing)")
    from geomconsistentfr_amd import _lib, build, combine_lights
    dev = torch.device("cuda:0")
    L_ = _lib.load()

    def timed(fn):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / a.iters * 1e3            # us per call

    def summary(v):
        return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"commit": commit, "library_source_hash": build.source_hash()[:16], "device": torch.cuda.get_device_name(dev),
           "repeats": a.repeats, "iters": a.iters, "warmup": a.warmup, "shapes": []}

    # the copy probe: as many bytes as the large shape's forward moves, half read and half written
    n = kernel_bytes(*SHAPES[0], False) // 2 // 16 * 16
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    probe = lambda: _lib.check(L_.gcfr_copy_probe(src.data_ptr(), dst.data_ptr(), n, st), "gcfr_copy_probe")
    for _ in range(a.warmup):
        probe()
    probe_us = [timed(probe) for _ in range(a.repeats)]
    res["copy_probe"] = dict(summary(probe_us), bytes=2 * n, TBs=2 * n / statistics.median(probe_us) / 1e6)
    del src, dst

    for B, L, H, W in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(L)
        final = (1.2 * torch.rand(B, L, H, W, generator=g)).to(dev)
        albedo = (0.1 + 0.8 * torch.rand(B, 3, H, W, generator=g)).to(dev)
        rgb = torch.rand(B, L, 3, generator=g).to(dev) / L
        G = torch.randn(B, 3, H, W, generator=g).to(dev)
        leaves = [t.clone().requires_grad_() for t in (final, albedo, rgb)]

        def leg_a(backward):
            f, al, r = leaves if backward else (final, albedo, rgb)
            out = (f[:, :, None] * r[..., None, None]).sum(1) * al
            if backward:
                return torch.autograd.grad(out, leaves, G)
            return out

        def leg_b(backward):
            f, al, r = leaves if backward else (final, albedo, rgb)
            out, _ = combine_lights(f, al, r)
            if backward:
                return torch.autograd.grad(out, leaves, G)
            return out

        with torch.no_grad():
            same = float((leg_a(False) - leg_b(False)).abs().max())
        ga, gb = leg_a(True), leg_b(True)
        gdiff = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(gb, ga)]
        entry = {"shape": [B, L, H, W], "forward_max_abs_diff": same, "gradient_max_rel_diff": gdiff}
        for mode, backward in (("forward", False), ("forward_backward", True)):
            def run(leg):
                if backward:
                    return leg(True)
                with torch.no_grad():
                    return leg(False)
            for leg in (leg_a, leg_b):
                for _ in range(a.warmup):
                    run(leg)
            ta, tb = [], []
            for _ in range(a.repeats):                        # interleaved
                ta.append(timed(lambda: run(leg_a)))
                tb.append(timed(lambda: run(leg_b)))
            nb = kernel_bytes(B, L, H, W, backward)
            entry[mode] = {"torch": summary(ta), "hip": summary(tb), "kernel_bytes": nb,
                           "torch_forward_bytes_at_least": torch_bytes(B, L, H, W),
                           "hip_TBs": nb / statistics.median(tb) / 1e6,
                           "hip_share_of_copy_probe": nb / statistics.median(tb) / 1e6 / res["copy_probe"]["TBs"]}
        res["shapes"].append(entry)
        del leaves, final, albedo, rgb, G
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
