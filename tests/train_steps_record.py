"""Records an optimiser trajectory and compares two of them: the instrument behind tests/golden/t8_train_steps.npz
(oracle/make_golden_train_steps.py: six iterations of the reference's own training loop on CPU) and
tests/test_gpu_train_steps.py (the same six iterations through Trainer on the GPU).

Every optimiser step is seen through torch.optim's global step hooks (Adam.step of either network).  Before the step: each
parameter tensor's gradient -- L2 norm, sum, and a fixed sample of its elements (positions from `sample_index`, stored with the
fixture).  After it: the parameter's distance from its initial value (norm, sum, the same sample) and the L2 norms of Adam's two
moment estimates.  A gradient that is None counts as zero (zero_grad() sets them to None)."""
import zlib

import numpy as np
import torch

N_SAMPLE = 16
NETS = ("G", "D")
PRINTED = ("Total loss", "Reconstruction loss", "Depth loss", "Ambient loss", "Lighting loss", "Albedo loss",
           "Generator loss", "Discriminator loss", "Discriminator Real loss", "Discriminator Fake loss", "DSSIM loss")   # T8:658-668
LOG_KEY = {"Total loss": "total", "Reconstruction loss": "recon", "Depth loss": "depth", "Ambient loss": "ambient",
           "Lighting loss": "lighting", "Albedo loss": "albedo", "Generator loss": "generator", "DSSIM loss": "DSSIM",
           "Discriminator loss": "discriminator"}          # (Trainer logs the discriminator's two terms as one sum)
STATS = ("grad_norm", "grad_sum", "grad_sample", "delta_norm", "delta_sum", "delta_sample", "m_norm", "v_norm")


def sample_index(name, numel, k=N_SAMPLE):
    if numel <= k:
        return np.arange(numel, dtype=np.int64)
    return np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(numel, k, replace=False)).astype(np.int64)


def index_of(fixture):
    """The sample positions a fixture was recorded with: {net: [positions of each parameter tensor, in name order]}."""
    return {tag: np.split(fixture[tag + "_index"], np.cumsum(fixture[tag + "_counts"])[:-1]) for tag in NETS}


def pre_bn_bias(name, names):
    """The bias of a convolution whose output goes straight into a training-mode BatchNorm: its gradient is zero up to rounding
    (the BatchNorm subtracts the batch mean), so it is noise on both sides and Adam turns that noise into full-size steps."""
    if not name.endswith(".bias"):
        return False
    mod = name[:-len(".bias")]
    for pre in ("deconv", "conv"):
        if mod.startswith(pre):
            return "bn" + mod[len(pre):] + ".weight" in names
    return False


class StepRecorder:
    """`add(tag, net)` each network (its parameters now are the initial ones), then run the optimiser steps inside `with rec:`,
    setting `rec.iteration` before each iteration.  `arrays()` -> the dict stored in / compared with the fixture."""

    def __init__(self, index=None):
        self.params, self.p0, self.index, self._idx = {}, {}, dict(index or {}), {}
        self.iteration, self.steps, self._pending = 0, [], None

    def add(self, tag, net):
        named = sorted(net.named_parameters())
        self.params[tag] = named
        self.p0[tag] = [p.detach().clone() for _, p in named]
        if tag not in self.index:
            self.index[tag] = [sample_index(n, p.numel()) for n, p in named]
        self._idx[tag] = [torch.from_numpy(np.asarray(i)).to(p.device) for i, (_, p) in zip(self.index[tag], named)]

    def _tag(self, opt):
        first = id(opt.param_groups[0]["params"][0])
        for tag, named in self.params.items():
            if any(id(p) == first for _, p in named):
                return tag
        return None

    def _stats(self, tag, tensors):
        norms, sums, samples = [], [], []
        for (_, p), t, idx in zip(self.params[tag], tensors, self._idx[tag]):
            t = torch.zeros_like(p) if t is None else t
            t = t.detach().reshape(-1).double()
            norms.append(t.norm())
            sums.append(t.sum())
            samples.append(t[idx])
        return (torch.stack(norms).cpu().numpy(), torch.stack(sums).cpu().numpy(),
                torch.cat(samples).float().cpu().numpy())

    def _pre(self, opt, _args, _kwargs):
        tag = self._tag(opt)
        if tag is not None:
            r = dict(net=tag, iteration=self.iteration)
            r["grad_norm"], r["grad_sum"], r["grad_sample"] = self._stats(tag, [p.grad for _, p in self.params[tag]])
            self._pending = r

    def _post(self, opt, _args, _kwargs):
        tag = self._tag(opt)
        if tag is None:
            return
        r, self._pending = self._pending, None
        named = self.params[tag]
        r["delta_norm"], r["delta_sum"], r["delta_sample"] = self._stats(tag, [p.detach() - p0 for (_, p), p0 in zip(named, self.p0[tag])])
        state = [opt.state[p] for _, p in named]
        r["m_norm"] = self._stats(tag, [s.get("exp_avg") for s in state])[0]
        r["v_norm"] = self._stats(tag, [s.get("exp_avg_sq") for s in state])[0]
        self.steps.append(r)

    def __enter__(self):
        from torch.optim.optimizer import register_optimizer_step_post_hook, register_optimizer_step_pre_hook
        self._handles = [register_optimizer_step_pre_hook(self._pre), register_optimizer_step_post_hook(self._post)]
        return self

    def __exit__(self, *exc):
        for h in self._handles:
            h.remove()
        return False

    def arrays(self):
        out = {"step_net": np.array([NETS.index(r["net"]) for r in self.steps], np.int64),
               "step_iter": np.array([r["iteration"] for r in self.steps], np.int64)}
        for tag, named in self.params.items():
            rs = [r for r in self.steps if r["net"] == tag]
            out[tag + "_names"] = np.array([n for n, _ in named])
            out[tag + "_index"] = np.concatenate(self.index[tag]).astype(np.int64)
            out[tag + "_counts"] = np.array([len(i) for i in self.index[tag]], np.int64)
            out[tag + "_iter"] = np.array([r["iteration"] for r in rs], np.int64)
            for s in STATS:
                out[tag + "_" + s] = np.stack([r[s] for r in rs]) if rs else np.zeros((0,))
        return out


def compare(ref, ours, logs, tol, n_iter=6):
    """The reference trajectory `ref` (fixture dict) against `ours` (StepRecorder.arrays()) and Trainer's per-iteration `logs`,
    for the first `n_iter` iterations.  `tol[kind][j]` for kind in loss / grad / m / v / delta bounds the relative differences
    of iteration j.  Returns (mismatches: list of str, observed: dict of the largest relative difference of each kind per step).
    Beyond the bounds: the order of the optimiser steps, a gradient that is zero on one side only, and on each network's FIRST
    step the sign of the update of every sampled element whose reference gradient is above 4x the sample's measured difference."""
    bad, obs = [], {}
    sched = lambda a: [(NETS[int(n)], int(i)) for n, i in zip(a["step_net"], a["step_iter"]) if i < n_iter]
    if sched(ref) != sched(ours):
        bad.append("schedule: reference steps %s, here %s" % (sched(ref), sched(ours)))
    d_iters = {i for n, i in sched(ref) if n == "D"}
    for j in range(n_iter):
        worst = 0.0
        for col, key in enumerate(PRINTED):
            k = LOG_KEY.get(key)
            if k is None or (k == "discriminator" and j not in d_iters):
                continue
            r = float(ref["printed"][j, col])
            if k not in logs[j]:
                bad.append("iteration %d: %s not logged" % (j, key))
                continue
            e = abs(logs[j][k] - r) / max(abs(r), 1e-12)
            worst = max(worst, e)
            if e > tol["loss"][j]:
                bad.append("iteration %d %s: %.9g, reference %.9g (rel %.2e)" % (j, key, logs[j][k], r, e))
        obs["loss_%d" % j] = worst
    for tag in NETS:
        names = [str(n) for n in ref[tag + "_names"]]
        if [str(n) for n in ours[tag + "_names"]] != names:
            bad.append("%s: other parameter names than the reference's" % tag)
            continue
        counts = ref[tag + "_counts"]
        live0 = ~np.array([pre_bn_bias(n, set(names)) for n in names])
        split = lambda a: np.split(a, np.cumsum(counts)[:-1])
        for s_ref, j in enumerate(ref[tag + "_iter"]):
            hits = np.nonzero(ours[tag + "_iter"] == j)[0]
            if j >= n_iter or not len(hits):
                continue
            R = {s: ref[tag + "_" + s][s_ref] for s in STATS}
            O = {s: ours[tag + "_" + s][hits[0]] for s in STATS}
            key = "%s%d" % (tag, j)
            zr, zo = R["grad_norm"] == 0, O["grad_norm"] == 0
            for i in np.nonzero(zr != zo)[0]:
                bad.append("%s %s: gradient %s in the reference, %s here" % (key, names[i], "zero" if zr[i] else "non-zero",
                                                                               "zero" if zo[i] else "non-zero"))
            live = live0 & ~zr & ~zo
            for stat, kind in (("grad_norm", "grad"), ("m_norm", "m"), ("v_norm", "v"), ("delta_norm", "delta")):
                e = np.where(live, np.abs(O[stat] - R[stat]) / np.maximum(np.abs(R[stat]), 1e-300), 0.0)
                obs["%s_%s" % (key, stat)] = float(e.max())
                for i in np.nonzero(e > tol[kind][j])[0]:
                    bad.append("%s %s: %s %.6g, reference %.6g (rel %.2e)" % (key, names[i], stat, O[stat][i], R[stat][i], e[i]))
            gr, go = split(R["grad_sample"].astype(np.float64)), split(O["grad_sample"].astype(np.float64))
            worst = 0.0
            for i in np.nonzero(live)[0]:
                nr = np.linalg.norm(gr[i])
                if nr == 0:
                    continue
                e = np.linalg.norm(go[i] - gr[i]) / nr
                worst = max(worst, e)
                if e > tol["grad"][j]:
                    bad.append("%s %s: sampled gradient elements differ by %.2e (relative L2)" % (key, names[i], e))
            obs[key + "_grad_sample"] = worst
            if s_ref == 0:
                dr, do = split(R["delta_sample"]), split(O["delta_sample"])
                checked = 0
                for i in np.nonzero(live)[0]:
                    sel = np.abs(gr[i]) > 4 * np.abs(go[i] - gr[i]).max()
                    checked += int(sel.sum())
                    flip = np.nonzero(np.sign(do[i][sel]) != np.sign(dr[i][sel]))[0]
                    if len(flip):
                        bad.append("%s %s: first update has the other sign on %d sampled element(s)" % (key, names[i], len(flip)))
                obs[key + "_sign_checked"] = checked
    return bad, obs
