"""Deterministic initial weights for the training-trajectory fixture (tests/golden/t8_train_steps.npz).

Every weight and bias of every convolution, transposed convolution and linear layer is drawn from
U(-1/sqrt(fan_in), +1/sqrt(fan_in)) -- PyTorch's default bounds, fan_in as `nn.init` computes it -- by numpy's PCG64 seeded
with (seed, crc32 of the parameter's name).  The same names therefore get the same values in any module that declares them (the
reference's networks and their mirrors, whose state_dicts are interchangeable) on any machine.  BatchNorm keeps its defaults
(weight 1, bias 0, running statistics 0 / 1)."""
import zlib

import numpy as np
import torch
import torch.nn as nn

SEED_G, SEED_D = 8, 15          # RelightNet, PatchGAN


def seeded_init_(module: nn.Module, seed: int) -> nn.Module:
    with torch.no_grad():
        for mname, m in module.named_modules():
            if not isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
                continue
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(m.weight)
            bound = 1.0 / np.sqrt(fan_in)
            for pname, p in m.named_parameters(recurse=False):
                name = (mname + "." if mname else "") + pname
                rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
                p.copy_(torch.from_numpy(rng.uniform(-bound, bound, tuple(p.shape)).astype(np.float32)))
    return module
