#!/usr/bin/env python3
"""Generate tests/golden/unet_resample.npz by RUNNING THE REFERENCE's unet6.UNet with resample_with_conv=False in train mode.

    python tests/golden/make_resample_golden.py

Needs the reference checkout (absent on the GPU box: the fixture is committed).  Only inputs / outputs are stored: the net is the
3-level NET3 of tests/_resample_ref.py (two pools, two bare upsamples; one seam changes the channel count, one does not), its
parameters are oracle.unet_ref.random_params(NET3, SEED) restricted to the keys the reference model has -- the fixture stores the
seed and the reference's state_dict key list, not the weights.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import REF, _stub_modules, npy, seed_all  # noqa: E402  (also puts the repository root on sys.path)
from oracle.unet_ref import random_params  # noqa: E402
from _resample_ref import NET3  # noqa: E402

SEED, N, HW = 2468, 2, 16
GRADS = ("in_conv.weight", "downsamples.level_1.0.0.conv1.weight", "upsamples.level_1.1.0.skip.weight", "out_conv.2.bias")


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    from models.unet import unet6
    torch.set_num_threads(4)
    cfg = NET3
    m = unet6.UNet(cfg["in_channels"], cfg["hid_channels"], cfg["out_channels"], cfg["ch_multipliers"], cfg["num_res_blocks"],
                   cfg["apply_attn"], resample_with_conv=False)
    keys = list(m.state_dict().keys())
    full = random_params(cfg, SEED)
    assert [k for k in full if k in set(keys)] == keys, "state_dict key grammar mismatch"
    m.load_state_dict({k: full[k] for k in keys})
    m.train()
    g = torch.Generator().manual_seed(19)
    x = torch.rand(N, 3, HW, HW, generator=g) * 2 - 1
    t = torch.tensor([5.0, 730.0])
    gy = torch.randn(N, 3, HW, HW, generator=g)
    seed_all(23)
    y = m(x, t)
    (y * gy).sum().backward()
    out = dict(seed=np.array(SEED), x=npy(x), t=npy(t), gy=npy(gy), y=npy(y), keys=np.array(keys))
    sd = dict(m.named_parameters())
    for k in GRADS:
        out["grad::" + k] = npy(sd[k].grad)
    path = os.path.join(HERE, "unet_resample.npz")
    np.savez_compressed(path, **out)
    print(f"unet_resample: {len(out)} arrays, {len(keys)} keys ({len(full) - len(keys)} fewer than the conv model) -> {path} "
          f"({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
