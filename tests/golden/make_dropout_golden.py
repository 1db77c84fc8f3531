#!/usr/bin/env python3
"""Generate tests/golden/unet_dropout.npz by RUNNING THE REFERENCE's unet6.UNet with drop_rate > 0 in train mode.

    python tests/golden/make_dropout_golden.py

Needs /root/reference (absent on the GPU box: the fixture is committed).  Only inputs / outputs are stored.  The keep mask of
every ResidualBlock.dropout (unet6.py:354, 360) is captured with a forward pre-hook (a clone of the in-place module's input) and
a forward hook (`out != 0`), so the oracle can replay the same forward with the masks made explicit (tests/_dropout_ref.py).
The parameters are oracle.unet_ref.random_params(TINY, SEED): the fixture stores the seed, not the weights.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, TINY, _stub_modules, npy, seed_all  # noqa: E402  (also puts the repository root on sys.path)
from oracle.unet_ref import random_params  # noqa: E402

SEED, RATE, N, HW = 4321, 0.3, 2, 8
GRADS = ("in_conv.weight", "middle.0.conv2.weight", "out_conv.2.bias")


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    from models.unet import unet6
    torch.set_num_threads(4)
    cfg = TINY
    m = unet6.UNet(cfg["in_channels"], cfg["hid_channels"], cfg["out_channels"], cfg["ch_multipliers"], cfg["num_res_blocks"],
                   cfg["apply_attn"], drop_rate=RATE)
    p = random_params(cfg, SEED)
    assert list(m.state_dict().keys()) == list(p.keys()), "state_dict key grammar mismatch"
    m.load_state_dict(p)
    m.train()
    masks, pending = {}, {}
    for name, mod in m.named_modules():
        if isinstance(mod, unet6.ResidualBlock):
            assert mod.dropout.p == RATE and mod.dropout.inplace

            def pre(_mod, args, name=name):
                pending[name] = args[0].detach().clone()

            def post(_mod, _args, out, name=name):
                assert name not in masks and bool((pending[name] != 0).all()), name     # no exact zero in front of the dropout
                masks[name] = (out.detach() != 0)
            mod.dropout.register_forward_pre_hook(pre)
            mod.dropout.register_forward_hook(post)
    g = torch.Generator().manual_seed(17)
    x = torch.rand(N, 3, HW, HW, generator=g) * 2 - 1
    t = torch.tensor([5.0, 730.0])
    gy = torch.randn(N, 3, HW, HW, generator=g)
    seed_all(23)
    y = m(x, t)
    (y * gy).sum().backward()
    out = dict(seed=np.array(SEED), rate=np.array(RATE), scale=np.array(1.0 / (1.0 - RATE)), x=npy(x), t=npy(t), gy=npy(gy), y=npy(y),
               sites=np.array(list(masks)))
    for name, k in masks.items():
        out["mask::" + name] = np.packbits(k.numpy().reshape(-1))
        out["shape::" + name] = np.array(k.shape)
    sd = dict(m.named_parameters())
    for k in GRADS:
        out["grad::" + k] = npy(sd[k].grad)
    keep = sum(int(k.sum()) for k in masks.values()) / sum(k.numel() for k in masks.values())
    path = os.path.join(HERE, "unet_dropout.npz")
    np.savez_compressed(path, **out)
    print(f"unet_dropout: {len(out)} arrays, {len(masks)} sites, keep fraction {keep:.4f} -> {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
