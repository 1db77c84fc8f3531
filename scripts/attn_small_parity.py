#!/usr/bin/env python3
"""sha256 digests of what the fused attention kernels write at L <= 64, to compare two builds of the library bit for bit.

    MDM_LIB_PATH=old.so python scripts/attn_small_parity.py > old.txt
    python scripts/attn_small_parity.py > new.txt ; diff old.txt new.txt

Cases and inputs are those of tests/test_attn_small_gpu.py (attn_draw of tests/_bounds.py, both draws): N = 3 at every
L in {16, 32, 48, 64} x C in {32, 64, 128, 256}, plus (33, 64, 256) and (33, 16, 256).  The backward runs on o / lse made on the
CPU in fp64 from the same inputs (o -> bf16, lse -> fp32), so a forward that differs between the builds does not leak into the
backward's digests.  One line per case: N L C draw, then o lse delta dqkv (first 12 hex digits each)."""
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "masked-diffusion-model_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from _bounds import attn_draw
from mdm import ops

CASES = [(3, L, C) for L in (16, 32, 48, 64) for C in (32, 64, 128, 256)] + [(33, 64, 256), (33, 16, 256)]
dev = torch.device("cuda:0")


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:12]


for N, L, C in CASES:
    for kind in ("flat", "peaked"):
        qkv, do = attn_draw(N, L, C, kind, seed=1000 + L + C)
        scale = 1.0 / math.sqrt(C)
        q, k, v = (t.double() for t in (qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]))
        s = q @ k.transpose(1, 2) * scale
        lse_in = torch.logsumexp(s, -1).float().to(dev)
        o_in = (torch.softmax(s, -1) @ v).float().to(torch.bfloat16).to(dev)
        qkv, do = qkv.to(dev), do.to(dev)
        o, lse = torch.zeros(N, L, C, device=dev, dtype=torch.bfloat16), torch.zeros(N, L, device=dev)
        delta, dqkv = torch.zeros(N, L, device=dev), torch.zeros(N, L, 3 * C, device=dev, dtype=torch.bfloat16)
        ops.attn_fwd(1, qkv, o, lse, N, L, C, scale)
        ops.attn_bwd(1, qkv, o_in, do, lse_in, delta, dqkv, N, L, C, scale)
        torch.cuda.synchronize()
        print(f"{N:3d} {L:3d} {C:4d} {kind:7s} o {digest(o)} lse {digest(lse)} delta {digest(delta)} dqkv {digest(dqkv)}")
