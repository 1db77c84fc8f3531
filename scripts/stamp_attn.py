#!/usr/bin/env python3
"""Where the short-sequence attention kernels spend their cycles: attn_fwd_kernel<256> / attn_bwd_kernel<256> at the train step's
shapes (N, L, C) = (32, 64, 256) and (32, 16, 256).

    [MDM_LIB_PATH=build.so] python scripts/stamp_attn.py [N=32]

Always prints the graph-timed launch (20 launches in one captured graph, so without the host's launch cost).  With a library
built with `make EXTRA=-DMDM_STAMP` it also prints cycles per wave for the segments
    entry -> operands in LDS | first product | softmax / dS | second product | stores
(mean over the waves that multiplied anything, and the slowest of them from entry to its last store; the counters of different
XCDs are not synchronised, so no span across waves is printed), once COLD -- q/k/v, o, dO and lse
were just rewritten by copy kernels, as in the step, where the projection gemm writes them right before -- and once WARM: the
same launch again on untouched inputs.  Every stamp drains the wave's memory counters, so stamped kernels run slower than the
shipped ones: the segments tell where the time goes, the graph-timed figure tells how much there is."""
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "masked-diffusion-model_amd"))
import numpy as np
import torch
from mdm import _lib, ops

dev = torch.device("cuda:0")
lib = _lib.load()
fn = getattr(lib, "mdm_debug_stamps_attn", None)
if fn is not None:
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
SEG = ("entry->LDS", "product 1", "softmax/dS", "product 2", "stores")
KIND = {1: "fwd", 2: "bwd dQ", 3: "bwd dK/dV"}


def stamps():
    buf = (ctypes.c_ulonglong * (4096 * 8))()
    assert fn(buf, 1) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(4096, 8).astype(np.float64)
    return a[a[:, 7] > 0]


def ev():
    e = ctypes.c_void_p()
    _lib.check(lib.mdm_event_create(ctypes.byref(e)))
    return e


def timeit(f, reps=20):
    f()
    torch.cuda.synchronize()
    with _lib.Recording() as rec:
        for _ in range(reps):
            f()
    gx = _lib.GraphExec(rec)
    gx.launch()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    a, b = ev(), ev()
    lib.mdm_event_record(a, st)
    gx.launch()
    lib.mdm_event_record(b, st)
    ms = ctypes.c_float()
    _lib.check(lib.mdm_event_elapsed_ms(a, b, ctypes.byref(ms)))
    return ms.value * 1e3 / reps


def report(tag, a):
    for kind in sorted(set(a[:, 7].astype(int))):
        r = a[a[:, 7] == kind]
        busy = r[r[:, 2] + r[:, 4] > 0] if (r[:, 2] + r[:, 4] > 0).any() else r      # waves that multiplied anything
        m = busy.mean(0)
        segs = " | ".join(f"{n} {v:.0f}" for n, v in zip(SEG, m[1:6]))
        print(f"    {tag} {KIND[kind]:9s}: {segs} cyc  (sum {m[1:6].sum():.0f}; waves {len(r)}, of them multiplying {len(busy)}; "
              f"slowest wave, entry -> stores done {(busy[:, 6] - busy[:, 0]).max():.0f} cyc)")


N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
C = 256
bf = torch.bfloat16
for L in (64, 16):
    scale = 1.0 / math.sqrt(C)
    g = torch.Generator().manual_seed(L)
    src_qkv = torch.randn(N, L, 3 * C, generator=g).to(dev, bf)
    src_do = torch.randn(N, L, C, generator=g).to(dev, bf)
    qkv, do = torch.empty_like(src_qkv), torch.empty_like(src_do)
    o, lse = torch.empty(N, L, C, device=dev, dtype=bf), torch.empty(N, L, device=dev)
    o_in, lse_in = torch.empty_like(o), torch.empty_like(lse)
    delta, dqkv = torch.empty(N, L, device=dev), torch.empty_like(qkv)
    fwd = lambda: ops.attn_fwd(1, qkv, o, lse, N, L, C, scale)
    bwd = lambda: ops.attn_bwd(1, qkv, o_in, do, lse_in, delta, dqkv, N, L, C, scale)

    def rewrite():          # every input of both directions written by a kernel right before the launch under test
        qkv.copy_(src_qkv)
        do.copy_(src_do)
        o_in.copy_(o)
        lse_in.copy_(lse)

    qkv.copy_(src_qkv)
    do.copy_(src_do)
    fwd()
    rewrite()
    bwd()
    torch.cuda.synchronize()
    print(f"N={N} L={L} C={C}: routes {_lib.attn_route_of(0, 1, L, C)} / {_lib.attn_route_of(1, 1, L, C)} | graph-timed "
          f"fwd {timeit(fwd):.2f} us, bwd {timeit(bwd):.2f} us per launch")
    if fn is None:
        continue
    for name, f in (("fwd", fwd), ("bwd", bwd)):
        rewrite()
        torch.cuda.synchronize()
        stamps()
        f()
        torch.cuda.synchronize()
        report("cold", stamps())
        f()
        torch.cuda.synchronize()
        report("warm", stamps())
