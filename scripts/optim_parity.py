#!/usr/bin/env python3
"""Digest what the optimizer pass and the two split-shadow kernels compute, comparable between two checkouts bit for bit.

    python scripts/optim_parity.py OUT.txt [--tree DIR] [--sizes N,N,...]

Seeded fp32 buffers at two lengths -- N_BIG of tests/test_optimizers_gpu.py (past one sweep of the capped grid, whole groups and a
tail) and the cfg2 store size scripts/prof_optimizers.py prints (unet6 preset at 32 x 32) --, three consecutive steps of every
optimizer variant below through the C entry point, for the five clip cases of tests/_optim_ref.py, with and without the EMA and
bf16-shadow pointers.  AdamW goes through `mdm_adamw_ema` where the loaded library exports it and through `mdm_optim_update`,
kind 3, where it does not: the names of the cases do not say which, so two files from the same arithmetic are equal.  After the
third step: sha256 of p, of the state buffers the kind has, and of the EMA and the shadow where they were given.

`agree/...` lines say whether Adam and AdamW, both at weight_decay = 0 and from the same inputs, gave the same bits: mathematically
they are one formula there, but each kernel's sums of two products are contracted as the compiler chose.

`split/...`: `mdm_split_shadow` and `mdm_split_shadow_t` over a table of two filters (9 taps 64 x 32, 1 tap 32 x 24).

`--tree DIR` imports `mdm`, and with it that checkout's library, from DIR/masked-diffusion-model_amd.  One case per line;
`cmp a.txt b.txt`.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

N_BIG = 2048 * 256 * 8 + 1003
SGD, SGD_M, ADAM, ADAMW = 0, 1, 2, 3
# name -> (kind, lr, hyper-parameters)
VARIANTS = {
    "sgd": (SGD, 0.1, {}),
    "sgd_momentum_dampening_wd": (SGD_M, 0.1, dict(momentum=0.9, dampening=0.5, weight_decay=0.1)),
    "sgd_nesterov": (SGD_M, 0.1, dict(momentum=0.9, nesterov=True)),
    "adam": (ADAM, 1e-3, {}),
    "adam_wd": (ADAM, 1e-2, dict(weight_decay=0.1)),
    "adamw": (ADAMW, 1e-3, dict(weight_decay=1e-2)),
    "adamw_wd": (ADAMW, 1e-2, dict(weight_decay=0.1)),
    "adamw_wd0": (ADAMW, 1e-3, {}),
}
CLIPS = [(6.25, 1.0, 1.0), (6.25, 1.0, 0.5), (0.25, 1.0, 1.0), (0.25, 1.0, 0.5), (6.25, 0.0, 0.5)]      # (sqnorm, max_norm, gmul)
EMA_DECAYS = (0.0, 0.4, 0.7)


def hp_block(torch, kind, step, lr, ema_decay, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """The 8 floats of include/mdm_hip.h for the optimizer's step `step` (1-based)."""
    if kind >= ADAM:
        b1, b2 = 0.9, 0.999
        h = [lr, b1, b2, 1e-8, weight_decay, 1 - b1 ** step, 1 - b2 ** step, ema_decay]
    else:
        first = kind == SGD or step == 1
        h = [lr, momentum, 0.0 if first else momentum, 1.0 if first else 1.0 - dampening, weight_decay, float(nesterov), 0.0, ema_decay]
    return torch.tensor(h, dtype=torch.float32)


def sha(torch, t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def optimizer_cases(torch, _lib, n, out):
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    p0, g0, e0 = (torch.randn(n, generator=gen) for _ in range(3))
    p0[::7] *= 1e-3
    p0, g0, e0 = p0.to(dev), g0.to(dev), e0.to(dev)
    grads = [torch.roll(g0, k).contiguous() for k in (1, 2, 3)]
    old_adamw = "mdm_adamw_ema" in _lib.EXPORTS
    for name, (kind, lr, kw) in VARIANTS.items():
        for ci, (sq, mx, gm) in enumerate(CLIPS):
            sqn = torch.tensor([sq], device=dev)
            for with_ema in (False, True):
                P, S0, S1, E = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), e0.clone()
                SH = torch.zeros(n, device=dev, dtype=torch.bfloat16)
                ema, shadow = (_lib.ptr(E), _lib.ptr(SH)) if with_ema else (None, None)
                for k in (1, 2, 3):
                    hp = hp_block(torch, kind, k, lr, EMA_DECAYS[k - 1], **kw).to(dev)
                    tail = (n, _lib.ptr(hp), _lib.ptr(sqn), mx, gm, _lib.stream())
                    if kind == ADAMW and old_adamw:
                        _lib.call("mdm_adamw_ema", _lib.ptr(P), _lib.ptr(grads[k - 1]), _lib.ptr(S0), _lib.ptr(S1), ema, shadow, *tail)
                    else:
                        _lib.call("mdm_optim_update", kind, _lib.ptr(P), _lib.ptr(grads[k - 1]), _lib.ptr(S0) if kind >= SGD_M else None,
                                  _lib.ptr(S1) if kind >= ADAM else None, ema, shadow, *tail)
                torch.cuda.synchronize()
                d = dict(p=sha(torch, P))
                if kind >= SGD_M:
                    d["s0"] = sha(torch, S0)
                if kind >= ADAM:
                    d["s1"] = sha(torch, S1)
                if with_ema:
                    d["ema"], d["shadow"] = sha(torch, E), sha(torch, SH)
                out[f"optim/n{n}/{name}/clip{ci}/ema{int(with_ema)}"] = d
    for ci in range(len(CLIPS)):
        for e in (0, 1):
            a, b = (out[f"optim/n{n}/{v}/clip{ci}/ema{e}"] for v in ("adam", "adamw_wd0"))
            out[f"agree/n{n}/adam_and_adamw_at_wd0/clip{ci}/ema{e}"] = {k: a[k] == b[k] for k in a}


def split_cases(torch, _lib, out):
    dev = torch.device("cuda")
    filters = [(9, 64, 32), (1, 32, 24)]
    offs, size = [], 0
    for taps, co, ci in filters:
        offs.append(size)
        size += taps * co * ci
    P = torch.randn(size, generator=torch.Generator().manual_seed(2)).to(dev)
    P[::5] *= 1e-4
    segs = torch.tensor([(o, t * co * ci) for o, (t, co, ci) in zip(offs, filters)], dtype=torch.int64, device=dev)
    segs_t = torch.tensor([(o, t, co, ci) for o, (t, co, ci) in zip(offs, filters)], dtype=torch.int64, device=dev)
    Ps, PsT = torch.zeros_like(P), torch.zeros_like(P)
    _lib.call("mdm_split_shadow", _lib.ptr(P), _lib.ptr(Ps), _lib.ptr(segs), len(filters), _lib.stream())
    _lib.call("mdm_split_shadow_t", _lib.ptr(P), _lib.ptr(PsT), _lib.ptr(segs_t), len(filters), _lib.stream())
    torch.cuda.synchronize()
    out["split/two_filters"] = dict(Ps=sha(torch, Ps), PsT=sha(torch, PsT))


def cfg2_store_size(torch, mdm):
    model = mdm.UNet(mdm.unet6_config(32), N=32, H=32, W=32, dtype=mdm.BF16, seed=0)
    return int(model.store.size)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import mdm from (default: the one this script lies in)")
    ap.add_argument("--sizes", default=None, help="comma-separated lengths instead of N_BIG and the cfg2 store size")
    opt = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(opt.tree), "masked-diffusion-model_amd"))
    import torch
    import mdm
    from mdm import _lib
    assert os.path.abspath(mdm.__file__).startswith(os.path.abspath(opt.tree)), mdm.__file__
    sizes = [int(x) for x in opt.sizes.split(",")] if opt.sizes else [N_BIG, cfg2_store_size(torch, mdm)]
    out = {}
    for n in sizes:
        optimizer_cases(torch, _lib, n, out)
        print(f"n = {n}: {len(out)} lines so far", flush=True)
    split_cases(torch, _lib, out)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        for name in sorted(out):
            f.write(name + " " + " ".join(f"{k}={v}" for k, v in sorted(out[name].items())) + "\n")
    agree = [all(v.values()) for k, v in out.items() if k.startswith("agree/")]
    print(f"wrote {opt.out}: {len(out)} lines, sha256 {hashlib.sha256(open(opt.out, 'rb').read()).hexdigest()}; "
          f"Adam and AdamW at weight_decay 0 agree in {sum(agree)} of {len(agree)} cases")


if __name__ == "__main__":
    main()
