#!/usr/bin/env python3
"""Describe the recorded launch plans of a matrix of nets as one JSON file, comparable between two processes.

    python scripts/plan_fingerprint.py OUT.json [--tree DIR] [--only NAME_SUBSTRING]

For every net of the matrix, `forward_plan` and `backward_plan` become a list with one entry per recorded call: the entry
point and every argument.  `mdm_gemm_desc` / `mdm_gn_desc` arguments are expanded field by field (`_fields_`), a grouped weight
gradient into the descriptors of its group, `note` entries appear by name only.  A descriptor is written as a dict WITHOUT its
zero / null fields (a field that is absent is zero), which keeps the file a few megabytes.  Every pointer is rewritten as
[index of the buffer that holds it, byte offset]; buffers are `net._bufs` in allocation order, then the store's P, G, Pb,
PbT, Ps, PsT, then the group tables -- so two processes (two checkouts) give the same text where they record the same
launches.  A pointer outside every known buffer is an error.  Next to the calls: `bwd_marks`, `sorted(overwritten)`,
`zero_floats`, `len(wgrad_groups)` and the FLOP table of each plan.

`--tree DIR` imports `mdm` from another checkout (DIR/masked-diffusion-model_amd), e.g. a `git worktree` of the parent commit;
MDM_LIB_PATH selects the library file for both.  Only attributes that a checkout before the plan/emit split also has are
used.  One process, no launches beyond what the constructors issue (parameter load, shadow emits).  Two files from the same
launches are byte-identical: `cmp a.json b.json`.

    python scripts/plan_fingerprint.py --summary FILE.json

prints, per net of such a file, the counts of the fusion decisions its launches show (no GPU, no mdm import): the figures
tests/test_unet_plan_cpu.py pins.
"""
from __future__ import annotations

import argparse
import bisect
import ctypes as C
import hashlib
import json
import os
import sys
import time

TINY = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[False, True])
CFG4 = dict(in_channels=4, hid_channels=128, out_channels=4, ch_multipliers=[1, 2, 2, 2], num_res_blocks=2, apply_attn=[True] * 4)


class Buffers:
    """Known device buffers of one net -> (index, offset) of a pointer."""

    def __init__(self, net):
        st = net.store
        self.tensors = list(net._bufs) + [getattr(st, k, None) for k in ("P", "G", "Pb", "PbT", "Ps", "PsT")]
        self.tensors += [g.table for g in net.wgrad_groups]
        spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), i)
                       for i, t in enumerate(self.tensors) if t is not None and t.numel())
        self.starts = [s[0] for s in spans]
        self.spans = spans

    def ref(self, p, what):
        if not p:
            return None
        k = bisect.bisect_right(self.starts, p) - 1
        if k < 0 or p >= self.spans[k][1]:
            raise SystemExit(f"plan_fingerprint: pointer {p:#x} ({what}) lies in no known buffer")
        return [self.spans[k][2], p - self.spans[k][0]]


def desc_fields(_lib, d, bufs, what):
    out = {}
    for name, typ in type(d)._fields_:
        v = getattr(d, name)
        if v:
            out[name] = bufs.ref(v, f"{what}.{name}") if typ is _lib.vp else v
    return out


def plan_entries(_lib, net, rec, bufs):
    groups = {g.handle.value: g for g in net.wgrad_groups}
    out = []
    for i, (name, fn, args) in enumerate(rec.calls):
        what = f"{name}#{i}"
        if name == "note":
            out.append([name])
        elif name == "mdm_wgrad_group_launch":
            grp = groups[args[0].value]
            out.append([name, [desc_fields(_lib, _lib._desc(f), bufs, what) for f in grp.keep]])
        else:
            types = _lib._PROTOS[name][0]
            vals = []
            for a, typ in zip(args, types):
                if isinstance(typ, type) and issubclass(typ, C._Pointer):
                    vals.append(desc_fields(_lib, a._obj, bufs, what))
                elif typ is _lib.vp:
                    vals.append(bufs.ref(a, what))
                else:
                    vals.append(a)
            out.append([name, vals])
    return out


def fingerprint(_lib, net):
    bufs = Buffers(net)
    fp = {}
    for key in ("forward_plan", "backward_plan"):
        rec = getattr(net, key)
        if rec is None:
            fp[key] = None
            continue
        fp[key] = dict(calls=plan_entries(_lib, net, rec, bufs), flops=[[i, f, dt] for i, (f, dt) in sorted(rec.flops.items())])
    fp["bwd_marks"] = [list(m) for m in net.bwd_marks] if net.backward_plan is not None else None
    fp["overwritten"] = sorted(net.overwritten)
    fp["zero_floats"] = net.zero_floats
    fp["wgrad_groups"] = len(net.wgrad_groups)
    fp["buffers"] = len(net._bufs)
    return fp


def summary(path):
    """Per net: how many launches of each fused / paired / grouped kind the recorded plans hold."""
    data = {}
    with open(path) as f:
        for line in f:
            data.update(json.loads(line))
    out = {}
    for name, fp in sorted(data.items()):
        c = dict(gn_fwd_fused=0, gn_bwd_fused=0, fwd_pairs=0, bwd_pairs=0, wgrad_grouped=0, wgrad_split=0, wgrad_single=0,
                 sums_by_norm=0, sums_by_wgrad=0, sums_by_colsum=0, attn_fused=0, attn_f32_small=0, dgrad_split=0, temb_skinny=0)
        for key in ("forward_plan", "backward_plan"):
            bwd = key == "backward_plan"
            for call in (fp[key] or {}).get("calls", []):
                nm, args = call[0], (call[1] if len(call) > 1 else [])
                descs = args if nm == "mdm_wgrad_group_launch" else [a for a in args if isinstance(a, dict)]
                if nm == "mdm_gemm_pair":
                    c["bwd_pairs" if bwd else "fwd_pairs"] += 1
                for d in descs:
                    c["gn_fwd_fused"] += "gnf_out" in d
                    c["gn_bwd_fused"] += "gnb_x" in d
                    c["sums_by_norm"] += "gnb_sum_all" in d
                    if bwd and d.get("conv") and d.get("layout") == 2:
                        c["wgrad_grouped" if nm == "mdm_wgrad_group_launch" else "wgrad_split" if nm == "mdm_conv_wgrad_split"
                          else "wgrad_single"] += 1
                        c["sums_by_wgrad"] += "dbias" in d
                    if bwd and nm == "mdm_gemm" and d.get("conv") and "B_split" in d:
                        c["dgrad_split"] += 1
                if nm == "mdm_groupnorm_bwd":
                    c["sums_by_norm"] += "sum_all" in args[0]
                if nm == "mdm_colsum" and args[2] > 1 or (nm == "mdm_colsum" and args[5] is not None):
                    c["sums_by_colsum"] += 1                            # a convolution's (the time-embedding path sums ONE image)
                c["attn_fused"] += nm == "mdm_attn_fwd"
                c["attn_f32_small"] += nm == "mdm_attn_f32_small_fwd"
                c["temb_skinny"] += (nm == "mdm_skinny_linear_fwd" and not bwd) / 3
        c["temb_skinny"] = int(round(c["temb_skinny"]))
        out[name] = c
        print(name, json.dumps(c, sort_keys=True))
    return out


def matrix(mdm):
    from mdm.unet2d import UNet2D, my_model_config
    u6 = mdm.unet6_config
    nets = [("tiny_n4_16", mdm.UNet, TINY, 4, 16), ("cfg2_n32", mdm.UNet, u6(32), 32, 32), ("cfg2_n100", mdm.UNet, u6(32), 100, 32),
            ("cfg3_n8", mdm.UNet, u6(64), 8, 64), ("cfg4_n16", mdm.UNet, CFG4, 16, 32), ("u128_n1", mdm.UNet, u6(128), 1, 128),
            ("unet2d_n4", UNet2D, my_model_config(3, 32, num_attention=1), 4, 32)]
    modes = [("bf16", dict(dtype=mdm.BF16)), ("f32", dict(dtype=mdm.F32)), ("f32_split", dict(dtype=mdm.F32, f32_products="split")),
             ("f32_split_grad", dict(dtype=mdm.F32, f32_products="split", grad_products="split"))]
    for name, cls, cfg, n, hw in nets:
        for mode, kw in modes:
            yield f"{name}/{mode}", (lambda cls=cls, cfg=cfg, n=n, hw=hw, kw=kw: cls(cfg, n, hw, hw, **kw))
    cfg2 = lambda **kw: mdm.UNet(u6(32), 32, 32, 32, dtype=mdm.BF16, **kw)
    yield "cfg2_n32/bf16/pair_convs=False", lambda: cfg2(pair_convs=False)
    yield "cfg2_n32/bf16/group_wgrads=False", lambda: cfg2(group_wgrads=False)
    yield "cfg2_n32/bf16/wgrad_group_bytes=32MiB", lambda: cfg2(wgrad_group_bytes=32 << 20)
    yield "cfg2_n32/bf16/with_uniform_t", lambda: cfg2().with_uniform_t()
    yield "cfg2_n32/bf16/with_batch(100)", lambda: cfg2().with_batch(100)
    for p in ("f32_split", "f32", "model"):
        yield f"cfg2_n32/bf16/sampling_plan(100,{p})", lambda p=p: cfg2().sampling_plan(100, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out", nargs="?")
    ap.add_argument("--summary", default=None, help="print the decision counts of a fingerprint file and exit")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import mdm from (default: the one this script lies in)")
    ap.add_argument("--only", default=None, help="only the nets whose name contains this")
    opt = ap.parse_args()
    if opt.summary:
        summary(opt.summary)
        return
    if not opt.out:
        ap.error("OUT.json is required")
    sys.path.insert(0, os.path.join(os.path.abspath(opt.tree), "masked-diffusion-model_amd"))
    import torch
    import mdm
    from mdm import _lib
    assert os.path.abspath(mdm.__file__).startswith(os.path.abspath(opt.tree)), mdm.__file__
    out = {}
    for name, make in matrix(mdm):
        if opt.only and opt.only not in name:
            continue
        t0 = time.time()
        net = make()
        torch.cuda.synchronize()
        out[name] = fingerprint(_lib, net)
        sha = hashlib.sha256(json.dumps(out[name], sort_keys=True).encode()).hexdigest()[:16]
        ncalls = sum(len(out[name][k]["calls"]) for k in ("forward_plan", "backward_plan") if out[name][k])
        print(f"{name}: {ncalls} calls, sha256 {sha}, {time.time() - t0:.1f} s", flush=True)
        del net
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        for name in sorted(out):          # one net per line
            f.write(json.dumps({name: out[name]}, sort_keys=True, separators=(",", ":")) + "\n")
    print(f"wrote {opt.out}: {len(out)} nets")


if __name__ == "__main__":
    main()
