#!/usr/bin/env python3
"""Digest what the diffusion path around the U-Net computes and launches, comparable between two checkouts.

    python scripts/path_parity.py OUT.json [--tree DIR] [--only NAME_SUBSTRING]

A fixed matrix on the TINY net at 16 x 16, N = 4 and N = 16 (N == W switches the reference's broadcast quirk D10 on), F32 and BF16:

  train/...    two steps each of `run_replay`, `run_device` as a graph and `run_device` eager (a fresh net each), for every
               `shift_type` and the base trainer (mean_shift=False), thresholding with a 1- and a 3-channel mask and indexing,
               `loss_weight_use` on and off.  After every step: sha256 of x_t, mask, s, x_in, mean_pixel, w, amount, ratio,
               model.t_in, loss.raw -- and of store.G / store.P in F32 only: in BF16 the bias gradients are summed by fp32
               atomics in an order that changes from run to run, so they, the parameters they update and with them the second
               step's loss are left out.
  sampler/...  T = 8: the graph loop, the host-driven loop with device RNG and with replay RNG (history off and on), for the
               three mask dependencies (`dependent_t` where `_check_dependent_args` lets it run) times the two momentum modes:
               sha256 of x0 and of every history tensor.

Next to the digests, the launch trace of the recordings this code emits -- the train step's front and tail, the sampler's
`body` and `last`: entry point names in order, every non-pointer argument, and null / non-null for every pointer
(`_lib._PROTOS` tells which is which).

`--tree DIR` imports `mdm` from another checkout (DIR/masked-diffusion-model_amd), e.g. a `git worktree` of the parent commit;
MDM_LIB_PATH gives both runs the same library.  Only what both sides of the emitter refactor have is used.  One case per
line; two files from the same behaviour are byte-identical: `cmp a.json b.json`.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

TINY = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[False, True])
HW = 16
SHIFTS = ["non_shift", "1-d_constant", "3-d_constant", "noise_reduction", "noise_with_perturbation", "noise_std_reduction", "base"]
# (name, select_degrade_pixel, degrade_channel, ddpm_schedule, mean_option, mean_area): the three mask sources, three fill modes
# ('degraded_area' on the exponential schedule, ratios 0.1 .. 1: no image without a degraded pixel, whose mean would be NaN)
MASKS = [("thr1", "thresholding", "1-channel", "linear", 0, "image-wise"),
         ("thr3", "thresholding", "3-channel", "exponential", "degraded_area", "channel-wise"),
         ("index", "indexing", None, "log", "non_degraded_area", "image-wise")]
# (dependency, mask row of MASKS or a dependent_t one, shift_type)
SAMPLER = [("independent", MASKS[0], "noise_with_perturbation"), ("independent", MASKS[2], "noise_reduction"),
           ("dependent_prev", MASKS[1], "noise_std_reduction"), ("dependent_prev", MASKS[2], "1-d_constant"),
           ("dependent_t", ("thr1da", "thresholding", "1-channel", "exponential", "degraded_area", "image-wise"), "noise_with_perturbation"),
           ("dependent_t", ("thr3s0", "thresholding", "3-channel", "linear", "0", "channel-wise"), "3-d_constant")]


def make_args(torch, **kw):
    a = argparse.Namespace(
        data_size=HW, in_channel=3, out_channel=3, batch_size=4, ddpm_num_steps=8, updated_ddpm_num_steps=8, ddpm_schedule="linear",
        ddpm_schedule_base=10.0, scheduler_num_scale_timesteps=1, select_degrade_pixel="thresholding", degrade_channel="1-channel",
        mean_option=0, mean_area="image-wise", shift_type="noise_with_perturbation", noise_mean=0.25, sample_latent_shape="uniform",
        momentum_adaptive="base_momentum", sampling_mask_dependency="independent", sample_num=4, loss_weight_use=False,
        loss_weight_power_base=10.0, weight_dtype=torch.float32, seed=11, rng_mode="device")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def trace(_lib, rec):
    """[[entry point, [argument | "null" | "ptr", ...]], ...] of a Recording."""
    scalars = (_lib.i32, _lib.i64, _lib.u64, _lib.f32)
    out = []
    for name, fn, args in rec.calls:
        if name == "note":
            out.append([name])
            continue
        vals = []
        for v, typ in zip(args, _lib._PROTOS[name][0]):
            if typ in scalars:
                vals.append(v)
            else:
                vals.append("null" if v is None or v == 0 or getattr(v, "value", 1) in (None, 0) else "ptr")
        out.append([name, vals])
    return out


def train_cases(torch, mdm, _lib, TrainStep):
    for N in (4, 16):
        for dt, dname in ((mdm.F32, "f32"), (mdm.BF16, "bf16")):
            for st in SHIFTS:
                for mname, sel, ch, sched_kind, mo, ma in MASKS:
                    for lw in (False, True):
                        yield f"train/n{N}/{dname}/{st}/{mname}/lw{int(lw)}", (lambda N=N, dt=dt, st=st, sel=sel, ch=ch, k=sched_kind, mo=mo,
                                                                                ma=ma, lw=lw: train_case(torch, mdm, _lib, TrainStep, N, dt, st, sel,
                                                                                                         ch, k, mo, ma, lw))


def train_case(torch, mdm, _lib, TrainStep, N, dt, st, sel, ch, sched_kind, mo, ma, lw):
    x0 = torch.rand(N, 3, HW, HW, generator=torch.Generator().manual_seed(100)) * 2 - 1
    out = {}
    for mode in ("replay", "device_graph", "device_eager"):
        model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=dt, seed=0)
        optim = mdm.AdamW(model, lr=1e-3)
        a = make_args(torch, batch_size=N, ddpm_schedule=sched_kind, select_degrade_pixel=sel, degrade_channel=ch, mean_option=mo, mean_area=ma,
                      shift_type="noise_with_perturbation" if st == "base" else st, loss_weight_use=lw,
                      rng_mode="replay" if mode == "replay" else "device", use_graph=mode == "device_graph")
        S = mdm.Scheduler(a)
        S.update_ddpm_num_steps(a.ddpm_num_steps)
        used = S.get_timesteps_epoch(0, 1)
        step = TrainStep(model, S, a, optim, None, mean_shift=st != "base")
        torch.manual_seed(21)
        for k in range(2):
            (step.run_replay if mode == "replay" else step.run_device)(x0.cuda(), used)
            torch.cuda.synchronize()
            d = {n: sha(getattr(step, n)) for n in ("x_t", "mask", "s", "x_in", "mean_pixel", "w", "amount", "ratio")}
            d["t_in"] = sha(model.t_in)
            if dt == mdm.F32 or k == 0:
                d["loss_raw"] = sha(step.loss.raw)
            if dt == mdm.F32:
                d["G"], d["P"] = sha(model.store.G), sha(model.store.P)
            out[f"{mode}/step{k}"] = d
        if mode == "device_eager":           # the recordings `_build_graphs` makes of this code
            with _lib.Recording() as front:
                step._emit_device_front()
            with _lib.Recording() as tail:
                step.opt.emit_update(None, step.max_norm, 1.0)
                step._emit_commit(True)
            out["trace"] = dict(front=trace(_lib, front), tail=trace(_lib, tail))
    return out


def sampler_cases(torch, mdm, _lib):
    models = {}
    for N in (4, 16):
        for dt, dname in ((mdm.F32, "f32"), (mdm.BF16, "bf16")):
            for dep, mask, st in SAMPLER:
                for mom in ("base_sampling", "base_momentum"):
                    def run(N=N, dt=dt, dep=dep, mask=mask, st=st, mom=mom):
                        if (N, dt) not in models:       # forward-only: one net serves every case of its batch and dtype
                            models[N, dt] = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=dt, seed=0).eval()
                        return sampler_case(torch, mdm, _lib, models[N, dt], N, dep, mask, st, mom)
                    yield f"sampler/n{N}/{dname}/{dep}/{mask[0]}/{st}/{mom}", run


def sampler_case(torch, mdm, _lib, model, N, dep, mask, st, mom):
    _, sel, ch, sched_kind, mo, ma = mask
    out = {}
    loops = [("graph", "device", False, True), ("host_device", "device", False, False), ("host_device_hist", "device", "device", False),
             ("host_replay", "replay", False, False), ("host_replay_hist", "replay", "device", False)]
    for name, rng_mode, hist_mode, graph in loops:
        a = make_args(torch, ddpm_schedule=sched_kind, select_degrade_pixel=sel, degrade_channel=ch, mean_option=mo, mean_area=ma, shift_type=st,
                      sampling_mask_dependency=dep, momentum_adaptive=mom, sample_num=N, sample_history=hist_mode, rng_mode=rng_mode,
                      sampler_graph=graph)
        S = mdm.Scheduler(a)
        S.update_ddpm_num_steps(a.ddpm_num_steps)
        smp = mdm.Sampler(None, a, S, [None] * 3)
        torch.manual_seed(31)
        x0, hist = smp.sample(model, S.get_timesteps_epoch(0, 1))
        torch.cuda.synchronize()
        out[name] = dict(x0=sha(x0), hist=[sha(h) for h in hist])
        if graph:
            _, gb, gl = smp._graph_keep
            out["trace"] = dict(body=trace(_lib, gb.rec), last=trace(_lib, gl.rec))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import mdm from (default: the one this script lies in)")
    ap.add_argument("--only", default=None, help="only the cases whose name contains this")
    opt = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(opt.tree), "masked-diffusion-model_amd"))
    import torch
    import mdm
    from mdm import _lib
    from mdm.train_step import TrainStep
    assert os.path.abspath(mdm.__file__).startswith(os.path.abspath(opt.tree)), mdm.__file__
    out, t0 = {}, time.time()
    cases = list(train_cases(torch, mdm, _lib, TrainStep)) + list(sampler_cases(torch, mdm, _lib))
    for i, (name, run) in enumerate(cases):
        if opt.only and opt.only not in name:
            continue
        out[name] = run()
        if len(out) % 20 == 0:
            print(f"{len(out)} cases, {time.time() - t0:.0f} s (at {name})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        for name in sorted(out):
            f.write(json.dumps({name: out[name]}, sort_keys=True, separators=(",", ":")) + "\n")
    whole = hashlib.sha256(open(opt.out, "rb").read()).hexdigest()
    print(f"wrote {opt.out}: {sum(n.startswith('train/') for n in out)} train cases, {sum(n.startswith('sampler/') for n in out)} sampler "
          f"cases, sha256 {whole}")


if __name__ == "__main__":
    main()
