#!/usr/bin/env python3
"""Benchmark of the masked-diffusion train step (and the 1k-step reverse sampler) on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload = BASELINE.json configs[1]: synthetic 32x3x32x32 per GPU, full unet6 from the reference's
`Model('unet6',3,32,32,3)` preset (35.75 M parameters, random init), bf16 compute, T=1000 linear
schedule with thresholding/1-channel masks, `noise_with_perturbation` shift (with the reference's
N==W broadcast), x0-space MSE, grad-norm clip 1.0, AdamW, EMA.  One "step" = one full
optimisation step (degrade -> shift -> U-Net fwd -> loss -> U-Net bwd -> [all-reduce] -> clip+AdamW+EMA)
on a batch that is already resident in HBM.  One JSON line on stdout (rank 0).

A plain run does only what the headline figure needs: set up, `--warmup` steps, `--steps` timed steps (`value`, `ms_per_step`),
one more step's outputs when `--dump-outputs DIR` is given (below), the line.  `--full` adds everything below (the spread
windows, the roofline replay, the CPU baseline child, the 1000-step sampler with its parity sample, the cfg3 / cfg4 / cfg5 legs);
the `--no-*` flags still take single legs out of a `--full` run, and the flags that ask for a measurement by name (`--windows K`,
`--config`, `--cut-graph`) run it in either mode.

`--dump-outputs DIR` (after the timed steps, before anything else runs) restores the seeded state the first step started from
(weights, AdamW moments and step count, EMA shadow and step count, device RNG offset), runs one more step of the timed path
through the same captured graph, and writes what that step computed, float32 unless said otherwise, rank 0: loss.npy (float64,
[1]), t.npy (the step's timesteps, [N]), shift.npy and x_in.npy (the shift and the U-Net input, NCHW), pred.npy (the U-Net
prediction, NCHW), params.npy and ema.npy (the weights and the EMA shadow after the update, in the reference's key order and
shapes, flattened and concatenated, sampled at DUMP_SAMPLE fixed positions drawn from a generator seeded with DUMP_SEED).  The inputs of that step (batch, state, RNG offset) depend on the arguments only, so runs and builds can be compared
file by file.  (The last timed step itself would not do: the bf16 step sums bias and GroupNorm-affine gradients with float atomics,
and over many steps AdamW carries their rounding into the weights.)

Extra objects in the `--full` line:
  roofline     the contraction kernel family (every `mdm_gemm` launch of the step -- `conv_halo_kernel` / `conv_lin2_kernel` /
               `wgrad_lin_kernel` / `gemm_ring_kernel`: conv fwd/dgrad/wgrad, 1x1 convs, attention products --
               and the batched split-K sum of the weight gradients): algorithmic FLOPs of those launches / their HIP-event
               time, against the dense bf16 MFMA peak;
  step_hbm     north_star's whole-step figure: algorithmic bytes (SURVEY 8(d) counting rule) /
               (step time x 8 TB/s);
  cpu_baseline the CPU oracle (own-words port of the reference trainer, oracle/) timed on this box's
               host cores on a bounded sample: 2 warm-up + median of 10 train steps, and a bounded sample of
               the reverse sampler (per-step time, scaled to 1000 steps x sample_num and said so) (rank 0, N=1 only);
  sampler      wall-clock of a 1000-step reverse sampling run (sample_num=100, history off; N=1 only), timed in
               fp32 AND bf16, each with `rel_l2_vs_oracle` measured on a bounded parity sample (same weights and
               host-replayed draws through the CPU oracle in the cpu_baseline child); the headline entry is the
               dtype that meets north_star's 1e-3.

`--config cfg3|cfg4|cfg5` adds `extras[<name>]` (the headline line stays cfg2): the 64x64 base-trainer step at 8 images per
GPU, the attention-everywhere 4-channel step at 16 images (L = 1024), the 250-step mean-shift sampler -- each with its step time
and contraction-family TFLOP/s.  `--cut-graph` adds `extras["cut_graph"]`: the SAME step in the form a data-parallel rank runs
it (front / bucket pieces / tail graphs instead of one graph, world = 1, no exchange), to price the cut on one GPU.

`--gpus N` without torchrun's environment starts the N ranks itself (child `python -m torch.distributed.run`,
before this process touches the GPU) and relays the JSON line; a line whose n_gpus != --gpus is never printed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "masked-diffusion-model_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA, MI355X_MICROARCH.md "Chip-level parameters"
PEAK_HBM_GBS = 8000.0          # HBM3E spec


_T0 = time.perf_counter()


def log(msg):
    """Progress line on stderr (keeps long runs visibly alive)."""
    print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def make_args(**kw):
    a = argparse.Namespace(
        dir_dataset="synthetic", data_size=32, in_channel=3, out_channel=3, batch_size=32,
        ddpm_num_steps=1000, updated_ddpm_num_steps=1000, ddpm_schedule="linear", ddpm_schedule_base=10.0,
        scheduler_num_scale_timesteps=1, select_degrade_pixel="thresholding", degrade_channel="1-channel",
        mean_option=0, mean_area="image-wise", shift_type="noise_with_perturbation", noise_mean=0.0,
        sample_latent_shape="zero", sampling="momentum", momentum_adaptive="base_momentum",
        sampling_mask_dependency="independent", sample_num=100, sample_history=False,
        loss_weight_use=False, loss_weight_power_base=10.0, use_ema=True, ema_inv_gamma=1.0, ema_power=0.75,
        ema_max_decay=0.9999, weight_dtype=torch.float32, save_images_epochs=10, mixed_precision="bf16",
        gradient_accumulation_steps=1, rng_mode="device", reference_quirks=True, use_graph=True, seed=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


PARITY_N, PARITY_T, PARITY_SEED, PARITY_FREE = 2, 1000, 4321, 100
# The sampler parity sample: PARITY_N images through ALL 1000 reverse steps of the schedule the timed run uses, host-replayed
# draws, bench architecture with non-degenerate weights.  Two figures per dtype, both against oracle/sampler_ref.py (fp32):
#   teacher-forced  every step starts from the oracle's x_t of that step (Sampler.step_hook); the worst and the median
#                   rel-L2 of x0_hat over the 1000 steps -- the per-step error of the kernels at every t of the schedule;
#   free-running    the LAST PARITY_FREE steps (t = 100 .. 1) as one contiguous run from the oracle's x_t at t = 100;
#                   rel-L2 of the final sample.  (An untrained U-Net iterated 1000 times is a chaotic map: the oracle's
#                   own fp32 run is O(1) away from its fp64 run by then -- tests/test_device_path_gpu.py records it --
#                   so a free run over the whole schedule would measure conditioning, not the kernels.)


def parity_params(shapes, seed=77):
    """Non-degenerate weights for the sampler parity sample (the fresh-init model predicts ~0: its last conv is
    the reference's 1e-5 'zero' init, SURVEY D13 -- useless for an error measurement).  Keys are visited in
    sorted order so the GPU parent and the CPU child draw the same tensors from the same generator."""
    import math
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if len(shp) == 1:
            out[k] = 1.0 + 0.1 * torch.randn(shp, generator=g) if k.endswith("weight") else 0.05 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            out[k] = torch.randn(shp, generator=g) / math.sqrt(fan_in)
    return out


def _seed_host(s):
    import random

    import numpy as np
    torch.manual_seed(s); np.random.seed(s); random.seed(s)      # main_train_masked.py:441-445


def parity_args():
    return make_args(rng_mode="replay", sample_num=PARITY_N, sample_latent_shape="uniform", sample_history="device")


def cpu_baseline(n_steps=10, n_warm=2, parity_out=None):
    """CPU child: time the oracle's train step (and its reverse sampler) on the same workload shape (fp32, the box's host
    cores); leave the oracle's 1000-step sampler trajectory in `parity_out` for the GPU parent to check itself against."""
    import statistics

    import numpy as np
    from oracle.sampler_ref import HISTORY_NAMES, SamplerRef
    from oracle.scheduler_ref import SchedulerRef
    from oracle.trainer_ref import train_step_ref
    from oracle.unet_ref import UNetRef, param_shapes, unet6_config
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    cores = min(cores, 16)           # the GPU box gives one GPU a 16-core share
    torch.set_num_threads(cores)
    a = make_args(rng_mode="replay")
    torch.manual_seed(0)
    cfg = unet6_config(32)
    model = UNetRef(cfg, seed=0)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    ema = [p.detach().clone() for p in model.parameters()]
    s = SchedulerRef(a)
    s.update_ddpm_num_steps(1000)
    used = s.get_timesteps_epoch(0, 1)
    x0 = torch.rand(32, 3, 32, 32) * 2 - 1
    log(f"cpu baseline: oracle model built, {cores} threads")
    for k in range(n_warm):
        train_step_ref(model, opt, s, a, x0, used, s.rng, ema_params=ema, ema_step=k)
    log(f"cpu baseline: {n_warm} warm-up steps done")
    times = []
    for k in range(n_steps):
        t0 = time.perf_counter()
        train_step_ref(model, opt, s, a, x0, used, s.rng, ema_params=ema, ema_step=n_warm + k)
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    log(f"cpu baseline: {n_steps} timed steps, median {med:.3f}s (min {min(times):.3f}, max {max(times):.3f})")
    out = {"value": round(32 / med, 3), "unit": "images/s", "cores": cores, "kind": "port",
           "sample": f"median of {n_steps} optimisation steps of 32x3x32x32 after {n_warm} warm-up steps "
                     f"(oracle/trainer_ref.py, fp32); step times min/median/max {min(times):.3f}/{med:.3f}/{max(times):.3f} s"}
    # ---- the reverse sampler on the CPU: PARITY_N images through the whole 1000-step schedule (also the parity trajectory)
    pa = parity_args()
    ps = SchedulerRef(pa)
    ps.update_ddpm_num_steps(1000)
    ts = ps.get_timesteps_epoch(0, 1)
    pm = UNetRef(cfg, parity_params(param_shapes(cfg)))
    _seed_host(PARITY_SEED)
    t0 = time.perf_counter()
    want, hist = SamplerRef(None, pa, ps, [None] * 3).sample(pm, ts)
    sec = time.perf_counter() - t0
    per_img_step = sec / (len(ts) * PARITY_N)
    out["sampler"] = {"seconds_per_reverse_step_per_image": round(per_img_step, 5), "cores": cores,
                      "estimate_1000_steps_x100_seconds": round(per_img_step * 1000 * 100, 1),
                      "sample": f"{len(ts)} reverse steps x {PARITY_N} images timed ({sec:.2f} s, oracle/sampler_ref.py fp32, history on); "
                                "the 1000-step x sample_num=100 figure is that per-step-per-image time x 1e5 (an estimate, not a run)"}
    log(f"cpu baseline: sampler {len(ts)} steps x {PARITY_N} images {sec:.2f}s")
    if parity_out:
        h = dict(zip(HISTORY_NAMES, hist))
        np.savez(parity_out, sample_t=h["sample_t"].numpy(), sample_0=h["sample_0"].numpy(), x0=want.numpy())
    return out


SAMPLER_MODES = {
    "f32": "fp32 storage, exact fp32 products (v_mfma_f32_16x16x4_f32), fp32 accumulation",
    "f32_split": "fp32 storage and accumulation; forward convolutions multiply every operand as bf16(x) + bf16(x - bf16(x)): hi*hi + hi*lo + lo*hi "
                 "on v_mfma_f32_16x16x32_bf16 (<= 2^-16 per product); GroupNorm, attention, time embedding, scheduler kernels exact fp32",
    "bf16": "bf16 storage, bf16 products, fp32 accumulation",
}


def sampler_parity(mdm, cfg, sdt, dev, pparams, ref, products="exact"):
    """-> dict of the two parity figures (see PARITY_*) for one dtype; `ref` = the oracle child's trajectory (numpy)."""
    pa = parity_args()
    net = mdm.UNet(cfg, N=PARITY_N, H=32, W=32, dtype=sdt, params=pparams, use_graph=False, f32_products=products).eval()
    sch = mdm.Scheduler(pa, device=dev)
    sch.update_ddpm_num_steps(PARITY_T)
    ts = sch.get_timesteps_epoch(0, 1)
    ref_xt = torch.from_numpy(ref["sample_t"]).to(dev)
    ref_x0h = torch.from_numpy(ref["sample_0"]).to(dev).double()
    smp = mdm.Sampler(None, pa, sch, [None] * 3)
    smp.step_hook = lambda i, slot, x_t: x_t.copy_(ref_xt[slot])
    _seed_host(PARITY_SEED)
    _, hist = smp.sample(net, ts)
    got = hist[mdm.sampler.HISTORY_NAMES.index("sample_0")].double()
    e = ((got[1:] - ref_x0h[1:]).flatten(1).norm(dim=1) / ref_x0h[1:].flatten(1).norm(dim=1))
    out = {"teacher_forced_steps": PARITY_T, "teacher_forced_worst": float(e.max()), "teacher_forced_median": float(e.median())}
    # free-running over the last PARITY_FREE steps: the host RNG must stand where the oracle's stood at that step, so the
    # loop is run from the top with the hook forcing x_t up to the hand-over step and leaving it alone afterwards
    pa2 = parity_args()
    pa2.sample_history = False
    smp2 = mdm.Sampler(None, pa2, sch, [None] * 3)
    smp2.step_hook = lambda i, slot, x_t: x_t.copy_(ref_xt[slot]) if i >= PARITY_FREE - 1 else None
    _seed_host(PARITY_SEED)
    x0, _ = smp2.sample(net, ts)
    w = torch.from_numpy(ref["x0"]).to(dev).double()
    out["free_running_last_steps"] = PARITY_FREE
    out["free_running_rel_l2"] = float((x0.double() - w).norm() / w.norm())
    del net
    return out


def time_steps(step, used, warmup, steps):
    for _ in range(warmup):
        step.run_device(None, used)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.run_device(None, used)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


DUMP_SAMPLE, DUMP_SEED = 1 << 22, 2024      # 2 x 16 MB of sampled weights; the rest of a dump is < 2 MB at the default batch


class StepState:
    """Everything one step reads and writes besides the batch: fp32 weights, AdamW moments and step count, EMA shadow and step
    count, the device Philox offset.  `restore()` copies a snapshot back IN PLACE (the captured graph holds these buffers)."""

    def __init__(self, model, optim, ema, sched):
        self.model, self.optim, self.ema, self.rng = model, optim, ema, sched.dev_rng.dev
        torch.cuda.synchronize()
        self.bufs = [(t, t.clone()) for t in (model.store.P, optim.m, optim.v, self.rng) + ((ema.shadow,) if ema is not None else ())]
        self.t, self.ema_step = optim.t, (ema.optimization_step if ema is not None else None)

    def restore(self):
        torch.cuda.synchronize()
        for live, saved in self.bufs:
            live.copy_(saved)
        self.optim.t = self.t
        if self.ema is not None:
            self.ema.optimization_step = self.ema_step
        self.model.store.sync_shadow()          # bf16 / transposed / split shadows follow the restored fp32 weights
        torch.cuda.synchronize()


def dump_outputs(out_dir, step, model, ema, loss):
    """The dumped step's outputs as DIR/<name>.npy (see the module docstring).  Synchronises; nothing here is timed."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    nchw = lambda a: a.data.float().cpu()[..., :model.cout].permute(0, 3, 1, 2).contiguous()
    arrays = {"loss": np.array([loss], dtype=np.float64), "t": model.t_in.float().cpu(),
              "shift": step.s.cpu(), "x_in": step.x_in.cpu(), "pred": nchw(model.y_out)}
    order = model.reference_param_order()
    g = torch.Generator().manual_seed(DUMP_SEED)
    idx = None
    for name, src in [("params", None)] + ([("ema", ema.shadow)] if ema is not None else []):
        flat = torch.cat([v.reshape(-1) for v in model.store.state_dict(order=order, src=src).values()])
        if idx is None:
            idx = torch.randint(flat.numel(), (min(DUMP_SAMPLE, flat.numel()),), generator=g).sort().values
        arrays[name] = flat[idx]
    for name, a in arrays.items():
        a = a.numpy() if isinstance(a, torch.Tensor) else a
        np.save(os.path.join(out_dir, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))
    return sorted(arrays)


def family_roofline(_lib, step, model, optim, ema, dt, reps=3):
    """HIP events around every contraction launch of the step (see `roofline` in the module docstring) ->
    (TFLOP/s, ms per step in the family, launches per step, event-pair cost in ms)."""
    st = torch.cuda.current_stream().cuda_stream
    with _lib.Recording() as front:
        step._emit_device_front()
    pick = lambda rec: (lambda i, name: (name in ("mdm_gemm", "mdm_gemm_pair") and rec.flops.get(i, (0, -1))[1] == dt) or
                        name == "mdm_wgrad_group_launch")
    tot_ms, tot_fl, n_launch = 0.0, 0.0, 0
    step._hyper()
    front.run(st)
    pair_ms = front.event_overhead(st, pick(front))
    for _ in range(reps):
        step._hyper()
        for rec in (front, model.backward_plan):
            for i, ms in rec.run_timed(st, pick(rec), pair_ms):
                tot_ms += ms
                if i in rec.flops:
                    tot_fl += rec.flops[i][0]
                    n_launch += 1
        optim.emit_update(ema.shadow if ema is not None else None, 1.0, 1.0)
    torch.cuda.synchronize()
    return tot_fl / (tot_ms * 1e-3) / 1e12, tot_ms / reps, n_launch // reps, pair_ms, tot_fl / reps


def bench_cut_graph(mdm, TrainStep, model, sched, args, optim, ema, used, opt_, whole_ms):
    """The step as a data-parallel rank runs it -- front graph, one graph per gradient bucket, tail graph, the bucket hooks
    firing with world = 1 -- next to the one-graph form, same model, same box, back to back."""
    a2 = argparse.Namespace(**vars(args))
    a2.cut_step_graph = True
    # a rank of a data-parallel job groups its weight gradients in ~32 MB buckets (UNet's default once torch.distributed is up):
    # the same weights and optimizer, a second launch plan
    model = mdm.UNet(model.cfg, N=model.N, H=model.H, W=model.W, dtype=model.dt, store=model.store, wgrad_group_bytes=32 << 20)
    cut = TrainStep(model, sched, a2, optim, ema, mean_shift=True, comm=None)
    cut.x0.copy_(torch.rand(model.N, 3, model.H, model.W) * 2 - 1)
    ms = time_steps(cut, used, opt_.warmup, opt_.steps)
    pieces = len(cut._graphs[2]) + (1 if cut._graphs[3] is not None else 0)
    log(f"cut-graph form: {ms:.4f} ms/step in {pieces} backward pieces (+ front + tail) vs {whole_ms:.4f} whole")
    return {"ms_per_step": round(ms, 4), "whole_graph_ms_per_step": round(whole_ms, 4), "ratio": round(ms / whole_ms, 4),
            "graphs_per_step": pieces + 2, "note": "front / bucket pieces / tail hipGraphs over 32 MB weight-gradient groups, bucket hooks with world = 1 (no exchange); the one-graph form runs one group"}


def bench_config(mdm, _lib, TrainStep, name, dev, opt_, full=True):
    """One of BASELINE.json's other configurations on this GPU: step time, family TFLOP/s; cfg5: the 250-step sampler."""
    from mdm.unet import unet6_config
    dt = mdm.BF16
    if name == "cfg3":          # 64x3x64x64, base trainer (trainer_masked.py), 8 images per GPU (global 64 over DP=8)
        N, H, cfg, mean_shift, flops_img = 8, 64, unet6_config(64), False, 140.19e9
        a = make_args(batch_size=N, data_size=64, shift_type="non_shift", seed=77)
        what = "BASELINE.json configs[2]: 64x3x64x64, unet6 preset, base trainer (non_shift), 8 images per GPU"
    elif name == "cfg4":        # 16x4x32x32, attention at every level (models_Unet.py:146 alternative): L = 1024 .. 16
        N, H, mean_shift, flops_img = 16, 32, False, 48.10e9
        cfg = dict(in_channels=4, hid_channels=128, out_channels=4, ch_multipliers=[1, 2, 2, 2], num_res_blocks=2, apply_attn=[True] * 4)
        a = make_args(batch_size=N, data_size=32, in_channel=4, out_channel=4, shift_type="non_shift", seed=78)
        what = "BASELINE.json configs[3]: 16x4x32x32, unet6 with attention at all four levels (L = 1024, 256, 64, 16), base trainer"
    else:                       # cfg5: mean-shift trainer + 250-step reverse sampler, sample_num 100
        N, H, cfg, mean_shift, flops_img = 32, 32, unet6_config(32), True, 34.87e9
        a = make_args(batch_size=N, ddpm_num_steps=250, seed=79)
        what = "BASELINE.json configs[4]: mean-shift trainer (32x3x32x32) + 250-step reverse sampler, sample_num 100, bf16"
    C = cfg["in_channels"]
    model = mdm.UNet(cfg, N=N, H=H, W=H, dtype=dt, seed=0)
    optim = mdm.AdamW(model, lr=1e-4)
    ema = mdm.EMA(model)
    sched = mdm.Scheduler(a, device=dev)
    sched.update_ddpm_num_steps(a.ddpm_num_steps)
    used = sched.get_timesteps_epoch(0, 1)
    step = TrainStep(model, sched, a, optim, ema, mean_shift=mean_shift)
    step.x0.copy_(torch.rand(N, C, H, H) * 2 - 1)
    ms = time_steps(step, used, opt_.warmup, opt_.steps)
    tf, fam_ms, n_launch, pair_ms, fl = family_roofline(_lib, step, model, optim, ema, dt)
    out = {"workload": what, "ms_per_step": round(ms, 4), "images_per_s": round(N / (ms * 1e-3), 1), "per_gpu_batch": N,
           "params": model.num_parameters(), "tflops_step": round(flops_img * N / (ms * 1e-3) / 1e12, 1),
           "family": {"achieved_TFLOPs": round(tf, 1), "frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4), "kernel_ms_per_step": round(fam_ms, 3),
                      "launches_per_step": n_launch, "flops_per_step": fl, "event_pair_us": round(1e3 * pair_ms, 2)},
           "launches": {"forward": len(model.forward_plan.calls), "backward": len(model.backward_plan.calls)}}
    log(f"{name}: {ms:.3f} ms/step, family {tf:.0f} TFLOP/s")
    if name == "cfg5":
        a.sample_num = 100
        # "f32_split" = the sampler of record (fp32 storage, convolution products as bf16 hi / lo pairs): the model's own sampling plan
        for tag in (("bf16", "f32_split", "f32") if full else ("bf16", "f32_split")):
            net = (model.with_batch(100) if tag == "bf16" else model.sampling_plan(100, tag)).eval()
            smp = mdm.Sampler(None, a, sched, [None] * 3)
            smp.sample(net, used[:3])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            x0, _ = smp.sample(net, used)
            torch.cuda.synchronize()
            out[f"sampler_{tag}"] = {"steps": len(used), "sample_num": 100, "seconds": round(time.perf_counter() - t1, 3),
                                     "finite": bool(torch.isfinite(x0).all())}
            del net
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sampler", action="store_true")
    ap.add_argument("--sampler-steps", type=int, default=1000)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-roofline", action="store_true", help="skip the event-timed replay (kernel-count profiles: every profiled launch then belongs to a whole step)")
    ap.add_argument("--wgrad-group-mb", type=float, default=None,
                    help="size of a weight-gradient group = launch = gradient bucket unit (default: one group on one GPU, 32 MB under data parallelism)")
    ap.add_argument("--bucket-mb", type=float, default=None, help="gradient bucket size of the all-reduce (N > 1; default 32)")
    ap.add_argument("--reserve-cus", type=int, default=0,
                    help="N > 1: build the persistent weight-gradient launch for CUs - R workgroups so that RCCL's kernels find free CUs beside it")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline figure: windows, roofline, CPU baseline, sampler, cfg3 / cfg4 / cfg5")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, run one step of the timed path from the seeded initial state and write its outputs as DIR/<name>.npy")
    ap.add_argument("--windows", type=int, default=None,
                    help="further timed windows of --steps steps behind the headline one (spread: min / median / max; default 4 with --full, else 0)")
    ap.add_argument("--no-extras", action="store_true", help="skip the cfg3 / cfg4 / cfg5 legs of the --full run")
    ap.add_argument("--config", action="append", default=[], choices=["cfg3", "cfg4", "cfg5"],
                    help="also measure this BASELINE.json configuration (reported under `extras`; the headline stays cfg2)")
    ap.add_argument("--cut-graph", action="store_true", help="also time the data-parallel (cut) form of the step graph on this one GPU")
    ap.add_argument("--no-pair", action="store_true", help=argparse.SUPPRESS)                  # experiments only: every convolution its own launch
    ap.add_argument("--grad-wire", default="f32", choices=["f32", "bf16"], help="dtype of the gradient all-reduce payload (N > 1)")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parity-out", default=None, help=argparse.SUPPRESS)
    opt_ = ap.parse_args()
    if opt_.steps < 1 or opt_.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if opt_.windows is None:
        opt_.windows = 4 if opt_.full else 0
    if opt_.cpu_baseline_only:           # child process of the cpu_baseline leg: CPU only, never touches the GPU
        print(json.dumps(cpu_baseline(parity_out=opt_.parity_out)))
        return
    if "WORLD_SIZE" not in os.environ and opt_.gpus > 1:
        # `python bench.py --gpus N`: start the N ranks ourselves, one per GPU, BEFORE anything here touches the GPU
        # (a process that has initialised HIP must not be replaced or forked into ranks), and relay their output.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={opt_.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)

    import mdm
    from mdm import _lib
    from mdm.dist import GradComm, init_from_env
    from mdm.train_step import TrainStep

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != opt_.gpus:
        raise SystemExit(f"bench.py: --gpus {opt_.gpus} but WORLD_SIZE={world}: refusing to print a line for another job size")
    if not torch.cuda.is_available():
        raise RuntimeError("bench.py needs a GPU: the product path has no CPU fallback")
    # (MDM_FORCE_DEVICE / MDM_DIST_BACKEND exist so the multi-rank path can be rehearsed on a 1-GPU box: two
    # ranks on cuda:0 over gloo.  The driver's runs use one rank per GPU over "nccl" = RCCL.)
    if os.environ.get("MDM_FORCE_DEVICE") is not None:
        local = int(os.environ["MDM_FORCE_DEVICE"])
    torch.cuda.set_device(local)
    rehearse = world == 1 and os.environ.get("MDM_REHEARSE_COMM") == "1"      # one rank, RCCL collectives issued anyway (one-GPU box)
    if world > 1 or rehearse:
        init_from_env(os.environ.get("MDM_DIST_BACKEND", "nccl"), single=rehearse)
    dev = torch.device("cuda", local)
    dt = mdm.BF16 if opt_.dtype == "bf16" else mdm.F32
    N = opt_.batch
    args = make_args(batch_size=N, seed=1234 + rank, use_graph=not opt_.no_graph)   # per-rank RNG streams

    cfg = mdm.unet6_config(32)
    xk = {}
    if opt_.reserve_cus > 0:
        os.environ["MDM_WGRAD_RESERVE_CUS"] = str(opt_.reserve_cus)       # read by mdm_wgrad_group_create
    if opt_.wgrad_group_mb is not None:
        xk["wgrad_group_bytes"] = int(opt_.wgrad_group_mb * (1 << 20))
    if opt_.no_pair:
        xk["pair_convs"] = False
    model = mdm.UNet(cfg, N=N, H=32, W=32, dtype=dt, seed=0, use_graph=not opt_.no_graph, **xk)   # same weights on every rank
    optim = mdm.AdamW(model, lr=1e-4)
    ema = mdm.EMA(model, decay=args.ema_max_decay, inv_gamma=args.ema_inv_gamma, power=args.ema_power)
    sched = mdm.Scheduler(args, device=dev)
    sched.update_ddpm_num_steps(1000)
    used = sched.get_timesteps_epoch(0, 1)
    ck = {} if opt_.bucket_mb is None else {"bucket_bytes": int(opt_.bucket_mb * (1 << 20))}
    comm = GradComm(wire=opt_.grad_wire, always_exchange=rehearse, **ck) if (world > 1 or rehearse) else None
    step = TrainStep(model, sched, args, optim, ema, mean_shift=True, comm=comm)
    step.time_comm = comm is not None
    g = torch.Generator().manual_seed(100 + rank)
    step.x0.copy_(torch.rand(N, 3, 32, 32, generator=g) * 2 - 1)          # synthetic batch, resident in HBM

    log(f"model built: {model.num_parameters()} params, {len(model.forward_plan.calls)} fwd / {len(model.backward_plan.calls)} bwd launches")
    # --dump-outputs: the seeded state before the first step, so that the dumped step starts from the same inputs on every run (the
    # bf16 step sums some gradients with float atomics: over many steps AdamW carries their rounding into the weights)
    initial = StepState(model, optim, ema, sched) if opt_.dump_outputs else None

    def barrier():
        if world > 1 or rehearse:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for i in range(opt_.warmup):
        step.run_device(None, used)
        if i == 0:
            torch.cuda.synchronize()
            log("first step done (graphs captured)")
    barrier()
    step.comm_events = []            # the exposed-wait samples of the warm-up steps do not count
    log("warm-up done")
    t0 = time.perf_counter()
    for _ in range(opt_.steps):
        step.run_device(None, used)
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1 or rehearse:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tt)
    loss = float(step.loss)
    log(f"timed region: {elapsed:.3f}s for {opt_.steps} steps, loss {loss:.5f}")
    ms_per_step = 1e3 * elapsed / opt_.steps
    value = N * world * opt_.steps / elapsed
    comm_rep = step.comm_report() if comm is not None else None          # exposed wait of the headline region's steps
    if initial is not None:
        # one more step of the timed path (same captured graph, every rank), from the restored seeded state
        initial.restore()
        barrier()
        step.run_device(None, used)
        barrier()
        if rank == 0:
            dumped = dump_outputs(opt_.dump_outputs, step, model, ema, float(step.loss))
            log(f"outputs of one step of the timed path from the seeded state written to {opt_.dump_outputs}: {', '.join(dumped)}")
    # ---- spread: the same K steps again, `--windows` times, each bracketed like the headline region (which stays the `value`)
    wins = [ms_per_step]
    for _ in range(max(0, opt_.windows)):
        barrier()
        t1 = time.perf_counter()
        for _ in range(opt_.steps):
            step.run_device(None, used)
        barrier()
        el = time.perf_counter() - t1
        if world > 1 or rehearse:
            tt = torch.tensor([el], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
            el = float(tt)
        wins.append(1e3 * el / opt_.steps)
    step.comm_events = []
    ws = sorted(wins)
    windows = {"n": len(wins), "steps_each": opt_.steps, "ms_per_step_min": round(ws[0], 4), "ms_per_step_median": round(ws[len(ws) // 2], 4),
               "ms_per_step_max": round(ws[-1], 4), "note": "window 0 is the headline region (`value`, `ms_per_step`)"}
    log(f"windows: {[round(w, 4) for w in wins]}")

    # ---- roofline of the contraction kernel family: HIP events around every launch, on the launch stream
    roofline = None
    step_hbm = None
    if rank == 0 and opt_.full and not opt_.no_roofline:
        st = torch.cuda.current_stream().cuda_stream
        with _lib.Recording() as front:
            step._emit_device_front()
        # the family = every bf16 mdm_gemm / mdm_gemm_pair call plus the grouped weight-gradient launches (incl. their split-K sums)
        pick = lambda rec: (lambda i, name: (name in ("mdm_gemm", "mdm_gemm_pair") and rec.flops.get(i, (0, -1))[1] == dt) or
                            name == "mdm_wgrad_group_launch")
        tot_ms, tot_fl, n_launch = 0.0, 0.0, 0
        reps = 3
        # an event pair is not free: measured on the forward contractions as 2 T(one launch) - T(two launches)
        step._hyper()
        front.run(st)
        pair_ms = front.event_overhead(st, pick(front))
        for _ in range(reps):
            step._hyper()
            for rec in (front, model.backward_plan):
                for i, ms in rec.run_timed(st, pick(rec), pair_ms):
                    tot_ms += ms
                    if i in rec.flops:
                        tot_fl += rec.flops[i][0]
                        n_launch += 1
            optim.emit_update(ema.shadow, 1.0, 1.0 / world)
        torch.cuda.synchronize()
        log("event-timed replay done")
        ach = tot_fl / (tot_ms * 1e-3) / 1e12
        name = ("mdm_gemm bf16 family: conv_halo / conv_lin2 / wgrad_lin / gemm_ring kernels (+ split-K epilogue and batched reduce)" if dt == mdm.BF16
                else "gemm_f32_kernel")
        peak = PEAK_BF16_TFLOPS if dt == mdm.BF16 else 157.3
        # HBM bytes per launch of this kernel family from PMC counters: collected out of band by
        # scripts/pmc_traffic.sh (rocprofv3 cannot run inside the timed process) and committed under profiles/
        traffic = mfma_busy = pmc_src = None
        pmc_head = mfma_cal = None
        for fn in ("r04_pmc.json", "r03_pmc.json", "r02_pmc.json", "r01_pmc_traffic.json"):
            try:
                with open(os.path.join(ROOT, "profiles", fn)) as fh:
                    pj = json.load(fh)
                traffic, mfma_busy, pmc_src = round(pj["hbm_bytes_per_launch"]), pj.get("mfma_busy"), "profiles/" + fn
                pmc_head, mfma_cal = pj.get("git_head"), pj.get("mfma_busy_calibration")
                break
            except Exception:
                pass
        roofline = {"bound": "mfma", "kernel": name, "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(ach / peak, 4), "traffic": traffic, "mfma_busy": mfma_busy, "pmc_source": pmc_src,
                    "pmc_head": pmc_head, "mfma_busy_calibration": mfma_cal,
                    "launches_per_step": n_launch // reps, "flops_per_step": tot_fl / reps,
                    "avg_launch_us": round(1e3 * tot_ms / n_launch, 2), "kernel_ms_per_step": round(tot_ms / reps, 3),
                    "event_pair_us": round(1e3 * pair_ms, 2)}
        P = model.num_parameters()
        # 38 B/param (+8 EMA) + 5 passes x 2 B x A_out.  A_out is FROZEN in BASELINE.md at SURVEY's probed
        # figure (386.8 M leaf-op output elements at cfg2, N=32: what `frac` uses, scaled with N); the builder's own
        # census (residual / time-embedding adds, concats, upsample and SamePad copies counted as leaf outputs too) is
        # reported next to it.
        a_survey = int(386.8e6 * N / 32)
        a_census = model.census()
        b_survey, b_census = (38 + 8) * P + 10 * a_survey, (38 + 8) * P + 10 * a_census
        gbs = lambda b: b / (ms_per_step * 1e-3) / 1e9
        step_hbm = {"algorithmic_bytes": b_survey, "a_out": a_survey, "params": P,
                    "achieved_GBs": round(gbs(b_survey), 1), "peak_GBs": PEAK_HBM_GBS, "frac": round(gbs(b_survey) / PEAK_HBM_GBS, 4),
                    "census": {"a_out": a_census, "algorithmic_bytes": b_census, "frac": round(gbs(b_census) / PEAK_HBM_GBS, 4)},
                    "flops_per_step": 34.87e9 * N, "tflops": round(34.87e9 * N / (ms_per_step * 1e-3) / 1e12, 1)}

    # ---- CPU baseline leg first (bounded child process, own thread pool, no GPU context): it also leaves the oracle's
    # 1000-step sampler trajectory behind, which the sampler parity sample below is checked against
    cpu = None
    parity_file = None
    ref = None
    if rank == 0 and world == 1 and opt_.full and not opt_.no_cpu_baseline:
        import subprocess
        import tempfile

        import numpy as np
        try:
            env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
            cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only"]
            if not opt_.no_sampler:
                fd, parity_file = tempfile.mkstemp(suffix=".npz", prefix="mdm_parity_")
                os.close(fd)
                cmd += ["--parity-out", parity_file]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            sys.stderr.write(r.stderr)
            cpu = json.loads(r.stdout.strip().splitlines()[-1])
            if parity_file:
                ref = dict(np.load(parity_file))
        except Exception as e:          # never let the baseline leg take the bench line down
            cpu = {"value": None, "unit": "images/s", "cores": None, "kind": "port", "sample": f"failed: {type(e).__name__}: {e}"[:200]}
        finally:
            if parity_file:
                try:
                    os.unlink(parity_file)
                except OSError:
                    pass

    # ---- 1k-step sampler wall-clock (single GPU: samples are independent, no collective; N>1 shards sample_num)
    sampler = None
    if rank == 0 and world == 1 and opt_.full and not opt_.no_sampler:
        sampler = {}
        pparams = parity_params(model.reference_shapes())
        # "f32_split": fp32 storage and accumulation, the 3x3 convolutions' products on the bf16 matrix pipe as hi / lo pairs
        # (hi*hi + hi*lo + lo*hi, ~2^-16 per product: mdm_gemm_desc.B_split) -- measured against the oracle like the other two
        for tag, sdt, products in (("f32", mdm.F32, "exact"), ("f32_split", mdm.F32, "split"), ("bf16", mdm.BF16, "exact")):
            if sdt == dt:
                net = model.with_batch(args.sample_num).eval()
            else:
                net = mdm.UNet(cfg, N=args.sample_num, H=32, W=32, dtype=sdt, seed=0, use_graph=not opt_.no_graph,
                               f32_products=products).eval()
            smp = mdm.Sampler(None, args, sched, [None] * 3)
            smp.sample(net, used[:3])                            # warm-up / graph capture
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            x0_hat, _ = smp.sample(net, used[:opt_.sampler_steps])
            torch.cuda.synchronize()
            sec = time.perf_counter() - t1
            nst = min(opt_.sampler_steps, len(used))
            log(f"sampler {tag}: {sec:.2f}s")
            sampler[tag] = {"dtype": tag, "arithmetic": SAMPLER_MODES[tag], "steps": nst, "sample_num": args.sample_num, "seconds": round(sec, 3),
                            "ms_per_step": round(1e3 * sec / nst, 3), "finite": bool(torch.isfinite(x0_hat).all())}
            # roofline of the reverse step: algorithmic FLOPs of ONE U-Net forward at sample_num images (the launch list's own
            # bookkeeping: 2 N OH OW Cout Cin taps per convolution, 2 M N K per contraction) over the measured wall clock per step.
            # Ceilings: dense bf16 MFMA 2 500 TFLOP/s; split products issue three bf16 MFMAs per product -> 833; exact fp32 MFMA 157.3
            fl_step = float(sum(f for f, _ in net.forward_plan.flops.values()))
            ceil = {"f32": 157.3, "f32_split": PEAK_BF16_TFLOPS / 3.0, "bf16": PEAK_BF16_TFLOPS}[tag]
            tfs = fl_step * nst / sec / 1e12
            rf = {"bound": "mfma", "flops_per_step": fl_step, "achieved": round(tfs, 1), "unit": "TFLOP/s", "peak": round(ceil, 1),
                  "frac": round(tfs / ceil, 4), "frac_of_bf16_peak": round(tfs / PEAK_BF16_TFLOPS, 4),
                  "launches_per_step": len(net.forward_plan.calls)}
            try:        # the dominant kernel of this mode from the committed kernel trace (scripts/prof_sampler_mode.sh)
                with open(os.path.join(ROOT, "profiles", "r04_sampler_roofline.json")) as fh:
                    dk = json.load(fh).get(tag)
                if dk:
                    rf["dominant_kernel"] = dk
            except Exception:
                pass
            sampler[tag]["roofline"] = rf
            del net
            par = None
            if ref is not None:
                try:
                    par = sampler_parity(mdm, cfg, sdt, dev, pparams, ref, products)
                    log(f"sampler parity {tag}: {par}")
                except Exception as e:      # noqa: BLE001
                    par = {"error": f"{type(e).__name__}: {e}"[:200]}
            sampler[tag]["parity"] = par
            # the figure the 1e-3 claim is made on: the contiguous free run over the last PARITY_FREE steps of the schedule,
            # and nothing worse than that at any single step of the 1000
            sampler[tag]["rel_l2_vs_oracle"] = None if not par or "error" in par else max(par["free_running_rel_l2"], par["teacher_forced_worst"])
            sampler[tag]["parity_sample"] = (f"{PARITY_N} images, bench architecture with non-degenerate random weights, host-replayed draws, vs "
                                             f"oracle/sampler_ref.py fp32: max of (a) the worst per-step rel-L2 of x0_hat over all {PARITY_T} reverse "
                                             f"steps, each started from the oracle's x_t (teacher forcing), and (b) the rel-L2 of the final sample of "
                                             f"a contiguous free run over the last {PARITY_FREE} steps")
        ok = [t for t in sampler if sampler[t]["rel_l2_vs_oracle"] is not None and sampler[t]["rel_l2_vs_oracle"] < 1e-3]
        head = min(ok, key=lambda t: sampler[t]["seconds"]) if ok else "f32"
        sampler = {**sampler[head], "meets_1e-3": bool(ok), "by_dtype": sampler}

    # ---- extras: the cut (data-parallel) form of the step on this one GPU; the other BASELINE configurations
    extras = {}
    if rank == 0 and world == 1 and opt_.cut_graph:
        extras["cut_graph"] = bench_cut_graph(mdm, TrainStep, model, sched, args, optim, ema, used, opt_, ms_per_step)
    if rank == 0 and world == 1:
        # the other BASELINE configurations ride in the --full line (a few seconds each);
        # `--config` asks for one explicitly (cfg5 then also runs the exact-fp32 250-step sampler), `--no-extras` skips them
        names = list(opt_.config) if opt_.config else ([] if (not opt_.full or opt_.no_extras or opt_.no_sampler) else ["cfg3", "cfg4", "cfg5"])
        for name in names:
            log(f"extra configuration {name}")
            try:
                extras[name] = bench_config(mdm, _lib, TrainStep, name, dev, opt_, full=bool(opt_.config))
            except Exception as e:      # noqa: BLE001 -- an extra must never take the headline line down
                extras[name] = {"error": f"{type(e).__name__}: {e}"[:300]}

    if rank == 0:
        out = {
            "metric": "train images/sec at 32x3x32x32 (masked-diffusion step: degrade+shift+unet6 fwd/bwd+clip+AdamW+EMA)",
            "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": opt_.steps, "warmup": opt_.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": opt_.dtype, "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[1]: 32x3x32x32 per GPU, unet6 Model('unet6',3,32,32,3) 35.75M params "
                                   "random init, T=1000 linear/thresholding/1-channel, shift noise_with_perturbation, "
                                   "AdamW lr 1e-4 + clip 1.0 + EMA, device Philox RNG, hipGraph replay",
                       "global_batch": N * world, "per_gpu_batch": N, "image": "3x32x32",
                       "parallelism": f"dp{world}", "final_loss": round(loss, 5)},
            "roofline": roofline, "step_hbm": step_hbm, "cpu_baseline": cpu, "sampler": sampler, "windows": windows,
        }
        if comm_rep is not None:
            out["comm"] = comm_rep
        if extras:
            out["extras"] = extras
        print(json.dumps(out))
    if world > 1 or rehearse:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
