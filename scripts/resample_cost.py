"""What resample_with_conv=False costs (or saves) at cfg2 (unet6 at 32x32, N = 32, bf16, mean-shift trainer, device RNG, one hipGraph
per step): `TrainStep.run_device` of the default preset and of the pooled preset (average-pool downsampling, bare nearest upsampling:
six convolution layers fewer, twelve streaming passes more) on ONE box, in interleaved windows (conv, pool, conv, pool, ...; each
window = --steps back-to-back graph replays between two synchronisations, after --warmup steps per model; the figure of a run is the
median of its windows, every window is reported).  Then both recorded plans once more EAGERLY with a HIP event pair around every
launch (event overhead taken off, `_lib.Recording.run_timed`), summed per entry point, so that a difference can be read off as
"which launches grew": the lost conv -> GroupNorm epilogue fusions at the seams show as more / longer mdm_groupnorm_* launches.

Prints ONE JSON line.
    python scripts/resample_cost.py [--steps 20] [--warmup 5] [--windows 5] [--once]

--once: build the pooled model only and run --steps graph replays (the run a kernel trace is taken of: the achieved GB/s of
avgpool2_kernel / upsample2_kernel / sumpool2_kernel follow from its per-kernel times and the byte counts printed as `resample_bytes`).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "masked-diffusion-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench import make_args  # noqa: E402


def build(mdm, TrainStep, with_conv, N):
    dev = torch.device("cuda", torch.cuda.current_device())
    args = make_args(batch_size=N, seed=1234, mixed_precision="bf16")
    model = mdm.UNet(mdm.unet6_config(32, resample_with_conv=with_conv), N=N, H=32, W=32, seed=0, dtype=mdm.BF16)
    optim = mdm.AdamW(model, lr=1e-4)
    ema = mdm.EMA(model, decay=args.ema_max_decay, inv_gamma=args.ema_inv_gamma, power=args.ema_power)
    sched = mdm.Scheduler(args, device=dev)
    sched.update_ddpm_num_steps(1000)
    step = TrainStep(model, sched, args, optim, ema, mean_shift=True)
    step.x0.copy_(torch.rand(N, 3, 32, 32, generator=torch.Generator().manual_seed(100)) * 2 - 1)
    return step, sched.get_timesteps_epoch(0, 1)


def window(step, used, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.run_device(None, used)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def per_entry_point(model, reps=5):
    """{entry point: {launches, ms}} over the forward and backward plans, every launch event-timed (median over `reps` eager runs)."""
    st = torch.cuda.current_stream().cuda_stream
    out, ov = {}, None
    for rec in (model.forward_plan, model.backward_plan):
        if ov is None:
            ov = rec.event_overhead(st, lambda i, name: name == "mdm_gemm")
        runs = [rec.run_timed(st, lambda i, name: True, ov) for _ in range(reps + 1)][1:]
        for k, (i, _) in enumerate(runs[0]):
            name = rec.calls[i][0]
            c, t = out.get(name, (0, 0.0))
            out[name] = (c + 1, t + statistics.median(r[k][1] for r in runs))
    return {k: {"launches": v[0], "ms": round(v[1], 4)} for k, v in sorted(out.items())}, round(ov, 5)


def resample_bytes(model):
    """Algorithmic bytes of the resampling launches of one step, per kernel: pool 4 reads + 1 write per output element, upsample
    1 read + 4 writes per source element (the accumulate flag adds a read of the destination; counted from the recorded arguments)."""
    from mdm.unet import _Resample
    esz = 2 if model.dt == 1 else 4
    out = {"avgpool2_kernel": 0, "upsample2_kernel": 0, "sumpool2_kernel": 0}
    for rec in (model.forward_plan, model.backward_plan):
        for c in rec.calls:
            name, a = c[0], c[2]
            if name in ("mdm_avgpool2", "mdm_sumpool2"):
                acc, (N, H, W, C) = a[3], a[4:8]
                out[name[4:] + "_kernel"] += N * H * W * C * esz * (5 + (1 if acc else 0))
            elif name == "mdm_upsample2":
                acc, (N, H, W, C) = a[3], a[5:9]
                out["upsample2_kernel"] += N * H * W * C * esz * (5 + (4 if acc else 0))
    out["resample_specs"] = sum(isinstance(s, _Resample) for s in model.specs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--once", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_cost.py needs a GPU")
    import mdm
    from mdm.train_step import TrainStep
    if opt.once:
        step, used = build(mdm, TrainStep, False, opt.batch)
        for _ in range(opt.warmup):
            step.run_device(None, used)
        ms = window(step, used, opt.steps)
        print(json.dumps({"metric": "cfg2 bf16 pooled preset, graph replays for a kernel trace", "steps": opt.steps, "warmup": opt.warmup,
                          "ms_per_step": round(ms, 4), "resample_bytes": resample_bytes(step.model)}))
        return
    runs = {"conv": build(mdm, TrainStep, True, opt.batch), "pool": build(mdm, TrainStep, False, opt.batch)}
    for step, used in runs.values():
        for _ in range(opt.warmup):
            step.run_device(None, used)
    ms = {k: [] for k in runs}
    for _ in range(opt.windows):                    # interleaved: both runs see the same clocks and the same neighbours
        for k, (step, used) in runs.items():
            ms[k].append(window(step, used, opt.steps))
    res = {}
    for k, (step, used) in runs.items():
        m = step.model
        by, ov = per_entry_point(m)
        res[k] = {"ms_per_step": round(statistics.median(ms[k]), 4), "windows_ms": [round(v, 4) for v in ms[k]],
                  "launches": {"forward_plan": len(m.forward_plan.calls), "backward_plan": len(m.backward_plan.calls)},
                  "parameters": m.num_parameters(), "loss": float(step.loss), "by_entry_point": by, "event_overhead_ms": ov}
        print(f"[resample_cost] {k}: {res[k]['ms_per_step']} ms/step, launches {res[k]['launches']}", file=sys.stderr, flush=True)
    res["pool"]["resample_bytes"] = resample_bytes(runs["pool"][0].model)
    a, b = res["conv"], res["pool"]
    names = sorted(set(a["by_entry_point"]) | set(b["by_entry_point"]))
    delta = {n: round(b["by_entry_point"].get(n, {"ms": 0.0})["ms"] - a["by_entry_point"].get(n, {"ms": 0.0})["ms"], 4) for n in names}
    print(json.dumps({"metric": "cfg2 bf16 train step, default preset against resample_with_conv=False", "batch": opt.batch,
                      "steps": opt.steps, "warmup": opt.warmup, "windows": opt.windows,
                      "delta_ms_per_step": round(b["ms_per_step"] - a["ms_per_step"], 4), "delta_ms_by_entry_point": delta, "runs": res}))


if __name__ == "__main__":
    main()
