"""What residual-block dropout costs at cfg2 (unet6 at 32x32, N = 32, bf16, mean-shift trainer, device RNG, one hipGraph per step):
`TrainStep.run_device` with drop_rate 0 and 0.1 on ONE box, in interleaved windows (0, 0.1, 0, 0.1, ...; each window = --steps
back-to-back graph replays between two synchronisations, after --warmup steps per model; the figure of a run is the median of its
windows, the spread is reported next to it).  Then both recorded plans once more EAGERLY with a HIP event pair around every
GroupNorm and every contraction launch (event overhead taken off, `_lib.Recording.run_timed`), to split the difference into

  - the small-map epilogue fusions a dropout site gives up (its norm2 runs as a launch of its own in both directions:
    more GroupNorm launches, and conv launches without the gnf / gnb epilogue), and
  - the Philox arithmetic inside the GroupNorm kernels that ran as launches before as well (the large maps).

Prints ONE JSON line.
    python scripts/dropout_cost.py [--steps 20] [--warmup 5] [--windows 5] [--rate 0.1]
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

GN = ("mdm_groupnorm_fwd", "mdm_groupnorm_bwd")
GN_KEYS = GN + tuple(n + "_dropout" for n in GN)      # per_launch reports a launch whose descriptor has rng under NAME_dropout
CONV = ("mdm_gemm", "mdm_gemm_pair", "mdm_wgrad_group_launch")


def build(mdm, TrainStep, rate, N):
    dev = torch.device("cuda", torch.cuda.current_device())
    args = make_args(batch_size=N, seed=1234, mixed_precision="bf16")
    model = mdm.UNet(mdm.unet6_config(32, drop_rate=rate), N=N, H=32, W=32, seed=0, dtype=mdm.BF16)
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


def per_launch(model, reps=5):
    """Summed time (ms, median over `reps` eager replays) and count of the GroupNorm and the contraction launches of both plans,
    GroupNorm launches also per kernel family: {name: (count, ms)}."""
    st = torch.cuda.current_stream().cuda_stream
    pick = lambda i, name: name in GN or name in CONV
    sums = []
    for rec in (model.forward_plan, model.backward_plan):
        ov = rec.event_overhead(st, lambda i, name: name == "mdm_gemm") if rec is model.forward_plan else sums[0][1]
        runs = [rec.run_timed(st, pick, ov) for _ in range(reps + 1)][1:]
        names = [rec.calls[i][0] + ("_dropout" if rec.calls[i][0] in GN and rec.calls[i][2][0]._obj.rng else "") for i, _ in runs[0]]
        med = [statistics.median(r[k][1] for r in runs) for k in range(len(names))]
        sums.append((list(zip(names, med)), ov))
    out = {}
    for name, ms in sums[0][0] + sums[1][0]:
        c, t = out.get(name, (0, 0.0))
        out[name] = (c + 1, t + ms)
    tot = lambda group: (sum(out[n][0] for n in group if n in out), round(sum(out[n][1] for n in group if n in out), 4))
    return {"groupnorm": dict(zip(("launches", "ms"), tot(GN_KEYS))), "conv": dict(zip(("launches", "ms"), tot(CONV))),
            "by_entry_point": {k: {"launches": v[0], "ms": round(v[1], 4)} for k, v in sorted(out.items())},
            "event_overhead_ms": round(sums[0][1], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rate", type=float, default=0.1)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dropout_cost.py needs a GPU")
    import mdm
    from mdm.train_step import TrainStep
    runs = {"drop_0": build(mdm, TrainStep, 0.0, opt.batch), f"drop_{opt.rate:g}": build(mdm, TrainStep, opt.rate, opt.batch)}
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
        res[k] = {"ms_per_step": round(statistics.median(ms[k]), 4), "windows_ms": [round(v, 4) for v in ms[k]],
                  "launches": {"forward_plan": len(m.forward_plan.calls), "backward_plan": len(m.backward_plan.calls)},
                  "dropout_sites": len(m.dropout_sites()), "loss": float(step.loss)}
        res[k].update(per_launch(m))
        print(f"[dropout_cost] {k}: {res[k]['ms_per_step']} ms/step, GroupNorm {res[k]['groupnorm']}, conv {res[k]['conv']}",
              file=sys.stderr, flush=True)
    a, b = res["drop_0"], res[f"drop_{opt.rate:g}"]
    print(json.dumps({"metric": "cfg2 bf16 train step with and without residual-block dropout", "batch": opt.batch, "steps": opt.steps,
                      "warmup": opt.warmup, "windows": opt.windows, "rate": opt.rate,
                      "delta_ms_per_step": round(b["ms_per_step"] - a["ms_per_step"], 4),
                      "delta_groupnorm_ms": round(b["groupnorm"]["ms"] - a["groupnorm"]["ms"], 4),
                      "delta_conv_ms": round(b["conv"]["ms"] - a["conv"]["ms"], 4), "runs": res}))


if __name__ == "__main__":
    main()
