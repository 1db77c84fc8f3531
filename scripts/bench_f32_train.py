"""fp32 training step of cfg2 (unet6 at 32x32, N = 32 per GPU, T = 1000, mean-shift trainer, device RNG, one hipGraph per step)
in four precisions, timed the way bench.py times its headline step (warm-up steps, then --steps back-to-back graph replays between
two synchronisations):

  f32_exact        UNet(dtype=F32)                                            every contraction exact fp32
  f32_split_fwd    UNet(dtype=F32, f32_products="split")                      forward products as bf16 hi / lo pairs
  f32_split_grad   UNet(dtype=F32, f32_products="split", grad_products="split")   ... and the backward's convolution products too
  bf16             UNet(dtype=BF16)                                           bf16 storage, for context

Prints ONE JSON line: ms/step, images/s and TFLOP/s (bench.py's flop count: 34.87 GFLOP per image) for each mode.
    python scripts/bench_f32_train.py [--steps 20] [--warmup 5] [--modes f32_exact,f32_split_grad]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "masked-diffusion-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench import make_args  # noqa: E402

FLOPS_IMG = 34.87e9         # bench.py's cfg2 count per image and train step
MODES = {
    "f32_exact": dict(dtype=0),
    "f32_split_fwd": dict(dtype=0, f32_products="split"),
    "f32_split_grad": dict(dtype=0, f32_products="split", grad_products="split"),
    "bf16": dict(dtype=1),
}


def run_mode(mdm, TrainStep, kw, N, steps, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    args = make_args(batch_size=N, seed=1234, mixed_precision="no" if kw["dtype"] == 0 else "bf16")
    model = mdm.UNet(mdm.unet6_config(32), N=N, H=32, W=32, seed=0, **kw)
    optim = mdm.AdamW(model, lr=1e-4)
    ema = mdm.EMA(model, decay=args.ema_max_decay, inv_gamma=args.ema_inv_gamma, power=args.ema_power)
    sched = mdm.Scheduler(args, device=dev)
    sched.update_ddpm_num_steps(1000)
    used = sched.get_timesteps_epoch(0, 1)
    step = TrainStep(model, sched, args, optim, ema, mean_shift=True)
    g = torch.Generator().manual_seed(100)
    step.x0.copy_(torch.rand(N, 3, 32, 32, generator=g) * 2 - 1)
    for _ in range(warmup):
        step.run_device(None, used)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.run_device(None, used)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    out = {"ms_per_step": round(ms, 4), "images_per_s": round(N / (ms * 1e-3), 1),
           "tflops": round(FLOPS_IMG * N / (ms * 1e-3) / 1e12, 1), "loss": float(step.loss)}
    if kw.get("grad_products") == "split":
        tab = model.grad_products_table()
        out["split_grads"] = sum(1 for v in tab.values() for r in v.values() if not r.startswith("exact"))
        out["exact_grads"] = sum(1 for v in tab.values() for r in v.values() if r.startswith("exact"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--modes", default=",".join(MODES))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f32_train.py needs a GPU")
    import mdm
    from mdm.train_step import TrainStep
    res = {}
    for name in opt.modes.split(","):
        res[name] = run_mode(mdm, TrainStep, MODES[name], opt.batch, opt.steps, opt.warmup)
        print(f"[bench_f32_train] {name}: {res[name]}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "cfg2 train step, fp32 precisions", "batch": opt.batch, "steps": opt.steps, "warmup": opt.warmup,
                      "flops_per_image": FLOPS_IMG, "modes": res}))


if __name__ == "__main__":
    main()
