#!/usr/bin/env python3
"""A short cfg2 loop (bench.py's workload: 32x3x32x32, unet6 preset, 35.75 M parameters, bf16, EMA) with each optimizer in ONE process,
for one `rocprofv3 --kernel-trace --stats` run: the four `optim_update_kernel<KIND, W>` instantiations next to each other (time per
byte moved).  Bytes per parameter with EMA and bf16 shadow (csrc/optim.hip): AdamW / Adam 20 read + 18 written, SGD with momentum
16 + 14, SGD 12 + 10.  (A trace of a revision that still had the separate `adamw_kernel` is summarised too.)

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 scripts/prof_optimizers.py [steps]
    python3 scripts/prof_optimizers.py --summarise OUT/.../kernel_stats.csv STORE_SIZE     # -> the optimizer rows + ps per byte
"""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "masked-diffusion-model_amd")):
    sys.path.insert(0, p)

BYTES = {3: 38, 2: 38, 1: 30, 0: 22}           # by kind: AdamW, Adam, SGD with momentum, SGD


def _bytes_of(name):
    m = re.search(r"optim_update_kernel<(?:\(int\))?(\d)", name)      # the kind is the first template argument
    if m:
        return BYTES[int(m.group(1))]
    return BYTES[3] if "adamw_kernel" in name else None


def summarise(path, n):
    """`n`: the length of the sweep = the store size `main()` prints (the flat store pads channels to multiples of 8)."""
    with open(path) as fh:
        rows = list(csv.DictReader(fh))
    out = csv.writer(sys.stdout)
    out.writerow(["Name", "Calls", "AverageNs", "MinNs", "MaxNs", "bytes_per_element", "GB_moved", "TB_per_s_at_average", "ps_per_byte"])
    for r in rows:
        b = _bytes_of(r["Name"])
        if b:
            avg = float(r["AverageNs"])
            out.writerow([r["Name"], r["Calls"], round(avg), r["MinNs"], r["MaxNs"], b, round(n * b / 1e9, 3),
                          round(n * b / avg / 1e3, 2), round(avg * 1e3 / (n * b), 4)])


def main(steps):
    import torch

    import mdm
    from bench import make_args
    from mdm.train_step import TrainStep
    dev = torch.device("cuda", 0)
    a = make_args(seed=1234)
    model = mdm.UNet(mdm.unet6_config(32), N=32, H=32, W=32, dtype=mdm.BF16, seed=0)
    sched = mdm.Scheduler(a, device=dev)
    sched.update_ddpm_num_steps(1000)
    used = sched.get_timesteps_epoch(0, 1)
    x0 = torch.rand(32, 3, 32, 32) * 2 - 1
    for make in (lambda: mdm.AdamW(model, lr=1e-4), lambda: mdm.Adam(model, lr=1e-4), lambda: mdm.SGD(model, lr=1e-4, momentum=0.9),
                 lambda: mdm.SGD(model, lr=1e-4)):
        opt = make()
        ema = mdm.EMA(model, decay=a.ema_max_decay, inv_gamma=a.ema_inv_gamma, power=a.ema_power)
        step = TrainStep(model, sched, a, opt, ema, mean_shift=True)
        step.x0.copy_(x0)
        for _ in range(steps):
            loss = step.run_device(None, used)
        torch.cuda.synchronize()
        print(type(opt).__name__, opt.param_groups[0].get("momentum", ""), "store size", model.store.size, "loss", float(loss), flush=True)
        del step, opt, ema


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], int(sys.argv[3]))
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
