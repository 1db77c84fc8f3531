"""`sample` next to `sample_inpaint` at the sampler-of-record shape (100 x 3 x 64 x 64, fp32 storage with split products, history off,
device RNG, one graph per step): wall clock per reverse step of both, and -- run under `rocprofv3 --kernel-trace --stats` -- the
kernels of both in one trace.  `--summary stats.csv` prints the rows of the x0 / inpaint kernels from such a trace instead.

    python scripts/prof_inpaint.py [--steps 40] [--size 64] [--num 100]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/prof_inpaint.py
    python scripts/prof_inpaint.py --summary OUT/.../..._kernel_stats.csv
"""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "masked-diffusion-model_amd"))


def summary(path):
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        if any(k in r["Name"] for k in ("sampler_x0_kernel", "inpaint_x0_kernel", "inpaint_start_kernel", "sampler_update_kernel")):
            print(f"{r['Name'][:96]:96s} calls {int(r['Calls']):5d}  mean {float(r['AverageNs']) / 1e3:8.2f} us  min {float(r['MinNs']) / 1e3:8.2f}"
                  f"  max {float(r['MaxNs']) / 1e3:8.2f}  stddev {float(r['StdDev']) / 1e3:7.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--num", type=int, default=100)
    ap.add_argument("--summary")
    o = ap.parse_args()
    if o.summary:
        return summary(o.summary)
    import torch
    import mdm
    from bench import make_args
    H, N = o.size, o.num
    a = make_args(data_size=H, sample_num=N)
    model = mdm.UNet(mdm.unet6_config(H), N=N, H=H, W=H, dtype=mdm.F32, seed=0, f32_products="split").eval()
    S = mdm.Scheduler(a)
    S.update_ddpm_num_steps(1000)
    full = S.get_timesteps_epoch(0, 1)
    stride = max(1, len(full) // o.steps)
    used = full[stride - 1::stride]                                  # evenly spread and ending at T, so a 'matched' run has steps to skip
    smp = mdm.Sampler(None, a, S, [None] * 3)
    g = torch.Generator().manual_seed(0)
    known = (torch.rand(N, 3, H, H, generator=g) * 2 - 1).cuda()
    keep = mdm.inpaint_keep("box", N, H, H, top=H // 4, left=H // 4, height=H // 2, width=H // 2).cuda()
    runs = {"sample": lambda ts: smp.sample(model, ts), "sample_inpaint": lambda ts: smp.sample_inpaint(model, ts, known, keep),
            "sample_inpaint matched": lambda ts: smp.sample_inpaint(model, ts, known, keep, "matched")}
    for name, f in runs.items():
        f(used[:3]); torch.cuda.synchronize()                       # warm-up / graph capture
        per = []
        for _ in range(3):
            t0 = time.perf_counter()
            x0, _ = f(used)
            torch.cuda.synchronize()
            per.append(1e3 * (time.perf_counter() - t0))
        ran = len(smp._graph_keep[0][1])
        print(f"{name}: {ran} steps, ms per run {[round(p, 2) for p in per]}, ms per step {min(per) / ran:.4f} (best of 3), "
              f"finite {bool(torch.isfinite(x0).all())}", flush=True)


if __name__ == "__main__":
    main()
