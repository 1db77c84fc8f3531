"""What the drop-in trainer surface costs per step at cfg2 (unet6 at 32x32, N = 32, bf16, mean-shift trainer, device RNG, one
hipGraph per step): `Trainer._run_epoch` over 200 device-resident batches in three modes

    off      args.monitor unset: `_run_batch` ends in the LossCell read (one host sync per step)        -- the parent's behaviour
    monitor  args.monitor: five monitors summed in the loss kernel + one commit launch; `_run_batch` ends in a 32-byte ring read
    defer    args.monitor + args.defer_loss: no host sync per step, the ring is read once per epoch

Every measurement is a CHILD process of its own under `timeout` (one mode, one warm-up epoch that also captures the graph, then
--epochs timed epochs), and the children are interleaved off, monitor, defer, off, ... so that all modes see the same box at the
same time.  A child that fails, faults or runs into its time limit ends the run: nothing more is started on the GPU.
The figure of a mode is the median over its timed epochs of all rounds, in ms/step; a last child times the loss and the commit
launch on their own (HIP events around eager launches).  Writes profiles/<--out> and prints it.

    python scripts/time_trainer_surface.py [--rounds 3] [--epochs 3] [--batches 200] [--limit 240] [--out r10_trainer_surface.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "masked-diffusion-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODES = {"off": {}, "monitor": dict(monitor=True), "defer": dict(monitor=True, defer_loss=True)}


def child(mode, batches, epochs, N=32):
    import torch

    import mdm
    from bench import make_args
    dev = torch.device("cuda", torch.cuda.current_device())
    args = make_args(batch_size=N, seed=1234, mixed_precision="bf16", **MODES[mode])
    model = mdm.UNet(mdm.unet6_config(32), N=N, H=32, W=32, seed=0, dtype=mdm.BF16)
    optim = mdm.AdamW(model, lr=1e-4)
    ema = mdm.EMA(model, decay=args.ema_max_decay, inv_gamma=args.ema_inv_gamma, power=args.ema_power)
    g = torch.Generator().manual_seed(100)
    loader = [((torch.rand(N, 3, 32, 32, generator=g) * 2 - 1).to(dev), None, None) for _ in range(batches)]
    tr = mdm.Trainer(args, loader, None, [None] * 3, model, ema, optim, mdm.get_lr_scheduler("constant", optim, 0, 1), mdm.Accelerator())
    args.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(args.ddpm_num_steps)
    losses = tr._run_epoch(0, 1, 0, None, None)                   # warm-up: captures the step graph
    torch.cuda.synchronize()
    ms = []
    for e in range(epochs):
        t0 = time.perf_counter()
        losses = tr._run_epoch(0, 1, 0, None, None)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / batches)
    assert len(losses) == batches and all(v == v for v in losses), "an epoch returned a short or NaN loss list"
    launches = len(tr.step._graphs[1].rec.calls)
    print(json.dumps({"mode": mode, "ms_per_step": ms, "launches_per_step": launches, "last_loss": losses[-1]}), flush=True)


def per_launch(batches=4, reps=7, N=32):
    """Event-timed loss launch of the unmonitored and the monitored step and the commit launch (eager replays of the recorded
    step, `_lib.Recording.run_timed`, event overhead taken off; median over `reps`), in microseconds."""
    import torch

    import mdm
    from bench import make_args
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    for mode in ("off", "monitor"):
        args = make_args(batch_size=N, seed=1234, mixed_precision="bf16", **MODES[mode])
        model = mdm.UNet(mdm.unet6_config(32), N=N, H=32, W=32, seed=0, dtype=mdm.BF16)
        optim = mdm.AdamW(model, lr=1e-4)
        ema = mdm.EMA(model, decay=args.ema_max_decay, inv_gamma=args.ema_inv_gamma, power=args.ema_power)
        g = torch.Generator().manual_seed(100)
        loader = [((torch.rand(N, 3, 32, 32, generator=g) * 2 - 1).to(dev), None, None) for _ in range(batches)]
        tr = mdm.Trainer(args, loader, None, [None] * 3, model, ema, optim, mdm.get_lr_scheduler("constant", optim, 0, 1), mdm.Accelerator())
        args.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(args.ddpm_num_steps)
        tr._run_epoch(0, 1, 0, None, None)
        torch.cuda.synchronize()
        rec = tr.step._graphs[1].rec
        st = torch.cuda.current_stream().cuda_stream
        ov = rec.event_overhead(st, lambda i, name: name == "mdm_gemm")
        pick = lambda i, name: name in ("mdm_loss_fwd_bwd", "mdm_loss_fwd_bwd_mon", "mdm_monitor_commit")
        runs = [rec.run_timed(st, pick, ov) for _ in range(reps + 1)][1:]
        torch.cuda.synchronize()
        for k, (i, _) in enumerate(runs[0]):
            out[f"{mode}:{rec.calls[i][0]}"] = round(1e3 * statistics.median(r[k][1] for r in runs), 2)
        out[f"{mode}:event_overhead"] = round(1e3 * ov, 2)
    print(json.dumps({"per_launch_us": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=sorted(MODES) + ["launches"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child, seconds")
    ap.add_argument("--out", default="r10_trainer_surface.json")
    opt = ap.parse_args()
    if opt.child == "launches":
        return per_launch()
    if opt.child:
        return child(opt.child, opt.batches, opt.epochs)
    runs = {m: [] for m in MODES}
    launches = {}
    for r in range(opt.rounds):
        for m in MODES:                                            # interleaved
            cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), "--child", m,
                   "--batches", str(opt.batches), "--epochs", str(opt.epochs)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                raise SystemExit(f"[time_trainer_surface] {m} (round {r}) ended with status {p.returncode}: stopping, nothing more is started")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            runs[m].extend(res["ms_per_step"])
            launches[m] = res["launches_per_step"]
            print(f"[time_trainer_surface] round {r} {m}: {[round(v, 4) for v in res['ms_per_step']]} ms/step", file=sys.stderr, flush=True)
    out = {"metric": "cfg2 bf16 Trainer._run_epoch, ms per step over device-resident batches", "batches": opt.batches,
           "rounds": opt.rounds, "epochs_per_round": opt.epochs,
           "modes": {m: {"ms_per_step": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                         "launches_per_step": launches[m], "epochs_ms_per_step": [round(x, 4) for x in v]} for m, v in runs.items()}}
    off = out["modes"]["off"]["ms_per_step"]
    for m in ("monitor", "defer"):
        out["modes"][m]["vs_off_percent"] = round(100.0 * (out["modes"][m]["ms_per_step"] / off - 1.0), 2)
    p = subprocess.run(["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), "--child", "launches"],
                       stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise SystemExit(f"[time_trainer_surface] per-launch timing ended with status {p.returncode}")
    out.update(json.loads(p.stdout.strip().splitlines()[-1]))
    path = os.path.join(ROOT, "profiles", opt.out)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
