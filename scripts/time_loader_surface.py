"""What feeding the drop-in trainer costs per step at cfg2 (unet6 at 32x32, N = 32, bf16, mean-shift trainer, device RNG, one hipGraph
per step, args.monitor + args.defer_loss: no host sync per step): `Trainer._run_epoch` over 200 batches of the same 6 400 images from

    resident  a Python list of device batches (what scripts/time_trainer_surface.py and bench.py feed: nothing to load)
    host0     upstream's data path: the set in RAM as one fp32 tensor behind DataLoader(shuffle=True, drop_last=True, pin_memory=True),
    host8     num_workers 0 and 8 (persistent workers, as main_train_masked.py:92-102)
    device    mdm.DeviceLoader over the set as uint8 in device memory: one mdm_data_gather launch per batch, into TrainStep.x0

Every measurement is a CHILD process of its own under `timeout` (one loader, one warm-up epoch that also captures the graph and
starts the workers, then --epochs timed epochs), and the children are interleaved resident, host0, host8, device, resident, ... so
that all loaders see the same box at the same time.  A child that fails, faults or runs into its time limit ends the run: nothing
more is started on the GPU.  The figure of a loader is the median over its timed epochs of all rounds, in ms/step; the spread of
`resident` between rounds (max - min of the rounds' medians) is reported next to it as the yardstick for "no difference".  A last
child times the gather launch on its own (HIP events).  Writes profiles/<--out> and prints it.

    python scripts/time_loader_surface.py [--rounds 3] [--epochs 3] [--batches 200] [--limit 240] [--out loader_surface.json]
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

MODES = ("resident", "host0", "host8", "device")


def images(batches, N):
    """The data set of every mode: uint8 [batches N, 3, 32, 32] and its fp32 values under upstream's Normalize."""
    import torch
    u8 = torch.randint(0, 256, (batches * N, 3, 32, 32), generator=torch.Generator().manual_seed(100), dtype=torch.uint8)
    lut = (torch.arange(256, dtype=torch.uint8).float().div(255) - 0.5) / 0.5
    return u8, lut


def child(mode, batches, epochs, N=32):
    import torch
    from torch.utils.data import DataLoader, Dataset
    u8, lut = images(batches, N)

    class InMemory(Dataset):                                       # MyDataset (utils/mydataset.py:235-278) without the file reading
        def __init__(self):
            self.data, self.label = lut[u8.long()], torch.zeros(len(u8))
            self.random = torch.FloatTensor(len(u8), 1).uniform_(-1.0, 1.0)

        def __len__(self):
            return len(self.data)

        def __getitem__(self, i):
            return self.data[i], self.label[i], self.random[i]
    loader = None
    if mode.startswith("host"):
        w = int(mode[4:])
        loader = DataLoader(InMemory(), batch_size=N, drop_last=True, shuffle=True, pin_memory=True, num_workers=w,
                            persistent_workers=w > 0, generator=torch.Generator().manual_seed(0))
        if w:
            iter(loader)                                           # the workers are forked here, before this process opens the GPU

    import mdm
    from bench import make_args
    dev = torch.device("cuda", torch.cuda.current_device())
    args = make_args(batch_size=N, seed=1234, mixed_precision="bf16", monitor=True, defer_loss=True)
    model = mdm.UNet(mdm.unet6_config(32), N=N, H=32, W=32, seed=0, dtype=mdm.BF16)
    optim = mdm.AdamW(model, lr=1e-4)
    ema = mdm.EMA(model, decay=args.ema_max_decay, inv_gamma=args.ema_inv_gamma, power=args.ema_power)
    if mode == "resident":
        x = lut[u8.long()]
        loader = [(x[k * N:(k + 1) * N].to(dev), None, None) for k in range(batches)]
    elif mode == "device":
        loader = mdm.DeviceLoader(mdm.DeviceDataset(u8, device=dev), N, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(0))
    assert len(loader) == batches
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
    print(json.dumps({"mode": mode, "ms_per_step": ms, "last_loss": losses[-1]}), flush=True)
    del tr, loader                                                 # (persistent workers end with their loader)


def gather_launch(batches, N=32, reps=50):
    """The mdm_data_gather launch of a cfg2 batch on its own, uint8 storage, shuffled indices, labels and random with it: HIP events
    around one launch (median of `reps`) and around `batches` back-to-back launches (per launch), in microseconds."""
    import torch

    import mdm
    dev = torch.device("cuda", torch.cuda.current_device())
    u8, _ = images(batches, N)
    ds = mdm.DeviceDataset(u8, device=dev)
    index = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0)).to(dev)
    x0, lab, rnd = torch.empty(N, 3, 32, 32, device=dev), torch.empty(N, device=dev), torch.empty(N, ds.R, device=dev)

    def timed(first_list):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for f in first_list:
            ds.gather(index, f, N, x0, None, lab, rnd)
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b)
    firsts = [k * N for k in range(batches)]
    timed(firsts[:20])                                             # warm
    one = [timed([firsts[k % batches]]) for k in range(reps)]
    many = [timed(firsts) / batches for _ in range(5)]
    print(json.dumps({"gather_us": {"one_launch_event_pair": round(statistics.median(one), 2),
                                    "back_to_back_per_launch": round(statistics.median(many), 2),
                                    "bytes_in": N * 3 * 32 * 32, "bytes_out": 4 * N * 3 * 32 * 32}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=list(MODES) + ["gather"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child, seconds")
    ap.add_argument("--out", default="loader_surface.json")
    opt = ap.parse_args()
    if opt.child == "gather":
        return gather_launch(opt.batches)
    if opt.child:
        return child(opt.child, opt.batches, opt.epochs)
    runs = {m: [] for m in MODES}
    round_medians = {m: [] for m in MODES}
    for r in range(opt.rounds):
        for m in MODES:                                            # interleaved
            cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), "--child", m,
                   "--batches", str(opt.batches), "--epochs", str(opt.epochs)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                raise SystemExit(f"[time_loader_surface] {m} (round {r}) ended with status {p.returncode}: stopping, nothing more is started")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            runs[m].extend(res["ms_per_step"])
            round_medians[m].append(statistics.median(res["ms_per_step"]))
            print(f"[time_loader_surface] round {r} {m}: {[round(v, 4) for v in res['ms_per_step']]} ms/step", file=sys.stderr, flush=True)
    out = {"metric": "cfg2 bf16 Trainer._run_epoch (monitor + defer_loss), ms per step, 200 batches of the same 6400 images per epoch",
           "batches": opt.batches, "rounds": opt.rounds, "epochs_per_round": opt.epochs,
           "modes": {m: {"ms_per_step": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                         "round_medians": [round(x, 4) for x in round_medians[m]], "epochs_ms_per_step": [round(x, 4) for x in v]}
                     for m, v in runs.items()}}
    p = subprocess.run(["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), "--child", "gather",
                        "--batches", str(opt.batches)], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise SystemExit(f"[time_loader_surface] the gather timing ended with status {p.returncode}")
    out.update(json.loads(p.stdout.strip().splitlines()[-1]))
    med = {m: out["modes"][m]["ms_per_step"] for m in MODES}
    spread = max(round_medians["resident"]) - min(round_medians["resident"])
    diff = med["device"] - med["resident"]
    out["resident_round_spread_ms"] = round(spread, 4)
    out["device_minus_resident_ms"] = round(diff, 4)
    out["device_minus_resident_minus_gather_ms"] = round(diff - 1e-3 * out["gather_us"]["back_to_back_per_launch"], 4)
    out["device_within_resident_spread_of_gather_time"] = bool(abs(diff - 1e-3 * out["gather_us"]["back_to_back_per_launch"]) <= spread)
    out["device_not_slower_than_host"] = bool(med["device"] <= min(med["host0"], med["host8"]))
    path = os.path.join(ROOT, "profiles", opt.out)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
