#!/usr/bin/env python3
"""Golden values of the reference's per-step monitors (trainer_masked_mean_shift.py:175-179).

    python tests/golden/make_monitor_golden.py       # writes tests/golden/train_monitors.npz

Drives the reference's `_run_batch` exactly as make_golden.py's `gen_train_step` builds the `step_*` fixtures of
train_step.npz (same model, same batch, seed 500) and stores, per fixture, the five scalars the trainer leaves behind:
train_loss, inverse_reconstruct_train_mean, reconstruct_train_mean, shifted_degrade_img_mean, degraded_train_mean --
in fp32 as the reference's `.mean()` returns them, and again as fp64 means over the same fp32 tensors (what a summation
bound is measured against), plus rms(pred).  The base trainer (trainer_masked.py:161-162) keeps two of them; without a
shift the other two are the same tensors.  Floats only.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

NAMES = ("train_loss", "inverse_reconstruct_train_mean", "reconstruct_train_mean", "shifted_degrade_img_mean", "degraded_train_mean")


def gen_monitors(scheduler_mod, unet6, out):
    import accelerate
    import trainer_masked
    import trainer_masked_mean_shift
    tmp = tempfile.mkdtemp()
    dirs = types.SimpleNamespace(list_dir={"train_loss": tmp, "checkpoint": tmp, "ema_sample_img": tmp})
    g = torch.Generator().manual_seed(21)
    x0 = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1
    out["mon_x0"] = mg.npy(x0)
    out["mon_names"] = np.array(NAMES)
    for name, mod, st, sel, ch, kind, lw in (
            ("ms", trainer_masked_mean_shift, "noise_with_perturbation", "thresholding", "1-channel", "linear", False),
            ("ms_w", trainer_masked_mean_shift, "1-d_constant", "thresholding", "3-channel", "exponential", True),
            ("base", trainer_masked, "non_shift", "indexing", None, "log", False)):
        a = mg.base_args(data_size=16, ddpm_schedule=kind, ddpm_num_steps=10, select_degrade_pixel=sel, degrade_channel=ch,
                         shift_type=st, loss_weight_use=lw, batch_size=4, sample_num=2, sample_latent_shape="zero")
        model = mg._Wrap(mg.build_ref_unet(unet6, mg.TINY))
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        lr_s = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0)
        acc = accelerate.Accelerator(cpu=True)
        if name == "base":
            class T(mod.Trainer):                      # constructor bypass
                def __init__(self, args, model, opt, lr_s, acc):
                    self.args, self.model, self.optimizer, self.lr_scheduler, self.accelerator = args, model, opt, lr_s, acc
                    self.ema_model = None; self.lr_list = []; self.global_step = 0
                    self.Scheduler = scheduler_mod.Scheduler(args)
            tr = T(a, model, opt, lr_s, acc)
        else:
            tr = mod.Trainer(a, None, None, [None] * 3, model, None, opt, lr_s, acc)
        a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(a.ddpm_num_steps)
        tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
        mg.seed_all(500)
        r = tr._run_batch(0, (x0, None, None), 0, 1, 0, dirs, None)
        if name == "base":
            loss = r[0]
            tensors = (tr.reconstructed_img, tr.reconstructed_img, tr.degraded_img, tr.degraded_img)
            vals = [loss, float(tr.reconstruct_train_mean), float(tr.reconstruct_train_mean), float(tr.degraded_train_mean),
                    float(tr.degraded_train_mean)]
        else:
            loss = r
            tensors = (tr.inverse_shift_reconstructed_img, tr.reconstructed_img, tr.shifted_degrade_img, tr.degraded_img)
            vals = [float(getattr(tr, n)) for n in NAMES]
            assert vals[0] == loss
        out[f"mon_{name}"] = np.array(vals, dtype=np.float64)
        out[f"mon_{name}_f64"] = np.array([float(t.detach().double().mean()) for t in tensors], dtype=np.float64)
        out[f"mon_{name}_absmean"] = np.array([float(t.detach().double().abs().mean()) for t in tensors], dtype=np.float64)
        out[f"mon_{name}_pred_rms"] = np.array(float(tr.mask.detach().double().pow(2).mean().sqrt()))
        print(f"  mon_{name}: {vals}")


def main():
    mg._stub_modules()
    sys.path.insert(0, mg.REF)
    import scheduler as scheduler_mod
    from models.unet import unet6
    torch.set_num_threads(4)
    o = {}
    gen_monitors(scheduler_mod, unet6, o)
    path = os.path.join(HERE, "train_monitors.npz")
    np.savez_compressed(path, **o)
    print(f"train_monitors: {len(o)} arrays -> {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
