"""Trainers with the reference's call surface.

`Trainer` mirrors reference trainer_masked_mean_shift.py (`Trainer.__init__` :29-66, `_run_batch`
:82-193, `_run_epoch` :196-215, `train` :218-273, `_save_ema_momentum_sample` :409-425);
`BaseTrainer` mirrors trainer_masked.py (:31-82, :95-183, :186-208, :211-272), whose constructor is
broken upstream (D2) -- the arithmetic is mean-shift with no shift, int timesteps and three return
values.  wandb / matplotlib output of the reference is out of scope; samples are saved as tensors, and with
`args.visuals` also as the PNG upstream writes.

`args.visuals` turns on the reference's image surface (ms:58-59, 235-236, 263-264, 301-318, 423-425): `train()` calls
`visualizer.reset()` at the top of every epoch and `visualizer.display_current_results(epoch, self.get_current_visuals(epoch))`
in the save block, and `_save_ema_momentum_sample` sets the two EMA sample grids and writes `ema_sample_{epoch:05d}.png`.
`get_current_visuals` is upstream's OrderedDict of fp32 CHW grids, built on the device (mdm/visuals.py: per grid one range launch
and one grid launch, no host sync).  The visual tensors the step does not keep (`degradation_mask`, `mean_pixel`,
`reconstructed_img`, `inverse_shift_reconstructed_img`, `mask`) are made when it is called, from the buffers the last step
left; with `visuals` off `_run_batch` and `train()` issue exactly what they did before.  Under data parallelism the training
grids are THIS rank's tensors (upstream draws the main process's too).

`args.monitor` turns on the reference's per-step logging surface (ms:61-64, 175-179, 249-250, 321-334): `loss_names` is
its five names, the five attributes hold the step's values after every `_run_batch`, `get_current_losses()` /
`get_current_mean()` return its OrderedDicts and `train()` hands them to `visualizer.plot_current_losses`.  The values
come from the device-side ring of mdm.MonitorRing, not from torch reductions.  Under data parallelism they are THIS
rank's (upstream logs the main process's local values too: ms:249 runs on the main process over its own tensors).
`args.defer_loss` (needs `monitor`): `_run_batch` returns a handle instead of a float and `_run_epoch` reads the ring once
per epoch (once per `monitor_cap` steps when the dataloader is longer), so an epoch runs without a host sync per step.
"""
from __future__ import annotations

import os
import statistics
from collections import OrderedDict

import torch

from .data import DeviceLoader
from .dist import GradComm
from .sampler import Sampler
from .scheduler import Scheduler
from .train_step import DeferredLoss, MonitorRing, TrainStep


class Trainer:
    mean_shift = True

    def __init__(self, args, dataloader, dataset, dataset_hist, model, ema_model, optimizer, lr_scheduler, accelerator):
        self.args, self.dataloader, self.dataset, self.dataset_hist = args, dataloader, dataset, dataset_hist
        self.model, self.ema_model, self.optimizer, self.lr_scheduler = model, ema_model, optimizer, lr_scheduler
        self.lr_list = []
        self.accelerator = accelerator
        self.Scheduler = Scheduler(args, device=model.device)
        self.Sampler = Sampler(self.dataset, self.args, self.Scheduler, self.dataset_hist)
        self.global_step = 0
        self.timesteps_used_epoch = None
        comm = GradComm(wire=getattr(args, "grad_wire_dtype", "f32")) if getattr(accelerator, "num_processes", 1) > 1 else None
        ema = ema_model if getattr(args, "use_ema", False) else None
        self.step = TrainStep(model, self.Scheduler, args, optimizer, ema, mean_shift=self.mean_shift, comm=comm,
                              grad_accum=getattr(accelerator, "gradient_accumulation_steps", 1))
        if isinstance(dataloader, DeviceLoader):       # the gather writes the batch where the step reads it: `_step` passes x0=None
            if dataloader.batch_size != model.N:
                raise ValueError(f"DeviceLoader batch_size {dataloader.batch_size} is not the model's batch {model.N}")
            dataloader.bind(self.step.x0)
        self.monitor = self.step.mon is not None
        self.defer_loss = bool(getattr(args, "defer_loss", False))
        if self.defer_loss and not self.monitor:
            raise ValueError("args.defer_loss needs args.monitor: a deferred loss is read from the monitor ring")
        self.loss_names = list(MonitorRing.COLUMNS[:5]) if self.monitor else ["train_loss"]          # ms:61
        self.mean_names = ["ema_sample_mean"]                                                        # ms:64
        self.visuals = bool(getattr(args, "visuals", False))
        self.train_visual_names = ["input", "degraded_img", "degrade_binary_masks", "degradation_mask", "mean_pixel", "shift",
                                   "shifted_degrade_img", "reconstructed_img", "inverse_shift_reconstructed_img", "mask"]   # ms:58
        self.sample_visual_names = ["ema_sample_result_normalize_global", "ema_sample_result_normalize_local"]          # ms:59
        # what `accelerator.save_state(path)` / `load_state(path)` cover (main_train_masked.py:195-225 hooks)
        reg = getattr(accelerator, "register_for_checkpointing", None)
        if reg is not None:
            reg(model=model, optimizer=optimizer, ema=ema, lr_scheduler=lr_scheduler, scheduler=self.Scheduler)

    # ------------------------------------------------------------------------------------------
    def _batch_images(self, input):
        if "huggingface" in getattr(self.args, "dir_dataset", ""):
            return input["image"]
        return input[0]

    def _step(self, input):
        """ms:139-172.  `accelerator.accumulate` decides whether this micro-step syncs; clip + optimizer update + EMA are one fused
        launch inside the step and run only then.  The LR schedule advances only on a syncing step, and -- like accelerate's
        AcceleratedScheduler, which the reference's `prepare()` at main_train_masked.py:299 wraps it in -- `num_processes`
        times per optimizer step unless `split_batches`: schedules are written in single-process steps."""
        x0 = self._batch_images(input)
        acc = self.accelerator
        with acc.accumulate(self.model):
            sync = getattr(acc, "sync_gradients", True)
            if self.Scheduler.rng_mode == "replay":
                loss = self.step.run_replay(x0, self.timesteps_used_epoch, sync=sync)
            else:
                # (a bound DeviceLoader yields `step.x0` itself: the batch is already there)
                loss = self.step.run_device(None if x0 is self.step.x0 else x0, self.timesteps_used_epoch, sync=sync)
            if sync:
                for _ in range(1 if getattr(acc, "split_batches", False) else max(1, getattr(acc, "num_processes", 1))):
                    self.lr_scheduler.step()
        if sync:                                  # (EMA is folded into the optimizer kernel of the step)
            self.global_step += 1
        self.learning_rate = self.lr_scheduler.get_last_lr()[0]
        self.lr_list.append(self.learning_rate)
        self.reconstruct_loss = loss
        return loss

    def _set_monitors(self, row):
        """ms:175-179: the five attributes of `loss_names`, as Python floats, from one ring row."""
        for name, v in zip(MonitorRing.COLUMNS[:5], row[:5]):
            setattr(self, name, float(v))
        if row[6] != 0:                            # a partial sum was not representable and is missing from some mean: say so
            for name in MonitorRing.COLUMNS[1:5]:
                setattr(self, name, float("nan"))

    def _monitored(self, columns):
        """What `_run_batch` returns under `monitor`: ring columns of the step just issued -- read now (one 32-byte copy: the
        step's one sync, like ms:193), or as handles under `defer_loss` (no sync)."""
        ring = self.step.mon
        if self.defer_loss:
            return [DeferredLoss(ring, ring.issued - 1, c) for c in columns]
        row = ring.last()
        self._set_monitors(row)
        return [float(row[c]) for c in columns]

    def _run_batch(self, batch, input, epoch, epoch_length, resume_step, dirs, visualizer):
        loss = self._step(input)
        s = self.step
        self.input, self.degraded_img, self.degrade_binary_masks = s.x0, s.x_t, s.mask
        self.shift, self.shifted_degrade_img = s.s, s.x_in
        if self.monitor:
            return self._monitored((0,))[0]
        self.train_loss = loss.item()              # the reference syncs here too (ms:175, 193)
        return self.train_loss

    def _deferred_rows(self, epoch, epoch_length, resume_step, dirs, visualizer):
        """The batch loop of an epoch under `defer_loss`: every step is issued without a host sync and the ring is read once at the
        end -- or every `monitor_cap` steps when the dataloader is longer than the ring.  -> the epoch's rows [n, 8]."""
        import numpy as np
        ring = self.step.mon
        ring.read()                                # rows of earlier steps (direct `_run_batch` calls) are read here and left out:
        chunks, pending = [], 0                    # they are not this epoch's -- one sync per epoch, before its first step

        def drain():
            rows, dropped = ring.read()
            if dropped:
                raise RuntimeError(f"monitor ring overran: {dropped} rows were overwritten before they were read (monitor_cap={ring.cap})")
            chunks.append(rows)
        for i, input in enumerate(self.dataloader, 0):
            self._mark_end_of_dataloader(i)
            self._run_batch(i, input, epoch, epoch_length, resume_step, dirs, visualizer)
            pending += 1
            if pending == ring.cap:
                drain()
                pending = 0
        drain()
        rows = np.concatenate(chunks)
        if len(rows):
            self._set_monitors(rows[-1])
        return rows

    def _run_epoch(self, epoch, epoch_length, resume_step, dirs, visualizer):
        loss_batch = []
        self.timesteps_used_epoch = self.Scheduler.get_timesteps_epoch(epoch, epoch_length)
        if self.defer_loss:
            rows = self._deferred_rows(epoch, epoch_length, resume_step, dirs, visualizer)
            return [float(v) for v in rows[:, 0]] if self.accelerator.is_main_process else loss_batch
        for i, input in enumerate(self.dataloader, 0):
            self._mark_end_of_dataloader(i)
            loss = self._run_batch(i, input, epoch, epoch_length, resume_step, dirs, visualizer)
            if self.accelerator.is_main_process:
                loss_batch.append(loss)
        return loss_batch

    def _make_visual_tensors(self):
        """The visual tensors of ms:58 that the step does not keep, from what the last step left: `mask` (ms:140),
        `reconstructed_img` (ms:142) and `inverse_shift_reconstructed_img` (ms:145) are the three outputs of ONE mdm_sampler_x0
        launch on the net's output, `step.x_in` and `step.s`; `degradation_mask` / `mean_pixel` are the expressions of
        `Scheduler.degrade_training` (scheduler.py:320-321) on `step.mask` / `step.mean_pixel`.  With 'non_shift' (and in the
        base trainer) `step.s` is never written and is the zero tensor upstream's shift is.  No host sync."""
        from ._lib import call, ptr, stream
        s, m = self.step, self.model
        if not hasattr(self, "input"):
            raise RuntimeError("get_current_visuals: no step has run yet")
        self.degradation_mask, self.mean_pixel = Scheduler.degradation_visuals(s.mask, s.mean_pixel)
        self.shift = s.s
        self.mask, self.reconstructed_img, self.inverse_shift_reconstructed_img = (torch.empty_like(s.x0) for _ in range(3))
        call("mdm_sampler_x0", dtype=m.dt, pred_nhwc=ptr(m.y_out.data), Cp=m.cout_p, x_in=ptr(s.x_in), s=ptr(s.s), N=m.N, C=m.cin,
             H=m.H, W=m.W, pred_nchw=ptr(self.mask), shifted0=ptr(self.reconstructed_img),
             x0_hat=ptr(self.inverse_shift_reconstructed_img), stream=stream())

    def get_current_visuals(self, epoch):
        """ms:301-318: for every name of `train_visual_names` its batch as a grid, normalised over the batch ('_normalize_global')
        and per image ('_normalize_local'), then the `sample_visual_names` as `_save_ema_momentum_sample` left them -> OrderedDict
        of fp32 [Cg, Hg, Wg] device tensors."""
        self._make_visual_tensors()
        ret = OrderedDict()
        for name in self.train_visual_names:
            img = getattr(self, name)
            ret[name + "_normalize_global"] = self.Sampler._save_image_grid(img, normalization="global")
            ret[name + "_normalize_local"] = self.Sampler._save_image_grid(img, normalization="image")
        for name in self.sample_visual_names:
            ret[name] = getattr(self, name)
        return ret

    def get_current_losses(self):
        """ms:321-327."""
        return OrderedDict((name, float(getattr(self, name))) for name in self.loss_names if isinstance(name, str))

    def get_current_mean(self):
        """ms:329-334.  As upstream, `ema_sample_mean` exists once `_save_ema_momentum_sample` has run."""
        return OrderedDict((name, float(getattr(self, name))) for name in self.mean_names if isinstance(name, str))

    def _mark_end_of_dataloader(self, i):
        """accelerate's prepared dataloader flags its last batch, and `accumulate` syncs there whatever the micro-step
        count is (Accelerator._do_sync); ours is told by the loop."""
        n = len(self.dataloader) if hasattr(self.dataloader, "__len__") else None
        if hasattr(self.accelerator, "end_of_dataloader"):
            self.accelerator.end_of_dataloader = n is not None and i == n - 1

    def _epoch_losses(self, r):
        return r

    def train(self, epoch_start, epoch_length, resume_step, global_step, dirs, visualizer):
        a = self.args
        a.updated_ddpm_num_steps = self.Scheduler.update_ddpm_num_steps(a.ddpm_num_steps)
        self.global_step = global_step
        loss_mean_epoch = []
        self.model.train()
        show = self.visuals and visualizer is not None and self.accelerator.is_main_process
        for epoch in range(epoch_start, epoch_start + epoch_length):
            if show:
                visualizer.reset()                                                                   # ms:235-236
            loss = self._epoch_losses(self._run_epoch(epoch, epoch_length, resume_step, dirs, visualizer))
            if self.accelerator.is_main_process:
                loss_mean_epoch.append(statistics.mean(loss))
                if self.monitor and visualizer is not None:
                    visualizer.plot_current_losses(epoch, self.get_current_losses(), 'value')        # ms:249-250
            last = epoch == (epoch_start + epoch_length - 1)
            if (epoch > 0 and (epoch + 1) % a.save_images_epochs == 0) or last or \
                    (epoch + 1) % (epoch_length / a.scheduler_num_scale_timesteps) == 0:      # ms:252
                # Upstream does this block on the main process only (ms:244).  Here EVERY rank enters it: the
                # reverse sampler shards `sample_num` over the ranks and save_state ends in a barrier;
                # files are still written by the main process alone.
                if getattr(a, "use_ema", False) and getattr(a, "sampling", "momentum") == "momentum":
                    self._save_ema_momentum_sample(dirs, epoch)
                if show:
                    visualizer.display_current_results(epoch, self.get_current_visuals(epoch))       # ms:263-264
                save_path = os.path.join(dirs.list_dir["checkpoint"], f"checkpoint-epoch-{epoch}")
                self.accelerator.save_state(save_path)                                           # ms:267-268
        self.loss_mean_epoch = loss_mean_epoch

    def _save_ema_momentum_sample(self, dirs, epoch):
        """ms:409-425 -- sample with the EMA weights, then put the training weights back."""
        a = self.args
        self.ema_model.store(None)
        self.ema_model.copy_to(None)
        # this rank's share of sample_num, on the sampler of record (fp32 storage, split products) unless args.sample_precision says
        # otherwise: a bf16 model's own plan is 1e-2 away from the reference sampler after 100 steps
        net = self.model.sampling_plan(self.Sampler.local_sample_num(), getattr(a, "sample_precision", "f32_split")).eval()
        sample_0, _hist = self.Sampler.sample(net, self.timesteps_used_epoch)    # gathered: [sample_num, C, H, W] on every rank
        self.ema_model.restore(None)
        self.model.train()
        self.ema_sample = sample_0
        self.ema_sample_mean = sample_0.mean()                                   # ms:421
        if self.accelerator.is_main_process:
            torch.save(sample_0.cpu(), os.path.join(dirs.list_dir["ema_sample_img"], f"ema_sample_{epoch:05d}.pt"))
        if self.visuals:                                                         # ms:423-425; the PNG is the global grid
            png = (dirs.list_dir["ema_sample_img"], f"ema_sample_{epoch:05d}.png") if self.accelerator.is_main_process else (None, None)
            self.ema_sample_result_normalize_global = self.Sampler._save_image_grid(sample_0, "global", *png)
            self.ema_sample_result_normalize_local = self.Sampler._save_image_grid(sample_0, "image")
        return sample_0


class BaseTrainer(Trainer):
    """trainer_masked.py surface: no dataset_hist argument, `_run_batch` -> (loss, recon_mean, degraded_mean)."""
    mean_shift = False

    def __init__(self, args, dataloader, dataset, model, ema_model, optimizer, lr_scheduler, accelerator):
        super().__init__(args, dataloader, dataset, [None] * 3, model, ema_model, optimizer, lr_scheduler, accelerator)
        self.train_visual_names = ["input", "degraded_img", "degradation_mask", "mask", "mean_pixel", "degrade_binary_masks",
                                   "reconstructed_img"]                                                              # base:58

    def _run_batch(self, batch, input, epoch, epoch_length, resume_step, dirs, visualizer):
        loss = self._step(input)
        s = self.step
        self.input, self.degraded_img, self.degrade_binary_masks = s.x0, s.x_t, s.mask
        if self.monitor:
            # base:161-162 from the ring: mean(x_t + pred) and mean(x_t) are the reconstruction and degraded columns (no shift:
            # x_in is x_t).  No layout kernel, no torch arithmetic, one sync; `mask` / `reconstructed_img` are not materialised.
            return tuple(self._monitored((0, 2, 4)))
        pred = torch.empty_like(s.x0)
        from . import ops
        m = self.model
        ops.nhwc_to_nchw(m.dt, m.y_out.data, pred, m.N, m.cout, m.H, m.W, m.cout_p)
        self.mask = pred
        self.reconstructed_img = s.x_t + pred                                               # base:126
        self.train_loss = loss.item()
        return self.train_loss, self.reconstructed_img.mean().item(), s.x_t.mean().item()   # base:183

    def _run_epoch(self, epoch, epoch_length, resume_step, dirs, visualizer):
        out = ([], [], [])
        self.timesteps_used_epoch = self.Scheduler.get_timesteps_epoch(epoch, epoch_length)
        if self.defer_loss:
            rows = self._deferred_rows(epoch, epoch_length, resume_step, dirs, visualizer)
            return tuple([float(v) for v in rows[:, c]] for c in (0, 2, 4)) if self.accelerator.is_main_process else out
        for i, input in enumerate(self.dataloader, 0):
            self._mark_end_of_dataloader(i)
            r = self._run_batch(i, input, epoch, epoch_length, resume_step, dirs, visualizer)
            if self.accelerator.is_main_process:
                for lst, v in zip(out, r):
                    lst.append(v)
        return out

    def _epoch_losses(self, r):
        return r[0]
