"""Reverse (cold-diffusion) sampler on the GPU -- same surface as the reference `Sampler`.

Mirrors reference code/sampler.py: `_get_latent_initial` (:46-83), `sample` (:102-106),
`_get_latent_initial_interpolation` (:86-99) with `_sample_interpolation` (:264-366, public here as
`sample_interpolation`: nothing calls it upstream) and
`_sample_mean_shift_momentum` (:109-261) for the options that run upstream at HEAD
(`sampling_mask_dependency` in {independent, dependent_prev, dependent_t -- the last for
'thresholding' with mean_option 'degraded_area' or "0", scheduler.py:480-549}, `momentum_adaptive`
in {base_sampling, base_momentum}).  `sample_inpaint` has no upstream counterpart: the same
loop with every prediction projected onto the given pixels (include/mdm_inpaint.h).  Nor has `sample_restore`: the
projection is onto given block means instead -- super-resolution and colourisation (include/mdm_restore.h).

What is different from the reference loop (same arithmetic, same RNG order in replay mode):
  * the whole state stays on the GPU; nothing is copied to the host inside the loop.  The
    reference's 11 history tensors are optional (`args.sample_history`: True -> returned on
    the CPU like the reference, "device" -> kept in HBM, False -> skipped, empty list);
  * per step: one fused shift+perturb kernel, the U-Net forward plan, one fused
    x0-reconstruction kernel, two degrade kernels and one update kernel.
"""
from __future__ import annotations

import functools
import os
import types

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, ptr, stream

HISTORY_NAMES = ["sample_t", "shift", "shifted", "mask", "shifted_result", "sample_0",
                 "degraded_mask", "degraded_mask_next", "degraded_t", "difference", "degraded_next_t"]
# the ten lists of the interpolation sampler (sampler.py:366): one mask per step, shared by the batch
INTERP_HISTORY_NAMES = [k for k in HISTORY_NAMES if k != "degraded_mask_next"]


def shard_bounds(n, rank, world):
    """[lo, hi) of rank's share when n independent samples are dealt to `world` ranks (the first n % world ranks
    take one more).  Samples are independent (sampler.py:137-258), so the split needs no collective."""
    base, rem = divmod(int(n), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_shards(local, n, group=None):
    """All-gather of uneven shards along dim 0 -> the full [n, ...] tensor on every rank (the ONE collective of a
    sharded sampling run, after the loop).  Works on any backend: shards are padded to the largest one."""
    import torch.distributed as dist
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    sizes = [shard_bounds(n, r, world)[1] - shard_bounds(n, r, world)[0] for r in range(world)]
    big = max(sizes)
    pad = torch.zeros((big,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[:local.shape[0]] = local
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([p[:k] for p, k in zip(parts, sizes)], 0)


def inpaint_start_index(ratio_list, timesteps, unknown_fraction):
    """Where a 'matched' inpainting run begins: the first j with ratio_list[timesteps[j] - 1] >= unknown_fraction (the schedule at
    that timestep hides at least as much as the hole does), len(timesteps) - 1 if no used timestep reaches it.  The reverse loop
    then walks timesteps[:j + 1] from its end.  Pure host arithmetic in fp64."""
    frac = float(unknown_fraction)
    for j, t in enumerate(timesteps):
        if float(ratio_list[int(t) - 1]) >= frac:
            return j
    return len(timesteps) - 1


def inpaint_keep(kind, N, H, W, **kw):
    """A keep mask [N, 1, H, W] fp32 on the host, 1 = given, 0 = not given.  kind "box": the rectangle `top, left, height, width`
    is not given; "half": the `side` ('left', 'right', 'top', 'bottom') half is not given; "random": each pixel is not given with
    probability `p`, drawn as torch.rand(N, 1, H, W, generator=generator) < p."""
    keep = torch.ones(N, 1, H, W)
    def take(*names):
        extra = set(kw) - set(names)
        if extra or len(kw) != len(names):
            raise TypeError(f"inpaint_keep({kind!r}): takes {', '.join(names)}, got {', '.join(sorted(kw)) or 'nothing'}")
        return [kw[k] for k in names]
    if kind == "box":
        top, left, height, width = take("top", "left", "height", "width")
        if not (0 <= top and 0 <= left and height >= 0 and width >= 0 and top + height <= H and left + width <= W):
            raise ValueError(f"inpaint_keep('box'): {(top, left, height, width)} does not lie inside {H} x {W}")
        keep[:, :, top:top + height, left:left + width] = 0
    elif kind == "half":
        side, = take("side")
        if side not in ("left", "right", "top", "bottom"):
            raise ValueError(f"inpaint_keep('half'): side={side!r}: one of 'left', 'right', 'top', 'bottom'")
        if side in ("left", "right"):
            keep[..., :W // 2] = 0
            if side == "right":
                keep = keep.flip(-1)
        else:
            keep[:, :, :H // 2] = 0
            if side == "bottom":
                keep = keep.flip(-2)
    elif kind == "random":
        p, generator = take("p", "generator")
        keep[torch.rand(N, 1, H, W, generator=generator) < p] = 0
    else:
        raise ValueError(f"inpaint_keep: kind={kind!r}: one of 'box', 'half', 'random'")
    return keep.contiguous()


def _check_restore_groups(pool, gray, channels):
    """the group description of include/mdm_restore.h: -> (k, gray as int), or the error that names the argument"""
    if isinstance(pool, bool) or not isinstance(pool, int) or pool not in (1, 2, 4, 8):
        raise ValueError(f"pool={pool!r}: one of 1, 2, 4, 8")
    if not isinstance(gray, (bool, int)) or gray not in (0, 1):
        raise ValueError(f"gray={gray!r}: True or False")
    if pool * pool * (channels if gray else 1) == 1:
        raise ValueError(f"pool=1 with {'gray on one channel' if gray else 'gray=False'}: groups of one element constrain nothing")
    return pool, int(gray)


def _check_restore_tensor(name, t, dev=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch.Tensor is needed, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: dtype {t.dtype}, float32 is needed")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name}: on {t.device}, the sampler runs on {dev}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if t.dim() != 4:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, four dimensions are needed")


def restore_measure(x, pool, gray=False):
    """The measurement of a batch on the device (`mdm_restore_measure`): x [N, C, H, W] fp32 -> y [N, 1 if gray else C, H / pool,
    W / pool], the mean of every pool x pool block (over the channels too with `gray`), summed in the order mdm_restore.h states."""
    _check_restore_tensor("x", x)
    n, c, h, w = x.shape
    k, g = _check_restore_groups(pool, gray, c)
    if h % k or w % k:
        raise ValueError(f"x: shape {tuple(x.shape)}, H and W must be multiples of pool={k}")
    if c > 8:
        raise ValueError(f"x: shape {tuple(x.shape)}, at most 8 channels")
    y = torch.empty(n, 1 if g else c, h // k, w // k, dtype=torch.float32, device=x.device)
    call("mdm_restore_measure", x=ptr(x), k=k, gray=g, N=n, C=c, H=h, W=w, y=ptr(y), stream=stream())
    return y


def restore_expand(y, channels, pool, gray=False):
    """A measurement broadcast over its groups on the device (`mdm_restore_start`): y [N, 1 if gray else channels, h, w] ->
    [N, channels, h pool, w pool], nearest upsampling with the grey value copied to every channel.  The trivial completion that
    has the measurement (its block means are y to rounding) and the one any quality number is to be read against."""
    _check_restore_tensor("y", y)
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= 8:
        raise ValueError(f"channels={channels!r}: an int from 1 to 8")
    k, g = _check_restore_groups(pool, gray, channels)
    n, cy, h, w = y.shape
    if cy != (1 if g else channels):
        raise ValueError(f"y: shape {tuple(y.shape)}, {1 if g else channels} channel(s) are needed for channels={channels}, gray={bool(g)}")
    out = torch.empty(n, channels, h * k, w * k, dtype=torch.float32, device=y.device)
    call("mdm_restore_start", y=ptr(y), k=k, gray=g, per_channel=0, N=n, C=channels, H=h * k, W=w * k, mu=None, expand=ptr(out),
         stream=stream())
    return out


class Sampler:
    def __init__(self, dataset, args, Scheduler, dataset_hist):
        self.dataset, self.args, self.Scheduler, self.dataset_hist = dataset, args, Scheduler, dataset_hist
        # Optional observer `f(i, slot, x_t)` called at the top of every reverse step of the host-driven loop; it may
        # overwrite x_t in place.  The parity tests use it for TEACHER FORCING (x_t <- the oracle's x_t of that step): an
        # untrained U-Net iterated 1000 times is a chaotic map -- the reference's own fp32 run is O(1) away from its fp64
        # run by then -- so a long free-running comparison measures conditioning; the per-step one measures the kernels.
        self.step_hook = None

    # ---- multi-GPU: `sample_num` is partitioned over the ranks of the default process group ----------------
    def _shard(self):
        """(rank, world) when sharded sampling applies, else (0, 1).  Off with `args.shard_sampling=False`."""
        import torch.distributed as dist
        if not getattr(self.args, "shard_sampling", True) or not (dist.is_available() and dist.is_initialized()):
            return 0, 1
        return dist.get_rank(), dist.get_world_size()

    def local_sample_num(self):
        rank, world = self._shard()
        lo, hi = shard_bounds(self.args.sample_num, rank, world)
        return hi - lo

    def _get_latent_initial(self, model=None):
        """Constant-colour start image per sample, drawn on the host like sampler.py:46-83.  Sharded sampling: drawn for the
        FULL sample_num on every rank (all ranks are seeded alike, main_train_masked.py:441-445) and sliced to this rank's rows
        by the caller -- a rank drawing only its own share would start from the same colours as every other rank."""
        a = self.args
        if a.mean_area == "image-wise":
            d = 1
        elif a.mean_area == "channel-wise":
            d = 3
        else:
            raise UnboundLocalError("mean_area")
        shape = a.sample_latent_shape.lower()
        if shape == "data":
            hshape, edges, cum = self.dataset_hist
            idx = torch.searchsorted(cum, torch.rand(a.sample_num))
            idx = np.unravel_index(idx, hshape)
            mean = torch.empty(a.sample_num, 0)
            for c in range(d):
                r = torch.rand(a.sample_num)
                lo, hi = edges[c][idx[c]], edges[c][idx[c] + 1]
                mean = torch.cat((mean, ((hi - lo) * r + lo).unsqueeze(-1)), 1)
        elif shape == "zero":
            mean = torch.zeros(a.sample_num, d)
        elif shape == "normal":
            mean = torch.randn(a.sample_num, d)
        elif shape == "uniform":
            mean = torch.empty(a.sample_num, d).uniform_(-1, 1)
        else:
            raise IndexError(f"sample_latent_shape={shape!r} does not run upstream")
        return mean[:, :, None, None].expand(a.sample_num, a.out_channel, a.data_size, a.data_size)

    def sample(self, model, timesteps_used_epoch, interpolation_shift=None):
        """sampler.py:102-106.  With a process group of W ranks every rank runs the loop on its own
        `local_sample_num()` samples (`model` must be built for that batch; per-rank Philox key, see
        Scheduler) and the shards are all-gathered once at the end: every rank returns [sample_num, C, H, W]."""
        rank, world = self._shard()
        if world == 1:
            return self._sample_mean_shift_momentum(model, timesteps_used_epoch)
        import argparse
        full = self.args
        n = full.sample_num
        lo, hi = shard_bounds(n, rank, world)
        try:
            if hi == lo:
                raise ValueError(f"sample_num={n} < world size {world}: a rank would sample nothing")
            latent = self._get_latent_initial(model)[lo:hi]           # the full draw, this rank's rows
            self.args = argparse.Namespace(**vars(full))
            self.args.sample_num = hi - lo
            self.Scheduler.replay_rows = (lo, hi, n)                  # every later host draw: full batch, sliced (replay mode)
            x0, hist = self._sample_mean_shift_momentum(model, timesteps_used_epoch, latent=latent)
        finally:
            self.args = full
            self.Scheduler.replay_rows = None
        def gather_hist(h):             # [T+1, n_local, C, H, W], on the host when args.sample_history is True
            g = gather_shards(h.to(x0.device).transpose(0, 1).contiguous(), n).transpose(0, 1)
            return g if h.is_cuda else g.cpu()
        return gather_shards(x0, n), [gather_hist(h) for h in hist]

    # ---- set-level quality (no upstream counterpart; include/mdm_moment.h, DESIGN.md finding 73) -----------------
    def evaluate_frechet(self, model, timesteps_used_epoch, rounds=1, features="pixels", reference=None):
        """Run `sample` `rounds` times -- the draws of that many successive `sample` calls from the host generator and the device
        Philox state, both left where those calls leave them -- fold every round's `sample_0` into one `mdm.moments.SetMoments` on
        the device (no image is kept) and return `mdm.moments.frechet_distance(samples, reference)`, a FrechetResult.
          features "pixels": a row is a raw image at full resolution, d = C H W; the default `reference` is the data set's own pixel
                             moments, read in place (uint8 through its table) once and kept on the data set object;
                   "bank":   a row is a row of the 32 x 32 `NeighborBank` of `get_nearest_neighbor`, the samples put through the
                             bank's own map (`NeighborBank.source_moments`); the default `reference` is `bank.moments()`.
          reference: a `SetMoments` of the same d, e.g. `SetMoments.load` of a stats file, or None.
        A pixel-space (or bank-space) Frechet distance, NOT FID.  rounds x sample_num <= d gives a rank-deficient sample covariance:
        the number is defined and biased upward (`rank_deficient`).  Under sharded sampling every rank holds the gathered batch and
        folds all of it, so every rank returns the same bits."""
        from . import evaluate, moments
        if features not in ("pixels", "bank"):
            raise ValueError(f"features={features!r}: 'pixels' or 'bank'")
        if isinstance(rounds, bool) or not isinstance(rounds, int) or rounds < 1:
            raise ValueError(f"rounds={rounds!r}: a positive int")
        if reference is not None and not isinstance(reference, moments.SetMoments):
            raise TypeError(f"reference: a SetMoments or None is needed, not {type(reference).__name__}")
        bank = None
        if features == "bank":
            antialias = bool(getattr(self, "nn_antialias", getattr(self.args, "nn_antialias", True)))
            bank = getattr(self, "_nn_bank", None)
            if bank is None or bank.antialias != antialias:
                bank = self._nn_bank = evaluate.NeighborBank(self.dataset, size=32, antialias=antialias)
        if reference is None:
            reference = bank.moments() if bank is not None else moments.dataset_moments(self.dataset)
        acc = None
        for _ in range(rounds):
            x0, _hist = self.sample(model, timesteps_used_epoch)
            if bank is not None:
                acc = bank.source_moments(x0, into=acc)
            else:
                if acc is None:
                    acc = moments.SetMoments(x0[0].numel(), x0.device)
                acc.update(x0)
        return moments.frechet_distance(acc, reference)

    # ---- inpainting (no upstream counterpart; include/mdm_inpaint.h, DESIGN.md finding 70) ----------------------
    def sample_inpaint(self, model, timesteps_used_epoch, known, keep, start="latent"):
        """Complete partly given images: -> (sample_0, history lists) like `sample`.  `known` [sample_num, C, H, W] fp32 on the
        device, in the data range; `keep` [sample_num, 1 or C, H, W] fp32 on the device, a pixel is GIVEN where keep != 0.

        Every reverse step runs as `sample` runs it, then its prediction is projected onto the data -- x0_hat = keep != 0 ? known :
        x0_hat, a select -- and the degrades, fill means, mask dependencies and momentum modes go on from the projected x0_hat.
        Given pixels are hidden and revealed by the schedule like any others and come out bit-equal to `known`.  `start`:
          "latent"      `_get_latent_initial`, the host draws of `sample`;
          "known_mean"  a constant image per sample, the mean of its given values (per channel for mean_area 'channel-wise'); an
                        image with nothing given takes its row of the "latent" draw, which is made either way;
          "matched"     keep ? known : mean, and the loop begins at the first used timestep whose ratio reaches the largest
                        unknown fraction of the batch (`inpaint_start_index`; one host read before the loop).  Fewer steps for
                        small holes.  Measured on the trained 16 x 16 fixture net over 64 held-out images
                        (`evaluate_inpaint`; DESIGN.md finding 71): 250 to 602 of 1000 steps for a quarter box, a half and a 50 %
                        random hole, hole PSNR and SSIM within 0.04 dB / 0.008 of the full "latent" run, far inside the 2 dB
                        spread over images -- on that fixture the shorter run costs nothing that can be seen.
        With a process group every rank gets the full `known` / `keep`, runs its rows (`model` built for `local_sample_num()`) and
        the shards are all-gathered at the end; the start index of "matched" comes from the full batch on every rank."""
        rank, world = self._shard()
        if world == 1:
            return self._sample_inpaint(model, timesteps_used_epoch, known, keep, start)
        n = self.args.sample_num
        lo, hi = shard_bounds(n, rank, world)
        if hi == lo:
            raise ValueError(f"sample_num={n} < world size {world}: a rank would sample nothing")
        x0, hist = self._sample_inpaint(model, timesteps_used_epoch, known, keep, start, rows=(lo, hi))
        def gather_hist(h):             # [T+1, n_local, C, H, W], on the host when args.sample_history is True
            g = gather_shards(h.to(x0.device).transpose(0, 1).contiguous(), n).transpose(0, 1)
            return g if h.is_cuda else g.cpu()
        return gather_shards(x0, n), [gather_hist(h) for h in hist]

    def evaluate_inpaint(self, model, timesteps_used_epoch, truth, keep, starts=("latent", "known_mean", "matched"), trajectory=False):
        """Complete `truth` under `keep` with every start of `starts` and measure the completions against `truth` on the device
        (mdm.image_metrics: MSE, PSNR, SSIM, whole-image and hole-only): -> {start: ImageMetrics}, device tensors of shape
        [sample_num], nothing read to the host.  Every start runs `sample_inpaint(..., known=truth, keep=keep, start=s)` from the
        host generator state and the device Philox state found at the call, so the runs differ by their start and not by their
        draws; both states are put back at the end.  `self.inpaint_steps_run[s]` is the number of reverse steps start s walked.
        `trajectory=True` (needs args.sample_history == "device"): the `sample_0` history list is measured in place instead and
        the tensors are [T_run + 1, sample_num] -- row k is the prediction after k steps (row 0: the empty slot 0 of the list, an
        all-zero image), the last row is `sample_0` itself."""
        from .metrics import image_metrics
        S = self.Scheduler
        if trajectory and getattr(self.args, "sample_history", True) != "device":
            raise ValueError("trajectory=True measures the history where it lies: args.sample_history == 'device' is needed")
        host_state, dev_state = torch.get_rng_state(), S.dev_rng.dev.clone()
        out, steps_run = {}, {}
        try:
            for s in starts:
                torch.set_rng_state(host_state)
                S.dev_rng.dev.copy_(dev_state)
                x0, hist = self.sample_inpaint(model, timesteps_used_epoch, truth, keep, start=s)
                steps_run[s] = self._inpaint_steps
                pred = hist[HISTORY_NAMES.index("sample_0")][:steps_run[s] + 1] if trajectory else x0
                out[s] = image_metrics(pred, truth, keep)
        finally:
            torch.set_rng_state(host_state)
            S.dev_rng.dev.copy_(dev_state)
        self.inpaint_steps_run = steps_run
        return out

    def _check_inpaint_args(self, known, keep, start):
        a, dev = self.args, self.Scheduler.device
        if start not in ("latent", "known_mean", "matched"):
            raise ValueError(f"start={start!r}: one of 'latent', 'known_mean', 'matched'")
        want = (a.sample_num, a.out_channel, a.data_size, a.data_size)
        for name, t in (("known", known), ("keep", keep)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name}: a torch.Tensor is needed, not {type(t).__name__}")
            if t.dtype != torch.float32:
                raise TypeError(f"{name}: dtype {t.dtype}, float32 is needed")
            if t.device != dev:
                raise ValueError(f"{name}: on {t.device}, the sampler runs on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"{name}: not contiguous")
        if tuple(known.shape) != want:
            raise ValueError(f"known: shape {tuple(known.shape)}, (sample_num, C, H, W) = {want} is needed")
        if keep.dim() != 4 or (keep.shape[0], *keep.shape[2:]) != (want[0], *want[2:]) or keep.shape[1] not in (1, want[1]):
            raise ValueError(f"keep: shape {tuple(keep.shape)}, {(want[0], 1, *want[2:])} or {want} is needed")

    def _sample_inpaint(self, model, timesteps, known, keep, start="latent", rows=None):
        """`sample_inpaint` on rows [lo, hi) of the batch (`rows`; all of it by default): `known` / `keep` and every host draw are
        the full batch's, `model` is built for hi - lo samples."""
        import argparse
        self._check_inpaint_args(known, keep, start)
        full, S = self.args, self.Scheduler
        n, c, hw = full.sample_num, full.out_channel, full.data_size
        lo, hi = rows if rows is not None else (0, n)
        steps = list(timesteps)
        latent = self._get_latent_initial(model)                      # the full draw in every start: the host generator moves as in `sample`
        x_t = latent[lo:hi]
        if start != "latent":
            fallback = latent[:, :, 0, 0].to(S.device, torch.float32).contiguous()
            x_start = torch.empty_like(known) if start == "matched" else None
            mu = torch.empty(n, c, device=S.device) if start == "known_mean" else None
            unknown = torch.empty(n, dtype=torch.int32, device=S.device) if start == "matched" else None
            call("mdm_inpaint_start", known=ptr(known), keep=ptr(keep), keep_C=keep.shape[1], fallback=ptr(fallback),
                 per_channel=int(full.mean_area == "channel-wise"), N=n, C=c, HW=hw * hw, x_start=ptr(x_start), mu=ptr(mu),
                 unknown=ptr(unknown), stream=stream())
            if start == "matched":      # the ONE host read: the largest hole of the FULL batch, so every shard walks the same steps
                j = inpaint_start_index(S.ratio_list, steps, int(unknown.max()) / float(hw * hw))
                steps, x_t = steps[:j + 1], x_start[lo:hi]
            else:
                x_t = mu[lo:hi, :, None, None].expand(hi - lo, c, hw, hw)
        inpaint = (known[lo:hi], keep[lo:hi])                         # leading-dimension slices: contiguous views
        self._inpaint_steps = len(steps)                              # what `evaluate_inpaint` reports per start
        if rows is None:
            return self._sample_mean_shift_momentum(model, steps, latent=x_t, inpaint=inpaint, hist_steps=len(timesteps))
        try:
            self.args = argparse.Namespace(**vars(full))
            self.args.sample_num = hi - lo
            S.replay_rows = (lo, hi, n)                               # every later host draw: full batch, sliced (replay mode)
            return self._sample_mean_shift_momentum(model, steps, latent=x_t, inpaint=inpaint, hist_steps=len(timesteps))
        finally:
            self.args = full
            S.replay_rows = None

    # ---- restoration: super-resolution and colourisation (no upstream counterpart; include/mdm_restore.h) ------
    def sample_restore(self, model, timesteps_used_epoch, measurement, pool, gray=False, start="latent"):
        """Complete images of which only block means are given: -> (sample_0, history lists) like `sample_inpaint`.
        `measurement` [sample_num, 1 if gray else C, H / pool, W / pool] fp32 on the device (`restore_measure` makes one): the mean
        of every pool x pool block, taken over the channels too with `gray` -- a box-downsampled image (pool > 1), a grey one
        (pool 1, gray) or both.

        Every reverse step runs as `sample` runs it, then its prediction is projected orthogonally onto the images that have this
        measurement -- x0_hat += measurement[g] - mean_g(x0_hat) for every group g -- and the degrades, fill means, mask
        dependencies and momentum modes go on from the projected x0_hat.  `start`:
          "latent"    `_get_latent_initial`, the host draws of `sample`;
          "measured"  a constant image per sample, the mean of its measurement (per channel for mean_area 'channel-wise' without
                      `gray`): the colour the loop otherwise draws.  The latent draw is made either way.
        There is no "matched" start: a measurement has no hole fraction that a timestep could be matched to.
        With a process group every rank gets the full `measurement`, runs its rows (`model` built for `local_sample_num()`) and the
        shards are all-gathered at the end."""
        rank, world = self._shard()
        if world == 1:
            return self._sample_restore(model, timesteps_used_epoch, measurement, pool, gray, start)
        n = self.args.sample_num
        lo, hi = shard_bounds(n, rank, world)
        if hi == lo:
            raise ValueError(f"sample_num={n} < world size {world}: a rank would sample nothing")
        x0, hist = self._sample_restore(model, timesteps_used_epoch, measurement, pool, gray, start, rows=(lo, hi))
        def gather_hist(h):             # [T+1, n_local, C, H, W], on the host when args.sample_history is True
            g = gather_shards(h.to(x0.device).transpose(0, 1).contiguous(), n).transpose(0, 1)
            return g if h.is_cuda else g.cpu()
        return gather_shards(x0, n), [gather_hist(h) for h in hist]

    def evaluate_restore(self, model, timesteps_used_epoch, truth, pool, gray=False, starts=("latent", "measured"), trajectory=False):
        """Measure `truth` (`restore_measure`), restore it with every start of `starts` and compare with `truth` on the device
        (mdm.image_metrics, whole-image slots): -> {start: ImageMetrics, "expand": ImageMetrics of `restore_expand(y)`}, device
        tensors of shape [sample_num], nothing read to the host.  Every start runs from the host generator state and the device
        Philox state found at the call; both are put back at the end.  `trajectory=True` (needs args.sample_history == "device"):
        the `sample_0` history list is measured in place and the tensors of the starts are [T + 1, sample_num]."""
        from .metrics import image_metrics
        S = self.Scheduler
        if trajectory and getattr(self.args, "sample_history", True) != "device":
            raise ValueError("trajectory=True measures the history where it lies: args.sample_history == 'device' is needed")
        _check_restore_tensor("truth", truth, S.device)
        y = restore_measure(truth, pool, gray)
        host_state, dev_state = torch.get_rng_state(), S.dev_rng.dev.clone()
        out = {}
        try:
            for s in starts:
                torch.set_rng_state(host_state)
                S.dev_rng.dev.copy_(dev_state)
                x0, hist = self.sample_restore(model, timesteps_used_epoch, y, pool, gray, start=s)
                out[s] = image_metrics(hist[HISTORY_NAMES.index("sample_0")] if trajectory else x0, truth)
        finally:
            torch.set_rng_state(host_state)
            S.dev_rng.dev.copy_(dev_state)
        out["expand"] = image_metrics(restore_expand(y, truth.shape[1], pool, gray), truth)
        return out

    def _check_restore_args(self, measurement, pool, gray, start):
        a, dev = self.args, self.Scheduler.device
        if start not in ("latent", "measured"):
            raise ValueError(f"start={start!r}: one of 'latent', 'measured' (there is no 'matched' start: a measurement has no hole)")
        k, g = _check_restore_groups(pool, gray, a.out_channel)
        if a.data_size % k:
            raise ValueError(f"pool={k}: data_size={a.data_size} is no multiple of it")
        _check_restore_tensor("measurement", measurement, dev)
        want = (a.sample_num, 1 if g else a.out_channel, a.data_size // k, a.data_size // k)
        if tuple(measurement.shape) != want:
            raise ValueError(f"measurement: shape {tuple(measurement.shape)}, (sample_num, 1 if gray else C, H / pool, W / pool) = "
                             f"{want} is needed")
        return k, g

    def _sample_restore(self, model, timesteps, measurement, pool, gray=False, start="latent", rows=None):
        """`sample_restore` on rows [lo, hi) of the batch (`rows`; all of it by default): `measurement` and every host draw are the
        full batch's, `model` is built for hi - lo samples."""
        import argparse
        k, g = self._check_restore_args(measurement, pool, gray, start)
        full, S = self.args, self.Scheduler
        n, c, hw = full.sample_num, full.out_channel, full.data_size
        lo, hi = rows if rows is not None else (0, n)
        latent = self._get_latent_initial(model)                      # the full draw in every start: the host generator moves as in `sample`
        x_t = latent[lo:hi]
        if start == "measured":
            mu = torch.empty(n, c, device=S.device)
            call("mdm_restore_start", y=ptr(measurement), k=k, gray=g, per_channel=int(full.mean_area == "channel-wise"), N=n, C=c,
                 H=hw, W=hw, mu=ptr(mu), expand=None, stream=stream())
            x_t = mu[lo:hi, :, None, None].expand(hi - lo, c, hw, hw)
        restore = (measurement[lo:hi], k, g)                          # a leading-dimension slice: a contiguous view
        if rows is None:
            return self._sample_mean_shift_momentum(model, timesteps, latent=x_t, restore=restore)
        try:
            self.args = argparse.Namespace(**vars(full))
            self.args.sample_num = hi - lo
            S.replay_rows = (lo, hi, n)                               # every later host draw: full batch, sliced (replay mode)
            return self._sample_mean_shift_momentum(model, timesteps, latent=x_t, restore=restore)
        finally:
            self.args = full
            S.replay_rows = None

    # ---- latent interpolation (sampler.py:86-99, 264-366) ------------------------------------------------------
    def _get_latent_initial_interpolation(self, interpolation_shift):
        """sampler.py:86-99 -> (latent [N, C, H, W], grid [N, 1, 1, 1]) on the host: a ramp of constant start colours whose ends
        leave room for the shift -- linspace(-1, 1 - shift) for a positive shift, linspace(-1 - shift, 1) for a negative one."""
        a = self.args
        if interpolation_shift > 0:
            grid = torch.linspace(-1, 1 - interpolation_shift, a.sample_num)
        elif interpolation_shift < 0:
            grid = torch.linspace(-1 - interpolation_shift, 1, a.sample_num)
        else:
            grid = torch.linspace(-1, 1, a.sample_num)
        grid = grid[:, None, None, None]
        return torch.zeros(a.sample_num, a.out_channel, a.data_size, a.data_size) + grid, grid

    def sample_interpolation(self, model, timesteps_used_epoch, interpolation_shift):
        """The latent-interpolation sampler (upstream's `_sample_interpolation`, which nothing calls there): -> (sample_0, mu,
        history lists in INTERP_HISTORY_NAMES order).  With a process group every rank runs its rows of the ramp (`model` built
        for `local_sample_num()`), the ramp and the host draws are made for the full batch on every rank, and the shards are
        all-gathered once at the end: every rank returns what one process computes; `mu` is the full grid."""
        rank, world = self._shard()
        if world == 1:
            return self._sample_interpolation(model, timesteps_used_epoch, interpolation_shift)
        n = self.args.sample_num
        lo, hi = shard_bounds(n, rank, world)
        if hi == lo:
            raise ValueError(f"sample_num={n} < world size {world}: a rank would sample nothing")
        x0, mu, hist = self._sample_interpolation(model, timesteps_used_epoch, interpolation_shift, rows=(lo, hi))
        def gather_hist(h):             # [T+1, n_local, C, H, W], on the host when args.sample_history is True
            g = gather_shards(h.to(x0.device).transpose(0, 1).contiguous(), n).transpose(0, 1)
            return g if h.is_cuda else g.cpu()
        return gather_shards(x0, n), mu, [gather_hist(h) for h in hist]

    def _emit_interp_step(self, b, more, params, forward):
        """One reverse step of the interpolation loop (sampler.py:297-361) over the fixed buffers `b`, launched or recorded: the
        clamped shift, the forward, x0 reconstruction and -- with `more`, every step but the last -- the fill through the mask of
        the step before, the new batch-shared row mask, the fill through it and the momentum write.  `params()` fills b.time /
        ratio / amt_next and bumps the Philox offset, `forward()` runs the net on b.x_in -> (pred NHWC, Cp, dtype), `b.draw_row()`
        is the row's random input in the scheduler's RNG mode."""
        a, S = self.args, self.Scheduler
        n, c, h, w = b.x_t.shape
        params()
        S.emit_shift_interp(b.x_t, b.mu, b.ratio, b.shift, b.s, b.x_in, nhwc=b.nhwc)                                     # :302-303
        pred, cp, pdt = forward()                                                                                      # :305
        call("mdm_sampler_x0", dtype=pdt, pred_nhwc=ptr(pred), Cp=cp, x_in=ptr(b.x_in), s=ptr(b.s), N=n, C=c, H=h, W=w,
             pred_nchw=ptr(b.pred_nchw), shifted0=ptr(b.shifted0), x0_hat=ptr(b.x0_hat), stream=stream())              # :306-307
        if not more:
            return
        S.emit_degrade(b.x0_hat, b.d_t, b.mp, rng_stream=0, mean_option=a.mean_option, mean_area=a.mean_area, mask_in=b.m_next)   # :321
        mo, ma = S._interp_fill(a.mean_option)
        S.emit_row_mask(b.amt_next, b.m_next, u_row=b.draw_row())                                                      # :323
        S.emit_degrade(b.x0_hat, b.d_next, b.mp, rng_stream=0, mean_option=mo, mean_area=ma, mask_in=b.m_next)
        call("mdm_interp_update", d_t=ptr(b.d_t), d_next=ptr(b.d_next), x_t=ptr(b.x_t), diff=ptr(b.diff),
             update=int(a.momentum_adaptive == "base_momentum"), n=b.x_t.numel(), stream=stream())                     # :326-333

    def _sample_interpolation_graph(self, model, timesteps, b):
        """The host-driven loop of `_sample_interpolation` (history off, device RNG) with ONE hipGraph per reverse step, like
        `_sample_graph`: a body graph replayed T - 1 times and a last graph (shift, forward, x0) once; the per-step scalars come
        from `mdm_sampler_step_params`."""
        S = self.Scheduler
        dev, T, n = S.device, len(timesteps), b.x_t.shape[0]
        amount_tab = (S.pixels_dev if b.indexing else S.ratio_dev).to(dev, torch.float64).contiguous()
        ratio_tab = S.ratio_dev.to(dev, torch.float64).contiguous()
        ts_dev = torch.as_tensor([int(t) for t in timesteps], dtype=torch.int32, device=dev)
        ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        amt_t = torch.empty(n, dtype=torch.float64, device=dev)       # the amount at t: the entry point writes it, this loop reads t - 1 only

        def params():
            call("mdm_sampler_step_params", timesteps=ptr(ts_dev), T=T, step_ctr=ptr(ctr), ratio_tab=ptr(ratio_tab),
                 amount_tab=ptr(amount_tab), n=n, time_out=ptr(b.time), ratio_out=ptr(b.ratio), amt_t=ptr(amt_t),
                 amt_next=ptr(b.amt_next), rng=ptr(S.dev_rng.dev), stream=stream())

        def forward():
            _lib._recording.extend(model.forward_plan)
            return model.y_out.data, model.cout_p, model.dt

        graphs = []
        for more in ((True, False) if T > 1 else (False,)):
            with _lib.Recording() as rec:
                self._emit_interp_step(b, more, params, forward)
            graphs.append(_lib.GraphExec(rec))
        for _ in range(T - 1):
            graphs[0].launch()
        graphs[-1].launch()
        self._graph_keep = ((b, ts_dev, ctr, amount_tab, ratio_tab, amt_t), graphs)
        return b.x0_hat

    def _sample_interpolation(self, model, timesteps, interpolation_shift, rows=None):
        """sampler.py:264-366.  `rows = (lo, hi)`: compute rows [lo, hi) of the batch only (a shard of `sample_interpolation`):
        the ramp and every host draw are made for the full batch and sliced, `model` is built for hi - lo samples, the returned
        `mu` stays the full grid."""
        from .unet import UNet
        a, S = self.args, self.Scheduler
        dev, T = S.device, len(timesteps)
        n_full, c, hw = a.sample_num, a.out_channel, a.data_size
        lo, hi = rows if rows is not None else (0, n_full)
        n = hi - lo
        mode = a.momentum_adaptive
        if mode in ("momentum", "boosting"):     # :341, 352 read `momentum` before anything binds it
            raise UnboundLocalError(f"momentum_adaptive={mode!r} does not run upstream (D4)")
        hist_mode = getattr(a, "sample_history", True)
        fused = isinstance(model, UNet)
        if fused and getattr(a, "sampler_uniform_t", True):
            model = model.with_uniform_t()      # every reverse step passes ONE timestep for the whole batch (sampler.py:298-305)
        if fused:
            assert (model.N, model.H, model.W) == (n, hw, hw), "UNet plan was built for another batch/extent"
        latent, mu = self._get_latent_initial_interpolation(interpolation_shift)
        x_t = latent[lo:hi].to(dev, torch.float32).contiguous()
        if S.rng_mode == "replay" and a.sampling_mask_dependency == "dependent":
            for _ in range(n_full):             # :295: drawn for every sample of the batch, never read
                torch.randperm(hw * hw)
        graph = (fused and not hist_mode and S.rng_mode == "device" and model.use_graph and getattr(a, "sampler_graph", True)
                 and self.step_hook is None)
        img = lambda on=True: torch.empty_like(x_t) if on else None
        b = types.SimpleNamespace(
            x_t=x_t, mu=mu[lo:hi].reshape(n).to(dev, torch.float32).contiguous(), shift=float(interpolation_shift),
            indexing=a.select_degrade_pixel == "indexing", nhwc=(model.dt, model.x_in.data, model.cin_p) if fused else None,
            time=model.t_in if graph else torch.empty(n, device=dev), ratio=torch.empty(n, dtype=torch.float64, device=dev),
            amt_next=torch.empty(n, dtype=torch.float64, device=dev), s=img(), x_in=img(), pred_nchw=img(hist_mode),
            shifted0=img(hist_mode), x0_hat=img(), d_t=img(), d_next=img(), m_next=torch.zeros_like(x_t),
            mp=torch.empty(n, c, device=dev), diff=img())
        b.draw_row = (lambda: S.host_uniform_row(hw * hw)) if S.rng_mode == "replay" else (lambda: None)
        if graph:
            return self._sample_interpolation_graph(model, timesteps, b), mu, []
        hist = {k: torch.zeros(T + 1, n, c, hw, hw, device=dev) for k in INTERP_HISTORY_NAMES} if hist_mode else None

        def params(i):                          # what mdm_sampler_step_params does for the graph loop
            S.dev_rng.advance()
            b.time.fill_(float(timesteps[i]))
            torch.index_select(S.ratio_dev, 0, b.time.int() - 1, out=b.ratio)
            if i > 0:
                b.amt_next.copy_(S.get_black_area_num_pixels_time(b.time - 1))          # :317-319
        for i in range(T - 1, -1, -1):
            slot = T - i
            if self.step_hook is not None:
                self.step_hook(i, slot, x_t)
            self._emit_interp_step(b, i > 0, functools.partial(params, i), lambda: self._predict(model, b.x_in, b.time, fused))
            if hist_mode:
                hist["shift"][slot].copy_(b.s); hist["shifted"][slot].copy_(b.x_in); hist["mask"][slot].copy_(b.pred_nchw)
                hist["shifted_result"][slot].copy_(b.shifted0); hist["sample_0"][slot].copy_(b.x0_hat)
                if i > 0:                       # :357-361: sample_t is the UPDATED x_t, degraded_mask the row mask just drawn
                    hist["degraded_next_t"][slot].copy_(b.d_next); hist["degraded_t"][slot].copy_(b.d_t)
                    hist["difference"][slot].copy_(b.diff); hist["sample_t"][slot].copy_(x_t)
                    hist["degraded_mask"][slot].copy_(b.m_next)
        return b.x0_hat, mu, [hist[k] if hist_mode == "device" else hist[k].cpu() for k in INTERP_HISTORY_NAMES] if hist_mode else []

    # ---- image grids (mdm/visuals.py: one range launch + one grid launch each, built on the device) ---------
    def _batch(self, sample):
        """A batch as the grid kernels read it: float32 on the scheduler's device, images contiguous (a strided view stays a view)."""
        x = sample.to(self.Scheduler.device, torch.float32)
        ok = x.dim() == 4 and x[0].is_contiguous() and (x.shape[0] == 1 or x.stride(0) >= x[0].numel())
        return x if ok else x.contiguous()

    def _save_image_grid(self, sample, normalization="global", dir_save=None, file_sample=None):
        """sampler.py:369-387: `nrow = ceil(sqrt(batch))`, normalize01_global ('global') / normalize01 ('image') / nothing (anything
        else, as upstream), make_grid -> the fp32 grid [Cg, Hg, Wg] on the device; with both path parts also the PNG `save_image`
        writes.  An empty batch returns None (upstream's ZeroDivisionError branch)."""
        from . import visuals
        if sample.shape[0] == 0:
            return None
        nrow = int(np.ceil(np.sqrt(sample.shape[0])))
        norm = normalization if normalization in ("global", "image") else None
        if dir_save is None or file_sample is None:
            return visuals.make_grid(self._batch(sample), nrow, norm)
        grid, u8 = visuals.make_grid(self._batch(sample), nrow, norm, out="both")
        visuals.save_png(u8, os.path.join(dir_save, file_sample))
        return grid

    def _save_multi_index_image_grid(self, sample, nrow=None, normalization="global", option=None, time_major=False):
        """sampler.py:390-417: one grid per sample over its time axis -> list of fp32 grids on the device.  `sample` is upstream's
        [N, T', C, H, W], or with `time_major` a history of `sample()` as it lies in memory, [T+1, N, C, H, W]: sample n is then
        read in place, its frames N C H W elements apart, and no transposed copy is made.  'skip_first' drops frame 0."""
        from . import visuals
        if normalization not in ("global", "image", None):
            raise UnboundLocalError(f"sample_i undefined for normalization={normalization!r}")
        frames = sample.to(self.Scheduler.device, torch.float32)
        if not time_major:
            frames = frames.transpose(0, 1)                         # a view: [T', N, C, H, W]
        if option == "skip_first":
            frames = frames[1:]
        if nrow is None:
            nrow = int(np.ceil(np.sqrt(sample.shape[0 if time_major else 1])))      # of T' BEFORE the skip, as upstream
        return [visuals.make_grid(self._batch(frames[:, i]), nrow, normalization) for i in range(frames.shape[1])]

    def _save_image_pair_grid(self, data1, data2, dir_save, file_save):
        """sampler.py:474-484: the two batches interleaved (one device copy), normalize01 per image, `nrow = 2 ceil(sqrt(batch))`,
        written as a PNG; -> the fp32 grid.  Upstream passes the result through `make_grid(normalize=True)` once more: a min-max
        over the whole batch, which after normalize01 runs from 0 to 1 whenever at least one image is not constant -- (v - 0) / 1,
        the identity bit for bit -- so that pass is not built (a batch of constant images is all 0 here and there)."""
        from . import visuals
        d1, d2 = self._batch(data1), self._batch(data2)
        data = torch.stack((d1, d2), 1).reshape(2 * d1.shape[0], *d1.shape[1:])
        nrow = int(np.ceil(np.sqrt(d1.shape[0]))) * 2
        grid, u8 = visuals.make_grid(data, nrow, "image", out="both")
        visuals.save_png(u8, os.path.join(dir_save, file_save))
        return grid

    # ------------------------------------------------------------------------------
    def get_nearest_neighbor(self, source, augment=False, metric="cosine"):
        """sampler.py:487-518: for every source image the data image with the largest cosine similarity, both sides resized to
        32 x 32 (`transforms.Resize([32, 32])`), the data `normalize01`-ed first and the source as it is; `augment`: the score is the
        larger of the similarity and the similarity with the data batch under `RandomHorizontalFlip()` -- the transform sees a batch of
        `source.shape[0]` images as one tensor, so one `torch.rand(1) < 0.5` from the default host generator per batch, in data
        order.  -> `zeros_like(source)` filled with `dataset[idx][0]`.

        Served by an `evaluate.NeighborBank` made once per Sampler (include/mdm_neighbor.h): the data set's 32 x 32 unit rows are
        built on the device from the storage as it is.  `nn_antialias` (an attribute of the Sampler or of args, default True) is the
        `antialias` of the resize: True is what torchvision >= 0.17 does on tensors, False what older releases did after a warning."""
        from . import evaluate
        if metric.lower() != "cosine":
            raise UnboundLocalError("score")              # upstream leaves `score` unset for any other metric
        antialias = bool(getattr(self, "nn_antialias", getattr(self.args, "nn_antialias", True)))
        bank = getattr(self, "_nn_bank", None)
        if bank is None or bank.antialias != antialias:
            bank = self._nn_bank = evaluate.NeighborBank(self.dataset, size=32, antialias=antialias)
        rows = evaluate.neighbor_flip_rows(len(bank.dataset), source.shape[0]) if augment else None
        nearest = torch.zeros_like(source)
        nearest.copy_(bank.nearest(source, rows))
        return nearest

    def _predict(self, model, x_in_nchw, time, fused_nhwc):
        """-> (pred as NHWC tensor, Cp, dtype) ready for mdm_sampler_x0."""
        from .unet import UNet
        if isinstance(model, UNet):
            if not fused_nhwc:      # x_in was not written into the net by the shift kernel
                ops.nchw_to_nhwc(model.dt, x_in_nchw, model.x_in.data, model.N, model.cin, model.H, model.W, model.cin_p)
            model.t_in.copy_(time, non_blocking=True)
            model.run_forward()
            return model.y_out.data, model.cout_p, model.dt
        pred = model(x_in_nchw, time).sample.to(x_in_nchw.device, torch.float32).contiguous()   # any callable model
        n, c, h, w = pred.shape
        cp = (c + 7) // 8 * 8
        nh = torch.empty(n, h, w, cp, device=pred.device)
        ops.nchw_to_nhwc(_lib.F32, pred, nh, n, c, h, w, cp)
        return nh, cp, _lib.F32

    def _emit_step(self, b, update, params, forward):
        """One reverse step (sampler.py:137-216) over the fixed buffers `b`, launched or recorded: shift + perturb, the forward,
        x0 reconstruction, the two degrades, and with `update` the write of x_t.  What the two loops do differently comes in:
        `params()` fills b.time / ratio / amt_t / amt_next and bumps the Philox offset, `forward()` runs the net on b.x_in ->
        (pred NHWC, Cp, dtype); `b.draw_z` / `b.mask_src` (`_draws`) make a launch's random input in the scheduler's RNG mode."""
        a, S = self.args, self.Scheduler
        n, c, h, w = b.x_t.shape
        dep, mask_src = a.sampling_mask_dependency, b.mask_src
        params()
        S.emit_shift(b.x_t, b.s, b.x_in, kind=b.kind, ratio=b.ratio if b.kind != 0 else None, z=b.draw_z(), nhwc=b.nhwc)  # :142-143
        pred, cp, pdt = forward()                                                                                      # :145
        if getattr(b, "known", None) is not None:       # inpainting: the same reconstruction, then the given pixels put back
            call("mdm_inpaint_x0", dtype=pdt, pred_nhwc=ptr(pred), Cp=cp, x_in=ptr(b.x_in), s=ptr(b.s), known=ptr(b.known),
                 keep=ptr(b.keep), keep_C=b.keep.shape[1], N=n, C=c, H=h, W=w, pred_nchw=ptr(b.pred_nchw), shifted0=ptr(b.shifted0),
                 x0_hat=ptr(b.x0_hat), stream=stream())
        elif getattr(b, "measurement", None) is not None:   # restoration: the same reconstruction, then the group means put right
            call("mdm_restore_x0", dtype=pdt, pred_nhwc=ptr(pred), Cp=cp, x_in=ptr(b.x_in), s=ptr(b.s), y=ptr(b.measurement), k=b.pool,
                 gray=b.gray, N=n, C=c, H=h, W=w, pred_nchw=ptr(b.pred_nchw), shifted0=ptr(b.shifted0), x0_hat=ptr(b.x0_hat),
                 stream=stream())
        else:
            call("mdm_sampler_x0", dtype=pdt, pred_nhwc=ptr(pred), Cp=cp, x_in=ptr(b.x_in), s=ptr(b.s), N=n, C=c, H=h, W=w,
                 pred_nchw=ptr(b.pred_nchw), shifted0=ptr(b.shifted0), x0_hat=ptr(b.x0_hat), stream=stream())          # :146-152
        degrade = functools.partial(S.emit_degrade, b.x0_hat, mean_pixel=b.mp, mean_option=a.mean_option, mean_area=a.mean_area)
        if dep == "independent":                                                                                       # :175-181
            degrade(b.d_t, rng_stream=3, mask_out=b.m_t, **mask_src(b.amt_t, b.mi_t))
            degrade(b.d_next, rng_stream=4, mask_out=b.m_next, **mask_src(b.amt_next, b.mi_next))
        elif dep == "dependent_t":      # :191-196, nested masks: ONE draw (the same Philox stream) thresholded at both ratios
            src = mask_src(b.amt_t, b.mi_t)
            degrade(b.d_t, rng_stream=3, mask_out=b.m_t, **src)
            degrade(b.d_next, rng_stream=3, mask_out=b.m_next, **dict(src, amount=b.amt_next))
        else:                           # :184-188: the mask of the step before, read before this step's takes its place
            degrade(b.d_t, rng_stream=0, mask_in=b.m_next)
            degrade(b.d_next, rng_stream=4, mask_out=b.m_next, **mask_src(b.amt_next, b.mi_next))
        if update:                                                                                                     # :206-216
            call("mdm_sampler_update", ptr(b.d_t), ptr(b.d_next), ptr(b.x_t), ptr(b.diff), int(a.momentum_adaptive == "base_momentum"),
                 b.x_t.numel(), stream())

    def _sample_graph(self, model, timesteps, b):
        """The same loop as the host-driven one of `_sample_mean_shift_momentum` (history off, device RNG) with ONE hipGraph per
        reverse step: the per-step scalars (t, t-1, shift ratio, degrade amounts, Philox offset) are produced on the device by
        `mdm_sampler_step_params` from a step counter, so T replays need no host work in between."""
        S = self.Scheduler
        dev, T, n = S.device, len(timesteps), b.x_t.shape[0]
        amount_tab = (S.pixels_dev if b.indexing else S.ratio_dev).to(dev, torch.float64).contiguous()
        ratio_tab = S.ratio_dev.to(dev, torch.float64).contiguous()
        ts_dev = torch.as_tensor([int(t) for t in timesteps], dtype=torch.int32, device=dev)
        ctr = torch.zeros(1, dtype=torch.int32, device=dev)

        def params():
            call("mdm_sampler_step_params", timesteps=ptr(ts_dev), T=T, step_ctr=ptr(ctr), ratio_tab=ptr(ratio_tab),
                 amount_tab=ptr(amount_tab), n=n, time_out=ptr(b.time), ratio_out=ptr(b.ratio) if b.kind != 0 else None,
                 amt_t=ptr(b.amt_t), amt_next=ptr(b.amt_next), rng=ptr(S.dev_rng.dev), stream=stream())

        def forward():
            _lib._recording.extend(model.forward_plan)
            return model.y_out.data, model.cout_p, model.dt

        with _lib.Recording() as body:
            self._emit_step(b, True, params, forward)
        with _lib.Recording() as last:                       # i == 0: base_sampling breaks before the write, momentum skips it
            self._emit_step(b, False, params, forward)
        gb, gl = _lib.GraphExec(body), _lib.GraphExec(last)
        for _ in range(T - 1):
            gb.launch()
        gl.launch()
        self._graph_keep = ((b, ts_dev, ctr, amount_tab, ratio_tab), gb, gl)
        return b.x0_hat

    def _draws(self, b):
        """-> (z(), mask_src(amount, index_buffer)): the random input of a shift / a degrade launch as keywords of the Scheduler's
        emitters.  Device RNG: the kernels draw (Philox), 'indexing' pairs the degrade with the index-mask launch.  Replay RNG: the
        host's draws, made when asked for -- where the reference makes them (shift, degrade t, degrade t-1)."""
        S = self.Scheduler
        n, c, h, w = b.x_t.shape
        if S.rng_mode == "device":
            return (lambda: None), (lambda amount, mi: dict(index_mask=(amount, mi)) if b.indexing else dict(amount=amount))
        def mask_src(amount, mi):
            if b.indexing:
                return dict(mask_in=S.host_index_mask(S._host_full(amount.cpu().long(), n), n, c, h, w))
            return dict(amount=amount, u=S.host_uniforms(b.x_t))
        return (lambda: S.host_shift_z(S._host_full(b.ratio.cpu(), n), n, c, h, w) if b.kind != 0 else None), mask_src

    def _sample_mean_shift_momentum(self, model, timesteps, latent=None, inpaint=None, hist_steps=None, restore=None):
        """sampler.py:109-261.  `inpaint = (known, keep)`: the rows of this run on the device; every step then projects its
        prediction onto them (`sample_inpaint`).  `restore = (y, k, gray)`: the measurement rows of this run on the device; every
        step then projects its prediction onto the images with these group means (`sample_restore`).  `hist_steps`: the history
        lists get that many slots + 1 (a 'matched' run walks fewer steps than the list it was given has; the slots behind them
        stay zero)."""
        from .unet import UNet
        if inpaint is not None and restore is not None:
            raise ValueError("inpaint and restore: one projection per run, a keep mask and a measurement do not combine")
        a, S = self.args, self.Scheduler
        dev, T = S.device, len(timesteps)
        n, c, hw = a.sample_num, a.out_channel, a.data_size
        dep, mode = a.sampling_mask_dependency, a.momentum_adaptive
        if dep not in ("independent", "dependent_prev", "dependent_t"):
            raise UnboundLocalError(f"sampling_mask_dependency={dep!r} is not an option upstream")
        if dep == "dependent_t":                # runs upstream for a sub-case only (scheduler.py:480-549); same errors here
            S._check_dependent_args(a, a.mean_option, a.mean_area)
            S._check_degrade_args(torch.empty(1, c, 1, 1))
        if mode not in ("base_sampling", "base_momentum"):
            raise UnboundLocalError(f"momentum_adaptive={mode!r} does not run upstream (D4)")
        hist_mode = getattr(a, "sample_history", True)
        fused = isinstance(model, UNet)
        if fused and getattr(a, "sampler_uniform_t", True):
            model = model.with_uniform_t()      # every reverse step passes ONE timestep for the whole batch (sampler.py:137-145)
        if fused:
            assert (model.N, model.H, model.W) == (n, hw, hw), "UNet plan was built for another batch/extent"
        x_t = (latent if latent is not None else self._get_latent_initial(model)).to(dev, torch.float32).contiguous()
        graph = (fused and not hist_mode and S.rng_mode == "device" and model.use_graph and getattr(a, "sampler_graph", True)
                 and self.step_hook is None)
        # the step's buffers, allocated once: both loops run `_emit_step` over them
        img = lambda on=True: torch.empty_like(x_t) if on else None
        f64 = lambda: torch.empty(n, dtype=torch.float64, device=dev)
        indexing = a.select_degrade_pixel == "indexing"
        b = types.SimpleNamespace(
            x_t=x_t, kind=S.shift_kind(), indexing=indexing, nhwc=(model.dt, model.x_in.data, model.cin_p) if fused else None,
            time=model.t_in if graph else torch.empty(n, device=dev), ratio=f64(), amt_t=f64(), amt_next=f64(),
            s=img(), x_in=img(), pred_nchw=img(hist_mode), shifted0=img(hist_mode), x0_hat=img(), d_t=img(), d_next=img(), m_t=img(),
            m_next=torch.zeros_like(x_t), mi_t=img(indexing and S.rng_mode == "device"), mi_next=img(indexing and S.rng_mode == "device"),
            mp=torch.empty(n, c, device=dev), diff=torch.zeros_like(x_t))
        if inpaint is not None:
            b.known, b.keep = inpaint
        if restore is not None:
            b.measurement, b.pool, b.gray = restore
        b.draw_z, b.mask_src = self._draws(b)
        if graph:
            return self._sample_graph(model, timesteps, b), []
        slots = (T if hist_steps is None else hist_steps) + 1
        hist = {k: torch.zeros(slots, n, c, hw, hw, device=dev) for k in HISTORY_NAMES} if hist_mode else None

        def params(i):                          # what mdm_sampler_step_params does for the graph loop
            S.dev_rng.advance()
            b.time.fill_(float(timesteps[i]))
            n_t = S.get_black_area_num_pixels_time(b.time)
            n_next = S.get_black_area_num_pixels_time(b.time - 1 if i > 0 else b.time)       # :167-170
            S._check_counts(n_t)
            b.amt_t.copy_(n_t); b.amt_next.copy_(n_next)
            if b.kind != 0:
                torch.index_select(S.ratio_dev, 0, b.time.int() - 1, out=b.ratio)
        for i in range(T - 1, -1, -1):
            slot = T - i
            if self.step_hook is not None:
                self.step_hook(i, slot, x_t)
            if hist_mode:
                hist["sample_t"][slot].copy_(x_t)
            last = mode == "base_sampling" and i == 0                                  # :204-205 (break before the writes)
            self._emit_step(b, not last and (i > 0 or mode == "base_sampling"), functools.partial(params, i),      # :206-216
                            lambda: self._predict(model, b.x_in, b.time, fused))
            if hist_mode:                       # (the update writes x_t and diff only: these read what the step left)
                hist["shift"][slot].copy_(b.s); hist["shifted"][slot].copy_(b.x_in); hist["mask"][slot].copy_(b.pred_nchw)
                hist["shifted_result"][slot].copy_(b.shifted0); hist["sample_0"][slot].copy_(b.x0_hat)
                if dep in ("independent", "dependent_t"):
                    hist["degraded_mask"][slot].copy_(b.m_t); hist["degraded_mask_next"][slot].copy_(b.m_next)
                else:
                    hist["degraded_mask"][slot].copy_(b.m_next)
            if last:
                break
            if hist_mode:
                hist["degraded_next_t"][slot].copy_(b.d_next); hist["degraded_t"][slot].copy_(b.d_t); hist["difference"][slot].copy_(b.diff)
        return b.x0_hat, [hist[k] if hist_mode == "device" else hist[k].cpu() for k in HISTORY_NAMES] if hist_mode else []
