"""Forward-process scheduler on the GPU -- same surface as the reference `Scheduler(args)`.

Mirrors reference code/scheduler.py: `update_ddpm_num_steps` (:27-65), schedule tables
(:103-142), `get_timesteps_epoch` (:173-192), `get_black_area_num_pixels_time` (:88-100),
`degrade_training` (:266-323), `degrade_independent_base_sampling` (:418-477),
`degrade_with_mask` (:572-598), `get_schedule_shift_time` (:612-732), `perturb_shift(_inverse)`
(:757-777), `get_weight_timesteps` (:780-794).  Options that do not run upstream at HEAD
 raise the same kind of error here.

Randomness (`args.rng_mode`, default "replay"):
  replay : draws come from torch's CPU generator in exactly the reference's order and shape
           (scheduler.py:282,288,294,620,658,675,694,703-707) and are shipped to the device, so a
           run seeded like the reference reproduces its masks/shifts bit for bit;
  device : Philox4x32-10 inside the kernels (no host round trip; what bench.py and the
           captured train-step graph use).  Same distributions, different stream.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

SHIFT_KINDS = {"non_shift": 0, "1-d_constant": 1, "3-d_constant": 2, "noise_reduction": 3,
               "noise_with_perturbation": 4, "noise_std_reduction": 5}


class DeviceRng:
    """Philox key/offset pair living in device memory.  `advance()` bumps the offset ON the device, in stream order
    (recorded like any other launch, so a captured step bumps it on every replay); a host-side counter copied over
    asynchronously would be read late by a GPU that the host runs ahead of."""

    def __init__(self, device, seed=0, rank=0):
        # key = (seed, rank): data-parallel ranks and sampler shards draw from disjoint streams (the reference seeds
        # every rank alike, main_train_masked.py:441-445 -- all ranks would draw identical t / masks)
        key = (int(seed) & 0xFFFFFFFF) | ((int(rank) & 0x7FFFFFFF) << 32)
        self.dev = torch.tensor([key, 0], dtype=torch.int64, device=device) if torch.cuda.is_available() \
            else torch.tensor([key, 0], dtype=torch.int64)

    def advance(self):
        call("mdm_rng_advance", ptr(self.dev), stream())


def _fill_mode(mean_option, mean_area):
    """-> (fill_mode, fill_const) of mdm_degrade; float(mean_option) first, like scheduler.py:298-317."""
    try:
        return 0, float(mean_option)
    except ValueError:
        pass
    if mean_option == "degraded_area":
        if mean_area == "image-wise":
            return 1, 0.0
        if mean_area == "channel-wise":
            return 2, 0.0
    elif mean_option == "non_degraded_area":
        return 3, 0.0
    raise UnboundLocalError(f"mean_pixel undefined for mean_option={mean_option!r}, mean_area={mean_area!r}")


class Scheduler:
    def __init__(self, args, device=None):
        _lib.load()
        self.args = args
        self.height = self.width = args.data_size
        self.image_size = self.height * self.width
        self.updated_ddpm_num_steps = None
        self.ratio_list = None
        self.black_area_pixels = None
        if device is not None:
            self.device = torch.device(device)
        elif torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        else:       # host-only use: schedule tables, timestep lists, gathers (every kernel call needs the GPU)
            self.device = torch.device("cpu")
        self.rng_mode = getattr(args, "rng_mode", "replay")
        self.reference_quirks = getattr(args, "reference_quirks", True)
        rank = getattr(args, "rng_rank", None)
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
        self.dev_rng = DeviceRng(self.device, getattr(args, "seed", 0), rank)
        # Sharded sampling (mdm.Sampler over a process group): (lo, hi, n) = this rank computes rows [lo, hi) of an n-sample
        # batch.  The reference seeds every rank alike (main_train_masked.py:441-445), so a rank that drew only ITS rows from the
        # host generator would draw the same numbers as every other rank -- W copies of the same samples.  Host draws are
        # therefore made for all n samples on every rank (same seed -> same numbers) and sliced: the gathered batch equals
        # what one process computes.
        self.replay_rows = None

    def _host_rows(self, n_local):
        """(n to draw on the host, slice of it that is ours)."""
        if self.replay_rows is None:
            return n_local, slice(None)
        lo, hi, n = self.replay_rows
        assert hi - lo == n_local, (self.replay_rows, n_local)
        return n, slice(lo, hi)

    # ---- schedule tables (host, once per run) -------------------------------------
    def update_ddpm_num_steps(self, max_time=None):
        a = self.args          # the argument is ignored upstream too (scheduler.py:40-49, D15)
        kind, T = a.ddpm_schedule, a.ddpm_num_steps
        if kind == "linear":                                   # :103-109
            table = np.linspace(1e-3, 1, T)
            self.ratio_list = torch.tensor(table)
            self.black_area_pixels = self.ratio_list
        elif kind == "exponential":                            # :130-142
            e = getattr(a, "ddpm_schedule_base", 10.0) ** np.linspace(0, 1, T)
            self.ratio_list = torch.tensor(e / e[-1])
            self.black_area_pixels = self.ratio_list
        elif kind == "log":                                    # :112-127, 54-56
            if T > self.image_size:
                raise ValueError("Desired to remove number of pixels is greater than the size of input image.")
            v = np.log(np.linspace(1, self.image_size, T))
            v = v - v.min() + 1
            v = v * (self.image_size / v.max())
            counts = np.array(sorted(set(np.asarray(v, dtype=int))))
            counts[-1] = self.image_size
            self.black_area_pixels = counts
            self.ratio_list = torch.tensor(counts / self.image_size)
        elif kind == "sigmoid":
            raise TypeError("ddpm_schedule='sigmoid' does not run upstream (torch.flip of an ndarray, scheduler.py:58-61)")
        else:
            raise ValueError("Invalid mask ratio scheduler")
        self.updated_ddpm_num_steps = len(self.ratio_list)
        self.reverse_ratio = torch.flip(self.ratio_list, dims=(0,))
        # the device tables keep their addresses across calls (captured graphs hold raw pointers to them)
        def put(name, host):
            old = getattr(self, name, None)
            if old is not None and old.shape == host.shape and old.dtype == host.dtype:
                old.copy_(host)
            else:
                setattr(self, name, host.to(self.device))
        put("ratio_dev", self.ratio_list)
        put("pixels_dev", torch.as_tensor(np.asarray(self.black_area_pixels)))
        return self.updated_ddpm_num_steps

    def get_black_area_num_pixels_all(self):
        return self.black_area_pixels

    def get_updated_ddpm_num_steps(self):
        return self.updated_ddpm_num_steps

    def get_ratio_list(self):
        return self.ratio_list

    def get_reverse_ratio_list(self):
        return self.reverse_ratio

    def get_timesteps_epoch(self, epoch, epoch_length):
        scale = self.args.scheduler_num_scale_timesteps
        section = math.ceil((epoch + 1) / (epoch_length / scale))
        expo = scale - section
        stride = 2 ** expo if expo >= 0 else 1
        used = [i for i in range(1, self.updated_ddpm_num_steps + 1) if i % stride == 0]
        used[-1] = self.updated_ddpm_num_steps
        return used

    def get_black_area_num_pixels_time(self, time):
        idx = (time - 1).int() if hasattr(time, "int") else torch.as_tensor(time - 1).int()
        sel = self.args.select_degrade_pixel
        if sel == "indexing":
            tab = self.pixels_dev
        elif sel == "thresholding":
            tab = self.ratio_dev
        else:
            raise UnboundLocalError("select_degrade_pixel must be 'indexing' or 'thresholding'")
        return torch.index_select(tab.to(idx.device), 0, idx)

    def get_weight_timesteps(self, timesteps, power_base=2.0):
        alpha = torch.linspace(start=1, end=0, steps=self.updated_ddpm_num_steps)
        power = torch.pow(power_base, alpha).to(timesteps.device)
        return power[timesteps]

    # ---- masks / degrade ---------------------------------------------------------------
    def _check_degrade_args(self, img):
        sel, ch = self.args.select_degrade_pixel, getattr(self.args, "degrade_channel", None)
        if sel == "thresholding":
            if ch == "1-channel":
                return 1
            if ch == "3-channel":
                if img.shape[1] != 3:
                    raise RuntimeError("degrade_channel='3-channel' is hard-wired to 3 channels (scheduler.py:294-296)")
                return 3
            raise UnboundLocalError("thresholding needs degrade_channel in {'1-channel','3-channel'} (D8)")
        if sel == "indexing":
            return 1
        raise UnboundLocalError("select_degrade_pixel")

    def _check_counts(self, amount):
        if self.args.select_degrade_pixel == "indexing" and amount.dtype.is_floating_point:
            raise TypeError("indexing needs integer pixel counts (linear/exponential schedules give ratios, D7)")

    def emit_degrade(self, x0, x_t, mean_pixel, *, rng_stream, mean_option, mean_area, amount=None, u=None, mask_in=None,
                     index_mask=None, mask_out=None):
        """The one place that launches (or records) mdm_degrade, over the caller's contiguous fp32 device tensors; nothing is
        allocated, converted or read back.  The keep-mask comes from `mask_in` (degrade_with_mask; a replayed host mask), from
        `index_mask = (counts, buffer)` -- 'indexing' on the device: mdm_index_mask over `counts` [N] fp64 is issued in front into
        the caller's `buffer`, which then is the mask source -- or is drawn by the kernel: `amount` [N] fp64 ratios thresholding
        the uniforms `u` (replay) or Philox stream `rng_stream`.  Outputs: x_t, mean_pixel [N, C], optionally the mask."""
        N, C, HW = x0.shape[0], x0.shape[1], x0[0, 0].numel()
        fm, fc = _fill_mode(mean_option, mean_area)
        rng = ptr(self.dev_rng.dev)
        if index_mask is not None:
            counts, mask_in = index_mask
            call("mdm_index_mask", ptr(counts), 1, rng, rng_stream, N, C, HW, ptr(mask_in), stream())
        call("mdm_degrade", x0=ptr(x0), u=ptr(u), mask_in=ptr(mask_in), amount=ptr(amount), amount_stride=1, rng=rng,
             rng_stream=rng_stream, N=N, C=C, HW=HW, Cm=self._check_degrade_args(x0) if mask_in is None else C, fill_mode=fm,
             fill_const=fc, x_t=ptr(x_t), mask=ptr(mask_out), mean_pixel=ptr(mean_pixel), stream=stream())

    # replay mode: the host draws, in the reference's order and shape.  Each draws for the WHOLE batch and keeps this rank's rows
    # (`_host_rows`); `*_all` arguments are host values of the whole batch.
    def _host_full(self, v, n_local):
        """`v` [n_local] of a SAMPLER step for the whole batch: every sample of a step has the same, a shard repeats its first."""
        nh, _ = self._host_rows(n_local)
        return v if nh == n_local else v[:1].expand(nh)

    def host_index_mask(self, counts_all, N, C, H, W):
        """Serial CPU randperms like scheduler.py:281-282 -> keep-mask [N, C, H, W] on the device."""
        nh, rows = self._host_rows(N)
        m = torch.ones(nh, H * W)
        for i, num in enumerate(counts_all):
            m[i, torch.randperm(H * W)[:num]] = 0.0
        return m[rows].reshape(N, 1, H, W).expand(N, C, H, W).contiguous().to(self.device)

    def host_uniforms(self, img):
        """The uniforms 'thresholding' compares with the ratio (scheduler.py:288/294) -> [N, Cm * HW] on the device."""
        N, HW = img.shape[0], img[0, 0].numel()
        nh, rows = self._host_rows(N)
        return torch.empty(nh, self._check_degrade_args(img) * HW, dtype=torch.float32).uniform_(0.0, 1.0)[rows].contiguous().to(self.device)

    def host_shift_z(self, ratio_all, N, C, H, W):
        """-> z of mdm_shift on the device (None for 'non_shift'), scheduler.py:620,658,675,694,703-707."""
        nh, rows = self._host_rows(N)
        st, mean = self.args.shift_type, float(getattr(self.args, "noise_mean", 0.0))
        if st == "1-d_constant":
            z = torch.empty(nh).uniform_(-1.0, 1.0)
        elif st == "3-d_constant":
            z = torch.empty(nh, 3, 1, 1).uniform_(-1.0, 1.0)
        elif st == "noise_reduction":
            z = torch.empty(nh, 1, H, W).normal_(mean=mean, std=1)
        elif st == "noise_std_reduction":
            z = torch.zeros(nh, 3, H, W)
            for i in range(nh):
                z[i] = torch.empty(1, 3, H, W).normal_(mean=mean, std=float(ratio_all[i]))
        elif st == "noise_with_perturbation":
            torch.empty((nh,) if nh == 1 else (nh, 1, 1, 1)).uniform_(-1.0, 1.0)      # consumed then discarded (D11)
            z = torch.empty(nh, 3, H, W).normal_(mean=mean, std=1)
        else:
            return None
        return z[rows].to(self.device).contiguous()

    def _degrade(self, amount, img, mean_option, mean_area, rng_stream, mask_in=None, want_mask=True, u=None):
        """Allocate-then-emit core of the degrade_* methods -> (x_t, mask, mean_pixel[N,C], u).  `u`: uniforms already on the
        device to threshold (replay mode) instead of drawing; the ones this call used are returned."""
        img = img.to(self.device, torch.float32).contiguous()
        N, C, H, W = img.shape
        x_t = torch.empty_like(img)
        mask = torch.empty_like(img) if want_mask else None
        mp = torch.empty(N, C, device=self.device)
        _fill_mode(mean_option, mean_area)          # a mean_option that does not run raises before the mask options do
        if mask_in is not None:
            src = dict(mask_in=mask_in.to(self.device, torch.float32).contiguous())
        else:
            self._check_degrade_args(img)
            self._check_counts(amount)
            if self.args.select_degrade_pixel != "indexing":
                if self.rng_mode == "replay" and u is None:
                    u = self.host_uniforms(img)
                src = dict(amount=amount.to(self.device, torch.float64).contiguous(), u=u)
            elif self.rng_mode == "replay":
                src = dict(mask_in=self.host_index_mask(self._host_full(amount.cpu(), N), N, C, H, W))
            else:
                src = dict(index_mask=(amount.to(self.device, torch.float64).contiguous(), torch.empty_like(img)))
        self.emit_degrade(img, x_t, mp, rng_stream=rng_stream, mean_option=mean_option, mean_area=mean_area, mask_out=mask, **src)
        return x_t, mask, mp, u

    def degrade_training(self, black_area_num, img, mean_option=None, mean_area=None):
        x_t, masks, mp, _ = self._degrade(black_area_num, img, mean_option, mean_area, rng_stream=1)
        return (x_t, masks) + self.degradation_visuals(masks, mp)

    @staticmethod
    def degradation_visuals(masks, mp):
        """(degradation_mask, mean_pixel) of scheduler.py:320-321 from the keep-mask [N, C, H, W] and the fill colour [N, C]:
        the two tensors `degrade_training` returns for visualisation only."""
        mp4 = mp[:, :, None, None]
        return (1 - masks) * mp4 + masks, torch.ones_like(masks) * mp4

    def degrade_independent_base_sampling(self, black_area_num_t, img, mean_option=None, mean_area=None, _stream=3):
        x_t, masks, mp, _ = self._degrade(black_area_num_t, img, mean_option, mean_area, rng_stream=_stream)
        return x_t, masks, mp[:, :, None, None] * torch.ones_like(x_t)

    def degrade_with_mask(self, img, masks, mean_option, mean_area):
        return self._degrade(None, img, mean_option, mean_area, rng_stream=0, mask_in=masks, want_mask=False)[0]

    @staticmethod
    def _check_dependent_args(args, mean_option, mean_area):
        """What degrade_dependent_base_sampling runs for upstream (scheduler.py:480-549): 'thresholding' only (the 'indexing'
        branch is `pass`, :490-491), and mean_option 'degraded_area' or the STRING "0" -- there is no float() attempt in that
        function, so the int 0, numbers and 'non_degraded_area' leave mean_pixel_t unbound (D5)."""
        if args.select_degrade_pixel != "thresholding":
            raise UnboundLocalError("masks_t undefined: degrade_dependent_base_sampling has no 'indexing' branch (D5)")
        if not ((mean_option == "degraded_area" and mean_area in ("image-wise", "channel-wise"))
                or (isinstance(mean_option, str) and mean_option == "0")):
            raise UnboundLocalError(f"mean_pixel_t undefined for mean_option={mean_option!r}, mean_area={mean_area!r} (D5)")

    def degrade_dependent_base_sampling(self, black_area_num_t, black_area_num_next_t, img, mean_option, mean_area, _stream=3):
        """scheduler.py:480-549: the masks of t and t-1 are NESTED -- one uniform draw per pixel thresholded at both
        ratios -> (degraded_t, mask_t, mean_mask_t, degraded_next, mask_next, mean_mask_next).  Two launches of the degrade
        kernel over the SAME uniforms: the host draw shipped once (replay), or the same Philox stream id (device)."""
        self._check_dependent_args(self.args, mean_option, mean_area)
        x_t, m_t, mp_t, u = self._degrade(black_area_num_t, img, mean_option, mean_area, rng_stream=_stream)
        x_n, m_n, mp_n, _ = self._degrade(black_area_num_next_t, img, mean_option, mean_area, rng_stream=_stream, u=u)
        ones = torch.ones_like(x_t)
        return x_t, m_t, mp_t[:, :, None, None] * ones, x_n, m_n, mp_n[:, :, None, None] * ones

    # ---- shift -------------------------------------------------------------------------
    def shift_kind(self, mean_shift=True):
        """`kind` of mdm_shift; the base trainer is the mean-shift one with 'non_shift' (SURVEY 3.2)."""
        st = self.args.shift_type if mean_shift else "non_shift"
        if st not in SHIFT_KINDS:
            raise UnboundLocalError(f"shift_time undefined for shift_type={st!r}")
        return SHIFT_KINDS[st]

    def emit_shift(self, x_t, s, x_in, *, kind, ratio=None, z=None, nhwc=None):
        """The one place that launches (or records) mdm_shift: s = z * ratio, x_in = x_t + s over the caller's contiguous fp32
        device tensors (`ratio` [N] fp64; `z`: replayed host draws, else Philox stream 2), optionally x_in once more as NHWC
        into `nhwc = (dtype, tensor, Cp)` for the U-Net.  Nothing is allocated, converted or read back."""
        N, C, H, W = x_t.shape
        # reference broadcast quirk: [N,*,H,W] * [N] lines up with the LAST axis when W == N (D10)
        per_col = int(self.reference_quirks and kind in (3, 4) and N == W and N > 1)
        dt, nh, Cp = nhwc if nhwc is not None else (0, None, 0)
        call("mdm_shift", x_t=ptr(x_t), z=ptr(z), ratio=ptr(ratio), rng=ptr(self.dev_rng.dev), rng_stream=2, kind=kind,
             noise_mean=float(getattr(self.args, "noise_mean", 0.0)), per_column=per_col, N=N, C=C, H=H, W=W, s=ptr(s), x_in=ptr(x_in),
             dtype=dt, x_in_nhwc=ptr(nh), Cp=Cp, stream=stream())

    def shift_and_perturb(self, timesteps, x_t, want_nhwc=None):
        """Fused get_schedule_shift_time + perturb_shift: -> (s, x_in); optionally also writes x_in as
        NHWC into `want_nhwc = (dtype, tensor, Cp)` for the U-Net."""
        kind = self.shift_kind()
        x_t = x_t.to(self.device, torch.float32).contiguous()
        N, C, H, W = x_t.shape
        ratio = z = None
        if kind != 0:
            idx = (timesteps.int() - 1).to(self.device)
            ratio = torch.index_select(self.ratio_dev, 0, idx).contiguous()
            if self.rng_mode == "replay":
                z = self.host_shift_z(self._host_full(ratio.cpu(), N), N, C, H, W)
        s, x_in = torch.empty_like(x_t), torch.empty_like(x_t)
        self.emit_shift(x_t, s, x_in, kind=kind, ratio=ratio, z=z, nhwc=want_nhwc)
        return s, x_in

    def get_schedule_shift_time(self, timesteps, binarymasks):
        zero = torch.zeros(binarymasks.shape, device=self.device, dtype=torch.float32)
        s, _ = self.shift_and_perturb(timesteps, zero)
        return s.to(getattr(self.args, "weight_dtype", torch.float32))

    # ---- latent interpolation (scheduler.py:552-569, 735-754) ---------------------------
    def emit_shift_interp(self, x_t, mu, ratio, interpolation_shift, s, x_in, *, nhwc=None):
        """The one place that launches (or records) mdm_interp_shift over the caller's contiguous device tensors: per sample
        s = clamp(float32(shift * ratio), -mu - ratio, -mu + ratio) in the reference's arithmetic (`mu` [N] fp32, `ratio` [N]
        fp64), x_in = x_t + s, optionally x_in once more as NHWC into `nhwc = (dtype, tensor, Cp)`.  `s` / `x_in` may be None.
        Nothing is drawn, allocated, converted or read back."""
        N, C, H, W = x_t.shape
        dt, nh, Cp = nhwc if nhwc is not None else (0, None, 0)
        call("mdm_interp_shift", x_t=ptr(x_t), mu=ptr(mu), ratio=ptr(ratio), shift=float(interpolation_shift), N=N, C=C, H=H, W=W,
             s=ptr(s), x_in=ptr(x_in), dtype=dt, x_in_nhwc=ptr(nh), Cp=Cp, stream=stream())

    def host_uniform_row(self, HW):
        """The ONE row of uniforms degrade_interpolation_sampling draws for the whole batch (scheduler.py:553) -> [HW] on the
        device.  The same on every shard of a batch: all ranks are seeded alike and the row does not depend on the batch."""
        return torch.empty(1, HW, dtype=torch.float32).uniform_(0.0, 1.0).reshape(HW).to(self.device)

    def emit_row_mask(self, amount, mask, *, u_row=None):
        """The one place that launches (or records) mdm_interp_row_mask: mask[n, c, p] = float64(u[p]) > amount[n] into the
        caller's `mask` [N, C, H, W] (`amount` [N] fp64).  `u_row` [HW]: the replayed host draw; None: the kernel draws the row
        (Philox stream 6, the key without its rank half -- the shards of one batch draw the same row)."""
        N, C, HW = mask.shape[0], mask.shape[1], mask[0, 0].numel()
        call("mdm_interp_row_mask", amount=ptr(amount), u_row=ptr(u_row), rng=ptr(self.dev_rng.dev), N=N, C=C, HW=HW,
             mask=ptr(mask), stream=stream())

    @staticmethod
    def _interp_fill(mean_option):
        """(mean_option, mean_area) of the masked fill degrade_interpolation_sampling makes (scheduler.py:559-563): float(mean_option)
        when that works, for ANY string the image-wise mean of the degraded area -- the option's name and mean_area are not looked
        at -- and for None the TypeError float() raises."""
        try:
            return float(mean_option), "image-wise"
        except ValueError:
            return "degraded_area", "image-wise"

    def get_schedule_shift_time_interpolation(self, timesteps, mu, interpolation_shift):
        """scheduler.py:735-754 -> [N, 1, 1, 1] in weight_dtype: the constant shift scaled by the ratio of each timestep and
        clamped to [-mu - ratio, -mu + ratio] per sample."""
        idx = (timesteps.int() - 1).to(self.device)
        N = idx.numel()
        ratio = torch.index_select(self.ratio_dev, 0, idx).contiguous()
        mu = torch.as_tensor(mu).to(self.device, torch.float32).reshape(N).contiguous()
        s = torch.empty(N, 1, 1, 1, device=self.device)
        self.emit_shift_interp(torch.zeros_like(s), mu, ratio, interpolation_shift, s, None)
        return s.to(getattr(self.args, "weight_dtype", torch.float32))

    def degrade_interpolation_sampling(self, black_area_num_t, img, mean_option=None, mean_area=None):
        """scheduler.py:552-569: ONE uniform row for the whole batch, thresholded at each sample's amount -> (degraded, mask,
        fill * ones).  Pixel counts ('indexing') are compared like ratios, as upstream does: every count is >= 1 > u, so that
        mask is all zero."""
        img = img.to(self.device, torch.float32).contiguous()
        N, C, H, W = img.shape
        amount = torch.as_tensor(black_area_num_t).to(self.device, torch.float64).reshape(N).contiguous()
        u_row = self.host_uniform_row(H * W) if self.rng_mode == "replay" else None
        mo, ma = self._interp_fill(mean_option)
        mask, x_t, mp = torch.empty_like(img), torch.empty_like(img), torch.empty(N, C, device=self.device)
        self.emit_row_mask(amount, mask, u_row=u_row)
        self.emit_degrade(img, x_t, mp, rng_stream=0, mean_option=mo, mean_area=ma, mask_in=mask)
        return x_t, mask, mp[:, :, None, None] * torch.ones_like(x_t)

    def perturb_shift(self, data, shift):
        return data + shift.to(data.device)

    def perturb_shift_inverse(self, data, shift):
        return data - shift.to(data.device)
