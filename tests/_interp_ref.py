"""CPU restatement of the latent-interpolation sampler (helpers only, no test functions), built on the classes of oracle/.

Own-words restatement of reference code/sampler.py:86-99 (`_get_latent_initial_interpolation`), :264-366 (`_sample_interpolation`)
and scheduler.py:552-569 (`degrade_interpolation_sampling`), :735-754 (`get_schedule_shift_time_interpolation`), with every draw
going through the scheduler's `rng` object like the rest of oracle/; and the host predictor of the device draw of
csrc/interp.hip `interp_row_mask_kernel`.  tests/test_interp_cpu.py checks both against tests/golden/sampler_interp.npz and
wrong twins; the gpu tests compare the kernels and the product loop with them.
"""
import numpy as np
import torch

from _philox_ref import u01, words
from oracle.sampler_ref import HISTORY_NAMES, SamplerRef
from oracle.scheduler_ref import SchedulerRef, apply_degrade

INTERP_HISTORY_NAMES = [k for k in HISTORY_NAMES if k != "degraded_mask_next"]
STREAM_INTERP_ROW = 6
FIXTURE_LISTS = ["sample_t", "mask", "degraded_mask", "degraded_t", "degraded_next_t"]     # what sampler_interp.npz stores of the ten


# ------------------------------------------------------------------------------------------ the device row
def row_uniforms(key, offset, HW, stream=STREAM_INTERP_ROW, lane=None, mask_key=True):
    """float32 [HW].  interp_row_mask_kernel: `Philox ph(rng[0] & 0xFFFFFFFF); w = ph(p >> 2, rng[1] * 8 + 6); u[p] = u01(lane p & 3
    of (w.x, w.y, w.z, w.w))`.  `stream`, `lane` (a fixed lane for every pixel) and `mask_key=False` (the rank half kept) make the
    wrong twins the cpu test rejects."""
    k = int(key) & 0xFFFFFFFF if mask_key else int(key)
    p = np.arange(HW)
    w = words(k, offset, stream, np.arange((HW + 3) >> 2))
    return u01(w[p >> 2, (p & 3) if lane is None else lane])


def row_keep(u, amount, C):
    """float32 [N, C, HW] of 0 / 1: `((double)u[p] > amount[n]) ? 1.f : 0.f`, the same for every channel."""
    k = (np.asarray(u, dtype=np.float64)[None, :] > np.asarray(amount, dtype=np.float64).reshape(-1, 1)).astype(np.float32)
    return np.repeat(k[:, None, :], C, axis=1)


# ------------------------------------------------------------------------------------------ numpy statements of the two other kernels
def shift_np(x_t, mu, ratio, shift):
    """(s, x_in) float32 like x_t [N, C, H, W]: sv = float32(float64(float32(shift)) * ratio); s = float32(clamp(float64(sv),
    -float64(mu) - ratio, -float64(mu) + ratio)) with torch.clamp's NaN rule (np.minimum / np.maximum propagate a NaN)."""
    ratio = np.asarray(ratio, dtype=np.float64)
    m = -np.asarray(mu, dtype=np.float32).astype(np.float64)
    sv = (np.float64(np.float32(shift)) * ratio).astype(np.float32)
    s = np.minimum(np.maximum(sv.astype(np.float64), m - ratio), m + ratio).astype(np.float32)
    s = np.broadcast_to(s.reshape(-1, 1, 1, 1), x_t.shape).copy()
    return s, (x_t + s).astype(np.float32)


def latent_grid(shift, N):
    """The closed form of the ramp's ends (sampler.py:89-94) -> (first, last)."""
    return (-1.0, 1.0 - shift) if shift > 0 else (-1.0 - shift, 1.0) if shift < 0 else (-1.0, 1.0)


# ------------------------------------------------------------------------------------------ the four upstream functions
class InterpSchedulerRef(SchedulerRef):
    def get_schedule_shift_time_interpolation(self, timesteps, mu, interpolation_shift):
        t = timesteps.int()
        ratio = torch.index_select(self.ratio_list, 0, t - 1)
        wd = getattr(self.args, "weight_dtype", torch.float32)
        s = ((torch.ones(len(t)) * interpolation_shift) * ratio).to(wd)                     # :739-745
        s = torch.clamp(s, min=-1 * mu - ratio, max=-1 * mu + ratio)                        # :747-749 (fp64 bounds promote)
        return s[:, None, None, None].to(wd)

    def degrade_interpolation_sampling(self, black_area_num_t, img, mean_option=None, mean_area=None):
        n = len(black_area_num_t)
        u = self.rng.uniform((1, self.height * self.width), 0.0, 1.0)                       # :553: ONE row for the batch
        masks = (u > black_area_num_t.unsqueeze(1)).float().reshape(n, 1, self.height, self.width).expand_as(img)
        try:
            mp = torch.ones(n, img.shape[1], 1, 1) * float(mean_option)                     # None: TypeError, not caught upstream
        except ValueError:                                                                  # ANY string: image-wise degraded area
            gone = 1 - masks
            mp = (img * gone).sum(dim=(1, 2, 3), keepdim=True) / gone.sum(dim=(1, 2, 3), keepdim=True)
        return apply_degrade(img, masks, mp), masks, mp * torch.ones(n, masks.shape[1], self.height, self.width)


class InterpSamplerRef(SamplerRef):
    def _get_latent_initial_interpolation(self, interpolation_shift):
        a = self.args
        if interpolation_shift > 0:
            grid = torch.linspace(-1, 1 - interpolation_shift, a.sample_num)
        elif interpolation_shift < 0:
            grid = torch.linspace(-1 - interpolation_shift, 1, a.sample_num)
        else:
            grid = torch.linspace(-1, 1, a.sample_num)
        grid = grid[:, None, None, None]
        return torch.zeros(a.sample_num, a.out_channel, a.data_size, a.data_size) + grid, grid

    def _sample_interpolation(self, model, timesteps, interpolation_shift):
        a, S = self.args, self.Scheduler
        T, n, c, hw = len(timesteps), a.sample_num, a.out_channel, a.data_size
        latent, mu = self._get_latent_initial_interpolation(interpolation_shift)
        x_t = latent
        m_next = torch.zeros(1, c, hw, hw)
        hist = {k: torch.zeros(T + 1, n, c, hw, hw) for k in INTERP_HISTORY_NAMES}
        if a.sampling_mask_dependency == "dependent":                                       # :293-295: drawn, never read
            for _ in range(n):
                self.rng.randperm(hw * hw)
        x0_hat = None
        with torch.no_grad():
            for i in range(T - 1, -1, -1):
                slot = T - i
                time = torch.Tensor([timesteps[i]]).expand(n)
                s = S.get_schedule_shift_time_interpolation(time, mu.squeeze(), interpolation_shift)
                x_in = S.perturb_shift(x_t, s)
                pred = model(x_in, time).sample
                shifted0 = x_in + pred
                x0_hat = S.perturb_shift_inverse(shifted0, s)
                hist["shift"][slot] = s; hist["shifted"][slot] = x_in; hist["mask"][slot] = pred
                hist["shifted_result"][slot] = shifted0; hist["sample_0"][slot] = x0_hat
                if i > 0:
                    n_next = S.get_black_area_num_pixels_time(time - 1)
                    d_t = S.degrade_with_mask(x0_hat, m_next, mean_option=a.mean_option, mean_area=a.mean_area)
                    d_next, m_next, _ = S.degrade_interpolation_sampling(n_next, x0_hat, mean_option=a.mean_option, mean_area=a.mean_area)
                    diff = x_t - d_t
                    mode = a.momentum_adaptive
                    if mode == "base_momentum":
                        x_t = d_next + diff
                    elif mode in ("momentum", "boosting"):                                  # :341, 352: `momentum` is read unbound
                        raise UnboundLocalError("momentum_adaptive=%r does not run upstream (D4)" % mode)
                    hist["degraded_next_t"][slot] = d_next; hist["degraded_t"][slot] = d_t; hist["difference"][slot] = diff
                    hist["sample_t"][slot] = x_t; hist["degraded_mask"][slot] = m_next
        return x0_hat, mu, [hist[k] for k in INTERP_HISTORY_NAMES]


# ------------------------------------------------------------------------------------------ the fixture
def fixture_args(cfg, base_args, **kw):
    """The args of a fixture row `cfg` = [dependency, momentum_adaptive, mean_option, type of mean_option, mean_area, select, channel,
    schedule, interpolation_shift] -> (args, interpolation_shift)."""
    dep, mode, mo, mo_type, ma, sel, ch, kind, shift = [str(v) for v in cfg]
    mo = {"int": int, "float": float, "str": str, "NoneType": lambda v: None}[mo_type](mo)
    a = base_args(data_size=16, ddpm_schedule=kind, ddpm_num_steps=6, select_degrade_pixel=sel, degrade_channel=None if ch == "None" else ch,
                  sampling_mask_dependency=dep, momentum_adaptive=mode, mean_option=mo, mean_area=ma, sample_num=4, **kw)
    return a, float(shift)


def fixture_hist(g, i, latent):
    """The ten lists [10, T+1, N, C, H, W] of fixture case `i`.  The file stores `shift` as one value per sample and, of the rest,
    FIXTURE_LISTS; the other four are single fp32 operations of stored ones, which its generator checked bit for bit against the
    reference's own tensors before leaving them out: shifted = x_t + shift (x_t: the latent, then sample_t of the slot before),
    shifted_result = shifted + mask, sample_0 = shifted_result - shift, difference = x_t - degraded_t."""
    h = {k: g[f"interp{i}_{k}"].astype(np.float32) for k in FIXTURE_LISTS}
    T1, shape = h["mask"].shape[0], h["mask"].shape
    h["shift"] = np.broadcast_to(g[f"interp{i}_shift"].astype(np.float32).reshape(T1, shape[1], 1, 1, 1), shape).copy()
    h["shifted"], h["difference"] = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    x_t = np.asarray(latent, dtype=np.float32)
    for slot in range(1, T1):
        h["shifted"][slot] = x_t + h["shift"][slot]
        if slot < T1 - 1:
            h["difference"][slot] = x_t - h["degraded_t"][slot]
            x_t = h["sample_t"][slot]
    h["shifted_result"] = h["shifted"] + h["mask"]
    h["sample_0"] = h["shifted_result"] - h["shift"]
    return np.stack([h[k] for k in INTERP_HISTORY_NAMES])
