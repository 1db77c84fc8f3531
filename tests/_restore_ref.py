"""CPU restatement of the restoration sampler (helpers only, no test functions), built on the classes of oracle/.

Upstream has no restoration function, so this file -- not a golden file -- pins `mdm.Sampler.sample_restore`: it is
`oracle.sampler_ref.SamplerRef._sample_mean_shift_momentum` with the projection `x0_hat += y[g] - mean_g(x0_hat)` after every
reconstruction and the two starts, every draw going through the scheduler's `rng` like the rest of oracle/.  With the projection
skipped it is the oracle's loop bit for bit (tests/test_restore_cpu.py), which anchors it to the pinned oracle.
Also the numpy statements of the three kernels of csrc/restore.hip in the order include/mdm_restore.h states, and the fp64
reference of the projection with its derived bound.
"""
import numpy as np
import torch

from oracle.sampler_ref import HISTORY_NAMES, SamplerRef

STARTS = ("latent", "measured")
U = 2.0 ** -24
F32 = np.float32


# ------------------------------------------------------------------------------------------ groups
def group_size(k, gray, C):
    return k * k * (C if gray else 1)


def to_groups(x, k, gray):
    """x [N, C, H, W] -> [N, Cg, H / k, W / k, |g|]: every group's elements (in no particular order)"""
    N, C, H, W = x.shape
    v = x.reshape(N, C, H // k, k, W // k, k).transpose(0, 2, 4, 1, 3, 5)                  # n, by, bx, c, r, j
    if gray:
        return v.reshape(N, 1, H // k, W // k, C * k * k)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2, 4, 5)).reshape(N, C, H // k, W // k, k * k)


def from_groups(v, k, gray, C):
    """a value per group [N, Cg, H / k, W / k] -> [N, C, H, W], every element its group's value"""
    v = np.repeat(np.repeat(v, k, axis=2), k, axis=3)
    return np.repeat(v, C, axis=1) if gray and C > 1 else v


# ------------------------------------------------------------------------------------------ numpy statements of the three kernels
def group_sum_np(x, k, gray):
    """The fp32 sum of every group in the header's order: strips of min(k, 4) columns, each from +0 by sequential adds -- channels
    in order (gray), rows top to bottom, columns left to right -- and left + right for the two strips of k = 8."""
    x = np.asarray(x, dtype=F32)
    N, C, H, W = x.shape
    sw = min(k, 4)
    v = x.reshape(N, C, H // k, k, W // k, k // sw, sw)                                      # n, c, by, r, bx, strip, j
    strips = []
    for st in range(k // sw):
        acc = np.zeros((N, 1 if gray else C, H // k, W // k), dtype=F32)
        for c in (range(C) if gray else [slice(None)]):
            for r in range(k):
                for j in range(sw):
                    term = v[:, c, :, r, :, st, j]
                    acc = (acc + (term[:, None] if gray else term)).astype(F32)
        strips.append(acc)
    return strips[0] if len(strips) == 1 else (strips[0] + strips[1]).astype(F32)


def measure_np(x, k, gray):
    """mdm_restore_measure: sum / (float)|g|, one correctly rounded division"""
    return (group_sum_np(x, k, gray) / F32(group_size(k, gray, x.shape[1]))).astype(F32)


def parent_np(pred_nhwc, x_in, s):
    """what mdm_sampler_x0 writes -> (pred_nchw, shifted0, x0_hat): pred [N, H, W, Cp] already as float32"""
    C = x_in.shape[1]
    pv = np.ascontiguousarray(np.asarray(pred_nhwc, dtype=F32)[..., :C].transpose(0, 3, 1, 2))
    sh0 = (x_in + pv).astype(F32)
    return pv, sh0, ((sh0 - s).astype(F32) if s is not None else sh0)


def project_np(x, y, k, gray):
    """x' = x + (y[g] - m[g]): two fp32 operations after the mean"""
    C = x.shape[1]
    d = (np.asarray(y, dtype=F32) - measure_np(x, k, gray)).astype(F32)
    return (x + from_groups(d, k, gray, C)).astype(F32)


def x0_np(pred_nhwc, x_in, s, y, k, gray):
    """mdm_restore_x0 -> (pred_nchw, shifted0, x0_hat)"""
    pv, sh0, x = parent_np(pred_nhwc, x_in, s)
    return pv, sh0, project_np(x, y, k, gray)


def expand_np(y, k, gray, C):
    """mdm_restore_start's `expand`: exact"""
    return np.ascontiguousarray(from_groups(np.asarray(y, dtype=F32), k, gray, C))


# ------------------------------------------------------------------------------------------ fp64 references and bounds
def _gamma(n):
    return n * U / (1 - n * U)


def mean_ref(x, k, gray):
    """-> (m fp64 per group, bound): the group means of x in fp64 and how far an fp32 evaluation may lie from them.  Derived from
    the arithmetic (nothing measured), in the style of tests/_inpaint_ref.mean_given_ref: an fp32 sum of n terms added in ANY order
    carries at most gamma(n - 1) sum |x_i|, gamma(j) = j u / (1 - j u), u = 2^-24 (Higham, eq. 4.4); the division rounds the
    quotient it forms once (u relative, or half the smallest subnormal):
        |m32 - m| <= E (1 + u) + u (|m| + E) + 2^-150,    E = gamma(|g| - 1) sum |x_i| / |g|."""
    g = to_groups(np.asarray(x, dtype=np.float64), k, gray)
    n = g.shape[-1]
    m = g.sum(-1) / n
    E = _gamma(n - 1) * np.abs(g).sum(-1) / n
    return m, E * (1 + U) + U * (np.abs(m) + E) + 2.0 ** -150


def project_ref(x, y, k, gray):
    """-> (x' fp64 per element, bound per element) for the fp32 x the parent kernel writes.  After the mean (bound Em above) the
    kernel forms d = fl(y - m32) and fl(x + d), each one u-relative rounding of what it forms:
        |d32 - (y - m)|        <= Em + u (|y - m| + Em)                  =: Ed
        |x'32 - (x + y - m)|   <= Ed + u (|x + (y - m)| + Ed)."""
    C = x.shape[1]
    m, Em = mean_ref(x, k, gray)
    d = np.asarray(y, dtype=np.float64) - m
    Ed = Em + U * (np.abs(d) + Em)
    ref = np.asarray(x, dtype=np.float64) + from_groups(d, k, gray, C)
    return ref, from_groups(Ed, k, gray, C) + U * (np.abs(ref) + from_groups(Ed, k, gray, C))


def mu_ref(y, C, gray, per_channel):
    """-> (mu fp64 [N, C], bound [N, C]) of mdm_restore_start: the mean of y [N, Cy, h, w] per channel (per_channel and not gray)
    or over everything, the bound of `mean_ref` with n the number of values."""
    y = np.asarray(y, dtype=np.float64)
    N = y.shape[0]
    v = y.reshape(N, y.shape[1], -1) if per_channel and not gray else y.reshape(N, 1, -1)
    n = v.shape[-1]
    m = v.sum(-1) / n
    E = _gamma(n - 1) * np.abs(v).sum(-1) / n
    bound = E * (1 + U) + U * (np.abs(m) + E) + 2.0 ** -150
    return np.broadcast_to(m, (N, C)), np.broadcast_to(bound, (N, C))


# ------------------------------------------------------------------------------------------ the loop
def measure_t(x, k, gray):
    """the measurement of a torch batch: fp64 means, ONE rounding (the kernel's fp32 mean lies in its bound)"""
    v = x.double().mean(dim=1, keepdim=True) if gray else x.double()
    return torch.nn.functional.avg_pool2d(v, k).float() if k > 1 else v.float()


def project_t(x, y, k, gray):
    d = y - measure_t(x, k, gray)
    return x + d.repeat_interleave(k, 2).repeat_interleave(k, 3)                          # (a grey d broadcasts over the channels)


class RestoreSamplerRef(SamplerRef):
    def _start(self, model, y, gray, start):
        """The latent draw is made in every start."""
        a = self.args
        n, c, hw = a.sample_num, a.out_channel, a.data_size
        latent = self._get_latent_initial(model).clone()
        if start == "latent":
            return latent
        dims = (2, 3) if a.mean_area == "channel-wise" and not gray else (1, 2, 3)
        return y.double().mean(dim=dims, keepdim=True).float().expand(n, c, hw, hw).clone()

    def sample_restore(self, model, timesteps, y, pool, gray=False, start="latent", project=True):
        if start not in STARTS:
            raise ValueError(start)
        a, S = self.args, self.Scheduler
        n, c, hw = a.sample_num, a.out_channel, a.data_size
        x_t = self._start(model, y, gray, start)
        T = len(timesteps)
        m_t = torch.zeros(n, c, hw, hw)
        m_next = torch.zeros(n, c, hw, hw)
        hist = {k: torch.zeros(T + 1, n, c, hw, hw) for k in HISTORY_NAMES}
        x0_hat, diff = None, torch.zeros(n, c, hw, hw)
        with torch.no_grad():
            for i in range(T - 1, -1, -1):
                slot = T - i
                time = torch.Tensor([timesteps[i]]).expand(n)
                s = S.get_schedule_shift_time(time, m_t)
                x_in = S.perturb_shift(x_t, s)
                pred = model(x_in, time).sample
                shifted0 = x_in + pred
                x0_hat = S.perturb_shift_inverse(shifted0, s)
                if project:
                    x0_hat = project_t(x0_hat, y, pool, gray)
                hist["sample_t"][slot] = x_t; hist["shift"][slot] = s; hist["shifted"][slot] = x_in
                hist["mask"][slot] = pred; hist["shifted_result"][slot] = shifted0; hist["sample_0"][slot] = x0_hat
                next_t = time - 1 if i > 0 else time
                n_t = S.get_black_area_num_pixels_time(time)
                n_next = S.get_black_area_num_pixels_time(next_t)
                dep = a.sampling_mask_dependency
                if dep == "independent":
                    d_t, m_t, _ = S.degrade_independent_base_sampling(n_t, x0_hat, mean_option=a.mean_option, mean_area=a.mean_area)
                    d_next, m_next, _ = S.degrade_independent_base_sampling(n_next, x0_hat, mean_option=a.mean_option, mean_area=a.mean_area)
                    hist["degraded_mask"][slot] = m_t; hist["degraded_mask_next"][slot] = m_next
                elif dep == "dependent_prev":
                    d_t = S.degrade_with_mask(x0_hat, m_next, mean_option=a.mean_option, mean_area=a.mean_area)
                    d_next, m_next, _ = S.degrade_independent_base_sampling(n_next, x0_hat, mean_option=a.mean_option, mean_area=a.mean_area)
                    hist["degraded_mask"][slot] = m_next
                elif dep == "dependent_t":
                    d_t, m_t, _, d_next, m_next, _ = S.degrade_dependent_base_sampling(n_t, n_next, x0_hat, mean_option=a.mean_option,
                                                                                       mean_area=a.mean_area)
                    hist["degraded_mask"][slot] = m_t; hist["degraded_mask_next"][slot] = m_next
                else:
                    raise UnboundLocalError("sampling_mask_dependency=%r is not an option upstream" % dep)
                mode = a.momentum_adaptive
                if mode == "base_sampling":
                    if i == 0:
                        break
                    diff = d_next - d_t
                    x_t = d_next
                elif mode == "base_momentum":
                    if i > 0:
                        diff = d_next - d_t
                        x_t = x_t + diff
                else:
                    raise UnboundLocalError("momentum_adaptive=%r does not run upstream (D4)" % mode)
                hist["degraded_next_t"][slot] = d_next; hist["degraded_t"][slot] = d_t; hist["difference"][slot] = diff
        return x0_hat, [hist[k] for k in HISTORY_NAMES]
