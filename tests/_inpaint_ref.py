"""CPU restatement of the inpainting sampler (helpers only, no test functions), built on the classes of oracle/.

Upstream has no inpainting function, so this file -- not a golden file -- pins `mdm.Sampler.sample_inpaint`: it is
`oracle.sampler_ref.SamplerRef._sample_mean_shift_momentum` with the projection `x0_hat = keep != 0 ? known : x0_hat` after every
reconstruction and the three starts, every draw going through the scheduler's `rng` like the rest of oracle/.  With `keep` all
zero and start "latent" it is the oracle's loop bit for bit (tests/test_inpaint_cpu.py), which anchors it to the pinned oracle.
Also the numpy statements of the two kernels of csrc/inpaint.hip and the bound of the start kernel's mean.
"""
import numpy as np
import torch

from oracle.sampler_ref import HISTORY_NAMES, SamplerRef

STARTS = ("latent", "known_mean", "matched")


# ------------------------------------------------------------------------------------------ numpy statements of the two kernels
def given_np(keep, C):
    """bool [N, C, ...]: keep [N, Ck, ...] != 0 broadcast to C channels (-0 is not given, NaN is given)"""
    g = np.asarray(keep, dtype=np.float32) != 0
    return np.repeat(g, C, axis=1) if g.shape[1] == 1 and C > 1 else g


def x0_np(pred_nhwc, x_in, s, known, keep):
    """mdm_inpaint_x0 -> (pred_nchw, shifted0, x0_hat) float32 NCHW: pred [N, H, W, Cp] already as float32 (a bf16 value is one
    exactly), the three NCHW operands float32; two fp32 operations and a select."""
    C = x_in.shape[1]
    pv = np.ascontiguousarray(np.asarray(pred_nhwc, dtype=np.float32)[..., :C].transpose(0, 3, 1, 2))
    sh0 = (x_in + pv).astype(np.float32)
    x = (sh0 - s).astype(np.float32) if s is not None else sh0
    return pv, sh0, np.where(given_np(keep, C), known, x).astype(np.float32)


def unknown_np(keep):
    """int32 [N]: pixels with any channel not given; keep [N, Ck, HW]"""
    return (~(np.asarray(keep, dtype=np.float32) != 0)).any(axis=1).sum(axis=1).astype(np.int32)


def start_np(known, keep, mu):
    """x_start = given ? known : mu[n][c] for known [N, C, HW], exact given the mu [N, C] the kernel wrote"""
    return np.where(given_np(keep, known.shape[1]), known, np.asarray(mu, dtype=np.float32)[:, :, None]).astype(np.float32)


def mean_given_ref(known, keep, fallback, per_channel):
    """-> (mu fp64 [N, C], bound fp64 [N, C], zero-count flags [N, C]): the mean of the given values of known [N, C, HW] in fp64, over
    the image (per_channel false) or the channel, and how far an fp32 evaluation may lie from it.

    Bound, in the style of tests/_bounds.py (derived from the arithmetic, nothing measured): an fp32 sum of n terms added in ANY
    order carries at most gamma(n - 1) sum |x_i| of error, gamma(k) = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability,
    eq. 4.4); n < 2^24 is an fp32 number, so the division adds one rounding, u relative, of the quotient it actually forms:
        |mu32 - mu| <= E (1 + u) + u (|mu| + E),    E = gamma(n - 1) sum |x_i| / n.
    Where n = 0 the kernel copies `fallback`: the bound is 0."""
    known = np.asarray(known, dtype=np.float64)
    N, C, HW = known.shape
    g = given_np(keep, C)
    axes = (2,) if per_channel else (1, 2)
    n = g.sum(axis=axes, keepdims=True).astype(np.float64)
    tot = np.where(g, known, 0.0).sum(axis=axes, keepdims=True)
    mag = np.where(g, np.abs(known), 0.0).sum(axis=axes, keepdims=True)
    u = 2.0 ** -24
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = tot / n
        k = np.maximum(n - 1, 0)
        E = k * u / (1 - k * u) * mag / n
        bound = E * (1 + u) + u * (np.abs(mu) + E)
    n, mu, bound = (np.broadcast_to(v.reshape(N, -1), (N, C)) for v in (n, mu, bound))
    none = n == 0
    return np.where(none, np.asarray(fallback, dtype=np.float64), mu), np.where(none, 0.0, bound), none


# ------------------------------------------------------------------------------------------ the host helpers restated
def start_index(ratio_list, timesteps, frac):
    """the first j with ratio_list[timesteps[j] - 1] >= frac, else the last index"""
    hit = [j for j, t in enumerate(timesteps) if float(ratio_list[int(t) - 1]) >= float(frac)]
    return hit[0] if hit else len(timesteps) - 1


# ------------------------------------------------------------------------------------------ the loop
class InpaintSamplerRef(SamplerRef):
    def _start(self, model, known, keep, start):
        """-> (x_t [N, C, H, W], unknown [N]).  The latent draw is made in every start."""
        a = self.args
        n, c, hw = a.sample_num, a.out_channel, a.data_size
        latent = self._get_latent_initial(model).clone()
        given = (keep != 0).expand(n, c, hw, hw)
        unknown = (~given).any(dim=1).sum(dim=(1, 2))
        if start == "latent":
            return latent, unknown
        dims = (2, 3) if a.mean_area == "channel-wise" else (1, 2, 3)
        cnt = given.sum(dim=dims, keepdim=True)
        tot = torch.where(given, known, torch.zeros(())).double().sum(dim=dims, keepdim=True)        # fp64 sum, ONE rounding: the
        mean = torch.where(cnt > 0, (tot / cnt).float().expand(n, c, hw, hw), latent)                # kernel's fp32 sum lies in its bound
        return (mean if start == "known_mean" else torch.where(given, known, mean)), unknown

    def sample_inpaint(self, model, timesteps, known, keep, start="latent"):
        if start not in STARTS:
            raise ValueError(start)
        a, S = self.args, self.Scheduler
        n, c, hw = a.sample_num, a.out_channel, a.data_size
        x_t, unknown = self._start(model, known, keep, start)
        T_all = len(timesteps)
        if start == "matched":
            timesteps = timesteps[:start_index(S.ratio_list, timesteps, int(unknown.max()) / float(hw * hw)) + 1]
        T = len(timesteps)
        given = (keep != 0).expand(n, c, hw, hw)
        m_t = torch.zeros(n, c, hw, hw)
        m_next = torch.zeros(n, c, hw, hw)
        hist = {k: torch.zeros(T_all + 1, n, c, hw, hw) for k in HISTORY_NAMES}
        x0_hat, diff = None, torch.zeros(n, c, hw, hw)      # (a one-step 'matched' run with momentum reads `diff` before any write)
        with torch.no_grad():
            for i in range(T - 1, -1, -1):
                slot = T - i
                time = torch.Tensor([timesteps[i]]).expand(n)
                s = S.get_schedule_shift_time(time, m_t)
                x_in = S.perturb_shift(x_t, s)
                pred = model(x_in, time).sample
                shifted0 = x_in + pred
                x0_hat = torch.where(given, known, S.perturb_shift_inverse(shifted0, s))        # the projection: a select
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
