"""Host predictors of the device Philox draws of csrc/sched.hip (helpers only, numpy, no test functions).

Every draw of the scheduler kernels is one word of Philox4x32-10 (`philox4x32_10` of _dropout_ref.py, which restates
csrc/common.h `Philox::operator()`) at key = rng[0], counter = {idx, rng[1] * 8 + stream}; one function below per kernel rule,
each naming the line it restates.  tests/test_philox_ref_cpu.py checks them against scalar loops and wrong twins, and
tests/test_device_draws_gpu.py compares the kernels with them bit for bit.
"""
import numpy as np

from _dropout_ref import philox4x32_10

M64 = (1 << 64) - 1
STREAM_TIMESTEPS, STREAM_TRAIN_MASK, STREAM_SHIFT, STREAM_SAMPLER_T, STREAM_SAMPLER_NEXT = 0, 1, 2, 3, 4
_2P24 = np.float32(2.0 ** -24)


def words(key, offset, stream, idx):
    """uint32 [n, 4] (x, y, z, w) of the calls `idx`.  common.h `philox_at`: `ph(idx, rng[1] * 8 + (uint64_t)stream_id)` with
    `Philox ph(rng[0])`; the product and the sum are uint64 arithmetic, so they wrap mod 2^64."""
    return philox4x32_10(int(key) & M64, np.asarray(idx, dtype=np.uint64).reshape(-1), (int(offset) * 8 + int(stream)) & M64)


def u01(w):
    """float32 in [0, 1).  common.h `u01`: `(x >> 8) * (1.0f / 16777216.0f)` (both factors and the product are exact in fp32)."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * _2P24


def timestep_idx(key, offset, N, n_used):
    """int32 [N].  draw_timesteps_kernel: `r = philox_at(rng, 0, n); idx = (int)(((uint64_t)r.x * (uint64_t)n_used) >> 32)`."""
    x = words(key, offset, STREAM_TIMESTEPS, np.arange(N))[:, 0].astype(np.uint64)
    return ((x * np.uint64(n_used)) >> np.uint64(32)).astype(np.int32)


def degrade_uniforms(key, offset, stream, N, Cm, HW):
    """float32 [N, Cm * HW].  degrade_kernel, both branches: `e = ((uint64_t)img * Cm + cm) * HW + p; r = philox_at(rng,
    rng_stream, e >> 2); w = lane e & 3 of (r.x, r.y, r.z, r.w); uv = u01(w)` (the LDS branch writes the four lanes of call q
    to elements 4 q .. 4 q + 3, which is the same rule)."""
    E = N * Cm * HW
    w = words(key, offset, stream, np.arange((E + 3) >> 2))
    return u01(w.reshape(-1)[:E]).reshape(N, Cm * HW)


def degrade_keep(u, amount):
    """float32 [N, Cm * HW] of 0 / 1.  degrade_kernel: `((double)uv > thr) ? 1.f : 0.f` with thr = amount[img] (fp64)."""
    return (np.asarray(u, dtype=np.float64) > np.asarray(amount, dtype=np.float64).reshape(-1, 1)).astype(np.float32)


def index_keep(key, offset, stream, N, HW, counts):
    """float32 [N, HW] of 0 / 1.  index_mask_kernel: `keys[p] = philox_at(rng, rng_stream, (uint64_t)img * HW + p).x;
    rank = #{q: keys[q] < keys[p] || (keys[q] == keys[p] && q < p)}; k = rank < (int)count[img] ? 0.f : 1.f`."""
    keys = words(key, offset, stream, np.arange(N * HW))[:, 0].reshape(N, HW)
    keep = np.ones((N, HW), dtype=np.float32)
    for img in range(N):
        order = np.argsort(keys[img], kind="stable")          # by (key, p)
        keep[img, order[:max(0, int(counts[img]))]] = 0.0      # (int) of a double truncates toward zero
    return keep


def shift_uniform_z(key, offset, stream, kind, N):
    """float32 [N] (kind 1) / [N, 3] (kind 2).  shift_kernel: `zi = n` / `n * 3 + c; q = philox_at(rng, rng_stream, zi >> 1);
    zv = u01((zi & 1) ? q.z : q.x) * 2.f - 1.f` (u * 2 is exact, so a fused multiply-add rounds the same once)."""
    nz = N * (3 if kind == 2 else 1)
    zi = np.arange(nz)
    w = words(key, offset, stream, np.arange((nz + 1) >> 1))[zi >> 1]
    u = u01(np.where(zi & 1, w[:, 2], w[:, 0]))
    z = (u * np.float32(2.0)).astype(np.float32) - np.float32(1.0)
    return z.astype(np.float32).reshape((N, 3) if kind == 2 else (N,))


def shift_normal_z(key, offset, stream, kind, N, HW, dtype):
    """`dtype` [N, 1, HW] (kind 3) / [N, 3, HW] (kinds 4, 5): the standard normal draw g of every z element, without mean or
    ratio.  shift_kernel: `zi = n * HW + p` / `(n * 3 + c) * HW + p; q = philox_at(rng, rng_stream, zi >> 1);
    g = box_muller(q.x, q.y); (zi & 1) ? g.y : g.x`, and common.h `box_muller`: `u1 = ((a >> 8) + 1) * 2^-24; u2 = u01(b);
    r = sqrtf(-2.f * __logf(u1)); __sincosf(6.2831853f * u2, &s, &c); return (r * c, r * s)`.  Evaluated wholly in `dtype`,
    2 pi included: float64 is the reference, float32 the rounding floor of the same formula."""
    dt = np.dtype(dtype).type
    zc = 1 if kind == 3 else 3
    nz = N * zc * HW
    zi = np.arange(nz)
    w = words(key, offset, stream, np.arange((nz + 1) >> 1))[zi >> 1]
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.uint32) + np.uint32(1)).astype(dt) * dt(2.0 ** -24)
    u2 = u01(w[:, 1]).astype(dt)
    r = np.sqrt(dt(-2.0) * np.log(u1))
    ang = dt(2.0 * np.pi) * u2
    g = np.where(zi & 1, r * np.sin(ang), r * np.cos(ang))
    assert g.dtype == np.dtype(dtype)
    return g.reshape(N, zc, HW)


def shift_normal_s(g, kind, ratio, noise_mean):
    """The shift of a normal kind from its draws g [N, zc, HW] in g's dtype; `ratio` broadcasts against g ([N, 1, 1], or
    ratio[p % W] as [1, 1, HW] under per_column).  shift_kernel: kinds 3, 4 `zv = g + noise_mean; sv = (float)((double)zv * rt)`,
    kind 5 `sv = (float)((double)noise_mean + (double)g * ratio[n])`."""
    dt = g.dtype.type
    ratio = np.asarray(ratio, dtype=np.float64)
    if kind == 5:
        return (np.float64(noise_mean) + g.astype(np.float64) * ratio).astype(dt)
    return ((g + dt(noise_mean)).astype(np.float64) * ratio).astype(dt)


def step_params(timesteps, T, step):
    """(t, t_next).  sampler_step_kernel: `i = T - 1 - step; t = timesteps[i < 0 ? 0 : i]; tn = i > 0 ? t - 1 : t`."""
    i = T - 1 - step
    t = int(timesteps[0 if i < 0 else i])
    return t, (t - 1 if i > 0 else t)
