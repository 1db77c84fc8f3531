"""The device Philox draws of csrc/sched.hip, predicted on the host and compared bit for bit.

Every kernel that draws -- mdm_draw_timesteps, mdm_degrade, mdm_index_mask, mdm_shift -- is called through the C ABI with the
`rng` words set directly, and its output is compared with tests/_philox_ref.py (kept honest by tests/test_philox_ref_cpu.py, which
also shows that each assertion here rejects a wrong lane, stream id, offset fold, 32-bit offset, swapped Box-Muller pair or
unshifted index).  Three states, all with a live high key word: offset 1; 2^29 + 3, where offset * 8 reaches counter word 3;
2^61 + 5, where offset * 8 wraps mod 2^64 as philox_at's uint64 arithmetic does.  Every output starts as NaN or a sentinel, and
no mask, index, timestep or uniform-shift comparison leaves an element out.

Bounds that are not equalities:
  * data-dependent fills (`_fill_bound`): the summation bound of tests/test_monitor_gpu.py restated for degrade_kernel -- a term
    passes through ceil(HW / 256) serial additions in its thread, 6 wave levels and 2 levels over the four waves, mode 1 adds C
    more (the channels' sums), and one division follows: |error| <= (ceil(HW/256) + 8 + [C] + 1) 2^-24 sum|terms| / count
    + 2^-23 |fill|.  Derived, not tuned.
  * normal shifts: the reference is the float64 Box-Muller of the same words; E32 is the largest |float32 - float64| value of that
    formula over this file's own normal draws (computed below, not hard-coded), and |s - s64| <= ratio 64 E32 + 2^-23 |s64|.
    The 64 covers the device's __logf / __sincosf, whose accuracy is not stated anywhere; what a run measures is written with
    tests/_notes.note and kept in profiles/r17_device_draws.md.

The tie rule of index_mask_kernel (equal keys: the lower pixel first) stays untested on the device: equal keys cannot be injected
through the ABI.  The host predictor's tie rule is checked on planted keys in test_philox_ref_cpu.py.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _philox_ref as R  # noqa: E402
from _notes import note  # noqa: E402
from golden.make_golden import TINY, base_args  # noqa: E402

KEY = (0x9E3779B9 << 32) | 12345
STATES = [1, 2 ** 29 + 3, 2 ** 61 + 5]
NAN = float("nan")


def _rng(key, offset):
    return torch.from_numpy(np.array([key, offset], dtype=np.uint64).view(np.int64)).cuda()


def _state(t):
    """(key, offset) of an rng tensor as unsigned Python ints."""
    k, o = t.cpu().numpy().view(np.uint64).tolist()
    return int(k), int(o)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cached references stay read-only


def host(t):
    return t.cpu().numpy()


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, device="cuda", dtype=dtype)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _call(name, *args):
    from mdm._lib import call, stream
    call(name, *args, stream())
    torch.cuda.synchronize()


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------ timesteps
@pytest.mark.parametrize("offset", STATES)
@pytest.mark.parametrize("N", [1, 300])
@pytest.mark.parametrize("n_used", [1, 7, 1000])
@pytest.mark.parametrize("with_w", [False, True])
def test_draw_timesteps(offset, N, n_used, with_w):
    """N = 300: two workgroups, the second with a tail.  `used` skips values, so idx, used[idx] and table[t - 1] cannot be
    confused with one another."""
    g = np.random.default_rng(1000 * n_used + N)
    used = (3 * np.arange(n_used) + 2 + (np.arange(n_used) % 2)).astype(np.int32)
    L = int(used.max())
    table, table2 = g.random(L), g.random(L)
    wtab = (g.random(n_used) + 0.5).astype(np.float32)
    rng, d_used, d_tab, d_tab2, d_w = _rng(KEY, offset), dev(used), dev(table), dev(table2), dev(wtab)
    t_out, w_out = _full((N,), NAN), _full((N,), NAN)
    amount, out2 = _full((N,), NAN, torch.float64), _full((N,), NAN, torch.float64)
    idx = _full((N,), -1, torch.int32)
    zero = torch.tensor([0x5A5A5A5A5A5A, -7], device="cuda", dtype=torch.int64)
    _call("mdm_draw_timesteps", _p(rng), _p(d_used), n_used, _p(d_tab), _p(d_w) if with_w else None, N, _p(t_out), _p(amount),
          _p(w_out), _p(idx), _p(d_tab2), _p(out2), _p(zero))
    want = R.timestep_idx(KEY, offset, N, n_used)
    t = used[want]
    assert np.array_equal(host(idx), want)
    assert np.array_equal(host(t_out), t.astype(np.float32))
    assert np.array_equal(host(amount), table[t - 1]) and np.array_equal(host(out2), table2[t - 1])
    assert np.array_equal(_bits(host(w_out)), _bits(wtab[want] if with_w else np.ones(N, dtype=np.float32)))
    assert zero.tolist() == [0, 0]
    assert _state(rng) == (KEY, offset)                         # the state is only read
    idx2 = _full((N,), -1, torch.int32)                         # every optional output but idx_out NULL
    _call("mdm_draw_timesteps", _p(rng), _p(d_used), n_used, _p(d_tab), None, N, None, None, None, _p(idx2), None, None, None)
    assert np.array_equal(host(idx2), want)


# ------------------------------------------------------------------------------------------ drawn masks
@functools.lru_cache(maxsize=None)
def _uniforms(key, offset, stream_id, N, Cm, HW):
    u = R.degrade_uniforms(key, offset, stream_id, N, Cm, HW)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _x0(N, C, HW):
    x = (np.random.default_rng(N * 100003 + C * 1009 + HW).random((N, C, HW), dtype=np.float32) * 2 - 1).astype(np.float32)
    x.setflags(write=False)
    return x


def _amounts(N, k):
    """Image 0 always draws at 0.3 (not an fp32 number); images 1 and 2 meet 0.0 and 1.0 over the three states."""
    A = [0.3, 0.0, 1.0, 0.55, 0.7]
    return np.array([A[(i * (k + 1)) % 5] for i in range(N)], dtype=np.float64)


def _degrade(x0, amount, stride, rng, stream_id, Cm, mode, fill_const, u=None, mask_in=None):
    N, C, HW = x0.shape
    x_t, mask, mp = _full((N, C, HW), NAN), _full((N, C, HW), NAN), _full((N, C), NAN)
    _call("mdm_degrade", _p(x0), _p(u), _p(mask_in), _p(amount), stride, _p(rng), stream_id, N, C, HW, Cm, mode, fill_const,
          _p(x_t), _p(mask), _p(mp))
    return host(x_t), host(mask), host(mp)


def _mask_ncp(keep, N, C, Cm, HW):
    return np.ascontiguousarray(np.broadcast_to(keep.reshape(N, Cm, HW), (N, C, HW)))


DRAWN = [(3, 3, 8, 8, 1), (3, 3, 8, 8, 3),            # LDS path, fewer elements than threads
         (2, 3, 5, 7, 1), (2, 3, 5, 7, 3),            # HW = 35: direct path, image boundaries inside a Philox call
         (2, 1, 37, 37, 1),                           # HW = 1369 > 1024: integer-division branch, threads loop
         (1, 3, 128, 128, 3),                         # Cm * HW = 49152: LDS path at exactly 48 KiB
         (1, 1, 224, 224, 1),                         # 50176 > 48 KiB with HW % 4 == 0: direct path
         (2, 8, 16, 16, 8)]                           # C = 8, the kernel's maximum


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("case", DRAWN)
@pytest.mark.parametrize("stride", [1, 0])
def test_drawn_mask(k, case, stride):
    N, C, H, W, Cm = case
    HW, offset = H * W, STATES[k]
    x0h = _x0(N, C, HW)
    amount = _amounts(N, k)
    eff = amount if stride == 1 else np.repeat(amount[:1], N)
    u = _uniforms(KEY, offset, 1, N, Cm, HW)
    want = _mask_ncp(R.degrade_keep(u, eff), N, C, Cm, HW)
    x0, rng, d_amount = dev(x0h), _rng(KEY, offset), dev(amount)
    x_t, mask, mp = _degrade(x0, d_amount, stride, rng, 1, Cm, 0, 0.25)
    assert np.array_equal(_bits(mask), _bits(want)), f"{int((mask != want).sum())} of {mask.size} mask elements differ"
    assert np.array_equal(x_t, np.where(want > 0, x0h, np.float32(0.25)))
    assert np.array_equal(mp, np.full((N, C), 0.25, dtype=np.float32))
    assert _state(rng) == (KEY, offset)
    # replay path: the predicted uniforms handed in as `u` (rng NULL)
    x_t2, mask2, mp2 = _degrade(x0, d_amount, stride, None, 1, Cm, 0, 0.25, u=dev(u))
    assert np.array_equal(_bits(mask2), _bits(mask)) and np.array_equal(_bits(x_t2), _bits(x_t)) and np.array_equal(mp2, mp)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("case", [(3, 3, 8, 8, 3), (2, 3, 5, 7, 1)])
def test_mask_streams_are_their_own(k, case):
    """Streams 1 (training), 3 and 4 (the sampler's t and t - 1) at one state: each is its own prediction, no two agree."""
    N, C, H, W, Cm = case
    HW, offset = H * W, STATES[k]
    x0, rng, amount = dev(_x0(N, C, HW)), _rng(KEY, offset), np.full(N, 0.5)
    got = {}
    for sid in (1, 3, 4):
        _, mask, _ = _degrade(x0, dev(amount), 1, rng, sid, Cm, 0, 0.25)
        want = _mask_ncp(R.degrade_keep(_uniforms(KEY, offset, sid, N, Cm, HW), amount), N, C, Cm, HW)
        assert np.array_equal(_bits(mask), _bits(want)), sid
        got[sid] = mask
    for a, b in ((1, 3), (1, 4), (3, 4)):
        assert np.mean(got[a] != got[b]) > 0.25, (a, b)         # independent fair coins disagree on half


# ------------------------------------------------------------------------------------------ data-dependent fills
def _fill_bound(mode, C, HW, sum_abs, count, fill):
    levels = -(-HW // 256) + 8 + (C if mode == 1 else 0) + 1
    return levels * 2.0 ** -24 * sum_abs / count + 2.0 ** -23 * abs(fill)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("case", [(3, 3, 8, 8, 1), (2, 3, 37, 37, 3)])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_data_dependent_fill(k, case, mode):
    """mean_pixel against the fp64 value over the PREDICTED mask.  The last image draws at amount 0 over an all-zero x0: nothing
    is degraded and the kept sum is 0, so mode 3's fill is -(0 / 0) and must come out 0 (scheduler.py:314), modes 1 and 2 give
    the reference's NaN (0 / 0, scheduler.py:305, 309).  With three images, image 1 also draws at amount 0 over a non-zero x0:
    mode 3's fill is then -(sum / 0) = -+inf exactly as upstream, which the NaN rule leaves alone."""
    N, C, H, W, Cm = case
    HW, offset = H * W, STATES[k]
    x0h = _x0(N, C, HW).copy()
    x0h[N - 1] = 0.0
    amount = np.array([0.3, 0.0, 0.0][:N] if N == 3 else [0.3, 0.0], dtype=np.float64)
    keep = _mask_ncp(R.degrade_keep(_uniforms(KEY, offset, 1, N, Cm, HW), amount), N, C, Cm, HW).astype(np.float64)
    x_t, mask, mp = _degrade(dev(x0h), dev(amount), 1, _rng(KEY, offset), 1, Cm, mode, 0.0)
    assert np.array_equal(_bits(mask), _bits(keep.astype(np.float32)))
    x64 = x0h.astype(np.float64)
    terms = x64 * keep if mode == 3 else x64 * (1 - keep)
    gone = 1 - keep
    for img in range(N):
        for c in range(C):
            sel = (img, slice(None)) if mode == 1 else (img, c)
            s, sa, cnt = terms[sel].sum(), np.abs(terms[sel]).sum(), gone[sel].sum()
            with np.errstate(divide="ignore", invalid="ignore"):
                want = np.float64(s) / np.float64(cnt) * (-1.0 if mode == 3 else 1.0)
            if mode == 3 and np.isnan(want):
                want = 0.0
            got = float(mp[img, c])
            if cnt == 0:            # nothing degraded: x / 0 has no rounding -- NaN, an infinity of the sum's sign, or mode 3's 0
                assert (np.isnan(got) and np.isnan(want)) or got == want, (img, c, got, want)
                continue
            bound = _fill_bound(mode, C, HW, sa, cnt, want)
            assert abs(got - want) <= bound, (img, c, got, want, abs(got - want), bound)
    assert np.isfinite(mp[0]).all() and (mode != 3 or np.array_equal(mp[N - 1], np.zeros(C, dtype=np.float32)))
    with np.errstate(invalid="ignore"):
        k32 = keep.astype(np.float32)
        want_xt = (np.float32(1) - k32) * mp[:, :, None] + k32 * x0h       # one of the two products is always 0 or exact
    assert np.array_equal(x_t, want_xt, equal_nan=True)


# ------------------------------------------------------------------------------------------ index masks
def _count_sets(N, HW):
    vals = [0.0, 1.0, float(HW), float(HW // 2), 5.9]           # 5.9 truncates to 5
    return [[vals[(j * N + i) % 5] for i in range(N)] for j in range(-(-5 // N))]


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("case", [(3, 3, 64), (2, 1, 1369), (1, 3, 16384)])     # 16384 keys: the 64 KiB LDS limit
@pytest.mark.parametrize("stride", [1, 0])
def test_index_mask(k, case, stride):
    N, C, HW = case
    offset = STATES[k]
    x0h = _x0(N, C, HW)
    x0, rng = dev(x0h), _rng(KEY, offset)
    for counts in _count_sets(N, HW):
        eff = counts if stride == 1 else counts[:1] * N
        want = R.index_keep(KEY, offset, 3, N, HW, eff)
        mask = _full((N, C, HW), NAN)
        _call("mdm_index_mask", _p(dev(np.array(counts, dtype=np.float64))), stride, _p(rng), 3, N, C, HW, _p(mask))
        got = host(mask)
        assert np.array_equal(_bits(got), _bits(_mask_ncp(want, N, C, 1, HW))), (counts, int((got[:, 0] != want).sum()))
        assert [int((got[i, 0] == 0).sum()) for i in range(N)] == [min(HW, int(c)) for c in eff]
        x_t, mask2, mp = _degrade(x0, None, 1, None, 3, C, 0, 0.25, mask_in=mask)
        assert np.array_equal(x_t, np.where(got > 0, x0h, np.float32(0.25))) and np.array_equal(_bits(mask2), _bits(got))
        assert np.array_equal(mp, np.full((N, C), 0.25, dtype=np.float32))
    assert _state(rng) == (KEY, offset)


# ------------------------------------------------------------------------------------------ shift
SHIFT = ([(kind, (4, 3, 8, 8), 0) for kind in range(6)]
         + [(kind, (3, 3, 5, 7), 0) for kind in range(6)]        # odd HW: draw pairs straddle channel and image boundaries
         + [(1, (2, 1, 5, 7), 0)]
         + [(kind, (8, 3, 8, 8), pc) for kind in (3, 4) for pc in (1, 0)])
NOISE_MEAN = 0.25
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _normals(offset, kind, N, HW):
    return tuple(R.shift_normal_z(KEY, offset, 2, kind, N, HW, dt) for dt in (np.float32, np.float64))


@functools.lru_cache(maxsize=None)
def _e32():
    """The rounding floor: the largest |float32 - float64| Box-Muller value over every normal draw this file predicts."""
    worst, n = 0.0, 0
    for kind, (N, C, H, W), pc in SHIFT:
        if kind >= 3 and pc == 0:
            for offset in STATES:
                z32, z64 = _normals(offset, kind, N, H * W)
                worst, n = max(worst, float(np.abs(z32.astype(np.float64) - z64).max())), n + z64.size
    print(f"E32 = {worst:.4e} over {n} draws")
    return worst


def _shift(x_t, ratio, rng, kind, per_col, shape, dt, want_s=True, want_x=True, want_nhwc=True):
    N, C, H, W = shape
    s = _full(shape, NAN) if want_s else None
    x_in = _full(shape, NAN) if want_x else None
    nhwc = _full((N, H * W, 8), SENTINEL, torch.float32 if dt == 0 else torch.bfloat16) if want_nhwc else None
    _call("mdm_shift", _p(x_t), None, _p(ratio), _p(rng), 2, kind, NOISE_MEAN, per_col, N, C, H, W, _p(s), _p(x_in), dt, _p(nhwc),
          8 if want_nhwc else 0)
    return (None if s is None else host(s)), (None if x_in is None else host(x_in)), nhwc


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("case", SHIFT, ids=lambda c: f"kind{c[0]}-{'x'.join(map(str, c[1]))}-pc{c[2]}")
def test_shift(k, case):
    kind, shape, per_col = case
    N, C, H, W = shape
    HW, offset = H * W, STATES[k]
    g = np.random.default_rng(17 * N + HW)
    ratio = g.random(N) * 0.9 + 0.1                             # fp64, not fp32 numbers
    assert not np.any(ratio == ratio.astype(np.float32))
    x_th = (g.random(shape, dtype=np.float32) * 2 - 1).astype(np.float32)
    x_t, rng, d_ratio = dev(x_th), _rng(KEY, offset), (dev(ratio) if kind else None)
    s, x_in, nhwc = _shift(x_t, d_ratio, rng if kind else None, kind, per_col, shape, 0)
    assert _state(rng) == (KEY, offset)
    s4 = s.reshape(N, C, HW)
    relem = np.broadcast_to(ratio[np.arange(HW) % W].reshape(1, 1, HW) if per_col else ratio.reshape(N, 1, 1), (N, C, HW))
    if kind == 0:
        assert not _bits(s).any()
    elif kind in (1, 2):            # exact: s = fl32(float64(z) * ratio)
        z = R.shift_uniform_z(KEY, offset, 2, kind, N).reshape(N, -1, 1)
        want = np.broadcast_to((z.astype(np.float64) * ratio.reshape(N, 1, 1)).astype(np.float32), (N, C, HW))
        assert np.array_equal(_bits(s4), _bits(want)), f"{int((s4 != want).sum())} of {s4.size} differ"
    else:
        z32, z64 = _normals(offset, kind, N, HW)
        e32 = _e32()
        rz = relem[:, :z64.shape[1]]                            # the ratio of every z element ([N, 1 | 3, HW])
        s64z = R.shift_normal_s(z64, kind, rz, NOISE_MEAN)
        s64 = np.broadcast_to(s64z, (N, C, HW))
        err = np.abs(s4.astype(np.float64) - s64)
        bound = relem * 64 * e32 + 2.0 ** -23 * np.abs(s64)
        worst = float((err / relem).max() / e32)
        floor = float((np.abs(R.shift_normal_s(z32, kind, rz, NOISE_MEAN).astype(np.float64) - s64z) / rz).max() / e32)
        print(f"kind {kind} {shape} pc {per_col} offset {offset}: max |s - s64| / ratio = {worst:.3f} E32 (host fp32 {floor:.3f} E32), allowed 64")
        note("device_draws_shift_normal", dict(kind=kind, shape=list(shape), per_column=per_col, offset=offset, e32=e32,
                                              err_over_e32=worst, host_fp32_over_e32=floor, n=int(z64.size)))
        assert np.isfinite(s4).all() and bool((err <= bound).all()), (worst, int((err > bound).sum()))
        if kind == 3:
            assert np.array_equal(_bits(s4[:, 0]), _bits(s4[:, 1])) and np.array_equal(_bits(s4[:, 0]), _bits(s4[:, 2]))
    # every kind: x_in = fl32(x_t + s), its NHWC copy, the pad channels
    want_x = x_th + s
    assert want_x.dtype == np.float32 and np.array_equal(_bits(x_in), _bits(want_x))
    want_nhwc = torch.from_numpy(want_x.reshape(N, C, HW).transpose(0, 2, 1).copy())
    nh = nhwc.cpu()
    assert torch.equal(nh[..., :C].contiguous().view(torch.int32), want_nhwc.view(torch.int32))
    assert bool((nh[..., C:] == SENTINEL).all())
    # s NULL with a bf16 NHWC copy; x_in NULL; both NULL but the NHWC copy
    _, x_in2, nhwc2 = _shift(x_t, d_ratio, rng if kind else None, kind, per_col, shape, 1, want_s=False)
    assert np.array_equal(_bits(x_in2), _bits(x_in))
    nh2 = nhwc2.cpu()
    assert torch.equal(nh2[..., :C].contiguous().view(torch.int16), want_nhwc.to(torch.bfloat16).view(torch.int16))     # round to nearest even
    assert bool((nh2[..., C:] == SENTINEL).all())
    s3, _, _ = _shift(x_t, d_ratio, rng if kind else None, kind, per_col, shape, 0, want_x=False, want_nhwc=False)
    assert np.array_equal(_bits(s3), _bits(s))


# ------------------------------------------------------------------------------------------ offset and step parameters
def test_rng_advance_carries_into_the_high_word():
    rng = _rng(KEY, 2 ** 32 - 1)
    _call("mdm_rng_advance", _p(rng))
    assert _state(rng) == (KEY, 2 ** 32)
    rng = _rng(KEY, 2 ** 64 - 1)                                # uint64 wrap, as philox_at's own arithmetic
    _call("mdm_rng_advance", _p(rng))
    assert _state(rng) == (KEY, 0)


@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("with_ratio", [True, False])
def test_sampler_step_params(n, with_ratio):
    ts, T = [1, 4, 9, 20, 41], 5
    g = np.random.default_rng(41)
    ratio_tab, amount_tab = g.random(41), g.random(41)
    d_ts, d_rt, d_at = dev(np.array(ts, dtype=np.int32)), dev(ratio_tab), dev(amount_tab)
    ctr = torch.zeros(1, device="cuda", dtype=torch.int32)
    offset = 2 ** 32 - 3                                        # the five bumps cross the 32-bit carry
    rng = _rng(KEY, offset)
    for step in range(T):
        time = _full((n,), NAN)
        r_out, a_t, a_n = (_full((n,), NAN, torch.float64) for _ in range(3))
        _call("mdm_sampler_step_params", _p(d_ts), T, _p(ctr), _p(d_rt) if with_ratio else None, _p(d_at), n, _p(time),
              _p(r_out) if with_ratio else None, _p(a_t), _p(a_n), _p(rng))
        t, tn = R.step_params(ts, T, step)
        assert tn == (t - 1 if step < T - 1 else t)
        assert np.array_equal(host(time), np.full(n, t, dtype=np.float32))
        assert np.array_equal(host(a_t), np.full(n, amount_tab[t - 1])) and np.array_equal(host(a_n), np.full(n, amount_tab[tn - 1]))
        if with_ratio:
            assert np.array_equal(host(r_out), np.full(n, ratio_tab[t - 1]))
        else:
            assert bool(torch.isnan(r_out).all())
        assert ctr.item() == step + 1 and _state(rng) == (KEY, offset + step + 1)


# ------------------------------------------------------------------------------------------ Python wiring
def test_scheduler_methods_draw_from_their_streams():
    """Scheduler(rng_mode="device", seed=77, rng_rank=3) after two advance(): key = 77 | 3 << 32, offset 2; degrade_training is
    stream 1, shift_and_perturb stream 2, the sampler's masks stream 3 -- the nested pair one draw thresholded at two amounts."""
    from mdm import Scheduler
    N, C, H, W = 3, 3, 8, 8
    HW = H * W
    key = 77 | 3 << 32
    x0h = _x0(N, C, HW).reshape(N, C, H, W)
    x0 = torch.from_numpy(x0h.copy())
    amount = np.array([0.3, 0.55, 0.0])
    nxt = np.array([0.2, 0.55, 0.7])
    for channel, Cm in (("1-channel", 1), ("3-channel", 3)):
        a = base_args(data_size=H, ddpm_num_steps=10, rng_mode="device", seed=77, rng_rank=3, shift_type="1-d_constant",
                      degrade_channel=channel)
        S = Scheduler(a)
        S.update_ddpm_num_steps(10)
        S.dev_rng.advance()
        S.dev_rng.advance()
        torch.cuda.synchronize()
        assert _state(S.dev_rng.dev) == (key, 2)

        def want(sid, amt):
            return _mask_ncp(R.degrade_keep(_uniforms(key, 2, sid, N, Cm, HW), amt), N, C, Cm, HW).reshape(N, C, H, W)
        x_t, m, _, _ = S.degrade_training(torch.from_numpy(amount), x0, mean_option=0, mean_area="image-wise")
        assert np.array_equal(_bits(host(m)), _bits(want(1, amount)))
        assert np.array_equal(host(x_t), np.where(want(1, amount) > 0, x0h, np.float32(0)))
        x_t, m, _ = S.degrade_independent_base_sampling(torch.from_numpy(amount), x0, mean_option=0, mean_area="image-wise")
        assert np.array_equal(_bits(host(m)), _bits(want(3, amount)))
        assert np.array_equal(host(x_t), np.where(want(3, amount) > 0, x0h, np.float32(0)))
        out = S.degrade_dependent_base_sampling(torch.from_numpy(amount), torch.from_numpy(nxt), x0, "0", "image-wise")
        assert np.array_equal(_bits(host(out[1])), _bits(want(3, amount))) and np.array_equal(_bits(host(out[4])), _bits(want(3, nxt)))
        assert np.array_equal(host(out[3]), np.where(want(3, nxt) > 0, x0h, np.float32(0)))
        t = torch.tensor([3.0, 7.0, 10.0])
        s, x_in = S.shift_and_perturb(t.cuda(), x_t)
        ratio = S.ratio_list.numpy()[[2, 6, 9]]
        z = R.shift_uniform_z(key, 2, 2, 1, N)
        want_s = np.broadcast_to((z.astype(np.float64) * ratio).astype(np.float32).reshape(N, 1, 1, 1), (N, C, H, W))
        assert np.array_equal(_bits(host(s)), _bits(want_s))
        assert np.array_equal(_bits(host(x_in)), _bits(host(x_t) + want_s))
        assert _state(S.dev_rng.dev) == (key, 2)                # the methods draw, only advance() moves the offset


def test_train_step_draws_are_predicted():
    """One eager fp32 device-RNG train step with the set-up of test_device_path_gpu.py's oracle replay (TINY, n = 4, 16 x 16):
    the timestep indices and the keep-mask it left behind are the host prediction from the state read back after the step."""
    import mdm
    from oracle.unet_ref import random_params
    n, hw, T = 4, 16, 50
    a = base_args(data_size=hw, ddpm_schedule="linear", ddpm_num_steps=T, shift_type="noise_with_perturbation", noise_mean=0.25,
                  rng_mode="device", loss_weight_use=True, batch_size=n, use_graph=False, seed=9)
    model = mdm.UNet(TINY, N=n, H=hw, W=hw, dtype=mdm.F32, params=random_params(TINY), use_graph=False)
    opt = mdm.AdamW(model, lr=1e-3)
    tr = mdm.Trainer(a, None, None, [None] * 3, model, None, opt, mdm.get_lr_scheduler("constant", opt, 0, 1), mdm.Accelerator())
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(T)
    used = tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    x0 = torch.rand(n, 3, hw, hw, generator=torch.Generator().manual_seed(21)) * 2 - 1
    tr._run_batch(0, (x0, None, None), 0, 1, 0, None, None)
    torch.cuda.synchronize()
    key, offset = _state(tr.Scheduler.dev_rng.dev)
    assert (key, offset) == (9, 1)                              # seed 9, rank 0; the step's first launch bumped the offset once
    st = tr.step
    tidx = R.timestep_idx(key, offset, n, len(used))
    assert np.array_equal(host(st.tidx), tidx)
    assert np.array_equal(host(model.t_in), np.array(used)[tidx].astype(np.float32))
    amount = host(st.amount)
    assert np.array_equal(amount, tr.Scheduler.ratio_list.numpy()[np.array(used)[tidx] - 1])
    want = _mask_ncp(R.degrade_keep(R.degrade_uniforms(key, offset, 1, n, 1, hw * hw), amount), n, 3, 1, hw * hw)
    assert np.array_equal(_bits(host(st.mask).reshape(n, 3, hw * hw)), _bits(want))
    # the shift of this step: stream 2, kind 4, within the normal-shift bound of this file
    z32, z64 = (R.shift_normal_z(key, offset, 2, 4, n, hw * hw, dt) for dt in (np.float32, np.float64))
    per_col = n == hw
    assert not per_col
    ratio = host(st.ratio).reshape(n, 1, 1)
    s64 = R.shift_normal_s(z64, 4, ratio, 0.25)
    e32 = float(np.abs(z32.astype(np.float64) - z64).max())
    err = np.abs(host(st.s).reshape(n, 3, hw * hw).astype(np.float64) - s64)
    assert bool((err <= ratio * 64 * e32 + 2.0 ** -23 * np.abs(s64)).all()), float((err / ratio).max() / e32)
