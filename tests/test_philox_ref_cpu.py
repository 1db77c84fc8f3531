"""Keeps tests/_philox_ref.py honest without a GPU: the published Philox4x32-10 known-answer vectors, every vectorised predictor
against a scalar loop that follows its kernel in csrc/sched.hip line by line, and -- the reason the GPU assertions of
tests/test_device_draws_gpu.py mean something -- a deliberately wrong twin of every rule, which those assertions must reject:

    lanes    lane e & 3 rotated by one (degrade); the x / z words of a call swapped (uniform shift)
    stream   stream id off by one
    no_x8    offset not multiplied by 8
    trunc32  offset * 8 + stream kept to 32 bits (shows where offset * 8 reaches counter word 3: the state 2^29 + 3)
    cossin   the cos / sin halves of a Box-Muller pair swapped
    unshift  element index used as the call index (e instead of e >> 2, zi instead of zi >> 1)

Masks (amount 0.5; index masks at count HW / 2; timestep indices of 1000) must differ on >= 40 % of the elements, uniforms on
>= 95 %, and normals by more than 100 x the GPU test's bound (64 E32 + 2^-23 |z|, ratio 1) on >= 95 % of the elements.
"""
import functools
import math

import numpy as np
import pytest

import _philox_ref as R
from _dropout_ref import philox4x32_10

KEY = (0x9E3779B9 << 32) | 12345
STATES = [1, 2 ** 29 + 3, 2 ** 61 + 5]
SHAPES = [(2, 3, 5, 7), (3, 3, 8, 8)]
M64 = (1 << 64) - 1


def test_known_answer_vectors():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter words, key words -> output words."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for c, k, want in kat:
        got = philox4x32_10(k[0] | k[1] << 32, np.array([c[0] | c[1] << 32], dtype=np.uint64), c[2] | c[3] << 32)
        assert got.dtype == np.uint32 and tuple(int(v) for v in got[0]) == want, ([hex(int(v)) for v in got[0]], [hex(v) for v in want])
    # `words` places offset * 8 + stream in counter words 2, 3 and the call index in words 0, 1
    c = kat[2][0]
    off8 = c[2] | c[3] << 32
    got = R.words(kat[2][1][0] | kat[2][1][1] << 32, off8 >> 3, off8 & 7, [c[0] | c[1] << 32])
    assert tuple(int(v) for v in got[0]) == kat[2][2]


# ---------------------------------------------------------------------------- the kernels as scalar loops (with the twins' bugs)
@functools.lru_cache(maxsize=None)
def _call(key, lo, hi):
    return tuple(int(v) for v in philox4x32_10(key, np.array([lo], dtype=np.uint64), hi)[0])


def _at(key, offset, stream, idx, bug):
    """common.h philox_at: ph(idx, rng[1] * 8 + stream_id), uint64."""
    if bug == "stream":
        stream += 1
    hi = (offset + stream if bug == "no_x8" else offset * 8 + stream) & M64
    if bug == "trunc32":
        hi &= 0xFFFFFFFF
    return _call(key, idx, hi)


def _u01(w):
    return np.float32(w >> 8) * np.float32(1.0 / 16777216.0)


def loop_timesteps(key, offset, N, n_used, bug=None):
    return np.array([(_at(key, offset, 0, n, bug)[0] * n_used) >> 32 for n in range(N)], dtype=np.int32)


def loop_degrade_u(key, offset, stream, N, Cm, HW, bug=None):
    out = np.empty((N, Cm * HW), dtype=np.float32)
    for img in range(N):
        for cm in range(Cm):
            for p in range(HW):
                e = (img * Cm + cm) * HW + p
                r = _at(key, offset, stream, e if bug == "unshift" else e >> 2, bug)
                out[img, cm * HW + p] = _u01(r[(e + 1) & 3 if bug == "lanes" else e & 3])
    return out


def loop_index_keep(key, offset, stream, N, HW, counts, bug=None):
    out = np.empty((N, HW), dtype=np.float32)
    for img in range(N):
        keys = [_at(key, offset, stream, img * HW + p, bug)[0] for p in range(HW)]
        cnt = int(counts[img])
        for p in range(HW):
            rank = sum((keys[q] < keys[p]) or (keys[q] == keys[p] and q < p) for q in range(HW))
            out[img, p] = 0.0 if rank < cnt else 1.0
    return out


def loop_uniform_z(key, offset, stream, kind, N, bug=None):
    zc = 3 if kind == 2 else 1
    out = np.empty(N * zc, dtype=np.float32)
    for zi in range(N * zc):
        q = _at(key, offset, stream, zi if bug == "unshift" else zi >> 1, bug)
        odd = bool(zi & 1) != (bug == "lanes")
        out[zi] = np.float32(_u01(q[2] if odd else q[0]) * np.float32(2.0)) - np.float32(1.0)
    return out.reshape((N, 3) if kind == 2 else (N,))


def loop_normal_z(key, offset, stream, kind, N, HW, dtype, bug=None):
    dt = np.dtype(dtype).type
    zc = 1 if kind == 3 else 3
    out = np.empty(N * zc * HW, dtype=dtype)
    for zi in range(N * zc * HW):
        q = _at(key, offset, stream, zi if bug == "unshift" else zi >> 1, bug)
        u1 = dt((q[0] >> 8) + 1) * dt(1.0 / 16777216.0)
        u2 = dt(_u01(q[1]))
        r = np.sqrt(dt(-2.0) * np.log(u1))
        ang = dt(2.0 * math.pi) * u2
        gx, gy = r * np.cos(ang), r * np.sin(ang)
        if bug == "cossin":
            gx, gy = gy, gx
        out[zi] = gy if zi & 1 else gx
    return out.reshape(N, zc, HW)


# ---------------------------------------------------------------------------- predictors == scalar loops
@pytest.mark.parametrize("offset", STATES)
def test_timestep_idx_matches_the_loop(offset):
    for N, n_used in ((1, 1), (1, 1000), (70, 7), (70, 1000)):
        got = R.timestep_idx(KEY, offset, N, n_used)
        assert got.dtype == np.int32 and np.array_equal(got, loop_timesteps(KEY, offset, N, n_used))
        assert got.min() >= 0 and got.max() < n_used


@pytest.mark.parametrize("offset", STATES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("Cm", [1, 3])
def test_degrade_uniforms_match_the_loop(offset, shape, Cm):
    N, C, H, W = shape
    got = R.degrade_uniforms(KEY, offset, 1, N, Cm, H * W)
    want = loop_degrade_u(KEY, offset, 1, N, Cm, H * W)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.min() >= 0.0 and got.max() < 1.0
    amount = [0.3, 0.0, 1.0][:N]
    keep = R.degrade_keep(got, amount)
    for img in range(N):
        assert np.array_equal(keep[img], [1.0 if float(v) > amount[img] else 0.0 for v in want[img]])


@pytest.mark.parametrize("offset", STATES)
@pytest.mark.parametrize("shape", SHAPES)
def test_index_keep_matches_the_loop(offset, shape):
    N, C, H, W = shape
    HW = H * W
    for counts in ([0, 1, HW][:N], [HW // 2, 5.9, HW + 3][:N]):
        got = R.index_keep(KEY, offset, 3, N, HW, counts)
        assert np.array_equal(got, loop_index_keep(KEY, offset, 3, N, HW, counts))
        assert [int((got[i] == 0).sum()) for i in range(N)] == [min(HW, int(c)) for c in counts]


def test_index_keep_breaks_ties_by_pixel_index(monkeypatch):
    """Equal keys cannot come out of Philox on demand; the rule `keys[q] == kp && q < p` is checked on planted keys."""
    keys = np.array([5, 2, 5, 2, 9, 2], dtype=np.uint32)
    monkeypatch.setattr(R, "words", lambda key, offset, stream, idx: np.stack([keys] * 4, axis=1))
    for cnt, zeros in ((1, [1]), (2, [1, 3]), (3, [1, 3, 5]), (4, [0, 1, 3, 5])):
        got = R.index_keep(0, 0, 0, 1, 6, [cnt])
        assert sorted(np.flatnonzero(got[0] == 0).tolist()) == zeros


@pytest.mark.parametrize("offset", STATES)
@pytest.mark.parametrize("kind,N", [(1, 1), (1, 2), (1, 5), (2, 3), (2, 4)])
def test_shift_uniform_z_matches_the_loop(offset, kind, N):
    got = R.shift_uniform_z(KEY, offset, 2, kind, N)
    want = loop_uniform_z(KEY, offset, 2, kind, N)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)
    assert got.min() >= -1.0 and got.max() < 1.0


@pytest.mark.parametrize("offset", STATES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", [3, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shift_normal_z_matches_the_loop(offset, shape, kind, dtype):
    """The same numpy functions element by element; an array loop and a scalar call may round a transcendental differently,
    so the comparison allows 2 ulp of the result's own size class and no more."""
    N, C, H, W = shape
    got = R.shift_normal_z(KEY, offset, 2, kind, N, H * W, dtype)
    want = loop_normal_z(KEY, offset, 2, kind, N, H * W, dtype)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape
    eps = np.finfo(dtype).eps
    assert np.all(np.abs(got - want) <= 2 * eps * 8.0), float(np.abs(got - want).max())       # |g| < 5.8 < 8


def test_shift_normal_s_rules():
    g = np.array([[[0.5, -1.25]]], dtype=np.float32)
    ratio = np.array([0.3]).reshape(1, 1, 1)
    s34 = R.shift_normal_s(g, 4, ratio, 0.25)
    assert s34.dtype == np.float32 and np.array_equal(s34, np.array([[[0.75 * 0.3, -1.0 * 0.3]]]).astype(np.float32))
    s5 = R.shift_normal_s(g, 5, ratio, 0.25)
    assert np.array_equal(s5, np.array([[[0.25 + 0.5 * 0.3, 0.25 - 1.25 * 0.3]]]).astype(np.float32))
    assert R.shift_normal_s(g.astype(np.float64), 3, ratio, 0.25).dtype == np.float64


def test_step_params():
    ts = [1, 4, 9, 20, 41]
    assert [R.step_params(ts, 5, k) for k in range(7)] == [(41, 40), (20, 19), (9, 8), (4, 3), (1, 1), (1, 1), (1, 1)]


# ---------------------------------------------------------------------------- the wrong twins are rejected
def _states_for(bug):
    return [2 ** 29 + 3] if bug == "trunc32" else STATES


def _differ(a, b):
    return float(np.mean(np.asarray(a) != np.asarray(b)))


@pytest.mark.parametrize("bug", ["stream", "no_x8", "trunc32"])
def test_twin_timesteps(bug):
    for offset in _states_for(bug):
        right = R.timestep_idx(KEY, offset, 300, 1000)
        frac = _differ(right, loop_timesteps(KEY, offset, 300, 1000, bug))
        print(bug, offset, frac)
        assert frac >= 0.40


@pytest.mark.parametrize("bug", ["lanes", "stream", "no_x8", "trunc32", "unshift"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("Cm", [1, 3])
def test_twin_degrade_mask(bug, shape, Cm):
    N, C, H, W = shape
    for offset in _states_for(bug):
        right = R.degrade_keep(R.degrade_uniforms(KEY, offset, 1, N, Cm, H * W), [0.5] * N)
        twin = R.degrade_keep(loop_degrade_u(KEY, offset, 1, N, Cm, H * W, bug), [0.5] * N)
        frac = _differ(right, twin)
        print(bug, shape, Cm, offset, frac)
        assert frac >= 0.40


@pytest.mark.parametrize("bug", ["stream", "no_x8", "trunc32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_index_mask(bug, shape):
    N, C, H, W = shape
    HW = H * W
    for offset in _states_for(bug):
        right = R.index_keep(KEY, offset, 3, N, HW, [HW // 2] * N)
        frac = _differ(right, loop_index_keep(KEY, offset, 3, N, HW, [HW // 2] * N, bug))
        print(bug, shape, offset, frac)
        assert frac >= 0.40


@pytest.mark.parametrize("bug", ["lanes", "stream", "no_x8", "trunc32", "unshift"])
@pytest.mark.parametrize("kind", [1, 2])
def test_twin_uniform_shift(bug, kind):
    for offset in _states_for(bug):
        right = R.shift_uniform_z(KEY, offset, 2, kind, 100)
        frac = _differ(right, loop_uniform_z(KEY, offset, 2, kind, 100, bug))
        print(bug, kind, offset, frac)
        assert frac >= 0.95


@functools.lru_cache(maxsize=None)
def _normal_pair(offset, shape, kind):
    N, C, H, W = shape
    return tuple(R.shift_normal_z(KEY, offset, 2, kind, N, H * W, dt) for dt in (np.float32, np.float64))


def _e32():
    """The rounding floor as the GPU test defines it: the largest |float32 - float64| Box-Muller value over the draws in use."""
    return max(float(np.abs(z32.astype(np.float64) - z64).max())
               for z32, z64 in (_normal_pair(o, s, k) for o in STATES for s in SHAPES for k in (3, 4)))


def test_rounding_floor_is_fp32_sized():
    e = _e32()
    print("E32", e)
    assert 2.0 ** -24 < e < 64 * 2.0 ** -24        # a few ulp of values up to 5.8; 64 E32 stays far below any draw's size


@pytest.mark.parametrize("bug", ["stream", "no_x8", "trunc32", "cossin", "unshift"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", [3, 4])
def test_twin_normal_shift(bug, shape, kind):
    N, C, H, W = shape
    e32 = _e32()
    for offset in _states_for(bug):
        z64 = _normal_pair(offset, shape, kind)[1]
        twin = loop_normal_z(KEY, offset, 2, kind, N, H * W, np.float64, bug)
        bound = 64 * e32 + 2.0 ** -23 * np.abs(z64)                   # the GPU test's, at ratio 1
        frac = float(np.mean(np.abs(twin - z64) > 100 * bound))
        print(bug, shape, kind, offset, frac)
        assert frac >= 0.95


def test_swapped_pair_over_all_draws():
    """cos / sin swapped, over every draw of the shapes above at the three states: how visible the swap is in absolute terms."""
    d = []
    for offset in STATES:
        for shape in SHAPES:
            for kind in (3, 4):
                N, C, H, W = shape
                d.append(np.abs(loop_normal_z(KEY, offset, 2, kind, N, H * W, np.float64, "cossin") - _normal_pair(offset, shape, kind)[1]).ravel())
    d = np.concatenate(d)
    frac = float(np.mean(d > 1e-2))
    print(len(d), frac)
    assert frac >= 0.98
