"""The three kernels of csrc/interp.hip through the C ABI (include/mdm_interp.h), bit for bit against numpy.

mdm_interp_shift against the formula of the header (tests/_interp_ref.shift_np: fp32 shift times fp64 ratio rounded once, clamped in
fp64 with torch.clamp's NaN rule, rounded once; x_in one fp32 addition), on the 16-byte path (H W = 16) and the scalar one
(H W = 15), with every combination of absent outputs.  mdm_interp_row_mask against the thresholded replay row and against the host
predictor of its Philox row (tests/_interp_ref.row_uniforms) at the three generator states of test_device_draws_gpu.py.
mdm_interp_update against two fp32 numpy operations.  Every output buffer is pre-filled with a sentinel and compared whole, with a
guard band behind it; a refused call writes nothing.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _interp_ref as IR  # noqa: E402
from mdm import _lib  # noqa: E402

KEY = (0x9E3779B9 << 32) | 12345
STATES = [1, 2 ** 29 + 3, 2 ** 61 + 5]
SENT, GUARD = -512.0, 8                          # (exact in bf16 too)


def _rng(key, offset):
    return torch.from_numpy(np.array([key, offset], dtype=np.uint64).view(np.int64)).cuda()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _out(numel, dtype=torch.float32, skew=0):
    """(view of `numel` sentinels, the whole buffer): GUARD sentinels behind the view, and `skew` elements in front of it -- a view
    that starts `skew` elements into the allocation is not 16-byte aligned."""
    buf = torch.full((skew + numel + GUARD,), SENT, device="cuda", dtype=dtype)
    return buf[skew:skew + numel], buf


def _untouched(buf, numel, skew=0):
    h = buf.float().cpu().numpy()
    return (h[:skew] == SENT).all() and (h[skew + numel:] == SENT).all()


def _call(name, **kw):
    _lib.call(name, stream=_lib.stream(), **kw)
    torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """bit for bit, a NaN matching any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ------------------------------------------------------------------------------------------ shift
def _shift_case(case, N, C, H, W):
    g = np.random.default_rng(31 * N + H * W)
    ratio = g.random(N) * 0.9 + 0.1                                     # fp64, not fp32 numbers
    assert not np.any(ratio == ratio.astype(np.float32))
    shift = np.float32(-0.4)
    sv = (np.float64(shift) * ratio).astype(np.float32).astype(np.float64)
    if case == "below":                                                 # lo = sv + 0.3 > sv
        mu = -(sv + ratio) - 0.3
    elif case == "above":                                               # hi = sv - 0.3 < sv
        mu = ratio - sv + 0.3
    else:                                                               # lo = sv - 1.25 ratio < sv < sv + 0.75 ratio = hi
        mu = -sv + 0.25 * ratio
    mu = mu.astype(np.float32)
    if case == "nan":
        mu[0] = np.nan
    x_t = (g.random((N, C, H, W)) * 2 - 1).astype(np.float32)
    s, x_in = IR.shift_np(x_t, mu, ratio, shift)
    m = -mu.astype(np.float64)
    want = {"below": (m - ratio).astype(np.float32), "above": (m + ratio).astype(np.float32)}.get(case, sv.astype(np.float32))
    ok = ~np.isnan(mu)
    assert np.array_equal(s[ok, 0, 0, 0], want[ok]) and np.isnan(s[~ok]).all(), "the case is not in the regime it names"
    if case in ("below", "above"):
        assert np.all(s[:, 0, 0, 0] != sv.astype(np.float32))
    return x_t, mu, ratio, float(shift), s, x_in


@pytest.mark.parametrize("shape", [(3, 3, 4, 4), (2, 4, 5, 3)])
@pytest.mark.parametrize("case", ["below", "above", "inactive", "nan"])
@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
def test_shift(shape, case, dtype):
    N, C, H, W = shape
    Cp, numel = 8, N * C * H * W
    x_t, mu, ratio, shift, s_want, x_want = _shift_case(case, N, C, H, W)
    d_x, d_mu, d_ratio = dev(x_t), dev(mu), dev(ratio)
    tdt = _lib.torch_dtype(dtype)
    nh_want = torch.full((N, H, W, Cp), SENT, dtype=tdt)
    nh_want[..., :C] = torch.from_numpy(x_want).permute(0, 2, 3, 1).to(tdt)       # round to nearest even; the pad channels stay
    for has_s, has_x, has_nh in itertools.product((True, False), repeat=3):       # every combination of absent outputs
        (s, s_buf), (x_in, x_buf), (nh, nh_buf) = _out(numel), _out(numel), _out(N * H * W * Cp, tdt)
        _call("mdm_interp_shift", x_t=d_x.data_ptr(), mu=d_mu.data_ptr(), ratio=d_ratio.data_ptr(), shift=shift, N=N, C=C, H=H, W=W,
              s=s.data_ptr() if has_s else None, x_in=x_in.data_ptr() if has_x else None, dtype=dtype,
              x_in_nhwc=nh.data_ptr() if has_nh else None, Cp=Cp)
        which = (has_s, has_x, has_nh)
        if has_s:
            assert _same(s.cpu().numpy().reshape(shape), s_want), which
        if has_x:
            assert _same(x_in.cpu().numpy().reshape(shape), x_want), which
        if has_nh:
            assert _same(nh.float().cpu().numpy().reshape(N, H, W, Cp), nh_want.float().numpy()), which
        for buf, n, has in ((s_buf, numel, has_s), (x_buf, numel, has_x), (nh_buf, N * H * W * Cp, has_nh)):
            assert _untouched(buf, n if has else 0), which
    assert torch.equal(d_x.cpu(), torch.from_numpy(x_t))                           # the input is read only


def test_shift_on_the_scalar_path_of_unaligned_buffers():
    """H W = 16 with x_t, s and x_in each one element off a 16-byte boundary: the 16-byte path must not be taken"""
    N, C, H, W = 3, 3, 4, 4
    numel = N * C * H * W
    x_t, mu, ratio, shift, s_want, x_want = _shift_case("inactive", N, C, H, W)
    d_mu, d_ratio = dev(mu), dev(ratio)
    for skews in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        xb = torch.zeros(numel + 1, device="cuda")
        d_x = xb[skews[0]:skews[0] + numel].copy_(torch.from_numpy(x_t).reshape(-1))
        (s, s_buf), (x_in, x_buf) = _out(numel, skew=skews[1]), _out(numel, skew=skews[2])
        _call("mdm_interp_shift", x_t=d_x.data_ptr(), mu=d_mu.data_ptr(), ratio=d_ratio.data_ptr(), shift=shift, N=N, C=C, H=H,
              W=W, s=s.data_ptr(), x_in=x_in.data_ptr(), dtype=0, x_in_nhwc=None, Cp=0)
        assert _same(s.cpu().numpy().reshape(s_want.shape), s_want) and _same(x_in.cpu().numpy().reshape(x_want.shape), x_want), skews
        assert _untouched(s_buf, numel, skews[1]) and _untouched(x_buf, numel, skews[2]), skews


# ------------------------------------------------------------------------------------------ row mask
AMOUNTS = np.array([0.0, 0.5, 3.0])


def _row(HW):
    u = np.random.default_rng(HW).random(HW).astype(np.float32)
    u[0], u[1], u[HW - 1] = 0.0, 0.5, 0.5                                 # u == amount is NOT kept
    return u


@pytest.mark.parametrize("HW", [15, 16, 1028])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("skew", [0, 1])
def test_row_mask_of_a_replayed_row(HW, C, skew):
    N, u = 3, _row(HW)
    ub = torch.zeros(HW + 1, device="cuda")
    d_u = ub[skew:skew + HW].copy_(torch.from_numpy(u))
    mask, buf = _out(N * C * HW, skew=skew)
    d_amt = dev(AMOUNTS)
    _call("mdm_interp_row_mask", amount=d_amt.data_ptr(), u_row=d_u.data_ptr(), rng=None, N=N, C=C, HW=HW, mask=mask.data_ptr())
    got = mask.cpu().numpy().reshape(N, C, HW)
    assert np.array_equal(_bits(got), _bits(IR.row_keep(u, AMOUNTS, C)))
    assert (got == got[:, :1]).all() and got[0, 0, 0] == 0 and got[1, 0, 1] == 0 and not got[2].any()
    assert _untouched(buf, N * C * HW, skew)


@pytest.mark.parametrize("offset", STATES)
@pytest.mark.parametrize("HW", [15, 16, 1028])
@pytest.mark.parametrize("C", [1, 3])
def test_row_mask_of_the_philox_row(offset, HW, C):
    N = 3
    want = IR.row_keep(IR.row_uniforms(KEY, offset, HW), AMOUNTS, C)
    got = {}
    for key in (KEY, KEY & 0xFFFFFFFF, (0x12345 << 32) | (KEY & 0xFFFFFFFF)):      # keys that differ in the high word only
        mask, buf = _out(N * C * HW)
        rng, d_amt = _rng(key, offset), dev(AMOUNTS)
        _call("mdm_interp_row_mask", amount=d_amt.data_ptr(), u_row=None, rng=rng.data_ptr(), N=N, C=C, HW=HW, mask=mask.data_ptr())
        got[key] = mask.cpu().numpy().reshape(N, C, HW)
        assert np.array_equal(_bits(got[key]), _bits(want)), hex(key)
        assert _untouched(buf, N * C * HW) and torch.equal(rng.cpu(), _rng(key, offset).cpu())     # the state is read only
    g = got[KEY]
    assert (g == g[:, :1]).all() and not g[2].any()
    if HW == 1028:
        assert 0.4 < g[1].mean() < 0.6 and g[0].mean() > 0.99
        other = IR.row_keep(IR.row_uniforms(KEY, offset, HW, stream=4), AMOUNTS, C)
        assert not np.array_equal(g[1], other[1])                                # stream 6 is not the sampler's stream 4


# ------------------------------------------------------------------------------------------ update
@pytest.mark.parametrize("n", [1, 255, 1027])
@pytest.mark.parametrize("update", [0, 1, 5])
@pytest.mark.parametrize("skew", [0, 1])
def test_update(n, update, skew):
    g = np.random.default_rng(n)
    d_t, d_next, x_t = ((g.random(n) * 4 - 2).astype(np.float32) for _ in range(3))
    diff_want = (x_t - d_t).astype(np.float32)                            # two steps, each one fp32 rounding
    x_want = (d_next + diff_want).astype(np.float32) if update else x_t
    (x, x_buf), (diff, diff_buf) = _out(n, skew=skew), _out(n, skew=skew)
    x.copy_(torch.from_numpy(x_t))
    dt, dn = dev(d_t), dev(d_next)
    _call("mdm_interp_update", d_t=dt.data_ptr(), d_next=dn.data_ptr() if update != 0 or skew else None, x_t=x.data_ptr(),
          diff=diff.data_ptr(), update=update, n=n)
    assert np.array_equal(_bits(diff.cpu().numpy()), _bits(diff_want)) and np.array_equal(_bits(x.cpu().numpy()), _bits(x_want))
    assert _untouched(x_buf, n, skew) and _untouched(diff_buf, n, skew)
    assert np.array_equal(dt.cpu().numpy(), d_t) and np.array_equal(dn.cpu().numpy(), d_next)


# ------------------------------------------------------------------------------------------ refusals
def _refusal_rows():
    shift = dict(x_t="in", mu="in", ratio="in", shift=0.5, N=2, C=3, H=4, W=4, s="out", x_in="out", dtype=0, x_in_nhwc="nhwc", Cp=8)
    row = dict(amount="in", u_row="in", rng="in", N=2, C=3, HW=16, mask="out")
    upd = dict(d_t="in", d_next="in", x_t="out", diff="out", update=1, n=96)
    return [("mdm_interp_shift", shift, [dict(x_t=None), dict(mu=None), dict(ratio=None), dict(N=0), dict(C=-1), dict(H=0), dict(W=-3),
                                         dict(C=9), dict(dtype=2), dict(dtype=-1), dict(Cp=4), dict(Cp=12), dict(Cp=0)]),
            ("mdm_interp_row_mask", row, [dict(amount=None), dict(mask=None), dict(u_row=None, rng=None), dict(N=0), dict(C=0),
                                          dict(HW=-16), dict(C=9)]),
            ("mdm_interp_update", upd, [dict(d_t=None), dict(x_t=None), dict(diff=None), dict(d_next=None), dict(n=0), dict(n=-4)])]


@pytest.mark.parametrize("name,ok,rows", _refusal_rows(), ids=[r[0] for r in _refusal_rows()])
def test_refusals_write_nothing(name, ok, rows):
    """every pointer is a real buffer, far larger than any row's extents ask for"""
    lib = _lib.load()
    assert list(ok) + ["stream"] == _lib.INTERP_PARAMS[name]
    for change in rows:
        bufs = {"in": torch.zeros(4096, device="cuda", dtype=torch.float64), "out": _out(4096)[1], "nhwc": _out(4096)[1]}
        args = [bufs[v].data_ptr() if isinstance(v, str) else v for v in dict(ok, **change).values()]
        rc = getattr(lib, name)(*args, _lib.stream())
        text = lib.mdm_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and text.startswith(name[4:] + ":"), (change, rc, text)
        assert _untouched(bufs["out"], 0) and _untouched(bufs["nhwc"], 0) and not bufs["in"].any(), change


def test_a_shift_without_outputs_launches_nothing():
    P = torch.zeros(64, device="cuda", dtype=torch.float64).data_ptr()
    assert _lib.load().mdm_interp_shift(P, P, P, 0.5, 2, 3, 4, 4, None, None, 0, None, 0, _lib.stream()) == 0
    torch.cuda.synchronize()
