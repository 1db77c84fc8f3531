"""fp64 bounds for every compiled kernel of the time-embedding path (csrc/temb.hip) and every operand form its C ABI takes.

temb.hip compiles eight skinny kernels: skinny_nt_kernel<MB, NB, TEMB> for (2 | 8, 1 | 2, false) and (2 | 8, 1, true), and
skinny_nn_kernel<2 | 8, 1>.  FWD_ROWS / BWD_ROWS of tests/_temb_rows.py reach each of them (asserted by route name:
mdm_skinny_route_of before the launch, mdm_skinny_last_route after it) at every M edge of its row blocks, in every state of its
look-ahead loop, with bias / act_out / emb_out NULL and given and with dense and padded pitches -- the calls go through _lib.call,
because ops.skinny_linear_* always passes dense pitches.

Every output is held per element against the bounds derived in tests/_bounds.py.  Every operand and output sits in a `Buf` inside
NaN guard bands; the pad columns of a pitched operand hold the NaN pattern too, so a read past a row's end that reaches a result
turns it into NaN and a write there changes the pattern.  Outputs start as the pattern (an unwritten element fails), inputs must
come back bit for bit, and a second launch must repeat the first bit for bit."""
import pytest
import torch

from _bounds import Buf, check_bound, silu_bwd_sum_ref
from _notes import note
from _temb_rows import (BWD_ROWS, FWD_ROWS, REFUSALS, SUM_ROWS, bwd_id, bwd_problem, check_bwd, check_fwd, fwd_id, fwd_problem)

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _dev():
    return torch.device("cuda:0")


def _pitched(data, ld):
    """data [R][C] -> a Buf [R][ld] whose pad columns C .. ld - 1 hold the NaN pattern"""
    R, C = data.shape
    b = Buf((R, ld), F32, _dev())
    b.t[:, :C].copy_(data)
    return b


def _out(R, C, ld):
    return Buf((R, ld), F32, _dev())


def _raw_bits(B, names):
    return {k: B[k].raw.view(B[k].ity).clone() for k in names if k in B}


def _assert_intact(B, before, what):
    for name, b in B.items():
        assert b.guards_intact(), f"{what}: guard band of {name} touched at (below, above) = {b.first_bad_guard()}"
    for name, bits in before.items():
        assert torch.equal(B[name].raw.view(B[name].ity), bits), f"{what}: input {name} was modified"


def _pads_hold_the_pattern(b, C):
    return bool((b.t.view(b.ity)[:, C:] == b.pat).all())


def _run_fwd(r, T, emb=None):
    from mdm import _lib
    emb = r.emb if emb is None else emb
    ldx, ldw, ldy = r.K + r.pad, r.K + r.pad, r.N + r.pad
    B = dict(W=_pitched(T["W"], ldw), y=_out(r.M, r.N, ldy))
    if r.temb:
        B["t"] = Buf((r.M,), F32, _dev(), T["t"])
    else:
        B["x"] = _pitched(T["x"], ldx)
    if r.bias:
        B["bias"] = Buf((r.N,), F32, _dev(), T["bias"])
    if r.act:
        B["act"] = _out(r.M, r.N, ldy)
    if r.temb and emb:
        B["emb"] = Buf((r.M, r.K), F32, _dev())
    before = _raw_bits(B, ("W", "x", "t", "bias"))
    p = lambda k: B[k].t.data_ptr() if k in B else None
    flip, shift = r.variant if r.temb else (0, 1.0)
    assert _lib.skinny_route_of(0, r.M, r.N, r.K, r.temb) == r.route
    _lib.call("mdm_skinny_linear_fwd", x=p("x"), ldx=ldx, t=p("t"), flip_sin_to_cos=flip, freq_shift=shift, emb_out=p("emb"), W=p("W"),
              ldw=ldw, bias=p("bias"), M=r.M, N=r.N, K=r.K, y=p("y"), ldy=ldy, act_out=p("act"), stream=_lib.stream())
    assert _lib.skinny_last_route() == r.route
    torch.cuda.synchronize()
    _assert_intact(B, before, fwd_id(r))
    for k in ("y", "act"):
        assert k not in B or _pads_hold_the_pattern(B[k], r.N), f"{fwd_id(r)}: pad columns of {k} written"
    return B


def _fwd_got(B, r):
    return dict(y=B["y"].t[:, :r.N], act=B["act"].t[:, :r.N] if "act" in B else None, emb=B["emb"].t if "emb" in B else None)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("row", FWD_ROWS, ids=[fwd_id(r) for r in FWD_ROWS])
def test_skinny_forward_bounds(row):
    T = fwd_problem(row)
    got = _fwd_got(_run_fwd(row, T), row)
    for name, ratio in check_fwd(row, T, {k: (v.cpu() if v is not None else None) for k, v in got.items()}).items():
        note("temb_bounds", dict(row=fwd_id(row), out=name, ratio=ratio))
    again = _fwd_got(_run_fwd(row, T), row)
    for k, v in got.items():
        assert v is None or _same_bits(v, again[k]), f"{k} differs between two identical launches"
    if row.temb and not row.emb:          # storing the embedding does not change what is multiplied
        assert _same_bits(got["y"], _fwd_got(_run_fwd(row, T, emb=1), row)["y"]), "y depends on emb_out"


def _run_bwd(r, T):
    from mdm import _lib
    lddy, ldw = r.K + r.pad, r.N + r.pad
    B = dict(dy=_pitched(T["dy"], lddy), W=_pitched(T["W"], ldw))
    if r.splits == 1:
        B["dx"] = Buf((r.M, r.N), F32, _dev())
        if r.pre:
            B["pre"] = Buf((r.M, r.N), F32, _dev(), T["pre"])
    else:
        B["slabs"] = Buf((r.splits, r.M, r.N), F32, _dev())
    before = _raw_bits(B, ("dy", "W", "pre"))
    p = lambda k: B[k].t.data_ptr() if k in B else None
    assert _lib.skinny_route_of(1, r.M, r.N, r.K) == r.route
    _lib.call("mdm_skinny_linear_bwd", dy=p("dy"), lddy=lddy, W=p("W"), ldw=ldw, M=r.M, N=r.N, K=r.K, splits=r.splits, pre=p("pre"),
              dx=p("dx"), slabs=p("slabs"), stream=_lib.stream())
    assert _lib.skinny_last_route() == r.route
    if r.splits > 1:                      # silu_bwd_sum on the slabs the launch stored
        B["dx"] = Buf((r.M, r.N), F32, _dev())
        if r.pre:
            B["pre"] = Buf((r.M, r.N), F32, _dev(), T["pre"])
            before.update(_raw_bits(B, ("pre",)))
        _lib.call("mdm_silu_bwd_sum", pre=p("pre"), slabs=p("slabs"), nslab=r.splits, n=r.M * r.N, dx=p("dx"), stream=_lib.stream())
    torch.cuda.synchronize()
    _assert_intact(B, before, bwd_id(r))
    return B


@pytest.mark.parametrize("row", BWD_ROWS, ids=[bwd_id(r) for r in BWD_ROWS])
def test_skinny_backward_bounds(row):
    T = bwd_problem(row)
    B = _run_bwd(row, T)
    got = dict(dx=B["dx"].t.cpu(), slabs=B["slabs"].t.cpu() if "slabs" in B else None)
    for name, ratio in check_bwd(row, T, got).items():
        note("temb_bounds", dict(row=bwd_id(row), out=name, ratio=ratio))
    B2 = _run_bwd(row, T)
    for k in ("dx", "slabs"):
        assert k not in B or _same_bits(B[k].t, B2[k].t), f"{k} differs between two identical launches"


@pytest.mark.parametrize("nslab,pre,n", SUM_ROWS)
def test_silu_bwd_sum_bounds(nslab, pre, n):
    """n = 4: one float4, one live lane; n = 4 x 257: the second workgroup has one"""
    from mdm import _lib
    g = torch.Generator().manual_seed(nslab + n)
    slabs, p = torch.randn(nslab, n, generator=g), (torch.randn(n, generator=g) * 2.5 if pre else None)
    outs = []
    for _ in range(2):
        B = dict(slabs=Buf((nslab, n), F32, _dev(), slabs), dx=Buf((n,), F32, _dev()))
        if pre:
            B["pre"] = Buf((n,), F32, _dev(), p)
        before = _raw_bits(B, ("slabs", "pre"))
        _lib.call("mdm_silu_bwd_sum", pre=B["pre"].t.data_ptr() if pre else None, slabs=B["slabs"].t.data_ptr(), nslab=nslab, n=n,
                  dx=B["dx"].t.data_ptr(), stream=_lib.stream())
        torch.cuda.synchronize()
        _assert_intact(B, before, "silu_bwd_sum")
        outs.append(B["dx"].t)
    ratio, _ = check_bound("silu_bwd_sum", outs[0], *silu_bwd_sum_ref(slabs, p))
    note("temb_bounds", dict(row=f"silu_bwd_sum-{nslab}x{n}-{'pre' if pre else 'lin'}", out="dx", ratio=ratio))
    assert _same_bits(outs[0], outs[1])


# ------------------------------------------------------------------ refusals: nothing is written, no route is left
def _refusal_bufs():
    dev = _dev()
    z = lambda *s: Buf(s, F32, dev, torch.zeros(*s))
    return dict(x=z(129, 132), t=z(129), W=z(132, 132), bias=z(132), pre=z(129, 132),
                y=Buf((129, 132), F32, dev), act=Buf((129, 132), F32, dev), emb=Buf((129, 132), F32, dev), slabs=Buf((16, 129, 132), F32, dev))


def _untouched(b):
    return bool((b.raw.view(b.ity) == b.pat).all())


def _fwd_args(B, **kw):
    from mdm import _lib
    a = dict(x=B["x"].t.data_ptr(), ldx=132, t=None, flip_sin_to_cos=0, freq_shift=1.0, emb_out=B["emb"].t.data_ptr(), W=B["W"].t.data_ptr(),
             ldw=132, bias=B["bias"].t.data_ptr(), M=4, N=16, K=64, y=B["y"].t.data_ptr(), ldy=132, act_out=B["act"].t.data_ptr(),
             stream=_lib.stream())
    a.update(kw)
    return a


def _bwd_args(B, **kw):
    from mdm import _lib
    a = dict(dy=B["x"].t.data_ptr(), lddy=132, W=B["W"].t.data_ptr(), ldw=132, M=4, N=16, K=64, splits=1, pre=B["pre"].t.data_ptr(),
             dx=B["y"].t.data_ptr(), slabs=B["slabs"].t.data_ptr(), stream=_lib.stream())
    a.update(kw)
    return a


def _refused(B, name, args):
    from mdm import _lib
    with pytest.raises(RuntimeError, match="skinny_linear"):
        _lib.call(name, **args)
    assert _lib.skinny_last_route() == "none"
    torch.cuda.synchronize()
    for k in ("y", "act", "emb", "slabs"):
        assert _untouched(B[k]), f"a refused call wrote {k}"


def test_refusals_write_nothing_and_leave_no_route():
    from mdm import _lib
    B = _refusal_bufs()
    tp = B["t"].t.data_ptr()
    _lib.call("mdm_skinny_linear_fwd", **_fwd_args(B, emb_out=None, y=B["pre"].t.data_ptr(), act_out=None))      # a route to lose
    assert _lib.skinny_last_route() == "nt<2,1>"
    for which, M, N, K, splits in REFUSALS:
        if which == 0:
            _refused(B, "mdm_skinny_linear_fwd", _fwd_args(B, M=M, N=N, K=K))
            _refused(B, "mdm_skinny_linear_fwd", _fwd_args(B, M=M, N=N, K=K, x=None, t=tp))
        else:
            _refused(B, "mdm_skinny_linear_bwd", _bwd_args(B, M=M, N=N, K=K, splits=splits))
    _refused(B, "mdm_skinny_linear_fwd", _fwd_args(B, t=tp))                      # both x and t
    _refused(B, "mdm_skinny_linear_fwd", _fwd_args(B, x=None))                    # neither
    for pitch in ("ldx", "ldw", "ldy"):
        _refused(B, "mdm_skinny_linear_fwd", _fwd_args(B, **{pitch: 130}))
    _refused(B, "mdm_skinny_linear_fwd", _fwd_args(B, x=None, t=tp, ldw=130))
    _refused(B, "mdm_skinny_linear_bwd", _bwd_args(B, lddy=130))
    _refused(B, "mdm_skinny_linear_bwd", _bwd_args(B, dx=None))
    _refused(B, "mdm_skinny_linear_bwd", _bwd_args(B, K=128, splits=2, slabs=None))
    for b in B.values():
        assert b.guards_intact()
