"""mdm_loss_fwd_bwd, mdm_sampler_x0 and mdm_sampler_update through the C ABI against their own statements (tests/_bounds.py, the
section on the store, loss, sampler and evaluation kernels): the loss word inside its fp64 bound, dpred and every sampler output bit
for bit.  Rows: tests/_store_rows.py.

Every operand sits in a `Buf` (the loss words in an `IntBuf`) inside guard bands, destinations start as the NaN pattern, the pad
channels of `pred` hold NaN, inputs must come back bit for bit and a second launch must repeat the first."""
import pytest
import torch

import _store_rows as SR
from _bounds import Buf, sampler_update_want, sampler_x0_want
from _notes import note
from _store_rows import IntBuf, call, check_loss, refused, same_f32

pytestmark = pytest.mark.gpu
F32 = torch.float32
DT = {"f32": 0, "bf16": 1}


def _dev():
    return torch.device("cuda:0")


def _p(b):
    return None if b is None else b.t.data_ptr()


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _intact(bufs, inputs=()):
    for b in bufs:
        if b is not None:
            assert b.guards_intact(), b.first_bad_guard()
    for b, want in inputs:
        if b is not None:
            assert torch.equal(_bits(b.t).cpu(), _bits(want.to(b.dtype))), "an input was modified"


def _buf(t, dtype=F32):
    return None if t is None else Buf(t.shape, dtype, _dev(), t)


# ------------------------------------------------------------------ mdm_loss_fwd_bwd
def _run_loss(r, T):
    N, C, H, W, Cp, dt, ws, ww = r
    B = dict(pred=_buf(T["pred"], SR.TD[dt]), x_in=_buf(T["x_in"]), s=_buf(T["s"]), x0=_buf(T["x0"]), w=_buf(T["w"]))
    dpred, words = Buf((N, H, W, Cp), SR.TD[dt], _dev()), IntBuf(2, _dev(), fill=0)
    call("mdm_loss_fwd_bwd", DT[dt], _p(B["pred"]), _p(B["x_in"]), _p(B["s"]), _p(B["x0"]), _p(B["w"]), N, C, H, W, Cp, SR.LOSS_GSCALE,
         _p(dpred), _p(words))
    _intact(list(B.values()) + [dpred, words], [(B[k], T[k]) for k in B])
    w = words.t.cpu().tolist()
    return w[0], w[1], dpred.t.cpu()


@pytest.mark.parametrize("row", SR.LOSS_ROWS, ids=[SR.loss_id(r) for r in SR.LOSS_ROWS])
def test_loss_word_bound_and_dpred_bit_for_bit(row):
    T = SR.loss_problem(row)
    word, flag, dpred = _run_loss(row, T)
    ratio = check_loss(SR.loss_id(row), row, T, word, flag, dpred)
    note("store_eval_bounds", dict(row=f"loss-{SR.loss_id(row)}", out="loss", ratio=ratio))
    word2, flag2, dpred2 = _run_loss(row, T)
    assert (word, flag) == (word2, flag2) and torch.equal(_bits(dpred), _bits(dpred2)), "two identical launches differ"


def test_loss_without_dpred_gives_the_same_words():
    row = SR.LOSS_ROWS[0]
    N, C, H, W, Cp, dt, ws, ww = row
    T = SR.loss_problem(row)
    word, flag, _ = _run_loss(row, T)
    B = dict(pred=_buf(T["pred"], SR.TD[dt]), x_in=_buf(T["x_in"]), x0=_buf(T["x0"]))
    words = IntBuf(2, _dev(), fill=0)
    call("mdm_loss_fwd_bwd", DT[dt], _p(B["pred"]), _p(B["x_in"]), None, _p(B["x0"]), None, N, C, H, W, Cp, SR.LOSS_GSCALE, None, _p(words))
    _intact(list(B.values()) + [words])
    assert words.t.cpu().tolist() == [word, flag]


def test_loss_refusals():
    row = SR.LOSS_ROWS[0]
    N, C, H, W, Cp, dt, ws, ww = row
    T = SR.loss_problem(row)
    pred, x_in, x0 = _buf(T["pred"], SR.TD[dt]), _buf(T["x_in"]), _buf(T["x0"])
    dpred, words = Buf((N, H, W, Cp), SR.TD[dt], _dev()), IntBuf(2, _dev(), fill=0)
    ok = [DT[dt], _p(pred), _p(x_in), None, _p(x0), None, N, C, H, W, Cp, SR.LOSS_GSCALE, _p(dpred), _p(words)]
    for i, v in ((1, None), (2, None), (4, None), (13, None), (10, 12), (10, 0)):      # pred, x_in, x0, loss words; Cp % 8, Cp < C
        bad = list(ok)
        bad[i] = v
        assert refused("mdm_loss_fwd_bwd", *bad), (i, v)
    torch.cuda.synchronize()
    _intact((pred, x_in, x0, dpred, words))
    assert words.t.cpu().tolist() == [0, 0] and bool((_bits(dpred.t) == dpred.pat).all()), "a refused call wrote"


# ------------------------------------------------------------------ mdm_sampler_x0
@pytest.mark.parametrize("form", SR.SAMPLER_FORMS, ids=lambda f: f"{f[0]}-s{f[1]}-p{f[2]}-h{f[3]}")
@pytest.mark.parametrize("shape", SR.SAMPLER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sampler_x0_bit_for_bit(shape, form):
    N, C, H, W, Cp = shape
    dt, ws, wp, wh = form
    T = SR.sampler_problem(shape, dt)
    want = sampler_x0_want(T["pred"], T["x_in"], T["s"] if ws else None, C)
    outs = []
    for _ in range(2):
        pred, x_in, s = _buf(T["pred"], SR.TD[dt]), _buf(T["x_in"]), _buf(T["s"]) if ws else None
        o = [Buf((N, C, H, W), F32, _dev()) if give else None for give in (wp, wh, 1)]
        call("mdm_sampler_x0", DT[dt], _p(pred), Cp, _p(x_in), _p(s), N, C, H, W, _p(o[0]), _p(o[1]), _p(o[2]))
        _intact([pred, x_in, s] + o, [(pred, T["pred"]), (x_in, T["x_in"]), (s, T["s"])])
        outs.append([None if b is None else b.t.cpu() for b in o])
    for name, got, again, w in zip(("pred_nchw", "shifted0", "x0_hat"), outs[0], outs[1], want):
        if got is not None:
            assert not bool(torch.isnan(got).any()), f"{name}: a NaN (a pad channel of pred, or an element never written)"
            assert same_f32(got, w), f"{name} differs from the fp32 expression"
            assert same_f32(got, again)


def test_sampler_x0_refusals():
    shape = SR.SAMPLER_SHAPES[1]
    N, C, H, W, Cp = shape
    T = SR.sampler_problem(shape, "f32")
    pred, x_in, out = _buf(T["pred"]), _buf(T["x_in"]), Buf((N, C, H, W), F32, _dev())
    ok = [0, _p(pred), Cp, _p(x_in), None, N, C, H, W, None, None, _p(out)]
    for i, v in ((0, 2), (0, -1), (1, None), (3, None), (11, None), (5, 0), (6, 0), (7, 0), (8, -1), (2, C - 1)):
        bad = list(ok)
        bad[i] = v
        assert refused("mdm_sampler_x0", *bad), (i, v)
    torch.cuda.synchronize()
    _intact((pred, x_in, out))
    assert bool((_bits(out.t) == out.pat).all()), "a refused call wrote"


# ------------------------------------------------------------------ mdm_sampler_update
@pytest.mark.parametrize("form", SR.UPDATE_FORMS, ids=lambda f: f"momentum{f[0]}-diff{f[1]}")
@pytest.mark.parametrize("shape", SR.SAMPLER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sampler_update_bit_for_bit(shape, form):
    N, C, H, W, _ = shape
    mom, wd = form
    n = N * C * H * W
    T = SR.sampler_problem(shape, "f32")
    wdiff, wx = sampler_update_want(T["d_t"], T["d_next"], T["x_t"], mom)
    outs = []
    for _ in range(2):
        d_t, d_next, x_t = _buf(T["d_t"]), _buf(T["d_next"]), _buf(T["x_t"])
        diff = Buf((N, C, H, W), F32, _dev()) if wd else None
        call("mdm_sampler_update", _p(d_t), _p(d_next), _p(x_t), _p(diff), mom, n)
        _intact((d_t, d_next, x_t, diff), [(d_t, T["d_t"]), (d_next, T["d_next"])])
        outs.append((x_t.t.cpu(), None if diff is None else diff.t.cpu()))
    assert same_f32(outs[0][0], wx), "x_t differs from x_t + (d_next - d_t)" if mom else "x_t does not hold the bits of d_next"
    assert same_f32(outs[0][0], outs[1][0])
    if wd:
        assert same_f32(outs[0][1], wdiff) and same_f32(outs[0][1], outs[1][1])


def test_sampler_update_refusals():
    T = SR.sampler_problem(SR.SAMPLER_SHAPES[1], "f32")
    d_t, d_next, x_t = _buf(T["d_t"]), _buf(T["d_next"]), _buf(T["x_t"])
    ok = [_p(d_t), _p(d_next), _p(x_t), None, 1, T["x_t"].numel()]
    for i, v in ((0, None), (1, None), (2, None), (5, 0), (5, -3)):
        bad = list(ok)
        bad[i] = v
        assert refused("mdm_sampler_update", *bad), (i, v)
    torch.cuda.synchronize()
    _intact((d_t, d_next, x_t), [(x_t, T["x_t"])])
