"""The evaluation kernels of csrc/eval.hip through the C ABI against their own statements (tests/_bounds.py, the section on the store,
loss, sampler and evaluation kernels): mdm_normalize01 and mdm_col_argmax bit for bit against torch on the CPU -- NaN pixels, NaN
and -inf columns and equal maxima included --, mdm_unit_rows inside its fp64 bound.  Rows: tests/_store_rows.py.

Every operand sits in a `Buf` (the indices in an `IntBuf`) inside guard bands, destinations start as the NaN pattern or a sentinel,
inputs must come back bit for bit and a second launch must repeat the first.  No index a kernel returned is used to address memory."""
import pytest
import torch

import _store_rows as SR
from _bounds import Buf
from _notes import note
from _store_rows import IntBuf, call, check_col_argmax, check_normalize01, check_unit_rows, refused, same_f32

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _dev():
    return torch.device("cuda:0")


def _intact(bufs, inputs=()):
    for b in bufs:
        assert b.guards_intact(), b.first_bad_guard()
    for b, want in inputs:
        assert torch.equal(b.t.cpu().view(torch.int32), want.contiguous().view(torch.int32)), "an input was modified"


# ------------------------------------------------------------------ mdm_normalize01
@pytest.mark.parametrize("E", SR.NORM_ES)
def test_normalize01_bit_for_bit(E):
    """one image per kind: plain, the extremum in the last element, all negative, constant (zeros), one +inf, one NaN (all zeros)"""
    x = SR.normalize_problem(E)
    N = x.shape[0]
    outs = []
    for _ in range(2):
        xb, yb = Buf((N, E), F32, _dev(), x), Buf((N, E), F32, _dev())
        call("mdm_normalize01", xb.t.data_ptr(), yb.t.data_ptr(), N, E)
        _intact((xb, yb), [(xb, x)])
        outs.append(yb.t.cpu())
    y = outs[0]
    k = SR.NORM_KINDS.index
    assert not bool(y[k("nan")].any()), f"an image with one NaN pixel must come out all zero: {int((y[k('nan')] != 0).sum())} of {E} are not"
    assert not bool(y[k("constant")].any())
    check_normalize01(f"normalize01 {E}", y, x)
    assert same_f32(outs[0], outs[1])


# ------------------------------------------------------------------ mdm_unit_rows
@pytest.mark.parametrize("R", SR.UNIT_RS)
@pytest.mark.parametrize("D", SR.UNIT_DS)
def test_unit_rows_bound(D, R):
    x = SR.unit_problem(R, D)
    outs = []
    for _ in range(2):
        xb, yb = Buf((R, D), F32, _dev(), x), Buf((R, D), F32, _dev())
        call("mdm_unit_rows", xb.t.data_ptr(), yb.t.data_ptr(), R, D, SR.UNIT_EPS)
        _intact((xb, yb), [(xb, x)])
        outs.append(yb.t.cpu())
    ratio = check_unit_rows(f"unit_rows {R}x{D}", outs[0], x, SR.UNIT_EPS)
    note("store_eval_bounds", dict(row=f"unit_rows-{R}x{D}", out="y", ratio=ratio))
    assert same_f32(outs[0], outs[1])
    if R >= 5 and D <= 3072:                                     # ||x|| = 1e-10 sqrt(D) < eps: x / eps
        want = (x[2].double() / float(torch.tensor(SR.UNIT_EPS, dtype=F32))).float()
        assert float((outs[0][2] - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())


# ------------------------------------------------------------------ mdm_col_argmax
def _col_argmax(S, with_val=True):
    M, B = S.shape
    sb, vb, ib = Buf((M, B), F32, _dev(), S), (Buf((B,), F32, _dev()) if with_val else None), IntBuf(B, _dev())
    call("mdm_col_argmax", sb.t.data_ptr(), M, B, None if vb is None else vb.t.data_ptr(), ib.t.data_ptr())
    _intact([b for b in (sb, vb, ib) if b is not None], [(sb, S)])
    return (None if vb is None else vb.t.cpu()), ib.t.cpu()


@pytest.mark.parametrize("B", SR.ARGMAX_BS)
@pytest.mark.parametrize("M", SR.ARGMAX_MS)
def test_col_argmax_is_torch_max_dim0(M, B):
    """planted equal maxima (the same lane's serial loop, neighbouring rows, rows 5 and 700, two waves), an all-equal, an all-negative, an
    all -inf column, columns with one, two and only NaNs: values and indices of torch.max(dim=0), every index below M"""
    S, plan = SR.argmax_problem(M, B)
    val, idx = _col_argmax(S)
    check_col_argmax(f"col_argmax {M}x{B} {sorted(plan)}", val, idx, S)
    val2, idx2 = _col_argmax(S)
    assert torch.equal(idx, idx2) and torch.equal(val.view(torch.int32), val2.view(torch.int32))
    _, idx3 = _col_argmax(S, with_val=False)
    assert torch.equal(idx, idx3), "val = NULL changes the indices"


def test_eval_kernel_refusals():
    xb, yb, ib = Buf((4, 8), F32, _dev(), torch.ones(4, 8)), Buf((4, 8), F32, _dev()), IntBuf(8, _dev())
    x, y, i = xb.t.data_ptr(), yb.t.data_ptr(), ib.t.data_ptr()
    for args in ((None, y, 4, 8), (x, None, 4, 8), (x, y, 0, 8), (x, y, 4, 0)):
        assert refused("mdm_normalize01", *args), args
        assert refused("mdm_unit_rows", *args, 1e-8), args
    for args in ((None, 4, 8, y, i), (x, 4, 8, y, None), (x, 0, 8, y, i), (x, 4, 0, y, i)):
        assert refused("mdm_col_argmax", *args), args
    torch.cuda.synchronize()
    _intact((xb, yb, ib), [(xb, torch.ones(4, 8))])
    assert bool((yb.t.view(torch.int32) == yb.pat).all()) and bool((ib.t == 0x7A7A7A7A7A7A7A7A).all()), "a refused call wrote"
