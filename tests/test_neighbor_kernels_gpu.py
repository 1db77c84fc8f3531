"""The kernels of csrc/neighbor.hip through the C ABI (include/mdm_neighbor.h) against their own statements: mdm_nn_rows inside the
fp64 bound of tests/_neighbor_ref.py (its docstring derives it) at every shape, storage kind, table and switch, mdm_nn_col_argmax bit
for bit `torch.max(dim=0)` of the stated score -- the tie / NaN / -inf problems of tests/_store_rows.py, with and without the mirrored
matrix, and carried across two chunks.

Every operand sits inside guard bands (`Buf`, `IntBuf`, `ByteBuf`), destinations start as the NaN pattern or a sentinel, inputs must
come back bit for bit and a second launch must repeat the first.  No index a kernel returned is used to address memory."""
import numpy as np
import pytest
import torch

import _neighbor_ref as NR
import _store_rows as SR
from _bounds import Buf
from _guard_bufs import ByteBuf
from _store_rows import IntBuf, call, refused, same_f32

pytestmark = pytest.mark.gpu
F32 = torch.float32
EPS = NR.EPS


def _dev():
    return torch.device("cuda:0")


_TABLES = {}


def _tables(n_in, S, antialias):
    """device copies of mdm_nn_plan(n_in, S): (first, count, weight, taps), made once per (n_in, S, antialias)"""
    from mdm import evaluate
    key = (n_in, S, bool(antialias))
    if key not in _TABLES:
        first, count, weight, taps = evaluate.nn_plan(n_in, S, antialias)
        _TABLES[key] = (torch.from_numpy(first).to(_dev()), torch.from_numpy(count).to(_dev()), torch.from_numpy(weight).to(_dev()), taps)
    return _TABLES[key]


_IMAGES = {}


def _images(shape):
    """(float images [8][C][H][W], uint8 images, the table, the uint8 images' values) of one shape, drawn once"""
    from mdm.data import normalize_lut
    if shape not in _IMAGES:
        x = NR.kernel_images(*shape)
        u = NR.as_bytes(x)
        u[NR.CONSTANT] = 93
        lut = normalize_lut()
        _IMAGES[shape] = (x, u, lut, lut[u.long()])
    return _IMAGES[shape]


def _run(shape, kind, antialias, normalize, flip, S, first, R, pad_stride=0, pad_ld=0, shift=0, lut=None):
    """two launches of mdm_nn_rows -> (rows [R][D] of the first, the fp32 values of the stored images [8][C][H][W]).  Without
    `normalize` the one-NaN image is stored with 0.5 in the NaN's place: an unnormalised NaN is a NaN row, which is not a case."""
    C, H, W = shape
    x, u, lut0, uv = _images(shape)
    if not normalize:
        x = torch.nan_to_num(x, nan=0.5)
    lut = lut0 if lut is None else lut
    E, M = C * H * W, x.shape[0]
    stride = E + pad_stride
    D = C * S * S if S else E
    row_ld = (D + 3) // 4 * 4 + pad_ld
    if kind == 0:
        store = torch.full((M, stride), 7.5)
        store[:, :E] = x.reshape(M, E)
        sb = Buf((M * stride,), F32, _dev(), store.reshape(-1))
        values, src = x, sb.t.data_ptr()
    else:
        store = torch.full((M, stride), 201, dtype=torch.uint8)
        store[:, :E] = u.reshape(M, E)
        sb = ByteBuf(store, _dev(), shift=shift)
        values, src = lut[u.long()], sb.t.data_ptr()
    lb = Buf((256,), F32, _dev(), lut)
    (hf, hc, hw, ht), (vf, vc, vw, vt) = (_tables(W, S, antialias), _tables(H, S, antialias)) if S else ((None, None, None, 0),) * 2
    p = lambda t: None if t is None else t.data_ptr()
    outs = []
    for _ in range(2):
        rb = Buf((R, row_ld), F32, _dev())
        call("mdm_nn_rows", src, kind, stride, M, C, H, W, lb.t.data_ptr() if kind else None, first, R, normalize, flip, S,
             p(hf), p(hc), p(hw), ht, p(vf), p(vc), p(vw), vt, EPS, rb.t.data_ptr(), row_ld)
        assert rb.guards_intact(), rb.first_bad_guard()
        outs.append(rb.t.cpu())
    assert lb.guards_intact() and same_f32(lb.t, lut), "the table was modified"
    if kind == 0:
        assert sb.guards_intact() and torch.equal(sb.t.cpu().view(torch.int32), store.reshape(-1).view(torch.int32)), "an input was modified"
    else:
        assert sb.intact(), "an input was modified"
    assert same_f32(outs[0], outs[1]), "two launches differ"
    assert not bool(outs[0][:, D:].view(torch.int32).any()), "pad elements are not +0"
    return outs[0][:, :D], values


def _check(name, rows, values, first, normalize, flip, S, antialias):
    worst = 0.0
    for r in range(rows.shape[0]):
        ref, bound = NR.row_ref(values[first + r].numpy(), normalize, flip, S, antialias, EPS)
        got = rows[r].numpy()
        assert NR.inside(got, ref, bound), (name, r, NR.worst(got, ref, bound))
        if not bound.any():
            assert not got.view(np.int32).any(), (name, r, "a zero row is not +0")
        worst = max(worst, NR.worst(got, ref, bound))
    return worst


# ------------------------------------------------------------------ mdm_nn_rows
@pytest.mark.parametrize("antialias", (0, 1))
@pytest.mark.parametrize("kind", (0, 1))
@pytest.mark.parametrize("shape", NR.SHAPES, ids=str)
def test_nn_rows_inside_the_bound(shape, kind, antialias):
    """every (normalize, flip); img_stride = C H W and C H W + 3 (which moves every image off its alignment); first = 2 with
    R = 5 and R = 1; the five rows hold the one-NaN image (float storage: a zero row when normalised)"""
    from _notes import note
    for k, (normalize, flip) in enumerate([(1, 0), (1, 1), (0, 0), (0, 1)]):
        R = 1 if k == 2 else 5
        rows, values = _run(shape, kind, antialias, normalize, flip, 32, 2, R, pad_stride=3 * (k % 2), pad_ld=4 * (k // 2), shift=k)
        name = f"nn_rows {shape} kind {kind} aa {antialias} n {normalize} f {flip}"
        ratio = _check(name, rows, values, 2, normalize, flip, 32, antialias)
        note("neighbor_bounds", dict(row=name, out="rows", ratio=ratio))


@pytest.mark.parametrize("kind", (0, 1))
def test_nn_rows_without_resize(kind):
    """S = 0 at (3, 33, 47): D = 4653 is not a multiple of 4; the whole set in one launch, and first = 2 with R = 5"""
    shape = (3, 33, 47)
    for k, (normalize, flip) in enumerate([(1, 0), (1, 1), (0, 1), (0, 0)]):
        first, R = (0, 8) if k == 0 else (2, 5)
        rows, values = _run(shape, kind, 0, normalize, flip, 0, first, R, pad_stride=3 * (k % 2), pad_ld=8 * (k % 2), shift=3 * k)
        _check(f"nn_rows S=0 kind {kind} n {normalize} f {flip}", rows, values, first, normalize, flip, 0, 0)


@pytest.mark.parametrize("S", (0, 32))
def test_constant_and_nan_images_give_zero_rows(S):
    shape = (3, 33, 47)
    rows, values = _run(shape, 0, 1, 1, 0, S, 0, 8)
    for i in (NR.CONSTANT, NR.WITH_NAN):
        assert not bool(rows[i].view(torch.int32).any()), i
    assert bool(rows[0].any()) and bool(rows[2].any())
    rows, _ = _run(shape, 1, 1, 1, 0, S, 0, 8)
    assert not bool(rows[NR.CONSTANT].view(torch.int32).any())
    lut = _images(shape)[2].clone()
    byte = int(_images(shape)[1][4, 1, 5, 6])
    lut[byte] = float("nan")                                  # a table entry that is NaN: image 4 holds that byte
    rows, _ = _run(shape, 1, 1, 1, 0, S, 0, 8, lut=lut)
    held = [(i, bool((_images(shape)[1][i] == byte).any())) for i in range(8) if i != NR.CONSTANT]
    for i, has in held:
        assert bool(rows[i].view(torch.int32).any()) != has, (i, has)


def test_nn_rows_refusals_launch_nothing():
    C, H, W, S, M = 3, 8, 8, 4, 4
    E, D = C * H * W, C * S * S
    x = torch.rand(M, E)
    xb, rb, lb = Buf((M, E), F32, _dev(), x), Buf((M, D), F32, _dev()), Buf((256,), F32, _dev(), torch.rand(256))
    (hf, hc, hw, ht), (vf, vc, vw, vt) = _tables(W, S, 1), _tables(H, S, 1)
    ok = dict(src=xb.t.data_ptr(), kind=0, img_stride=E, M=M, C=C, H=H, W=W, lut=lb.t.data_ptr(), first=0, R=M, normalize=1, flip=0, S=S,
              hfirst=hf.data_ptr(), hcount=hc.data_ptr(), hweight=hw.data_ptr(), htaps=ht, vfirst=vf.data_ptr(), vcount=vc.data_ptr(),
              vweight=vw.data_ptr(), vtaps=vt, eps=EPS, rows=rb.t.data_ptr(), row_ld=D)
    bad = [dict(src=None), dict(rows=None), dict(kind=2), dict(kind=-1), dict(kind=1, lut=None), dict(M=0), dict(R=0), dict(C=0), dict(H=0),
           dict(W=0), dict(S=-1), dict(img_stride=E - 1), dict(first=-1), dict(first=1), dict(R=M + 1), dict(row_ld=D - 1),
           dict(S=0, row_ld=E - 1), dict(hfirst=None), dict(hcount=None), dict(hweight=None), dict(vfirst=None), dict(vcount=None),
           dict(vweight=None), dict(htaps=0), dict(vtaps=0), dict(C=1 << 11, H=1 << 10, W=1 << 10, img_stride=1 << 40)]
    for change in bad:
        assert refused("mdm_nn_rows", *{**ok, **change}.values()), change
    torch.cuda.synchronize()
    assert xb.guards_intact() and rb.guards_intact() and bool((rb.t.view(torch.int32) == rb.pat).all()), "a refused call wrote"
    call("mdm_nn_rows", *ok.values())                         # and the accepted call does write
    assert bool(torch.isfinite(rb.t).all())


# ------------------------------------------------------------------ mdm_nn_col_argmax
def _score(S, S_aug, row_aug):
    if S_aug is None:
        return S
    both = torch.max(S, S_aug)                                # elementwise: a NaN on either side gives NaN
    return both if row_aug is None else torch.where(row_aug.bool()[:, None], both, S)


def _same_val(got, want):
    """bit equality of the numbers, NaN where torch has NaN: torch.max of two tensors ORs a NaN lane with all ones in its vector
    body and returns the quiet NaN in its scalar tail, so the payload of the reference's NaN says nothing"""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and same_f32(got[~nan], want[~nan])


def _argmax(S, S_aug, row_aug, row0=0, ld=None, carry=None):
    """one call -> (val, idx) on the host; `carry`: the (val, idx) of the chunks before"""
    M, B = S.shape
    ld = B if ld is None else ld
    wide = lambda t: torch.cat((t, torch.full((M, ld - B), 9.0e9)), dim=1)
    sb = Buf((M, ld), F32, _dev(), wide(S))
    ab = None if S_aug is None else Buf((M, ld), F32, _dev(), wide(S_aug))
    rb = None if row_aug is None else ByteBuf(row_aug, _dev(), shift=1)
    vb, ib = Buf((B,), F32, _dev()), IntBuf(B, _dev())
    if carry is not None:
        vb.t.copy_(carry[0])
        ib.t.copy_(carry[1])
    call("mdm_nn_col_argmax", sb.t.data_ptr(), None if ab is None else ab.t.data_ptr(), None if rb is None else rb.t.data_ptr(), M, B, ld,
         row0, int(carry is not None), vb.t.data_ptr(), ib.t.data_ptr())
    for b in (sb, ab, vb, ib):
        assert b is None or b.guards_intact()
    assert same_f32(sb.t, wide(S)) and (ab is None or same_f32(ab.t, wide(S_aug))) and (rb is None or rb.intact()), "an input was modified"
    return vb.t.cpu(), ib.t.cpu()


def _aug_problem(S, M, B):
    """a mirrored matrix for S: its rows rolled (so the planted columns meet other rows: ties against S, NaN against numbers) and a
    mask over about half of the rows"""
    g = torch.Generator().manual_seed(M * 7 + B)
    S_aug = torch.roll(S, shifts=max(1, M // 3), dims=0).clone()
    return S_aug, (torch.rand(M, generator=g) < 0.5).to(torch.uint8)


@pytest.mark.parametrize("B", SR.ARGMAX_BS)
@pytest.mark.parametrize("M", SR.ARGMAX_MS)
def test_nn_col_argmax_is_torch_max_dim0_of_the_score(M, B):
    S, plan = SR.argmax_problem(M, B)
    S_aug, mask = _aug_problem(S, M, B)
    for name, (A, rows, row0, ld) in dict(plain=(None, None, 0, None), plain_row0=(None, None, 4096, B + 3), aug=(S_aug, mask, 0, None),
                                          aug_all=(S_aug, None, 17, B + 1)).items():
        want = _score(S, A, rows).max(dim=0)
        val, idx = _argmax(S, A, rows, row0=row0, ld=ld)
        assert bool(((idx >= row0) & (idx < row0 + M)).all()), (name, idx.tolist()[:8])
        assert torch.equal(idx, want.indices + row0), (name, sorted(plan), idx.tolist()[:8], want.indices.tolist()[:8])
        assert _same_val(val, want.values), (name, val.tolist()[:8], want.values.tolist()[:8])
        val2, idx2 = _argmax(S, A, rows, row0=row0, ld=ld)
        assert torch.equal(idx, idx2) and same_f32(val, val2)


@pytest.mark.parametrize("with_aug", (False, True))
@pytest.mark.parametrize("M, cut", [(1000, 256), (257, 256), (600, 1), (512, 300)])
def test_nn_col_argmax_carries_across_two_chunks(M, cut, with_aug):
    """columns with equal maxima on both sides of the chunk edge (rows cut - 1 and cut, and cut - 1 and M - 1): the earlier chunk must
    win; a NaN in the first chunk must survive a larger number and a NaN in the second"""
    B = 100
    S, plan = SR.argmax_problem(M, B)
    S[cut - 1, 0] = S[cut, 0] = 3.0
    S[cut - 1, 1] = S[M - 1, 1] = 3.5
    S[0, 2] = float("nan")
    S[M - 1, 2] = float("nan")
    S[cut, 3] = float("nan")
    S_aug, mask = _aug_problem(S, M, B) if with_aug else (None, None)
    if with_aug:
        S_aug[:, :4] = -2.0
    want = _score(S, S_aug, mask).max(dim=0)
    sl = lambda t, a, b: None if t is None else t[a:b].contiguous()
    first = _argmax(S[:cut].contiguous(), sl(S_aug, 0, cut), sl(mask, 0, cut))
    val, idx = _argmax(S[cut:].contiguous(), sl(S_aug, cut, M), sl(mask, cut, M), row0=cut, carry=first)
    assert torch.equal(idx, want.indices), (idx.tolist()[:8], want.indices.tolist()[:8])
    assert _same_val(val, want.values)
    assert idx[:4].tolist() == [cut - 1, cut - 1, 0, cut]


def test_nn_col_argmax_refusals_launch_nothing():
    sb, vb, ib = Buf((4, 8), F32, _dev(), torch.ones(4, 8)), Buf((8,), F32, _dev()), IntBuf(8, _dev())
    s, v, i = sb.t.data_ptr(), vb.t.data_ptr(), ib.t.data_ptr()
    for args in ((None, None, None, 4, 8, 8, 0, 0, v, i), (s, None, None, 4, 8, 8, 0, 0, None, i), (s, None, None, 4, 8, 8, 0, 0, v, None),
                 (s, None, None, 0, 8, 8, 0, 0, v, i), (s, None, None, 4, 0, 8, 0, 0, v, i), (s, None, None, 4, 8, 7, 0, 0, v, i),
                 (s, None, None, 4, 8, 8, -1, 0, v, i)):
        assert refused("mdm_nn_col_argmax", *args), args
    torch.cuda.synchronize()
    assert vb.guards_intact() and ib.guards_intact()
    assert bool((vb.t.view(torch.int32) == vb.pat).all()) and bool((ib.t == 0x7A7A7A7A7A7A7A7A).all()), "a refused call wrote"
