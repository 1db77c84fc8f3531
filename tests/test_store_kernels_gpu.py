"""The kernels of csrc/optim.hip apart from the update sweep, through the C ABI, each against its own statement (tests/_bounds.py, the
section on the store kernels): mdm_sqnorm inside its fp64 bound and exact on the one-hot rows; mdm_cast_bf16, the two fills,
mdm_transpose_shadow_bf16, mdm_split_shadow and mdm_split_shadow_t bit for bit.  Rows: tests/_store_rows.py.

Every operand sits in a `Buf` inside NaN guard bands, destinations start as the NaN pattern, inputs must come back bit for bit and a
second launch must repeat the first.  The refusals are host checks in front of any launch."""
import pytest
import torch

import _store_rows as SR
from _bounds import Buf, split_t_want, split_want, sqnorm_geom, transpose_want
from _notes import note
from _store_rows import call, check_sqnorm, refused

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
PAT16 = 0x7FE5


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a).cpu(), _bits(b).cpu())


def _intact(bufs, inputs=()):
    for b in bufs:
        assert b.guards_intact(), b.first_bad_guard()
    for b, want in inputs:
        assert _same_bits(b.t, want.to(b.dtype)), "an input was modified"


def _sqnorm(gb, n, out=None):
    out = out or Buf((1,), F32, _dev())
    call("mdm_sqnorm", gb.t.data_ptr(), n, out.t.data_ptr())
    _intact((gb, out))
    return out.t.cpu()


# ------------------------------------------------------------------ mdm_sqnorm
@pytest.mark.parametrize("n", SR.SQNORM_NS)
def test_sqnorm_bound_onehot_rows_and_repeat(n):
    g = SR.sqnorm_row(n)
    gb = Buf((n,), F32, _dev(), g)
    y1, y2 = _sqnorm(gb, n), _sqnorm(gb, n)
    _intact((gb,), [(gb, g)])
    ratio = check_sqnorm(f"sqnorm {n}", y1[0], g)
    n4, nb, T = sqnorm_geom(n)
    note("store_eval_bounds", dict(row=f"sqnorm-{n}-nb{nb}-T{T}", out="sqnorm", ratio=ratio))
    assert _same_bits(y1, y2), "two identical launches differ"
    for p in SR.onehot_positions(n):
        gb.t.zero_()
        gb.t[p] = 3.0
        y = _sqnorm(gb, n)
        assert float(y[0]) == 9.0, f"n = {n}: 3.0 at element {p} gives {float(y[0])!r}, not 9.0"


def test_sqnorm_small_call_after_a_large_one():
    """the module-global partials of the large call (1024 of them) are still there: the second stage of the small one reads its own 5"""
    nl, ns = SR.SQNORM_NS[-1], SR.SQNORM_NS[6]
    big, small = SR.sqnorm_row(nl), SR.sqnorm_row(ns)
    bb, sb = Buf((nl,), F32, _dev(), big), Buf((ns,), F32, _dev(), small)
    alone = _sqnorm(sb, ns)
    _sqnorm(bb, nl)
    after = _sqnorm(sb, ns)
    check_sqnorm("sqnorm small after large", after[0], small)
    assert _same_bits(alone, after), "the stale partials of the large call reached the small one"
    _sqnorm(Buf((4,), F32, _dev(), torch.zeros(4)), 4)                     # one workgroup: partial 0 alone is rewritten
    again = _sqnorm(sb, ns)
    assert _same_bits(after, again)


def test_sqnorm_refusals():
    gb, out = Buf((64,), F32, _dev(), torch.ones(64)), Buf((1,), F32, _dev())
    g, o = gb.t.data_ptr(), out.t.data_ptr()
    for args in ((g, 0, o), (g, -4, o), (None, 64, o), (g, 64, None), (g + 4, 32, o)):
        assert refused("mdm_sqnorm", *args), args
    torch.cuda.synchronize()
    _intact((gb, out), [(gb, torch.ones(64))])
    assert bool((_bits(out.t) == out.pat).all()), "a refused call wrote its output"


# ------------------------------------------------------------------ mdm_cast_bf16, mdm_fill_f32
@pytest.mark.parametrize("n", SR.FLAT_NS)
def test_cast_bf16_bit_for_bit(n):
    x = SR.cast_row(n)
    want = SR.cast_want(x)
    outs = []
    for _ in range(2):
        xb, yb = Buf((n,), F32, _dev(), x), Buf((n,), BF, _dev())
        call("mdm_cast_bf16", xb.t.data_ptr(), yb.t.data_ptr(), n)
        _intact((xb, yb), [(xb, x)])
        outs.append(_bits(yb.t).cpu())
    got = outs[0]
    if not SR.cast_matches(got, want, x):
        bad = ((got != want) & ~torch.isnan(x)).nonzero().flatten()[:6].tolist()
        raise AssertionError(f"cast_bf16 n = {n}: (index, fp32 bits, got, want) "
                             f"{[(i, hex(int(_bits(x)[i]) & 0xFFFFFFFF), hex(int(got[i]) & 0xFFFF), hex(int(want[i]) & 0xFFFF)) for i in bad]}")
    assert torch.equal(outs[0], outs[1])
    assert n == 1 or not SR.cast_matches(SR.cast_want(x, "truncate"), got, x), "the row cannot tell rounding from truncation"


@pytest.mark.parametrize("v", SR.FILL_VALUES)
@pytest.mark.parametrize("n", SR.FLAT_NS)
def test_fill_f32_bits(n, v):
    yb = Buf((n,), F32, _dev())
    call("mdm_fill_f32", yb.t.data_ptr(), v, n)
    _intact((yb,))
    want = int(torch.tensor([v], dtype=F32).view(torch.int32))
    assert bool((_bits(yb.t) == want).all()), f"fill({v!r}, n = {n}): {int((_bits(yb.t) != want).sum())} elements differ"


def test_cast_and_fill_refusals_and_the_emptycall():
    from mdm import _lib
    xb, yb, fb = Buf((64,), F32, _dev(), torch.ones(64)), Buf((64,), BF, _dev()), Buf((64,), F32, _dev())
    x, y, f = xb.t.data_ptr(), yb.t.data_ptr(), fb.t.data_ptr()
    for args in ((None, y, 64), (x, None, 64), (x, y, -1)):
        assert refused("mdm_cast_bf16", *args), args
    for args in ((None, 1.0, 64), (f, 1.0, -1)):
        assert refused("mdm_fill_f32", *args), args
    lib = _lib.load()
    assert lib.mdm_cast_bf16(x, y, 0, _lib.stream()) == 0 and lib.mdm_fill_f32(f, 1.0, 0, _lib.stream()) == 0
    torch.cuda.synchronize()
    _intact((xb, yb, fb), [(xb, torch.ones(64))])
    assert bool((_bits(yb.t) == yb.pat).all()) and bool((_bits(fb.t) == fb.pat).all()), "a refused or empty call wrote"


# ------------------------------------------------------------------ mdm_fill_segments_f32
@pytest.mark.parametrize("v", [0.0, -0.0, 2.5])
def test_fill_segments_writes_its_segments_and_nothing_else(v):
    n = SR.FILL_SEG_SIZE
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n, generator=g)
    xb = Buf((n,), F32, _dev(), x)
    segs = torch.tensor(SR.FILL_SEGS, dtype=torch.int64, device=_dev())
    call("mdm_fill_segments_f32", xb.t.data_ptr(), segs.data_ptr(), len(SR.FILL_SEGS), v)
    _intact((xb,))
    assert segs.cpu().tolist() == [list(s) for s in SR.FILL_SEGS]
    inside = torch.zeros(n, dtype=torch.bool)
    for o, ln in SR.FILL_SEGS:
        assert o % 4 == 0 and ln % 4 == 0 and ln <= 4096 and not bool(inside[o:o + ln].any())
        inside[o:o + ln] = True
    got, vb = _bits(xb.t).cpu(), int(torch.tensor([v], dtype=F32).view(torch.int32))
    assert bool((got[inside] == vb).all()), "a segment element was not filled"
    assert torch.equal(got[~inside], _bits(x)[~inside]), "an element outside the segments changed"


def test_fill_segments_refusals():
    xb = Buf((64,), F32, _dev(), torch.ones(64))
    segs = torch.tensor([[0, 8]], dtype=torch.int64, device=_dev())
    for args in ((None, segs.data_ptr(), 1, 0.0), (xb.t.data_ptr(), None, 1, 0.0), (xb.t.data_ptr(), segs.data_ptr(), 0, 0.0)):
        assert refused("mdm_fill_segments_f32", *args), args
    torch.cuda.synchronize()
    _intact((xb,), [(xb, torch.ones(64))])


# ------------------------------------------------------------------ mdm_transpose_shadow_bf16
def test_transpose_shadow_table_of_seven_filters():
    """(taps, Cout, Cin) from the thin end (Cout = 8) to channel counts that are no multiple of 64, back to back with a gap that
    belongs to no filter: every filter transposed per tap, every other byte of PT as it was"""
    filters, n = SR.pack_filters(SR.TRANSPOSE_FILTERS, SR.TRANSPOSE_GAP_AFTER)
    g = torch.Generator().manual_seed(4)
    src = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g, dtype=torch.int32).to(torch.int16)
    rows = SR.transpose_tiles(filters)
    tiles = torch.tensor(rows, dtype=torch.int64, device=_dev())
    outs = []
    for _ in range(2):
        pb, pt = Buf((n,), BF, _dev(), src.view(BF)), Buf((n,), BF, _dev())
        call("mdm_transpose_shadow_bf16", pb.t.data_ptr(), pt.t.data_ptr(), tiles.data_ptr(), len(rows))
        _intact((pb, pt), [(pb, src.view(BF))])
        outs.append(_bits(pt.t).cpu())
    got, want = outs[0], transpose_want(src, filters)
    inside = torch.zeros(n, dtype=torch.bool)
    for off, t, co, ci in filters:
        inside[off:off + t * co * ci] = True
        bad = got[off:off + t * co * ci] != want[off].reshape(-1)
        assert not bool(bad.any()), f"filter {(t, co, ci)}: {int(bad.sum())} elements differ, first at {int(bad.nonzero()[0])}"
    assert int((~inside).sum()) >= 40 and bool((got[~inside] == PAT16).all()), "a byte outside the filters was written"
    assert torch.equal(outs[0], outs[1])


def test_transpose_shadow_through_the_param_store():
    """the tile table ParamStore.allocate builds: wT(name) == w(name).transpose(1, 2) bit for bit for every filter"""
    from mdm import BF16
    from mdm.unet import ParamStore
    st = ParamStore()
    names = []
    for i, (t, co, ci) in enumerate(SR.TRANSPOSE_FILTERS):
        name = f"f{i}.weight"
        st.declare(name, "conv" if t == 9 else "convlin", (co, ci, 3, 3) if t == 9 else (co, ci), (t, co, ci))
        st.declare(f"f{i}.bias", "vecpad", (co,), (co,))
        if i % 2:
            st.declare(f"n{i}.weight", "vec", (co + 3,), (co + 3,))
        names.append(name)
    st.allocate(_dev(), BF16)
    assert st.tiles.shape[0] == len(SR.transpose_tiles([(0,) + f for f in SR.TRANSPOSE_FILTERS]))
    g = torch.Generator().manual_seed(6)
    src = torch.randint(-2 ** 15, 2 ** 15, (st.size,), generator=g, dtype=torch.int32).to(torch.int16)
    st.Pb.copy_(src.view(BF))
    st.PbT.view(torch.int16).fill_(PAT16)
    st.emit_transposed_shadow()
    torch.cuda.synchronize()
    assert torch.equal(_bits(st.Pb).cpu(), src)
    inside = torch.zeros(st.size, dtype=torch.bool)
    for name in names:
        e = st.entries[name]
        inside[e.off:e.off + e.n] = True
        assert _same_bits(st.wT(name), st.w(name).transpose(1, 2).contiguous()), name
    assert bool((_bits(st.PbT).cpu()[~inside] == PAT16).all()), "PbT was written outside the filters"


def test_transpose_shadow_refusals():
    pb = Buf((64,), BF, _dev(), torch.ones(64))
    tiles = torch.tensor([[0, 8, 8, 0, 0]], dtype=torch.int64, device=_dev())
    p, t = pb.t.data_ptr(), tiles.data_ptr()
    for args in ((None, p, t, 1), (p, None, t, 1), (p, p, None, 1), (p, p, t, 0)):
        assert refused("mdm_transpose_shadow_bf16", *args), args
    torch.cuda.synchronize()
    _intact((pb,), [(pb, torch.ones(64))])


# ------------------------------------------------------------------ mdm_split_shadow, mdm_split_shadow_t
def test_split_shadows_three_segments_one_past_the_first_trip():
    """one call each over a 3x3 64 x 96, a 3x3 256 x 256 (589 824 elements: the grid covers 131 072 per trip) and a 1x1 32 x 32 filter with a
    gap behind the first: the numpy restatement of the layout bit for bit, everything outside the segments as it was"""
    filters, n, P = SR.split_problem()
    segs = [(off, t * co * ci) for off, t, co, ci in filters]
    dev = _dev()
    pb, ps, pst = Buf((n,), F32, dev, P), Buf((n,), F32, dev), Buf((n,), F32, dev)
    s2 = torch.tensor(segs, dtype=torch.int64, device=dev)
    s4 = torch.tensor(filters, dtype=torch.int64, device=dev)
    call("mdm_split_shadow", pb.t.data_ptr(), ps.t.data_ptr(), s2.data_ptr(), len(segs))
    call("mdm_split_shadow_t", pb.t.data_ptr(), pst.t.data_ptr(), s4.data_ptr(), len(filters))
    _intact((pb, ps, pst), [(pb, P)])
    inside = torch.zeros(n, dtype=torch.bool)
    for off, ln in segs:
        inside[off:off + ln] = True
    for what, buf, want in (("split_shadow", ps, split_want(P, segs)), ("split_shadow_t", pst, split_t_want(P, filters))):
        got = buf.t.cpu()
        for (off, ln), f in zip(segs, filters):
            bad = got[off:off + ln].view(torch.int16) != want[off]
            assert not bool(bad.any()), f"{what} {f[1:]}: {int(bad.sum())} halves differ, first at {int(bad.nonzero()[0])} of {2 * ln}"
        assert bool((got.view(torch.int32)[~inside] == buf.pat).all()), f"{what}: an element outside the segments was written"
