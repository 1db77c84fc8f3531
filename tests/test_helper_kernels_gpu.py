"""The helper kernels at the end of csrc/norm.hip, each against its own statement: the fallback of the time-embedding path
(timestep_embedding, silu_fwd, silu_bwd: batches above 128 or an odd hid) and colsum inside the fp64 bounds of tests/_bounds.py; add,
add3, sumpool2 with acc = 1 and the layout converters bit for bit; and one row each of the four kernels that share the grid-stride
loop (add, sumpool2, avgpool2, upsample2) with just over 4096 x 256 vectors -- the grid is capped at 4096 workgroups, so those rows are
the only ones whose lanes take a second trip, which is what the training step's big maps do.

Every operand sits in a `Buf` inside NaN guard bands, overwrite outputs start as the NaN pattern, inputs must come back bit for bit
and a second launch must repeat the first bit for bit (except the bf16 colsum over several images: float atomics)."""
import pytest
import torch

from _bounds import Buf, check_bound, colsum_ref, silu_bwd_ref, silu_ref, temb_ref
from _notes import note
from _temb_rows import COLSUM_CS, VARIANTS, colsum_problem, colsum_rows, timesteps

pytestmark = pytest.mark.gpu
DT = {"f32": 0, "bf16": 1}
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
F32 = torch.float32
SHAPES = [(2, 1, 1, 8), (3, 3, 5, 40), (2, 16, 16, 128)]        # (N, H, W, C) of tests/test_resample_gpu.py
BIG_VEC = 4096 * 256                                            # vectors one trip of the capped grid covers


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a).cpu(), _bits(b).cpu())


def _intact(bufs, inputs=()):
    for b in bufs:
        assert b.guards_intact(), b.first_bad_guard()
    for b, want in inputs:
        assert _same_bits(b.t, want.to(b.dtype)), "an input was modified"


# ------------------------------------------------------------------ the fallback of the time-embedding path
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("dim", [4, 64, 128, 129])
def test_timestep_embedding_bounds(dim, N, variant):
    from mdm import ops
    t = timesteps(N, dim + N)
    ref, bound = temb_ref(t, dim, *variant)
    outs = []
    for v in ([None] if variant == (0, 1.0) else []) + [variant, variant]:      # mdm_timestep_embedding is variant (0, 1) of ..._embedding2
        tb, y = Buf((N,), F32, _dev(), t), Buf((N, dim), F32, _dev())
        ops.timestep_embedding(tb.t, N, dim, y.t, variant=v)
        torch.cuda.synchronize()
        _intact((tb, y), [(tb, t)])
        ratio, _ = check_bound(f"temb {dim} {N} {variant}", y.t, ref, bound)
        note("temb_bounds", dict(row=f"temb_kernel-{N}x{dim}-v{variant[0]}{variant[1]:g}", out="y", ratio=ratio))
        if dim & 1:
            assert bool((_bits(y.t)[:, -1] == 0).all()), "the pad column of an odd dim is +0"
        outs.append(y.t)
    assert all(_same_bits(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_silu_fwd_bwd_bounds(n, acc):
    from mdm import ops
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=g) * 40 - 20
    x[0], x[-1] = -20.0, (20.0 if n > 1 else -20.0)
    dy, prior = torch.randn(n, generator=g), torch.randn(n, generator=g)
    outs = []
    for _ in range(2):
        xb, db = Buf((n,), F32, _dev(), x), Buf((n,), F32, _dev(), dy)
        yb, gb = Buf((n,), F32, _dev()), Buf((n,), F32, _dev(), prior if acc else "nan")
        ops.silu_fwd(xb.t, yb.t, n)
        ops.silu_bwd(xb.t, db.t, gb.t, acc, n)
        torch.cuda.synchronize()
        _intact((xb, db, yb, gb), [(xb, x), (db, dy)])
        outs.append((yb.t, gb.t))
    r1, _ = check_bound(f"silu_fwd {n}", outs[0][0], *silu_ref(x))
    r2, _ = check_bound(f"silu_bwd {n} acc={acc}", outs[0][1], *silu_bwd_ref(x, dy, prior if acc else None))
    note("temb_bounds", dict(row=f"silu-{n}-acc{acc}", out="fwd", ratio=r1))
    note("temb_bounds", dict(row=f"silu-{n}-acc{acc}", out="bwd", ratio=r2))
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1])


# ------------------------------------------------------------------ colsum
def _run_colsum(dt, d, P, N, C, per_img, acc_img, dbias, pi, pb):
    from mdm import ops
    dev = _dev()
    B = dict(dY=Buf((N, P, C), TD[dt], dev, d))
    pim, ld = None, 0
    if per_img:
        ld, off = (C, 0) if per_img == "dense" else (C + 16, 8)
        B["per_img"] = Buf((N, ld), F32, dev)
        pim = B["per_img"].t.reshape(-1)[off:]
        if acc_img:
            B["per_img"].t[:, off:off + C].copy_(pi)
    if dbias:
        B["dbias"] = Buf((C,), F32, dev, pb)
    ops.colsum(DT[dt], B["dY"].t, N, P, C, per_img=pim, ld=ld, acc_img=acc_img, dbias=B["dbias"].t if dbias else None)
    torch.cuda.synchronize()
    _intact(B.values(), [(B["dY"], d)])
    got = {}
    if per_img:
        off = 0 if per_img == "dense" else 8
        got["per_img"] = B["per_img"].t[:, off:off + C]
        iv = B["per_img"].t.view(torch.int32)
        assert bool((iv[:, :off] == B["per_img"].pat).all()) and bool((iv[:, off + C:] == B["per_img"].pat).all()), "pad columns written"
    if dbias:
        got["dbias"] = B["dbias"].t
    return got


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", COLSUM_CS)
def test_colsum_bounds(dt, C):
    """C = 8: one vector of a 64-channel workgroup; 72 and 136: a partial last workgroup; P below, at and above the 32 pixel lanes"""
    for P, N, per_img, acc_img, dbias in colsum_rows(dt, C):
        d, pi, pb = colsum_problem(dt, C, P, N)
        R = colsum_ref(d, pi if acc_img else None, pb)
        got = _run_colsum(dt, d, P, N, C, per_img, acc_img, dbias, pi, pb)
        again = _run_colsum(dt, d, P, N, C, per_img, acc_img, dbias, pi, pb)
        for name, y in got.items():
            ratio, _ = check_bound(f"colsum {dt} {N}x{P}x{C} {per_img} acc={acc_img} {name}", y, *R[name])
            note("temb_bounds", dict(row=f"colsum-{dt}-{N}x{P}x{C}-{per_img}-acc{acc_img}", out=name, ratio=ratio))
            if dt == "f32" or N == 1 or name == "per_img":          # one writer, a fixed order
                assert _same_bits(y, again[name]), f"{name} differs between two identical launches"


# ------------------------------------------------------------------ bit exact: add, add3, sumpool2 with acc = 1, the converters
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_add_and_add3_bit_for_bit(dt, shape):
    from mdm import ops
    dev, td = _dev(), TD[dt]
    g = torch.Generator().manual_seed(sum(shape))
    x, y = (torch.randn(shape, generator=g) * 1.5).to(td), torch.randn(shape, generator=g).to(td)
    want = (x.float() + y.float()).to(td)
    xb, yb = Buf(shape, td, dev, x), Buf(shape, td, dev, y)
    s1, s2, cp, al, a3 = Buf(shape, td, dev), Buf(shape, td, dev), Buf(shape, td, dev), Buf(shape, td, dev, x), Buf(shape, td, dev, x)
    ops.add3(DT[dt], s1.t, xb.t, yb.t)
    ops.add3(DT[dt], s2.t, xb.t, yb.t)
    ops.add3(DT[dt], cp.t, xb.t, None)
    ops.add_(DT[dt], al.t, yb.t)                       # mdm_add: dst is its own first operand
    ops.add3(DT[dt], a3.t, a3.t, yb.t)                 # and the same aliasing spelled out on mdm_add3
    torch.cuda.synchronize()
    _intact((xb, yb, s1, s2, cp, al, a3), [(xb, x), (yb, y)])
    assert _same_bits(s1.t.cpu(), want) and _same_bits(s2.t.cpu(), want)
    assert _same_bits(cp.t.cpu(), x), "add3(x, NULL) moves bits unchanged"
    assert _same_bits(al.t.cpu(), want) and _same_bits(a3.t.cpu(), want)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_sumpool2_accumulate_bit_for_bit(dt, shape):
    """as test_avgpool2's accumulate case: the taps in the kernel's order, then + prior, then one rounding"""
    from mdm import ops
    N, H, W, C = shape
    dev, td = _dev(), TD[dt]
    g = torch.Generator().manual_seed(3 + sum(shape))
    big = (torch.randn(N, 2 * H, 2 * W, C, generator=g) * 1.5 + 0.2).to(td)
    prior = torch.randn(shape, generator=g).to(td)
    src = Buf(big.shape, td, dev, big)
    ow, a1, a2 = Buf(shape, td, dev), Buf(shape, td, dev, prior), Buf(shape, td, dev, prior)
    ops.sumpool2(DT[dt], src.t, ow.t, 0, N, H, W, C)
    ops.sumpool2(DT[dt], src.t, a1.t, 1, N, H, W, C)
    ops.sumpool2(DT[dt], src.t, a2.t, 1, N, H, W, C)
    torch.cuda.synchronize()
    _intact((src, ow, a1, a2), [(src, big)])
    f = big.float()
    taps = ((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2]
    assert _same_bits(ow.t.cpu(), taps.to(td))
    assert _same_bits(a1.t.cpu(), (taps + prior.float()).to(td)) and _same_bits(a1.t, a2.t)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,Cp", [(3, 8), (8, 8), (5, 16)])
@pytest.mark.parametrize("shape", SHAPES)
def test_layout_converters_move_bits(dt, C, Cp, shape):
    from mdm import ops
    N, H, W, _ = shape
    dev, td = _dev(), TD[dt]
    g = torch.Generator().manual_seed(C + Cp + sum(shape))
    x = torch.randn(N, C, H, W, generator=g).to(td).float()              # fp32 values the storage type holds exactly
    xb, yb, y2 = Buf(x.shape, F32, dev, x), Buf((N, H, W, Cp), td, dev), Buf((N, H, W, Cp), td, dev)
    ops.nchw_to_nhwc(DT[dt], xb.t, yb.t, N, C, H, W, Cp)
    ops.nchw_to_nhwc(DT[dt], xb.t, y2.t, N, C, H, W, Cp)
    torch.cuda.synchronize()
    _intact((xb, yb, y2), [(xb, x)])
    y = yb.t.cpu()
    assert _same_bits(y[..., :C].contiguous(), x.permute(0, 2, 3, 1).contiguous().to(td))
    assert bool((_bits(y)[..., C:] == 0).all()), "pad channels C .. Cp - 1 are +0"
    assert _same_bits(yb.t, y2.t)
    # back: the pad channels of the source hold the NaN pattern and must not reach the result
    src = Buf((N, H, W, Cp), td, dev)
    src.t[..., :C].copy_(x.permute(0, 2, 3, 1))
    before = _bits(src.t).clone()
    zb, z2 = Buf(x.shape, F32, dev), Buf(x.shape, F32, dev)
    ops.nhwc_to_nchw(DT[dt], src.t, zb.t, N, C, H, W, Cp)
    ops.nhwc_to_nchw(DT[dt], src.t, z2.t, N, C, H, W, Cp)
    torch.cuda.synchronize()
    _intact((src, zb, z2))
    assert torch.equal(_bits(src.t), before)
    assert _same_bits(zb.t.cpu(), x) and _same_bits(zb.t, z2.t)


# ------------------------------------------------------------------ the second trip of the grid-stride loop (bf16 only)
def test_add_second_trip_of_the_grid_stride_loop():
    from mdm import ops
    dev, bf = _dev(), torch.bfloat16
    n = 8 * (BIG_VEC + 300)
    g = torch.Generator(device=dev).manual_seed(1)
    x, y = torch.randn(n, generator=g, device=dev).to(bf), torch.randn(n, generator=g, device=dev).to(bf)
    xb, yb, s, al = Buf((n,), bf, dev, x), Buf((n,), bf, dev, y), Buf((n,), bf, dev), Buf((n,), bf, dev, x)
    ops.add3(1, s.t, xb.t, yb.t)
    ops.add_(1, al.t, yb.t)
    torch.cuda.synchronize()
    _intact((xb, yb, s, al), [(xb, x), (yb, y)])
    want = (x.cpu().float() + y.cpu().float()).to(bf)
    assert _same_bits(s.t.cpu(), want) and _same_bits(al.t.cpu(), want)


def test_pool_and_upsample_second_trip_of_the_grid_stride_loop():
    from mdm import ops
    dev, bf = _dev(), torch.bfloat16
    N, H, W, C = 1, 1025, 1024, 8                                   # H W C / 8 = 4096 x 256 + 1024 vectors of the small map
    assert N * H * W * C // 8 > BIG_VEC
    g = torch.Generator(device=dev).manual_seed(2)
    big = torch.randn(N, 2 * H, 2 * W, C, generator=g, device=dev).to(bf)
    src = Buf(big.shape, bf, dev, big)
    sp, ap = Buf((N, H, W, C), bf, dev), Buf((N, H, W, C), bf, dev)
    ops.sumpool2(1, src.t, sp.t, 0, N, H, W, C)
    ops.avgpool2(1, src.t, ap.t, 0, N, H, W, C)
    torch.cuda.synchronize()
    _intact((src, sp, ap), [(src, big)])
    f = big.cpu().float()
    taps = ((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2]
    assert _same_bits(sp.t.cpu(), taps.to(bf))
    assert _same_bits(ap.t.cpu(), (0.25 * taps).to(bf))
    small = sp.t.cpu()
    del src, f, taps, big
    sm, up = Buf((N, H, W, C), bf, dev, small), Buf((N, 2 * H, 2 * W, C), bf, dev)
    ops.upsample2(1, sm.t, up.t, 0, 1.0, N, H, W, C)
    torch.cuda.synchronize()
    _intact((sm, up), [(sm, small)])
    assert _same_bits(up.t.cpu(), small.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
