"""Route-complete fp64 parity of the attention kernels (csrc/attn.hip) and the row softmax (csrc/norm.hip).

Every row of ROWS names the fused forward and backward kernel it expects (mdm_attn_route_of before, mdm_attn_last_route after
each call) and runs on two input draws.  The forward is compared with fp64; the backward runs on CPU-made o (fp64 -> bf16) and
lse (fp64 -> fp32) and is compared with fp64 as a function of exactly those inputs, so neither direction can hide the other's
error.  Every output -- o, lse, delta, dq, dk, dv -- is checked per element against the bounds derived in tests/_bounds.py and,
for the bf16 ones, by rel-L2 against 1.5 x the storage-precision emulation on the same inputs.  Every input and output sits
inside NaN guard bands, outputs start as the NaN pattern, and a second identical launch must repeat the first bit for bit
(attn.hip has no atomics).  No row checks a subset of its outputs: the fp64 reference of the two L = 4096 rows takes 1 - 3 s.

The exact-fp32 short-sequence kernel, the multi-head VALU kernel and the row softmax get the same treatment below."""
import math

import pytest
import torch

from _bounds import (REL_L2_MARGIN, Buf, attn_bwd_ref, attn_draw, attn_fused_refs, attn_fwd_ref, check_bound, rne_bf16,
                     softmax_bwd_ref, softmax_fwd_ref)
from _notes import note

pytestmark = pytest.mark.gpu

BF, FP = 1, 0
# (N, L, C, forward route, backward route): the smallest shapes that still reach the edge
ROWS = [
    (3, 16, 32, "fwd<32>", "bwd<32>"),              # one quarter-filled tile
    (2, 80, 32, "fwd<32>", "bwd<32>"),              # last tile 16 of 64
    (1, 320, 32, "fwd<32>", "bwd<32>"),             # five tiles, never LDS-DMA
    (2, 48, 64, "fwd<64>", "bwd<64>"),
    (3, 64, 64, "fwd<64>", "bwd<64>"),
    (1, 272, 64, "fwd<64>", "bwd<64>"),             # L >= 256 but L % 64 != 0: four full tiles and a 16-key one
    (2, 16, 128, "fwd<128>", "bwd<128>"),
    (1, 208, 128, "fwd<128>", "bwd<128>"),
    (3, 16, 256, "fwd<256>", "bwd<256>"),
    (2, 64, 256, "fwd<256>", "bwd<256>"),
    (1, 144, 256, "fwd<256>", "bwd<256>"),
    (2, 256, 64, "fwd_dma<64>", "bwd_dma<64>"),     # four tiles: the three-stage prologue plus two steady steps
    (1, 320, 64, "fwd_dma<64>", "bwd_dma<64>"),
    (3, 256, 128, "fwd_dma<128>", "bwd_dma<128>"),
    (1, 1024, 128, "fwd_dma<128>", "bwd_dma<128>"),
    (2, 256, 256, "fwd_dma<256>", "bwd_dma<256>"),  # cfg3's shape: the two-stage pipeline
    (1, 512, 256, "fwd_dma<256>", "bwd_dma<256>"),
    (1, 4096, 256, "fwd_dma<256>", "bwd_dma<256>"),  # the backward's limit: 160 KiB of LDS
    (1, 4096, 32, "fwd<32>", "bwd<32>"),            # ... and in the register-staged kernel
]
# Routes no row reaches, with the proof that none can.  (None: every fused kernel is reachable.)
EXCLUDED = {}


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _untouched(b):
    """the whole allocation, data included, still holds the guard pattern"""
    return bool((b.raw.view(b.ity) == b.pat).all())


def _assert_guards(bufs, what):
    for name, b in bufs.items():
        assert b.guards_intact(), f"{what}: guard band of {name} touched at (below, above) = {b.first_bad_guard()}"


def _run_fused(qkv, do, o_in, lse_in, N, L, C, scale, fwd, bwd):
    """forward, then backward on the GIVEN o / lse, into NaN-filled guarded buffers -> dict of Bufs"""
    from mdm import _lib, ops
    dev = _dev()
    B = dict(qkv=Buf((N, L, 3 * C), torch.bfloat16, dev, qkv), do=Buf((N, L, C), torch.bfloat16, dev, do),
             o_in=Buf((N, L, C), torch.bfloat16, dev, o_in), lse_in=Buf((N, L), torch.float32, dev, lse_in),
             o=Buf((N, L, C), torch.bfloat16, dev), lse=Buf((N, L), torch.float32, dev),
             delta=Buf((N, L), torch.float32, dev), dqkv=Buf((N, L, 3 * C), torch.bfloat16, dev))
    ops.attn_fwd(BF, B["qkv"].t, B["o"].t, B["lse"].t, N, L, C, scale)
    assert _lib.attn_last_route() == fwd
    ops.attn_bwd(BF, B["qkv"].t, B["o_in"].t, B["do"].t, B["lse_in"].t, B["delta"].t, B["dqkv"].t, N, L, C, scale)
    assert _lib.attn_last_route() == bwd
    torch.cuda.synchronize()
    return B


@pytest.mark.parametrize("kind", ["flat", "peaked"])
@pytest.mark.parametrize("row", ROWS, ids=[f"{r[3]}-{r[0]}x{r[1]}x{r[2]}" for r in ROWS])
def test_fused_route_parity(row, kind):
    from mdm import _lib
    N, L, C, fwd, bwd = row
    assert (_lib.attn_route_of(0, BF, L, C), _lib.attn_route_of(1, BF, L, C)) == (fwd, bwd)
    qkv, do = attn_draw(N, L, C, kind, seed=1000 + L + C)
    scale = 1.0 / math.sqrt(C)
    R = attn_fused_refs(qkv, do, scale)
    B = _run_fused(qkv, do, R["o_in"], R["lse_in"], N, L, C, scale, fwd, bwd)
    _assert_guards(B, f"{fwd}/{bwd}")
    got = dict(o=B["o"].t, lse=B["lse"].t, delta=B["delta"].t, dq=B["dqkv"].t[..., :C], dk=B["dqkv"].t[..., C:2 * C],
               dv=B["dqkv"].t[..., 2 * C:])
    for name in ("o", "lse", "delta", "dq", "dk", "dv"):
        ref, bound = R[name]
        ratio, rel = check_bound(f"{fwd if name in ('o', 'lse') else bwd} {N}x{L}x{C} {kind} {name}", got[name], ref, bound)
        rec = dict(route=fwd if name in ("o", "lse") else bwd, N=N, L=L, C=C, draw=kind, out=name, ratio=ratio, rel_l2=rel)
        if name in R["emu"]:
            emu = float((R["emu"][name] - ref).norm() / ref.norm())
            rec.update(emu_rel_l2=emu)
        note("attn_routes", rec)
        if name in R["emu"]:
            assert rel <= REL_L2_MARGIN * emu, f"{name}: rel-L2 {rel:.3e} above {REL_L2_MARGIN} x the storage precision's {emu:.3e}"
    # the same launches again, into fresh buffers: the same bits
    B2 = _run_fused(qkv, do, R["o_in"], R["lse_in"], N, L, C, scale, fwd, bwd)
    for name in ("o", "lse", "delta", "dqkv"):
        assert torch.equal(_bits(B[name].t), _bits(B2[name].t)), f"{name} differs between two identical launches"


def test_every_fused_route_is_reached():
    from mdm import _lib
    names = set(_lib.attn_route_names())
    assert len(names) == 14 and set(EXCLUDED) <= names
    hit = {r for row in ROWS for r in row[3:]}
    assert hit <= names, hit - names
    missing = names - hit - set(EXCLUDED)
    assert not missing, f"routes no row reaches: {sorted(missing)}"


def test_fused_refusals_write_nothing():
    """An unsupported request (L = 24, C = 96, fp32) and a backward at L = 4112 come back as errors through mdm_last_error, launch
    nothing (no route) and leave every output as it was."""
    from mdm import _lib, ops
    dev = _dev()
    N, L, C = 2, 24, 96
    qkv = Buf((N, L, 3 * C), torch.float32, dev, torch.randn(N, L, 3 * C))
    o, lse = Buf((N, L, C), torch.float32, dev), Buf((N, L), torch.float32, dev)
    assert not ops.attn_supported(FP, L, C) and _lib.attn_route_of(0, FP, L, C) is None
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.attn_fwd(FP, qkv.t, o.t, lse.t, N, L, C, 0.1)
    assert _lib.attn_last_route() == "none"
    N, L, C = 1, 4112, 64
    assert ops.attn_supported(BF, L, C) and _lib.attn_route_of(1, BF, L, C) is None
    qkv, do = attn_draw(N, L, C, "flat", seed=7)
    q = Buf((N, L, 3 * C), torch.bfloat16, dev, qkv)
    g, oi = Buf((N, L, C), torch.bfloat16, dev, do), Buf((N, L, C), torch.bfloat16, dev, do)
    li = Buf((N, L), torch.float32, dev, torch.zeros(N, L))
    delta, dqkv = Buf((N, L), torch.float32, dev), Buf((N, L, 3 * C), torch.bfloat16, dev)
    with pytest.raises(RuntimeError, match="L=4112 > 4096"):
        ops.attn_bwd(BF, q.t, oi.t, g.t, li.t, delta.t, dqkv.t, N, L, C, 0.125)
    assert _lib.attn_last_route() == "none"
    torch.cuda.synchronize()
    for b in (o, lse, delta, dqkv):
        assert _untouched(b)


# ------------------------------------------------------------------ exact-fp32 short sequences
F32_SMALL = [(3, L, C) for L in (16, 32, 48, 64) for C in (64, 128, 256)] + [(100, 64, 256)]


@pytest.mark.parametrize("N,L,C", F32_SMALL)
def test_attn_f32_small_parity(N, L, C):
    """attn_f32_small_kernel<64|128|256> at all twelve supported (L, C): the output and the probabilities it leaves for the unfused
    backward, per element."""
    from mdm import ops
    dev = _dev()
    g = torch.Generator().manual_seed(N + L + C)
    qkv = torch.randn(N, L, 3 * C, generator=g)
    qkv[..., 2 * C:] += 0.5
    scale = 1.0 / math.sqrt(C)
    R = attn_fwd_ref(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], scale, "f32", p_bf16=False, want_P=True)
    assert ops.attn_f32_small_supported(L, C)
    B = dict(qkv=Buf((N, L, 3 * C), torch.float32, dev, qkv), o=Buf((N, L, C), torch.float32, dev), S=Buf((N, L, L), torch.float32, dev))
    ops.attn_f32_small_fwd(B["qkv"].t, B["o"].t, B["S"].t, N, L, C, scale)
    torch.cuda.synchronize()
    _assert_guards(B, "attn_f32_small")
    for name, key in (("o", "o"), ("S", "P")):
        ratio, rel = check_bound(f"attn_f32_small {N}x{L}x{C} {name}", B[name].t, *R[key])
        note("attn_f32_small", dict(N=N, L=L, C=C, out=name, ratio=ratio, rel_l2=rel))


@pytest.mark.parametrize("L,C", [(80, 64), (32, 96)])
def test_attn_f32_small_refusals_write_nothing(L, C):
    from mdm import ops
    dev = _dev()
    N = 2
    qkv = Buf((N, L, 3 * C), torch.float32, dev, torch.randn(N, L, 3 * C))
    o, S = Buf((N, L, C), torch.float32, dev), Buf((N, L, L), torch.float32, dev)
    assert not ops.attn_f32_small_supported(L, C)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.attn_f32_small_fwd(qkv.t, o.t, S.t, N, L, C, 0.1)
    torch.cuda.synchronize()
    assert _untouched(o) and _untouched(S)


# ------------------------------------------------------------------ many small heads
@pytest.mark.parametrize("L", [1, 17, 255, 256, 257, 300])
@pytest.mark.parametrize("D", [8, 16, 32])
@pytest.mark.parametrize("dt", [FP, BF], ids=["f32", "bf16"])
def test_attn_mh_parity(dt, D, L):
    """attn_mh_kernel<T, 8|16|32, 0|1|2> on both sides of its 256-row chunk boundary, two images and three heads (a wrong head or
    image stride shows), the backward on CPU-made o / lse: o, lse, delta ([N][H][L]), dq, dk, dv per element."""
    from mdm import ops
    dev = _dev()
    N, H = 2, 3
    C = H * D
    td, store = (torch.bfloat16, "bf16") if dt == BF else (torch.float32, "f32")
    g = torch.Generator().manual_seed(10 * L + D + dt)
    q, k, v, do = (torch.randn(N, L, C, generator=g) for _ in range(4))
    v += 0.5
    q, k, v, do = (t.to(td) for t in (q, k, v, do))
    scale = 1.0 / math.sqrt(D)
    heads = lambda t: t.reshape(N, L, H, D).permute(0, 2, 1, 3).reshape(N * H, L, D)          # [N][L][C] -> [N H][L][D]
    unheads = lambda t: t.reshape(N, H, L, D).permute(0, 2, 1, 3).reshape(N, L, C)
    R = attn_fwd_ref(heads(q), heads(k), heads(v), scale, store, p_bf16=False, per_key=True)
    o_in = rne_bf16(R["o"][0]) if dt == BF else R["o"][0].float()
    lse_in = R["lse"][0].float()
    R.update(attn_bwd_ref(heads(q), heads(k), heads(v), o_in, heads(do), lse_in, scale, store, round_bf16=False))
    mk = lambda fill=None, shape=(N, L, C), ty=td: Buf(shape, ty, dev, fill if fill is not None else "nan")
    B = dict(q=mk(q), k=mk(k), v=mk(v), do=mk(do), o_in=mk(unheads(o_in)), lse_in=mk(lse_in.reshape(N, H, L), (N, H, L), torch.float32),
             o=mk(), lse=mk(None, (N, H, L), torch.float32), delta=mk(None, (N, H, L), torch.float32), dq=mk(), dk=mk(), dv=mk())
    ops.attn_mh_fwd(dt, B["q"].t, B["k"].t, B["v"].t, B["o"].t, B["lse"].t, N, L, C, H, scale)
    ops.attn_mh_bwd(dt, B["q"].t, B["k"].t, B["v"].t, B["o_in"].t, B["do"].t, B["lse_in"].t, B["delta"].t, B["dq"].t, B["dk"].t,
                    B["dv"].t, N, L, C, H, scale)
    torch.cuda.synchronize()
    _assert_guards(B, "attn_mh")
    for name in ("o", "lse", "delta", "dq", "dk", "dv"):
        ref, bound = R[name]
        if name in ("lse", "delta"):
            ref, bound = ref.reshape(N, H, L), bound.reshape(N, H, L)
        else:
            ref, bound = unheads(ref), unheads(bound)
        ratio, rel = check_bound(f"attn_mh {store} D={D} L={L} {name}", B[name].t, ref, bound)
        note("attn_mh", dict(dtype=store, D=D, L=L, out=name, ratio=ratio, rel_l2=rel))


# ------------------------------------------------------------------ row softmax
@pytest.mark.parametrize("rows,L", [(5, 16), (7, 63), (9, 64), (6, 65), (3, 1000), (2, 4096)])
@pytest.mark.parametrize("dt", [FP, BF], ids=["f32", "bf16"])
def test_softmax_parity(dt, rows, L):
    """softmax_fwd/bwd_kernel at the row lengths of the unfused attention path, row counts that leave waves idle in the last
    workgroup, in place inside guards: scores of amplitude 3 with one entry per row at +30."""
    from mdm import ops
    dev = _dev()
    td, store = (torch.bfloat16, "bf16") if dt == BF else (torch.float32, "f32")
    g = torch.Generator().manual_seed(rows + L + dt)
    x = 3.0 * torch.randn(rows, L, generator=g)
    x[torch.arange(rows), torch.randint(0, L, (rows,), generator=g)] += 30.0
    x = x.to(td)
    P, Pb = softmax_fwd_ref(x, store)
    S = Buf((rows, L), td, dev, x)
    ops.softmax_fwd(dt, S.t, rows, L)
    torch.cuda.synchronize()
    _assert_guards(dict(S=S), "softmax_fwd")
    ratio, rel = check_bound(f"softmax_fwd {store} {rows}x{L}", S.t, P, Pb)
    note("softmax", dict(dtype=store, rows=rows, L=L, out="fwd", ratio=ratio, rel_l2=rel))
    # the backward's P: the reference's probabilities as stored -- of these scores (nearly one-hot rows: g - sum P g cancels on the
    # dominant entry) and of the same scores without the +30 entry (every entry carries weight)
    gr = torch.randn(rows, L, generator=g).to(td)
    for tag, P64 in (("peaked", P), ("flat", torch.softmax(3.0 * torch.randn(rows, L, generator=g).double(), -1))):
        P_in = rne_bf16(P64) if dt == BF else P64.float()
        dS, dSb = softmax_bwd_ref(P_in, gr, store)
        Pg, G = Buf((rows, L), td, dev, P_in), Buf((rows, L), td, dev, gr)
        ops.softmax_bwd(dt, Pg.t, G.t, rows, L)
        torch.cuda.synchronize()
        _assert_guards(dict(P=Pg, dP=G), "softmax_bwd")
        ratio, rel = check_bound(f"softmax_bwd {store} {rows}x{L} {tag}", G.t, dS, dSb)
        note("softmax", dict(dtype=store, rows=rows, L=L, out="bwd_" + tag, ratio=ratio, rel_l2=rel))
