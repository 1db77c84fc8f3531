"""The one-tile bodies of the fused attention kernels (csrc/attn.hip: attn_fwd_tile1, attn_bwd_dq_tile1, attn_bwd_dkv_tile1), which
serve every L <= 64 under the route names fwd<C> / bwd<C>.

Every L in {16, 32, 48, 64} x head width in {32, 64, 128, 256} at N = 3, plus N = 33 at (64, 256) and (16, 256) -- the train step's
two shapes with an image count no workgroups-per-image factor divides -- on both draws of attn_draw.  As in test_attn_routes_gpu:
inputs inside NaN guard bands, outputs pre-filled with the NaN pattern, the backward on CPU-made o (fp64 -> bf16) and lse
(fp64 -> fp32) so that neither direction hides the other, every element of o, lse, delta, dq, dk, dv against its fp64 bound of
tests/_bounds.py, the bf16 outputs also by rel-L2 against REL_L2_MARGIN x the storage-precision emulation, guards intact, a second
identical launch bit-equal, route names asserted before and after the launches.

test_poisoned_tail: the kernels stage only the L real rows and skip 16-row blocks beyond L.  With every buffer allocated for 64
rows and rows L .. 63 holding NaN, a row that is staged or multiplied without its mask turns the outputs NaN; rows >= L of
the outputs must come back untouched."""
import math

import pytest
import torch

from _bounds import REL_L2_MARGIN, Buf, attn_draw, attn_fused_refs, check_bound
from _notes import note

pytestmark = pytest.mark.gpu

BF = 1
CASES = [(3, L, C) for L in (16, 32, 48, 64) for C in (32, 64, 128, 256)] + [(33, 64, 256), (33, 16, 256)]
OUTS = ("o", "lse", "delta", "dq", "dk", "dv")


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _launch(qkv, do, o_in, lse_in, N, L, C, scale, rows=None):
    """forward, then backward on the GIVEN o / lse, into NaN-filled guarded buffers of `rows` (default L) rows per image: rows
    beyond L keep the NaN pattern in the inputs too -> dict of Bufs"""
    from mdm import _lib, ops
    dev, R = _dev(), rows or L
    B = dict(qkv=Buf((N, R, 3 * C), torch.bfloat16, dev), do=Buf((N, R, C), torch.bfloat16, dev),
             o_in=Buf((N, R, C), torch.bfloat16, dev), lse_in=Buf((N, R), torch.float32, dev),
             o=Buf((N, R, C), torch.bfloat16, dev), lse=Buf((N, R), torch.float32, dev),
             delta=Buf((N, R), torch.float32, dev), dqkv=Buf((N, R, 3 * C), torch.bfloat16, dev))
    for name, src in (("qkv", qkv), ("do", do), ("o_in", o_in), ("lse_in", lse_in)):
        B[name].t[:, :L].copy_(src.to(B[name].dtype))
    assert (_lib.attn_route_of(0, BF, L, C), _lib.attn_route_of(1, BF, L, C)) == (f"fwd<{C}>", f"bwd<{C}>")
    ops.attn_fwd(BF, B["qkv"].t, B["o"].t, B["lse"].t, N, L, C, scale)
    assert _lib.attn_last_route() == f"fwd<{C}>"
    ops.attn_bwd(BF, B["qkv"].t, B["o_in"].t, B["do"].t, B["lse_in"].t, B["delta"].t, B["dqkv"].t, N, L, C, scale)
    assert _lib.attn_last_route() == f"bwd<{C}>"
    torch.cuda.synchronize()
    for name, b in B.items():
        assert b.guards_intact(), f"guard band of {name} touched at (below, above) = {b.first_bad_guard()}"
    return B


def _outputs(B, L, C):
    d = B["dqkv"].t[:, :L]
    return dict(o=B["o"].t[:, :L], lse=B["lse"].t[:, :L], delta=B["delta"].t[:, :L], dq=d[..., :C], dk=d[..., C:2 * C], dv=d[..., 2 * C:])


def _check(tag, got, R, N, L, C, kind):
    for name in OUTS:
        ref, bound = R[name]
        ratio, rel = check_bound(f"{tag} {N}x{L}x{C} {kind} {name}", got[name], ref, bound)
        rec = dict(case=tag, N=N, L=L, C=C, draw=kind, out=name, ratio=ratio, rel_l2=rel)
        if name in R["emu"]:
            emu = float((R["emu"][name] - ref).norm() / ref.norm())
            rec.update(emu_rel_l2=emu)
        note("attn_small", rec)
        print(rec)
        if name in R["emu"]:
            assert rel <= REL_L2_MARGIN * emu, f"{name}: rel-L2 {rel:.3e} above {REL_L2_MARGIN} x the storage precision's {emu:.3e}"


@pytest.mark.parametrize("kind", ["flat", "peaked"])
@pytest.mark.parametrize("N,L,C", CASES, ids=[f"{n}x{l}x{c}" for n, l, c in CASES])
def test_one_tile_parity(N, L, C, kind):
    qkv, do = attn_draw(N, L, C, kind, seed=1000 + L + C)
    scale = 1.0 / math.sqrt(C)
    R = attn_fused_refs(qkv, do, scale)
    B = _launch(qkv, do, R["o_in"], R["lse_in"], N, L, C, scale)
    _check("one_tile", _outputs(B, L, C), R, N, L, C, kind)
    B2 = _launch(qkv, do, R["o_in"], R["lse_in"], N, L, C, scale)
    for name in ("o", "lse", "delta", "dqkv"):
        assert torch.equal(_bits(B[name].t), _bits(B2[name].t)), f"{name} differs between two identical launches"


@pytest.mark.parametrize("C", [32, 64, 128, 256])
@pytest.mark.parametrize("L", [16, 48])
def test_poisoned_tail(L, C):
    N, ROWS, kind = 1, 64, "flat"
    qkv, do = attn_draw(N, L, C, kind, seed=2000 + L + C)
    scale = 1.0 / math.sqrt(C)
    R = attn_fused_refs(qkv, do, scale)
    B = _launch(qkv, do, R["o_in"], R["lse_in"], N, L, C, scale, rows=ROWS)
    for name in ("qkv", "do", "o_in"):                       # the poison is where it was put
        assert bool(torch.isnan(B[name].t[:, L:].float()).all())
    _check("poisoned_tail", _outputs(B, L, C), R, N, L, C, kind)
    for name in ("o", "lse", "delta", "dqkv"):
        b = B[name]
        assert bool((b.t[:, L:].contiguous().view(b.ity) == b.pat).all()), f"{name}: rows >= {L} were written"
