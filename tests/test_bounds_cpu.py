"""CPU self-test of the error-bound checker (tests/_bounds.py): it accepts a correctly rounded bf16 convolution and rejects
each planted fault a wrong kernel could make -- a dropped tap at one border pixel, a dropped 32-channel K-chunk, the rowvec of
the neighbouring image on one tile, truncation instead of round-to-nearest-even, a write one past the end, a NaN left in an
overwrite destination, an ignored acc1.

The attention bounds the same way: a CPU emulation of the fused kernels' arithmetic (fp32 scores, 64-key online softmax, P and dS
rounded to bf16, fp32 second product, bf16 store) is accepted, and each fault a wrong kernel could make is planted into that
emulation and rejected."""
import pytest
import torch

import math

from _bounds import (REL_L2_MARGIN, Buf, attn_draw, attn_fused_refs, check, check_bound, conv_dgrad_ref, conv_fwd_ref,
                     epilogue_ref, rne_bf16, trunc_bf16, violations)

N, H, C, CO, TAPS = 3, 8, 64, 32, 9
PADS = (1, 1, 1, 1)


def _problem():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, H, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(TAPS, CO, C, generator=g) / (TAPS * C) ** 0.5).to(torch.bfloat16)
    bias = torch.randn(CO, generator=g)
    rv_ld, rv_off = CO + 16, 8
    rv = torch.randn(N * rv_ld + rv_off, generator=g)
    acc, mag = conv_fwd_ref(x, None, w, 3, 3, 1, PADS, 0)
    ref, mg = epilogue_ref(acc.reshape(-1, CO), mag.reshape(-1, CO), bias=bias, rowvec=rv, rv_ld=rv_ld, rv_off=rv_off,
                           rows_per_img=H * H)
    return x, w, bias, rv, rv_ld, rv_off, ref, mg


def _ok(y, ref, mg):
    check("conv", y, ref, mg, TAPS * C, "bf16")


def test_accepts_correctly_rounded_result():
    *_, ref, mg = _problem()
    ratio, rel = check("conv", rne_bf16(ref), ref, mg, TAPS * C, "bf16")
    assert ratio <= 1.0 and 5e-4 < rel < 3e-3


def test_rejects_dropped_tap_at_border_pixel():
    x, w, *_, ref, mg = _problem()
    y = ref.clone()
    # output pixel (image 1, row 0, col 0): drop tap (1, 1) -- the centre tap, input pixel (0, 0)
    contrib = x[1, 0, 0].double() @ w[4].double().t()
    y[1 * H * H + 0] -= contrib
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(rne_bf16(y), ref, mg)


def test_rejects_dropped_k_chunk():
    x, w, *_, ref, mg = _problem()
    xz = x.clone()
    xz[..., 32:64] = 0          # channels 32..63 of every tap missing, on the first 64-pixel tile only
    acc, _ = conv_fwd_ref(xz, None, w, 3, 3, 1, PADS, 0)
    full, _ = conv_fwd_ref(x, None, w, 3, 3, 1, PADS, 0)
    y = ref.clone()
    y[:64] += (acc - full).reshape(-1, CO)[:64]
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(rne_bf16(y), ref, mg)


def test_rejects_rowvec_of_neighbouring_image():
    x, w, bias, rv, rv_ld, rv_off, ref, mg = _problem()
    y = ref.clone()
    tile = slice(2 * H * H, 2 * H * H + 32)       # one 32-pixel tile of the last image takes image 1's rowvec
    y[tile] += (rv[rv_off + 1 * rv_ld:rv_off + 1 * rv_ld + CO] - rv[rv_off + 2 * rv_ld:rv_off + 2 * rv_ld + CO]).double()
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(rne_bf16(y), ref, mg)


def test_rejects_truncation_instead_of_rne():
    *_, ref, mg = _problem()
    with pytest.raises(AssertionError, match="outside the bound"):
        _ok(trunc_bf16(ref), ref, mg)


def test_rejects_write_one_past_the_end():
    *_, ref, mg = _problem()
    b = Buf(ref.shape, torch.bfloat16, "cpu", rne_bf16(ref))
    assert b.guards_intact()
    b.raw[b.g + b.n] = 0.0          # the element after the last one
    assert not b.guards_intact()
    assert b.first_bad_guard() == (None, b.n)


def test_rejects_nan_left_in_overwrite_destination():
    *_, ref, mg = _problem()
    b = Buf(ref.shape, torch.bfloat16, "cpu")        # NaN-prefilled
    b.t.copy_(rne_bf16(ref))
    b.t[37, 5] = float("nan")                          # one element the kernel did not write
    with pytest.raises(AssertionError, match="non-finite"):
        _ok(b.t, ref, mg)


def test_rejects_ignored_acc1():
    """Data gradient into split destinations, acc0 = 0, acc1 = 1: D1 written as if acc1 were 0."""
    g = torch.Generator().manual_seed(6)
    C0, C1 = 32, 32
    dy = torch.randn(N, H, H, CO, generator=g).to(torch.bfloat16)
    w = (torch.randn(TAPS, CO, C0 + C1, generator=g) / (TAPS * CO) ** 0.5).to(torch.bfloat16)
    prior1 = torch.randn(N * H * H, C1, generator=g).to(torch.bfloat16)
    a, m = conv_dgrad_ref(dy, w, H, H, C0 + C1, 3, 3, 1, PADS)
    ref1, mg1 = epilogue_ref(a[..., C0:].reshape(-1, C1), m[..., C0:].reshape(-1, C1), prior=prior1)
    check("d1", rne_bf16(ref1), ref1, mg1, TAPS * CO, "bf16")
    no_acc, _ = epilogue_ref(a[..., C0:].reshape(-1, C1), m[..., C0:].reshape(-1, C1))
    with pytest.raises(AssertionError, match="outside the bound"):
        check("d1", rne_bf16(no_acc), ref1, mg1, TAPS * CO, "bf16")


# ------------------------------------------------------------------ attention
NEG_BIG = -1.0e30


def _emul_fwd(qkv, scale, fault=None):
    """attn_fwd_kernel's arithmetic in torch: fp32 scores per 64-key tile (rows past L repeat row L - 1 and are masked), online
    softmax, P rounded to bf16, fp32 second product, bf16 store.  -> (o bf16, lse fp32).  `fault` plants one defect."""
    N, L, C3 = qkv.shape
    C = C3 // 3
    x = qkv.float()
    q, k, v = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    m = torch.full((N, L), NEG_BIG)
    lsum = torch.zeros(N, L)
    O = torch.zeros(N, L, C)
    for k0 in range(0, L, 64):
        if fault == "dropped_tile" and k0 == 64:
            continue
        idx = torch.arange(k0, k0 + 64)
        valid = idx < L
        idx = idx.clamp(max=L - 1)
        s = (q @ k[:, idx].transpose(1, 2)) * scale
        if fault != "unmasked":
            s[..., ~valid] = NEG_BIG
        m_new = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new[..., None])
        lsum = lsum * alpha + p.sum(-1)
        if not (fault == "no_rescale" and k0 > 0):
            O = O * alpha[..., None]
        O = O + p.to(torch.bfloat16).float() @ v[:, idx]
        m = m_new
    inv = 1.0 / lsum
    if fault == "no_inv_rows48":
        inv = torch.where(torch.arange(L) % 64 >= 48, torch.ones(()), inv)
    o = O * inv[..., None]
    return (trunc_bf16(o.double()) if fault == "trunc_store" else o.to(torch.bfloat16)), m + torch.log(lsum)


def _emul_bwd(qkv, o, do, lse, scale, fault=None):
    """attn_bwd_kernel's arithmetic: fp32 scores, P from the given lse, delta from the given o, P and dS rounded to bf16 before
    the fp32 second products, bf16 stores.  -> (dq, dk, dv bf16, delta fp32)"""
    N, L, C3 = qkv.shape
    C = C3 // 3
    x = qkv.float()
    q, k, v = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    g, lse = do.float(), lse.float()
    delta = (g * o.float()).sum(-1)
    d_used = delta.roll(1, -1) if fault == "delta_of_neighbouring_query" else delta
    if fault == "lse_of_neighbouring_image":
        lse = lse.roll(1, 0)
    P = torch.exp((q @ k.transpose(1, 2)) * scale - lse[..., None])
    dS = P * (g @ v.transpose(1, 2) - d_used[..., None]) * scale
    Pb, dSb = P.to(torch.bfloat16).float(), dS.to(torch.bfloat16).float()
    dq = dSb @ k
    if fault == "dropped_query_tile":
        Pb[:, L - 64:], dSb[:, L - 64:] = 0, 0
    dk, dv = dSb.transpose(1, 2) @ q, Pb.transpose(1, 2) @ g
    return dq.to(torch.bfloat16), dk.to(torch.bfloat16), dv.to(torch.bfloat16), delta


_ATTN = {}


def _attn_problem(L, C, kind):
    """(qkv, dO, scale, refs) -- computed once per shape and draw, shared and left unchanged"""
    if (L, C, kind) not in _ATTN:
        qkv, do = attn_draw(2, L, C, kind, seed=L + C)
        scale = 1.0 / math.sqrt(C)
        _ATTN[L, C, kind] = (qkv, do, scale, attn_fused_refs(qkv, do, scale))
    return _ATTN[L, C, kind]


def _emulate(L, C, kind, fwd_fault=None, bwd_fault=None):
    qkv, do, scale, R = _attn_problem(L, C, kind)
    o, lse = _emul_fwd(qkv, scale, fwd_fault)
    dq, dk, dv, delta = _emul_bwd(qkv, R["o_in"], do, R["lse_in"], scale, bwd_fault)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, delta=delta), R


def _failing_rows(y, R, name):
    """fraction-of-rows helper: boolean [N][L], True where any element of the row is outside the bound"""
    over = violations(y, *R[name])
    return over if over.dim() == 2 else over.any(-1)


@pytest.mark.parametrize("kind", ["flat", "peaked"])
@pytest.mark.parametrize("L,C", [(48, 64), (256, 128)])
def test_attention_bounds_accept_the_emulated_kernel(L, C, kind):
    got, R = _emulate(L, C, kind)
    for name, y in got.items():
        ratio, rel = check_bound(name, y, *R[name])
        assert ratio <= 1.0
        if name in R["emu"]:
            ref = R[name][0]
            bar = REL_L2_MARGIN * float((R["emu"][name] - ref).norm() / ref.norm())
            assert rel <= bar, (name, rel, bar)
            check_bound(name + " (storage precision only)", R["emu"][name], *R[name])


def test_attention_rejects_unmasked_partial_key_tile():
    """L = 48: keys 48..63 of the tile counted as copies of key 47"""
    got, R = _emulate(48, 64, "flat", fwd_fault="unmasked")
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound("o", got["o"], *R["o"])
    assert _failing_rows(got["o"], R, "o").float().mean() >= 0.5


def test_attention_rejects_dropped_key_tile():
    got, R = _emulate(256, 128, "flat", fwd_fault="dropped_tile")
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound("o", got["o"], *R["o"])
    assert _failing_rows(got["o"], R, "o").float().mean() >= 0.5
    assert _failing_rows(got["lse"], R, "lse").float().mean() >= 0.5


def test_attention_rejects_accumulator_not_rescaled():
    """The running max rises in a later tile (peaked draw: keys L / 2 and L - 3 of image 0) and O is not multiplied by alpha.
    Affected: the rows whose tile maximum rises after tile 0 by enough to matter (alpha < 0.9)."""
    got, R = _emulate(256, 128, "peaked", fwd_fault="no_rescale")
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound("o", got["o"], *R["o"])
    qkv, _, scale, _ = _attn_problem(256, 128, "peaked")
    x = qkv.double()
    tmax = ((x[..., :128] @ x[..., 128:256].transpose(1, 2)) * scale).reshape(2, 256, 4, 64).max(-1).values
    run = tmax.cummax(-1).values
    affected = ((run[..., 1:] - run[..., :-1]) > -math.log(0.9)).any(-1)
    assert int(affected[0].sum()) >= 64, "the peaked draw does not make the running max rise"
    assert _failing_rows(got["o"], R, "o")[affected].float().mean() >= 0.5


def test_attention_rejects_missing_normalisation_on_last_rows_of_a_tile():
    """1 / lsum missing on rows >= 48 of each 64-row query tile"""
    got, R = _emulate(256, 128, "flat", fwd_fault="no_inv_rows48")
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound("o", got["o"], *R["o"])
    rows = torch.arange(256) % 64 >= 48
    bad = _failing_rows(got["o"], R, "o")
    assert bad[:, rows].float().mean() >= 0.5 and not bool(bad[:, ~rows].any())


@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_attention_rejects_lse_of_neighbouring_image(kind):
    """Every P of the image is scaled by exp(lse_i - lse'_i).  On the flat draw the two images' log-sum-exps differ by 0.09 in the
    median: every dv row leaves its bound (a P-weighted sum of dO, no cancellation), while dq and dk -- whose bound carries
    |dP| + |delta| without their cancellation -- are rejected on a quarter of their rows; on the peaked draw (the images differ
    by 0.9) on nearly all of them."""
    got, R = _emulate(256, 128, kind, bwd_fault="lse_of_neighbouring_image")
    for name in ("dq", "dk", "dv"):
        with pytest.raises(AssertionError, match="outside the bound"):
            check_bound(name, got[name], *R[name])
    assert _failing_rows(got["dv"], R, "dv").float().mean() >= 0.5
    if kind == "peaked":
        assert _failing_rows(got["dq"], R, "dq").float().mean() >= 0.5
        assert _failing_rows(got["dk"], R, "dk").float().mean() >= 0.5


def test_attention_rejects_delta_of_neighbouring_query():
    got, R = _emulate(256, 128, "flat", bwd_fault="delta_of_neighbouring_query")
    for name in ("dq", "dk"):
        with pytest.raises(AssertionError, match="outside the bound"):
            check_bound(name, got[name], *R[name])
    assert _failing_rows(got["dq"], R, "dq").float().mean() >= 0.5
    check_bound("dv", got["dv"], *R["dv"])          # dv does not read delta


def test_attention_rejects_dropped_query_tile_in_dk_dv():
    got, R = _emulate(256, 128, "flat", bwd_fault="dropped_query_tile")
    for name in ("dk", "dv"):
        with pytest.raises(AssertionError, match="outside the bound"):
            check_bound(name, got[name], *R[name])
        assert _failing_rows(got[name], R, name).float().mean() >= 0.5
    check_bound("dq", got["dq"], *R["dq"])


def test_attention_rel_l2_bar_rejects_truncated_store():
    """Truncating the bf16 store instead of rounding it stays inside the per-element bound's order of magnitude; the rel-L2 bar
    against the storage-precision emulation is what catches it."""
    got, R = _emulate(256, 128, "flat", fwd_fault="trunc_store")
    ref = R["o"][0]
    rel = float((got["o"].double() - ref).norm() / ref.norm())
    emu = float((R["emu"]["o"] - ref).norm() / ref.norm())
    assert rel > REL_L2_MARGIN * emu, (rel, emu)
    ok, _ = _emulate(256, 128, "flat")
    assert float((ok["o"].double() - ref).norm() / ref.norm()) <= REL_L2_MARGIN * emu
