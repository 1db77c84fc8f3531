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


# ------------------------------------------------------------------ GroupNorm
# An fp32 emulation of the kernels' arithmetic (csrc/gn_kernels.inc, the fused epilogues of csrc/gemm.hip) on the rows of
# tests/_gn_rows.py (the rows tests/test_gn_bounds_gpu.py runs): it must stay inside every bound of _bounds.gn_fwd_ref /
# gn_bwd_ref, and each fault planted into it must leave them on every row it is claimed for.  Sums run in numpy fp32, sequentially ("seq") or pairwise ("pair").
import numpy as np

import _gn_rows as GN
from _bounds import gn_bwd_ref, gn_draw, gn_fwd_ref, gn_stats_in, rel_l2_bar

F32 = torch.float32


def _np_sum(t, dim, order):
    a = t.contiguous().numpy()
    r = np.cumsum(a, axis=dim, dtype=np.float32).take(-1, axis=dim) if order == "seq" else a.sum(axis=dim, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(r))


def _sig32(z):
    return 1.0 / (1.0 + torch.exp(-z))


def _gn_store(t, dt, fault=None):
    if dt == "f32":
        return t
    return trunc_bf16(t.double()) if fault == "trunc_store" else t.to(torch.bfloat16)


def _pixel_mask(P, fault):
    """1 for the pixels that enter the sums: all but the last one / the first one of the last 64-pixel stretch (the first pixel of a
    tail loop; P / 2 on maps of one stretch: pixel 0 holds the pivots, and a pivot adds nothing to the shifted sums)"""
    m = torch.ones(P)
    if fault == "last_pixel":
        m[P - 1] = 0
    if fault == "tail_pixel":
        m[(P - 1) // 64 * 64 or P // 2] = 0
    return m


def _per_c(t, cpg):
    return t.repeat_interleave(cpg, 1)[:, None, :].clone()


def _flip_lanes(keep):
    """one kept lane dropped and one dropped lane kept"""
    k = keep.clone().reshape(-1)
    k[int(k.nonzero()[5])] = False
    k[int((~keep.reshape(-1)).nonzero()[5])] = True
    return k.reshape(keep.shape)


def _gn_emul_fwd(x, gamma, beta, G, eps, silu, dt, order="pair", scheme="pivot", keep=None, scale=1.0, fault=None):
    """gn_fwd_kernel / gn_fwd_reg_kernel ("pivot") or the fused forward epilogue ("two_pass") -> (y as stored, stats fp32)"""
    x, gamma, beta = x.float(), gamma.float(), beta.float()
    N, P, C = x.shape
    cpg = C // G
    xg = x.reshape(N, P, G, cpg)
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(cpg * P), dtype=F32)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(N, G, P * cpg)
    msk = _pixel_mask(P, fault)[None, :, None, None]
    if scheme == "pivot":
        K = xg[:, :1, :, :1].clone()
        if fault == "no_pivot":
            K = torch.zeros_like(K)
        d = (xg - K) * msk
        md = _np_sum(flat(d), 2, order) * inv
        var = (_np_sum(flat(d * d), 2, order) * inv - md * md).clamp_min(0)
        mean = K[:, 0, :, 0] + md
    else:
        mean = _np_sum(flat(xg * msk), 2, order) * inv
        c = (xg - mean[:, None, :, None]) * msk
        var = _np_sum(flat(c * c), 2, order) * inv
    rstd = torch.rsqrt(var + (0.0 if fault == "no_eps" else torch.tensor(eps, dtype=F32)))
    stats = torch.stack((mean, rstd), 2)
    m_e, r_e = _per_c(mean, cpg), _per_c(rstd.roll(1, 0) if fault == "rstd_neighbour_image" else rstd, cpg)
    if fault == "group_off_by_one":          # the first channel of a block takes the statistics of the group in front of it
        c0 = (G // 2) * cpg
        m_e[..., c0], r_e[..., c0] = mean[:, G // 2 - 1, None], rstd[:, G // 2 - 1, None]
    z = (x - m_e) * (r_e * gamma) + beta if scheme == "pivot" else ((x - m_e) * r_e) * gamma + beta
    if silu:
        z = z * _sig32(z)
    if keep is not None:
        kp = _flip_lanes(keep) if fault == "flip_lane" else keep
        z = torch.where(kp, z * torch.tensor(scale, dtype=F32), torch.zeros(()))
    return _gn_store(z, dt, fault), stats


def _gn_emul_bwd(x, dy, stats, gamma, beta, G, silu, dt, kernel, adds=(), prior=None, order="pair", keep=None, scale=1.0, fault=None):
    """gn_bwd_kernel ("stream") or gn_bwd_reg_kernel ("reg": xh and z as one fma from per-channel constants, the group sums as
    gamma-weighted sums of the column sums, k1 = fma(q2, -mean rstd, q1)) -> dict of outputs"""
    x, dy, gamma, beta = x.float(), dy.float(), gamma.float(), beta.float()
    N, P, C = x.shape
    cpg = C // G
    mean, rstd = stats[..., 0], stats[..., 1]
    if fault == "rstd_neighbour_image":
        rstd = rstd.roll(1, 0)
    m, r = _per_c(mean, cpg), _per_c(rstd, cpg)
    if keep is not None:
        kp = _flip_lanes(keep) if fault == "flip_lane" else keep
        dy = torch.where(kp, dy * torch.tensor(scale, dtype=F32), torch.zeros(()))
    if kernel == "stream":
        xh = (x - m) * r
        zz = xh * gamma + beta
    else:
        nmr, za = -m * r, r * gamma
        zb = nmr * gamma + beta
        xh, zz = x * r + nmr, x * za + zb
    gz = dy
    if silu and fault != "no_silu_grad":
        s = _sig32(zz)
        gz = dy * (s * (1.0 + zz * (1.0 - s)))
    msk = _pixel_mask(P, fault)[None, :, None]
    dg_img, db_img = _np_sum(gz * xh * msk, 1, order), _np_sum(gz * msk, 1, order)          # [N][C]
    gsum = lambda t: _np_sum(t.reshape(N, P, G, cpg).permute(0, 2, 1, 3).reshape(N, G, P * cpg), 2, order)
    if kernel == "stream":
        gg = gz * gamma
        a1, a2 = gsum(gg * msk), gsum(gg * xh * msk)
    else:
        a1, a2 = _np_sum((db_img * gamma).reshape(N, G, cpg), 2, order), _np_sum((dg_img * gamma).reshape(N, G, cpg), 2, order)
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(cpg * P), dtype=F32)
    A1, A2 = _per_c(a1, cpg), _per_c(a2, cpg)
    if kernel == "stream":
        k1, k2 = r * A1 * inv, r * A2 * inv
        o = (r * gamma) * gz - (xh * k2 + k1)
    else:
        q1, q2 = r * A1 * inv, r * A2 * inv
        k1, k2 = q2 * nmr + q1, q2 * r
        o = za * gz - (x * k2 + k1)
    dx = o
    adds = [a.float() for a in adds]
    use = adds[:-1] if fault == "drop_add0b" else ([adds[0]] + adds if fault == "add0_twice" else adds)
    for a in use:
        o = o + a
    sum_img = _np_sum(o if fault == "sum_img_after_adds" else dx, 1, order)
    if fault == "sum_img_neighbour":
        sum_img = sum_img.roll(1, 0)
    pr = lambda k: prior[k].float() if prior and prior.get(k) is not None else 0.0
    dgam = _np_sum(_np_sum(gz * x * msk, 1, order), 0, order) if fault == "dgamma_x" else _np_sum(dg_img, 0, order)
    return dict(dx=_gn_store(o, dt, fault), dgamma=pr("dgamma") + dgam, dbeta=pr("dbeta") + _np_sum(db_img, 0, order),
                sum_img=sum_img, sum_all=pr("sum_all") + _np_sum(sum_img, 0, order))


_GN = {}


def _gn_fwd_problem(row):
    if row not in _GN:
        _GN[row] = GN.fwd_problem(row)
    return _GN[row]


def _gn_bwd_problem(row):
    if row not in _GN:
        _GN[row] = GN.bwd_problem(row)
    return _GN[row]


def _gn_fwd_emulate(row, order="pair", fault=None):
    route, dt, drop, (C0, C1, P, G), N, draw, silu = row
    x, gamma, beta, R = _gn_fwd_problem(row)
    keep, scale = GN.row_keep(row)
    y, stats = _gn_emul_fwd(x, gamma, beta, G, GN.EPS, silu, dt, order, "pivot", keep, scale, fault)
    return dict(y=y, stats=stats), R


def _gn_bwd_emulate(row, kernel, order="pair", fault=None):
    route, dt, drop, (C0, C1, P, G), N, draw, silu, form = row
    x, dy, stats, gamma, beta, adds, pri, R = _gn_bwd_problem(row)
    keep, scale = GN.row_keep(row)
    got = _gn_emul_bwd(x, dy, stats, gamma, beta, G, silu, dt, kernel, list(adds.values()), pri if form == "sums" else dict(pri, sum_all=None),
                       order, keep, scale, fault)
    return got, R


def _gn_margin(got, R, names):
    """largest err / bound over the named outputs (inf for a non-finite element)"""
    worst = 0.0
    for name in names:
        ref, bound = R[name]
        err = (got[name].double() - ref).abs()
        ratio = torch.where(torch.isfinite(err), err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
        ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(ratio), ratio)
        worst = max(worst, float(ratio.max()))
    return worst


BWD_OUT = ("dx", "dgamma", "dbeta", "sum_img", "sum_all")


@pytest.mark.parametrize("row", GN.FWD_ROWS, ids=[GN.row_id(r) for r in GN.FWD_ROWS])
def test_groupnorm_forward_bounds_accept_the_emulated_kernel(row):
    for order in ("pair", "seq"):
        got, R = _gn_fwd_emulate(row, order)
        for name in ("y", "stats"):
            ratio, rel = check_bound(f"{name} {order}", got[name], *R[name])
            assert ratio <= 1.0
            if name == "y" and row[1] == "bf16":
                assert rel <= rel_l2_bar(R["y"][0]), (rel, rel_l2_bar(R["y"][0]))


@pytest.mark.parametrize("row", GN.BWD_ROWS, ids=[GN.row_id(r) for r in GN.BWD_ROWS])
def test_groupnorm_backward_bounds_accept_both_emulated_kernels(row):
    for kernel, order in (("stream", "pair"), ("stream", "seq"), ("reg", "pair"), ("reg", "seq")):
        got, R = _gn_bwd_emulate(row, kernel, order)
        for name in BWD_OUT:
            ratio, rel = check_bound(f"{name} {kernel} {order}", got[name], *R[name])
            assert ratio <= 1.0
            if name == "dx" and row[1] == "bf16":
                assert rel <= rel_l2_bar(R["dx"][0]), (rel, rel_l2_bar(R["dx"][0]))


def _gn_n(row):
    C0, C1, P, G = row[3]
    return (C0 + C1) // G * P


# fault -> the rows it is claimed for.  A pixel missing from a sum moves it by that pixel's share: on a spike that is 40 times the
# typical term, on a plain pixel about 1 / n of the sum, which the summation bound (n + 8) 2^-23 overtakes near n = 4096 -- so a plain
# pixel is claimed up to n = 2048.  The backward's bounds are loose on the offset draw (e_xh carries |x| + |mean| = 2000 against a
# spread of 0.01): only the fault that reads x itself is claimed there.
_loose = lambda r: r[5] == "offset" and len(r) == 8
GN_FWD_FAULTS = {
    "last_pixel": lambda r: r[5] == "spiked" or _gn_n(r) <= 2048,
    "tail_pixel": lambda r: _gn_n(r) <= 2048,
    "no_pivot": lambda r: r[5] == "offset",
    "group_off_by_one": lambda r: True,
    "no_eps": lambda r: r[5] == "constant",
    "rstd_neighbour_image": lambda r: True,
    "flip_lane": lambda r: r[2] == 1,
}
GN_BWD_FAULTS = {
    "last_pixel": lambda r: (r[5] == "spiked" or _gn_n(r) <= 2048) and not _loose(r),
    "tail_pixel": lambda r: _gn_n(r) <= 2048 and not _loose(r),
    "no_silu_grad": lambda r: r[6] == 1 and not _loose(r),
    "rstd_neighbour_image": lambda r: not _loose(r),
    "dgamma_x": lambda r: True,
    "drop_add0b": lambda r: r[7] == "add2",
    "add0_twice": lambda r: r[7] in ("acc", "add2", "sums"),
    "sum_img_after_adds": lambda r: r[7] == "sums",
    "sum_img_neighbour": lambda r: r[7] == "sums",
    "flip_lane": lambda r: r[2] == 1,
}
_FWD_CLAIMS = [(f, r) for f, rule in GN_FWD_FAULTS.items() for r in GN.FWD_ROWS if rule(r)]
_BWD_CLAIMS = [(f, r) for f, rule in GN_BWD_FAULTS.items() for r in GN.BWD_ROWS if rule(r)]


@pytest.mark.parametrize("fault,row", _FWD_CLAIMS, ids=[f"{f}-{GN.row_id(r)}" for f, r in _FWD_CLAIMS])
def test_groupnorm_forward_rejects_planted_fault(fault, row):
    got, R = _gn_fwd_emulate(row, fault=fault)
    margin = _gn_margin(got, R, ("y", "stats"))
    print(f"{fault} on {GN.row_id(row)}: {margin:.3g} x the bound")
    assert margin > 1.0
    with pytest.raises(AssertionError, match="outside the bound|non-finite"):
        for name in ("y", "stats"):
            check_bound(name, got[name], *R[name])


@pytest.mark.parametrize("fault,row", _BWD_CLAIMS, ids=[f"{f}-{GN.row_id(r)}" for f, r in _BWD_CLAIMS])
def test_groupnorm_backward_rejects_planted_fault(fault, row):
    """in the arithmetic of the kernel the row runs on; held against the outputs the GPU row checks"""
    got, R = _gn_bwd_emulate(row, "reg" if "reg" in row[0] else "stream", fault=fault)
    names = ("sum_img", "sum_all") if fault.startswith("sum_img") else ("dx", "dgamma", "dbeta") + (("sum_img", "sum_all") if row[7] == "sums" else ())
    margin = _gn_margin(got, R, names)
    print(f"{fault} on {GN.row_id(row)}: {margin:.3g} x the bound")
    assert margin > 1.0


def test_groupnorm_every_fault_is_claimed_somewhere():
    assert {f for f, _ in _FWD_CLAIMS} == set(GN_FWD_FAULTS) and {f for f, _ in _BWD_CLAIMS} == set(GN_BWD_FAULTS)


_BF16_FWD = [r for r in GN.FWD_ROWS if r[1] == "bf16"]
_BF16_BWD = [r for r in GN.BWD_ROWS if r[1] == "bf16"]


@pytest.mark.parametrize("row", _BF16_FWD + _BF16_BWD, ids=[GN.row_id(r) for r in _BF16_FWD + _BF16_BWD])
def test_groupnorm_rel_l2_bar_rejects_truncated_store(row):
    """truncation instead of round-to-nearest-even at the bf16 store stays inside twice the per-element bound; the rel-L2 bar of the
    storage precision is what rejects it, on every bf16 row"""
    if len(row) == 7:
        (got, R), name = _gn_fwd_emulate(row, fault="trunc_store"), "y"
    else:
        (got, R), name = _gn_bwd_emulate(row, "reg" if "reg" in row[0] else "stream", fault="trunc_store"), "dx"
    ref = R[name][0]
    rel, bar = float((got[name].double() - ref).norm() / ref.norm()), rel_l2_bar(ref)
    print(f"trunc_store on {GN.row_id(row)}: rel-L2 {rel:.3e} = {rel / bar:.2f} x the bar")
    assert rel > bar


# the fused forward epilogues: statistics in two passes over the bf16-rounded y.  (N, P, C, G) of the maps they run on
TWO_PASS = sorted({(r[2], r[1] * r[1], r[4], GN.FUSED_G) for r in GN.GNF_ROWS})
FUSED_BWD = sorted({(r[2], r[1] * r[1], r[3], GN.FUSED_G) for r in GN.GNB_ROWS})


@pytest.mark.parametrize("N,P,C,G", FUSED_BWD)
def test_groupnorm_fused_backward_shapes_accept_the_emulation(N, P, C, G):
    """the fused backward epilogues compute as gn_bwd_kernel does, on an fp32 dz, with up to two addends and a bf16 store"""
    x, dz = gn_draw(N, P, C, "plain", 3 * P + C, "bwd", G, "f32")
    x = x.bfloat16().float()
    g = torch.Generator().manual_seed(C + P)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    adds = [torch.randn(N, P, C, generator=g).bfloat16().float(), (0.5 * torch.randn(N, P, C, generator=g)).bfloat16().float()]
    stats = gn_stats_in(x, G, 1e-6)
    R = gn_bwd_ref(x, dz, stats[..., 0], stats[..., 1], gamma, beta, G, True, "bf16", adds)
    for order in ("pair", "seq"):
        got = _gn_emul_bwd(x, dz, stats, gamma, beta, G, True, "bf16", "stream", adds, None, order)
        for name in BWD_OUT:
            assert check_bound(name, got[name], *R[name])[0] <= 1.0
    for fault in ("last_pixel", "drop_add0b", "add0_twice", "sum_img_after_adds"):
        got = _gn_emul_bwd(x, dz, stats, gamma, beta, G, True, "bf16", "stream", adds, None, "pair", fault=fault)
        margin = _gn_margin(got, R, ("sum_img",) if fault.startswith("sum_img") else ("dx", "dgamma", "dbeta"))
        print(f"fused backward {fault} {N}x{P}x{C}: {margin:.3g} x the bound")
        assert margin > 1.0


@pytest.mark.parametrize("N,P,C,G", TWO_PASS)
@pytest.mark.parametrize("draw", ["plain", "spiked", "constant"])
def test_groupnorm_two_pass_bounds_accept_the_emulation_and_reject_a_missing_pixel(N, P, C, G, draw):
    x, _ = gn_draw(N, P, C, draw, 5 * P + C, "fwd", G, "bf16")
    g = torch.Generator().manual_seed(C)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    R = gn_fwd_ref(x, gamma, beta, G, 1e-6, True, "bf16", "two_pass")
    for order in ("pair", "seq"):
        y, stats = _gn_emul_fwd(x, gamma, beta, G, 1e-6, True, "bf16", order, "two_pass")
        assert check_bound("y", y, *R["y"])[0] <= 1.0 and check_bound("stats", stats, *R["stats"])[0] <= 1.0
    for fault in ("last_pixel", "rstd_neighbour_image") + (("no_eps",) if draw == "constant" else ()):
        y, stats = _gn_emul_fwd(x, gamma, beta, G, 1e-6, True, "bf16", "pair", "two_pass", fault=fault)
        margin = _gn_margin(dict(y=y, stats=stats), R, ("y", "stats"))
        print(f"two_pass {fault} {N}x{P}x{C}g{G} {draw}: {margin:.3g} x the bound")
        assert margin > 1.0


# ------------------------------------------------------------------ the time-embedding path and the helper kernels
# An fp32 emulation of each kernel's arithmetic (tests/_temb_rows.py) stays inside the bounds of tests/_bounds.py on every row the
# GPU tests run, and every planted fault leaves them on every row that can show it.
import _temb_rows as TE  # noqa: E402
from _bounds import colsum_ref, silu_bwd_ref, silu_bwd_sum_ref, silu_ref, temb_ref  # noqa: E402


@pytest.mark.parametrize("row", TE.FWD_ROWS, ids=[TE.fwd_id(r) for r in TE.FWD_ROWS])
def test_skinny_forward_bounds_accept_the_emulated_kernel(row):
    T = TE.fwd_problem(row)
    ratios = TE.check_fwd(row, T, TE.emulate_fwd(row, T))
    print("emulation err / bound", TE.fwd_id(row), ratios)
    assert max(ratios.values()) <= 1.0


@pytest.mark.parametrize("row", TE.BWD_ROWS, ids=[TE.bwd_id(r) for r in TE.BWD_ROWS])
def test_skinny_backward_bounds_accept_the_emulated_kernel(row):
    T = TE.bwd_problem(row)
    ratios = TE.check_bwd(row, T, TE.emulate_bwd(row, T))
    print("emulation err / bound", TE.bwd_id(row), ratios)
    assert max(ratios.values()) <= 1.0


_TE_FWD_CLAIMS = [(f, r) for f, rule in TE.FWD_FAULTS.items() for r in TE.FWD_ROWS if rule(r)]
_TE_BWD_CLAIMS = [(f, r) for f, rule in TE.BWD_FAULTS.items() for r in TE.BWD_ROWS if rule(r)]


@pytest.mark.parametrize("fault,row", _TE_FWD_CLAIMS, ids=[f"{f}-{TE.fwd_id(r)}" for f, r in _TE_FWD_CLAIMS])
def test_skinny_forward_rejects_planted_fault(fault, row):
    T = TE.fwd_problem(row)
    with pytest.raises(AssertionError, match="outside the bound|non-finite"):
        TE.check_fwd(row, T, TE.emulate_fwd(row, T, fault))


@pytest.mark.parametrize("fault,row", _TE_BWD_CLAIMS, ids=[f"{f}-{TE.bwd_id(r)}" for f, r in _TE_BWD_CLAIMS])
def test_skinny_backward_rejects_planted_fault(fault, row):
    T = TE.bwd_problem(row)
    with pytest.raises(AssertionError, match="outside the bound|non-finite"):
        TE.check_bwd(row, T, TE.emulate_bwd(row, T, fault))


def test_skinny_every_fault_is_claimed_somewhere():
    assert {f for f, _ in _TE_FWD_CLAIMS} == set(TE.FWD_FAULTS) and {f for f, _ in _TE_BWD_CLAIMS} == set(TE.BWD_FAULTS)
    # the suspected launcher defect is claimed on the row that was added for it
    assert [r for f, r in _TE_FWD_CLAIMS if f == "upper_half_unwritten"] == [TE.FWD_ROWS[-1]]


@pytest.mark.parametrize("nslab,pre,n", TE.SUM_ROWS)
def test_silu_bwd_sum_bounds_accept_the_emulation_and_reject_its_faults(nslab, pre, n):
    g = torch.Generator().manual_seed(nslab + n)
    slabs, p = torch.randn(nslab, n, generator=g), (torch.randn(n, generator=g) * 2.5 if pre else None)
    ratio, _ = check_bound("sum", TE.emulate_sum(slabs, p), *silu_bwd_sum_ref(slabs, p))
    assert ratio <= 1.0
    for fault in (["last_slab_left_out"] if nslab > 1 else []) + (["no_silu_grad_on_split"] if pre else []):
        with pytest.raises(AssertionError, match="outside the bound"):
            check_bound(fault, TE.emulate_sum(slabs, p, fault), *silu_bwd_sum_ref(slabs, p))


@pytest.mark.parametrize("variant", TE.VARIANTS)
@pytest.mark.parametrize("dim", [4, 64, 128, 129])
def test_embedding_bound_accepts_fp32_numpy_and_rejects_its_faults(dim, variant):
    t = TE.timesteps(5, dim)
    ref, bound = temb_ref(t, dim, *variant)
    ratio, _ = check_bound("temb", TE.temb32(t, dim, *variant), ref, bound)
    print("emulation err / bound", dim, variant, ratio)
    assert ratio <= 1.0
    for fault in ("shift_swapped", "j_off_by_one", "sin_cos_swapped"):
        with pytest.raises(AssertionError, match="outside the bound"):
            check_bound(fault, TE.temb32(t, dim, *variant, fault=fault), ref, bound)
    if dim & 1:
        assert float(ref[:, -1].abs().max()) == 0.0 and float(bound[:, -1].max()) == 0.0
    # column j = 0 is held to the accuracy of sinf / cosf alone, at t up to 1000
    assert float(bound[:, 0].max()) == 2.0 ** -21 and float(t.max()) == 1000.0


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_silu_bounds_accept_fp32_and_reject_a_missing_factor(n):
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=g) * 40 - 20
    dy, prior = torch.randn(n, generator=g), torch.randn(n, generator=g)
    assert check_bound("silu", TE.silu32(x), *silu_ref(x))[0] <= 1.0
    gz = dy * TE.silu_grad32(x)
    assert check_bound("silu_bwd", gz, *silu_bwd_ref(x, dy))[0] <= 1.0
    assert check_bound("silu_bwd acc", prior + gz, *silu_bwd_ref(x, dy, prior))[0] <= 1.0
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound("ignored acc", gz, *silu_bwd_ref(x, dy, prior))
    with pytest.raises(AssertionError, match="outside the bound"):
        check_bound("sigmoid for silu'", dy / (1 + torch.exp(-x)), *silu_bwd_ref(x, dy))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", TE.COLSUM_CS)
def test_colsum_bounds_accept_the_emulation_and_reject_its_faults(dt, C):
    for P, N, per_img, acc_img, dbias in TE.colsum_rows(dt, C):
        d, pi, pb = TE.colsum_problem(dt, C, P, N)
        R = colsum_ref(d, pi if acc_img else None, pb)
        got = dict(zip(("per_img", "dbias"), TE.emulate_colsum(d, pi if acc_img else None, pb)))
        names = (["per_img"] if per_img else []) + (["dbias"] if dbias else [])
        for name in names:
            assert check_bound(f"colsum {name}", got[name], *R[name])[0] <= 1.0
        for fault in (["no_lane_31"] if P >= 32 else []) + (["store_not_accumulate"] if acc_img or dbias else []):
            bad = dict(zip(("per_img", "dbias"), TE.emulate_colsum(d, pi if acc_img else None, pb, fault)))
            with pytest.raises(AssertionError, match="outside the bound"):
                for name in names:
                    check_bound(f"{fault} {name}", bad[name], *R[name])


def test_add3_bit_test_rejects_a_truncating_bf16_store():
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(4096, generator=g).bfloat16(), torch.randn(4096, generator=g).bfloat16()
    want = (x.float() + y.float()).to(torch.bfloat16)
    bad = trunc_bf16((x.float() + y.float()).double())
    assert not torch.equal(want.view(torch.int16), bad.view(torch.int16))
