"""A derived error bound for the eight outputs of mdm_metric_image against the fp64 statement of tests/_metric_ref.py -- derived from
the arithmetic include/mdm_metric.h specifies, never fitted to what a GPU returned (the discipline of tests/_bounds.py).

u = 2^-24 (one fp32 rounding), gamma(k) = k u / (1 - k u) (k roundings compounded).

The windowed moments.  The kernel holds d = fl(p - c_p), e = fl(t - c_t) about the tile's pivots and forms five fp32 moments of them,
along W then along H, each pass a chain of 11 fused multiply-adds with the float window.  A term of a first moment carries: the
rounding of d (1), the two float weights against the double window of the reference (2), at most 11 roundings of the first chain
and 11 of the second (22): K1 = 25.  A term of a second moment carries the roundings of both factors (2), of their product (1), the
weights (2) and the chains (22): K2 = 27.  With W2 the double window, about the SAME pivots,
    M1 = sum W2 (p - c),  A1 = sum W2 |p - c|,  M2 = sum W2 (p - c)^2,  A11 = sum W2 |p - c_p| |t - c_t|,
a correct kernel's fp32 moments satisfy
    |m - M1| <= em = gamma(K1) A1,     |s - M2| <= es = gamma(K2) M2,     |s_de - M11| <= es_de = gamma(K2) A11.
A pivot moves no variance and no covariance, and mu = c + M1 exactly, so in terms of the reference's mu, var, cov:
    e(mu)  = em                                         (the pivot is added back in double)
    e(var) = es + 2 |M1| em + em^2                      (var = s - m^2, in double)
    e(cov) = es_de + |M1_p| em_t + |M1_t| em_p + em_p em_t
The factors.  N1 = 2 mu_p mu_t + C1, D1 = mu_p^2 + mu_t^2 + C1, N2 = 2 cov + C2, D2 = var_p + var_t + C2:
    eN1 = 2 (|mu_p| em_t + |mu_t| em_p + em_p em_t),   eD1 = 2 |mu_p| em_p + em_p^2 + 2 |mu_t| em_t + em_t^2,
    eN2 = 2 e(cov),                                     eD2 = e(var_p) + e(var_t).
D1 >= C1 and D2 >= C2 in exact arithmetic; the computed denominators are at least D - eD, which must stay positive (it does while
the moment errors are below C1, C2 -- otherwise the bound is infinite and says so).  For a ratio A = N / D:
    |A^ - A| = |dN - A dD| / D^  <=  eA = (eN + |A| eD) / (D - eD),
and for the product S = A B:  |S^ - S| <= |A| eB + |B| eA + eA eB.  The expression itself is evaluated in double from the fp32 moments:
some 16 roundings of 2^-53, amplified at most by the cancellations var = s - m^2 against C2 and mu^2 against C1:
    e_dbl = 32 2^-53 (1 + |S|) (1 + (M2_p + M2_t + M1_p^2 + M1_t^2) / C2 + (mu_p^2 + mu_t^2) / C1).
The means.  A sum of n doubles in any order is off by at most n 2^-53 sum |.|; the quotient is rounded once to float:
    e(ssim) = mean(e_map) + n 2^-53 mean |S| + u |ssim|,        the same over the hole-centred positions for ssim_hole.
mse.  (p - t)^2 is fl(fl(p - t)^2): three roundings, gamma(3) relative, plus 2^-149 where the square is denormal; then the double sum
and one rounding:  e(mse) = (gamma(3) + n 2^-53) mse + 2^-149 + u mse.
psnr = 10 log10(L^2 / mse): the relative error rho = gamma(3) + n 2^-53 + 2^-149 / mse of the double mse moves it by at most
-10 log10(1 - rho); the double log10 and the division are good to a few 2^-53 of |psnr|; one rounding to float:
    e(psnr) = -10 log10(1 - rho) + (u + 8 2^-53) |psnr|.        mse = 0 gives +inf on both sides, exactly.
The two counts are integers below 2^24 in every test: exact.

A CPU emulation of this arithmetic (tests/test_metric_cpu.py) stays inside these bounds on every input class, and each planted
fault there leaves them on at least one."""
import math

import torch

import _metric_ref as MR

U = 2.0 ** -24
K1, K2 = 25, 27


def gamma(k):
    return k * U / (1 - k * U)


def pivots(x64, tile_h, tile_w):
    """[R, C, H - 10, W - 10]: the pivot of each map position's tile as the header states it -- the element at row
    min(y0 + 5 + tile_h / 2, H - 1), column min(x0 + 5 + tile_w / 2, W - 1), or 0 where it is not finite."""
    R, C, H, W = x64.shape
    ys, xs = torch.arange(H - MR.K + 1), torch.arange(W - MR.K + 1)
    yc = ((ys // tile_h) * tile_h + 5 + tile_h // 2).clamp_max(H - 1)
    xc = ((xs // tile_w) * tile_w + 5 + tile_w // 2).clamp_max(W - 1)
    c = x64[:, :, yc][:, :, :, xc]
    return torch.where(torch.isfinite(c), c, torch.zeros_like(c))


def _windows(x64):
    return x64.unfold(2, MR.K, 1).unfold(3, MR.K, 1)                         # [R, C, MH, MW, 11, 11], a view


def map_bound(ref, tile_h, tile_w):
    """the bound of every map position [R, C, MH, MW] (module docstring); +inf where a denominator's error reaches the denominator"""
    w = MR.window64()
    w2 = torch.outer(w, w)
    p, t, C1, C2 = ref["p"], ref["t"], ref["C1"], ref["C2"]
    d = _windows(p) - pivots(p, tile_h, tile_w)[..., None, None]
    e = _windows(t) - pivots(t, tile_h, tile_w)[..., None, None]
    s = lambda a: (a * w2).sum((-1, -2))
    M1p, M1t, A1p, A1t = s(d), s(e), s(d.abs()), s(e.abs())
    M2p, M2t, A11 = s(d * d), s(e * e), s((d * e).abs())
    del d, e
    g1, g2 = gamma(K1), gamma(K2)
    em_p, em_t = g1 * A1p, g1 * A1t
    ev_p = g2 * M2p + 2 * M1p.abs() * em_p + em_p * em_p
    ev_t = g2 * M2t + 2 * M1t.abs() * em_t + em_t * em_t
    ec = g2 * A11 + M1p.abs() * em_t + M1t.abs() * em_p + em_p * em_t
    mu_p, mu_t = ref["mu_p"], ref["mu_t"]
    N1, D1 = 2 * mu_p * mu_t + C1, mu_p * mu_p + mu_t * mu_t + C1
    N2, D2 = 2 * ref["cov"] + C2, ref["var_p"] + ref["var_t"] + C2
    eN1 = 2 * (mu_p.abs() * em_t + mu_t.abs() * em_p + em_p * em_t)
    eD1 = 2 * mu_p.abs() * em_p + em_p * em_p + 2 * mu_t.abs() * em_t + em_t * em_t
    eN2, eD2 = 2 * ec, ev_p + ev_t
    A, B = N1 / D1, N2 / D2
    inf = torch.full_like(A, math.inf)
    eA = torch.where(D1 - eD1 > 0, (eN1 + A.abs() * eD1) / (D1 - eD1), inf)
    eB = torch.where(D2 - eD2 > 0, (eN2 + B.abs() * eD2) / (D2 - eD2), inf)
    S = A * B
    e_dbl = 32 * 2.0 ** -53 * (1 + S.abs()) * (1 + (M2p + M2t + M1p * M1p + M1t * M1t) / C2 + (mu_p * mu_p + mu_t * mu_t) / C1)
    return A.abs() * eB + B.abs() * eA + eA * eB + e_dbl


def _mse_bounds(mse, n, L):
    """(e(mse), e(psnr)) of a mean of n squares (module docstring); mse a 0-dim double tensor"""
    g3 = gamma(3)
    e_mse = (g3 + n * 2.0 ** -53 + U) * mse + 2.0 ** -149
    if not bool(mse > 0):
        return e_mse, torch.zeros_like(mse)
    rho = g3 + n * 2.0 ** -53 + 2.0 ** -149 / mse
    psnr = 10 * torch.log10(L * L / mse)
    return e_mse, -10 * torch.log10(1 - rho) + (U + 8 * 2.0 ** -53) * psnr.abs()


def out_bound(ref, tile_h, tile_w):
    """[R, 8] fp64: the bound of every slot of every row; 0 for the counts and wherever the reference is NaN or infinite (such a slot
    is compared exactly by `check`)."""
    eb = map_bound(ref, tile_h, tile_w)
    out, smap, hole_c, L = ref["out"], ref["map"], ref["hole_c"], ref["L"]
    R = out.shape[0]
    bound = torch.zeros(R, 8, dtype=torch.float64)
    n_el = ref["p"][0].numel()
    for r in range(R):
        bound[r, 0], bound[r, 1] = _mse_bounds(out[r, 0], n_el, L)
        n = smap[r].numel()
        bound[r, 2] = eb[r].mean() + n * 2.0 ** -53 * smap[r].abs().mean() + U * out[r, 2].abs()
        nh, nhc = int(out[r, 6]), int(out[r, 7])
        if nh:
            bound[r, 3], bound[r, 4] = _mse_bounds(out[r, 3], nh, L)
        if nhc:
            hc = hole_c[r]
            bound[r, 5] = eb[r][hc].mean() + nhc * 2.0 ** -53 * smap[r][hc].abs().mean() + U * out[r, 5].abs()
    return torch.where(torch.isfinite(out), bound, torch.zeros_like(bound))


def check(name, got, ref_out, bound):
    """`got` [R, 8] (any float dtype) against the reference and its bound: a NaN where and only where the reference has one, an
    infinity equal to the reference's, every other slot within its bound, the counts exact.  -> the largest error / bound over the
    slots with a positive bound."""
    g = got.detach().cpu().double()
    assert g.shape == ref_out.shape == bound.shape, (name, g.shape, ref_out.shape)
    nan, inf = torch.isnan(ref_out), torch.isinf(ref_out)
    assert torch.equal(torch.isnan(g), nan), (name, "NaN slots", torch.isnan(g).nonzero().tolist(), nan.nonzero().tolist())
    assert torch.equal(g[inf], ref_out[inf]), (name, "infinite slots", g[inf], ref_out[inf])
    fin = ~nan & ~inf
    err = torch.where(fin, (g - ref_out).abs(), torch.zeros_like(g))
    over = fin & ~(err <= bound)
    if bool(over.any()):
        ex = [(i, MR.SLOTS[i[1]], float(g[tuple(i)]), float(ref_out[tuple(i)]), float(bound[tuple(i)])) for i in over.nonzero()[:4].tolist()]
        raise AssertionError(f"{name}: {int(over.sum())} slots outside the bound, e.g. (index, slot, got, ref, bound) {ex}")
    assert torch.equal(g[:, 6:], ref_out[:, 6:]), (name, "counts")
    pos = fin & (bound > 0)
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
