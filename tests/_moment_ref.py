"""What the moment tests share (include/mdm_moment.h): exact-grid rows and their int64 statement, the correctly rounded reference by
`math.fsum` with the header's bound, and a numpy emulation of the stated order (rows in order within a split, splits in index order,
then the carry) that can plant the faults the tests must catch.  Host code only."""
import math

import numpy as np

U = 2.0 ** -53
FAULTS = ("drop_tail", "double_boundary", "no_mirror", "carry_overwrite")


def gamma(k):
    return k * U / (1.0 - k * U)


def grid_ints(rng, R, d):
    """integers in [-128, 127]: times 2^-7 they are floats whose products are multiples of 2^-14 and whose sums over 10^5 rows stay
    far below 2^53 units -- every partial sum is representable, so every order gives the same bits"""
    return rng.integers(-128, 128, size=(R, d)).astype(np.int64)


def grid_rows(ints):
    return (ints.astype(np.float64) * 2.0 ** -7).astype(np.float32)


def grid_moments(ints):
    """the int64 statement: (sum [d], outer [d][d]) as doubles, exact"""
    return ints.sum(0).astype(np.float64) * 2.0 ** -7, (ints.T @ ints).astype(np.float64) * 2.0 ** -14


def fsum_moments(x):
    """x [R][d] (any float type, widened exactly) -> (sum, outer, abs_sum, abs_outer): the correctly rounded sums of the exact
    products by math.fsum (a product of two widened floats is exact in fp64) and the sums of their magnitudes"""
    x = np.asarray(x, np.float64)
    R, d = x.shape
    s = np.array([math.fsum(x[:, j]) for j in range(d)])
    sa = np.array([math.fsum(np.abs(x[:, j])) for j in range(d)])
    o, oa = np.zeros((d, d)), np.zeros((d, d))
    for i in range(d):
        p = x[:, i:i + 1] * x[:, i:]                                      # exact
        for j in range(i, d):
            o[i, j] = o[j, i] = math.fsum(p[:, j - i])
            oa[i, j] = oa[j, i] = math.fsum(np.abs(p[:, j - i]))
    return s, o, sa, oa


def bound(n, splits, calls, mag, ref):
    """gamma(n + s + c) sum |.| of the header, plus u |ref| (+ the smallest subnormal): fsum's own rounding of the reference"""
    return gamma(n + splits + calls) * mag + U * np.abs(ref) + 5e-324


def inside(got, ref, bnd):
    """elementwise |got - ref| <= bnd, a NaN or inf anywhere being outside"""
    with np.errstate(invalid="ignore"):
        return bool((np.abs(got - ref) <= bnd).all())


def emulate(x, rps, carry=None, fault=None):
    """The stated order in numpy fp64: within a split the rows one after the other onto +0 (the four products of one instruction in
    row order: one of the orders the hardware may take), the splits in index order, then the carry (sum, outer) with one rounding.
    `fault` plants one of FAULTS.  -> (sum, outer)"""
    x = np.asarray(x, np.float64)
    R, d = x.shape
    if fault == "drop_tail":
        x, R = x[:R - R % 4], R - R % 4
    tot_s, tot_o = None, None
    for k, r0 in enumerate(range(0, R, rps)):
        lo = r0 - 1 if fault == "double_boundary" and k > 0 else r0
        ps, po = np.zeros(d), np.zeros((d, d))
        for r in range(lo, min(R, r0 + rps)):
            ps = ps + x[r]
            po = po + np.outer(x[r], x[r])
        tot_s, tot_o = (ps, po) if tot_s is None else (tot_s + ps, tot_o + po)
    if tot_s is None:
        tot_s, tot_o = np.zeros(d), np.zeros((d, d))
    if carry is not None and fault != "carry_overwrite":
        tot_s, tot_o = carry[0] + tot_s, carry[1] + tot_o
    if fault == "no_mirror":
        tot_o = np.triu(tot_o) + (np.tril(carry[1], -1) if carry is not None else 0.0)
    return tot_s, tot_o
