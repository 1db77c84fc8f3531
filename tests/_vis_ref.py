"""CPU reference of the image grids (include/mdm_vis.h): upstream's two normalisations, torchvision's `make_grid` and `save_image`'s
quantisation, written from their semantics in torch / numpy, plus the row tables of tests/test_vis_kernels_gpu.py.  Helpers only, no
test functions; importable without a GPU.

`normalize01` is the oracle's (oracle/evaluate_ref.py, upstream utils/datautils.py:211-222).  `make_grid_ref` follows torchvision's
loop -- a canvas of pad_value, image k copied into cell (k // xmaps, k % xmaps) -- and is anchored by a hand-computed case in
tests/test_vis_cpu.py, since torchvision itself is not a dependency."""
import math

import numpy as np
import torch

from oracle.evaluate_ref import normalize01

NAN, INF = float("nan"), float("inf")


def normalize01_global(data):
    """utils/datautils.py:225-229: one min / max over the batch, no NaN handling (a constant batch is 0 / 0 = NaN)."""
    hi, lo = torch.max(data), torch.min(data)
    return (data - lo) / (hi - lo)


NORMALIZE = {None: lambda x: x, "image": normalize01, "global": normalize01_global}


def grid_shape_ref(K, C, H, W, nrow, padding):
    Cg = 3 if C == 1 else C
    if K == 1:
        return Cg, H, W
    xmaps = min(nrow, K)
    ymaps = int(math.ceil(K / xmaps))
    return Cg, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def make_grid_ref(x, nrow, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid(x, nrow, padding, pad_value=pad_value, normalize=False) for x [K, C, H, W] -> [Cg, Hg, Wg]"""
    x = x.float()
    K, C, H, W = x.shape
    if C == 1:
        x = torch.cat((x, x, x), 1)
    if K == 1:
        return x[0].clone()
    Cg, Hg, Wg = grid_shape_ref(K, C, H, W, nrow, padding)
    xmaps = min(nrow, K)
    grid = torch.full((Cg, Hg, Wg), float(pad_value), dtype=torch.float32)
    for k in range(K):
        r, c = divmod(k, xmaps)
        y0, x0 = r * (H + padding) + padding, c * (W + padding) + padding
        grid[:, y0:y0 + H, x0:x0 + W] = x[k]
    return grid


def to_u8_ref(grid):
    """save_image's `mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)` on a CHW grid -> [Hg, Wg, Cg] uint8: fp32
    product, then fp32 sum (numpy rounds each), NaN -> 0 (mdm_vis.h defines what torch leaves open), truncation."""
    g = grid.detach().cpu().float().numpy()
    with np.errstate(all="ignore"):
        q = g * np.float32(255.0)
        q = q + np.float32(0.5)
        assert q.dtype == np.float32
        q = np.where(np.isnan(q), np.float32(0.0), np.clip(q, np.float32(0.0), np.float32(255.0)))
    return torch.from_numpy(np.ascontiguousarray(q.astype(np.uint8).transpose(1, 2, 0)))


def grid_ref(x, nrow, normalization, padding=2, pad_value=0.0):
    """-> (fp32 CHW grid, uint8 HWC grid) of a CPU batch, as Sampler._save_image_grid chains the pieces"""
    g = make_grid_ref(NORMALIZE[normalization](x.detach().cpu().float()), nrow, padding, pad_value)
    return g, to_u8_ref(g)


def same_grid(got, want):
    """fp32 grids bit for bit where the reference is a number; where it is NaN the grid must be NaN (any payload)"""
    got, want = got.detach().cpu().float().contiguous(), want.detach().cpu().float().contiguous()
    if got.shape != want.shape:
        return False
    nan = torch.isnan(want)
    return bool(torch.isnan(got[nan]).all()) and torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


def range_ref(x, per_image):
    """x [K, E] -> [K, 2] (amin, amax per image) or [1, 2] (min, max of the batch); a NaN is handed on by both"""
    if per_image:
        return torch.stack((torch.amin(x, 1), torch.amax(x, 1)), 1)
    return torch.stack((torch.min(x), torch.max(x)))[None]


# ------------------------------------------------------------------ rows of tests/test_vis_kernels_gpu.py
RANGE_ES = (1, 3, 255, 257, 768, 1000)
RANGE_KS = (1, 5)
RANGE_STRIDE_EXTRA = (0, 7)
GRID_SHAPES = [(1, 1, 1), (1, 3, 5), (3, 16, 16), (4, 8, 24)]                   # (C, H, W)
GRID_KN = [(1, 1), (2, 2), (4, 2), (5, 3), (7, 8), (7, 1)]                      # (K, nrow): (5, 3) leaves a cell unfilled, (7, 8) has nrow > K
GRID_PADS = [(0, 0.0), (3, 0.5)]                                                # besides (2, 0.0), on GRID_PAD_SHAPES only
GRID_PAD_SHAPES = [(3, 16, 16), (1, 3, 5)]
GRID_ROWS = [(s, kn, 2, 0.0) for s in GRID_SHAPES for kn in GRID_KN] + [(s, kn, p, pv) for s in GRID_PAD_SHAPES for kn in GRID_KN for p, pv in GRID_PADS]


def grid_row_id(r):
    (C, H, W), (K, nrow), p, pv = r
    return f"{C}x{H}x{W}-K{K}-nrow{nrow}-pad{p}-{pv}"


FINITE_KINDS = ("plain", "max_last", "min_last", "negative", "constant")


def image_kinds(K, E, seed=0, kinds=None):
    """K images of E elements cycling through `kinds` -- by default those of _store_rows.NORM_KINDS (plain, the extremum in the last
    element, all negative, constant, one +inf, one NaN) --, starting at kind number `seed`"""
    from _store_rows import NORM_KINDS
    kinds = NORM_KINDS if kinds is None else kinds
    g = torch.Generator().manual_seed(1000 * K + E + seed)
    x = torch.randn(K, E, generator=g) * 2.0 + 0.5
    for k in range(K):
        kind = kinds[(k + seed) % len(kinds)]
        if kind == "max_last":
            x[k, -1] = 50.0
        elif kind == "min_last":
            x[k, -1] = -50.0
        elif kind == "negative":
            x[k] = -x[k].abs() - 1.0
        elif kind == "constant":
            x[k] = 0.3
        elif kind == "inf":
            x[k, E // 2] = INF
        elif kind == "nan":
            x[k, (2 * E) // 3] = NAN
    return x


def quant_edges():
    """fp32 values around every rounding edge of the quantisation: the neighbours (-2 .. +2 ulp) of (k + 0.5) / 255 for k = 0 .. 254,
    then values below 0, above 1, infinities and NaN -> [n]"""
    e = (torch.arange(255, dtype=torch.float64) + 0.5) / 255.0
    c = e.float()
    vals = [c]
    up, dn = c.clone(), c.clone()
    for _ in range(2):
        up = torch.nextafter(up, torch.tensor(INF))
        dn = torch.nextafter(dn, torch.tensor(-INF))
        vals += [up.clone(), dn.clone()]
    extra = torch.tensor([-1.0, -1e-3, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -23, 1.5, 300.0, INF, -INF, NAN, 0.5 / 255 - 1e-9, 254.5 / 255])
    return torch.cat(vals + [extra])
