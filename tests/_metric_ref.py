"""The image metrics of include/mdm_metric.h stated in fp64 torch, written from the header's formulas and not from the kernel: the
SSIM map through ONE non-separable 121-tap window (`F.conv2d` in double, valid region), the eight outputs per row, and what the derived
bound of tests/_metric_bounds.py needs per position.  Also the input classes the CPU and the GPU tests share.  Helpers only, no test
functions; importable without a GPU.

Parity with torchmetrics / skimage is UNPINNED (neither package was available); tests/test_metric_cpu.py holds this statement to a
second one through scipy.ndimage.gaussian_filter."""
import math

import numpy as np
import torch
import torch.nn.functional as F

K, SIGMA = 11, 1.5
SLOTS = ("mse", "psnr", "ssim", "mse_hole", "psnr_hole", "ssim_hole", "hole_count", "hole_windows")


def window64():
    """the 11 Gaussian weights, normalised, in double"""
    g = torch.exp(-(torch.arange(K, dtype=torch.float64) - K // 2) ** 2 / (2 * SIGMA * SIGMA))
    return g / g.sum()


def clamp_keep_nan(pred, clamp):
    """what save_image shows, by comparisons: a NaN stays a NaN"""
    if clamp is None or not clamp[0] < clamp[1]:
        return pred
    lo, hi = (torch.tensor(v, dtype=pred.dtype) for v in clamp)
    p = torch.where(pred < lo, lo, pred)
    return torch.where(p > hi, hi, p)


def hole_mask(keep, N, C, H, W):
    """bool [N, C, H, W]: keep == 0 (so -0 is hole and NaN is given); everything with keep None"""
    if keep is None:
        return torch.ones(N, C, H, W, dtype=torch.bool)
    assert keep.shape[0] == N and keep.shape[1] in (1, C) and tuple(keep.shape[2:]) == (H, W)
    return (keep == 0).expand(N, C, H, W).clone()


def _win(x64, w2):
    R, C, H, W = x64.shape
    return F.conv2d(x64.reshape(R * C, 1, H, W), w2).reshape(R, C, H - K + 1, W - K + 1)


def reference(pred, truth, keep=None, data_range=2.0, clamp=(-1.0, 1.0)):
    """pred [R, C, H, W] and truth [N, C, H, W] fp32 on the host, keep None or [N, Ck, H, W] -> dict of fp64 tensors:
    `out` [R, 8] (the slots of the header; NaN and inf where the header says so), `map` [R, C, H - 10, W - 10], the per-position
    moments `mu_p mu_t var_p var_t cov`, `p` (clamped) and `t` (row r's truth) [R, C, H, W], the masks `hole` and `hole_c`."""
    R, C, H, W = pred.shape
    N = truth.shape[0]
    assert R % N == 0 and truth.shape[1:] == pred.shape[1:] and H >= K and W >= K
    L = float(np.float32(data_range))
    C1, C2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    p = clamp_keep_nan(pred.float(), clamp).double()
    t = truth.double().repeat(R // N, 1, 1, 1)                               # row r reads truth[r % N]
    hole = hole_mask(keep, N, C, H, W).repeat(R // N, 1, 1, 1)
    hole_c = hole[:, :, K // 2:H - K // 2, K // 2:W - K // 2]                # the centre element of each window
    w = window64()
    w2 = torch.outer(w, w)[None, None]
    mu_p, mu_t = _win(p, w2), _win(t, w2)
    var_p, var_t, cov = _win(p * p, w2) - mu_p * mu_p, _win(t * t, w2) - mu_t * mu_t, _win(p * t, w2) - mu_p * mu_t
    smap = ((2 * mu_p * mu_t + C1) * (2 * cov + C2)) / ((mu_p * mu_p + mu_t * mu_t + C1) * (var_p + var_t + C2))
    sq = (p - t) ** 2
    out = torch.empty(R, 8, dtype=torch.float64)
    for r in range(R):
        h, hc = hole[r], hole_c[r]
        nh, nhc = int(h.sum()), int(hc.sum())
        mse = sq[r].mean()
        mse_h = sq[r][h].sum() / nh if nh else torch.tensor(math.nan, dtype=torch.float64)
        out[r, 0], out[r, 3] = mse, mse_h
        out[r, 1], out[r, 4] = (10 * torch.log10(L * L / m) for m in (mse, mse_h))
        out[r, 2] = smap[r].mean()
        out[r, 5] = smap[r][hc].sum() / nhc if nhc else math.nan
        out[r, 6], out[r, 7] = nh, nhc
    return dict(out=out, map=smap, mu_p=mu_p, mu_t=mu_t, var_p=var_p, var_t=var_t, cov=cov, p=p, t=t, hole=hole, hole_c=hole_c,
                C1=C1, C2=C2, L=L)


def reference_scipy(pred, truth, data_range=2.0, clamp=(-1.0, 1.0)):
    """The SSIM map once more, through scipy.ndimage.gaussian_filter(sigma = 1.5, truncate = 3.5) per plane, cropped by 5."""
    from scipy.ndimage import gaussian_filter
    R, C, H, W = pred.shape
    L = float(np.float32(data_range))
    C1, C2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    p = clamp_keep_nan(pred.float(), clamp).double().numpy()
    t = truth.double().repeat(R // truth.shape[0], 1, 1, 1).numpy()
    f = lambda a: np.stack([[gaussian_filter(a[r, c], sigma=SIGMA, truncate=3.5)[5:H - 5, 5:W - 5] for c in range(C)] for r in range(R)])
    mp, mt = f(p), f(t)
    vp, vt, cv = f(p * p) - mp * mp, f(t * t) - mt * mt, f(p * t) - mp * mt
    return torch.from_numpy(((2 * mp * mt + C1) * (2 * cv + C2)) / ((mp * mp + mt * mt + C1) * (vp + vt + C2)))


# ------------------------------------------------------------------ the input classes
IMAGE_KINDS = ("noise", "smooth", "two_level", "equal", "near", "outside")
KEEP_KINDS = ("none", "zeros", "ones", "box", "random", "random_c", "nan")


def _smooth(g, n, C, H, W):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = torch.rand(n, C, 1, 1, generator=g) * 1.2 - 0.6
    for _ in range(3):
        fx, fy = (torch.randint(0, 3, (n, C, 1, 1), generator=g).float() for _ in range(2))
        ph, amp = torch.rand(n, C, 1, 1, generator=g) * 2 * math.pi, torch.rand(n, C, 1, 1, generator=g) * 0.25
        img = img + amp * torch.cos(2 * math.pi * (fx * xx / W + fy * yy / H) + ph)
    return img.clamp(-1, 1)


def _two_level(g, n, C, H, W):
    """each plane holds two constants, split along a row or a column drawn per plane: the variances cancel exactly"""
    a, b = torch.rand(n, C, 1, 1, generator=g) * 2 - 1, torch.rand(n, C, 1, 1, generator=g) * 2 - 1
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cut_y, cut_x = torch.randint(1, H, (n, C, 1, 1), generator=g), torch.randint(1, W, (n, C, 1, 1), generator=g)
    by_row = torch.rand(n, C, 1, 1, generator=g) < 0.5
    first = torch.where(by_row, yy < cut_y, xx < cut_x)
    return torch.where(first, a, b).contiguous()


def draw_images(kind, R, N, C, H, W, seed=0):
    """-> (pred [R, C, H, W], truth [N, C, H, W]) fp32, contiguous"""
    g = torch.Generator().manual_seed(1000 * IMAGE_KINDS.index(kind) + 17 * H + W + seed)
    reps = R // N
    if kind == "noise":
        pred, truth = torch.rand(R, C, H, W, generator=g) * 2 - 1, torch.rand(N, C, H, W, generator=g) * 2 - 1
    elif kind == "smooth":
        pred, truth = _smooth(g, R, C, H, W), _smooth(g, N, C, H, W)
    elif kind == "two_level":
        pred, truth = _two_level(g, R, C, H, W), _two_level(g, N, C, H, W)
    elif kind == "equal":
        truth = _smooth(g, N, C, H, W)
        pred = truth.repeat(reps, 1, 1, 1)
    elif kind == "near":
        truth = _smooth(g, N, C, H, W) * 0.9
        pred = truth.repeat(reps, 1, 1, 1) + 1e-4 * (torch.rand(R, C, H, W, generator=g) * 2 - 1)
    elif kind == "outside":
        pred, truth = torch.rand(R, C, H, W, generator=g) * 6 - 3, _smooth(g, N, C, H, W)
    else:
        raise ValueError(kind)
    return pred.float().contiguous(), truth.float().contiguous()


def draw_keep(kind, N, C, H, W, seed=0):
    """-> None or keep [N, Ck, H, W] fp32"""
    g = torch.Generator().manual_seed(77 + KEEP_KINDS.index(kind) + seed)
    if kind == "none":
        return None
    if kind == "zeros":
        return torch.zeros(N, 1, H, W)
    if kind == "ones":
        return torch.ones(N, 1, H, W)
    if kind == "box":
        k = torch.ones(N, 1, H, W)
        k[:, :, H // 4:H // 4 + max(1, H // 2), W // 3:W // 3 + max(1, W // 2)] = 0
        return k
    if kind == "random":
        return (torch.rand(N, 1, H, W, generator=g) >= 0.4).float()
    if kind == "random_c":
        return (torch.rand(N, C, H, W, generator=g) >= 0.4).float() * 0.5     # 0.5 is given like 1
    if kind == "nan":
        k = (torch.rand(N, C, H, W, generator=g) >= 0.5).float()
        k.reshape(-1)[::5] = math.nan                                         # a NaN counts as given
        k.reshape(-1)[1::7] = -0.0                                            # -0 is hole
        return k
    raise ValueError(kind)
