"""The nearest-neighbour kernels of csrc/neighbor.hip (include/mdm_neighbor.h) restated: torch's interpolate tap tables and one
feature row in fp64 numpy, the per-element error bound of `mdm_nn_rows`, a numpy fp32 emulation of the kernel's arithmetic with the
faults a wrong kernel could make, and the torch CPU statement of upstream's `Sampler.get_nearest_neighbor` (sampler.py:487-518).
Shared by tests/test_neighbor_cpu.py, tests/test_neighbor_kernels_gpu.py and tests/test_neighbor_gpu.py.  Helpers only, no test
functions; importable without a GPU.

THE BOUND (`row_ref` returns it; nothing in it is measured on the kernel).  u = 2^-24, the unit roundoff of fp32.  The kernel forms
    v   = fl(fl(x - lo) / fl(hi - lo))                       normalize01: three roundings, |v^ - v| <= 3u |v|      (k_n = 3, else 0)
    t   = sum_i fl(wh_i) v_i     over n_h taps, fmaf chain    |t^ - t| <= (n_h + 1 + k_n) u sum_i |wh_i| |v_i|
    o   = sum_j fl(wv_j) t_j     over n_v taps, fmaf chain    |o^ - o| <= (n_v + 1 + n_h + 1 + k_n) u A
with A = sum_j |wv_j| sum_i |wh_i| |v_ij| (the resize of |v| under the absolute tables): a chain of n fused multiply-adds is off by at
most n u of its absolute sum, a table weight is the fp64 weight rounded once to fp32 (+1 per axis), and the error of an operand goes
through a sum with its absolute weights.  So with k = n_h + n_v + 2 + k_n taps-and-roundings (k = k_n without a resize)
    |o^_e - o_e| <= k u A_e.
The norm: every lane sums its own squares in a chain of ceil(D / 256) fused multiply-adds, a wave butterfly adds 6 times and the
workgroup twice more; all terms are non-negative, so the sum is off by (ceil(D / 256) + 8) u relative, its root by half of that plus
u; that o^ stands for o moves the norm by at most ||o^ - o|| <= k u ||A||.  The reciprocal rounds once, the product -- the stored
value -- once.  With n = max(||o||, eps) and y = o / n
    |y^_e - y_e| <= u [ k A_e / n + |y_e| ( (ceil(D / 256) + 8) / 2 + 3 + k ||A|| / ||o|| ) ]  x 1.01      (second-order terms)
A row whose image is constant or holds a NaN is 0 exactly, and so is its bound.
"""
import numpy as np
import torch
import torch.nn.functional as F

from _store_rows import block_sum32, fma32

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
SHAPES = [(3, 32, 32), (1, 28, 28), (3, 33, 47), (3, 64, 64), (3, 100, 100), (3, 256, 256)]     # identity, up, odd non-square, x2, fractional, x8
FAULTS = ("drop_last_tap", "edge_unnormalised", "neighbour_range", "flip_wrong_axis", "nan_kept")
EPS = 1e-8


def plan(n_in, n_out, antialias):
    """-> (first [n_out] int, count [n_out] int, weight [n_out][taps] fp64, zero behind the taps): the rule of mdm_nn_plan in fp64"""
    scale = n_in / n_out
    rows = []
    for i in range(n_out):
        if antialias:
            support = max(scale, 1.0)
            inv = 1.0 / support
            c = scale * (i + 0.5)
            lo = max(0, int(c - support + 0.5))
            hi = min(n_in, int(c + support + 0.5))
            w = np.array([max(0.0, 1.0 - abs((j - c + 0.5) * inv)) for j in range(lo, hi)], f64)
            if w.sum() != 0.0:
                w = w / w.sum()
        else:
            s = max(scale * (i + 0.5) - 0.5, 0.0)
            j0 = min(int(s), n_in - 1)
            j1 = min(j0 + 1, n_in - 1)
            lo = j0
            w = np.array([1.0 - (s - j0), s - j0], f64) if j1 != j0 else np.array([(1.0 - (s - j0)) + (s - j0)], f64)
        rows.append((lo, w))
    taps = max(len(w) for _, w in rows)
    W = np.zeros((n_out, taps), f64)
    for i, (_, w) in enumerate(rows):
        W[i, :len(w)] = w
    return np.array([lo for lo, _ in rows], np.int64), np.array([len(w) for _, w in rows], np.int64), W


def dense(n_in, table, absolute=False, dtype=f64):
    """the table as an [n_out][n_in] matrix"""
    first, count, w = table
    A = np.zeros((len(first), n_in), dtype)
    for i in range(len(first)):
        A[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
    return np.abs(A) if absolute else A


def resize64(x, S, antialias):
    """x [..., H, W] -> [..., S, S] in fp64 under the two tables"""
    x = np.asarray(x, f64)
    Ah, Av = dense(x.shape[-1], plan(x.shape[-1], S, antialias)), dense(x.shape[-2], plan(x.shape[-2], S, antialias))
    return np.einsum("oy,...yx,px->...op", Av, x, Ah)


def normalize64(x):
    """normalize01 of one image [C][H][W] (fp32 values) in fp64; constant or NaN -> None (the row is zero)"""
    x = np.asarray(x, f64)
    if np.isnan(x).any() or x.max() == x.min():
        return None
    return (x - x.min()) / (x.max() - x.min())


def row_ref(x, normalize, flip, S, antialias, eps=EPS):
    """x [C][H][W] as stored (fp32 values) -> (row [D] fp64, bound [D] fp64), the module docstring's"""
    C, H, W = x.shape
    v = np.asarray(x, f64)
    kn = 0
    if normalize:
        v, kn = normalize64(x), 3
        if v is None:
            D = C * S * S if S else C * H * W
            return np.zeros(D), np.zeros(D)
    if flip:
        v = v[..., ::-1]
    if S:
        th, tv = plan(W, S, antialias), plan(H, S, antialias)
        Ah, Av = dense(W, th), dense(H, tv)
        o = np.einsum("oy,cyx,px->cop", Av, v, Ah).reshape(-1)
        A = np.einsum("oy,cyx,px->cop", np.abs(Av), np.abs(v), np.abs(Ah)).reshape(-1)
        k = int(th[1].max()) + int(tv[1].max()) + 2 + kn
    else:
        o, A, k = v.reshape(-1), np.abs(v).reshape(-1), kn
    D = o.size
    e = float(f32(eps))
    no = np.linalg.norm(o)
    n = max(no, e)
    y = o / n
    bound = U * (k * A / n + np.abs(y) * ((-(-D // 256) + 8) / 2 + 3 + k * np.linalg.norm(A) / max(no, 1e-300))) * 1.01
    return y, bound


def emulate_row(x, normalize, flip, S, antialias, eps=EPS, fault=None, neighbour=None):
    """nn_rows_kernel in numpy fp32: the range, (x - lo) / range with NaN -> 0, the mirror, fmaf chains along W then along H in tap
    order, every lane's chain of squares (lane t owns e = t + 256 k of each channel, or the four-element groups g = t + 256 k
    without a resize), the workgroup sum, 1 / max(sqrt, eps), one product.  `fault`: one of FAULTS; `neighbour`: the image whose
    range "neighbour_range" takes."""
    x = np.asarray(x, f32)
    C, H, W = x.shape
    with np.errstate(all="ignore"):
        if normalize:
            src = np.asarray(neighbour, f32) if fault == "neighbour_range" else x
            lo, hi = src.min(), src.max()                     # numpy hands a NaN on, as the kernel's carried flag does
            v = (x - lo) / (hi - lo)
            assert v.dtype == f32
            if fault != "nan_kept":
                v[np.isnan(v)] = 0.0
        else:
            v = x.copy()
    if flip and fault != "flip_wrong_axis":
        v = v[..., ::-1]
    if S:
        th, tv = plan(W, S, antialias), plan(H, S, antialias)
        if fault == "edge_unnormalised" and antialias:
            th = _raw_edges(W, S, th)
        hf, hc, hw = th[0], th[1].copy(), th[2].astype(f32)
        vf, vc, vw = tv[0], tv[1], tv[2].astype(f32)
        if fault == "drop_last_tap":
            hc = np.maximum(hc - 1, 1)
        t = np.zeros((C, H, S), f32)
        for ox in range(S):
            for i in range(hc[ox]):
                t[:, :, ox] = fma32(hw[ox, i], v[:, :, hf[ox] + i], t[:, :, ox])
        o = np.zeros((C, S, S), f32)
        for oy in range(S):
            for j in range(vc[oy]):
                o[:, oy, :] = fma32(vw[oy, j], t[:, vf[oy] + j, :], o[:, oy, :])
        if flip and fault == "flip_wrong_axis":
            o = o[:, ::-1, :]
        SS = S * S
        per = -(-SS // 256) * 256
        lanes = np.zeros((C, per), f32)
        lanes[:, :SS] = o.reshape(C, SS)
        acc = np.zeros(256, f32)
        for c in range(C):
            for k in range(per // 256):
                q = lanes[c, 256 * k:256 * (k + 1)]
                acc = fma32(q, q, acc)
        u = o.reshape(-1)
    else:
        if flip and fault == "flip_wrong_axis":
            v = v[:, ::-1, :]
        u = np.ascontiguousarray(v).reshape(-1)
        D = u.size
        G = -(-D // 4)
        per = -(-G // 256) * 256
        grp = np.zeros((per, 4), f32)
        grp.reshape(-1)[:D] = u
        acc = np.zeros(256, f32)
        for k in range(per // 256):
            for j in range(4):
                q = grp[256 * k:256 * (k + 1), j]
                acc = fma32(q, q, acc)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(block_sum32(acc.reshape(1, 256))[0])
        assert nrm.dtype == f32
        inv = f32(1.0) / np.maximum(nrm, f32(eps))
        return (u * inv).astype(f32)


def _raw_edges(n_in, n_out, table):
    """the fault "edge_unnormalised": the first and last output keep their raw triangle weights (no division by their sum)"""
    first, count, w = table
    w = w.copy()
    scale = n_in / n_out
    support = max(scale, 1.0)
    for i in (0, n_out - 1):
        c = scale * (i + 0.5)
        w[i, :count[i]] = [max(0.0, 1.0 - abs((j - c + 0.5) / support)) for j in range(first[i], first[i] + count[i])]
    return first, count, w


def inside(y, ref, bound):
    y = np.asarray(y, f64)
    return bool(np.isfinite(y).all()) and bool((np.abs(y - ref) <= bound).all())


def worst(y, ref, bound):
    """largest err / bound over the elements with a non-zero bound"""
    err = np.abs(np.asarray(y, f64) - ref)
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ------------------------------------------------------------------ problems
def kernel_images(C, H, W, n=8, seed=0):
    """n float images [n][C][H][W]: smooth structure plus noise, unlike ranges and offsets; image 1 is constant, image 3 holds one NaN
    (callers that want plain images skip them or take PLAIN)"""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    coarse = torch.randn(n, C, 5, 7, generator=g)
    x = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False) + 0.3 * torch.randn(n, C, H, W, generator=g)
    x = x * torch.linspace(0.5, 3.0, n).view(n, 1, 1, 1) + torch.linspace(-1.0, 2.0, n).view(n, 1, 1, 1)
    x[1] = 0.25
    x[3, C - 1, H // 2, W // 3] = float("nan")
    return x


CONSTANT, WITH_NAN = 1, 3


def as_bytes(x):
    """float images -> uint8 images of the same structure (each image's own range spread over 0..255, NaN -> 0)"""
    x = torch.nan_to_num(x, nan=0.0)
    lo, hi = x.amin((1, 2, 3), keepdim=True), x.amax((1, 2, 3), keepdim=True)
    return ((x - lo) / (hi - lo).clamp_min(1e-6) * 255.0).round().clamp(0, 255).to(torch.uint8)


def host_set(M, C, size, seed=0):
    """the data of tests/test_neighbor_gpu.py: every image a random 4 x 4 x C grid bilinearly upsampled plus 0.05 randn"""
    g = torch.Generator().manual_seed(seed)
    grid = torch.rand(M, C, 4, 4, generator=g) * 2 - 1
    return F.interpolate(grid, size=(size, size), mode="bilinear", align_corners=False) + 0.05 * torch.randn(M, C, size, size, generator=g)


def host_sources(data, picks, seed=1):
    """normalize01 of the picked data images plus 0.05 randn"""
    g = torch.Generator().manual_seed(seed)
    x = normalize01_torch(data[picks])
    return x + 0.05 * torch.randn(x.shape, generator=g)


def normalize01_torch(x):
    """utils/datautils.py:211-222 on a batch [N][C][H][W], torch fp32 on the CPU"""
    lo, hi = x.amin((1, 2, 3), keepdim=True), x.amax((1, 2, 3), keepdim=True)
    return torch.nan_to_num((x - lo) / (hi - lo), nan=0.0)


# ------------------------------------------------------------------ upstream's method on the CPU
def resize_torch(x, size, antialias):
    """what torchvision's tensor Resize([size, size]) dispatches to (torchvision/transforms/v2/functional/_geometry.py resize_image:
    interpolate(mode="bilinear", align_corners=False, antialias=...)); taken from its published source, parity unpinned"""
    return F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False, antialias=antialias)


def flip_draws(M, B):
    """the draws of RandomHorizontalFlip() applied to each data-loader batch as ONE tensor (sampler.py:492, 504): one
    `torch.rand(1) < 0.5` from the default host generator per batch of B images, in data order -> a bool per batch"""
    return [bool(torch.rand(1) < 0.5) for _ in range(0, M, B)]


def scores_torch(source, data, antialias, size=32, augment=False):
    """score [M][B] of sampler.py:487-512 on the CPU (data: the stored fp32 images); draws from the default generator as upstream"""
    B = source.shape[0]
    small = lambda x: x if size is None else resize_torch(x, size, antialias)
    src = small(source).flatten(1)
    out = []
    for i in range(0, data.shape[0], B):
        d = normalize01_torch(data[i:i + B])
        sim = F.cosine_similarity(src[None, :, :], small(d).flatten(1)[:, None, :], dim=2)
        if augment:
            d_aug = torch.flip(d, dims=[-1]) if bool(torch.rand(1) < 0.5) else d
            sim = torch.max(sim, F.cosine_similarity(src[None, :, :], small(d_aug).flatten(1)[:, None, :], dim=2))
        out.append(sim)
    return torch.cat(out, dim=0)


def similar_neighbor_ref(generated, img_set, idx, th):
    """tester.py:209-223 line for line, torch on the CPU"""
    cs = lambda a, b: F.cosine_similarity(a.flatten(), b.flatten(), dim=0)
    for i in range(len(generated)):
        is_similar = False
        if img_set[idx[i]].shape[0] > 0:
            for j in range(img_set[idx[i]].shape[0]):
                score = cs(generated[i], img_set[idx[i]][j])
                if score > th:
                    is_similar = True
                    break
            if not is_similar:
                img_set[idx[i]] = torch.cat((img_set[idx[i]], generated[i].unsqueeze(dim=0)), dim=0)
        else:
            img_set[idx[i]] = torch.cat((img_set[idx[i]], generated[i].unsqueeze(dim=0)), dim=0)
    return img_set
