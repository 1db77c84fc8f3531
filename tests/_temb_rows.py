"""Row tables of the time-embedding path and helper-kernel bound tests, what draws a row's problem, and an fp32 emulation of each
kernel's arithmetic with the faults a wrong kernel could make.  Shared by tests/test_temb_bounds_gpu.py and
tests/test_helper_kernels_gpu.py (which run the rows on the GPU) and by tests/test_temb_bounds_cpu.py and tests/test_bounds_cpu.py
(which check the routes and emulate the rows without one).  Helpers only, no test functions."""
from collections import namedtuple

import numpy as np
import torch

# ------------------------------------------------------------------ the skinny kernels (csrc/temb.hip)
# forward: bias / act / emb: the optional operand is given; pad: what every pitch (ldx, ldw, ldy) has over the dense one; temb: the
# input is the embedding of t (K = hid) in `variant` = (flip_sin_to_cos, freq_shift)
Fwd = namedtuple("Fwd", "route M N K bias act pad temb variant emb")
# backward: pre given (splits == 1: applied by the kernel; splits > 1: by silu_bwd_sum on the slabs); pad on lddy and ldw
Bwd = namedtuple("Bwd", "route M N K splits pre pad")

MS = (1, 15, 16, 17, 32, 33, 100, 128)             # MB = 2: the edges of one and two 16-row blocks; MB = 8: 3, 7 and 8 blocks
NS = (16, 48, 80, 2048, 2080, 2064)                # one, three, five workgroups; NB = 2 (64 and 65 workgroups); >= 2048 with NB = 1
# every state of the look-ahead loop.  MB = 2 (DEPTH 8, a wave owns K / 64 chunks): one live chunk of eight, two, exactly one full
# trip, a full trip plus one live chunk.  MB = 8 (DEPTH 2): one live chunk of two, one full trip, a full trip plus one live chunk
KS = {2: (64, 128, 512, 576), 8: (64, 128, 192)}
HIDS = (64, 128, 192)
PADS = (0, 4, 20)
VARIANTS = ((0, 1.0), (1, 0.0))
SPLITS = (1, 2, 13, 16)
BWD_NS = (16, 80, 512)


def route_rule(which, M, N, K, has_t):
    """the rule of csrc/temb.hip's skinny_route, restated: MB from M, NB from N, TEMB from t; None for a refused shape"""
    if not (1 <= M <= 128 and N >= 16 and N % 16 == 0 and K >= 64 and K % 64 == 0):
        return None
    mb = 2 if M <= 32 else 8
    if which == 1:
        return None if has_t else f"nn<{mb},1>"
    if has_t:
        return f"nt<{mb},1,temb>"
    return f"nt<{mb},{2 if N >= 2048 and N % 32 == 0 else 1}>"


def _fwd_rows():
    rows = []
    for i, M in enumerate(MS):
        mb = 2 if M <= 32 else 8
        for j, N in enumerate(NS):
            q = 5 * i + j
            K = KS[mb][(i + j) % len(KS[mb])]
            rows.append(Fwd(route_rule(0, M, N, K, 0), M, N, K, q % 2, (q // 2) % 2, PADS[q % 3], 0, None, 0))
    for i, M in enumerate(MS):
        for j, N in enumerate(NS[:3]):
            q = 3 * i + j
            K = HIDS[(i + j) % 3]
            rows.append(Fwd(route_rule(0, M, N, K, 1), M, N, K, q % 2, (q // 2) % 2, PADS[(q // 2) % 3], 1, VARIANTS[(q // 3) % 2], int(q % 4 != 3)))
    # timesteps into a wide layer: the launcher once sized this grid for two column blocks per workgroup and launched the kernel
    # that covers one, so that columns N / 2 .. N - 1 were never written
    rows.append(Fwd("nt<2,1,temb>", 1, 2048, 64, 1, 1, 0, 1, VARIANTS[0], 1))
    return rows


def _bwd_rows():
    rows = []
    for i, M in enumerate(MS):
        for j, s in enumerate(SPLITS):
            N = BWD_NS[(i + j) % 3]
            K = (64, 128)[(i + j // 2) % 2] * s
            rows.append(Bwd(route_rule(1, M, N, K, 0), M, N, K, s, int((i + j) % 2 == 0), PADS[(i + 2 * j) % 3]))
    return rows


FWD_ROWS, BWD_ROWS = _fwd_rows(), _bwd_rows()
# (which, M, N, K, splits, what): refused by shape (mdm_skinny_supported / the route query).  The entry points also refuse both or
# neither of x and t and a pitch that is not a multiple of 4 (tests/test_temb_bounds_gpu.py)
REFUSALS = [(w, M, N, K, s) for w in (0, 1) for (M, N, K, s) in
            ((0, 16, 64, 1), (129, 16, 64, 1), (4, 8, 64, 1), (4, 24, 64, 1), (4, 16, 32, 1), (4, 16, 96, 1))] + [(1, 4, 16, 128, 3)]
SUM_ROWS = [(nslab, pre, n) for nslab in (1, 2, 13) for pre in (0, 1) for n in (4, 4 * 257)]      # silu_bwd_sum on drawn slabs


def fwd_id(r):
    form = ("b" if r.bias else "") + ("a" if r.act else "") + ("e" if r.emb else "")
    v = f"-v{r.variant[0]}{r.variant[1]:g}" if r.temb else ""
    return f"{r.route}-{r.M}x{r.N}x{r.K}-{form or 'plain'}-pad{r.pad}{v}"


def bwd_id(r):
    return f"{r.route}-{r.M}x{r.N}x{r.K}-s{r.splits}-{'pre' if r.pre else 'lin'}-pad{r.pad}"


def timesteps(M, seed):
    """0, 1, 999, 1000, a non-integer and random integers; rows 0 and 16 differ"""
    g = torch.Generator().manual_seed(seed)
    base = [1000.0, 0.0, 1.0, 999.0, 41.5]
    t = torch.randint(2, 999, (M,), generator=g).float()
    if M == 1:
        t[0] = base[seed % 5]
    else:
        t[:min(M, 5)] = torch.tensor(base[:min(M, 5)])
    assert M <= 16 or float(t[0]) != float(t[16])
    return t


def fwd_problem(r):
    """-> dict(x [M][K] | t [M], W [N][K], bias [N]) of fp32 tensors"""
    seed = 1000 * r.M + r.N + 7 * r.K + r.temb
    g = torch.Generator().manual_seed(seed)
    T = dict(W=torch.randn(r.N, r.K, generator=g) * 0.5, bias=torch.randn(r.N, generator=g))
    if r.temb:
        T["t"] = timesteps(r.M, seed)
    else:
        T["x"] = torch.randn(r.M, r.K, generator=g)
    return T


def bwd_problem(r):
    """-> dict(dy [M][K], W [K][N], pre [M][N]): pre spans silu''s sign change (silu' < 0 below -1.28)"""
    g = torch.Generator().manual_seed(1000 * r.M + r.N + 7 * r.K + r.splits)
    return dict(dy=torch.randn(r.M, r.K, generator=g), W=torch.randn(r.K, r.N, generator=g) * 0.5,
                pre=torch.randn(r.M, r.N, generator=g) * 2.5)


# ------------------------------------------------------------------ fp32 emulation of the skinny kernels, with planted faults
FWD_FAULTS = {                       # fault -> the rows that can show it
    "drop_last_chunk": lambda r: True,
    "chunk_twice": lambda r: True,
    "row16_takes_t0": lambda r: r.temb and r.M >= 17,
    "bias_shifted": lambda r: r.bias,
    "act_before_bias": lambda r: r.bias and r.act,
    "shift_swapped": lambda r: r.temb and r.emb,
    "j_off_by_one": lambda r: r.temb and r.emb,
    "sin_cos_swapped": lambda r: r.temb and r.emb,
    "half_from_N": lambda r: r.temb and r.emb and r.N != r.K,
    "upper_half_unwritten": lambda r: r.temb and r.N >= 2048 and r.N % 32 == 0,
}
BWD_FAULTS = {
    "drop_last_chunk": lambda r: True,
    "chunk_twice": lambda r: True,
    "no_silu_grad_on_split": lambda r: r.splits > 1 and r.pre,
    "last_slab_left_out": lambda r: r.splits > 1,
    "slab_range_shifted": lambda r: r.splits > 1,
}


def silu32(v):
    return v / (1 + torch.exp(-v))


def silu_grad32(v):
    s = 1 / (1 + torch.exp(-v))
    return s * (1 + v * (1 - s))


def temb32(t, dim, flip, shift, fault=None, N=None):
    """the embedding in fp32 numpy, operation for operation as temb_elem / temb_kernel -> fp32 tensor [M][dim]"""
    f32 = np.float32
    half = dim // 2
    t = np.asarray(t, dtype=f32).copy()
    if fault == "row16_takes_t0":
        t[16] = t[0]
    if fault == "shift_swapped":
        shift = 1.0 - shift
    j = np.arange(half) + (1 if fault == "j_off_by_one" else 0)
    den = f32(N // 2 if fault == "half_from_N" else half) - f32(shift)
    c = np.log(f32(10000.0)) / den
    assert c.dtype == f32
    a = t[:, None] * np.exp(-(j.astype(f32)) * c)[None]
    assert a.dtype == f32
    s, co = np.sin(a), np.cos(a)
    if fault == "sin_cos_swapped":
        s, co = co, s
    parts = [co, s] if flip else [s, co]
    if dim & 1:
        parts.append(np.zeros((len(t), 1), f32))
    return torch.from_numpy(np.concatenate(parts, 1))


def _waves(A, B, k0, k1, fault):
    """sum_{k in [k0, k1)} A[:, k] B[:, k]^T as the workgroup forms it: four wave partials over a quarter of the range each, in
    fp32, summed w0 + w1 + w2 + w3.  A [M][K], B [N][K] fp32."""
    kq = (k1 - k0) // 4
    parts = []
    for w in range(4):
        lo, hi = k0 + w * kq, k0 + (w + 1) * kq
        if fault == "drop_last_chunk" and w == 2:
            hi -= 16
        p = A[:, lo:hi] @ B[:, lo:hi].t() if hi > lo else torch.zeros(A.shape[0], B.shape[0])
        if fault == "chunk_twice" and w == 1:
            p = p + A[:, lo - 16:lo] @ B[:, lo - 16:lo].t()
        parts.append(p)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def emulate_fwd(r, T, fault=None):
    """-> dict(y, act, emb) fp32 (act / emb None where the row has none).  An unwritten element is NaN."""
    emb = None
    if r.temb:
        emb = temb32(T["t"], r.K, r.variant[0], r.variant[1], fault, r.N)
        x = emb
    else:
        x = T["x"]
    acc = _waves(x, T["W"], 0, r.K, fault)
    bias = T["bias"] if r.bias else None
    if bias is not None and fault == "bias_shifted":
        bias = torch.roll(bias, -4)
    y = acc + bias if bias is not None else acc
    act = silu32(acc if fault == "act_before_bias" else y) if r.act else None
    if fault == "upper_half_unwritten":
        y = y.clone()
        y[:, r.N // 2:] = float("nan")
        if act is not None:
            act[:, r.N // 2:] = float("nan")
    return dict(y=y, act=act, emb=emb if r.emb else None, emb_used=emb)


def emulate_bwd(r, T, fault=None):
    """-> dict(slabs [splits][M][N] | None, dx [M][N]): the split launch and silu_bwd_sum behind it, or the unsplit launch"""
    dy, Wt = T["dy"], T["W"].t().contiguous()                  # [N][K]
    ks = r.K // r.splits
    slabs = []
    for s in range(r.splits):
        k0 = s * ks + (16 if fault == "slab_range_shifted" and s == 0 else 0)
        slabs.append(_waves(dy, Wt, k0, k0 + ks, fault if s == r.splits - 1 else None))
    if r.splits == 1:
        return dict(slabs=None, dx=slabs[0] * silu_grad32(T["pre"]) if r.pre else slabs[0])
    slabs = torch.stack(slabs)
    return dict(slabs=slabs, dx=emulate_sum(slabs, T["pre"] if r.pre else None, fault))


def emulate_sum(slabs, pre, fault=None):
    s = slabs[0].clone()
    for q in range(1, slabs.shape[0] - (1 if fault == "last_slab_left_out" else 0)):
        s = s + slabs[q]
    return s * silu_grad32(pre) if pre is not None and fault != "no_silu_grad_on_split" else s


def clamped_reads(r):
    """Every address the loads of a row's launch form, as the kernels compute them (clamped row / column, dead chunks at the wave's
    first chunk, the four k-rows of skinny_nn_kernel): -> {operand: (lowest, highest) element offset read}.  Host arithmetic."""
    bwd = isinstance(r, Bwd)
    mb = 2 if r.M <= 32 else 8
    depth = 8 if mb <= 2 else 2
    nb = 2 if (not bwd and not r.temb and r.N >= 2048 and r.N % 32 == 0) else 1
    splits = r.splits if bwd else 1
    ks = r.K // splits
    kq = ks // 4
    lane = np.arange(64)
    r16, kg = lane & 15, 4 * (lane >> 4)
    out = {}

    def see(name, idx):
        lo, hi = int(idx.min()), int(idx.max())
        a, b = out.get(name, (lo, hi))
        out[name] = (min(a, lo), max(b, hi))
    blk = np.arange(-(-r.N // (16 * nb)), dtype=np.int64)[:, None]          # every workgroup of the grid at once
    for sp in range(splits):
        for wave in range(4):
            kbeg = sp * ks + wave * kq
            for kb in range(kbeg, kbeg + kq, 16 * depth):
                for u in range(depth):
                    live = kb + 16 * u < kbeg + kq
                    kc = ((kb + 16 * u + kg) if live else kbeg + kg).astype(np.int64)[None]
                    for j in range(nb):
                        n = np.minimum(blk * 16 * nb + j * 16 + r16[None], r.N - 1)
                        for d in (0, 3):                                    # first and last element of the float4 / of the four k-rows
                            see("W", (kc + d) * (r.N + r.pad) + n if bwd else n * (r.K + r.pad) + kc + d)
                    if bwd or not r.temb:
                        for i in range(mb):
                            m = np.minimum(i * 16 + r16, r.M - 1).astype(np.int64)[None]
                            for d in (0, 3):
                                see("dy" if bwd else "x", m * (r.K + r.pad) + kc + d)
    return out


# ------------------------------------------------------------------ the helper kernels (end of csrc/norm.hip)
COLSUM_CS, COLSUM_PS, COLSUM_NS = (8, 64, 72, 136), (1, 31, 32, 33, 50), (1, 3)
# (per_img: None | "dense" | "pitched" (ld = C + 16, column offset 8), acc_img, dbias given)
COLSUM_FORMS = [(pi, acc, db) for pi in (None, "dense", "pitched") for acc in (0, 1) for db in (0, 1)
                if (pi is not None or (db and not acc))]


def colsum_rows(dt, C):
    """the rows of one (storage type, C): every P and N, the operand forms cycling -> [(P, N, per_img, acc_img, dbias)]"""
    base = COLSUM_CS.index(C) * 3 + (5 if dt == "bf16" else 0)
    return [(P, N) + COLSUM_FORMS[(base + 2 * i + j) % len(COLSUM_FORMS)]
            for i, P in enumerate(COLSUM_PS) for j, N in enumerate(COLSUM_NS)]


def colsum_problem(dt, C, P, N):
    g = torch.Generator().manual_seed(C + 10 * P + N)
    d = torch.randn(N, P, C, generator=g)
    d = d.bfloat16().float() if dt == "bf16" else d
    return d, torch.randn(N, C, generator=g), torch.randn(C, generator=g) + 2.0


def emulate_colsum(d, prior_img, prior_bias, fault=None):
    """32 pixel-lane partials (pixel p on lane p % 32, in order), then their 32-term sum in lane order; the images in order onto the
    prior of dbias -> (per_img [N][C], dbias [C]) fp32"""
    N, P, C = d.shape
    lanes = torch.zeros(N, 32, C)
    for p in range(P):
        lanes[:, p % 32] = lanes[:, p % 32] + d[:, p]
    a = torch.zeros(N, C)
    for l in range(31 if fault == "no_lane_31" else 32):
        a = a + lanes[:, l]
    per = a if prior_img is None or fault == "store_not_accumulate" else prior_img + a
    tot = torch.zeros(C)
    for n in range(N):
        tot = tot + a[n]
    return per, (tot if fault == "store_not_accumulate" else prior_bias + tot)


# ------------------------------------------------------------------ what a row's outputs are held to (GPU rows and emulation alike)
def check_fwd(r, T, got, name=None):
    """got = dict(y, act, emb) as stored by the launch (or by emulate_fwd) -> {output: largest err / bound}; raises where one
    leaves its bound (tests/_bounds.py, the time-embedding section)"""
    from _bounds import U_F32, check, check_bound, linear_ref, silu_ref, temb_ref
    name, out = name or fwd_id(r), {}
    bias = T["bias"] if r.bias else None
    if r.temb and r.emb:
        out["emb"] = check_bound(f"{name} emb_out", got["emb"], *temb_ref(T["t"], r.K, *r.variant))[0]
    if r.temb and not r.emb:
        eref, eb = temb_ref(T["t"], r.K, *r.variant)
        ref, mag = linear_ref(eref, T["W"], bias)
        g = (r.K + 1 + 8) * 2.0 ** -23
        bound = U_F32 * ref.abs() + (1 + U_F32) * (g * mag + (1 + g) * (eb @ T["W"].double().abs().t()))
        out["y"] = check_bound(f"{name} y", got["y"], ref, bound)[0]
    else:
        ref, mag = linear_ref(got["emb"] if r.temb else T["x"], T["W"], bias)
        out["y"] = check(f"{name} y", got["y"], ref, mag, r.K + 1, "f32")[0]
    if r.act:
        out["act"] = check_bound(f"{name} act_out", got["act"], *silu_ref(got["y"]))[0]
    return out


def check_bwd(r, T, got, name=None):
    """got = dict(slabs, dx) -> {output: largest err / bound}: the slabs against the fp64 partial sums, dx of a split row against
    silu_bwd_sum's reference on the slabs the launch stored"""
    from _bounds import check_bound, silu_bwd_sum_ref, skinny_bwd_ref
    name = name or bwd_id(r)
    pre = T["pre"] if r.pre else None
    if r.splits == 1:
        return dict(dx=check_bound(f"{name} dx", got["dx"], *skinny_bwd_ref(T["dy"], T["W"], 1, pre))[0])
    out = dict(slabs=check_bound(f"{name} slabs", got["slabs"], *skinny_bwd_ref(T["dy"], T["W"], r.splits))[0])
    out["dx"] = check_bound(f"{name} silu_bwd_sum", got["dx"], *silu_bwd_sum_ref(got["slabs"], pre))[0]
    return out
