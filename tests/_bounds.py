"""Error bounds for the contraction kernels (csrc/gemm.hip) against an fp64 reference of the same operation.

The reference is computed in fp64 from the exact stored operand values (bf16 upcasts exactly), epilogue included: alpha,
bias, rowvec (row pitch rv_ld, image = row // rows_per_img), resid and, where the destination accumulates, its prior value.
`mag` is the same computation on absolute values.  Per element, a correct kernel satisfies

    |y - ref| <= u_out |ref| + (1 + u_out) gamma mag,    gamma = (K_terms + 8) 2^-23  (+ 2^-15 on split-product routes)

u_out = 2^-8 for a bf16 store, 2^-24 for fp32: fp32 accumulation in any order (split-K, atomics, faithfully rounded adds),
then one rounding of the store.  The split-product routes multiply hi / lo bf16 pairs, ~2^-16 relative per product
(include/mdm_hip.h, B_split).  The bound does not depend on the data, so it never fails on a correct kernel; a missing tap,
K-chunk, row, image or epilogue term moves an element by about mag / K_terms or more and fails it.

Every output and input lives inside guard bands of a fixed NaN bit pattern (`Buf`): a write past either end changes the
bands, a read past either end that reaches a result turns it into NaN.

Attention (csrc/attn.hip) and the row softmax (csrc/norm.hip)
--------------------------------------------------------------
o = softmax(q k^T scale) v over L keys, head width C.  All references are fp64 functions of exactly the stored inputs.  With

    g  = (C + 8) 2^-23       fp32 accumulation of the C products of one score (or of dO . v, dO . o), any order
    gL = (L + 8) 2^-23       fp32 accumulation over the L keys (or queries) of a second product
    u  = 2^-8 | 2^-24        one rounding of a bf16 | fp32 store
    eps = 2^-20              the fast exponential: v_exp_f32 is good to 2^-23 relative, its argument x log2(e) and the result's
                             use carry two more roundings; 8x head room.  The rounding of the argument itself, 2^-24 |s - m|, is
                             below g smag because |s| <= smag and g >= 40 * 2^-23
    smag_ij = scale sum_d |q_id| |k_jd|

forward.  The computed score is s_ij + d_ij with |d_ij| <= g smag_ij, so exp(.) of it is off by that much RELATIVELY, in the
numerator term j and -- at most max_j of it -- in the denominator: 2 (g max_j smag_ij + eps).  The bf16 kernels round the
unnormalised p_ij once to bf16 before the second product (2^-8 relative per term: bf16 keeps 8 significant bits, so round to
nearest is off by up to 2^-8 of the value -- 2^-9 is only the mean, and an output element that one probability near 1 dominates,
as the peaked draws make them, attains the worst case: with 2^-9 the CPU emulation of a correct kernel left the dv bound); the sums over keys add gL (numerator: L
roundings of half an ulp; denominator: 16 per lane, two shuffles and one add per 64-key tile; each rescale of a tile step
multiplies numerator and denominator by the same alpha).  Hence, per query row i,

    eta_i = [2^-8] + 2 (g max_j smag_ij + eps) + gL,        |o - P v| <= u |P v| + (1 + u) eta_i (P |v|)
    |lse - logsumexp(s)| <= g max_j smag_ij + eps + gL + 2^-23 |lse|

([..]: kernels that round P to bf16 only.)  attn_mh_kernel rescales at every KEY, not every tile: numerator and denominator each
take two roundings per key (2 gL in all for o), and every rise of the running max multiplies what was summed so far by a fresh
fast exponential, so eps counts once per rise of the row's running max in key order (`rises_i`, from the fp64 scores, + 1).
The probabilities attn_f32_small leaves behind: |S_ij - P_ij| <= u P_ij + (1 + u) (g (smag_ij + max_j smag_ij) + 2 eps + gL) P_ij.

backward, as a function of its five inputs (qkv, o, dO, lse, scale) -- the o and lse handed to the kernel are the quantities
of the reference, whatever produced them: P = exp(s - lse), delta = sum_d dO o, dP = dO v^T, dS = P (dP - delta) scale, and
mdS = P (|dO| |v|^T + sum_d |dO| |o|) scale.

    ep_ij = g smag_ij + eps + 2^-23 |lse_i|                         relative error of the recomputed P_ij
    eS_ij = ([2^-8] + ep_ij + g + 2^-22) mdS_ij                     dS: its bf16 rounding, P, the two C-term sums, three roundings
    eP_ij = ([2^-8] + ep_ij) P_ij
    dq: (1 + gL) eS |k| + gL mdS |k|      dk: the same with eS^T, mdS^T, |q|      dv: (1 + gL) eP^T |dO| + gL P^T |dO|
    each wrapped as u |ref| + (1 + u) (...);          |delta - sum dO o| <= g sum |dO| |o|

row softmax in place: |y - P| <= u P + (1 + u) (2^-23 |x_ij - max_i| + 2 eps + gL) P (no score error: the inputs are exact; the
argument's rounding is kept because a single probability, unlike a weighted sum of them, has nothing to hide it in); backward
ref = P (g - sum P g), mag = P (|g| + sum P |g|), eta = gL + 2^-22.

A CPU emulation of the fused kernels' arithmetic (fp32 scores, 64-key online softmax, P and dS rounded to bf16, fp32 second
product, bf16 store; tests/test_bounds_cpu.py) stays inside these bounds, and each planted fault there leaves them.  The bounds
are derived, never fitted to what a GPU returned.

rel-L2 bar of the bf16 outputs: `attn_emulate_bf16` is the storage precision alone -- fp64 arithmetic with exactly the bf16
roundings above.  A kernel's rel-L2 against fp64 may be at most REL_L2_MARGIN = 1.5 times the emulation's on the same inputs:
the emulation does not depend on the tile order, while truncating P or the output instead of rounding lands at 1.7 - 2.0 times.
"""
import torch
import torch.nn.functional as F

U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -24
SPLIT_PRODUCT = 2.0 ** -15
EPS_EXP = 2.0 ** -20          # fast exponential (module docstring)
REL_L2_MARGIN = 1.5           # kernel rel-L2 <= this x the rel-L2 of the storage-precision emulation
# guard pattern: a quiet NaN with a payload no kernel produces
_PAT = {torch.float32: (torch.int32, 0x7FC0A5A5), torch.bfloat16: (torch.int16, 0x7FE5)}


class Buf:
    """A tensor `.t` of `shape` inside [guard | data | guard] of one allocation.  Guards hold the NaN pattern and are at least
    `min_guard_rows` rows of `row` elements and at least 64 KiB.  fill: "nan" (the pattern), or a tensor of values."""

    def __init__(self, shape, dtype, device, fill="nan", row=None, min_guard_rows=256):
        self.shape, self.dtype = tuple(shape), dtype
        n = 1
        for s in self.shape:
            n *= s
        row = row if row is not None else (self.shape[-1] if len(self.shape) > 1 else 1)
        esz = torch.finfo(dtype).bits // 8
        self.g = max(min_guard_rows * row, 65536 // esz)
        self.n = n
        self.raw = torch.empty(2 * self.g + n, dtype=dtype, device=device)
        ity, pat = _PAT[dtype]
        self.ity, self.pat = ity, pat
        self.raw.view(ity).fill_(pat)
        self.t = self.raw[self.g:self.g + n].view(self.shape)
        if not isinstance(fill, str):
            self.t.copy_(fill.to(dtype).reshape(self.shape))

    def guards_intact(self):
        iv = self.raw.view(self.ity)
        return bool((iv[:self.g] == self.pat).all()) and bool((iv[self.g + self.n:] == self.pat).all())

    def first_bad_guard(self):
        iv = self.raw.view(self.ity).cpu()
        lo = (iv[:self.g] != self.pat).nonzero()
        hi = (iv[self.g + self.n:] != self.pat).nonzero()
        return (int(lo[-1]) - self.g if len(lo) else None, int(hi[0]) + self.n if len(hi) else None)


def rne_bf16(x64):
    """fp64 -> bf16 with round-to-nearest-even through fp32 (fp32 first is exact enough: the fp32 rounding is far below a bf16 ulp
    except at exact ties, which random data does not hit)."""
    return x64.float().to(torch.bfloat16)


def trunc_bf16(x64):
    """fp64 -> bf16 by dropping the low 16 bits of the fp32 value (round toward zero): a planted fault."""
    i = x64.float().view(torch.int32) & ~0xFFFF
    return i.view(torch.float32).to(torch.bfloat16)


def _finite64(name, y):
    y64 = y.detach().cpu().double()
    if not bool(torch.isfinite(y64).all()):
        bad = (~torch.isfinite(y64)).nonzero()[:4].tolist()
        raise AssertionError(f"{name}: non-finite output at {bad} ({int((~torch.isfinite(y64)).sum())} elements)")
    return y64


def violations(y, ref, bound):
    """Boolean mask of the elements of `y` outside |y - ref| <= bound (non-finite elements count as outside)."""
    y64 = y.detach().cpu().double()
    return ~((y64 - ref.double()).abs() <= bound.double())


def check_bound(name, y, ref, bound, rows=None):
    """`check` with a precomputed per-element `bound` tensor (same shape as ref): NaN / Inf anywhere in y fails, then every
    element of y (or y[rows]) must satisfy |y - ref| <= bound.  Returns (largest err / bound, rel-L2)."""
    y64 = _finite64(name, y)
    if rows is not None:
        y64 = y64[rows]
    ref, bound = ref.double(), bound.double()
    assert y64.shape == ref.shape == bound.shape, (name, y64.shape, ref.shape, bound.shape)
    err = (y64 - ref).abs()
    over = err > bound
    if bool(over.any()):
        idx = over.nonzero()[:4].tolist()
        ex = [(i, float(y64[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx]
        raise AssertionError(f"{name}: {int(over.sum())} elements outside the bound, e.g. (index, y, ref, bound) {ex}")
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    rel = float((y64 - ref).norm() / (ref.norm() + 1e-300))
    return ratio, rel


def check(name, y, ref, mag, k_terms, store, split=False, rows=None):
    """Per-element hard bound and tensor rel-L2 of output `y` (any device, any float dtype) against the fp64 `ref` / `mag`
    (same shape as y, or as y[rows] when `rows` selects a subset of the leading dimension).  NaN / Inf anywhere in y fails.
    Returns (largest err / bound, rel-L2)."""
    ref, mag = ref.double(), mag.double()
    assert ref.shape == mag.shape, (name, ref.shape, mag.shape)
    u = U_BF16 if store == "bf16" else U_F32
    gamma = (k_terms + 8) * 2.0 ** -23 + (SPLIT_PRODUCT if split else 0.0)
    return check_bound(name, y, ref, u * ref.abs() + (1 + u) * gamma * mag, rows=rows)


# ------------------------------------------------------------------ fp64 references (CPU)
def _nchw(x):
    return x.double().cpu().permute(0, 3, 1, 2)


def _w4(wt, KH, KW):
    """w[tap][Cout][Cin] -> [Cout][Cin][KH][KW]"""
    T, Co, Ci = wt.shape
    return wt.double().cpu().reshape(KH, KW, Co, Ci).permute(2, 3, 0, 1)


def _conv(xv, w4, pads, stride):
    pt, pl, pb, pr = pads
    return F.conv2d(F.pad(xv, (pl, pr, pt, pb)), w4, stride=stride)


def conv_fwd_ref(x0, x1, wt, KH, KW, stride, pads, ups, imgs=None):
    """(acc, mag) of the convolution only, [n][OH][OW][Cout] fp64; x0/x1 NHWC (x1 may be None), imgs = subset of images."""
    xs = [x0] + ([x1] if x1 is not None else [])
    x = torch.cat([_nchw(t if imgs is None else t[imgs]) for t in xs], 1)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    w4 = _w4(wt, KH, KW)
    acc = _conv(x, w4, pads, stride)
    mag = _conv(x.abs(), w4.abs(), pads, stride)
    return acc.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def conv_dgrad_ref(dy, wt, VH, VW, C, KH, KW, stride, pads, imgs=None):
    """(acc, mag) of the data gradient on the (virtual) input map [n][VH][VW][C]; dy NHWC, wt[tap][Cout][Cin]."""
    dyv = _nchw(dy if imgs is None else dy[imgs])
    w4 = _w4(wt, KH, KW)

    def vjp(g, w):
        x = torch.zeros(g.shape[0], C, VH, VW, dtype=torch.float64, requires_grad=True)
        out = _conv(x, w, pads, stride)
        return torch.autograd.grad(out, x, g)[0]
    return vjp(dyv, w4).permute(0, 2, 3, 1), vjp(dyv.abs(), w4.abs()).permute(0, 2, 3, 1)


def conv_wgrad_ref(dy, x0, x1, KH, KW, stride, pads, ups):
    """(acc, mag) of the weight gradient [tap][Cout][Cin] fp64 over all images, and the bias gradient (sum, sum|.|) [Cout]."""
    xs = [x0] + ([x1] if x1 is not None else [])
    x = torch.cat([_nchw(t) for t in xs], 1)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    dyv = _nchw(dy)
    Co, Ci = dyv.shape[1], x.shape[1]

    def vjp(g, xx):
        w = torch.zeros(Co, Ci, KH, KW, dtype=torch.float64, requires_grad=True)
        out = _conv(xx, w, pads, stride)
        return torch.autograd.grad(out, w, g)[0].permute(2, 3, 0, 1).reshape(KH * KW, Co, Ci)
    db = dyv.sum((0, 2, 3)), dyv.abs().sum((0, 2, 3))
    return vjp(dyv, x), vjp(dyv.abs(), x.abs()), db


def epilogue_ref(acc, mag, alpha=1.0, bias=None, rowvec=None, rv_ld=0, rv_off=0, rows_per_img=1, resid=None, prior=None,
                 img0=None):
    """acc / mag [M][N] fp64 -> (ref, mag) of the stored value: alpha acc + bias[n] + rowvec[rv_off + img * rv_ld + n] + resid + prior.
    img0: image index of each row block when the rows are a subset (default: row // rows_per_img)."""
    M, N = acc.shape
    ref, mg = alpha * acc, abs(alpha) * mag
    if bias is not None:
        b = bias.double().cpu()[:N]
        ref, mg = ref + b, mg + b.abs()
    if rowvec is not None:
        img = (torch.arange(M) // rows_per_img) if img0 is None else img0
        rv = rowvec.double().cpu().reshape(-1)
        idx = rv_off + img[:, None] * rv_ld + torch.arange(N)[None, :]
        r = rv[idx]
        ref, mg = ref + r, mg + r.abs()
    for extra in (resid, prior):
        if extra is not None:
            e = extra.double().cpu().reshape(M, N)
            ref, mg = ref + e, mg + e.abs()
    return ref, mg


# ------------------------------------------------------------------ attention and row softmax (module docstring)
def _u(store):
    return U_BF16 if store == "bf16" else U_F32


def _wrap(ref, m, u):
    return ref, u * ref.abs() + (1 + u) * m


def attn_fwd_ref(q, k, v, scale, store, p_bf16, per_key=False, want_P=False, chunk=1024):
    """q, k, v [B][L][D] (any float dtype: the stored values) -> dict of (ref, bound) pairs "o" [B][L][D], "lse" [B][L] and, with
    want_P, "P" [B][L][L].  store: "bf16" | "f32" of o (and P); p_bf16: the kernel rounds P to bf16 before the second product;
    per_key: it rescales at every key (attn_mh_kernel).  Queries are walked in chunks to bound the memory."""
    q, k, v = (t.detach().cpu().double() for t in (q, k, v))
    B, L, D = q.shape
    u, g, gL = _u(store), (D + 8) * 2.0 ** -23, (L + 8) * 2.0 ** -23
    o, ob, ls, lb, Ps, Pb = [], [], [], [], [], []
    for i0 in range(0, L, chunk):
        qs = q[:, i0:i0 + chunk]
        s = qs @ k.transpose(1, 2) * scale
        smag = qs.abs() @ k.abs().transpose(1, 2) * abs(scale)
        smax = smag.max(-1).values
        lse = torch.logsumexp(s, -1)
        P = torch.exp(s - lse[..., None])
        eps = torch.full_like(lse, EPS_EXP)
        if per_key:
            eps = eps * (1 + (s[..., 1:] > s.cummax(-1).values[..., :-1]).sum(-1) + 1)
        sums = (2 if per_key else 1) * gL
        eta = (U_BF16 if p_bf16 else 0.0) + 2 * (g * smax + eps) + sums
        r, b = _wrap(P @ v, eta[..., None] * (P @ v.abs()), u)
        o.append(r); ob.append(b)
        ls.append(lse); lb.append(g * smax + eps + gL + 2.0 ** -23 * lse.abs())
        if want_P:
            r, b = _wrap(P, (g * (smag + smax[..., None]) + 2 * eps[..., None] + gL) * P, u)
            Ps.append(r); Pb.append(b)
    out = {"o": (torch.cat(o, 1), torch.cat(ob, 1)), "lse": (torch.cat(ls, 1), torch.cat(lb, 1))}
    if want_P:
        out["P"] = (torch.cat(Ps, 1), torch.cat(Pb, 1))
    return out


def attn_bwd_ref(q, k, v, o, do, lse, scale, store, round_bf16, chunk=1024):
    """The backward as a function of its inputs (q, k, v, o, dO [B][L][D], lse [B][L], as stored) -> dict of (ref, bound) pairs
    "dq", "dk", "dv" [B][L][D] and "delta" [B][L].  round_bf16: the kernel rounds P and dS to bf16 before the second products."""
    q, k, v, o, do, lse = (t.detach().cpu().double() for t in (q, k, v, o, do, lse))
    B, L, D = q.shape
    u, g, gL = _u(store), (D + 8) * 2.0 ** -23, (L + 8) * 2.0 ** -23
    r9 = U_BF16 if round_bf16 else 0.0
    delta, dmag = (do * o).sum(-1), (do.abs() * o.abs()).sum(-1)
    z = lambda: torch.zeros(B, L, D, dtype=torch.float64)
    dq, dqm, dk, dkm, dv, dvm = [], [], z(), z(), z(), z()
    ka, va = k.abs(), v.abs()
    for i0 in range(0, L, chunk):
        sl = slice(i0, i0 + chunk)
        qs, gs = q[:, sl], do[:, sl]
        s = qs @ k.transpose(1, 2) * scale
        smag = qs.abs() @ ka.transpose(1, 2) * abs(scale)
        P = torch.exp(s - lse[:, sl, None])
        dS = P * (gs @ v.transpose(1, 2) - delta[:, sl, None]) * scale
        mdS = P * (gs.abs() @ va.transpose(1, 2) + dmag[:, sl, None]) * abs(scale)
        ep = g * smag + EPS_EXP + 2.0 ** -23 * lse[:, sl, None].abs()
        eS = (r9 + ep + g + 2.0 ** -22) * mdS
        eP = (r9 + ep) * P
        dq.append(dS @ k); dqm.append((1 + gL) * (eS @ ka) + gL * (mdS @ ka))
        dk += dS.transpose(1, 2) @ qs; dkm += (1 + gL) * (eS.transpose(1, 2) @ qs.abs()) + gL * (mdS.transpose(1, 2) @ qs.abs())
        dv += P.transpose(1, 2) @ gs; dvm += (1 + gL) * (eP.transpose(1, 2) @ gs.abs()) + gL * (P.transpose(1, 2) @ gs.abs())
    return {"dq": _wrap(torch.cat(dq, 1), torch.cat(dqm, 1), u), "dk": _wrap(dk, dkm, u), "dv": _wrap(dv, dvm, u),
            "delta": (delta, g * dmag)}


def attn_emulate_bf16(q, k, v, do, scale, o=None, lse=None, chunk=1024):
    """The storage precision of the fused bf16 kernels and nothing else: fp64 arithmetic with the unnormalised P rounded to bf16
    before P v, P and dS rounded to bf16 before the backward's second products, and every output rounded to bf16.  The backward
    (when `o` and `lse` are given) is the same function of (qkv, o, dO, lse) as attn_bwd_ref.  -> dict of fp64 tensors."""
    r = lambda x: rne_bf16(x).double()
    q, k, v, do = (t.detach().cpu().double() for t in (q, k, v, do))
    B, L, D = q.shape
    out = {}
    oo = []
    bwd = o is not None
    if bwd:
        o, lse = o.detach().cpu().double(), lse.detach().cpu().double()
        delta = (do * o).sum(-1)
        dq, dk, dv = [], torch.zeros_like(q), torch.zeros_like(q)
    for i0 in range(0, L, chunk):
        sl = slice(i0, i0 + chunk)
        s = q[:, sl] @ k.transpose(1, 2) * scale
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        oo.append(r((r(p) @ v) / p.sum(-1, keepdim=True)))
        if bwd:
            P = torch.exp(s - lse[:, sl, None])
            dS = r(P * (do[:, sl] @ v.transpose(1, 2) - delta[:, sl, None]) * scale)
            dq.append(r(dS @ k))
            dk += dS.transpose(1, 2) @ q[:, sl]
            dv += r(P).transpose(1, 2) @ do[:, sl]
    out["o"] = torch.cat(oo, 1)
    if bwd:
        out.update(dq=torch.cat(dq, 1), dk=r(dk), dv=r(dv))
    return out


def softmax_fwd_ref(x, store):
    """x [rows][L] as stored -> (P, bound) of the in-place row softmax."""
    x = x.detach().cpu().double()
    L = x.shape[-1]
    mx = x.max(-1, keepdim=True).values
    P = torch.softmax(x, -1)
    eta = 2.0 ** -23 * (x - mx).abs() + 2 * EPS_EXP + (L + 8) * 2.0 ** -23
    return _wrap(P, eta * P, _u(store))


def softmax_bwd_ref(P, g, store):
    """P, g [rows][L] as stored -> (ref, bound) of dS = P (g - sum_j P g) written over g."""
    P, g = P.detach().cpu().double(), g.detach().cpu().double()
    L = P.shape[-1]
    ref = P * (g - (P * g).sum(-1, keepdim=True))
    mag = P.abs() * (g.abs() + (P.abs() * g.abs()).sum(-1, keepdim=True))
    return _wrap(ref, ((L + 8) * 2.0 ** -23 + 2.0 ** -22) * mag, _u(store))


def attn_draw(N, L, C, kind, seed):
    """Inputs of the fused-attention tests, pre-rounded to bf16: qkv [N][L][3C], dO [N][L][C] ~ N(0, 1).
    "flat": q, k ~ N(0, 1), every key carries weight.  "peaked": amplitude 1.5, key L - 3 of image 0 scaled x6 and key L / 2 x4:
    the running max rises in the last and in a middle key tile while the accumulator is non-zero.  v gets +0.5 on both, so that
    a missing or doubled key moves the output."""
    g = torch.Generator().manual_seed(seed)
    amp = {"flat": 1.0, "peaked": 1.5}[kind]
    qkv = torch.randn(N, L, 3 * C, generator=g) * amp
    qkv[..., 2 * C:] += 0.5
    qkv = qkv.to(torch.bfloat16).float()
    if kind == "peaked":
        qkv[0, L - 3, C:2 * C] *= 6.0
        qkv[0, L // 2, C:2 * C] *= 4.0
    do = torch.randn(N, L, C, generator=g)
    return qkv.to(torch.bfloat16), do.to(torch.bfloat16)


def attn_fused_refs(qkv, do, scale, emulate=True):
    """Everything a test of the fused bf16 kernels compares with: the forward's (ref, bound) pairs, the o (fp64 -> bf16) and lse
    (fp64 -> fp32) the backward is GIVEN, the backward's pairs as a function of those, and the storage-precision emulation."""
    C = do.shape[-1]
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    R = attn_fwd_ref(q, k, v, scale, "bf16", p_bf16=True)
    R["o_in"], R["lse_in"] = rne_bf16(R["o"][0]), R["lse"][0].float()
    R.update(attn_bwd_ref(q, k, v, R["o_in"], do, R["lse_in"], scale, "bf16", round_bf16=True))
    if emulate:
        R["emu"] = attn_emulate_bf16(q, k, v, do, scale, R["o_in"], R["lse_in"])
    return R
