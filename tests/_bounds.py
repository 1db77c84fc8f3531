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
"""
import torch
import torch.nn.functional as F

U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -24
SPLIT_PRODUCT = 2.0 ** -15
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


def check(name, y, ref, mag, k_terms, store, split=False, rows=None):
    """Per-element hard bound and tensor rel-L2 of output `y` (any device, any float dtype) against the fp64 `ref` / `mag`
    (same shape as y, or as y[rows] when `rows` selects a subset of the leading dimension).  NaN / Inf anywhere in y fails.
    Returns (largest err / bound, rel-L2)."""
    y64 = y.detach().cpu().double()
    if not bool(torch.isfinite(y64).all()):
        bad = (~torch.isfinite(y64)).nonzero()[:4].tolist()
        raise AssertionError(f"{name}: non-finite output at {bad} ({int((~torch.isfinite(y64)).sum())} elements)")
    if rows is not None:
        y64 = y64[rows]
    ref, mag = ref.double(), mag.double()
    assert y64.shape == ref.shape == mag.shape, (name, y64.shape, ref.shape, mag.shape)
    u = U_BF16 if store == "bf16" else U_F32
    gamma = (k_terms + 8) * 2.0 ** -23 + (SPLIT_PRODUCT if split else 0.0)
    bound = u * ref.abs() + (1 + u) * gamma * mag
    err = (y64 - ref).abs()
    over = err > bound
    if bool(over.any()):
        idx = over.nonzero()[:4].tolist()
        ex = [(i, float(y64[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx]
        raise AssertionError(f"{name}: {int(over.sum())} elements outside the bound, e.g. (index, y, ref, bound) {ex}")
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    rel = float((y64 - ref).norm() / (ref.norm() + 1e-300))
    return ratio, rel


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
