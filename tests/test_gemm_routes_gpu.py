"""Route-complete fp64 parity of the contraction kernels (csrc/gemm.hip).

Every row of CASES names the kernel route it expects (mdm_gemm_last_route) and one entry point; the test checks the route,
then every output against an fp64 reference with the per-element bound and the tensor rel-L2 bar of tests/_bounds.py.
Outputs and inputs sit inside NaN guard bands; overwrite destinations start as NaN, accumulating ones as random finite
values, workspaces as NaN.  The coverage test fails when a route of the library is reached by no row (a new kernel, or a
dispatch rule that moved every row away from one), the determinism test when a route without float atomics is not
bit-reproducible."""
import os

import pytest
import torch

from _bounds import Buf, check, conv_dgrad_ref, conv_fwd_ref, conv_wgrad_ref, epilogue_ref
from _notes import note

pytestmark = pytest.mark.gpu

BF, FP = 1, 0
# Tensor rel-L2 bars against fp64, per output kind, at <= 4x the largest value measured over CASES on an MI355X:
# bf16 store 1.70e-3 (lin2_64_1x1_Co40_N3) | fp32 from bf16 products 2.6e-7 (wgrad_lin128) | exact fp32 5.7e-7
# (halo_f32_64_8x8_N100) | fp32 with split (hi / lo bf16) products 4.6e-6 (halo_split64x32_4x4)
REL_BAR = {"bf16": 6.5e-3, "f32_bf16": 1e-6, "f32": 2e-6, "f32_split": 1.8e-5}

# Routes no row reaches, with the reason.
EXCLUDED = {
    # conv_variant takes the 64-channel small-map tile only for a fused GroupNorm epilogue of 64 channels per group (gnb_/gnf_)
    "halo<64,2,3,64>": "only with a fused GroupNorm epilogue of 64-channel groups (values, route and guard bands: tests/test_gn_bounds_gpu.py test_fused_backward_bounds / test_fused_forward_bounds)",
    "halo<64,3,3,64>": "only with a fused GroupNorm epilogue of 64-channel groups (values, route and guard bands: tests/test_gn_bounds_gpu.py test_fused_backward_bounds / test_fused_forward_bounds)",
}
# Float atomics: only the bias gradient (`dbias`) of the bf16 layout-2 kernels sums with atomicAdd (csrc/gemm.hip:
# `if (m < d.M) atomicAdd(&d.dbias[m], accb[i][0]);` in gemm_ring_kernel and wgrad_lin_kernel, and the per-wave
# atomicAdd(&d.dbias[...]) of wgrad_taps_body).  So the dbias rows (wgrad_lin<128>+splitk, wgrad_lin<64>, ring<64>) are
# not in the determinism test; every other row, every fp32 route included, must repeat its bits.


def _dt(dt):
    return torch.bfloat16 if dt == BF else torch.float32


class Case:
    def __init__(self, cid, route, kind, **p):
        self.id, self.route, self.kind, self.p = cid, route, kind, p

    def __repr__(self):
        return self.id


def C(cid, route, kind, **p):
    return pytest.param(Case(cid, route, kind, **p), id=cid)


def _geom(p):
    from mdm import ops
    k, s = p.get("k", 3), p.get("s", 1)
    pads = (1, 1, 1, 1) if k == 3 and s == 1 else (0, 0, 1, 1) if k == 3 else (0, 0, 0, 0)
    H = p["H"]
    return ops.ConvGeom(N=p["N"], IH=H, IW=H, C0=p["C0"], C1=p.get("C1", 0), Cout=p["Co"], KH=k, KW=k, stride=s,
                        pad_t=pads[0], pad_l=pads[1], pad_b=pads[2], pad_r=pads[3], ups=p.get("ups", 0)), pads


def _imgs(N, sub):
    """Images the forward / data-gradient reference checks: all, or first, second, middle, last two."""
    if not sub or N <= 6:
        return None
    return sorted({0, 1, N // 2, N - 2, N - 1})


def _split_shadow(w, dev):
    from mdm import _lib
    ws = torch.empty_like(w)
    segs = torch.tensor([0, w.numel()], dtype=torch.int64, device=dev)
    _lib.call("mdm_split_shadow", w.data_ptr(), ws.data_ptr(), segs.data_ptr(), 1, _lib.stream())
    return ws, segs


class Prob:
    """One call: descriptor fields, guarded buffers, and the checks to run after it."""

    def __init__(self, dev):
        self.dev, self.bufs, self.outs, self.keep = dev, [], [], []

    def buf(self, shape, dtype, fill="nan", row=None):
        b = Buf(shape, dtype, self.dev, fill, row)
        self.bufs.append(b)
        return b

    def out(self, name, b, ref_fn, k_terms, store, split=False, rows=None):
        self.outs.append((name, b, ref_fn, k_terms, store, split, rows))


def _rand(g, shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def build_conv_fwd(P, p, g):
    from mdm import ops
    dt = p.get("dt", BF)
    geom, pads = _geom(p)
    N, C0, C1, Co = geom.N, geom.C0, geom.C1, geom.Cout
    T = _dt(dt)
    x0 = _rand(g, (N, geom.IH, geom.IW, C0)).to(T)
    x1 = _rand(g, (N, geom.IH, geom.IW, C1)).to(T) if C1 else None
    wt = (_rand(g, (geom.taps, Co, geom.Cin)) / (geom.taps * geom.Cin) ** 0.5).to(T)
    s0 = P.buf(x0.shape, T, x0)
    s1 = P.buf(x1.shape, T, x1) if C1 else None
    wb = P.buf(wt.shape, T, wt)
    bias = _rand(g, (Co,)) if p.get("bias") else None
    bb = P.buf((Co,), torch.float32, bias) if bias is not None else None
    rv_ld = rv_off = 0
    rvb = None
    if p.get("rowvec"):
        rv_ld, rv_off = Co + 24, 8
        rv = _rand(g, (N * rv_ld + rv_off,))
        rvb = P.buf(rv.shape, torch.float32, rv)
    out_f32 = p.get("out_f32", 0) or dt == FP
    OT = torch.float32 if out_f32 else T
    resid = _rand(g, (N, geom.OH, geom.OW, Co)).to(T) if p.get("resid") else None
    rb = P.buf(resid.shape, T, resid) if resid is not None else None
    ob = P.buf((N, geom.OH, geom.OW, Co), OT, row=Co)
    ws = P.buf((p["ws"],), torch.float32) if p.get("ws") else None
    w_split = None
    if p.get("B_split"):
        w_split, segs = _split_shadow(wb.t, P.dev)
        P.keep += [w_split, segs]
    f = ops.conv_fwd_fields(dt, geom, s0.t, s1.t if s1 else None, wb.t, bb.t if bb else None, ob.t,
                            rowvec=rvb.t[rv_off:] if rvb else None, rv_ld=rv_ld, resid=rb.t if rb else None,
                            out_f32=int(bool(p.get("out_f32", 0))), ws=ws.t if ws else None, w_split=w_split,
                            f32_split=p.get("f32_split", 0))
    f.pop("_flops")
    imgs = _imgs(N, p.get("sub"))
    P_img = geom.OH * geom.OW

    def ref():
        acc, mag = conv_fwd_ref(x0, x1, wt, geom.KH, geom.KW, geom.stride, pads, geom.ups, imgs)
        img_ids = torch.arange(N) if imgs is None else torch.tensor(imgs)
        img_rows = img_ids.repeat_interleave(P_img)
        rs = resid[img_ids].reshape(-1, Co) if resid is not None else None
        return epilogue_ref(acc.reshape(-1, Co), mag.reshape(-1, Co), bias=bias, rowvec=rvb.t.cpu() if rvb else None,
                            rv_ld=rv_ld, rv_off=rv_off, resid=rs, img0=img_rows)
    store = "f32_split" if p.get("B_split") or p.get("f32_split") else ("f32" if dt == FP else ("f32_bf16" if out_f32 else "bf16"))
    P.out("y", ob, ref, geom.taps * geom.Cin, store, split=store == "f32_split",
          rows=None if imgs is None else imgs)
    return f


def build_conv_dgrad(P, p, g, transposed_w=True):
    from mdm import ops
    dt = p.get("dt", BF)
    geom, pads = _geom(p)
    N, C0, C1, Co = geom.N, geom.C0, geom.C1, geom.Cout
    T = _dt(dt)
    dy = _rand(g, (N, geom.OH, geom.OW, Co)).to(T)
    wt = (_rand(g, (geom.taps, Co, geom.Cin)) / (geom.taps * Co) ** 0.5).to(T)
    dyb = P.buf(dy.shape, T, dy)
    wsrc = wt.permute(0, 2, 1).contiguous() if transposed_w else wt
    wb = P.buf(wsrc.shape, T, wsrc)
    acc0, acc1 = p.get("acc0", 0), p.get("acc1", 0)
    VH, VW = geom.VH, geom.VW
    pr0 = _rand(g, (N, VH, VW, C0)).to(T) if acc0 else None
    pr1 = _rand(g, (N, VH, VW, C1)).to(T) if (acc1 and C1) else None
    d0 = P.buf((N, VH, VW, C0), T, pr0 if acc0 else "nan", row=C0)
    d1 = P.buf((N, VH, VW, C1), T, pr1 if pr1 is not None else "nan", row=C1) if C1 else None
    ws = P.buf((p["ws"],), torch.float32) if p.get("ws") else None
    if transposed_w:
        f = ops.conv_dgrad_t_fields(dt, geom, dyb.t, wb.t, d0.t, acc0, d1.t if d1 else None, acc1, ws=ws.t if ws else None)
    else:
        f = dict(dtype=dt, layout=1, M=N * VH * VW, N=geom.Cin, K=geom.taps * Co, conv=1, OH=VH, OW=VW, IH=geom.OH, IW=geom.OW,
                 KH=geom.KH, KW=geom.KW, stride=geom.stride, pad_t=geom.pad_t, pad_l=geom.pad_l, transposed=1, ups=0, C0=Co, C1=0,
                 Ck=Co, src0=dyb.t, ld0=Co, B=wb.t, ldb=geom.Cin, wtap=Co * geom.Cin, D0=d0.t, ldd0=C0, D1=d1.t if d1 else None,
                 ldd1=C1, N0=C0, acc0=acc0, acc1=acc1, ws=ws.t if ws else None, ws_bytes=ws.t.numel() * 4 if ws else 0)
    f.pop("_flops", None)
    imgs = _imgs(N, p.get("sub"))
    cache = {}

    def full():
        if "r" not in cache:
            cache["r"] = conv_dgrad_ref(dy, wt, VH, VW, geom.Cin, geom.KH, geom.KW, geom.stride, pads, imgs)
        return cache["r"]
    sel = (lambda t: t) if imgs is None else (lambda t: t[imgs])

    def ref0():
        a, m = full()
        return epilogue_ref(a[..., :C0].reshape(-1, C0), m[..., :C0].reshape(-1, C0), prior=sel(pr0) if pr0 is not None else None)

    def ref1():
        a, m = full()
        return epilogue_ref(a[..., C0:].reshape(-1, C1), m[..., C0:].reshape(-1, C1), prior=sel(pr1) if pr1 is not None else None)
    store = "f32" if dt == FP else "bf16"
    P.out("d0", d0, ref0, geom.taps * Co, store, rows=imgs)
    if C1:
        P.out("d1", d1, ref1, geom.taps * Co, store, rows=imgs)
    return f


def build_conv_wgrad(P, p, g):
    from mdm import ops
    dt = p.get("dt", BF)
    geom, pads = _geom(p)
    N, C0, C1, Co = geom.N, geom.C0, geom.C1, geom.Cout
    T = _dt(dt)
    dy = _rand(g, (N, geom.OH, geom.OW, Co)).to(T)
    x0 = _rand(g, (N, geom.IH, geom.IW, C0)).to(T)
    x1 = _rand(g, (N, geom.IH, geom.IW, C1)).to(T) if C1 else None
    dyb, s0 = P.buf(dy.shape, T, dy), P.buf(x0.shape, T, x0)
    s1 = P.buf(x1.shape, T, x1) if C1 else None
    acc = p.get("acc", 0)
    prior = _rand(g, (geom.taps, Co, geom.Cin)) if acc else None
    dw = P.buf((geom.taps, Co, geom.Cin), torch.float32, prior if acc else "nan", row=Co * geom.Cin)
    dbp = _rand(g, (Co,)) if p.get("dbias") else None
    db = P.buf((Co,), torch.float32, dbp) if dbp is not None else None
    ws = P.buf((p["ws"],), torch.float32) if p.get("ws") else None
    f = ops.wgrad_fields(dt, geom, dyb.t, s0.t, s1.t if s1 else None, dw.t, splitk=p.get("splitk", 0), ws=ws.t if ws else None,
                         dbias=db.t if db else None, acc=acc)
    f.pop("_flops")
    cache = {}

    def full():
        if "r" not in cache:
            cache["r"] = conv_wgrad_ref(dy, x0, x1, geom.KH, geom.KW, geom.stride, pads, geom.ups)
        return cache["r"]

    def refw():
        a, m, _ = full()
        return epilogue_ref(a.reshape(-1, geom.Cin), m.reshape(-1, geom.Cin), prior=prior.reshape(-1, geom.Cin) if acc else None)

    def refb():
        _, _, (s, sa) = full()
        return s + dbp.double(), sa + dbp.double().abs()
    K = N * geom.OH * geom.OW
    store = "f32" if dt == FP else "f32_bf16"
    P.out("dw", dw, refw, K, store)
    if db is not None:
        P.out("dbias", db, refb, K, store)
    return f


def build_matmul(P, p, g):
    dt, L = p.get("dt", BF), p["layout"]
    M, N, K, B = p["M"], p["N"], p["K"], p.get("batch", 1)
    T = _dt(dt)
    a_shape = (B, M, K) if L in (0, 1) else (B, K, M)
    b_shape = (B, N, K) if L == 0 else (B, K, N)
    A = _rand(g, a_shape).to(T)
    Bm = (_rand(g, b_shape) / K ** 0.5).to(T)
    ab, bb = P.buf(A.shape, T, A), P.buf(Bm.shape, T, Bm)
    alpha = p.get("alpha", 1.0)
    bias = _rand(g, (N,)) if p.get("bias") else None
    biasb = P.buf((N,), torch.float32, bias) if bias is not None else None
    out_f32 = p.get("out_f32", 0) or dt == FP
    OT = torch.float32 if out_f32 else T
    acc = p.get("acc", 0)
    prior = _rand(g, (B, M, N)).to(OT) if acc else None
    D = P.buf((B, M, N), OT, prior if acc else "nan", row=N)
    ws = P.buf((p["ws"],), torch.float32) if p.get("ws") else None
    f = dict(dtype=dt, layout=L, M=M, N=N, K=K, batch=B, sA=A[0].numel(), sB=Bm[0].numel(), sD=M * N, A=ab.t, lda=a_shape[2],
             B=bb.t, ldb=b_shape[2], D0=D.t, ldd0=N, N0=N, alpha=alpha, bias=biasb.t if biasb else None, acc0=acc,
             out_f32=int(bool(p.get("out_f32", 0))), splitk=p.get("splitk", 1 if L != 2 else 0), f32_split=p.get("f32_split", 0),
             ws=ws.t if ws else None, ws_bytes=ws.t.numel() * 4 if ws else 0)

    def ref():
        a, b = A.double(), Bm.double()
        eq = {0: "bmk,bnk->bmn", 1: "bmk,bkn->bmn", 2: "bkm,bkn->bmn"}[L]
        r, m = torch.einsum(eq, a, b), torch.einsum(eq, a.abs(), b.abs())
        return epilogue_ref(r.reshape(-1, N), m.reshape(-1, N), alpha=alpha, bias=bias,
                            prior=prior.reshape(-1, N) if acc else None)
    store = "f32_split" if p.get("f32_split") else ("f32" if dt == FP else ("f32_bf16" if out_f32 else "bf16"))
    P.out("D", D, ref, K, store, split=store == "f32_split")
    return f


BUILD = {"fwd": build_conv_fwd, "dgrad_t": build_conv_dgrad, "dgrad": lambda P, p, g: build_conv_dgrad(P, p, g, False),
         "wgrad": build_conv_wgrad, "mm": build_matmul}


def launch(case, dev, seed=0):
    """Build and run one case; returns (route, Prob)."""
    from mdm import _lib
    g = torch.Generator().manual_seed(hash(case.id) & 0xffffff ^ seed)
    P = Prob(dev)
    kind, p = case.kind, case.p
    if kind == "pair":
        fa = BUILD["fwd"](P, p["a"], g)
        Pb = Prob(dev)
        fb = BUILD["fwd"](Pb, p["b"], g)
        P.bufs += Pb.bufs
        P.outs += [("b." + o[0],) + o[1:] for o in Pb.outs]
        P.keep += Pb.keep
        _lib.gemm_pair(fa, fb)
    elif kind == "group":
        fl = []
        for i, m in enumerate(p["members"]):
            Pm = Prob(dev)
            fl.append(BUILD["wgrad"](Pm, m, g))
            P.bufs += Pm.bufs
            P.outs += [(f"m{i}." + o[0],) + o[1:] for o in Pm.outs]
        old = os.environ.get("MDM_TAPS_MIN_SHARE")
        if p.get("min_share") is not None:
            os.environ["MDM_TAPS_MIN_SHARE"] = str(p["min_share"])
        try:
            grp = _lib.WgradGroup(fl, dev)
        finally:
            if old is None:
                os.environ.pop("MDM_TAPS_MIN_SHARE", None)
            else:
                os.environ["MDM_TAPS_MIN_SHARE"] = old
        P.keep.append(grp)
        grp.launch()
    else:
        f = BUILD[kind](P, p, g)
        _lib.gemm(**f)
    return _lib.last_route(), P


def verify(case, P):
    """Guards, then every output against its fp64 reference: -> [(output, ratio, rel-L2, store)]."""
    torch.cuda.synchronize()
    res = []
    for b in P.bufs:
        assert b.guards_intact(), f"{case.id}: guard band of a {tuple(b.shape)} buffer changed at {b.first_bad_guard()}"
    for name, b, ref_fn, k_terms, store, split, rows in P.outs:
        ref, mag = ref_fn()
        if rows is not None:        # no NaN / Inf anywhere; the bound on the images the reference covers
            assert bool(torch.isfinite(b.t.float()).all()), f"{case.id}.{name}: non-finite output"
        y = (b.t if rows is None else b.t[rows]).reshape(ref.shape)
        ratio, rel = check(f"{case.id}.{name}", y, ref, mag, k_terms, "bf16" if store == "bf16" else "f32", split=split)
        res.append((name, ratio, rel, store))
    return res


# ---------------------------------------------------------------------------------------------------------------- cases
F32_SUB = dict(dt=FP, sub=True)
CASES = [
    # fp32 linears
    C("skinny_f32_M25", "linear_skinny_f32", "mm", dt=FP, layout=0, M=25, N=64, K=256, alpha=0.5, bias=1),
    C("tn_skinny_f32", "tn_skinny_f32", "mm", dt=FP, layout=2, M=64, N=128, K=100),
    # fp32 split-product convolutions (sampler shapes: N = 100)
    C("lin_split128_1x1_N100", "lin_split<128>", "fwd", H=16, N=100, C0=128, Co=128, k=1, B_split=1, bias=1, rowvec=1, resid=1, **F32_SUB),
    C("lin_split64_s2_N5", "lin_split<64>", "fwd", H=8, N=5, C0=96, Co=64, k=3, s=2, B_split=1, bias=1, dt=FP),
    C("halo_split_smallN_N100", "halo<256,6,2,32,f32,split>", "fwd", H=32, N=100, C0=128, Co=8, B_split=1, bias=1, **F32_SUB),
    C("halo_split_bn128_N100", "halo<256,6,4,128,f32,split>", "fwd", H=16, N=100, C0=256, Co=256, B_split=1, bias=1, rowvec=1, **F32_SUB),
    C("halo_split_mixed_N80", "halo_mixed<256|128,f32,split>", "fwd", H=32, N=80, C0=64, Co=64, B_split=1, bias=1, **F32_SUB),
    C("halo_split256_N100", "halo<256,6,NSB,64,f32,split>", "fwd", H=32, N=100, C0=64, Co=64, B_split=1, resid=1, **F32_SUB),
    C("halo_split128_3", "halo<128,3,3,64,f32,split>", "fwd", H=16, N=4, C0=64, Co=64, B_split=1, bias=1, dt=FP),
    C("halo_split128_4", "halo<128,4,3,64,f32,split>", "fwd", H=32, N=2, C0=64, Co=64, B_split=1, dt=FP),
    C("halo_split128_6", "halo<128,6,3,64,f32,split>", "fwd", H=64, N=1, C0=32, Co=64, B_split=1, dt=FP),
    C("halo_split64x32_8x8", "halo<64,2,3,32,f32,split>", "fwd", H=8, N=4, C0=64, Co=64, B_split=1, rowvec=1, dt=FP),
    C("halo_split64x32_4x4", "halo<64,3,3,32,f32,split>", "fwd", H=4, N=4, C0=64, Co=64, B_split=1, dt=FP),
    C("halo_split64_8x8_N100", "halo<64,2,3,64,f32,split>", "fwd", H=8, N=100, C0=128, Co=128, B_split=1, bias=1, **F32_SUB),
    C("halo_split64_4x4_N100", "halo<64,3,3,64,f32,split>", "fwd", H=4, N=100, C0=64, Co=512, B_split=1, **F32_SUB),
    C("halo_split128_8x8_N100", "halo<128,4,3,64,f32,split>", "fwd", H=8, N=100, C0=128, Co=256, B_split=1, **F32_SUB),
    # exact fp32 convolutions
    C("halo_f32_256_N100", "halo<256,6,2,64,f32>", "fwd", H=32, N=100, C0=64, Co=64, bias=1, rowvec=1, resid=1, **F32_SUB),
    C("halo_f32_128_3", "halo<128,3,3,64,f32>", "fwd", H=16, N=4, C0=64, Co=64, dt=FP),
    C("halo_f32_128_4_dgrad", "halo<128,4,3,64,f32>", "dgrad_t", H=32, N=2, C0=64, Co=64, acc0=1, dt=FP),
    C("halo_f32_128_6", "halo<128,6,3,64,f32>", "fwd", H=64, N=1, C0=32, Co=64, dt=FP),
    C("halo_f32_64x32_8x8", "halo<64,2,3,32,f32>", "fwd", H=8, N=4, C0=64, Co=64, bias=1, dt=FP),
    C("halo_f32_64x32_4x4", "halo<64,3,3,32,f32>", "fwd", H=4, N=4, C0=64, Co=64, dt=FP),
    C("halo_f32_64_8x8_N100", "halo<64,2,3,64,f32>", "fwd", H=8, N=100, C0=128, Co=128, **F32_SUB),
    C("halo_f32_64_4x4_N100", "halo<64,3,3,64,f32>", "fwd", H=4, N=100, C0=64, Co=512, **F32_SUB),
    C("f32_mfma128_mm_L1", "f32_mfma<128>", "mm", dt=FP, layout=1, M=1024, N=1024, K=96, batch=4),
    C("f32_mfma128_split_1x1", "f32_mfma<128,split>", "fwd", H=32, N=32, C0=64, Co=128, k=1, f32_split=1, bias=1, **F32_SUB),
    C("f32_mfma64_mm_L0", "f32_mfma<64>", "mm", dt=FP, layout=0, M=100, N=72, K=64, alpha=0.5, bias=1, acc=1),
    C("f32_mfma64_mm_L2_batched", "f32_mfma<64>", "mm", dt=FP, layout=2, M=40, N=48, K=200, batch=3, alpha=2.0),
    C("f32_mfma64_dgrad_s2", "f32_mfma<64>", "dgrad_t", H=8, N=3, C0=64, Co=64, s=2, dt=FP),
    C("f32_mfma64_splitk_wgrad", "f32_mfma<64>+splitk", "wgrad", H=16, N=4, C0=64, Co=64, acc=1, ws=1 << 22, dt=FP),
    C("f32_mfma128_splitk_wgrad", "f32_mfma<128>+splitk", "wgrad", H=16, N=8, C0=128, Co=128, ws=1 << 23, dt=FP),
    C("f32_mfma128_split_splitk", "f32_mfma<128,split>+splitk", "mm", dt=FP, layout=0, M=1024, N=1024, K=512, splitk=4,
      f32_split=1, ws=1 << 23),
    # bf16: the 8-channel ends
    C("thin1_N3", "conv_thin_k<1>", "fwd", H=16, N=3, C0=8, Co=16, bias=1),
    C("thin2_Co24", "conv_thin_k<2>", "fwd", H=8, N=5, C0=8, Co=24, bias=1),
    C("thin4_Co48", "conv_thin_k<4>", "fwd", H=32, N=1, C0=8, Co=48),
    C("thin8_dgrad", "conv_thin_k<8>", "dgrad_t", H=16, N=3, C0=128, Co=8),
    # bf16 halo / small / lin2
    C("halo256_N32_epi", "halo<256,6,NSB,64>", "fwd", H=32, N=32, C0=64, Co=128, bias=1, rowvec=1, resid=1, sub=True),
    C("halo128_3_N63", "halo<128,3,3,64>", "fwd", H=16, N=63, C0=64, Co=128, bias=1, rowvec=1, sub=True),
    C("halo128_4_N13_dgrad_split", "halo<128,4,3,64>", "dgrad_t", H=32, N=13, C0=64, C1=64, Co=128, acc0=0, acc1=1, sub=True),
    C("halo128_6_64x64", "halo<128,6,3,64>", "fwd", H=64, N=4, C0=64, Co=128, resid=1, sub=True),
    C("halo64x32_8x8_N5", "halo<64,2,3,32>", "fwd", H=8, N=5, C0=64, Co=64, bias=1, rowvec=1, resid=1),
    C("halo64x32_8x8_dgrad_split", "halo<64,2,3,32>", "dgrad_t", H=8, N=3, C0=64, C1=64, Co=64, acc0=1, acc1=0),
    C("halo64x32_4x4_N4", "halo<64,3,3,32>", "fwd", H=4, N=4, C0=64, Co=64, bias=1),
    C("halo64x32_4x4_ups", "halo<64,2,3,32>", "fwd", H=4, N=2, C0=64, Co=64, ups=1),
    C("small4_8x8", "conv_small<4,64,32>", "fwd", H=8, N=2, C0=128, Co=128, bias=1, rowvec=1, resid=1),
    C("small5_4x4_N100", "conv_small<5,64,32>", "fwd", H=4, N=100, C0=128, Co=256, bias=1, sub=True),
    C("small3_4x4_N4", "conv_small<3,32,16>", "fwd", H=4, N=4, C0=128, Co=128, bias=1, rowvec=1),
    C("small3_4x4_dgrad_concat", "conv_small<3,32,16>", "dgrad_t", H=4, N=4, C0=128, C1=128, Co=128, acc0=1, acc1=0),
    C("lin2_128_1x1", "lin2<128,128>", "fwd", H=32, N=32, C0=64, Co=128, k=1, bias=1, rowvec=1, resid=1, sub=True),
    C("lin2_64x128_1x1_N50", "lin2<64,128>", "fwd", H=16, N=50, C0=64, Co=128, k=1, bias=1, sub=True),
    C("lin2_64_1x1_Co40_N3", "lin2<64,64>", "fwd", H=8, N=3, C0=64, Co=40, k=1, bias=1, rowvec=1, resid=1),
    C("lin2_64_s2_N3", "lin2<64,64>", "fwd", H=8, N=3, C0=64, Co=64, s=2, bias=1),
    C("lin2_64_outf32", "lin2<64,64>", "fwd", H=8, N=1, C0=64, Co=64, k=1, out_f32=1, bias=1),
    C("lin2_64_tapsplit_N2", "lin2<64,64>+tapsplit", "fwd", H=16, N=2, C0=64, Co=64, ws=1 << 20, bias=1, rowvec=1, resid=1),
    C("lin2_64x128_tapsplit_N6", "lin2<64,128>+tapsplit", "fwd", H=16, N=6, C0=64, Co=128, ws=1 << 21, bias=1),
    C("ups_16x16_fwd", "halo<128,3,3,64>", "fwd", H=8, N=63, C0=64, Co=128, ups=1, sub=True),
    C("ups_32x32_fwd", "halo<256,6,NSB,64>", "fwd", H=16, N=32, C0=64, Co=128, ups=1, sub=True),
    # bf16 weight gradients
    C("wgrad_lin128", "wgrad_lin<128>", "wgrad", H=16, N=8, C0=128, Co=128, acc=1),
    C("wgrad_lin128_splitk_dbias", "wgrad_lin<128>+splitk", "wgrad", H=16, N=8, C0=64, C1=64, Co=128, acc=1, dbias=1, ws=1 << 22),
    C("wgrad_lin64_dbias", "wgrad_lin<64>", "wgrad", H=8, N=3, C0=64, Co=40, acc=1, dbias=1),
    C("wgrad_lin64_splitk_explicit", "wgrad_lin<64>+splitk", "wgrad", H=16, N=4, C0=64, Co=64, splitk=3, ws=1 << 21),
    C("wgrad_lin64_s2", "wgrad_lin<64>+splitk", "wgrad", H=16, N=16, C0=64, Co=64, s=2, ws=1 << 21, acc=1),
    C("wgrad_lin64_ups", "wgrad_lin<64>+splitk", "wgrad", H=8, N=4, C0=64, Co=64, ups=1, ws=1 << 21),
    C("ring64_wgrad_4x4_N1", "ring<64>", "wgrad", H=4, N=1, C0=64, Co=24, acc=1, dbias=1),
    C("ring64_wgrad_splitk_12x12", "ring<64>+splitk", "wgrad", H=12, N=5, C0=64, Co=64, ws=1 << 21, acc=1),
    C("ring128_mm_L2_splitk", "ring<128>+splitk", "mm", layout=2, M=128, N=128, K=2048, out_f32=1, ws=1 << 20, acc=1),
    # bf16 ring / generic
    C("ring128_mm_L0_batched", "ring<128>", "mm", layout=0, M=1024, N=1024, K=64, batch=4, alpha=0.5, bias=1),
    C("ring64_mm_L1", "ring<64>", "mm", layout=1, M=100, N=64, K=128, bias=1, acc=1),
    C("ring64_dgrad_s2_N3", "ring<64>", "dgrad_t", H=8, N=3, C0=64, Co=64, s=2),
    C("ring64_dgrad_s2_tapsplit", "ring<64>+tapsplit", "dgrad_t", H=8, N=3, C0=64, Co=64, s=2, ws=1 << 20, acc0=1),
    C("ring128_dgrad_s2_N33", "ring<128>", "dgrad_t", H=32, N=33, C0=128, Co=128, s=2, sub=True),
    C("ring64_dgrad_L1", "ring<64>", "dgrad", H=8, N=3, C0=64, C1=64, Co=64, acc0=0, acc1=1),
    C("bf16_128_mm_L0", "bf16<128>", "mm", layout=0, M=1024, N=1024, K=72, batch=4),
    C("bf16_64_conv_Cin24", "bf16<64>", "fwd", H=8, N=3, C0=24, Co=40, bias=1, rowvec=1, resid=1),
    C("bf16_64_mm_L1_K40", "bf16<64>", "mm", layout=1, M=100, N=48, K=40, alpha=2.0),
    C("bf16_128_splitk", "bf16<128>+splitk", "mm", layout=0, M=2048, N=2048, K=128, out_f32=1, splitk=4, ws=1 << 25),
    C("bf16_64_splitk", "bf16<64>+splitk", "mm", layout=1, M=128, N=128, K=256, out_f32=1, splitk=4, ws=1 << 20, acc=1),
    # fused pairs (a: 3x3 halo / small conv, b: 1x1 projection) and the two-launch fallback
    C("pair_small4", "pair_small<4>", "pair", a=dict(H=8, N=2, C0=128, Co=128, bias=1, rowvec=1), b=dict(H=8, N=2, C0=128, Co=64, k=1, bias=1)),
    C("pair_small5", "pair_small<5>", "pair", a=dict(H=4, N=100, C0=128, Co=256, sub=True), b=dict(H=4, N=100, C0=128, Co=256, k=1, sub=True)),
    C("pair_small3", "pair_small<3,32,16>", "pair", a=dict(H=4, N=4, C0=128, Co=128, resid=1), b=dict(H=4, N=4, C0=128, Co=128, k=1, bias=1)),
    C("pair_halo64_2", "pair<halo<64,2,3,32>,lin2<64,64>>", "pair", a=dict(H=8, N=5, C0=64, Co=64, bias=1, rowvec=1),
      b=dict(H=8, N=5, C0=64, Co=64, k=1, resid=1)),
    C("pair_halo64_3", "pair<halo<64,3,3,32>,lin2<64,64>>", "pair", a=dict(H=4, N=4, C0=64, Co=64, bias=1), b=dict(H=4, N=4, C0=64, Co=64, k=1)),
    C("pair_halo128_l64x128", "pair<halo<128,3,3,64>,lin2<64,128>>", "pair", a=dict(H=16, N=63, C0=64, Co=128, bias=1, sub=True),
      b=dict(H=16, N=63, C0=64, Co=128, k=1, bias=1, sub=True)),
    C("pair_halo128_l64", "pair<halo<128,3,3,64>,lin2<64,64>>", "pair", a=dict(H=16, N=63, C0=64, Co=128, sub=True),
      b=dict(H=16, N=63, C0=64, Co=64, k=1, sub=True)),
    C("pair_halo256_l128", "pair<halo<256,6,NSB,64>,lin2<128,128>>", "pair", a=dict(H=32, N=32, C0=64, Co=128, bias=1, sub=True),
      b=dict(H=32, N=32, C0=64, Co=128, k=1, bias=1, sub=True)),
    C("pair_two_launches", "pair:two launches", "pair", a=dict(H=8, N=3, C0=8, Co=64), b=dict(H=8, N=3, C0=64, Co=64, k=1, bias=1)),
    # grouped weight gradients
    C("group_per_tap", "wgrad_group", "group", members=[dict(H=8, N=4, C0=64, Co=64, splitk=1), dict(H=16, N=2, C0=64, Co=128, k=1, splitk=1)]),
    C("group_splitk", "wgrad_group+splitk", "group", members=[dict(H=16, N=8, C0=128, Co=128, splitk=4, ws=1 << 22),
                                                              dict(H=8, N=4, C0=64, C1=64, Co=64, splitk=1)]),
    C("group_taps", "wgrad_taps_group", "group", min_share=0, members=[dict(H=16, N=4, C0=64, Co=64, splitk=1), dict(H=8, N=3, C0=64, Co=128, splitk=1)]),
    C("group_taps_splitk", "wgrad_taps_group+splitk", "group", min_share=0,
      members=[dict(H=32, N=2, C0=64, Co=64, splitk=1), dict(H=8, N=4, C0=64, Co=64, k=1, splitk=2, ws=1 << 20)]),
]


def _case_list():
    return [p.values[0] for p in CASES]


@pytest.mark.parametrize("case", CASES)
def test_route_parity(case):
    route, P = launch(case, torch.device("cuda:0"))
    assert route == case.route, f"{case.id}: ran {route}, expected {case.route}"
    for name, ratio, rel, store in verify(case, P):
        note("gemm_routes", dict(case=case.id, route=route, out=name, ratio=ratio, rel_l2=rel, store=store))
        assert rel <= REL_BAR[store], f"{case.id}.{name}: rel-L2 {rel:.3e} above the {store} bar {REL_BAR[store]:.1e}"


def test_every_route_is_reached():
    from mdm import _lib
    names = set(_lib.route_names())
    assert set(EXCLUDED) <= names, set(EXCLUDED) - names
    hit = {c.route for c in _case_list()}
    assert hit <= names, hit - names
    missing = names - hit - set(EXCLUDED)
    assert not missing, f"routes no case reaches: {sorted(missing)}"


@pytest.mark.parametrize("case", [c for c in CASES if not (c.values[0].kind == "wgrad" and c.values[0].p.get("dbias"))])
def test_route_is_bit_reproducible(case):
    """Two runs into fresh NaN-prefilled buffers give the same bits (no row here sums with float atomics)."""
    dev = torch.device("cuda:0")
    outs = []
    for _ in range(2):
        route, P = launch(case, dev)
        torch.cuda.synchronize()
        outs.append([b.t.clone() for name, b, *_ in P.outs])
        assert route == case.route
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), case.id
