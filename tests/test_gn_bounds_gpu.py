"""fp64 bounds for every compiled GroupNorm kernel and every operand it takes (csrc/gn_kernels.inc; the fused epilogues of
csrc/gemm.hip further down).

norm.hip compiles 38 standalone kernels: five gn_fwd_reg rungs x {bf16, fp32} x {plain, dropout}, gn_fwd x 2 x 2, five gn_bwd_reg
rungs (bf16) x {plain, dropout}, gn_bwd x 2 x 2.  A route name (mdm_gn_route_of) carries neither the storage type nor dropout, so the
rows do: FWD_ROWS / BWD_ROWS of tests/_gn_rows.py hold at least one row per instantiation (test_every_instantiation_has_a_row; the
routes are checked without a GPU in tests/test_gn_bounds_cpu.py), at the smallest shapes that reach each edge -- P below the pixel
lanes, a partial last vector per lane, 48- and 24-channel blocks, a block that straddles the two sources, a partial last channel block
(C = 72, G = 24: the `c < C`, `cb + t < C` and `g0 + t < G` guards), a block that is the whole tensor -- and the backward rows every
operand form on both compile-time paths of gn_bwd_reg_kernel (NP <= 4 fetches the addends ahead of the reduction, NP = 8 in the apply
loop) and on the streaming kernel in both storage types.

Every output is held per element against the bounds derived in tests/_bounds.py (gn_fwd_ref / gn_bwd_ref): the backward runs on
CPU-made statistics (fp64 -> fp32), so neither direction can hide the other's error.  bf16 y and dx also meet the rel-L2 bar of the
storage precision.  Every tensor sits inside NaN guard bands; overwrite outputs and the workspace start as the NaN pattern; addends
must come back bit for bit; a second launch must repeat the first bit for bit (except bf16 dgamma / dbeta / sum_all: float atomics
across the images)."""
import struct

import pytest
import torch

from _bounds import EPS_EXP, Buf, check_bound, gn_bwd_ref, gn_fwd_ref, gn_stats_in, rel_l2_bar, rne_bf16
from _dropout_ref import ctl_words
from _gn_rows import (BWD_ROWS, DROP_BASE, DT, EPS, FUSED_G, FWD_ROWS, GNB_BIG_ROWS, GNB_ROWS, GNF_BIG_ROWS, GNF_ROWS, KEY, OFFSET, R2, RATE,
                      S128, TD, bwd_problem, fused_geom, fused_id, fused_route, fwd_problem, row_id, row_keep,
                      rows_cover_every_instantiation)
from _notes import note

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _untouched(b):
    return bool((b.raw.view(b.ity) == b.pat).all())


def _assert_guards(bufs, what):
    for name, b in bufs.items():
        assert b.guards_intact(), f"{what}: guard band of {name} touched at (below, above) = {b.first_bad_guard()}"


def _drop_fields(drop, rate=RATE):
    if not drop:
        return {}
    dev = _dev()
    thr, scale = ctl_words(rate)
    return dict(rng=torch.tensor([KEY, OFFSET], dtype=torch.int64, device=dev), drop_base=DROP_BASE,
                ctl=torch.tensor([thr, struct.unpack("<i", struct.pack("<f", scale))[0]], dtype=torch.int32, device=dev))


def _src_bufs(x, C0, C1, td):
    dev = _dev()
    B = dict(s0=Buf(x[..., :C0].shape, td, dev, x[..., :C0].contiguous()))
    if C1:
        B["s1"] = Buf(x[..., C0:].shape, td, dev, x[..., C0:].contiguous())
    return B


def _vec(t):
    return Buf(t.shape, torch.float32, _dev(), t)


def _run_fwd(row, x, gamma, beta, drop_fields):
    from mdm import _lib
    route, dt, drop, (C0, C1, P, G), N, draw, silu = row
    dev, td = _dev(), TD[dt]
    B = dict(_src_bufs(x, C0, C1, td), gamma=_vec(gamma), beta=_vec(beta), y=Buf((N, P, C0 + C1), td, dev),
             stats=Buf((N, G, 2), torch.float32, dev), ws=Buf((256,), torch.float32, dev))
    _lib.groupnorm("mdm_groupnorm_fwd", dtype=DT[dt], src0=B["s0"].t, C0=C0, src1=B["s1"].t if C1 else None, C1=C1, N=N, P=P, G=G,
                   gamma=B["gamma"].t, beta=B["beta"].t, silu=silu, stats=B["stats"].t, ws=B["ws"].t, y=B["y"].t, eps=EPS, **drop_fields)
    assert _lib.gn_last_route() == route
    torch.cuda.synchronize()
    return B


@pytest.mark.parametrize("row", FWD_ROWS, ids=[row_id(r) for r in FWD_ROWS])
def test_forward_bounds(row):
    from mdm import _lib
    route, dt, drop, (C0, C1, P, G), N, draw, silu = row
    C = C0 + C1
    assert _lib.gn_route_of(0, dtype=DT[dt], N=N, P=P, G=G, C0=C0, C1=C1) == route
    x, gamma, beta, R = fwd_problem(row)
    B = _run_fwd(row, x, gamma, beta, _drop_fields(drop))
    _assert_guards(B, row_id(row))
    assert _untouched(B["ws"]), "the forward wrote its workspace"
    for name in ("y", "stats"):
        ratio, rel = check_bound(f"{row_id(row)} {name}", B[name].t, *R[name])
        note("gn_bounds", dict(row=row_id(row), out=name, ratio=ratio, rel_l2=rel))
        if name == "y" and dt == "bf16":
            bar = rel_l2_bar(R["y"][0])
            assert rel <= bar, f"y: rel-L2 {rel:.3e} above the storage precision's bar {bar:.3e}"
    if drop:
        keep, _ = row_keep(row)
        assert float(B["y"].t.float().cpu()[~keep].abs().max()) == 0.0          # dropped elements: exact zeros
    if draw == "constant":
        # gn_pivot's promise: the constant group's mean is K itself and its variance exactly 0, so rstd = rsqrtf(eps).  rsqrtf is
        # within 1 ulp of the true value and the correctly rounded fp32 value within half of one: two fp32 numbers less than two
        # ulps apart are neighbours at most, so rstd's bits are those of fp32(1 / sqrt(eps)) or of a neighbour (a variance of 1e-13
        # moves rstd by most of an ulp, one of 1e-12 by eight).  No tighter statement exists without the bits of the device
        # library's rsqrtf, which no document gives.
        st, yc = B["stats"].t.cpu(), B["y"].t.cpu()[N - 1, :, (G - 1) * (C // G):]
        bc = beta[(G - 1) * (C // G):]
        assert float(st[N - 1, G - 1, 0]) == 0.75
        eps32 = torch.tensor(EPS, dtype=torch.float32)
        want = eps32.double().rsqrt().float()
        assert abs(int(st[N - 1, G - 1, 1].view(torch.int32)) - int(want.view(torch.int32))) <= 1, (float(st[N - 1, G - 1, 1]), float(want))
        assert bool((_bits(yc) == _bits(yc)[:1]).all())                        # the same bits at every pixel of a channel
        if not silu:                # y = fma(0, a, beta) = beta, through the store's rounding
            assert torch.equal(yc, bc.to(TD[dt]).expand_as(yc))
        else:
            # z = beta exactly, so y = silu(beta) up to the fast exponential, the add, the reciprocal and the product alone:
            # e = (EPS_EXP + 2^-23 |beta| + 2^-22) |silu(beta)| (tests/_bounds.py).  A bf16 store rounds that to rne_bf16(silu(beta))
            # itself unless silu(beta) lies within e of a rounding tie; then to one of the two candidates.  fp32: within e.
            s = bc.double() * torch.sigmoid(bc.double())
            e = (EPS_EXP + 2.0 ** -23 * bc.double().abs() + 2.0 ** -22) * s.abs()
            if dt == "bf16":
                lo, hi = rne_bf16(s - e), rne_bf16(s + e)
                assert bool(((yc[0] == lo) | (yc[0] == hi)).all()), (yc[0], lo, hi)
                assert bool((lo == hi).any()), "no channel of the constant group pins silu(beta) to one bf16 value"
            else:
                assert bool(((yc[0].double() - s).abs() <= e + 2.0 ** -24 * s.abs()).all())
    B2 = _run_fwd(row, x, gamma, beta, _drop_fields(drop))
    for name in ("y", "stats"):
        assert torch.equal(_bits(B[name].t), _bits(B2[name].t)), f"{name} differs between two identical launches"


def _run_bwd(row, x, dy, stats, gamma, beta, adds, pri, drop_fields):
    from mdm import _lib
    route, dt, drop, (C0, C1, P, G), N, draw, silu, form = row
    dev, td = _dev(), TD[dt]
    C = C0 + C1
    need = _lib.load().mdm_groupnorm_bwd_ws_floats(DT[dt], N, C)
    B = dict(_src_bufs(x, C0, C1, td), gamma=_vec(gamma), beta=_vec(beta), dy=Buf((N, P, C), td, dev, dy), stats=_vec(stats),
             dgamma=_vec(pri["dgamma"]), dbeta=_vec(pri["dbeta"]), ws=Buf((need or 256,), torch.float32, dev),
             d0=Buf((N, P, C0), td, dev, adds["a"][..., :C0] if form in ("acc", "add2", "sums") else "nan"))
    if C1:
        B["d1"] = Buf((N, P, C1), td, dev)
    f = dict(dst0=B["d0"].t, dst1=B["d1"].t if C1 else None)
    if form in ("acc", "add2", "sums"):
        f["add0"] = B["d0"].t
    if form == "add":
        B["a0"] = Buf((N, P, C0), td, dev, adds["a"][..., :C0])
        f["add0"] = B["a0"].t
        if C1:                      # (none of the rows: an addend of a two-source dx goes to both halves)
            B["a1"] = Buf((N, P, C1), td, dev, adds["a"][..., C0:])
            f["add1"] = B["a1"].t
    if form == "add2":
        B["a0b"] = Buf((N, P, C0), td, dev, adds["b"][..., :C0])
        f["add0b"] = B["a0b"].t
    if form == "add1":
        B["a1"] = Buf((N, P, C1), td, dev, adds["a"][..., C0:])
        f["add1"] = B["a1"].t
    if form == "sums":
        B["sum_img"] = Buf((N, C + 8), torch.float32, dev)
        B["sum_all"] = _vec(pri["sum_all"])
        f.update(sum_img=B["sum_img"].t.reshape(-1)[4:], sum_ld=C + 8, sum_all=B["sum_all"].t)
    _lib.groupnorm("mdm_groupnorm_bwd", dtype=DT[dt], src0=B["s0"].t, C0=C0, src1=B["s1"].t if C1 else None, C1=C1, N=N, P=P, G=G,
                   gamma=B["gamma"].t, beta=B["beta"].t, silu=silu, stats=B["stats"].t, ws=B["ws"].t, dy=B["dy"].t,
                   dgamma=B["dgamma"].t, dbeta=B["dbeta"].t, **f, **drop_fields)
    assert _lib.gn_last_route() == route
    torch.cuda.synchronize()
    return B


def _bwd_outputs(B, row):
    C0, C1, P, G = row[3]
    C = C0 + C1
    out = dict(dx=torch.cat((B["d0"].t, B["d1"].t), 2) if C1 else B["d0"].t, dgamma=B["dgamma"].t, dbeta=B["dbeta"].t)
    if "sum_img" in B:
        out.update(sum_img=B["sum_img"].t[:, 4:4 + C], sum_all=B["sum_all"].t)
    return out


@pytest.mark.parametrize("row", BWD_ROWS, ids=[row_id(r) for r in BWD_ROWS])
def test_backward_bounds(row):
    from mdm import _lib
    route, dt, drop, (C0, C1, P, G), N, draw, silu, form = row
    C = C0 + C1
    assert _lib.gn_route_of(1, dtype=DT[dt], N=N, P=P, G=G, C0=C0, C1=C1) == route
    x, dy, stats, gamma, beta, adds, pri, R = bwd_problem(row)
    B = _run_bwd(row, x, dy, stats, gamma, beta, adds, pri, _drop_fields(drop))
    _assert_guards(B, row_id(row))
    if dt == "bf16":
        assert _untouched(B["ws"]), "the bf16 backward wrote its workspace"
    got = _bwd_outputs(B, row)
    for name, y in got.items():
        ratio, rel = check_bound(f"{row_id(row)} {name}", y, *R[name])
        note("gn_bounds", dict(row=row_id(row), out=name, ratio=ratio, rel_l2=rel))
        if name == "dx" and dt == "bf16":
            bar = rel_l2_bar(R["dx"][0])
            assert rel <= bar, f"dx: rel-L2 {rel:.3e} above the storage precision's bar {bar:.3e}"
    if form == "sums":          # the pad columns of the pitched sum_img still hold the pattern
        si = B["sum_img"]
        iv = si.t.view(si.ity)
        assert bool((iv[:, :4] == si.pat).all()) and bool((iv[:, 4 + C:] == si.pat).all())
    for name, key, sl in (("a0", "a", slice(0, C0)), ("a1", "a", slice(C0, C)), ("a0b", "b", slice(0, C0))):
        if name in B:
            assert torch.equal(_bits(B[name].t.cpu()), _bits(adds[key][..., sl].to(TD[dt]).contiguous())), f"{name} was modified"
    for name in ("s0", "s1", "dy", "stats", "gamma", "beta"):
        assert name not in B or not bool(torch.isnan(B[name].t.float()).any())
    B2 = _run_bwd(row, x, dy, stats, gamma, beta, adds, pri, _drop_fields(drop))
    got2 = _bwd_outputs(B2, row)
    for name in got:
        if dt == "f32" or name in ("dx", "sum_img"):
            assert torch.equal(_bits(got[name].contiguous()), _bits(got2[name].contiguous())), f"{name} differs between two identical launches"


def test_every_instantiation_has_a_row():
    rows_cover_every_instantiation()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_zero_threshold_reproduces_the_plain_descriptor(dt):
    """a dropout descriptor whose ctl holds thr = 0 (eval mode): the bits of the plain descriptor, forward and backward"""
    shape = S128
    frow = ("fwd_" + R2, dt, 0, shape, 2, "plain", 1)
    x, gamma, beta, _ = fwd_problem(frow)
    a, b = _run_fwd(frow, x, gamma, beta, {}), _run_fwd(frow, x, gamma, beta, _drop_fields(1, rate=0.0))
    for name in ("y", "stats"):
        assert torch.equal(_bits(a[name].t), _bits(b[name].t)), name
    brow = ("bwd_" + R2 if dt == "bf16" else "bwd+reduce", dt, 0, shape, 2, "plain", 1, "acc")
    x, dy, stats, gamma, beta, adds, pri, _ = bwd_problem(brow)
    a = _bwd_outputs(_run_bwd(brow, x, dy, stats, gamma, beta, adds, pri, {}), brow)
    b = _bwd_outputs(_run_bwd(brow, x, dy, stats, gamma, beta, adds, pri, _drop_fields(1, rate=0.0)), brow)
    for name in a:
        if dt == "f32" or name == "dx":
            assert torch.equal(_bits(a[name].contiguous()), _bits(b[name].contiguous())), name


def _fused_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return g, 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def _q16(t):
    return t.bfloat16().float()


def _run_gnb(row, T, variant):
    from mdm import _lib, ops
    route, H, N, C, Co, k = row
    dev, P, bf = _dev(), H * H, torch.bfloat16
    B = dict(x=Buf((N, P, C), bf, dev, T["x"]), dy=Buf((N, H, H, Co), bf, dev, T["dy"]), wT=Buf(T["wT"].shape, bf, dev, T["wT"]),
             stats=_vec(T["stats"]), gamma=_vec(T["gamma"]), beta=_vec(T["beta"]), dgamma=_vec(T["pri"]["dgamma"]),
             dbeta=_vec(T["pri"]["dbeta"]), dx=Buf((N, P, C), bf, dev, T["prior"] if "acc" in variant else "nan"))
    gnb = dict(x=B["x"].t, stats=B["stats"].t, gamma=B["gamma"].t, beta=B["beta"].t, dgamma=B["dgamma"].t, dbeta=B["dbeta"].t,
               G=FUSED_G, silu=T["silu"])
    if "add" in variant:
        B["add"] = Buf((N, P, C), bf, dev, T["addt"])
        gnb["add"] = B["add"].t
    if "sums" in variant:
        B["sum_img"] = Buf((N, C + 8), torch.float32, dev)
        B["sum_all"] = _vec(T["pri"]["sum_all"])
        gnb.update(sum_img=B["sum_img"].t.reshape(-1)[4:], sum_ld=C + 8, sum_all=B["sum_all"].t)
    ops.conv_dgrad_t(1, fused_geom(H, N, C, Co, k), B["dy"].t, B["wT"].t, B["dx"].t, int("acc" in variant), gnb=gnb)
    assert _lib.last_route() == route
    torch.cuda.synchronize()
    return B


GNB_ALL, GNF_ALL = GNB_ROWS + GNB_BIG_ROWS, GNF_ROWS + GNF_BIG_ROWS


@pytest.mark.parametrize("row", GNB_ALL, ids=[fused_id(r) for r in GNB_ALL])
def test_fused_backward_bounds(row):
    """dz = the data gradient (fp64 conv_dgrad_ref; the kernel's dz is off by at most (K + 8) 2^-23 mag, handed on as dy_err), then
    gn_bwd_ref of it: dx accumulated (acc0), with a residual-branch addend and the column sums (gnb_add, gnb_sum_img / _sum_all),
    and with both addends; dgamma / dbeta onto random priors."""
    from _bounds import conv_dgrad_ref
    route, H, N, C, Co, k = row
    assert fused_route("gnb", H, N, C, Co, k) == route
    P, taps, pd = H * H, k * k, k // 2
    g, gamma, beta = _fused_params(C, 11 * C + Co + H + k)
    x = _q16(torch.randn(N, P, C, generator=g) * 1.2 + 0.3)
    dy = _q16(torch.randn(N, H, H, Co, generator=g))
    wt = _q16(torch.randn(taps, Co, C, generator=g) / (taps * Co) ** 0.5)                 # [tap][Cout][Cin]
    T = dict(x=x, dy=dy, wT=wt.transpose(1, 2).contiguous(), stats=gn_stats_in(x, FUSED_G, EPS), gamma=gamma, beta=beta,
             silu=int(GNB_ALL.index(row) % 3 != 2), prior=_q16(torch.randn(N, P, C, generator=g)),
             addt=_q16(0.5 * torch.randn(N, P, C, generator=g)),
             pri=dict(dgamma=torch.randn(C, generator=g), dbeta=torch.randn(C, generator=g), sum_all=torch.randn(C, generator=g) + 2.0))
    dz, dzmag = conv_dgrad_ref(dy, wt, H, H, C, k, k, 1, (pd, pd, pd, pd))
    dz, dz_err = dz.reshape(N, P, C), (taps * Co + 8) * 2.0 ** -23 * dzmag.reshape(N, P, C)
    for variant, adds in (("acc", [T["prior"]]), ("add+sums", [T["addt"]]), ("acc+add", [T["prior"], T["addt"]])):
        R = gn_bwd_ref(x, dz, T["stats"][..., 0], T["stats"][..., 1], gamma, beta, FUSED_G, T["silu"], "bf16", adds, dy_err=dz_err,
                       prior=T["pri"] if "sums" in variant else dict(T["pri"], sum_all=None))
        B = _run_gnb(row, T, variant)
        _assert_guards(B, f"{fused_id(row)} {variant}")
        got = dict(dx=B["dx"].t, dgamma=B["dgamma"].t, dbeta=B["dbeta"].t)
        if "sums" in variant:
            got.update(sum_img=B["sum_img"].t[:, 4:4 + C], sum_all=B["sum_all"].t)
            iv = B["sum_img"].t.view(B["sum_img"].ity)
            assert bool((iv[:, :4] == B["sum_img"].pat).all()) and bool((iv[:, 4 + C:] == B["sum_img"].pat).all())
        for name, y in got.items():
            ratio, rel = check_bound(f"gnb {fused_id(row)} {variant} {name}", y, *R[name])
            note("gn_bounds", dict(row="gnb-" + fused_id(row) + "-" + variant, out=name, ratio=ratio, rel_l2=rel))
            if name == "dx":
                assert rel <= rel_l2_bar(R["dx"][0]), (rel, rel_l2_bar(R["dx"][0]))
        if "add" in variant:
            assert torch.equal(_bits(B["add"].t.cpu()), _bits(T["addt"].bfloat16())), "gnb_add was modified"
        B2 = _run_gnb(row, T, variant)
        assert torch.equal(_bits(B["dx"].t), _bits(B2["dx"].t)), "dx differs between two identical launches"
        if "sums" in variant:
            assert torch.equal(_bits(B["sum_img"].t), _bits(B2["sum_img"].t)), "sum_img differs between two identical launches"


def _run_gnf(row, T):
    from mdm import _lib, ops
    route, H, N, C, Co, k = row
    dev, bf = _dev(), torch.bfloat16
    B = dict(x=Buf((N, H, H, C), bf, dev, T["x"]), w=Buf(T["wt"].shape, bf, dev, T["wt"]), bias=_vec(T["bias"]), rv=_vec(T["rv"]),
             resid=Buf((N, H, H, Co), bf, dev, T["resid"]), gamma=_vec(T["gamma"]), beta=_vec(T["beta"]),
             y=Buf((N, H, H, Co), bf, dev), z=Buf((N, H, H, Co), bf, dev), stats=Buf((N, FUSED_G, 2), torch.float32, dev))
    ops.conv_fwd(1, fused_geom(H, N, C, Co, k), B["x"].t, None, B["w"].t, B["bias"].t, B["y"].t, rowvec=B["rv"].t, rv_ld=Co,
                 resid=B["resid"].t, gnf=dict(out=B["z"].t, gamma=B["gamma"].t, beta=B["beta"].t, stats=B["stats"].t, G=FUSED_G,
                                              silu=T["silu"], eps=EPS))
    assert _lib.last_route() == route
    torch.cuda.synchronize()
    return B


@pytest.mark.parametrize("row", GNF_ALL, ids=[fused_id(r) for r in GNF_ALL])
def test_fused_forward_bounds(row):
    """y = conv + bias + time-embedding row + residual against fp64 (_bounds.check); the normalised output and the statistics as
    gn_fwd_ref(scheme="two_pass") of the y the kernel stored, read back: the GroupNorm's bound does not carry the convolution's."""
    from _bounds import check, conv_fwd_ref, epilogue_ref
    route, H, N, C, Co, k = row
    assert fused_route("gnf", H, N, C, Co, k) == route
    P, taps, pd = H * H, k * k, k // 2
    g, gamma, beta = _fused_params(Co, 7 * C + Co + H + k)
    T = dict(x=_q16(torch.randn(N, H, H, C, generator=g)), wt=_q16(torch.randn(taps, Co, C, generator=g) / (taps * C) ** 0.5),
             bias=torch.randn(Co, generator=g), rv=torch.randn(N, Co, generator=g), resid=_q16(torch.randn(N, H, H, Co, generator=g)),
             gamma=gamma, beta=beta, silu=int(GNF_ALL.index(row) % 3 != 2))
    B = _run_gnf(row, T)
    _assert_guards(B, fused_id(row))
    acc, mag = conv_fwd_ref(T["x"], None, T["wt"], k, k, 1, (pd, pd, pd, pd), 0)
    ref, mg = epilogue_ref(acc.reshape(-1, Co), mag.reshape(-1, Co), bias=T["bias"], rowvec=T["rv"], rv_ld=Co, rows_per_img=P,
                           resid=T["resid"].reshape(-1, Co))
    ratio, rel = check(f"gnf {fused_id(row)} y", B["y"].t.reshape(-1, Co), ref, mg, taps * C, "bf16")
    note("gn_bounds", dict(row="gnf-" + fused_id(row), out="conv_y", ratio=ratio, rel_l2=rel))
    R = gn_fwd_ref(B["y"].t.cpu().float().reshape(N, P, Co), gamma, beta, FUSED_G, EPS, T["silu"], "bf16", "two_pass")
    for name, y in (("y", B["z"].t.reshape(N, P, Co)), ("stats", B["stats"].t)):
        ratio, rel = check_bound(f"gnf {fused_id(row)} {name}", y, *R[name])
        note("gn_bounds", dict(row="gnf-" + fused_id(row), out="gnf_out" if name == "y" else "gnf_stats", ratio=ratio, rel_l2=rel))
        if name == "y":
            assert rel <= rel_l2_bar(R["y"][0]), (rel, rel_l2_bar(R["y"][0]))
    B2 = _run_gnf(row, T)
    for name in ("y", "z", "stats"):
        assert torch.equal(_bits(B[name].t), _bits(B2[name].t)), f"{name} differs between two identical launches"
