"""Row tables of the GroupNorm bound tests and what builds a row's problem, shared by tests/test_gn_bounds_gpu.py (which runs the
rows on the GPU) and by tests/test_bounds_cpu.py and tests/test_gn_bounds_cpu.py (which emulate them and check their routes without
one).  Helpers only, no test functions."""
import torch

from _bounds import gn_bwd_ref, gn_draw, gn_fwd_ref, gn_stats_in
from _dropout_ref import ctl_words, keep_mask

DT = {"f32": 0, "bf16": 1}
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS = 1e-6
RATE, KEY, OFFSET, DROP_BASE = 0.25, 0x1234ABCD | (3 << 32), (1 << 33) + 7, 8 * 12345

R1, R2, R3, R4, R5 = "reg<1,256>", "reg<2,256>", "reg<2,512>", "reg<4,512>", "reg<8,512>"
S16, S64, S128, S256, S512 = (32, 0, 16, 32), (32, 0, 64, 32), (32, 0, 128, 32), (32, 0, 256, 32), (32, 0, 512, 32)
S576, S2048, S4096 = (32, 0, 576, 32), (32, 0, 2048, 32), (32, 0, 4096, 32)
S96, S384, S2SRC, S72, S16C = (96, 0, 64, 32), (384, 0, 1024, 32), (64, 32, 64, 32), (72, 0, 64, 24), (16, 0, 1024, 2)
S2SRC8, S2SRCS = (16, 16, 2048, 32), (16, 16, 4096, 32)          # two sources at NP = 8 and on the streaming kernels
# groups of two channels for the column sums of dx: with one channel per group every column sum is zero, whatever the kernel does
S64W, S256W, S4096W = (64, 0, 64, 32), (64, 0, 256, 32), (64, 0, 4096, 32)

# (route, storage, dropout, (C0, C1, P, G), N, draw, silu)
FWD_ROWS = [
    ("fwd_" + R1, "f32", 0, S16, 2, "plain", 1),                  # P < PL: three quarters of the pixel lanes idle
    ("fwd_" + R1, "f32", 0, S64, 3, "constant", 0),
    ("fwd_" + R2, "f32", 0, S128, 2, "spiked", 1),
    ("fwd_" + R2, "f32", 0, S2SRC, 2, "plain", 1),                # 48-channel blocks, the second straddles the sources
    ("fwd_" + R2, "f32", 0, S72, 2, "plain", 1),                  # partial last channel block, 24 groups
    ("fwd_" + R3, "f32", 0, S256, 2, "offset", 1),
    ("fwd_" + R4, "f32", 0, S512, 2, "spiked", 1),                # the widened fp32 block at np = 8
    ("fwd_" + R4, "f32", 0, S16C, 2, "plain", 1),                 # the block is the whole tensor
    ("fwd_" + R5, "f32", 0, S576, 2, "spiked", 0),                # partial last vector of a lane
    ("fwd_" + R5, "f32", 0, S384, 2, "spiked", 1),                # 24-channel blocks, 85 pixel lanes, np = 13
    ("fwd_" + R5, "f32", 0, S2048, 2, "offset", 1),
    ("fwd", "f32", 0, S4096, 2, "spiked", 1),
    ("fwd", "f32", 0, S4096, 2, "offset", 0),
    ("fwd_" + R1, "f32", 1, S64, 2, "plain", 1),
    ("fwd_" + R2, "f32", 1, S96, 2, "plain", 1),
    ("fwd_" + R3, "f32", 1, S256, 2, "spiked", 1),
    ("fwd_" + R4, "f32", 1, S512, 2, "plain", 1),
    ("fwd_" + R5, "f32", 1, S576, 2, "spiked", 1),
    ("fwd", "f32", 1, S4096, 2, "plain", 1),
    ("fwd_" + R1, "bf16", 0, S16, 2, "plain", 1),
    ("fwd_" + R1, "bf16", 0, S64, 3, "constant", 1),
    ("fwd_" + R2, "bf16", 0, S128, 2, "spiked", 1),
    ("fwd_" + R2, "bf16", 0, S96, 2, "plain", 0),                 # VB = 6: the column sums that do not shuffle
    ("fwd_" + R2, "bf16", 0, S2SRC, 2, "spiked", 1),
    ("fwd_" + R2, "bf16", 0, S72, 2, "constant", 0),
    ("fwd_" + R3, "bf16", 0, S256, 2, "plain", 1),
    ("fwd_" + R3, "bf16", 0, S512, 2, "spiked", 1),
    ("fwd_" + R4, "bf16", 0, S576, 2, "spiked", 1),
    ("fwd_" + R4, "bf16", 0, S16C, 2, "plain", 1),
    ("fwd_" + R5, "bf16", 0, S2048, 2, "spiked", 1),
    ("fwd_" + R5, "bf16", 0, S384, 2, "plain", 1),
    ("fwd", "bf16", 0, S4096, 2, "spiked", 1),
    ("fwd_" + R1, "bf16", 1, S16, 2, "plain", 1),
    ("fwd_" + R2, "bf16", 1, S128, 2, "spiked", 1),
    ("fwd_" + R3, "bf16", 1, S256, 2, "plain", 1),
    ("fwd_" + R4, "bf16", 1, S576, 2, "spiked", 0),
    ("fwd_" + R5, "bf16", 1, S2048, 2, "plain", 1),
    ("fwd", "bf16", 1, S4096, 2, "spiked", 1),
]
# operand forms of the backward: "ow" overwrite; "acc" add0 == dst0; "add" add0 = another tensor; "add2" add0 == dst0 and add0b;
# "add1" an addend of the second source's dx; "sums" sum_img (row pitch C + 8, pad columns untouched) + sum_all (prior non-zero) on
# an accumulating dx, as the step has them: the sums are those of dx in front of the addition
FORMS = ("ow", "acc", "add", "add2", "add1", "sums")
# (route, storage, dropout, (C0, C1, P, G), N, draw, silu, form)
BWD_ROWS = [
    ("bwd_" + R1, "bf16", 0, S16, 2, "plain", 1, "ow"),
    ("bwd_" + R1, "bf16", 0, S64, 2, "spiked", 1, "acc"),
    ("bwd_" + R2, "bf16", 0, S128, 2, "plain", 1, "add"),
    ("bwd_" + R2, "bf16", 0, S96, 3, "spiked", 1, "sums"),
    ("bwd_" + R2, "bf16", 0, S2SRC, 2, "plain", 1, "add1"),
    ("bwd_" + R2, "bf16", 0, S72, 2, "spiked", 0, "add2"),
    ("bwd_" + R3, "bf16", 0, S256, 2, "spiked", 1, "add2"),
    ("bwd_" + R3, "bf16", 0, S256W, 3, "plain", 1, "sums"),
    ("bwd_" + R4, "bf16", 0, S576, 2, "spiked", 1, "acc"),
    ("bwd_" + R4, "bf16", 0, S16C, 2, "plain", 1, "add"),
    ("bwd_" + R5, "bf16", 0, S2048, 2, "spiked", 1, "ow"),        # NP = 8: the addends are loaded in the apply loop
    ("bwd_" + R5, "bf16", 0, S2048, 2, "plain", 1, "acc"),
    ("bwd_" + R5, "bf16", 0, S384, 2, "spiked", 1, "add"),
    ("bwd_" + R5, "bf16", 0, S2048, 2, "spiked", 0, "add2"),
    ("bwd_" + R5, "bf16", 0, S2SRC8, 2, "plain", 1, "add1"),
    ("bwd_" + R5, "bf16", 0, S384, 3, "spiked", 1, "sums"),
    ("bwd", "bf16", 0, S4096, 2, "spiked", 1, "ow"),
    ("bwd", "bf16", 0, S4096, 2, "plain", 1, "acc"),
    ("bwd", "bf16", 0, S4096, 2, "spiked", 0, "add"),
    ("bwd", "bf16", 0, S4096, 2, "plain", 1, "add2"),
    ("bwd", "bf16", 0, S2SRCS, 2, "spiked", 1, "add1"),
    ("bwd", "bf16", 0, S4096W, 3, "spiked", 1, "sums"),
    ("bwd+reduce", "f32", 0, S64, 2, "plain", 1, "ow"),
    ("bwd+reduce", "f32", 0, S576, 2, "spiked", 1, "acc"),
    ("bwd+reduce", "f32", 0, S96, 2, "plain", 1, "add"),
    ("bwd+reduce", "f32", 0, S72, 2, "spiked", 1, "add2"),
    ("bwd+reduce", "f32", 0, S2SRC, 2, "plain", 0, "add1"),
    ("bwd+reduce", "f32", 0, S4096W, 3, "spiked", 1, "sums"),
    ("bwd+reduce", "f32", 0, S16C, 2, "constant", 1, "ow"),
    ("bwd+reduce", "f32", 0, S384, 2, "spiked", 1, "acc"),
    ("bwd+reduce", "f32", 0, S256, 2, "offset", 1, "ow"),
    ("bwd_" + R1, "bf16", 1, S64W, 3, "plain", 1, "sums"),
    ("bwd_" + R2, "bf16", 1, S128, 2, "spiked", 1, "acc"),
    ("bwd_" + R3, "bf16", 1, S256, 2, "plain", 1, "ow"),
    ("bwd_" + R4, "bf16", 1, S576, 2, "spiked", 1, "add"),
    ("bwd_" + R5, "bf16", 1, S2048, 2, "plain", 1, "add2"),
    ("bwd", "bf16", 1, S4096W, 3, "spiked", 1, "sums"),
    ("bwd+reduce", "f32", 1, S576, 2, "spiked", 1, "acc"),
]


def instantiations():
    """The compiled standalone kernels as (route, storage, dropout), from the library's own route names (mdm_gn_route_names) and the
    launchers of csrc/norm.hip: every forward route resolves both storage types (gn_resolve), the register backward is bf16 only,
    "bwd" is gn_bwd_kernel<bf16> and "bwd+reduce" gn_bwd_kernel<float>; each once plain and once with dropout.  A route the library
    gains shows up here, and in rows_cover_every_instantiation, by itself."""
    from mdm import _lib
    out = []
    for name in _lib.gn_route_names():
        dts = ("f32", "bf16") if name.startswith("fwd") else ("f32",) if name == "bwd+reduce" else ("bf16",)
        out += [(name, dt, dr) for dt in dts for dr in (0, 1)]
    return out


def rows_cover_every_instantiation():
    """asserts: every compiled kernel has a row, and every operand form of the backward sits on a register row with NP <= 4, on one
    with NP = 8 and on the streaming kernel in both storage types"""
    inst = instantiations()
    have = {r[:3] for r in FWD_ROWS} | {r[:3] for r in BWD_ROWS}
    assert len(inst) == 38 and len(set(inst)) == 38, len(inst)
    assert not set(inst) - have, f"compiled kernels no row launches: {sorted(set(inst) - have)}"
    assert have <= set(inst), have - set(inst)
    np8 = lambda r: r[0].endswith(R5)
    reg = [r for r in BWD_ROWS if "reg" in r[0]]
    for form in FORMS:
        assert any(r[7] == form and not np8(r) for r in reg), f"{form}: no row with NP <= 4"
        assert any(r[7] == form and np8(r) for r in reg), f"{form}: no row with NP = 8"
        for kern in ("bwd", "bwd+reduce"):
            assert any(r[7] == form and r[0] == kern for r in BWD_ROWS), f"{form}: no row on {kern}"


def row_id(row):
    route, dt, drop, (C0, C1, P, G), N, draw, silu, *form = row
    return "-".join([route, dt, "drop" if drop else "plain", f"{N}x{P}x{C0}+{C1}g{G}", draw, "silu" if silu else "lin"] + form)


def row_seed(row):
    _, dt, drop, (C0, C1, P, G), N, draw, silu, *form = row
    return 7 * P + 13 * (C0 + C1) + 3 * C1 + N + len(draw) + (100 if dt == "f32" else 0) + (1000 * (1 + FORMS.index(form[0])) if form else 0)


def row_params(row):
    """gamma, beta (fp32 [C]) of a row"""
    C = row[3][0] + row[3][1]
    g = torch.Generator().manual_seed(row_seed(row) + 1)
    return 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def row_keep(row):
    """(keep bool [N][P][C], scale) of a dropout row, (None, 1.0) of a plain one"""
    _, _, drop, (C0, C1, P, G), N, *_ = row
    if not drop:
        return None, 1.0
    keep = torch.from_numpy(keep_mask(KEY, OFFSET, DROP_BASE, N * P * (C0 + C1), RATE).reshape(N, P, C0 + C1))
    return keep, ctl_words(RATE)[1]


def row_addends(row):
    """the tensors a backward row adds to dx, as fp32 [N][P][C] already rounded to the storage type: {"a": ..., "b": ...}; which
    operand each becomes is the form's business (bwd_fields)"""
    _, dt, _, (C0, C1, P, G), N, _, _, form = row
    g = torch.Generator().manual_seed(row_seed(row) + 2)
    q = (lambda t: t.bfloat16().float()) if dt == "bf16" else (lambda t: t)
    a, b = q(torch.randn(N, P, C0 + C1, generator=g)), q(torch.randn(N, P, C0 + C1, generator=g) * 0.5)
    if form == "add1":
        a[..., :C0] = 0          # only the second source's dx takes it
    return {"ow": {}, "sums": dict(a=a), "acc": dict(a=a), "add": dict(a=a), "add1": dict(a=a), "add2": dict(a=a, b=b)}[form]


def row_priors(row):
    """the finite values dgamma, dbeta and sum_all are accumulated onto"""
    C = row[3][0] + row[3][1]
    g = torch.Generator().manual_seed(row_seed(row) + 3)
    return dict(dgamma=torch.randn(C, generator=g), dbeta=torch.randn(C, generator=g), sum_all=torch.randn(C, generator=g) + 2.0)


def fwd_problem(row):
    """-> (x, gamma, beta, refs) of a forward row"""
    route, dt, drop, (C0, C1, P, G), N, draw, silu = row
    x, _ = gn_draw(N, P, C0 + C1, draw, row_seed(row), "fwd", G, dt)
    gamma, beta = row_params(row)
    keep, scale = row_keep(row)
    return x, gamma, beta, gn_fwd_ref(x, gamma, beta, G, EPS, silu, dt, "pivot", keep, scale)


def bwd_problem(row):
    """-> (x, dy, stats fp32 [N][G][2], gamma, beta, addends, priors, refs) of a backward row"""
    route, dt, drop, (C0, C1, P, G), N, draw, silu, form = row
    x, dy = gn_draw(N, P, C0 + C1, draw, row_seed(row), "bwd", G, dt)
    gamma, beta = row_params(row)
    keep, scale = row_keep(row)
    stats = gn_stats_in(x, G, EPS)
    adds, pri = row_addends(row), row_priors(row)
    R = gn_bwd_ref(x, dy, stats[..., 0], stats[..., 1], gamma, beta, G, silu, dt, list(adds.values()), keep=keep, scale=scale,
                   prior=pri if form == "sums" else dict(pri, sum_all=None))
    return x, dy, stats, gamma, beta, adds, pri, R


# ------------------------------------------------------------------ the fused epilogues (csrc/gemm.hip)
# GroupNorm's backward in the epilogue of the data gradient that produces dz (gnb_* on ops.conv_dgrad_t) and its forward in the
# epilogue of the convolution that produces y (gnf_* on ops.conv_fwd): epilogue_tile_gnb / epilogue_tile_gnf on the halo and lin2
# tiles, epilogue_rows on conv_small.  One row per route a qualifying descriptor can take (tests/test_gn_bounds_cpu.py sweeps them
# with mdm_gemm_route_of), at the smallest batch of the sweep.  (route, H, N, C, Cout, k): H x H maps, C channels into the
# convolution, Cout out of it; the GroupNorm has 32 groups of the C (gnb) / Cout (gnf) channels.
FUSED_G = 32
GNB_ROWS = [
    ("conv_small<3,32,16>", 4, 4, 256, 128, 3),
    ("conv_small<4,64,32>", 8, 4, 128, 128, 3),
    ("conv_small<5,64,32>", 4, 4, 128, 128, 3),
    ("halo<64,2,3,32>", 8, 4, 128, 64, 3),
    ("halo<64,2,3,64>", 8, 4, 2048, 64, 3),           # 64-channel groups: the 64-channel small-map tile
    ("halo<64,3,3,32>", 4, 4, 128, 64, 3),
    ("halo<64,3,3,64>", 4, 4, 2048, 64, 3),
    ("lin2<64,64>", 4, 4, 128, 64, 1),
    ("lin2<64,64>", 8, 4, 256, 64, 1),
]
GNF_ROWS = [
    ("conv_small<3,32,16>", 4, 4, 128, 256, 3),
    ("conv_small<4,64,32>", 8, 4, 128, 128, 3),
    ("conv_small<5,64,32>", 4, 4, 128, 128, 3),
    ("halo<64,2,3,32>", 8, 4, 64, 128, 3),
    ("halo<64,2,3,64>", 8, 4, 64, 2048, 3),
    ("halo<64,3,3,32>", 4, 4, 64, 128, 3),
    ("halo<64,3,3,64>", 4, 4, 64, 2048, 3),
    ("lin2<64,64>", 4, 4, 64, 128, 1),
    ("lin2<64,64>", 8, 4, 64, 256, 1),
]
# The fused 1x1 rows again where the generic tile rule of the unfused routes says 128 x 128 (M = 6400 pixels by 512 channels: 50 x 4 =
# 200 such tiles, the smallest count that sets it, at K = 64): the fused epilogues live on the 64 x 64 tile, whose grid is 800
# workgroups.  A launch with the 200 of the other tile leaves three quarters of every output unwritten.
GNB_BIG_ROWS = [
    ("lin2<64,64>", 8, 100, 512, 64, 1),
    ("lin2<64,64>", 4, 400, 512, 64, 1),
]
GNF_BIG_ROWS = [
    ("lin2<64,64>", 8, 100, 64, 512, 1),
    ("lin2<64,64>", 4, 400, 64, 512, 1),
]


def fused_id(row):
    route, H, N, C, Co, k = row
    return f"{route}-{N}x{H}x{H}-{C}to{Co}-k{k}"


def fused_geom(H, N, C, Co, k):
    from mdm import ops
    pd = k // 2
    return ops.ConvGeom(N=N, IH=H, IW=H, C0=C, C1=0, Cout=Co, KH=k, KW=k, pad_t=pd, pad_l=pd, pad_b=pd, pad_r=pd)


def fused_route(kind, H, N, C, Co, k):
    """the gemm route of a fused descriptor of this geometry (dummy non-null pointers: host arithmetic, no launch), or None where
    the geometry does not qualify for the epilogue"""
    from mdm import _lib, ops
    geom = fused_geom(H, N, C, Co, k)
    if kind == "gnf":
        if not ops.conv_fwd_can_fuse_gn(1, geom, FUSED_G):
            return None
        f = ops.conv_fwd_fields(1, geom, 16, None, 16, 16, 16, rowvec=16, rv_ld=Co, resid=16,
                                gnf=dict(out=16, gamma=16, beta=16, stats=16, G=FUSED_G, silu=1))
    else:
        if not ops.conv_dgrad_t_can_fuse_gn_bwd(1, geom, FUSED_G):
            return None
        f = ops.conv_dgrad_t_fields(1, geom, 16, 16, 16, 0, gnb=dict(x=16, stats=16, gamma=16, beta=16, dgamma=16, dbeta=16, G=FUSED_G, silu=1))
    return _lib.route_of(**f)
