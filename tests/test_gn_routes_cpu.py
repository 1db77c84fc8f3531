"""The kernel choice of mdm_groupnorm_fwd / mdm_groupnorm_bwd, asked for without a GPU (mdm_gn_route_of): the rule of csrc/norm.hip
(gn_route) written down as a table, the refusals, and every row of test_gn_routes_gpu.ROWS against the routes it names."""
import ctypes

import pytest

import test_gn_routes_gpu as R

BF, FP = 1, 0
NAMES = ["fwd_reg<1,256>", "fwd_reg<2,256>", "fwd_reg<2,512>", "fwd_reg<4,512>", "fwd_reg<8,512>", "fwd",
         "bwd_reg<1,256>", "bwd_reg<2,256>", "bwd_reg<2,512>", "bwd_reg<4,512>", "bwd_reg<8,512>", "bwd", "bwd+reduce"]

# C, P, G, forward bf16, forward fp32, backward bf16 (the fp32 backward is always "bwd+reduce"): np = 16-byte vectors per lane of a
# 256-thread workgroup = ceil(P / floor(256 / (block / 8))), block = 32 channels (16 above 256 pixels) rounded up to whole groups
# and whole vectors; np <= 1, 2, 4, 8, 16 -> <1,256>, <2,256>, <2,512>, <4,512>, <8,512>, above that the streaming kernels
RULE = [
    (32, 16, 32, "fwd_reg<1,256>", "fwd_reg<1,256>", "bwd_reg<1,256>"),         # block 32: 64 pixel lanes
    (32, 128, 32, "fwd_reg<2,256>", "fwd_reg<2,256>", "bwd_reg<2,256>"),
    (32, 256, 32, "fwd_reg<2,512>", "fwd_reg<2,512>", "bwd_reg<2,512>"),        # np 4
    (32, 576, 32, "fwd_reg<4,512>", "fwd_reg<8,512>", "bwd_reg<4,512>"),        # block 16: np 5; fp32 forward widened to 32: np 9
    (128, 1024, 32, "fwd_reg<4,512>", "fwd_reg<8,512>", "bwd_reg<4,512>"),      # np 8; widened: np 16, the last that fits
    (32, 2048, 32, "fwd_reg<8,512>", "fwd_reg<8,512>", "bwd_reg<8,512>"),       # np 16; widened it would be 32: not widened
    (32, 4096, 32, "fwd", "fwd", "bwd"),                                        # np 32
    (96, 64, 32, "fwd_reg<2,256>", "fwd_reg<2,256>", "bwd_reg<2,256>"),         # groups of 3: 48-channel block, 42 pixel lanes
    (384, 1024, 32, "fwd_reg<8,512>", "fwd_reg<8,512>", "bwd_reg<8,512>"),      # groups of 12: 24-channel block, np 13
    (16, 1024, 2, "fwd_reg<4,512>", "fwd_reg<4,512>", "bwd_reg<4,512>"),        # the block is the whole tensor, widened or not
]
REFUSALS = [      # fields, substring of mdm_last_error
    (dict(C0=12), "channel counts must be multiples of 8"),
    (dict(G=0), "not divisible by G"),
    (dict(G=65), "not divisible by G"),
    (dict(C0=40, G=32), "not divisible by G"),
    (dict(C0=72, G=8), "unsupported channel/group combination"),        # one group of 9 channels in whole vectors: a 72-channel block
    (dict(N=0), "bad N/P"),
]


def _routes(**shape):
    from mdm import _lib
    return tuple(_lib.gn_route_of(which, dtype=dt, N=2, **shape) for which, dt in ((0, BF), (0, FP), (1, BF), (1, FP)))


def test_route_names_are_the_thirteen():
    from mdm import _lib
    assert _lib.gn_route_names() == NAMES
    assert _lib.load().mdm_gn_route_names(None, 0) == 13


@pytest.mark.parametrize("C,P,G,fwd_bf,fwd_fp,bwd_bf", RULE, ids=[f"{C}-{P}-{G}" for C, P, G, *_ in RULE])
def test_dispatch_rule(C, P, G, fwd_bf, fwd_fp, bwd_bf):
    from mdm import _lib
    before = _lib.gn_last_route()
    want = (fwd_bf, fwd_fp, bwd_bf, "bwd+reduce")
    assert _routes(C0=C, C1=0, P=P, G=G) == want
    # two sources: only their sum counts; dropout (one source): the kernel of the plain descriptor
    assert _routes(C0=C - 8, C1=8, P=P, G=G) == want and _routes(C0=8, C1=C - 8, P=P, G=G) == want
    assert _routes(C0=C, C1=0, P=P, G=G, rng=16, ctl=16, drop_base=8) == want
    assert _lib.gn_last_route() == before, "asking for a route changed the record of the last launch"


@pytest.mark.parametrize("fields,message", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in f.items()) for f, _ in REFUSALS])
def test_refused_descriptors_have_no_route_and_launch_nothing(fields, message):
    """Without a device: the query answers None, both entry points come back non-zero with today's message, and the route record
    says "none"."""
    from mdm import _lib
    lib = _lib.load()
    f = dict(dtype=BF, N=2, P=16, G=32, C0=64, C1=0, silu=1, eps=1e-6, src0=16, gamma=16, beta=16, stats=16, y=16, dy=16, dst0=16,
             dgamma=16, dbeta=16)
    f.update(fields)
    for which, name in enumerate(("mdm_groupnorm_fwd", "mdm_groupnorm_bwd")):
        for dt in (BF, FP):
            d = _lib._desc(dict(f, dtype=dt, ws=16), _lib.GnDesc)
            assert _lib.gn_route_of(which, **dict(f, dtype=dt)) is None
            assert getattr(lib, name)(ctypes.byref(d), None) == -1
            assert message in lib.mdm_last_error().decode(), (name, lib.mdm_last_error().decode())
            assert _lib.gn_last_route() == "none"
    assert _lib.gn_route_of(2, **dict(f, C0=64, G=32, N=2)) is None and lib.mdm_gn_route_of(0, None) is None


@pytest.mark.parametrize("row", list(R.ROWS), ids=["+".join(map(str, r)) for r in R.ROWS])
def test_gpu_rows_name_the_route_the_library_takes(row):
    C0, C1, P = row
    fwd_bf, fwd_fp, bwd_bf, bwd_fp = _routes(C0=C0, C1=C1, P=P, G=R.G)
    assert {"bf16": (fwd_bf, bwd_bf), "f32": (fwd_fp, bwd_fp)} == R.ROWS[row]


def test_gpu_rows_reach_every_route():
    assert {r for per_dt in R.ROWS.values() for pair in per_dt.values() for r in pair} == set(NAMES)
