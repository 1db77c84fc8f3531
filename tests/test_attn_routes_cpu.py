"""The kernel choice of mdm_attn_fwd / mdm_attn_bwd, asked for without a GPU (mdm_attn_route_of): the dispatch rule of csrc/attn.hip
written down as a table, the refusals, and every row of test_attn_routes_gpu.ROWS against the route it names."""
import pytest

import test_attn_routes_gpu as R

BF, FP = 1, 0
NAMES = ["fwd<32>", "fwd<64>", "fwd<128>", "fwd<256>", "fwd_dma<64>", "fwd_dma<128>", "fwd_dma<256>",
         "bwd<32>", "bwd<64>", "bwd<128>", "bwd<256>", "bwd_dma<64>", "bwd_dma<128>", "bwd_dma<256>"]

RULE = [      # which, L, C, route
    (0, 272, 64, "fwd<64>"),            # L >= 256 but not a multiple of 64: register-staged, partial last tile
    (0, 256, 32, "fwd<32>"),            # no LDS-DMA kernel at head width 32
    (0, 256, 256, "fwd_dma<256>"),      # cfg3
    (0, 192, 64, "fwd<64>"),            # a multiple of 64 below 256
    (0, 240, 128, "fwd<128>"), (0, 256, 128, "fwd_dma<128>"), (0, 256, 64, "fwd_dma<64>"), (0, 16, 256, "fwd<256>"),
    (0, 8192, 128, "fwd_dma<128>"),     # the forward has no length limit
    (1, 272, 64, "bwd<64>"), (1, 256, 32, "bwd<32>"), (1, 256, 256, "bwd_dma<256>"), (1, 4096, 256, "bwd_dma<256>"),
    (1, 4096, 32, "bwd<32>"), (1, 4080, 128, "bwd<128>"), (1, 64, 128, "bwd<128>"), (1, 320, 64, "bwd_dma<64>"),
]


def test_route_names_are_the_fourteen_fused_kernels():
    from mdm import _lib
    assert _lib.attn_route_names() == NAMES
    assert _lib.load().mdm_attn_route_names(None, 0) == 14


@pytest.mark.parametrize("which,L,C,route", RULE, ids=[f"{'fb'[w]}-{L}-{C}" for w, L, C, _ in RULE])
def test_dispatch_rule(which, L, C, route):
    from mdm import _lib
    before = _lib.attn_last_route()
    assert _lib.attn_route_of(which, BF, L, C) == route
    assert _lib.attn_last_route() == before, "asking for a route changed the record of the last launch"


def test_unsupported_requests_have_no_route():
    from mdm import _lib
    lib = _lib.load()
    for which in (0, 1):
        for dt, L, C in ((FP, 64, 64), (FP, 24, 96), (BF, 24, 64), (BF, 0, 64), (BF, -16, 64), (BF, 64, 96), (BF, 64, 512), (BF, 64, 16)):
            assert _lib.attn_route_of(which, dt, L, C) is None, (which, dt, L, C)
            assert not lib.mdm_attn_supported(dt, L, C)
    assert _lib.attn_route_of(2, BF, 64, 64) is None and _lib.attn_route_of(-1, BF, 64, 64) is None
    # the backward keeps one float (LDS-DMA kernels: two) per query of the image in LDS: L <= 4096; the forward goes on
    assert _lib.attn_route_of(1, BF, 4112, 256) is None and _lib.attn_route_of(0, BF, 4112, 256) == "fwd<256>"
    assert _lib.attn_route_of(1, BF, 4160, 64) is None and _lib.attn_route_of(0, BF, 4160, 64) == "fwd_dma<64>"
    assert lib.mdm_attn_supported(BF, 4112, 256)


def test_refusals_come_back_before_any_device_work():
    """Without a device: a refused request returns its message, and the route record says "none"."""
    from mdm import _lib
    lib = _lib.load()
    assert lib.mdm_attn_fwd(FP, 16, 16, 16, 1, 24, 96, 0.1, None) != 0
    assert "unsupported" in lib.mdm_last_error().decode() and _lib.attn_last_route() == "none"
    assert lib.mdm_attn_bwd(BF, 16, 16, 16, 16, 16, 16, 1, 4112, 64, 0.1, None) != 0
    assert "L=4112 > 4096" in lib.mdm_last_error().decode() and _lib.attn_last_route() == "none"


@pytest.mark.parametrize("row", R.ROWS)
def test_gpu_rows_name_the_route_the_library_takes(row):
    from mdm import _lib
    N, L, C, fwd, bwd = row
    assert (_lib.attn_route_of(0, BF, L, C), _lib.attn_route_of(1, BF, L, C)) == (fwd, bwd)


def test_gpu_rows_reach_every_route():
    assert {r for row in R.ROWS for r in row[3:]} == set(NAMES)
