"""Without a GPU: every row of tests/_gn_rows.py (run on the GPU by tests/test_gn_bounds_gpu.py) names the kernel the library takes
for it (mdm_gn_route_of is host arithmetic), the rows cover the 38 compiled standalone GroupNorm kernels and every operand form,
and the fused rows cover every route a qualifying fused GroupNorm descriptor can take (mdm_gemm_route_of)."""
import pytest

import _gn_rows as R


@pytest.mark.parametrize("row", R.FWD_ROWS + R.BWD_ROWS, ids=[R.row_id(r) for r in R.FWD_ROWS + R.BWD_ROWS])
def test_rows_name_the_route_the_library_takes(row):
    from mdm import _lib
    route, dt, drop, (C0, C1, P, G), N = row[:5]
    fields = dict(dtype=R.DT[dt], N=N, P=P, G=G, C0=C0, C1=C1)
    if drop:
        assert C1 == 0, "a dropout site has one source"
        fields.update(rng=16, ctl=16, drop_base=R.DROP_BASE)
    assert _lib.gn_route_of(0 if len(row) == 7 else 1, **fields) == route


def test_every_instantiation_and_operand_form_has_a_row():
    R.rows_cover_every_instantiation()


def test_rows_cover_the_edges():
    """the shapes the kernels' guards and tails need: P below the pixel lanes, a partial last vector, a partial last channel block
    with G != 32, a block that straddles the sources, a block that is the whole tensor, and image order (N = 3) on every sums row"""
    shapes = {r[3] for r in R.FWD_ROWS} & {r[3] for r in R.BWD_ROWS}
    for s in (R.S16, R.S576, R.S72, R.S2SRC, R.S16C, R.S96, R.S384, R.S4096):
        assert s in shapes, s
    assert all(r[4] == 3 for r in R.BWD_ROWS if r[7] == "sums")
    assert {r[5] for r in R.FWD_ROWS} == {"plain", "spiked", "offset", "constant"}


SWEEP = [(H, N, C, Co, k) for H in (4, 8) for N in (4, 8, 12, 16, 32) for C in (64, 128, 256, 512, 2048)
         for Co in (64, 128, 256, 512, 2048) for k in (1, 3)]


@pytest.mark.parametrize("kind,rows", [("gnb", R.GNB_ROWS), ("gnf", R.GNF_ROWS)], ids=["gnb", "gnf"])
def test_fused_rows_reach_every_route_a_fused_descriptor_can_take(kind, rows):
    """4x4 and 8x8 maps, 1x1 and 3x3 filters, every batch and channel count of the presets: the routes a descriptor that qualifies
    for the fused GroupNorm epilogue takes, against the routes the GPU rows name (and each row against the route the library
    names for it)."""
    for row in rows:
        assert R.fused_route(kind, *row[1:]) == row[0], row
    reachable = {R.fused_route(kind, *s) for s in SWEEP} - {None}
    assert {"halo<64,2,3,64>", "halo<64,3,3,64>"} <= reachable
    missing = reachable - {row[0] for row in rows}
    assert not missing, f"{kind}: routes of fused descriptors that no GPU row reaches: {sorted(missing)}"
    # the smallest batch of the sweep keeps every route
    assert all(row[2] == 4 for row in rows)


@pytest.mark.parametrize("kind,rows", [("gnb", R.GNB_BIG_ROWS), ("gnf", R.GNF_BIG_ROWS)], ids=["gnb", "gnf"])
def test_big_fused_rows_take_the_64_tile_and_its_grid(kind, rows):
    """The fused 1x1 rows at M = 6400, N = 512, where an unfused convolution of the same shape takes 128 x 128 tiles: they qualify,
    name lin2<64,64>, and the launch is planned on that route's own tile -- 100 x 8 workgroups."""
    from mdm import _lib, ops
    assert len(rows) == 2 and {row[1] for row in rows} == {4, 8}
    for route, H, N, C, Co, k in rows:
        assert route == "lin2<64,64>" and R.fused_route(kind, H, N, C, Co, k) == route, (kind, H, N)
        g = R.fused_geom(H, N, C, Co, k)
        if kind == "gnf":
            plain = ops.conv_fwd_fields(1, g, 16, None, 16, 16, 16)
            fused = ops.conv_fwd_fields(1, g, 16, None, 16, 16, 16, gnf=dict(out=16, gamma=16, beta=16, stats=16, G=R.FUSED_G, silu=1))
        else:
            plain = ops.conv_dgrad_t_fields(1, g, 16, 16, 16, 0)
            fused = ops.conv_dgrad_t_fields(1, g, 16, 16, 16, 0, gnb=dict(x=16, stats=16, gamma=16, beta=16, dgamma=16, dbeta=16,
                                                                          G=R.FUSED_G, silu=1))
        assert _lib.route_of(**plain) == "lin2<128,128>" and _lib.launch_of(**plain)[:2] + _lib.launch_of(**plain)[4:] == (200, 1, 128, 128)
        assert _lib.launch_of(**fused)[:2] + _lib.launch_of(**fused)[4:] == (800, 1, 64, 64)
