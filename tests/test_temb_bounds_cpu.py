"""Without a GPU: every row of tests/_temb_rows.py (run on the GPU by tests/test_temb_bounds_gpu.py) names the kernel the library
takes for it (mdm_skinny_route_of is host arithmetic) and the kernel a Python restatement of the rule takes, the rows reach all
eight compiled skinny kernels in every state of their look-ahead loops and with every operand form, every refusal row is refused,
and no load of any row leaves its operand."""
import pytest

import _temb_rows as R

ALL = [(0, r) for r in R.FWD_ROWS] + [(1, r) for r in R.BWD_ROWS]
IDS = [R.fwd_id(r) for r in R.FWD_ROWS] + [R.bwd_id(r) for r in R.BWD_ROWS]


@pytest.mark.parametrize("which,row", ALL, ids=IDS)
def test_rows_name_the_route_the_library_takes(which, row):
    from mdm import _lib
    has_t = bool(which == 0 and row.temb)
    assert _lib.skinny_route_of(which, row.M, row.N, row.K, has_t) == row.route == R.route_rule(which, row.M, row.N, row.K, has_t)
    assert _lib.load().mdm_skinny_supported(row.M, row.N, row.K, row.splits if which else 1) == 1


def test_rule_restated_in_python_matches_the_library_everywhere():
    from mdm import _lib
    for which in (0, 1):
        for has_t in (0, 1):
            for M in (0, 1, 2, 16, 31, 32, 33, 64, 127, 128, 129, 256):
                for N in (0, 8, 16, 24, 32, 2032, 2048, 2064, 2080, 4992, 5008):
                    for K in (0, 32, 64, 96, 128, 512, 4992):
                        assert _lib.skinny_route_of(which, M, N, K, has_t) == R.route_rule(which, M, N, K, has_t), (which, M, N, K, has_t)


def test_rows_reach_all_eight_kernels_and_timesteps_never_take_two_column_blocks():
    from mdm import _lib
    names = _lib.skinny_route_names()
    assert len(names) == 8 and len(set(names)) == 8
    assert {r.route for r in R.FWD_ROWS} | {r.route for r in R.BWD_ROWS} == set(names)
    assert not any("temb" in n and ",2" in n for n in names)
    wide = [r for r in R.FWD_ROWS if r.temb and r.N >= 2048 and r.N % 32 == 0]
    assert wide and all(r.route == "nt<2,1,temb>" for r in wide)


def test_rows_cover_the_edges_of_every_kernel():
    """per instantiation: every M edge of its MB, every K (state of the look-ahead loop), every operand form and pitch"""
    fwd = {}
    for r in R.FWD_ROWS:
        fwd.setdefault(r.route, []).append(r)
    for route, rows in fwd.items():
        mb = int(route[3])
        assert {r.M for r in rows} == {m for m in R.MS if (m <= 32) == (mb == 2)}, route
        assert {r.K for r in rows} == set(R.HIDS if "temb" in route else R.KS[mb]), route
        assert {r.bias for r in rows} == {r.act for r in rows} == {0, 1}, route
        assert {r.pad for r in rows} == set(R.PADS), route
        if "temb" in route:
            assert {r.emb for r in rows} == {0, 1} and {r.variant for r in rows} == set(R.VARIANTS), route
            assert {r.N for r in rows} >= {16, 48, 80}
        elif route.endswith(",2>"):
            assert {r.N for r in rows} == {2048, 2080}
        else:
            assert {r.N for r in rows} == {16, 48, 80, 2064}
    assert any(r.temb and r.M == 17 for r in R.FWD_ROWS) and any(r.temb and r.M == 33 for r in R.FWD_ROWS)
    bwd = {}
    for r in R.BWD_ROWS:
        bwd.setdefault(r.route, []).append(r)
    for route, rows in bwd.items():
        mb = int(route[3])
        assert {r.M for r in rows} == {m for m in R.MS if (m <= 32) == (mb == 2)}, route
        assert {r.splits for r in rows} == set(R.SPLITS) and {r.N for r in rows} == set(R.BWD_NS), route
        assert {r.K // r.splits for r in rows} == {64, 128} and {r.pad for r in rows} == set(R.PADS), route
        assert {r.pre for r in rows if r.splits == 1} == {0, 1} and {r.pre for r in rows if r.splits > 1} == {0, 1}, route


@pytest.mark.parametrize("which,M,N,K,splits", R.REFUSALS)
def test_refusal_rows_are_refused(which, M, N, K, splits):
    from mdm import _lib
    assert _lib.load().mdm_skinny_supported(M, N, K, splits) == 0
    if splits == 1:
        assert _lib.skinny_route_of(which, M, N, K, 0) is None and R.route_rule(which, M, N, K, 0) is None
        assert _lib.skinny_route_of(0, M, N, K, 1) is None
    assert _lib.skinny_route_of(1, 4, 16, 64, 1) is None          # the backward takes no timesteps
    assert _lib.skinny_route_of(2, 4, 16, 64, 0) is None


@pytest.mark.parametrize("which,row", ALL, ids=IDS)
def test_no_load_leaves_its_operand(which, row):
    """the clamped-address loads (`n < N ? n : N - 1`, `m < M ? m : M - 1`, dead chunks at the wave's first chunk, the four k-rows
    of skinny_nn_kernel), restated as host arithmetic over every lane of every workgroup: inside [0, rows * pitch - pad)"""
    reads = R.clamped_reads(row)
    if which:
        size = dict(W=(row.K - 1) * (row.N + row.pad) + row.N, dy=(row.M - 1) * (row.K + row.pad) + row.K)
    else:
        size = dict(W=(row.N - 1) * (row.K + row.pad) + row.K, x=(row.M - 1) * (row.K + row.pad) + row.K)
    assert set(reads) == set(size) - ({"x"} if (not which and row.temb) else set())
    for name, (lo, hi) in reads.items():
        assert 0 <= lo and hi < size[name], (name, lo, hi, size[name])
        assert lo == 0 and hi == size[name] - 1, (name, lo, hi, size[name])      # and every element is reached


def test_colsum_rows_cover_every_operand_form():
    seen = {dt: set() for dt in ("f32", "bf16")}
    for dt in seen:
        for C in R.COLSUM_CS:
            rows = R.colsum_rows(dt, C)
            assert {(P, N) for P, N, *_ in rows} == {(P, N) for P in R.COLSUM_PS for N in R.COLSUM_NS}
            seen[dt] |= {tuple(r[2:]) for r in rows}
            assert {r[2] for r in rows} == {None, "dense", "pitched"}, (dt, C)
        assert seen[dt] == set(R.COLSUM_FORMS), dt
