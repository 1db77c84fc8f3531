"""The set-moment ABI, its plan and the host half of the Frechet distance without a GPU: include/mdm_moment.h parses to its four
functions and is bound next to the other headers without entering their tables, every `mdm_moment_*` symbol has a kernel-level
test, the plan covers the triangle and the rows once, `frechet_distance` is the scipy.linalg.sqrtm statement, `SetMoments` is
`np.cov`, and a numpy emulation of the stated summation order stays inside the header's bound while every planted fault leaves it.
No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg
import torch

import _moment_ref as MM
from mdm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
MOMENT_HEADER = os.path.join(ROOT, "include", "mdm_moment.h")
_K = "test_moment_kernels_gpu"
COVERAGE = {"mdm_moment_plan": (_K, "mdm_moment_plan"), "mdm_moment_tile_of": (_K, "mdm_moment_tile_of"), "mdm_moment_ws_bytes": (_K, "mdm_moment_ws_bytes"),
            "mdm_moment_accumulate": (_K, "mdm_moment_accumulate")}
PLAN_PARAMS = ["R", "d", "tile", "tiles", "splits", "rows_per_split", "grid", "lds_bytes"]
WS_PARAMS = ["R", "d"]
TILE_OF_PARAMS = ["d", "tile", "I", "J"]
ACC_PARAMS = ["rows", "kind", "lut", "row_ld", "R", "d", "carry", "sum", "outer", "outer_ld", "ws", "ws_bytes", "stream"]
NAMES = ["mdm_moment_plan", "mdm_moment_tile_of", "mdm_moment_ws_bytes", "mdm_moment_accumulate"]
OTHER_PREFIXES = ["mdm_vis_", "mdm_data_", "mdm_interp_", "mdm_ingest_", "mdm_nn_", "mdm_inpaint_", "mdm_metric_", "mdm_restore_"]


# ------------------------------------------------------------------ the tenth header and its tables
def test_the_header_parses_to_exactly_its_names():
    text = open(MOMENT_HEADER).read()
    structs, protos = _lib.parse_header(text)
    assert structs == {} and list(protos) == NAMES
    assert [n for n, _ in protos["mdm_moment_plan"][1]] == PLAN_PARAMS
    assert [n for n, _ in protos["mdm_moment_ws_bytes"][1]] == WS_PARAMS
    assert [n for n, _ in protos["mdm_moment_tile_of"][1]] == TILE_OF_PARAMS
    assert [n for n, _ in protos["mdm_moment_accumulate"][1]] == ACC_PARAMS
    a = dict(protos["mdm_moment_accumulate"][1])
    assert (a["rows"], a["lut"], a["R"], a["d"], a["sum"], a["outer"], a["ws"]) == ("void*", "float*", "int64_t", "int", "double*", "double*", "void*")
    assert [protos[n][0] for n in NAMES] == ["int", "int", "int64_t", "int"]
    assert ACC_PARAMS[-1] == "stream"
    # the other headers' tests read this one: it names none of their prefixes; and it says what the distance is not
    assert not [p for p in OTHER_PREFIXES if p[:-1] in text]
    assert "NOT FID" in text


def test_every_moment_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_moment_[a-z0-9_]+)\s*\(", open(MOMENT_HEADER).read()))
    assert declared == set(_lib.MOMENT_EXPORTS) == set(_lib.MOMENT_PROTOS) == set(_lib.MOMENT_PARAMS) == set(NAMES)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    for name in _lib.MOMENT_EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.MOMENT_PROTOS[name][0] and fn.restype is _lib.MOMENT_PROTOS[name][1], name
    assert _lib.MOMENT_PROTOS["mdm_moment_plan"] == ([i64, i32, vp, vp, vp, vp, vp, vp], i32)
    assert _lib.MOMENT_PROTOS["mdm_moment_ws_bytes"] == ([i64, i32], i64)
    assert _lib.MOMENT_PROTOS["mdm_moment_tile_of"] == ([i32, i64, vp, vp], i32)
    assert _lib.MOMENT_PROTOS["mdm_moment_accumulate"] == ([vp, i32, vp, i64, i64, i32, i32, vp, vp, i64, vp, i64, vp], i32)
    assert os.path.samefile(_lib.MOMENT_HEADER_PATH, MOMENT_HEADER)


def test_the_tables_stay_apart():
    others = [("mdm_hip.h", _lib.EXPORTS), ("mdm_vis.h", _lib.VIS_EXPORTS), ("mdm_data.h", _lib.DATA_EXPORTS),
              ("mdm_interp.h", _lib.INTERP_EXPORTS), ("mdm_ingest.h", _lib.INGEST_EXPORTS), ("mdm_neighbor.h", _lib.NEIGHBOR_EXPORTS),
              ("mdm_inpaint.h", _lib.INPAINT_EXPORTS), ("mdm_metric.h", _lib.METRIC_EXPORTS), ("mdm_restore.h", _lib.RESTORE_EXPORTS)]
    for header, exports in others:
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not [n for n in exports if n.startswith("mdm_moment_")] and "mdm_moment" not in text, header
    assert len(_lib.RESTORE_EXPORTS) == 3 and len(_lib._PROTOS) == 92
    for name in _lib.MOMENT_EXPORTS:
        assert name in _lib._ALL_PROTOS and name in _lib._ALL_PARAMS and name not in _lib._PROTOS
    assert _lib.MOMENT_PARAMS == {"mdm_moment_plan": PLAN_PARAMS, "mdm_moment_tile_of": TILE_OF_PARAMS, "mdm_moment_ws_bytes": WS_PARAMS, "mdm_moment_accumulate": ACC_PARAMS}


def test_call_binds_moment_keywords_against_the_moment_header():
    kw = dict(rows=1, kind=0, lut=None, row_ld=8, R=4, d=8, carry=0, sum=2, outer=3, outer_ld=8, ws=4, ws_bytes=64, stream=None)
    with _lib.Recording() as rec:
        _lib.call("mdm_moment_accumulate", **kw)
        with pytest.raises(TypeError, match="mdm_moment_accumulate"):
            _lib.call("mdm_moment_accumulate", **dict(kw, ld=8))
        with pytest.raises(TypeError, match="mdm_moment_accumulate"):
            _lib.call("mdm_moment_accumulate", **{k: v for k, v in kw.items() if k != "carry"})
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_moment_accumulate", (1, 0, None, 8, 4, 8, 0, 2, 3, 8, 4, 64))]


def test_every_moment_symbol_has_a_kernel_test():
    assert set(COVERAGE) == set(_lib.MOMENT_PROTOS)
    for sym, (mod, mention) in COVERAGE.items():
        text = open(os.path.join(TESTS, mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), f"{mod}.py does not mention {mention}"
        assert "pytest.mark.gpu" in text


# ------------------------------------------------------------------ the plan
PLAN_SHAPES = [(1, 1), (3, 15), (4, 16), (5, 17), (15, 63), (16, 64), (17, 65), (34, 129), (100, 3072), (4096, 192), (30000, 3072),
               (100000, 3072), (7, 8192), (1000003, 64), (513, 2048)]


@pytest.mark.parametrize("R,d", PLAN_SHAPES)
def test_the_plan_covers_the_triangle_and_the_rows_once(R, d):
    import mdm
    p = mdm.moment_plan(R, d)
    assert isinstance(p, mdm.MomentPlan) and p.tile == 64
    T = -(-d // p.tile)
    tiles = range(p.tiles) if p.tiles <= 600 else [0, 1, T - 1, T, 2 * T - 2, 2 * T - 1, p.tiles - 2, p.tiles - 1]
    pairs = [mdm.moment_tile_of(d, t) for t in tiles]                          # the map both launches use: host and device compile one function
    if p.tiles <= 600:
        assert pairs == [(i, j) for i in range(T) for j in range(i, T)]        # row I of the triangle, then J: every tile once
    else:
        assert pairs == [(0, 0), (0, 1), (0, T - 1), (1, 1), (1, T - 1), (2, 2), (T - 2, T - 1), (T - 1, T - 1)]
    pairs = [(i, j) for i in range(T) for j in range(i, T)]
    assert p.tiles == len(pairs) == len(set(pairs)) == T * (T + 1) // 2
    assert {(i, j) for i, j in pairs} | {(j, i) for i, j in pairs} == {(i, j) for i in range(T) for j in range(T)}
    assert p.rows_per_split % 4 == 0 and p.rows_per_split > 0 and p.splits >= 1
    assert (p.splits - 1) * p.rows_per_split < R <= p.splits * p.rows_per_split      # every row in one split, no empty split
    assert p.grid == (p.tiles * p.splits, 4 * p.tiles)                        # the combining launch: strips of 16 rows of a tile
    assert p.ws_bytes == p.splits * (p.tiles * p.tile * p.tile + T * p.tile) * 8
    assert len(p.lds_bytes) == 2 and all(0 < b <= 64 * 1024 for b in p.lds_bytes)
    if p.tiles >= 512:
        assert p.splits == 1
    elif R >= 16 * 512:
        assert p.tiles * p.splits >= 256                                       # enough workgroups for 256 CUs


def test_the_plan_of_the_workload_shapes():
    import mdm
    assert mdm.moment_plan(4096, 192).tiles == 6 and mdm.moment_plan(4096, 192).splits > 40
    assert mdm.moment_plan(30000, 3072).tiles == 1176 and mdm.moment_plan(30000, 3072).splits == 1


def test_plan_and_accumulate_refusals():
    lib = _lib.load()
    err = lambda: lib.mdm_last_error().decode()
    for d, tile, word in ((0, 0, "d"), (8193, 0, "d = 8193"), (129, 6, "tile = 6"), (129, -1, "tile = -1")):
        assert lib.mdm_moment_tile_of(d, tile, None, None) == -1 and word in err(), (d, tile)
    assert lib.mdm_moment_tile_of(129, 5, None, None) == 0
    for R, d, word in ((0, 4, "R"), (-1, 4, "R"), (4, 0, "d"), (4, -3, "d"), (4, 8193, "d = 8193")):
        assert lib.mdm_moment_plan(R, d, None, None, None, None, None, None) == -1 and word in err(), (R, d)
        assert lib.mdm_moment_ws_bytes(R, d) == -1 and word in err()
    assert lib.mdm_moment_plan(4, 8192, None, None, None, None, None, None) == 0             # every output may be NULL
    need = lib.mdm_moment_ws_bytes(8, 5)
    ok = dict(rows=64, kind=0, lut=None, row_ld=5, R=8, d=5, carry=0, sum=128, outer=256, outer_ld=5, ws=1024, ws_bytes=need, stream=None)
    bad = [(dict(rows=None), "rows"), (dict(sum=None), "sum"), (dict(outer=None), "outer"), (dict(ws=None), "ws"),
           (dict(kind=2), "kind"), (dict(kind=-1), "kind"), (dict(kind=1), "lut"), (dict(rows=66), "4-byte"), (dict(R=0), "R"), (dict(d=0), "d"), (dict(d=8193, row_ld=9000, outer_ld=9000), "d = 8193"),
           (dict(row_ld=4), "row_ld"), (dict(outer_ld=4), "outer_ld"), (dict(sum=132), "sum"), (dict(outer=260), "outer"),
           (dict(ws=1028), "ws"), (dict(ws_bytes=need - 8), "ws_bytes")]
    for change, word in bad:                                                   # refused on the host, before any launch: no device needed
        with pytest.raises(RuntimeError, match=word):
            _lib.call("mdm_moment_accumulate", **dict(ok, **change))


# ------------------------------------------------------------------ frechet_distance on host-made moments
def _rows(seed, n, d, shift=0.0, scale=1.0):
    g = np.random.default_rng(seed)
    mix = np.eye(d) + 0.3 * g.normal(size=(d, d)) / np.sqrt(d)               # correlated columns, a well-conditioned map
    return (g.normal(size=(n, d)) @ mix) * scale + shift + g.normal(size=d) * 0.3


def _sqrtm_statement(xa, xb):
    """pytorch-fid's calculate_frechet_distance: diff.diff + tr a + tr b - 2 tr sqrtm(S_a S_b), the real part taken"""
    mu_a, mu_b = xa.mean(0), xb.mean(0)
    S_a, S_b = np.cov(xa, rowvar=False).reshape(xa.shape[1], -1), np.cov(xb, rowvar=False).reshape(xa.shape[1], -1)
    root = scipy.linalg.sqrtm(S_a @ S_b)
    root = root[0] if isinstance(root, tuple) else root
    diff = mu_a - mu_b
    return float(diff @ diff + np.trace(S_a) + np.trace(S_b) - 2.0 * np.trace(root.real)), float(np.trace(S_a) + np.trace(S_b))


def test_diagonal_covariances_have_the_closed_form():
    import mdm
    d, n = 12, 2000
    g = np.random.default_rng(3)
    va, vb = g.uniform(0.2, 3.0, d), g.uniform(0.2, 3.0, d)
    mu_a, mu_b = g.normal(size=d), g.normal(size=d)
    def diag_moments(mu, var):            # outer such that cov(ddof=1) is exactly diag(var) up to rounding
        return mdm.SetMoments.from_arrays(n, n * mu, (n - 1) * np.diag(var) + n * np.outer(mu, mu))
    r = mdm.frechet_distance(diag_moments(mu_a, va), diag_moments(mu_b, vb))
    want = float(((np.sqrt(va) - np.sqrt(vb)) ** 2).sum() + ((mu_a - mu_b) ** 2).sum())
    # the differenced covariance carries u n |mu|^2 / (n - 1) per element; 1e-12 of the traces is far above it and far below a wrong formula
    assert abs(r.distance - want) <= 1e-12 * (r.trace_a + r.trace_b)
    assert abs(r.mean_term - ((mu_a - mu_b) ** 2).sum()) <= 1e-12 and not r.rank_deficient and (r.n_a, r.n_b, r.d) == (n, n, d)
    assert abs(r.cross_term - np.sqrt(va * vb).sum()) <= 1e-12 * (r.trace_a + r.trace_b)


@pytest.mark.parametrize("d,n", [(24, 400), (48, 400), (48, 60)])
def test_full_rank_pairs_equal_the_sqrtm_statement(d, n):
    import mdm
    xa, xb = _rows(10 * d + n, n, d), _rows(10 * d + n + 1, n + 7, d, shift=0.2, scale=1.3)
    a, b = mdm.SetMoments.from_rows(xa), mdm.SetMoments.from_rows(xb)
    want, traces = _sqrtm_statement(xa, xb)
    r, rev = mdm.frechet_distance(a, b), mdm.frechet_distance(b, a)
    print(f"d={d} n={n}: |ours - sqrtm| / traces = {abs(r.distance - want) / traces:.3g}, asymmetry {abs(r.distance - rev.distance) / traces:.3g}")
    assert abs(r.distance - want) <= 1e-12 * traces and not r.rank_deficient
    assert abs(r.trace_a + r.trace_b - traces) <= 1e-12 * traces
    assert abs(r.distance - rev.distance) <= 1e-12 * traces and (rev.trace_a, rev.n_a) == (r.trace_b, r.n_b)      # symmetric in its arguments
    assert r.distance > 1e-3 * traces and r.clipped <= 1e-12 * traces
    # the planted fault: without the mean term the number is off by far more than the bar
    assert abs((r.distance - r.mean_term) - want) > 1e-3 and r.mean_term > 1e-3


@pytest.mark.parametrize("d,n", [(48, 30), (192, 100)])
def test_rank_deficient_pairs(d, n):
    import mdm
    xa, xb = _rows(7 * d + n, n, d), _rows(7 * d + n + 1, n, d, shift=-0.1, scale=0.8)
    a, b = mdm.SetMoments.from_rows(xa), mdm.SetMoments.from_rows(xb)
    want, traces = _sqrtm_statement(xa, xb)
    r = mdm.frechet_distance(a, b)
    same = mdm.frechet_distance(a, mdm.SetMoments.from_rows(xa))
    print(f"d={d} n={n}: |ours - sqrtm| / traces = {abs(r.distance - want) / traces:.3g}, self {abs(same.distance) / (2 * same.trace_a):.3g}")
    assert r.rank_deficient and same.rank_deficient                          # flagged, not raised
    assert abs(r.distance - want) <= 1e-6 * traces
    assert abs(same.distance) <= 1e-6 * (same.trace_a + same.trace_b) and same.mean_term == 0.0


def test_frechet_refusals_name_the_argument():
    import mdm
    a = mdm.SetMoments.from_rows(_rows(1, 10, 4))
    with pytest.raises(TypeError, match="b"):
        mdm.frechet_distance(a, np.zeros(4))
    with pytest.raises(ValueError, match="b"):
        mdm.frechet_distance(a, mdm.SetMoments.from_rows(_rows(2, 10, 5)))
    with pytest.raises(ValueError, match="a: n = 1"):
        mdm.frechet_distance(mdm.SetMoments.from_rows(_rows(2, 1, 4)), a)


# ------------------------------------------------------------------ SetMoments against np.cov
def _cov_bar(x, ddof=1):
    """outer / (n - ddof) and n mu mu^T / (n - ddof) each carry gamma(n + 2) of their magnitude (a sum of n terms, a product, a
    division), np.cov's centred sum as much of a smaller one; four times the larger magnitude covers the difference of the two"""
    n = x.shape[0]
    mu = np.abs(x).mean(0)
    return 4 * MM.gamma(n + 2) * (np.abs(x).T @ np.abs(x) + n * np.outer(mu, mu)) / (n - ddof)


def test_set_moments_cov_merge_save_load(tmp_path):
    import mdm
    x = _rows(5, 300, 17, shift=0.7)
    a, b, whole = mdm.SetMoments.from_rows(x[:120]), mdm.SetMoments.from_rows(x[120:]), mdm.SetMoments.from_rows(x)
    assert (a.n, a.d, a.sum.dtype, a.outer.dtype, a.outer.device.type) == (120, 17, torch.float64, torch.float64, "cpu")
    for ddof in (0, 1):
        want = np.cov(x, rowvar=False, ddof=ddof)
        assert (np.abs(whole.cov(ddof) - want) <= _cov_bar(x, ddof)).all()
    assert (np.abs(whole.mean() - x.mean(0)) <= 4 * MM.gamma(301) * np.abs(x).mean(0)).all()
    # the planted fault: n for n - 1 is far outside the bar
    n, mu = whole.n, whole.mean()
    assert not (np.abs((whole.outer.numpy() - n * np.outer(mu, mu)) / n - np.cov(x, rowvar=False)) <= _cov_bar(x)).all()
    assert not (np.abs(whole.cov(0) - np.cov(x, rowvar=False)) <= _cov_bar(x)).all()
    m = a.merge(b)
    assert m is a and a.n == 300
    assert (np.abs(a.cov() - np.cov(x, rowvar=False)) <= _cov_bar(x)).all() and (np.abs(a.outer.numpy() - whole.outer.numpy()) <= 2 * MM.gamma(300) * (np.abs(x).T @ np.abs(x))).all()
    path = str(tmp_path / "stats.npz")
    a.save(path)
    back = mdm.SetMoments.load(path)
    assert back.n == 300 and torch.equal(back.sum, a.sum) and torch.equal(back.outer, a.outer) and back.d == 17
    with np.load(path) as z:
        assert sorted(z.files) == ["n", "outer", "sum"]
    with pytest.raises(ValueError, match="other"):
        a.merge(mdm.SetMoments(5, "cpu"))
    with pytest.raises(ValueError, match="outer"):
        mdm.SetMoments.from_arrays(3, np.zeros(4), np.zeros((4, 5)))
    with pytest.raises(ValueError, match="no rows"):
        mdm.SetMoments(3, "cpu").mean()


def test_update_refuses_before_any_launch():
    import mdm
    m = mdm.SetMoments(12, "cpu")
    x = torch.zeros(5, 12)
    bad = [(x.double(), TypeError, "rows"), (x.numpy(), TypeError, "rows"), (x[:, :8], ValueError, "rows"), (x.t()[:12], ValueError, "rows"),
           (torch.zeros(5, 12, 2), ValueError, "rows"), (torch.zeros(5, 3, 2, 3), ValueError, "rows"),
           (torch.zeros(2, 3, 4, 2).transpose(2, 3), ValueError, "rows"), (x.to("meta"), ValueError, "rows")]
    for t, err, word in bad:
        with pytest.raises(err, match=word):
            m.update(t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # rows that pass the checks on an object that is not on a GPU
        m.update(x)
    with pytest.raises(TypeError, match="dataset"):
        m.update_dataset(x)
    assert m.n == 0 and not bool(m.outer.any())
    with pytest.raises(ValueError, match="d"):
        mdm.SetMoments(0, "cpu")


# ------------------------------------------------------------------ the stated order inside the bound; planted faults outside it
EMU_CASES = [(1, 1, 16), (3, 2, 16), (5, 17, 16), (17, 5, 16), (34, 9, 16), (49, 3, 16), (200, 17, 48)]


def _touches(fault, R, d, rps, chunks):
    return {"drop_tail": R % 4 != 0, "double_boundary": any(c > rps for c in chunks), "no_mirror": d > 1,
            "carry_overwrite": len(chunks) > 1}[fault]


def _chunked(x, rps, cuts, fault=None):
    """the emulation over the chunks x[cuts[k]:cuts[k + 1]], carried; -> (sum, outer, splits of the largest call, carried calls)"""
    carry, splits = None, 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        carry = MM.emulate(x[lo:hi], rps, carry, fault)
        splits = max(splits, -(-(hi - lo) // rps))
    return carry[0], carry[1], splits, len(cuts) - 2


@pytest.mark.parametrize("R,d,rps", EMU_CASES)
def test_the_stated_order_is_inside_the_bound_and_every_fault_outside(R, d, rps):
    g = np.random.default_rng(1000 * R + d)
    cut_sets = [[0, R]] + ([[0, R // 3, R // 3 + 1 + R // 4, R]] if R >= 5 else [])
    ints = MM.grid_ints(g, R, d)
    ints[ints == 0] = 1                                                        # (a zero row would hide a dropped or doubled row)
    inputs = {"grid": MM.grid_rows(ints), "normal": g.normal(size=(R, d)).astype(np.float32),
              "uniform": g.uniform(-1, 1, size=(R, d)).astype(np.float32)}
    want_s, want_o = MM.grid_moments(ints)
    for name, x in inputs.items():
        ref_s, ref_o, mag_s, mag_o = MM.fsum_moments(x)
        for cuts in cut_sets:
            chunks = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
            s, o, splits, calls = _chunked(x, rps, cuts)
            assert MM.inside(s, ref_s, MM.bound(R, splits, calls, mag_s, ref_s)), (name, cuts)
            assert MM.inside(o, ref_o, MM.bound(R, splits, calls, mag_o, ref_o)) and np.array_equal(o, o.T), (name, cuts)
            if name == "grid":
                assert np.array_equal(s, want_s) and np.array_equal(o, want_o) and np.array_equal(ref_o, want_o)
            for fault in MM.FAULTS:
                if not _touches(fault, R, d, rps, chunks):
                    continue
                fs, fo, _, _ = _chunked(x, rps, cuts, fault)
                caught = not (MM.inside(fs, ref_s, MM.bound(R, splits, calls, mag_s, ref_s)) and
                              MM.inside(fo, ref_o, MM.bound(R, splits, calls, mag_o, ref_o)))
                assert caught, (fault, name, cuts)
                if name == "grid":
                    assert not (np.array_equal(fs, want_s) and np.array_equal(fo, want_o)), (fault, cuts)


def test_numpy_is_far_inside_the_bound():
    """for scale: numpy's own fp64 X^T X on 200 x 17 normal rows sits at 0.06 of n u sum |.|, far inside the bound"""
    x = np.random.default_rng(0).normal(size=(200, 17)).astype(np.float32).astype(np.float64)
    _, ref_o, _, mag_o = MM.fsum_moments(x)
    ratio = float((np.abs(x.T @ x - ref_o) / (200 * MM.U * mag_o)).max())
    print(f"numpy X^T X against fsum: {ratio:.3g} of n u sum |.|")
    assert ratio <= 1.0
