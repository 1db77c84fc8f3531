"""The rows of tests/_store_rows.py without a GPU: the numpy fp32 emulation of every summing kernel (sqnorm, the loss word, unit_rows)
stays inside the bounds of tests/_bounds.py on every row, the emulation of every bit-exact kernel meets the reference the GPU tests
hold the kernels to, and each planted fault is rejected by at least one row -- by the same checks the GPU tests apply
(`check_*` of tests/_store_rows.py).  Plus the contract between UNet._build_zero_table and mdm_fill_segments_f32 on a dry net."""
import numpy as np
import pytest
import torch

import _store_rows as SR
from _bounds import col_argmax_want, sampler_update_want, sampler_x0_want, split_t_want, split_want, transpose_want, trunc_bf16
from _store_rows import check_col_argmax, check_loss, check_normalize01, check_sqnorm, check_unit_rows, raises


# ------------------------------------------------------------------ sqnorm
@pytest.mark.parametrize("n", SR.SQNORM_NS)
def test_sqnorm_emulation_inside_the_bound_and_onehot_exact(n):
    g = SR.sqnorm_row(n)
    y, _ = SR.emulate_sqnorm(g.numpy())
    check_sqnorm(f"sqnorm {n}", y, g)
    for p in SR.onehot_positions(n):
        y, _ = SR.emulate_sqnorm(SR.onehot(n, p).numpy())
        assert float(y) == 9.0, (n, p, float(y))


def test_sqnorm_small_call_after_a_large_one():
    big, small = SR.sqnorm_row(SR.SQNORM_NS[-1]), SR.sqnorm_row(SR.SQNORM_NS[6])
    alone, _ = SR.emulate_sqnorm(small.numpy())
    _, stale = SR.emulate_sqnorm(big.numpy())
    after, _ = SR.emulate_sqnorm(small.numpy(), stale)
    assert np.float32(alone).tobytes() == np.float32(after).tobytes()
    wrong, _ = SR.emulate_sqnorm(small.numpy(), stale, fault="final_reads_all")
    assert raises(check_sqnorm, "stale", wrong, small)


@pytest.mark.parametrize("fault", SR.SQNORM_FAULTS[:3])
def test_sqnorm_onehot_rows_reject_a_missing_element(fault):
    """each fault loses an element that one of the one-hot rows holds: 0.0 where 9.0 is due"""
    hit = 0
    for n in SR.SQNORM_NS:
        for p in SR.onehot_positions(n):
            y, _ = SR.emulate_sqnorm(SR.onehot(n, p).numpy(), fault=fault)
            hit += float(y) != 9.0
    assert hit >= 1, fault


# ------------------------------------------------------------------ cast, transpose, split
@pytest.mark.parametrize("n", SR.FLAT_NS[:3])
def test_cast_edges_and_the_truncating_cast(n):
    x = SR.cast_row(n)
    want = SR.cast_want(x)
    assert SR.cast_matches(want, want, x)
    k = min(n, len(SR.CAST_EDGES))
    known = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80, 0x00000001: 0x0000, 0x00008000: 0x0000,
             0x00018000: 0x0002, 0x7F7FFFFF: 0x7F80, 0x80000000: 0x8000}
    for src, bits in zip(SR.CAST_EDGES[:k], want[:k].tolist()):
        if src in known:
            assert bits & 0xFFFF == known[src], (hex(src), hex(bits & 0xFFFF))
    if n > 1:
        assert not SR.cast_matches(SR.cast_want(x, "truncate"), want, x)
        assert torch.equal(SR.cast_want(x, "truncate")[~torch.isnan(x)].view(torch.bfloat16), trunc_bf16(x.double())[~torch.isnan(x)])


def test_transpose_emulation_and_its_faults():
    filters, n = SR.pack_filters(SR.TRANSPOSE_FILTERS, SR.TRANSPOSE_GAP_AFTER)
    g = torch.Generator().manual_seed(4)
    Pb = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g, dtype=torch.int32).to(torch.int16)
    want = transpose_want(Pb, filters)

    def run(fault):
        PT = np.full(n, 0x7FE5, np.int16)
        SR.emulate_transpose(Pb.numpy(), PT, SR.transpose_tiles(filters, fault))
        PT = torch.from_numpy(PT)
        inside = torch.zeros(n, dtype=torch.bool)
        bad = []
        for off, t, co, ci in filters:
            inside[off:off + t * co * ci] = True
            if not torch.equal(PT[off:off + t * co * ci], want[off].reshape(-1)):
                bad.append((t, co, ci))
        assert bool((PT[~inside] == 0x7FE5).all())
        return bad
    assert run(None) == []
    assert (9, 8, 128) in run("tap0_offset") and (1, 8, 8) not in run("tap0_offset")
    assert set(run("skip_partial_tile")) == {(1, 8, 8), (9, 8, 128), (9, 128, 8), (1, 40, 24), (9, 72, 136), (1, 200, 72)}


def test_split_rows_reach_the_second_trip():
    filters, n, P = SR.split_problem()
    segs = [(off, t * co * ci) for off, t, co, ci in filters]
    assert max(ln for _, ln in segs) == 589824 > SR.SPLIT_TRIP and (1, 32, 32) in [f[1:] for f in filters]
    want, wrong = split_want(P, segs), SR.emulate_split(P, segs, "no_second_trip")
    assert sum(not torch.equal(want[o], wrong[o]) for o, _ in segs) == 1
    wt = split_t_want(P, filters)
    assert all(wt[off].numel() == 2 * t * co * ci for off, t, co, ci in filters)


# ------------------------------------------------------------------ loss
@pytest.mark.parametrize("row", SR.LOSS_ROWS, ids=[SR.loss_id(r) for r in SR.LOSS_ROWS])
def test_loss_emulation_inside_the_bound(row):
    T = SR.loss_problem(row)
    check_loss(SR.loss_id(row), row, T, *SR.emulate_loss(row, T))


def test_loss_faults_are_rejected():
    hit = dict.fromkeys(SR.LOSS_FAULTS, 0)
    for row in SR.LOSS_ROWS:
        if row[2] > 40:
            continue
        T = SR.loss_problem(row)
        for f in SR.LOSS_FAULTS:
            hit[f] += raises(check_loss, f, row, T, *SR.emulate_loss(row, T, f))
    assert all(hit.values()), hit
    assert hit["no_gscale"] == sum(r[2] <= 40 for r in SR.LOSS_ROWS)


# ------------------------------------------------------------------ sampler
@pytest.mark.parametrize("shape", SR.SAMPLER_SHAPES[:3])
def test_sampler_emulations_and_their_faults(shape):
    N, C, H, W, Cp = shape
    for dt, ws, _, _ in SR.SAMPLER_FORMS:
        T = SR.sampler_problem(shape, dt)
        want = sampler_x0_want(T["pred"], T["x_in"], T["s"] if ws else None, C)
        got = SR.emulate_sampler_x0(T, C, ws)
        assert all(SR.same_f32(a, b) for a, b in zip(got, want)) and not any(bool(torch.isnan(a).any()) for a in got)
        if ws:
            assert not SR.same_f32(SR.emulate_sampler_x0(T, C, ws, "x0_plus_s")[2], want[2])
    T = SR.sampler_problem(shape, "f32")
    for mom, _ in SR.UPDATE_FORMS:
        want = sampler_update_want(T["d_t"], T["d_next"], T["x_t"], mom)
        assert SR.same_f32(SR.emulate_sampler_update(T, mom)[1], want[1])
        assert not SR.same_f32(SR.emulate_sampler_update(T, mom, "momentum_inverted")[1], want[1])


# ------------------------------------------------------------------ evaluation kernels
@pytest.mark.parametrize("E", SR.NORM_ES)
def test_normalize01_emulation_and_the_batch_wide_minimum(E):
    x = SR.normalize_problem(E)
    y = SR.emulate_normalize01(x)
    check_normalize01(f"normalize01 {E}", y, x)
    k = SR.NORM_KINDS.index
    assert not y[k("constant")].any() and not y[k("nan")].any()
    if E > 1:
        assert float(y[k("max_last"), -1]) == 1.0 and float(y[k("min_last"), -1]) == 0.0 and float(y[k("plain")].max()) == 1.0
        assert raises(check_normalize01, "batch_min", SR.emulate_normalize01(x, "batch_min"), x)


@pytest.mark.parametrize("R", SR.UNIT_RS)
@pytest.mark.parametrize("D", SR.UNIT_DS)
def test_unit_rows_emulation_inside_the_bound(D, R):
    x = SR.unit_problem(R, D)
    check_unit_rows(f"unit_rows {R}x{D}", SR.emulate_unit_rows(x, SR.UNIT_EPS), x, SR.UNIT_EPS)
    assert raises(check_unit_rows, "no_last_element", SR.emulate_unit_rows(x, SR.UNIT_EPS, "no_last_element"), x, SR.UNIT_EPS)
    if R >= 5:
        assert raises(check_unit_rows, "no_eps", SR.emulate_unit_rows(x, SR.UNIT_EPS, "no_eps"), x, SR.UNIT_EPS)


def test_col_argmax_emulation_and_its_faults():
    hit = dict.fromkeys(SR.ARGMAX_FAULTS, 0)
    seen = set()
    for M in SR.ARGMAX_MS:
        for B in SR.ARGMAX_BS:
            S, plan = SR.argmax_problem(M, B)
            seen |= set(plan)
            check_col_argmax(f"col_argmax {M}x{B}", *SR.emulate_col_argmax(S), S)
            for f in SR.ARGMAX_FAULTS:
                hit[f] += raises(check_col_argmax, f, *SR.emulate_col_argmax(S, f), S)
            if "all_neg_inf" in plan:
                v, i = SR.emulate_col_argmax(S, "finite_start")
                assert int(i[plan["all_neg_inf"]]) == SR.BIG_IDX
                assert int(col_argmax_want(S)[1][plan["all_neg_inf"]]) == 0
    assert all(hit.values()), hit
    assert seen == {"tie_same_lane", "tie_neighbours", "tie_5_700", "tie_two_waves", "all_equal", "all_negative", "all_neg_inf", "one_nan",
                    "two_nan", "all_nan"}


# ------------------------------------------------------------------ the zero table of a dry net
@pytest.mark.parametrize("which", ["none", "filters", "all"])
def test_zero_table_rows_are_what_fill_segments_takes(which):
    import mdm
    from golden.make_golden import TINY
    net = mdm.UNet(TINY, 1, 16, 16, _dry=True)
    ent = net.store.entries
    net.device = "cpu"
    net.overwritten = {"none": set(), "filters": {k for k, e in ent.items() if e.kind in ("conv", "convlin")}, "all": set(ent)}[which]
    net._build_zero_table()
    if which == "all":
        assert net.zero_table is None and net.zero_floats == 0
        return
    rows = net.zero_table.tolist()
    SR.check_zero_table(rows, ent, net.overwritten)
    assert net.zero_floats == sum(n for _, n in rows)
    assert any(n == 4096 for _, n in rows) or which == "filters"
    with pytest.raises(AssertionError):
        SR.check_zero_table(rows[:-1], ent, net.overwritten)
    with pytest.raises(AssertionError):
        SR.check_zero_table(rows + [rows[0]], ent, net.overwritten)
