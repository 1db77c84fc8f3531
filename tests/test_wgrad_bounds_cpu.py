"""The rows of tests/_wgrad_rows.py reach what test_wgrad_bounds_gpu.py relies on, shown without a GPU:

  * the schedule of every (group, queue count) through mdm_wgrad_group_schedule: the form, which members the nine-tap kernel
    takes, where tiles are cut.  These are conditions on the INPUTS of the GPU test: if a change of plan_wgrad_group breaks one,
    the member is chosen again, the condition stays;
  * the (split count, workspace bytes) of every mdm_conv_wgrad_split row through mdm_conv_wgrad_split_plan, and its refusals;
  * the criterion notices: the gradient a wrong edge mask, a dropped or doubled slab, a wrong source at a concat boundary, a wrong
    upsample row or a bias gradient short of one part would give (wgrad_flat, fp64) fails the per-element bound or is at least
    10x over the rel-L2 bar, at the small shapes of the rows.
"""
import ctypes

import pytest
import torch

import _wgrad_rows as R
from _bounds import check, conv_wgrad_ref, violations
from _wgrad_rows import DESC, GK_TAPS, K0, K1, KIND, SLOT


def _schedule(monkeypatch, name, n_cu, min_share=0):
    from mdm import _lib
    if min_share is None:
        monkeypatch.delenv("MDM_TAPS_MIN_SHARE", raising=False)
    else:
        monkeypatch.setenv("MDM_TAPS_MIN_SHARE", str(min_share))
    fields = R.group_fields(name)
    for i, f in enumerate(fields):
        assert _lib.wgrad_group_accepts(**{k: v for k, v in f.items() if k != "_flops"}), (name, i)
    rows, need, form = _lib.wgrad_group_schedule(fields, n_cu)
    R.slots_at(len(fields), rows, need, ctypes.sizeof(_lib.GemmDesc))          # the documented layout adds up to `need`
    return rows, form


def _nine(rows):
    return sorted({d for d, _ in R.tiles_of(rows)})


@pytest.mark.parametrize("name,n_cu,route", R.MERGED_RUNS)
def test_merged_runs_are_one_persistent_launch_with_whole_partitions(name, n_cu, route, monkeypatch):
    rows, form = _schedule(monkeypatch, name, n_cu)
    assert form == 1
    members = R.GROUPS[name]
    assert all(0 <= r[0] < n_cu for r in rows) and len(rows) % n_cu == 0
    for (d, tile), parts in R.tiles_of(rows).items():
        assert parts[0][K0] == 0 and parts[-1][K1] == R.slabs(members[d]), (d, tile)
        assert all(a[K1] == b[K0] for a, b in zip(parts, parts[1:]))
        assert (len(parts) == 1) == (parts[0][SLOT] == 0)
    has_reduce = any(m["splitk"] > 1 for i, m in enumerate(members) if i not in _nine(rows))
    assert route == "wgrad_taps_group" + ("+splitk" if has_reduce else "")


def test_edges_at_8_queues_has_no_slot(monkeypatch):
    rows, _ = _schedule(monkeypatch, "edges", 8)
    assert _nine(rows) == list(range(7)), "every member of `edges` is a nine-tap member"
    assert {r[KIND] for r in rows if r[DESC] >= 0} == {GK_TAPS}
    assert all(r[SLOT] == 0 for r in rows) and R.cuts_of(rows) == {}


def test_edges_at_24_queues_cuts_the_edge_members(monkeypatch):
    rows, _ = _schedule(monkeypatch, "edges", 24)
    members, cuts = R.GROUPS["edges"], R.cuts_of(rows)
    assert _nine(rows) == list(range(7))
    ups = [i for i, m in enumerate(members) if m["ups"]]
    oh2 = [i for i, m in enumerate(members) if R.geom(m).OH == 2]
    thin = [i for i, m in enumerate(members) if 8 in (m["C0"], m["Co"])]
    assert (len(ups), len(oh2), len(thin)) == (1, 1, 2)
    assert set(ups + oh2 + thin) <= set(cuts), cuts
    # every member of at least 16 slabs is cut, in two or four
    for i, m in enumerate(members):
        assert (i in cuts) == (R.slabs(m) >= 16), (i, cuts)
        assert len(cuts.get(i, [])) in (0, 1, 3)
    # a cut inside an image: the halo blocks k0 - 1 and k1 of a part are pixels of the same image
    inside = [(i, k) for i, ks in cuts.items() for k in ks if R.slabs_per_image(members[i]) > 1 and k % R.slabs_per_image(members[i])]
    assert inside and any(i == ups[0] for i, _ in inside), inside
    assert any(members[i]["dbias"] for i in cuts), "a cut tile with the BIAS body"


def test_wide_at_8_queues_is_cut_only_inside_the_one_image(monkeypatch):
    rows, _ = _schedule(monkeypatch, "wide", 8)
    assert _nine(rows) == [0, 1, 2]
    assert R.geom(R.GROUPS["wide"][0]).OW == 64 and R.GROUPS["wide"][0]["N"] == 1
    assert R.cuts_of(rows) == {0: [14, 28, 42, 56]}            # rows 14, 28, 42, 56 of the 64 x 64 image


def test_wide_at_16_queues_cuts_every_member(monkeypatch):
    rows, _ = _schedule(monkeypatch, "wide", 16)
    assert sorted(R.cuts_of(rows)) == [0, 1, 2]
    assert any(m["dbias"] for m in R.GROUPS["wide"])


def test_riders_holds_every_kind_and_cuts_the_dbias_and_the_short_tile(monkeypatch):
    rows, _ = _schedule(monkeypatch, "riders", 8)
    members, cuts = R.GROUPS["riders"], R.cuts_of(rows)
    assert tuple(_nine(rows)) == R.RIDERS_NINE_TAP
    assert {r[KIND] for r in rows if r[DESC] >= 0} == {0, 1, 2, 3}
    db = [i for i in cuts if members[i]["dbias"]]
    short = [i for i in cuts if members[i]["Co"] < R.TAPS_BM]
    assert db and short, cuts
    assert 8 in cuts[db[0]] and R.slabs_per_image(members[db[0]]) == 16          # mid-image
    assert members[short[0]]["splitk"] == 2, "its split is folded to one: the nine-tap kernel took it"
    # the per-tap members ride in the same table, the split one with all its k-ranges
    per_tap = {r[DESC] for r in rows if r[DESC] >= 0 and r[KIND] != GK_TAPS}
    assert per_tap == set(range(7)) - set(R.RIDERS_NINE_TAP)
    assert {members[i]["acc"] for i in per_tap if members[i]["splitk"] > 1} == {1}


@pytest.mark.parametrize("name,route", R.PER_TAP_RUNS)
@pytest.mark.parametrize("n_cu", [8, 64, 256, 304])
def test_per_tap_runs_are_form_0_on_any_device(name, route, n_cu, monkeypatch):
    rows, form = _schedule(monkeypatch, name, n_cu, min_share=None)
    assert form == 0 and all(r[KIND] != GK_TAPS for r in rows)
    assert route == "wgrad_group+splitk" and any(m["splitk"] > 1 for m in R.GROUPS[name])
    if name == "riders_all_per_tap":
        assert {m["acc"] for m in R.GROUPS[name] if m["splitk"] > 1} == {0, 1}, "the batched reduce with acc0 = 0 and 1"
        assert any(m["dbias"] for m in R.GROUPS[name])


# ------------------------------------------------------------------ mdm_conv_wgrad_split
@pytest.mark.parametrize("name", list(R.SPLIT_ROWS))
def test_split_plan(name):
    from mdm import _lib
    row = R.SPLIT_ROWS[name]
    f = R.split_fields(row)
    assert _lib.wgrad_split_plan(**f) == row["plan"]
    assert ("+splitk" in row["route"]) == (row["plan"][0] > 1)
    assert ("<128>" in row["route"]) == (f["M"] >= 128 and f["N"] >= 128), "the tile is implied by M, N"
    assert row["plan"][1] <= row["ws_bytes"] or row["plan"][1] == 0


def test_split_rows_reach_the_edges_they_name():
    rows = R.SPLIT_ROWS
    K = lambda n: R.split_fields(rows[n])["K"]
    assert [K(n) for n in ("bt64", "k_tail_48", "k_tail_80", "k_16", "k_16_1x1")] == [192, 48, 80, 16, 16]
    f = R.split_fields(rows["bt64_ragged_splitk"])
    assert (f["M"], f["N"]) == (64, 96)                                 # second n-tile: 32 of 64 columns
    f = R.split_fields(rows["bt128_ragged"])
    assert (f["M"] % 128, f["N"] % 128) == (32, 8)
    assert K("explicit3") == 128 + 128 + 64
    slab = 9 * 64 * 64 * 4
    assert rows["ws_cap"]["ws_bytes"] == 2 * slab and rows["ws_below_two"]["ws_bytes"] == 2 * slab - 4
    f = R.split_fields(rows["non_dense"])
    assert f["ldd0"] == 80 > f["N"] and f["dtap"] == 64 * 80 and f["ws_bytes"] >= 2 * slab
    assert R.split_fields(rows["pitched_lda"])["lda"] == 96 and R.split_fields(rows["pitched_ld0"])["ld0"] == 72
    g = R.geom(rows["concat_36_28"]["m"])
    assert 0 < g.C0 < 64 < g.Cin + 1 and g.C0 % 16, "the source boundary lies inside the one 64-column tile, not at a multiple of 16"


@pytest.mark.parametrize("bad", ["M6", "C06", "dbias"])
def test_split_refusals_without_a_device(bad):
    from mdm import _lib
    f = R.split_fields(dict(R.SPLIT_ROWS["bt64"], m=R.M(3, 8, 8, 6 if bad == "C06" else 64, 0, 6 if bad == "M6" else 64)))
    if bad == "dbias":
        f["dbias"] = 16
    with pytest.raises(RuntimeError, match="wgrad_split"):
        _lib.wgrad_split_plan(**f)


# ------------------------------------------------------------------ the criterion notices
NINE_TAP = R.GROUPS["edges"][2]            # (4, 16, 8, 40, 24, 128): concat inside a tile, four images, two slabs per image
NINE_TAP_UPS = R.M(2, 4, 4, 64, 0, 64, ups=1)
NINE_TAP_DBIAS = R.M(2, 16, 16, 64, 0, 64, dbias=1)
SPLIT = R.SPLIT_ROWS["concat_36_28"]["m"]
SPLIT_UPS = R.SPLIT_ROWS["ups"]["m"]


def _rejected(name, y, ref, mag, K, split, bar):
    """True if `y` fails the per-element bound or is at least 10x over the bar."""
    rel = float((y - ref).norm() / ref.norm())
    outside = bool(violations(y, ref, R.bound_of(ref, mag, K, split)).any())
    if not outside:
        check(name, y, ref, mag, K, "f32", split=split)             # the same bound as `check` holds: this does not raise
    return outside or rel >= 10 * bar


def test_bound_of_is_the_bound_check_applies():
    ref, mag = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64), torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64)
    for split in (False, True):
        b = R.bound_of(ref, mag, 512, split)
        check("inside", ref + 0.999 * b, ref, mag, 512, "f32", split=split)
        for i in range(3):
            y = ref.clone()
            y[i] += 1.001 * b[i]
            with pytest.raises(AssertionError):
                check("outside", y, ref, mag, 512, "f32", split=split)


@pytest.mark.parametrize("m", [NINE_TAP, NINE_TAP_UPS, SPLIT, SPLIT_UPS], ids=["concat", "ups", "split_concat", "split_ups"])
def test_wgrad_flat_without_a_fault_is_the_reference(m):
    d = R.member_draw(m, 5)
    g = d["g"]
    ref, mag, (db, _) = conv_wgrad_ref(d["dy"], d["x0"], d["x1"], 3, 3, 1, (1, 1, 1, 1), g.ups)
    dw, s = R.wgrad_flat(d["dy"], d["x0"], d["x1"], g.ups)
    assert float((dw - ref).abs().max()) <= 1e-12 * float(mag.max()) and float((s - db).abs().max()) <= 1e-12 * float(db.abs().max())


CRITERION = [("nine_tap", NINE_TAP, "x_mask", False), ("nine_tap", NINE_TAP, "y_mask", False), ("nine_tap", NINE_TAP, "slab_dropped", False),
             ("nine_tap", NINE_TAP, "slab_twice", False), ("nine_tap", NINE_TAP, "concat_source", False),
             ("nine_tap_ups", NINE_TAP_UPS, "ups_row", False),
             ("split", SPLIT, "x_mask", True), ("split", SPLIT, "y_mask", True), ("split", SPLIT, "slab_dropped", True),
             ("split", SPLIT, "slab_twice", True), ("split", SPLIT, "concat_source", True), ("split_ups", SPLIT_UPS, "ups_row", True)]


@pytest.mark.parametrize("row,m,fault,split", CRITERION, ids=[f"{c[0]}-{c[2]}" for c in CRITERION])
def test_planted_fault_is_rejected(row, m, fault, split):
    d = R.member_draw(m, 11, torch.float32 if split else torch.bfloat16)
    g = d["g"]
    ref, mag, _ = conv_wgrad_ref(d["dy"], d["x0"], d["x1"], 3, 3, 1, (1, 1, 1, 1), g.ups)
    K, bar = g.N * g.OH * g.OW, R.F32_SPLIT_BAR if split else R.F32_BF16_BAR
    good, _ = R.wgrad_flat(d["dy"], d["x0"], d["x1"], g.ups)
    assert not _rejected(row, good, ref, mag, K, split, bar)
    bad, _ = R.wgrad_flat(d["dy"], d["x0"], d["x1"], g.ups, fault=fault)
    assert _rejected(f"{row}.{fault}", bad, ref, mag, K, split, bar)
    # and both ways at once: outside the bound AND far over the bar (the faults are not marginal at these shapes)
    assert bool(violations(bad, ref, R.bound_of(ref, mag, K, split)).any())
    assert float((bad - ref).norm() / ref.norm()) >= 10 * bar


def test_dbias_short_of_one_part_is_rejected():
    d = R.member_draw(NINE_TAP_DBIAS, 13)
    g = d["g"]
    _, _, (s, sa) = conv_wgrad_ref(d["dy"], d["x0"], None, 3, 3, 1, (1, 1, 1, 1), 0)
    p = d["dbprior"].double()
    ref, mag, K = s + p, sa + p.abs(), g.N * g.OH * g.OW
    _, good = R.wgrad_flat(d["dy"], d["x0"], None)
    assert not _rejected("dbias", good + p, ref, mag, K, False, R.F32_BF16_BAR)
    _, bad = R.wgrad_flat(d["dy"], d["x0"], None, fault="dbias_part", part=(0, 4))       # the first of two parts of an image
    assert bool(violations(bad + p, ref, R.bound_of(ref, mag, K)).any())
    assert float((bad + p - ref).norm() / ref.norm()) >= 10 * R.F32_BF16_BAR
