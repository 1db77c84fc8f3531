"""The schedule of a group of weight gradients (csrc/gemm.hip plan_wgrad_group), asked for without a GPU through
mdm_wgrad_group_schedule: one decoded row (queue, round, desc, kind, tile_or_item, k0, k1, slot) per entry of the table that
mdm_wgrad_group_create would upload (include/mdm_hip.h).  Pointers are dummies; the library never dereferences them.

The groups are those of scripts/wgrad_group_parity.py: the 16 shapes of test_grouped_weight_gradients_match_self_contained_ones
with ops.wgrad_group_split splits (`mixed240` has more than 96 split members, so the split-K reduce table closes at least once),
and the per-flush groups of two nets."""
import ctypes
import importlib.util
import os

import pytest

Q, RND, DESC, KIND, ITEM, K0, K1, SLOT = range(8)
GK_64, GK_128, GK_256x128, GK_TAPS = range(4)
TAPS_BM, TAPS_BN, MINPART = 128, 64, 8
SLOT_BYTES, PART_TILE_BYTES = 9 * TAPS_BM * TAPS_BN * 4, 48
# recorded from the parent of the change that introduced plan_wgrad_group: a dump of the tables its mdm_wgrad_group_create built,
# decoded the same way, over the same matrix (profiles/r14_wgrad_group_plan.md).  A host-side refactor leaves them as they are; a
# change of the schedule re-records them on purpose.
PARITY_CASES, PARITY_SHA256 = 60, "7695374edc454c86bbda77a7c611ddd378b3254a4514bc7afbbd443bc8bd2fce"


def _script():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "wgrad_group_parity.py")
    spec = importlib.util.spec_from_file_location("wgrad_group_parity", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _script()
_groups = {}


def group(name):
    if not _groups:
        import mdm
        from mdm import ops
        _groups.update((n, f) for n, f in P.groups(mdm, ops) if "#" not in n or n.startswith(("tiny_n4_16", "cfg2_n32_32MiB")))
    return _groups[name]


GROUPS = ["mixed240", "mixed16", "per_tap", "taps3", "tiny_n4_16#0", "cfg2_n32_32MiB#0", "cfg2_n32_32MiB#1", "cfg2_n32_32MiB#2",
          "cfg2_n32_32MiB#3"]


def cdiv(a, b):
    return -(-a // b)


def pad256(v):
    return cdiv(v, 256) * 256


def schedule(monkeypatch, fields, n_cu, min_share):
    from mdm import _lib
    if min_share is None:
        monkeypatch.delenv("MDM_TAPS_MIN_SHARE", raising=False)
    else:
        monkeypatch.setenv("MDM_TAPS_MIN_SHARE", str(min_share))
    before = _lib.last_route()
    out = _lib.wgrad_group_schedule(fields, n_cu)
    assert _lib.last_route() == before, "asking for a schedule changed the record of the last route"
    return out


def check_per_tap_items(fields, rows, descs):
    """Every (desc, item) of the per-tap members `descs`, item < tiles x taps x splitk, appears exactly once."""
    seen = {}
    for r in rows:
        if r[DESC] >= 0 and r[KIND] != GK_TAPS:
            assert (r[K1], r[SLOT]) == (0, 0), r
            seen.setdefault(r[DESC], []).append(r)
    assert set(seen) == set(descs)
    for i, rs in seen.items():
        f = fields[i]
        kinds, tiles_x = {r[KIND] for r in rs}, {r[K0] for r in rs}
        assert len(kinds) == 1 and len(tiles_x) == 1, (i, kinds, tiles_x)
        kind, tx = kinds.pop(), tiles_x.pop()
        want = {GK_64: cdiv(f["M"], 64) * cdiv(f["N"], 64), GK_128: cdiv(f["M"], 128) * cdiv(f["N"], 128),
                GK_256x128: (f["M"] // 256) * cdiv(f["N"], 128)}[kind]
        assert tx == want and (kind != GK_256x128 or f["M"] % 256 == 0), (i, kind, tx)
        assert sorted(r[ITEM] for r in rs) == list(range(tx * f["KH"] * f["KW"] * max(f["splitk"], 1))), i


@pytest.mark.parametrize("min_share", [None, 0])
@pytest.mark.parametrize("n_cu", [256, 8])
@pytest.mark.parametrize("name", GROUPS)
def test_schedule(name, n_cu, min_share, monkeypatch):
    from mdm import _lib
    fields = group(name)
    rows, need, form = schedule(monkeypatch, fields, n_cu, min_share)
    queues = n_cu if form else 8
    assert len(rows) % queues == 0 and any(r[DESC] >= 0 for r in rows[-queues:]), "rows = rounds x queues, the last round is in use"
    for i, r in enumerate(rows):
        assert (r[Q], r[RND]) == (i % queues, i // queues)
        assert r[DESC] >= 0 or r[DESC:] == (-1, 0, 0, 0, 0, 0), r              # padding
        assert r[DESC] < len(fields) and 0 <= r[KIND] <= GK_TAPS
    taps = {}
    for r in rows:
        if r[DESC] >= 0 and r[KIND] == GK_TAPS:
            taps.setdefault((r[DESC], r[ITEM]), []).append(r)
    nine = {d for d, _ in taps}
    check_per_tap_items(fields, rows, set(range(len(fields))) - nine)
    need_want = pad256(len(fields) * ctypes.sizeof(_lib.GemmDesc)) + pad256(len(rows) * 16)
    if form == 0:                           # the per-tap flat grid: 8 x maxlen entries, nothing else in the table
        assert not taps
        assert need == need_want
        return
    assert taps, "the merged form exists for the nine-tap members"
    slots, cut = [], 0
    for d in nine:                          # every tile of a nine-tap member
        f = fields[d]
        assert {t for dd, t in taps if dd == d} == set(range(cdiv(f["M"], TAPS_BM) * cdiv(f["N"], TAPS_BN))), d
    for (d, tile), parts in taps.items():
        slabs = fields[d]["K"] // 64
        parts.sort(key=lambda r: r[SLOT])
        assert parts[0][K0] == 0 and parts[-1][K1] == slabs, (d, tile)
        assert all(a[K1] == b[K0] for a, b in zip(parts, parts[1:])), "the parts partition [0, K / 64), ascending in slot order"
        assert all(r[K0] < r[K1] for r in parts)
        assert all(r[K1] - r[K0] >= MINPART for r in parts) or (len(parts) == 1 and slabs < MINPART), (d, tile, parts)
        if len(parts) == 1:
            assert parts[0][SLOT] == 0, "an uncut tile goes straight to the gradient"
        else:
            assert [r[SLOT] for r in parts] == list(range(parts[0][SLOT], parts[0][SLOT] + len(parts))) and parts[0][SLOT] >= 1
            slots += [r[SLOT] for r in parts]
            cut += 1
    assert sorted(slots) == list(range(1, len(slots) + 1)), "slots are unique and dense from 1 to nslots"
    assert need == need_want + pad256(cut * PART_TILE_BYTES) + len(slots) * SLOT_BYTES


def test_both_forms_and_a_closed_reduce_table_are_covered(monkeypatch):
    forms = {(n, c, m): schedule(monkeypatch, group(n), c, m)[2] for n in GROUPS for c in (256, 8) for m in (None, 0)}
    assert set(forms.values()) == {0, 1}
    assert forms["mixed240", 256, None] == 0 and forms["mixed240", 256, 0] == 1 and forms["cfg2_n32_32MiB#0", 256, None] == 1
    assert sum(f["splitk"] > 1 for f in group("mixed240")) > 96             # REDUCE_MAX_SEGS of csrc/gemm.hip
    for name, n_cu in (("taps3", 8), ("mixed16", 256)):                     # (taps3 at 256 CUs: short tiles, none is cut)
        assert any(r[SLOT] > 0 for r in schedule(monkeypatch, group(name), n_cu, 0)[0]), f"{name} at {n_cu} CUs has cut tiles"


@pytest.mark.parametrize("n_cu", [256, 8])
def test_refusals_are_create_s(n_cu, monkeypatch):
    from mdm import _lib, ops
    ok = P.member(ops, P.geom(ops, 4, 8, 64, 0, 64), 1)
    g = P.geom(ops, 8, 16, 128, 0, 128)
    no_ws = P.member(ops, g, 4)
    no_ws.pop("ws")
    no_ws["ws_bytes"] = 0
    with pytest.raises(RuntimeError, match="wgrad_group_create: descriptor 1 is split 4 ways but has no workspace of its own"):
        schedule(monkeypatch, [ok, no_ws], n_cu, None)
    for bad in (dict(P.member(ops, g, 1), out_f32=0), dict(P.member(ops, g, 1), ldd0=256)):
        assert not _lib.wgrad_group_accepts(**bad)
        with pytest.raises(RuntimeError, match="wgrad_group_create: descriptor 2 is not a groupable weight gradient"):
            schedule(monkeypatch, [ok, ok, bad], n_cu, 0)
    with pytest.raises(RuntimeError, match="bad arguments"):
        _lib.wgrad_group_schedule([ok], 0)


def test_schedule_matches_the_recorded_parent(monkeypatch):
    import mdm
    from mdm import _lib, ops
    monkeypatch.delenv("MDM_TAPS_MIN_SHARE", raising=False)
    cases, lines = P.sweep(_lib, mdm, ops)
    assert (cases, P.digest(lines)) == (PARITY_CASES, PARITY_SHA256)
