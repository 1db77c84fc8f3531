"""The kernel choice of mdm_gemm / mdm_gemm_pair, asked for without a GPU (mdm_gemm_route_of, mdm_gemm_pair_route_of).

Every row of test_gemm_routes_gpu.CASES that goes through mdm_gemm or mdm_gemm_pair is built by the row's own builder on the CPU
and the route the library would take is compared with the one the row names -- the names were recorded from launches on an
MI355X.  The choice is host arithmetic on the descriptor: pointers only have to be non-null and are never dereferenced."""
import pytest
import torch

import test_gemm_routes_gpu as R

# Rows whose kernel is not chosen by mdm_gemm's dispatch, by id.
OUTSIDE = {cid: "grouped weight gradient: mdm_wgrad_group_create schedules it, mdm_gemm's dispatch is not asked"
           for cid in ("group_per_tap", "group_splitk", "group_taps", "group_taps_splitk")}


@pytest.fixture
def cpu_shadow(monkeypatch):
    """mdm_split_shadow is a kernel; the choice only needs a second filter tensor of the same shape."""
    monkeypatch.setattr(R, "_split_shadow", lambda w, dev: (torch.empty_like(w), torch.tensor([0, w.numel()], dtype=torch.int64)))


def route_of(case):
    from mdm import _lib
    dev, g = torch.device("cpu"), torch.Generator().manual_seed(0)
    if case.kind == "pair":
        return _lib.pair_route_of(R.BUILD["fwd"](R.Prob(dev), case.p["a"], g), R.BUILD["fwd"](R.Prob(dev), case.p["b"], g))
    return _lib.route_of(**R.BUILD[case.kind](R.Prob(dev), case.p, g))


@pytest.mark.parametrize("case", [c for c in R.CASES if c.values[0].id not in OUTSIDE])
def test_route_choice(case, cpu_shadow):
    from mdm import _lib
    before = _lib.last_route()
    assert route_of(case) == case.route, case.id
    assert _lib.last_route() == before, "asking for a route changed the record of the last launch"


def test_only_the_grouped_rows_are_left_out():
    kinds = {c.id: c.kind for c in R._case_list()}
    assert set(OUTSIDE) == {cid for cid, k in kinds.items() if k != "pair" and k not in R.BUILD}
    assert all(kinds[cid] == "group" for cid in OUTSIDE)


@pytest.mark.parametrize("case", [c for c in R.CASES if c.values[0].id in OUTSIDE])
def test_grouped_rows_take_the_form_their_route_names(case, monkeypatch):
    """The rows mdm_gemm is not asked about: mdm_wgrad_group_schedule says which form the group takes on a 256-CU device --
    `wgrad_group*` is the per-tap flat grid (form 0), `wgrad_taps_group*` the merged persistent launch (form 1)."""
    from mdm import _lib
    dev, g = torch.device("cpu"), torch.Generator().manual_seed(0)
    fields = [R.BUILD["wgrad"](R.Prob(dev), m, g) for m in case.p["members"]]
    if case.p.get("min_share") is None:
        monkeypatch.delenv("MDM_TAPS_MIN_SHARE", raising=False)
    else:
        monkeypatch.setenv("MDM_TAPS_MIN_SHARE", str(case.p["min_share"]))
    before = _lib.last_route()
    _, _, form = _lib.wgrad_group_schedule(fields, 256)
    assert case.route.split("+")[0] in ("wgrad_group", "wgrad_taps_group")
    assert form == int(case.route.startswith("wgrad_taps_group")), case.id
    assert _lib.last_route() == before


def test_refused_descriptor_has_no_route():
    from mdm import _lib
    f = dict(dtype=R.BF, layout=0, M=64, N=64, K=64, A=16, lda=64, B=16, ldb=64, D0=16, ldd0=64, N0=64)
    assert _lib.route_of(**f) == "ring<64>"
    assert _lib.route_of(**dict(f, N=60)) == "none"          # N must be a multiple of 8
    assert "N=60" in _lib.load().mdm_last_error().decode()
    assert _lib.pair_route_of(dict(f, N=60), f) == "none"
    assert _lib.pair_route_of(f, f) == "pair:two launches"


# ---- the whole dispatch, differentially: scripts/route_sweep.py asks the library about a fixed grid of ~22 000 descriptors (route,
# plan, both GroupNorm-fusion predicates, pair route).  The digests below were recorded from the parent of the change that made
# launch_route an indexed call into the route table and gave the halo tiles one geometry rule (profiles/r09_route_table.md): a
# host-side refactor of csrc/gemm.hip leaves them as they are, a change of the dispatch rule re-records them on purpose.
SWEEP_CASES, SWEEP_SHA256 = 21890, "acbf675c38408ee594e59488c4c4aaac43d15b2d377241c74c507539c95fb43d"
# ops.split_grad_reason of both gradients over the sweep's convolution geometries, recorded from the parent's mdm/ops.py (which
# restated the tile rule in Python; it now asks mdm_gemm_route_of)
REASON_ROWS, REASON_SHA256 = 5433, "89d1a19e206d444a7a4c65bf4a8049bc673efda265b35b5a4aa22fd8b080fd93"


@pytest.fixture(scope="module")
def route_sweep():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "route_sweep.py")
    spec = importlib.util.spec_from_file_location("route_sweep", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sweep_matches_the_recorded_dispatch(route_sweep):
    from mdm import _lib, ops
    lines, seen = route_sweep.sweep(_lib, ops)
    missing = [n for n in _lib.route_names() if n not in seen and n.split("+")[0] not in route_sweep.NOT_FROM_MDM_GEMM]
    assert not missing, f"the sweep never reaches {missing}"
    assert (len(lines), route_sweep.digest(lines)) == (SWEEP_CASES, SWEEP_SHA256)


def test_split_grad_reason_matches_the_recorded_table(route_sweep):
    from mdm import ops
    lines = route_sweep.reasons(ops)
    assert {ln.split(" | ")[1] for ln in lines} == {"dgrad None", "dgrad channels", "dgrad stride2", "dgrad geometry"}
    assert (len(lines), route_sweep.digest(lines)) == (REASON_ROWS, REASON_SHA256)
