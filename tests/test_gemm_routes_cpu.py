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
# `route_sweep.py --launch`: mdm_gemm_launch_of / mdm_gemm_pair_launch_of over the same cases, recorded from the change that made the
# launch geometry part of the plan (profiles/r20_gemm_launch_plan.md: on the sweep's cases it is what the parent launched)
LAUNCH_CASES, LAUNCH_SHA256 = 21890, "513492324af3e454bbbcc957a67151ae4300bbe43c51f89a4e89110706b506b5"


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


def test_launch_sweep_matches_the_recorded_geometry(route_sweep):
    from mdm import _lib, ops
    lines = route_sweep.launches(_lib, ops)
    assert (len(lines), route_sweep.digest(lines)) == (LAUNCH_CASES, LAUNCH_SHA256)


def test_a_route_is_named_exactly_where_a_launch_is_planned(route_sweep):
    """mdm_gemm_route_of says "none" exactly where mdm_gemm_launch_of refuses (and the pair queries likewise): the refusals that
    depend on the descriptor alone are part of the plan, not of the launchers."""
    from mdm import _lib, ops
    n = 0
    for case in list(route_sweep.conv_cases(ops)) + list(route_sweep.plain_cases()):
        for f in case[1:]:
            assert (_lib.route_of(**dict(f)) == "none") == (_lib.launch_of(**dict(f)) is None), case[0]
        if len(case) == 3:
            route, planned = _lib.pair_route_of(dict(case[1]), dict(case[2])), _lib.pair_launch_of(dict(case[1]), dict(case[2]))
            assert (route == "none") == (planned is None), case[0]
            assert (route == "pair:two launches") == (planned is not None and len(planned) == 2), case[0]
        n += 1
    assert n == SWEEP_CASES


# The fused 1x1 sites of the attention blocks on the 8x8 map, bf16, at the batches where the generic tile rule of the unfused routes
# says 128 x 128 (M = batch x 64 pixels, N = C channels: unet6_config(32) and (64) at batch 256, unet6_config(128) at batch 100).
# Before the geometry was planned from the route's own row these launched a quarter of the 64 x 64 tiles.
BIG_FUSED_SITES = [("unet6_32", 256, 256, 1024), ("unet6_64", 256, 256, 1024), ("unet6_128", 100, 512, 800)]


@pytest.mark.parametrize("preset,batch,chan,workgroups", BIG_FUSED_SITES, ids=[f"{p}-n{b}" for p, b, _, _ in BIG_FUSED_SITES])
def test_fused_1x1_sites_launch_the_grid_of_the_64_tile(preset, batch, chan, workgroups):
    """project_out with the next GroupNorm's forward fused (gnf) and the data gradient of project_in with the GroupNorm backward fused
    (gnb): lin2<64,64>, one workgroup of 512 threads (conv_lin2's 4 x 2 waves) per 64 x 64 tile of the output."""
    from mdm import _lib, ops
    g = ops.ConvGeom(batch, 8, 8, chan, 0, chan, KH=1, KW=1, pad_t=0, pad_l=0, pad_b=0, pad_r=0)
    gnf = ops.conv_fwd_fields(R.BF, g, 16, None, 16, 16, 16, gnf=dict(out=16, gamma=16, beta=16, stats=16, G=32, silu=1))
    gnb = ops.conv_dgrad_t_fields(R.BF, g, 16, 16, 16, 0, gnb=dict(x=16, stats=16, gamma=16, beta=16, dgamma=16, dbeta=16, G=32, silu=1))
    assert (batch * 64 // 128) * (chan // 128) >= 200
    for f, lds in ((gnf, 4 * (64 + 64) * 128), (gnb, 16384 + 65536 + 4096 + 512)):
        assert _lib.route_of(**f) == "lin2<64,64>"
        assert _lib.launch_of(**f) == (workgroups, 1, 512, lds, 64, 64)
        assert workgroups == (batch * 64 // 64) * (chan // 64)
