"""The kernels behind every weight gradient of the train step against fp64, with the per-element bound of tests/_bounds.py, NaN
guard bands, NaN-prefilled outputs, workspaces and slots (rows: tests/_wgrad_rows.py; what the rows reach: test_wgrad_bounds_cpu.py).

A. mdm_wgrad_group_launch with the queue count of the persistent launch PINNED (MDM_TAPS_MIN_SHARE = 0, MDM_WGRAD_RESERVE_CUS =
   CUs - Q): wgrad_taps_group_kernel / wgrad_taps_body (both BIAS bodies), its cut tiles through slots and
   tile_parts_reduce_kernel, the per-tap items of kinds 0, 1, 2 that ride in its queues, splitk_reduce_batched_kernel; and the
   per-tap form (wgrad_group_kernel) on the same members.  The uploaded table is the one mdm_wgrad_group_schedule describes.
   (A merged group whose split member overwrites -- acc0 = 0 -- is group_taps_splitk of test_gemm_routes_gpu.py.)
B. mdm_conv_wgrad_split at its edges: wgrad_split_kernel<64>, ragged tiles, K % 32 != 0, one and two slabs, explicit and capped
   splits, a non-dense destination, pitched operands, both acc0 through splitk_reduce_kernel; and its refusals.

Every output: guards intact, exact route string, per-element bound with k_terms = N OH OW, the rel-L2 bar of the output kind
(REL_BAR of test_gemm_routes_gpu.py; neither bar is raised here), the same bits on a second launch into re-poisoned buffers
(the bias gradient is summed with fp32 atomics: held to its bound, which does not depend on the order); the operands of a group
come back bit-unchanged."""
import ctypes

import pytest
import torch

import _wgrad_rows as R
from _bounds import Buf, check
from _notes import note
from test_gemm_routes_gpu import REL_BAR
from test_grad_split_gpu import F32_SPLIT_BAR
from test_wgrad_group_gpu import decode

pytestmark = pytest.mark.gpu

assert (REL_BAR["f32_bf16"], REL_BAR["f32_split"], F32_SPLIT_BAR) == (R.F32_BF16_BAR, R.F32_SPLIT_BAR, R.F32_SPLIT_BAR)
BF, F32 = torch.bfloat16, torch.float32


def _dev():
    return torch.device("cuda:0")


def _poison(b):
    b.t.view(b.ity).fill_(b.pat)


def _is_poison(t, b):
    return bool((t.contiguous().view(b.ity) == b.pat).all())


class Member:
    """The device side of one group member: operands, gradient, bias gradient and workspace, each inside guard bands."""

    def __init__(self, m, d, dev):
        g = d["g"]
        self.m, self.d = m, d
        self.dy, self.x0 = Buf(d["dy"].shape, BF, dev, d["dy"]), Buf(d["x0"].shape, BF, dev, d["x0"])
        self.x1 = Buf(d["x1"].shape, BF, dev, d["x1"]) if d["x1"] is not None else None
        self.dw = Buf((g.taps, g.Cout, g.Cin), F32, dev)
        self.db = Buf((g.Cout,), F32, dev) if m["dbias"] else None
        self.ws = Buf((R.ws_floats(m),), F32, dev) if m["splitk"] > 1 else None
        self.bufs = [b for b in (self.dy, self.x0, self.x1, self.dw, self.db, self.ws) if b is not None]

    def fields(self):
        t = lambda b: b.t if b is not None else None
        return R.member_fields(self.m, dy=self.dy.t, x0=self.x0.t, x1=t(self.x1), dw=self.dw.t, db=t(self.db), ws=t(self.ws))

    def reset(self):
        """dw: the NaN pattern (overwrite) or its finite prior (accumulate); dbias: its prior; workspace: NaN."""
        if self.m["acc"]:
            self.dw.t.copy_(self.d["prior"])
        else:
            _poison(self.dw)
        if self.db is not None:
            self.db.t.copy_(self.d["dbprior"])
        if self.ws is not None:
            _poison(self.ws)


_results = {}


def _run_group(name, Q, want_route, monkeypatch):
    """Build, launch twice, check everything; -> [(dw, dbias or None)] of the first launch on the CPU.  Q = None: the per-tap form."""
    from mdm import _lib
    if (name, Q) in _results:
        return _results[name, Q]
    dev, label = _dev(), f"{name}@{Q}" if Q else name
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    if Q is None:
        monkeypatch.delenv("MDM_TAPS_MIN_SHARE", raising=False)
        monkeypatch.delenv("MDM_WGRAD_RESERVE_CUS", raising=False)
    else:
        assert n_cu >= Q, f"a device of {n_cu} CUs cannot run {Q} queues"
        monkeypatch.setenv("MDM_TAPS_MIN_SHARE", "0")
        monkeypatch.setenv("MDM_WGRAD_RESERVE_CUS", str(n_cu - Q))
    members, refs = R.GROUPS[name], R.group_refs(name)
    devs = [Member(m, d, dev) for m, d in zip(members, R.group_draws(name))]
    fields = [dv.fields() for dv in devs]
    rows, need, form = _lib.wgrad_group_schedule(fields, Q or n_cu)
    assert form == (0 if Q is None else 1)
    grp = _lib.WgradGroup(fields, dev)
    assert grp.table.numel() == need
    assert decode(grp.table, len(fields), len(rows), form, Q or n_cu) == rows
    at, nbytes = R.slots_at(len(fields), rows, need, ctypes.sizeof(_lib.GemmDesc))
    slots = grp.table[at:at + nbytes].view(F32) if nbytes else None
    runs = []
    for rep in range(2):
        for dv in devs:
            dv.reset()
        if slots is not None:           # a part that leaves an element of its slot unwritten poisons the gradient
            slots.fill_(float("nan"))
        torch.cuda.synchronize()
        grp.launch()
        route = _lib.last_route()
        torch.cuda.synchronize()
        assert route == want_route, (name, Q, route)
        out = []
        for i, (dv, ref) in enumerate(zip(devs, refs)):
            for b in dv.bufs:
                assert b.guards_intact(), f"{label} member {i}: guard band of a {b.shape} buffer changed at {b.first_bad_guard()}"
            tag = f"{label}.m{i}"
            for b, src in ((dv.dy, "dy"), (dv.x0, "x0"), (dv.x1, "x1")):
                assert b is None or torch.equal(b.t.cpu(), dv.d[src]), f"{tag}: the launch changed {src}"
            ratio, rel = check(tag + ".dw", dv.dw.t, ref["dw"][0], ref["dw"][1], ref["K"], "f32")
            res = [("dw", ratio, rel)]
            if dv.db is not None:
                res.append(("dbias",) + check(tag + ".dbias", dv.db.t, ref["db"][0], ref["db"][1], ref["K"], "f32"))
            for o, ratio, rel in res:
                if rep == 0:
                    note("wgrad_bounds", dict(row=label, member=i, out=o, route=route, ratio=ratio, rel_l2=rel))
                assert rel <= REL_BAR["f32_bf16"], f"{tag}.{o}: rel-L2 {rel:.3e} above the bar {REL_BAR['f32_bf16']:.1e}"
            out.append((dv.dw.t.cpu(), dv.db.t.cpu() if dv.db is not None else None))
        runs.append(out)
    for i, ((a, _), (b, _)) in enumerate(zip(*runs)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label} member {i}: dw differs between two launches"
    _results[name, Q] = runs[0]
    return runs[0]


@pytest.mark.parametrize("name,Q,route", R.MERGED_RUNS, ids=[f"{n}@{q}" for n, q, _ in R.MERGED_RUNS])
def test_merged_group_vs_fp64(name, Q, route, monkeypatch):
    _run_group(name, Q, route, monkeypatch)


@pytest.mark.parametrize("name,route", R.PER_TAP_RUNS, ids=[n for n, _ in R.PER_TAP_RUNS])
def test_per_tap_group_vs_fp64(name, route, monkeypatch):
    _run_group(name, None, route, monkeypatch)


def test_cut_and_uncut_tiles_agree(monkeypatch):
    """`edges` at 8 queues (every tile stored straight to the gradient) and at 24 (tiles cut into slots): the same operands, two
    summation orders -- within the sum of the two bounds, not bit-equal by requirement."""
    uncut = _run_group("edges", 8, "wgrad_taps_group", monkeypatch)
    cut = _run_group("edges", 24, "wgrad_taps_group", monkeypatch)
    for i, ((a, ab), (b, bb), ref) in enumerate(zip(uncut, cut, R.group_refs("edges"))):
        bound = 2 * R.bound_of(ref["dw"][0], ref["dw"][1], ref["K"])
        assert bool(((a.double() - b.double()).abs() <= bound).all()), f"edges member {i}: cut and uncut differ by more than both bounds"
        if ab is not None:
            bound = 2 * R.bound_of(ref["db"][0], ref["db"][1], ref["K"])
            assert bool(((ab.double() - bb.double()).abs() <= bound).all()), f"edges member {i}: dbias"


# ------------------------------------------------------------------ mdm_conv_wgrad_split
def _slice_buf(values, width, at, dev):
    """`values` [..., C] as the channels [at, at + C) of a NaN-filled [..., width] buffer: -> (Buf, the view handed to the library)"""
    b = Buf(tuple(values.shape[:-1]) + (width,), F32, dev)
    view = b.t[..., at:at + values.shape[-1]]
    view.copy_(values)
    return b, view


def _launch_split(name, acc):
    """-> (dw Buf, the [taps][M][N] view of it, route): one launch into freshly poisoned buffers"""
    from mdm import _lib
    row = R.SPLIT_ROWS[name]
    d, _, _ = R.split_draw_and_ref(name)
    g, dev, over = d["g"], _dev(), row["over"]
    dyb, dy = _slice_buf(d["dy"], over.get("lda", g.Cout), 16 if "lda" in over else 0, dev)
    x0b, x0 = _slice_buf(d["x0"], over.get("ld0", g.C0), 4 if "ld0" in over else 0, dev)
    x1b = Buf(d["x1"].shape, F32, dev, d["x1"]) if d["x1"] is not None else None
    dwb = Buf((g.taps, g.Cout, over.get("ldd0", g.Cin)), F32, dev)
    dw = dwb.t[..., :g.Cin]
    if acc:
        dw.copy_(d["prior"])
    wsb = Buf((row["ws_bytes"] // 4,), F32, dev) if row["ws_bytes"] else None
    assert wsb is None or wsb.t.numel() * 4 == row["ws_bytes"]
    f = R.split_fields(row, dy=dy, x0=x0, x1=x1b.t if x1b else None, dw=dwb.t, ws=wsb.t if wsb else None, acc=acc)
    assert _lib.wgrad_split_plan(**f) == row["plan"]
    torch.cuda.synchronize()
    _lib.wgrad_split(**f)
    route = _lib.wgrad_split_last_route()
    torch.cuda.synchronize()
    assert route == row["route"], (name, route)
    for b in (dyb, x0b, x1b, dwb, wsb):
        assert b is None or b.guards_intact(), f"{name}: guard band of a {b.shape} buffer changed at {b.first_bad_guard()}"
    if "ldd0" in over:
        assert _is_poison(dwb.t[..., g.Cin:], dwb), f"{name}: the pitch gap of the destination was written"
    if wsb is not None and row["plan"][0] == 1:
        assert _is_poison(wsb.t, wsb), f"{name}: an unsplit reduction wrote its workspace"
    return dwb, dw, route


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("name", list(R.SPLIT_ROWS))
def test_split_wgrad_edges_vs_fp64(name, acc):
    _, refs, K = R.split_draw_and_ref(name)
    ref, mag = refs[acc]
    _, dw, route = _launch_split(name, acc)
    ratio, rel = check(f"{name}.acc{acc}", dw, ref, mag, K, "f32", split=True)
    note("wgrad_bounds", dict(row=f"split.{name}.acc{acc}", out="dw", route=route, ratio=ratio, rel_l2=rel))
    assert rel < F32_SPLIT_BAR, (name, acc, rel)
    _, dw2, route2 = _launch_split(name, acc)
    assert route2 == route and torch.equal(dw2.contiguous().view(torch.int32), dw.contiguous().view(torch.int32))


@pytest.mark.parametrize("bad", ["M6", "C06", "dbias"])
def test_split_wgrad_refusals(bad):
    """M = 6, C0 = 6 and a dbias pointer raise through mdm_last_error, leave the route at "none" and dw untouched."""
    from mdm import _lib
    _, _, route = _launch_split("bt64", 0)
    assert route == "wgrad_split<64>" and _lib.wgrad_split_last_route() == route
    dev = _dev()
    m = R.M(3, 8, 8, 6 if bad == "C06" else 64, 0, 6 if bad == "M6" else 64)
    d = R.member_draw(m, 77, F32)
    g = d["g"]
    dy, x0 = Buf(d["dy"].shape, F32, dev, d["dy"]), Buf(d["x0"].shape, F32, dev, d["x0"])
    dw, db = Buf((g.taps, g.Cout, g.Cin), F32, dev), Buf((g.Cout,), F32, dev, torch.zeros(g.Cout))
    f = R.split_fields(dict(R.SPLIT_ROWS["bt64"], m=m), dy=dy.t, x0=x0.t, dw=dw.t)
    if bad == "dbias":
        f["dbias"] = db.t
    with pytest.raises(RuntimeError, match="wgrad_split"):
        _lib.wgrad_split(**f)
    torch.cuda.synchronize()
    assert _lib.wgrad_split_last_route() == "none"
    assert _is_poison(dw.t, dw) and dw.guards_intact() and bool((db.t == 0).all())
