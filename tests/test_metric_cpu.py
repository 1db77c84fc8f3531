"""The image-quality ABI without a GPU: include/mdm_metric.h parses to its three functions and is bound next to the other headers
without entering their tables; mdm_metric_plan (host code) gives the window and refuses what the header says; the fp64 statement of
tests/_metric_ref.py agrees with a second one through scipy; an fp32 CPU emulation of the kernel's arithmetic as the header specifies it
(pivots, separable passes, fused multiply-adds in tap order, double from the moments on) stays inside the derived bound of
tests/_metric_bounds.py on every input class, and every planted fault leaves it on at least one.  No kernel is launched."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _metric_bounds as MB
import _metric_ref as MR
from mdm import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "mdm_metric.h")
NAMES = ["mdm_metric_plan", "mdm_metric_ws_bytes", "mdm_metric_image"]
IMAGE_PARAMS = ["pred", "truth", "keep", "Ck", "R", "N", "C", "H", "W", "clamp_lo", "clamp_hi", "data_range", "ws", "ws_bytes", "out", "stream"]
_K = "test_metric_kernels_gpu"
COVERAGE = {n: (_K, n) for n in NAMES}


# ------------------------------------------------------------------ the eighth header and its tables
def test_the_header_declares_exactly_the_exports_bound():
    structs, protos = _lib.parse_header(open(HEADER).read())
    assert structs == {} and list(protos) == NAMES
    assert [n for n, _ in protos["mdm_metric_image"][1]] == IMAGE_PARAMS
    assert protos["mdm_metric_ws_bytes"][0] == "int64_t" and protos["mdm_metric_plan"][0] == protos["mdm_metric_image"][0] == "int"
    declared = set(re.findall(r"\b(mdm_metric_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)))
    assert declared == set(NAMES) == set(_lib.METRIC_EXPORTS) == set(_lib.METRIC_PROTOS) == set(_lib.METRIC_PARAMS)
    lib = _lib.load()
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.METRIC_PROTOS[name][0] and fn.restype is _lib.METRIC_PROTOS[name][1], name
    assert _lib.METRIC_PROTOS["mdm_metric_image"] == ([vp, vp, vp, i32, i64, i32, i32, i32, i32, f32, f32, f32, vp, i64, vp, vp], i32)
    assert _lib.METRIC_PROTOS["mdm_metric_ws_bytes"] == ([i64, i32, i32, i32], i64)
    assert os.path.samefile(_lib.METRIC_HEADER_PATH, HEADER)


def test_the_tables_stay_apart():
    for name in NAMES:
        assert name in _lib._ALL_PROTOS and name in _lib._ALL_PARAMS and name not in _lib._PROTOS and name not in _lib.EXPORTS
    for header in ("mdm_hip.h", "mdm_vis.h", "mdm_data.h", "mdm_interp.h", "mdm_ingest.h", "mdm_neighbor.h", "mdm_inpaint.h"):
        assert "mdm_metric" not in open(os.path.join(ROOT, "include", header)).read(), header
    kw = dict(zip(IMAGE_PARAMS, (1, 2, None, 1, 6, 2, 3, 16, 16, -1.0, 1.0, 2.0, 3, 4096, 4, None)))
    with _lib.Recording() as rec:
        _lib.call("mdm_metric_image", **kw)
        with pytest.raises(TypeError, match="mdm_metric_image"):
            _lib.call("mdm_metric_image", **dict(kw, keep_C=1))
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_metric_image", tuple(kw.values())[:-1])]


def test_every_metric_symbol_has_a_kernel_test():
    assert set(COVERAGE) == set(_lib.METRIC_PROTOS)
    for sym, (mod, mention) in COVERAGE.items():
        text = open(os.path.join(TESTS, mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), f"{mod}.py does not mention {mention}"
        assert "pytest.mark.gpu" in text


# ------------------------------------------------------------------ mdm_metric_plan
def test_plan_window_and_geometry():
    import mdm
    plan = mdm.metrics.plan(6, 3, 64, 64)
    w = np.array(plan.window, dtype=np.float32)
    assert w.shape == (11,) and np.array_equal(w, w[::-1]) and (w > 0).all() and w.argmax() == 5
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 11 * 2.0 ** -24
    assert np.array_equal(w, MR.window64().numpy().astype(np.float32))       # the double Gaussian, each weight rounded once
    th, tw = plan.tile_h, plan.tile_w
    assert (plan.tiles_y, plan.tiles_x) == (-(-54 // th), -(-54 // tw)) and plan.grid == (6 * 3 * plan.tiles_y * plan.tiles_x, 6)
    assert plan.ws_bytes == 6 * 3 * plan.tiles_y * plan.tiles_x * 48
    assert plan.lds_bytes >= 2 * (th + 10) * (tw + 10) * 4 and plan.lds_bytes <= 65536
    one = mdm.metrics.plan(1, 1, 11, 11)
    assert (one.tiles_y, one.tiles_x, one.grid) == (1, 1, (1, 1)) and one.window == plan.window
    edge = mdm.metrics.plan(1, 1, th + 11, tw + 11)                           # one map position past a tile on both axes
    assert (edge.tiles_y, edge.tiles_x) == (2, 2)


def test_plan_refusals():
    import mdm
    lib = _lib.load()
    for bad, word in ((dict(R=0), "R"), (dict(C=0), "C"), (dict(H=10), "H"), (dict(W=10), "W"), (dict(H=-1), "H"),
                      (dict(C=4, H=32768, W=32768), "C H W")):
        kw = dict(dict(R=2, C=3, H=16, W=16), **bad)
        with pytest.raises(RuntimeError, match="metric_plan: .*" + re.escape(word)):
            mdm.metrics.plan(**kw)
        assert lib.mdm_metric_ws_bytes(kw["R"], kw["C"], kw["H"], kw["W"]) == -1
        assert lib.mdm_last_error().decode().startswith("metric_ws_bytes:")


# ------------------------------------------------------------------ the reference against scipy
def test_the_reference_agrees_with_scipy():
    pytest.importorskip("scipy")
    pred, truth = MR.draw_images("noise", 2, 2, 3, 16, 19)
    ref = MR.reference(pred * 1.5, truth)                                    # (some of pred outside the clamp)
    other = MR.reference_scipy(pred * 1.5, truth)
    assert ref["map"].shape == other.shape == (2, 3, 6, 9)
    assert float((ref["map"] - other).abs().max()) <= 1e-12
    assert abs(float(ref["out"][0, 2]) - float(other[0].mean())) <= 1e-12


def test_the_reference_slots():
    pred, truth = MR.draw_images("smooth", 4, 2, 3, 13, 12)
    keep = MR.draw_keep("box", 2, 3, 13, 12)
    ref = MR.reference(pred, truth, keep)
    out = ref["out"]
    sq = (pred.double() - truth.double().repeat(2, 1, 1, 1)) ** 2
    assert torch.allclose(out[:, 0], sq.mean((1, 2, 3)), rtol=1e-14) and torch.allclose(out[:, 1], 10 * torch.log10(4 / out[:, 0]), rtol=1e-14)
    hole = (keep == 0).expand(2, 3, 13, 12).repeat(2, 1, 1, 1)
    assert out[:, 6].tolist() == hole.sum((1, 2, 3)).tolist() and out[:, 7].tolist() == hole[:, :, 5:8, 5:7].sum((1, 2, 3)).tolist()
    assert torch.allclose(out[:, 0] * 3 * 13 * 12, sq.sum((1, 2, 3)), rtol=1e-14)
    none = MR.reference(pred, truth, MR.draw_keep("ones", 2, 3, 13, 12))["out"]
    assert bool(torch.isnan(none[:, 3:6]).all()) and not none[:, 6:].any() and torch.equal(none[:, :3], out[:, :3])
    same = MR.reference(truth.repeat(2, 1, 1, 1), truth)["out"]
    assert bool((same[:, 0] == 0).all()) and bool(torch.isinf(same[:, 1]).all()) and float((same[:, 2] - 1).abs().max()) < 1e-12


def test_a_nan_reaches_the_windows_that_hold_it_and_no_other():
    pred, truth = MR.draw_images("noise", 2, 2, 1, 14, 15)
    pred[1, 0, 2, 12] = math.nan
    m = MR.reference(pred, truth)["map"]
    want = torch.zeros(2, 1, 4, 5, dtype=torch.bool)
    want[1, 0, :3, 2:] = True                                                # windows [y, y + 11) x [x, x + 11) holding (2, 12)
    assert torch.equal(torch.isnan(m), want)


# ------------------------------------------------------------------ the kernel's arithmetic, emulated in fp32
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma(w, v, acc):
    """fl(w v + acc): the product of two floats is exact in double"""
    return (np.float64(w) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def emulate(pred, truth, keep, plan, data_range=2.0, clamp=(-1.0, 1.0), fault=None):
    """-> [R, 8] float32: include/mdm_metric.h step by step, tile by tile, on the host.  `fault` plants one of FAULTS."""
    R, C, H, W = pred.shape
    N = truth.shape[0]
    L = float(np.float32(data_range))
    C1, C2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    if fault == "swap_c":
        C1, C2 = C2, C1
    w = _f32(plan.window)
    if fault == "unnormalised":
        w = _f32(np.exp(-(np.arange(11.0) - 5) ** 2 / 4.5))
    p = MR.clamp_keep_nan(pred.float(), clamp).numpy()
    rows = np.arange(R) % N if fault != "truth_r" else np.minimum(np.arange(R), N - 1)
    t = truth.numpy()[rows]
    hole = MR.hole_mask(keep, N, C, H, W).numpy()[np.arange(R) % N]
    sq = (p - t) * (p - t)                                                    # two fp32 operations
    sq64 = sq.astype(np.float64)
    ps, ts, hs = p, t, hole
    if fault == "same":                                                       # zero padding instead of the valid region
        ps, ts = (np.pad(a, ((0, 0), (0, 0), (5, 5), (5, 5))) for a in (p, t))
        hs = np.pad(hole, ((0, 0), (0, 0), (5, 5), (5, 5)))
    if fault == "shift":                                                      # the window one element to the right
        ps, ts = (np.concatenate((a[..., 1:], a[..., -1:]), -1) for a in (ps, ts))
    Hs, Ws = ps.shape[2:]
    MH, MW = Hs - 10, Ws - 10
    th, tw = plan.tile_h, plan.tile_w
    smap = np.zeros((R, C, MH, MW), dtype=np.float64)
    for y0 in range(0, MH, th):
        for x0 in range(0, MW, tw):
            ny, nx = min(th, MH - y0), min(tw, MW - x0)
            yc, xc = min(y0 + 5 + th // 2, Hs - 1), min(x0 + 5 + tw // 2, Ws - 1)
            cp, ct = (np.where(np.isfinite(a[:, :, yc, xc]), a[:, :, yc, xc], np.float32(0))[:, :, None, None] for a in (ps, ts))
            d = _f32(ps[:, :, y0:y0 + ny + 10, x0:x0 + nx + 10] - cp)
            e = _f32(ts[:, :, y0:y0 + ny + 10, x0:x0 + nx + 10] - ct)
            vals = [d, e, d * d, e * e, d * e]
            hz = [np.zeros(d.shape[:3] + (nx,), dtype=np.float32) for _ in vals]
            for j in range(11):
                if fault == "drop_tap" and j == 3:
                    continue
                hz = [_fma(w[j], v[..., j:j + nx], h) for v, h in zip(vals, hz)]
            m = [np.zeros(d.shape[:2] + (ny, nx), dtype=np.float32) for _ in vals]
            for i in range(11):
                m = [_fma(w[i], h[:, :, i:i + ny], a) for h, a in zip(hz, m)]
            md, me, sdd, see, sde = (a.astype(np.float64) for a in m)
            mu_p, mu_t = cp.astype(np.float64) + md, ct.astype(np.float64) + me
            var_p, var_t, cov = sdd - md * md, see - me * me, sde - md * me
            if fault == "unbiased":
                var_p, var_t, cov = (v * (121.0 / 120.0) for v in (var_p, var_t, cov))
            smap[:, :, y0:y0 + ny, x0:x0 + nx] = ((2 * mu_p * mu_t + C1) * (2 * cov + C2)) / ((mu_p * mu_p + mu_t * mu_t + C1) * (var_p + var_t + C2))
    hole_c = hs[:, :, :MH, :MW] if fault == "corner" else hs[:, :, 5:5 + MH, 5:5 + MW]
    out = np.zeros((R, 8), dtype=np.float64)
    with np.errstate(all="ignore"):
        for r in range(R):
            nh, nhc = int(hole[r].sum()), int(hole_c[r].sum())
            mse, mse_h = sq64[r].sum() / sq64[r].size, sq64[r][hole[r]].sum() / np.float64(nh)
            out[r] = (mse, 10 * np.log10(L * L / mse), smap[r].sum() / smap[r].size, mse_h, 10 * np.log10(L * L / mse_h),
                      smap[r][hole_c[r]].sum() / np.float64(nhc), nh, nhc)
    return torch.from_numpy(out.astype(np.float32))


SHAPES = [(6, 2, 3, 16, 16), (3, 1, 1, 27, 43), (2, 2, 3, 11, 40)]          # (R, N, C, H, W): one tile; 2 x 2 tiles by one; one row
CLASSES = [(img, kp) for img in MR.IMAGE_KINDS for kp in ("none", "box")] + [("smooth", kp) for kp in MR.KEEP_KINDS] + \
          [("two_level", "random_c"), ("noise", "nan")]
FAULTS = ("drop_tap", "shift", "unnormalised", "swap_c", "same", "unbiased", "corner", "truth_r")


def _plan(shape):
    import mdm
    R, N, C, H, W = shape
    return mdm.metrics.plan(R, C, H, W)


_CASES = {}


def _case(shape, img, kp):
    """(pred, truth, keep, plan, reference out, bound), computed once"""
    key = (shape, img, kp)
    if key not in _CASES:
        R, N, C, H, W = shape
        pred, truth = MR.draw_images(img, R, N, C, H, W)
        keep = MR.draw_keep(kp, N, C, H, W)
        plan = _plan(shape)
        ref = MR.reference(pred, truth, keep)
        _CASES[key] = (pred, truth, keep, plan, ref["out"], MB.out_bound(ref, plan.tile_h, plan.tile_w))
    return _CASES[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_emulation_stays_inside_the_bound(shape):
    worst = 0.0
    for img, kp in CLASSES:
        pred, truth, keep, plan, ref_out, bound = _case(shape, img, kp)
        assert bool(torch.isfinite(bound).all()), (img, kp)
        ratio = MB.check(f"{img}/{kp}", emulate(pred, truth, keep, plan), ref_out, bound)
        worst = max(worst, ratio)
        if img == "equal":                                                    # pred == truth bit for bit
            assert bool((ref_out[:, 0] == 0).all()) and bool(torch.isinf(ref_out[:, 1]).all())
    print(f"emulation {shape}: largest error / bound = {worst:.3f}")
    assert 0 < worst <= 1


def test_the_bound_of_constant_areas_carries_no_cancellation():
    """a two-level image: where a tile is constant the pivot makes the moments exact, so the bound of those positions is the double
    term alone; across a level change it is gamma times the SQUARED step, against C2 = 3.6e-3"""
    pred, truth, keep, plan, ref_out, bound = _case(SHAPES[0], "two_level", "none")
    assert float(bound[:, 2].max()) < 2e-3 and float(bound[:, 2].min()) > 0


@pytest.mark.parametrize("fault", FAULTS)
def test_a_planted_fault_leaves_the_bound(fault):
    left = []
    for shape in SHAPES[:2]:
        for img, kp in CLASSES:
            pred, truth, keep, plan, ref_out, bound = _case(shape, img, kp)
            try:
                MB.check(fault, emulate(pred, truth, keep, plan, fault=fault), ref_out, bound)
            except AssertionError:
                left.append((shape, img, kp))
    print(f"{fault}: outside the bound on {len(left)} of {2 * len(CLASSES)} cases")
    assert left, fault
