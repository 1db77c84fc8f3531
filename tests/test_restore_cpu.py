"""The restoration ABI and its CPU restatement without a GPU: include/mdm_restore.h parses to its three functions and is bound next
to the other headers without entering their tables, every `mdm_restore_*` symbol has a kernel-level test, the restatement of the
loop (tests/_restore_ref.py) is the pinned oracle bit for bit when the projection is skipped, the numpy statement of the projection
is the orthogonal projection onto the measurement, and the host helpers refuse what they state.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _restore_ref as RR
from golden.make_golden import TINY, base_args, seed_all
from mdm import _lib
from oracle.sampler_ref import SamplerRef
from oracle.scheduler_ref import SchedulerRef
from oracle.unet_ref import UNetRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
RESTORE_HEADER = os.path.join(ROOT, "include", "mdm_restore.h")
_K = "test_restore_kernels_gpu"
COVERAGE = {"mdm_restore_x0": (_K, "mdm_restore_x0"), "mdm_restore_measure": (_K, "mdm_restore_measure"),
            "mdm_restore_start": (_K, "mdm_restore_start")}
X0_PARAMS = ["dtype", "pred_nhwc", "Cp", "x_in", "s", "y", "k", "gray", "N", "C", "H", "W", "pred_nchw", "shifted0", "x0_hat", "stream"]
MEASURE_PARAMS = ["x", "k", "gray", "N", "C", "H", "W", "y", "stream"]
START_PARAMS = ["y", "k", "gray", "per_channel", "N", "C", "H", "W", "mu", "expand", "stream"]
NAMES = ["mdm_restore_x0", "mdm_restore_measure", "mdm_restore_start"]


# ------------------------------------------------------------------ the ninth header and its tables
def test_the_header_parses_to_exactly_the_three_names():
    structs, protos = _lib.parse_header(open(RESTORE_HEADER).read())
    assert structs == {} and list(protos) == NAMES
    assert [n for n, _ in protos["mdm_restore_x0"][1]] == X0_PARAMS
    assert [n for n, _ in protos["mdm_restore_measure"][1]] == MEASURE_PARAMS
    assert [n for n, _ in protos["mdm_restore_start"][1]] == START_PARAMS
    x = dict(protos["mdm_restore_x0"][1])
    assert (x["pred_nhwc"], x["y"], x["k"], x["gray"], x["x0_hat"]) == ("void*", "float*", "int", "int", "float*")
    assert all(p[0] == "int" for p in protos.values())
    # mdm_sampler_x0's parameters with y, k, gray put in: the kernel takes its place launch for launch
    parent = _lib._PARAMS["mdm_sampler_x0"]
    assert [p for p in X0_PARAMS if p not in ("y", "k", "gray")] == parent


def test_every_restore_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_restore_[a-z0-9_]+)\s*\(", open(RESTORE_HEADER).read()))
    assert declared == set(_lib.RESTORE_EXPORTS) == set(_lib.RESTORE_PROTOS) == set(_lib.RESTORE_PARAMS) == set(NAMES)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    for name in _lib.RESTORE_EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.RESTORE_PROTOS[name][0] and fn.restype is i32, name
    assert _lib.RESTORE_PROTOS["mdm_restore_x0"][0] == [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    assert _lib.RESTORE_PROTOS["mdm_restore_measure"][0] == [vp, i32, i32, i32, i32, i32, i32, vp, vp]
    assert _lib.RESTORE_PROTOS["mdm_restore_start"][0] == [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    assert os.path.samefile(_lib.RESTORE_HEADER_PATH, RESTORE_HEADER)


def test_the_tables_stay_apart():
    others = [("mdm_hip.h", _lib.EXPORTS), ("mdm_vis.h", _lib.VIS_EXPORTS), ("mdm_data.h", _lib.DATA_EXPORTS),
              ("mdm_interp.h", _lib.INTERP_EXPORTS), ("mdm_ingest.h", _lib.INGEST_EXPORTS), ("mdm_neighbor.h", _lib.NEIGHBOR_EXPORTS),
              ("mdm_inpaint.h", _lib.INPAINT_EXPORTS), ("mdm_metric.h", _lib.METRIC_EXPORTS)]
    for header, exports in others:
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not [n for n in exports if n.startswith("mdm_restore_")] and "mdm_restore" not in text, header
    assert len(_lib.INPAINT_EXPORTS) == 2
    for name in _lib.RESTORE_EXPORTS:
        assert name in _lib._ALL_PROTOS and name in _lib._ALL_PARAMS and name not in _lib._PROTOS
    assert _lib.RESTORE_PARAMS == {"mdm_restore_x0": X0_PARAMS, "mdm_restore_measure": MEASURE_PARAMS, "mdm_restore_start": START_PARAMS}


def test_call_binds_restore_keywords_against_the_restore_header():
    kw = dict(x=1, k=2, gray=0, N=2, C=3, H=4, W=4, y=5, stream=None)
    with _lib.Recording() as rec:
        _lib.call("mdm_restore_measure", **kw)
        with pytest.raises(TypeError, match="mdm_restore_measure"):
            _lib.call("mdm_restore_measure", **dict(kw, pool=2))
        with pytest.raises(TypeError, match="mdm_restore_start"):
            _lib.call("mdm_restore_start", y=1, k=2, gray=0, N=1, C=1, H=4, W=4, mu=None, expand=2, stream=None)     # per_channel is missing
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_restore_measure", (1, 2, 0, 2, 3, 4, 4, 5))]


def test_every_restore_symbol_has_a_kernel_test():
    assert set(COVERAGE) == set(_lib.RESTORE_PROTOS)
    for sym, (mod, mention) in COVERAGE.items():
        text = open(os.path.join(TESTS, mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), f"{mod}.py does not mention {mention}"
        assert "pytest.mark.gpu" in text


# ------------------------------------------------------------------ the restatement against the pinned oracle
def _pair(**kw):
    a = base_args(data_size=16, ddpm_num_steps=6, sample_num=2, sample_latent_shape="uniform", **kw)
    s = SchedulerRef(a)
    s.update_ddpm_num_steps(6)
    return a, s, s.get_timesteps_epoch(0, 1)


def _truth(n, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, 16, 16, generator=g) * 2 - 1


CONFIGS = [dict(sampling_mask_dependency=dep, momentum_adaptive=mode, **extra)
           for dep, extra in (("independent", {}), ("dependent_prev", {}),
                              ("dependent_t", dict(mean_option="degraded_area", ddpm_schedule="exponential")))     # (ratios >= 0.1: no 0 / 0 fill)
           for mode in ("base_sampling", "base_momentum")]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"{c['sampling_mask_dependency']}-{c['momentum_adaptive']}" for c in CONFIGS])
def test_the_projection_skipped_is_the_oracle_bit_for_bit(cfg):
    a, s, ts = _pair(**cfg)
    net = UNetRef(TINY).eval()
    seed_all(5)
    x0, hist = SamplerRef(None, a, s, [None] * 3).sample(net, ts)
    after = torch.rand(4)
    seed_all(5)
    y = RR.measure_t(_truth(2), 2, False)
    y0, yhist = RR.RestoreSamplerRef(None, a, s, [None] * 3).sample_restore(net, ts, y, 2, False, project=False)
    assert torch.equal(after, torch.rand(4))                                 # the same draws were consumed
    assert len(yhist) == 11 and np.array_equal(x0.numpy().view(np.uint32), y0.numpy().view(np.uint32)) and bool(torch.isfinite(x0).all())
    for k, h, yh in zip(RR.HISTORY_NAMES, hist, yhist):
        assert h.shape == yh.shape and np.array_equal(h.numpy().view(np.uint32), yh.numpy().view(np.uint32)), k
    assert float(hist[RR.HISTORY_NAMES.index("difference")].abs().max()) > 0


@pytest.mark.parametrize("pool,gray", [(2, False), (4, True), (1, True)])
@pytest.mark.parametrize("start", RR.STARTS)
def test_the_restatement_returns_an_image_with_the_measurement(pool, gray, start):
    a, s, ts = _pair(mean_area="channel-wise")
    y = RR.measure_t(_truth(2), pool, gray)
    seed_all(6)
    ref = RR.RestoreSamplerRef(None, a, s, [None] * 3)
    x0, hist = ref.sample_restore(UNetRef(TINY).eval(), ts, y, pool, gray, start)
    assert float((RR.measure_t(x0, pool, gray) - y).abs().max()) < 1e-5 and bool(torch.isfinite(x0).all())
    first = hist[RR.HISTORY_NAMES.index("sample_t")][1]
    if start == "measured":                                                  # a constant per channel (colour) / per image (gray)
        dims = (1, 2, 3) if gray else (2, 3)
        want = y.double().mean(dim=dims, keepdim=True).float().expand(2, 3, 16, 16)
        assert torch.equal(first, want)
    else:
        assert bool((first == first[:, :, :1, :1]).all())


# ------------------------------------------------------------------ the numpy projection is the orthogonal projection
GROUPS = [(1, 1, 3), (2, 0, 3), (2, 1, 3), (4, 0, 1), (4, 1, 3), (8, 0, 3), (8, 1, 3), (2, 1, 1)]


@pytest.mark.parametrize("k,gray,C", GROUPS, ids=[f"k{k}-gray{g}-C{c}" for k, g, c in GROUPS])
def test_the_numpy_projection_is_the_orthogonal_projection(k, gray, C):
    g = np.random.default_rng(100 * k + 10 * gray + C)
    N, H, W = 3, 16, 24
    x = (g.random((N, C, H, W)) * 2 - 1).astype(np.float32)
    y = (g.random((N, 1 if gray else C, H // k, W // k)) * 2 - 1).astype(np.float32)
    p = RR.project_np(x, y, k, gray)
    # inside the fp64 bound, element by element
    ref, bound = RR.project_ref(x, y, k, gray)
    assert (np.abs(p.astype(np.float64) - ref) <= bound).all()
    # measure(x') = y: the fp32 mean of x' lies within its own bound of the exact mean of x', which lies within `bound` of y
    m, Em = RR.mean_ref(p, k, gray)
    gb = RR.to_groups(bound, k, gray).max(-1)
    assert (np.abs(RR.measure_np(p, k, gray).astype(np.float64) - y) <= Em + gb).all()
    # x' - x is constant on a group, to the rounding of x + d (u relative of x')
    step = RR.to_groups(p.astype(np.float64) - x, k, gray)
    slack = RR.U * RR.to_groups(np.abs(p).astype(np.float64), k, gray).max(-1)
    assert (step.max(-1) - step.min(-1) <= 2 * slack).all()
    # projecting x' again moves nothing beyond the bound
    pp = RR.project_np(p, y, k, gray)
    _, bound2 = RR.project_ref(p, y, k, gray)
    assert (np.abs(pp.astype(np.float64) - p) <= bound2 + RR.from_groups(Em + gb, k, gray, C)).all()
    # with y = measure(x) nothing moves beyond the bound
    same = RR.project_np(x, RR.measure_np(x, k, gray), k, gray)
    _, Emx = RR.mean_ref(x, k, gray)
    assert (np.abs(same.astype(np.float64) - x) <= RR.from_groups(Emx, k, gray, C) * (1 + RR.U) + RR.U * np.abs(x)).all()
    # the stated order: a k = 8 group is left strip + right strip, and its sum differs from a plain row-major one somewhere
    if k == 8 and not gray:
        v = x.reshape(N, C, H // 8, 8, W // 8, 8)
        left = np.zeros((N, C, H // 8, W // 8), np.float32)
        right = left.copy()
        for r in range(8):
            for j in range(4):
                left = left + v[:, :, :, r, :, j]
                right = right + v[:, :, :, r, :, 4 + j]
        assert np.array_equal(RR.group_sum_np(x, k, gray), left + right)


def test_a_nan_stays_in_its_group():
    x = np.linspace(-1, 1, 2 * 3 * 8 * 8, dtype=np.float32).reshape(2, 3, 8, 8)
    y = np.zeros((2, 1, 2, 2), np.float32)
    x[1, 2, 5, 6] = np.nan
    y[0, 0, 0, 1] = np.nan
    p = RR.project_np(x, y, 4, 1)
    want = np.zeros((2, 3, 8, 8), bool)
    want[1, :, 4:, 4:] = True
    want[0, :, :4, 4:] = True
    assert np.array_equal(np.isnan(p), want)


# ------------------------------------------------------------------ the host helpers refuse before anything is launched
def test_host_helpers_name_the_argument():
    import mdm
    x = torch.zeros(2, 3, 8, 8)
    bad = [
        (lambda: mdm.restore_measure(x, 3), ValueError, "pool"), (lambda: mdm.restore_measure(x, 16), ValueError, "pool"),
        (lambda: mdm.restore_measure(x, 2.0), ValueError, "pool"), (lambda: mdm.restore_measure(x, True), ValueError, "pool"),
        (lambda: mdm.restore_measure(x, 1), ValueError, "pool=1"), (lambda: mdm.restore_measure(x[:, :1].contiguous(), 1, gray=True), ValueError, "pool=1"),
        (lambda: mdm.restore_measure(x, 2, gray=2), ValueError, "gray"), (lambda: mdm.restore_measure(x, 2, gray="yes"), ValueError, "gray"),
        (lambda: mdm.restore_measure(x.double(), 2), TypeError, "x"), (lambda: mdm.restore_measure(x.numpy(), 2), TypeError, "x"),
        (lambda: mdm.restore_measure(x.transpose(2, 3)[:, :, :, :4], 2), ValueError, "x"), (lambda: mdm.restore_measure(x[0], 2), ValueError, "x"),
        (lambda: mdm.restore_measure(torch.zeros(2, 3, 8, 12), 8), ValueError, "x"),
        (lambda: mdm.restore_measure(torch.zeros(2, 9, 8, 8), 2), ValueError, "x"),
        (lambda: mdm.restore_expand(torch.zeros(2, 3, 4, 4), 3, 2, gray=True), ValueError, "y"),
        (lambda: mdm.restore_expand(torch.zeros(2, 1, 4, 4), 3, 2), ValueError, "y"),
        (lambda: mdm.restore_expand(torch.zeros(2, 3, 4, 4).half(), 3, 2), TypeError, "y"),
        (lambda: mdm.restore_expand(torch.zeros(2, 3, 4, 4), 0, 2), ValueError, "channels"),
        (lambda: mdm.restore_expand(torch.zeros(2, 3, 4, 4), 3, 5), ValueError, "pool"),
        (lambda: mdm.restore_expand(torch.zeros(2, 3, 4, 4), 3, 1), ValueError, "pool=1"),
        (lambda: mdm.restore_expand(torch.zeros(3, 4, 4), 3, 2), ValueError, "y"),
    ]
    for f, err, word in bad:
        with pytest.raises(err, match=word):
            f()


def test_sampler_refusals_name_the_argument():
    """the checks of `sample_restore` run before any host draw and before any launch"""
    import mdm
    a = base_args(data_size=16, ddpm_num_steps=6, sample_num=2, sample_latent_shape="uniform")
    smp = mdm.Sampler(None, a, type("S", (), {"device": torch.device("cpu")})(), [None] * 3)
    y = torch.zeros(2, 3, 8, 8)
    bad = [
        (dict(start="matched"), ValueError, "start"), (dict(start="known_mean"), ValueError, "start"),
        (dict(pool=3), ValueError, "pool"), (dict(pool=1), ValueError, "pool=1"), (dict(gray=3), ValueError, "gray"),
        (dict(measurement=y.double()), TypeError, "measurement"), (dict(measurement=y.numpy()), TypeError, "measurement"),
        (dict(measurement=y[:1].contiguous()), ValueError, "measurement"), (dict(measurement=y[:, :1].contiguous()), ValueError, "measurement"),
        (dict(measurement=y, gray=True), ValueError, "measurement"), (dict(measurement=torch.zeros(2, 3, 4, 4)), ValueError, "measurement"),
        (dict(measurement=y.transpose(2, 3)), ValueError, "measurement"), (dict(measurement=y, pool=4), ValueError, "measurement"),
    ]
    for change, err, word in bad:
        kw = dict(dict(measurement=y, pool=2, gray=False, start="latent"), **change)
        seed_all(0)
        with pytest.raises(err, match=word):
            smp.sample_restore(None, [1, 2, 3], kw["measurement"], kw["pool"], kw["gray"], kw["start"])
        assert torch.equal(torch.rand(2), (seed_all(0), torch.rand(2))[1])   # refused before any host draw
    with pytest.raises(ValueError, match="inpaint and restore"):
        smp._sample_mean_shift_momentum(None, [1], inpaint=(y, y), restore=(y, 2, 0))
