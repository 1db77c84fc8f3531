"""The inpainting ABI and its CPU restatement without a GPU: include/mdm_inpaint.h parses to its two functions and is bound next to the
other headers without entering their tables, every `mdm_inpaint_*` symbol has a kernel-level test, the restatement of the loop
(tests/_inpaint_ref.py) is the pinned oracle bit for bit when nothing is given and returns `known` when everything is, and the two
host helpers `mdm.inpaint_start_index` / `mdm.inpaint_keep` do what they state.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _inpaint_ref as PR
from golden.make_golden import TINY, base_args, seed_all
from mdm import _lib
from oracle.sampler_ref import SamplerRef
from oracle.scheduler_ref import SchedulerRef
from oracle.unet_ref import UNetRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
INPAINT_HEADER = os.path.join(ROOT, "include", "mdm_inpaint.h")
_K = "test_inpaint_kernels_gpu"
COVERAGE = {"mdm_inpaint_x0": (_K, "mdm_inpaint_x0"), "mdm_inpaint_start": (_K, "mdm_inpaint_start")}
X0_PARAMS = ["dtype", "pred_nhwc", "Cp", "x_in", "s", "known", "keep", "keep_C", "N", "C", "H", "W", "pred_nchw", "shifted0", "x0_hat",
             "stream"]
START_PARAMS = ["known", "keep", "keep_C", "fallback", "per_channel", "N", "C", "HW", "x_start", "mu", "unknown", "stream"]


# ------------------------------------------------------------------ the seventh header and its tables
def test_the_header_parses_to_exactly_the_two_names():
    structs, protos = _lib.parse_header(open(INPAINT_HEADER).read())
    assert structs == {} and list(protos) == ["mdm_inpaint_x0", "mdm_inpaint_start"]
    assert [n for n, _ in protos["mdm_inpaint_x0"][1]] == X0_PARAMS
    assert [n for n, _ in protos["mdm_inpaint_start"][1]] == START_PARAMS
    x = dict(protos["mdm_inpaint_x0"][1])
    assert (x["pred_nhwc"], x["known"], x["keep"], x["keep_C"], x["x0_hat"]) == ("void*", "float*", "float*", "int", "float*")
    s = dict(protos["mdm_inpaint_start"][1])
    assert (s["fallback"], s["per_channel"], s["HW"], s["mu"], s["unknown"]) == ("float*", "int", "int", "float*", "int32_t*")
    assert all(p[0] == "int" for p in protos.values())


def test_every_inpaint_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_inpaint_[a-z0-9_]+)\s*\(", open(INPAINT_HEADER).read()))
    assert declared == set(_lib.INPAINT_EXPORTS) == set(_lib.INPAINT_PROTOS) == set(_lib.INPAINT_PARAMS) and len(declared) == 2
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    for name in _lib.INPAINT_EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.INPAINT_PROTOS[name][0] and fn.restype is i32, name
    assert _lib.INPAINT_PROTOS["mdm_inpaint_x0"][0] == [i32, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    assert _lib.INPAINT_PROTOS["mdm_inpaint_start"][0] == [vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    assert os.path.samefile(_lib.INPAINT_HEADER_PATH, INPAINT_HEADER)


def test_the_tables_stay_apart():
    others = [("mdm_hip.h", _lib.EXPORTS, 92), ("mdm_vis.h", _lib.VIS_EXPORTS, 3), ("mdm_data.h", _lib.DATA_EXPORTS, 2),
              ("mdm_interp.h", _lib.INTERP_EXPORTS, 3), ("mdm_ingest.h", _lib.INGEST_EXPORTS, None),
              ("mdm_neighbor.h", _lib.NEIGHBOR_EXPORTS, None)]
    for header, exports, count in others:
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not [n for n in exports if n.startswith("mdm_inpaint_")] and "mdm_inpaint" not in text, header
        assert count is None or len(exports) == count, header
    for name in _lib.INPAINT_EXPORTS:
        assert name in _lib._ALL_PROTOS and name in _lib._ALL_PARAMS and name not in _lib._PROTOS
    assert _lib.INPAINT_PARAMS == {"mdm_inpaint_x0": X0_PARAMS, "mdm_inpaint_start": START_PARAMS}


def test_call_binds_inpaint_keywords_against_the_inpaint_header():
    kw = dict(known=1, keep=2, keep_C=1, fallback=3, per_channel=0, N=2, C=3, HW=16, x_start=4, mu=5, unknown=6, stream=None)
    with _lib.Recording() as rec:
        _lib.call("mdm_inpaint_start", **kw)
        with pytest.raises(TypeError, match="mdm_inpaint_start"):
            _lib.call("mdm_inpaint_start", **dict(kw, given=1))
        with pytest.raises(TypeError, match="mdm_inpaint_x0"):
            _lib.call("mdm_inpaint_x0", dtype=0, pred_nhwc=1, Cp=8, x_in=2, s=3, known=4, keep=5, N=1, C=1, H=4, W=4, pred_nchw=None,
                      shifted0=None, x0_hat=6, stream=None)                      # keep_C is missing
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_inpaint_start", (1, 2, 1, 3, 0, 2, 3, 16, 4, 5, 6))]


def test_every_inpaint_symbol_has_a_kernel_test():
    """as tests/test_interp_cpu.py does for the interpolation header"""
    assert set(COVERAGE) == set(_lib.INPAINT_PROTOS)
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


def _known(n, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, 16, 16, generator=g) * 2 - 1


CONFIGS = [dict(sampling_mask_dependency=dep, momentum_adaptive=mode, **extra)
           for dep, extra in (("independent", {}), ("dependent_prev", {}),
                              ("dependent_t", dict(mean_option="degraded_area", ddpm_schedule="exponential")))     # (ratios >= 0.1: no 0 / 0 fill)
           for mode in ("base_sampling", "base_momentum")]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"{c['sampling_mask_dependency']}-{c['momentum_adaptive']}" for c in CONFIGS])
def test_nothing_given_is_the_oracle_bit_for_bit(cfg):
    a, s, ts = _pair(**cfg)
    net = UNetRef(TINY).eval()
    seed_all(5)
    x0, hist = SamplerRef(None, a, s, [None] * 3).sample(net, ts)
    after = torch.rand(4)
    seed_all(5)
    y0, yhist = PR.InpaintSamplerRef(None, a, s, [None] * 3).sample_inpaint(net, ts, _known(2), torch.zeros(2, 1, 16, 16))
    assert torch.equal(after, torch.rand(4))                                 # the same draws were consumed
    assert len(yhist) == 11 and np.array_equal(x0.numpy().view(np.uint32), y0.numpy().view(np.uint32)) and bool(torch.isfinite(x0).all())
    for k, h, y in zip(PR.HISTORY_NAMES, hist, yhist):
        assert h.shape == y.shape and np.array_equal(h.numpy().view(np.uint32), y.numpy().view(np.uint32)), k
    assert float(hist[PR.HISTORY_NAMES.index("difference")].abs().max()) > 0


@pytest.mark.parametrize("start", PR.STARTS)
@pytest.mark.parametrize("ck", [1, 3])
def test_everything_given_returns_known(start, ck):
    a, s, ts = _pair()
    known = _known(2)
    seed_all(6)
    x0, hist = PR.InpaintSamplerRef(None, a, s, [None] * 3).sample_inpaint(UNetRef(TINY).eval(), ts, known, torch.ones(2, ck, 16, 16), start)
    assert torch.equal(x0, known)
    h0 = hist[PR.HISTORY_NAMES.index("sample_0")]
    steps = 1 if start == "matched" else len(ts)                             # no hole: the first used timestep already reaches it
    assert all(torch.equal(h0[k], known) for k in range(1, steps + 1)) and not h0[0].any() and not h0[steps + 1:].any()


def test_the_starts_of_the_restatement():
    a, s, ts = _pair(mean_area="channel-wise")
    known = _known(2)
    keep = torch.ones(2, 1, 16, 16)
    keep[0, :, 4:12, 4:12] = 0
    keep[1] = 0                                                              # nothing given: the latent row
    ref = PR.InpaintSamplerRef(None, a, s, [None] * 3)
    seed_all(8)
    latent, unknown = ref._start(None, known, keep, "latent")
    assert unknown.tolist() == [64, 256]
    seed_all(8)
    mean, _ = ref._start(None, known, keep, "known_mean")
    seed_all(8)
    matched, _ = ref._start(None, known, keep, "matched")
    g = (keep[0] != 0).expand(3, 16, 16)
    want = torch.stack([known[0, c][g[c]].double().mean().float() for c in range(3)])
    assert torch.equal(mean[0], want[:, None, None].expand(3, 16, 16)) and torch.equal(mean[1], latent[1])
    assert torch.equal(matched[0], torch.where(g, known[0], mean[0])) and torch.equal(matched[1], latent[1])
    a.mean_area = "image-wise"
    seed_all(8)
    mean1, _ = ref._start(None, known, keep, "known_mean")
    assert torch.equal(mean1[0], known[0][g].double().mean().float().expand(3, 16, 16))


# ------------------------------------------------------------------ inpaint_start_index
def test_start_index():
    import mdm
    ratio = torch.tensor(np.linspace(1e-3, 1, 10))                           # the linear table of 10 steps, fp64
    ts = list(range(1, 11))
    f = mdm.inpaint_start_index
    assert f(ratio, ts, 0.0) == 0                                            # no hole: the first used timestep
    assert f(ratio, ts, float(ratio[3])) == 3                                # equal to an entry: that entry (>=)
    assert f(ratio, ts, (float(ratio[3]) + float(ratio[4])) / 2) == 4        # between two entries: the upper one
    assert f(ratio, ts, np.nextafter(float(ratio[3]), 2.0)) == 4
    assert f(ratio, ts, 1.0) == 9 and f(ratio, ts, 1.5) == 9                 # above the last entry: the whole list
    strided = [2, 4, 6, 8, 10]
    assert f(ratio, strided, 0.0) == 0 and f(ratio, strided, float(ratio[3])) == 1 and f(ratio, strided, float(ratio[4])) == 2
    assert f(ratio, strided, float(ratio[9])) == 4 and f(ratio, strided[:3], 0.99) == 2
    for frac in (0.0, 0.25, float(ratio[5]), 0.77, 2.0):
        for tl in (ts, strided, [3, 7, 10]):
            assert f(ratio, tl, frac) == PR.start_index(ratio, tl, frac) == f(ratio.numpy(), tl, frac)


def test_start_index_of_a_quarter_box_on_the_linear_schedule():
    import mdm
    a, s, ts = _pair()
    frac = float((mdm.inpaint_keep("box", 1, 16, 16, top=4, left=4, height=8, width=8) == 0).sum()) / 256
    assert frac == 0.25
    j = mdm.inpaint_start_index(s.ratio_list, ts, frac)
    assert ts == [1, 2, 3, 4, 5, 6] and j == 2 and s.ratio_list[1] < 0.25 <= s.ratio_list[2]


# ------------------------------------------------------------------ inpaint_keep
def test_keep_masks():
    import mdm
    N, H, W = 3, 6, 7
    box = mdm.inpaint_keep("box", N, H, W, top=1, left=2, height=3, width=4)
    want = torch.ones(N, 1, H, W)
    want[:, :, 1:4, 2:6] = 0
    assert box.shape == (N, 1, H, W) and box.dtype == torch.float32 and box.is_contiguous() and torch.equal(box, want)
    assert torch.equal(mdm.inpaint_keep("box", N, H, W, top=0, left=0, height=0, width=0), torch.ones(N, 1, H, W))
    assert not mdm.inpaint_keep("box", N, H, W, top=0, left=0, height=H, width=W).any()
    cols, rows = torch.arange(W).expand(N, 1, H, W), torch.arange(H)[:, None].expand(N, 1, H, W)
    for side, w in (("left", cols >= W // 2), ("right", cols < W - W // 2), ("top", rows >= H // 2), ("bottom", rows < H - H // 2)):
        got = mdm.inpaint_keep("half", N, H, W, side=side)
        assert got.is_contiguous() and torch.equal(got, w.float()), side
    u = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(4))
    r1 = mdm.inpaint_keep("random", N, H, W, p=0.3, generator=torch.Generator().manual_seed(4))
    r2 = mdm.inpaint_keep("random", N, H, W, p=0.3, generator=torch.Generator().manual_seed(4))
    r3 = mdm.inpaint_keep("random", N, H, W, p=0.3, generator=torch.Generator().manual_seed(5))
    assert torch.equal(r1, (u >= 0.3).float()) and torch.equal(r1, r2) and not torch.equal(r1, r3)
    assert not mdm.inpaint_keep("random", N, H, W, p=1.0, generator=torch.Generator().manual_seed(4)).any()
    assert mdm.inpaint_keep("random", N, H, W, p=0.0, generator=torch.Generator().manual_seed(4)).all()
    for bad, err in ((("blob", N, H, W), ValueError), (("box", N, H, W), TypeError), (("half", N, H, W, dict(side="middle")), ValueError),
                     (("box", N, H, W, dict(top=4, left=0, height=3, width=1)), ValueError), (("half", N, H, W, dict(p=1)), TypeError)):
        kw = bad[4] if len(bad) > 4 else {}
        with pytest.raises(err):
            mdm.inpaint_keep(*bad[:4], **kw)
