"""The interpolation-sampler ABI and its CPU restatement without a GPU: include/mdm_interp.h parses to its three functions and is
bound next to the other three headers without entering their tables, every `mdm_interp_*` symbol has a kernel-level test, the torch
restatement of the four upstream functions (tests/_interp_ref.py) reproduces the reference's trajectories of
tests/golden/sampler_interp.npz and its failures, the ramp of start colours has its closed form, and the host predictor of the
device row is its scalar statement and none of its wrong twins.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _interp_ref as IR
from _dropout_ref import philox4x32_10
from _philox_ref import u01
from golden.make_golden import TINY, base_args, seed_all
from mdm import _lib
from oracle.unet_ref import UNetRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
INTERP_HEADER = os.path.join(ROOT, "include", "mdm_interp.h")
_K = "test_interp_kernels_gpu"
COVERAGE = {"mdm_interp_shift": (_K, "mdm_interp_shift"), "mdm_interp_row_mask": (_K, "mdm_interp_row_mask"),
            "mdm_interp_update": (_K, "mdm_interp_update")}
SHIFT_PARAMS = ["x_t", "mu", "ratio", "shift", "N", "C", "H", "W", "s", "x_in", "dtype", "x_in_nhwc", "Cp", "stream"]
ROW_PARAMS = ["amount", "u_row", "rng", "N", "C", "HW", "mask", "stream"]
UPDATE_PARAMS = ["d_t", "d_next", "x_t", "diff", "update", "n", "stream"]


# ------------------------------------------------------------------ the fourth header and the four tables
def test_the_header_parses_to_exactly_the_three_names():
    structs, protos = _lib.parse_header(open(INTERP_HEADER).read())
    assert structs == {} and list(protos) == ["mdm_interp_shift", "mdm_interp_row_mask", "mdm_interp_update"]
    assert [n for n, _ in protos["mdm_interp_shift"][1]] == SHIFT_PARAMS
    assert [n for n, _ in protos["mdm_interp_row_mask"][1]] == ROW_PARAMS
    assert [n for n, _ in protos["mdm_interp_update"][1]] == UPDATE_PARAMS
    s = dict(protos["mdm_interp_shift"][1])
    assert (s["mu"], s["ratio"], s["shift"], s["x_in_nhwc"]) == ("float*", "double*", "float", "void*")
    assert dict(protos["mdm_interp_row_mask"][1])["rng"] == "uint64_t*" and dict(protos["mdm_interp_update"][1])["n"] == "int64_t"
    assert all(p[0] == "int" for p in protos.values())


def test_every_interp_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_interp_[a-z0-9_]+)\s*\(", open(INTERP_HEADER).read()))
    assert declared == set(_lib.INTERP_EXPORTS) == set(_lib.INTERP_PROTOS) == set(_lib.INTERP_PARAMS) and len(declared) == 3
    C = ctypes
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    for name in _lib.INTERP_EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.INTERP_PROTOS[name][0] and fn.restype is i32, name
    assert _lib.INTERP_PROTOS["mdm_interp_shift"][0] == [vp, vp, vp, f32, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp]
    assert _lib.INTERP_PROTOS["mdm_interp_row_mask"][0] == [vp, vp, vp, i32, i32, i32, vp, vp]
    assert _lib.INTERP_PROTOS["mdm_interp_update"][0] == [vp, vp, vp, vp, i32, i64, vp]
    assert os.path.samefile(_lib.INTERP_HEADER_PATH, INTERP_HEADER)


def test_the_four_tables_are_still_exactly_their_headers():
    text = {n: open(os.path.join(ROOT, "include", n)).read() for n in ("mdm_hip.h", "mdm_vis.h", "mdm_data.h", "mdm_interp.h")}
    rows = [("mdm_hip.h", r"mdm_", _lib.EXPORTS, _lib._PROTOS, _lib._PARAMS, 92), ("mdm_vis.h", r"mdm_vis_", _lib.VIS_EXPORTS, _lib.VIS_PROTOS, _lib.VIS_PARAMS, 3),
            ("mdm_data.h", r"mdm_data_", _lib.DATA_EXPORTS, _lib.DATA_PROTOS, _lib.DATA_PARAMS, 2),
            ("mdm_interp.h", r"mdm_interp_", _lib.INTERP_EXPORTS, _lib.INTERP_PROTOS, _lib.INTERP_PARAMS, 3)]
    for header, prefix, exports, protos, params, count in rows:
        declared = re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text[header])
        assert set(exports) == set(protos) == set(params) == set(declared) and len(exports) == count, header
    for header, _, exports, *_ in rows[:3]:
        assert not [n for n in exports if n.startswith("mdm_interp_")] and "mdm_interp" not in text[header], header


def test_a_header_that_breaks_the_rules_is_refused(tmp_path):
    """prefix only, no struct, no name declared twice: the one loop keeps the checks of the three blocks it replaced"""
    core = os.path.join(ROOT, "include", "mdm_hip.h")
    for body in ("int mdm_other_thing(int a, void* stream);", "typedef struct mdm_x_s { int a; } mdm_x_t;",
                 "int mdm_version(void);"):
        bad = tmp_path / "bad.h"
        bad.write_text(body + "\n")
        with pytest.raises(RuntimeError, match="functions only"):
            _lib._read_headers(core, ((str(bad), "mdm_"),) if "version" in body else ((str(bad), "mdm_x_"),))
    twice = tmp_path / "twice.h"
    twice.write_text("int mdm_x_a(void* stream);\n")
    with pytest.raises(RuntimeError, match="twice"):
        _lib._read_headers(core, ((str(twice), "mdm_x_"), (str(twice), "mdm_x_")))
    with pytest.raises(RuntimeError, match="missing"):
        _lib._read_headers(core, ((str(tmp_path / "absent.h"), "mdm_x_"),))


def test_call_binds_interp_keywords_against_the_interp_header():
    kw = dict(d_t=1, d_next=2, x_t=3, diff=4, update=1, n=5, stream=None)
    with _lib.Recording() as rec:
        _lib.call("mdm_interp_update", **kw)
        with pytest.raises(TypeError, match="mdm_interp_update"):
            _lib.call("mdm_interp_update", d_t=1, momentum=2)
        with pytest.raises(TypeError, match="mdm_interp_row_mask"):
            _lib.call("mdm_interp_row_mask", amount=1, u=2, rng=3, N=1, C=1, HW=4, mask=5, stream=None)
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_interp_update", (1, 2, 3, 4, 1, 5))]


def test_every_interp_symbol_has_a_kernel_test():
    """as tests/test_data_cpu.py does for the data header"""
    assert set(COVERAGE) == set(_lib.INTERP_PROTOS)
    for sym, (mod, mention) in COVERAGE.items():
        text = open(os.path.join(TESTS, mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), f"{mod}.py does not mention {mention}"
        assert "pytest.mark.gpu" in text


# ------------------------------------------------------------------ the restatement against the reference's trajectories
def _ref_run(cfg, seed=None):
    a, shift = IR.fixture_args(cfg, base_args)
    s = IR.InterpSchedulerRef(a)
    s.update_ddpm_num_steps(a.ddpm_num_steps)
    ts = s.get_timesteps_epoch(0, 1)
    smp = IR.InterpSamplerRef(None, a, s, [None] * 3)
    if seed is not None:
        seed_all(seed)
    return ts, smp, shift, smp._sample_interpolation(UNetRef(TINY).eval(), ts, shift)


def test_restatement_reproduces_the_reference(golden):
    g = golden("sampler_interp")
    assert int(g["interp_n"]) == 4
    names = IR.INTERP_HISTORY_NAMES
    for i in range(int(g["interp_n"])):
        ts, smp, shift, (x0, mu, hist) = _ref_run(g[f"interp{i}_cfg"], int(g[f"interp{i}_seed"]))
        assert ts == list(g[f"interp{i}_ts"]) and len(hist) == 10
        ref = IR.fixture_hist(g, i, smp._get_latent_initial_interpolation(shift)[0].numpy())
        assert np.array_equal(mu.numpy(), g[f"interp{i}_mu"]) and mu.shape == (4, 1, 1, 1)
        # masks and shifts are bit-exact (same RNG stream, same arithmetic); the U-Net outputs agree to fp32 rounding
        assert np.array_equal(hist[names.index("shift")].numpy(), ref[names.index("shift")]), (i, "shift")
        assert np.array_equal(hist[names.index("degraded_mask")].numpy(), ref[names.index("degraded_mask")]), (i, "mask")
        for j in range(10):
            assert np.allclose(hist[j].numpy(), ref[j], rtol=1e-4, atol=5e-5), (i, names[j])
        assert np.allclose(x0.numpy(), g[f"interp{i}_x0"], rtol=1e-4, atol=5e-5)
        T = len(ts)
        assert not ref[:, 0].any() and not ref[[names.index(k) for k in ("sample_t", "degraded_mask", "degraded_t", "difference",
                                                                         "degraded_next_t")], T].any()
    assert not g["interp3_degraded_mask"].any()              # 'indexing': counts >= 1 > u, the mask is all zero upstream
    m = g["interp0_degraded_mask"][1:-1]
    assert (m == m[:, :1, :1]).all() and 0 < m.mean() < 1    # one row for the batch and for the channels


def test_restatement_fails_like_the_reference(golden):
    g = golden("sampler_interp")
    assert int(g["interp_nfail"]) == 2
    for j in range(int(g["interp_nfail"])):
        row = g[f"interp_fail{j}"]
        with pytest.raises(Exception) as ei:
            _ref_run(row[:-1])
        assert type(ei.value).__name__ == str(row[-1]) != "none", (j, type(ei.value).__name__)
    assert {str(g[f"interp_fail{j}"][-1]) for j in range(2)} == {"UnboundLocalError", "TypeError"}


def test_dependent_consumes_the_randperms_and_nothing_else_does(golden):
    """sampler.py:293-295: 'dependent' draws sample_num randperm(HW) before the loop; any other value draws nothing there"""
    g = golden("sampler_interp")
    cfg = g["interp1_cfg"].copy()
    assert str(cfg[0]) == "dependent"
    from oracle.scheduler_ref import RecordingRng
    for dep, want in (("dependent", 4), ("independent", 0), ("anything", 0)):
        cfg[0] = dep
        a, shift = IR.fixture_args(cfg, base_args)
        s = IR.InterpSchedulerRef(a, RecordingRng())
        s.update_ddpm_num_steps(6)
        IR.InterpSamplerRef(None, a, s, [None] * 3)._sample_interpolation(UNetRef(TINY).eval(), s.get_timesteps_epoch(0, 1), shift)
        kinds = [k for k, _ in s.rng.log]
        assert kinds == ["randperm"] * want + ["uniform"] * 5, (dep, kinds)
        assert all(tuple(t.shape) == (1, 256) for k, t in s.rng.log if k == "uniform")


# ------------------------------------------------------------------ the ramp of start colours
@pytest.mark.parametrize("shift", [0.3, -0.4, 0.0])
@pytest.mark.parametrize("N", [1, 4, 7])
def test_the_latent_grid_has_its_closed_form(shift, N):
    import mdm
    a = base_args(data_size=4, sample_num=N, out_channel=3)
    lo, hi = IR.latent_grid(shift, N)
    for cls in (mdm.Sampler, IR.InterpSamplerRef):
        latent, grid = cls(None, a, None, [None] * 3)._get_latent_initial_interpolation(shift)
        assert latent.shape == (N, 3, 4, 4) and grid.shape == (N, 1, 1, 1) and latent.dtype == grid.dtype == torch.float32
        assert torch.equal(latent, grid.expand(N, 3, 4, 4))
        assert torch.equal(grid.reshape(N), torch.linspace(lo, hi, N))
        assert float(grid[0]) == np.float32(lo)                          # N = 1: linspace gives the first end
        if N > 1:
            assert abs(float(grid[-1]) - hi) < 1e-6 and np.allclose(np.diff(grid.reshape(N).numpy()), (hi - lo) / (N - 1), atol=1e-6)
            assert float(grid.min() + min(shift, 0)) >= -1 - 1e-6 and float(grid.max() + max(shift, 0)) <= 1 + 1e-6


# ------------------------------------------------------------------ the host predictor of the device row
KEY = (0x9E3779B9 << 32) | 12345


@pytest.mark.parametrize("offset", [1, 2 ** 29 + 3, 2 ** 61 + 5])
@pytest.mark.parametrize("HW", [15, 16, 1028])
def test_the_row_predictor_is_its_scalar_statement_and_none_of_its_twins(offset, HW):
    want = np.empty(HW, dtype=np.float32)
    for p in range(HW):                                                  # one call per pixel, the kernel's rule read literally
        w = philox4x32_10(KEY & 0xFFFFFFFF, np.array([p >> 2], dtype=np.uint64), (offset * 8 + 6) & ((1 << 64) - 1))
        want[p] = u01(w[0, p & 3])
    got = IR.row_uniforms(KEY, offset, HW)
    assert got.dtype == np.float32 and np.array_equal(got, want) and (got >= 0).all() and (got < 1).all()
    assert np.array_equal(got, IR.row_uniforms(12345, offset, HW))       # the rank half of the key does not matter
    twins = dict(lane=IR.row_uniforms(KEY, offset, HW, lane=0), stream4=IR.row_uniforms(KEY, offset, HW, stream=4),
                 stream5=IR.row_uniforms(KEY, offset, HW, stream=5), key=IR.row_uniforms(KEY, offset, HW, mask_key=False))
    for name, t in twins.items():
        assert not np.array_equal(t, want) and (t != want).mean() > 0.5, name
    keep = IR.row_keep(got, [0.0, 0.5, 3.0], 3)
    assert keep.shape == (3, 3, HW) and (keep == keep[:, :1]).all() and not keep[2].any() and keep[0].sum() >= 3 * (HW - 1)
    assert np.array_equal(keep[1, 0], (got > 0.5).astype(np.float32))
