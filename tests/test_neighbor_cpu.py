"""The nearest-neighbour ABI without a GPU (include/mdm_neighbor.h, csrc/neighbor.hip): the fp64 restatement of the tap tables and of a
feature row (tests/_neighbor_ref.py) agrees with torch's CPU `interpolate`; `mdm_nn_plan` equals the restatement's tables and refuses
bad arguments with text; the header parses to exactly its three symbols and they are bound; a numpy fp32 emulation of
`nn_rows_kernel` stays inside the bound that tests/test_neighbor_kernels_gpu.py holds the kernel to, and each planted fault leaves it;
the augment draws are `RandomHorizontalFlip` per batch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _neighbor_ref as NR
from mdm import _lib, evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mdm_neighbor.h")
NAMES = ["mdm_nn_plan", "mdm_nn_rows", "mdm_nn_col_argmax"]
COVERAGE = {"mdm_nn_plan": ("test_neighbor_cpu", "mdm_nn_plan"), "mdm_nn_rows": ("test_neighbor_kernels_gpu", "mdm_nn_rows"),
            "mdm_nn_col_argmax": ("test_neighbor_kernels_gpu", "mdm_nn_col_argmax")}
AXES = sorted({n for _, H, W in NR.SHAPES for n in (H, W)} | {48, 96})


# ------------------------------------------------------------------ the restatement against torch
@pytest.mark.parametrize("antialias", (False, True))
@pytest.mark.parametrize("shape", NR.SHAPES, ids=str)
def test_the_restatement_agrees_with_torchs_interpolate(shape, antialias):
    C, H, W = shape
    x = NR.kernel_images(C, H, W, seed=5)[[0, 2]]
    want = F.interpolate(x, size=(32, 32), mode="bilinear", align_corners=False, antialias=antialias).double().numpy()
    got = NR.resize64(x.numpy(), 32, antialias)
    assert np.abs(got - want).max() <= 4 * 2.0 ** -23 * float(x.abs().max())


def test_a_same_size_table_is_the_identity_bit_for_bit():
    for antialias in (False, True):
        first, count, w = NR.plan(32, 32, antialias)
        A = NR.dense(32, (first, count, w))
        assert np.array_equal(A, np.eye(32)), antialias


# ------------------------------------------------------------------ mdm_nn_plan
@pytest.mark.parametrize("antialias", (0, 1))
@pytest.mark.parametrize("n_in", AXES)
def test_the_c_plan_equals_the_restatements_tables(n_in, antialias):
    first, count, weight, taps = evaluate.nn_plan(n_in, 32, antialias)
    rf, rc, rw = NR.plan(n_in, 32, antialias)
    assert taps == rw.shape[1] == int(rc.max()) and weight.dtype == np.float32
    assert np.array_equal(first, rf) and np.array_equal(count, rc)
    assert (np.abs(weight.astype(np.float64) - rw) <= 2.0 ** -24 * np.abs(rw)).all()          # one fp32 rounding
    assert not weight[np.arange(taps)[None, :] >= count[:, None]].any(), "weights behind the taps are not zero"
    assert _lib.load().mdm_nn_plan(n_in, 32, antialias, None, None, None, 0) == taps


def test_the_c_plan_upsamples_and_downsamples_other_sizes():
    for n_in, n_out in ((4, 32), (7, 5), (1, 3), (300, 7), (5, 5)):
        for antialias in (0, 1):
            first, count, weight, taps = evaluate.nn_plan(n_in, n_out, antialias)
            rf, rc, rw = NR.plan(n_in, n_out, antialias)
            assert np.array_equal(first, rf) and np.array_equal(count, rc) and np.allclose(weight, rw, rtol=2.0 ** -23, atol=0)
            assert (first >= 0).all() and (first + count <= n_in).all() and (count >= 1).all()


@pytest.mark.parametrize("args, word", [((0, 32, 1), "n_in"), ((32, 0, 1), "n_out"), ((-3, 32, 0), "positive")])
def test_the_plan_refuses_bad_sizes(args, word):
    lib = _lib.load()
    assert lib.mdm_nn_plan(*args, None, None, None, 0) == -1
    assert word in lib.mdm_last_error().decode()


def test_the_plan_refuses_partial_outputs_and_a_short_table():
    lib = _lib.load()
    first, count, weight = np.full(32, 77, np.int32), np.full(32, 77, np.int32), np.full((32, 16), 7.0, np.float32)
    assert lib.mdm_nn_plan(256, 32, 1, first.ctypes.data, None, None, 16) == -1 and "together" in lib.mdm_last_error().decode()
    assert lib.mdm_nn_plan(256, 32, 1, first.ctypes.data, count.ctypes.data, weight.ctypes.data, 15) == -1
    assert "max_taps" in lib.mdm_last_error().decode()
    assert (first == 77).all() and (count == 77).all() and (weight == 7.0).all(), "a refused plan wrote"


# ------------------------------------------------------------------ the sixth header and its tables
def test_the_header_parses_to_exactly_the_three_names():
    structs, protos = _lib.parse_header(open(HEADER).read())
    assert structs == {} and list(protos) == NAMES
    assert all(p[0] == "int" for p in protos.values())
    rows = dict(protos["mdm_nn_rows"][1])
    assert (rows["src"], rows["img_stride"], rows["M"], rows["lut"], rows["first"], rows["rows"], rows["row_ld"], rows["eps"]) == \
        ("void*", "int64_t", "int64_t", "float*", "int64_t", "float*", "int64_t", "float")
    assert [n for n, _ in protos["mdm_nn_rows"][1]][-1] == "stream" and [n for n, _ in protos["mdm_nn_col_argmax"][1]][-1] == "stream"
    assert "stream" not in dict(protos["mdm_nn_plan"][1])


def test_every_neighbor_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_nn_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    assert declared == set(_lib.NEIGHBOR_EXPORTS) == set(_lib.NEIGHBOR_PROTOS) == set(_lib.NEIGHBOR_PARAMS) == set(NAMES)
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.NEIGHBOR_PROTOS[name][0] and fn.restype is ctypes.c_int32, name
        assert name in _lib._ALL_PROTOS and name not in _lib._PROTOS
    assert os.path.samefile(_lib.NEIGHBOR_HEADER_PATH, HEADER)
    assert "mdm_nn_" not in open(os.path.join(ROOT, "include", "mdm_hip.h")).read()


def test_every_neighbor_symbol_has_a_test():
    assert set(COVERAGE) == set(_lib.NEIGHBOR_PROTOS)
    for sym, (mod, mention) in COVERAGE.items():
        text = open(os.path.join(ROOT, "tests", mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), (sym, mod)


def test_rows_refusals_name_the_argument():
    """host checks only: nothing is launched, so no device is needed"""
    lib = _lib.load()
    ok = dict(src=16, kind=1, img_stride=3 * 8 * 8, M=4, C=3, H=8, W=8, lut=16, first=0, R=4, normalize=1, flip=0, S=4, hfirst=16,
              hcount=16, hweight=16, htaps=3, vfirst=16, vcount=16, vweight=16, vtaps=3, eps=1e-8, rows=16, row_ld=48, stream=None)
    assert list(ok) == _lib.NEIGHBOR_PARAMS["mdm_nn_rows"]
    bad = [(dict(src=None), "src"), (dict(rows=None), "rows"), (dict(kind=2), "kind"), (dict(lut=None), "lut"), (dict(M=0), "M"),
           (dict(R=0), "R"), (dict(C=0), "C"), (dict(H=0), "H"), (dict(W=-1), "W"), (dict(S=-1), "S"),
           (dict(C=1 << 11, H=1 << 10, W=1 << 10, img_stride=1 << 40), "2^31"), (dict(img_stride=191), "img_stride"),
           (dict(first=-1), "first"), (dict(first=1), "first + R"), (dict(row_ld=47), "row_ld"), (dict(S=0, row_ld=191), "row_ld"),
           (dict(hweight=None), "tables"), (dict(vfirst=None), "tables"), (dict(htaps=0), "htaps"), (dict(S=65, row_ld=1 << 20), "S = 65"),
           (dict(W=4096, img_stride=1 << 20), "W = 4096"), (dict(htaps=600), "horizontal table")]
    for change, word in bad:
        rc = lib.mdm_nn_rows(*{**ok, **change}.values())
        assert rc != 0 and word in lib.mdm_last_error().decode(), (change, lib.mdm_last_error().decode())
    ok2 = dict(S=16, S_aug=None, row_aug=None, M=4, B=4, ld=4, row0=0, carry=0, val=16, idx=16, stream=None)
    assert list(ok2) == _lib.NEIGHBOR_PARAMS["mdm_nn_col_argmax"]
    for change, word in [(dict(S=None), "S is NULL"), (dict(val=None), "val"), (dict(idx=None), "idx"), (dict(M=0), "M"), (dict(B=0), "B"),
                         (dict(ld=3), "ld"), (dict(row0=-1), "row0")]:
        rc = lib.mdm_nn_col_argmax(*{**ok2, **change}.values())
        assert rc != 0 and word in lib.mdm_last_error().decode(), (change, lib.mdm_last_error().decode())


# ------------------------------------------------------------------ the emulation and the bound
EMU_SHAPES = [s for s in NR.SHAPES if s[1] <= 100]           # the 256 x 256 rows run on the GPU; numpy takes seconds for them


def _cases(shape):
    """(image index, normalize, flip, S, antialias) over one shape: every switch on and off, S = 0 once"""
    out = [(i, n, f, 32, aa) for i, (n, f, aa) in enumerate([(1, 0, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1)])]
    return out + [(4, 1, 1, 0, 0)]


@pytest.mark.parametrize("shape", EMU_SHAPES, ids=str)
def test_the_emulation_stays_inside_the_bound(shape):
    C, H, W = shape
    x = NR.kernel_images(C, H, W).numpy()
    plain = [0, 2, 4, 5, 6]
    for i, normalize, flip, S, aa in _cases(shape):
        img = x[plain[i]]
        ref, bound = NR.row_ref(img, normalize, flip, S, aa)
        got = NR.emulate_row(img, normalize, flip, S, aa)
        assert NR.inside(got, ref, bound), (shape, normalize, flip, S, aa, NR.worst(got, ref, bound))
        assert abs(np.linalg.norm(ref) - 1.0) < 1e-12


def test_constant_and_nan_images_are_zero_rows_with_a_zero_bound():
    x = NR.kernel_images(3, 33, 47).numpy()
    for i in (NR.CONSTANT, NR.WITH_NAN):
        for S in (0, 32):
            ref, bound = NR.row_ref(x[i], 1, 0, S, 1)
            got = NR.emulate_row(x[i], 1, 0, S, 1)
            assert not ref.any() and not bound.any() and not got.any() and NR.inside(got, ref, bound)


@pytest.mark.parametrize("fault", NR.FAULTS)
def test_a_planted_fault_leaves_the_bound(fault):
    x = NR.kernel_images(3, 33, 47).numpy()
    big = NR.kernel_images(3, 64, 64).numpy()
    if fault == "nan_kept":
        ref, bound = NR.row_ref(x[NR.CONSTANT], 1, 0, 32, 1)
        assert not NR.inside(NR.emulate_row(x[NR.CONSTANT], 1, 0, 32, 1, fault=fault), ref, bound)
        return
    for img, nb in ((x[2], x[4]), (big[5], big[6])):
        for S in ((32,) if fault in ("drop_last_tap", "edge_unnormalised") else (32, 0)):
            ref, bound = NR.row_ref(img, 1, 1, S, 1)
            assert NR.inside(NR.emulate_row(img, 1, 1, S, 1), ref, bound)
            got = NR.emulate_row(img, 1, 1, S, 1, fault=fault, neighbour=nb)
            assert not NR.inside(got, ref, bound), (fault, img.shape, S)


# ------------------------------------------------------------------ the augment draws
@pytest.mark.parametrize("M, B", [(48, 7), (48, 6), (40, 5), (5, 8)])
def test_the_augment_draws_are_random_horizontal_flip_per_batch(M, B):
    torch.manual_seed(1234 + M + B)
    want = NR.flip_draws(M, B)
    state = torch.get_rng_state()
    torch.manual_seed(1234 + M + B)
    rows = evaluate.neighbor_flip_rows(M, B)
    assert torch.equal(torch.get_rng_state(), state), "the host generator is not where upstream leaves it"
    assert rows.dtype == torch.uint8 and rows.shape == (M,)
    assert rows.tolist() == [int(want[m // B]) for m in range(M)]
    assert len(want) == -(-M // B)
