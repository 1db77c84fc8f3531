"""The ingest ABI and its host layer without a GPU: the numpy restatement (tests/_ingest_ref.py) equals the PIL-made fixture
(tests/golden/ingest.npz) and the installed PIL; `mdm_ingest_plan` equals the restatement's tables; include/mdm_ingest.h parses to
its three functions and is bound without entering the four older tables; the host checks refuse what the header says they refuse;
`resize_crop_plan`, `image_folder` and `get_dataset` follow torchvision and upstream; `mdm_ingest_launch_of` (the launcher's own
geometry, asked without a device) says that the cases of `_ingest_ref.GEOMETRY_CASES` reach the kernel instantiation, the row tile
and the loop trips they are there for, and refuses where and as the launcher does.  No kernel is launched."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

import _ingest_ref as R
from mdm import _lib
from mdm import ingest as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
INGEST_HEADER = os.path.join(ROOT, "include", "mdm_ingest.h")
PLAN_PARAMS = ["in_size", "out_size", "first", "count", "bounds", "coeffs"]
RESIZE_PARAMS = ["src", "src_stride", "K", "h", "w", "C", "hbounds", "hcoeffs", "ksh", "vbounds", "vcoeffs", "ksv", "dst", "dst_stride",
                 "M", "first", "S", "stream"]
LAUNCH_OF_PARAMS = ["w", "C", "S", "ksh", "out"]
COVERAGE = {"mdm_ingest_plan": ("test_ingest_cpu", "mdm_ingest_plan"), "mdm_ingest_resize_crop": ("test_ingest_gpu", "mdm_ingest_resize_crop"),
            "mdm_ingest_launch_of": ("test_ingest_cpu", "mdm_ingest_launch_of")}


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("ingest")


# ------------------------------------------------------------------ the restatement, the fixture and the installed PIL
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_restatement_equals_the_fixture_and_live_pil(fixture, name):
    h, w, C, size, fill = R.CASES[name]
    src = R.case_source(name)
    assert src.shape == (h, w, C) and int(fixture[name + "/crc"]) == zlib.crc32(src.tobytes())
    if name + "/src" in fixture.files:
        assert np.array_equal(fixture[name + "/src"], src)
    got = R.resize_crop(src, size)
    assert got.shape == (C, size, size) and got.dtype == np.uint8
    assert int((got != fixture[name + "/out"]).sum()) == 0
    assert int((got != R.pil_resize_crop(src, size)).sum()) == 0
    if fill is not None:
        assert (got == fill).all()


def test_the_cases_reach_what_they_are_there_for():
    for name, want in R.EXPECTED_PLANS.items():
        h, w, _, size, _ = R.CASES[name]
        assert R.resize_crop_plan(h, w, size) == want, name
    taps = {name: (R.plan(R.CASES[name][1], R.CASES[name][3])[0], R.plan(R.CASES[name][0], R.CASES[name][3])[0])
            for name in ("taps37_140x131", "taps261_1040x1031")}
    assert taps["taps37_140x131"][0] == 35 and taps["taps37_140x131"][1] == 37
    assert taps["taps261_1040x1031"][0] == 259 and taps["taps261_1040x1031"][1] == 261 > 64
    ks, b, c = R.plan(16, 16)
    assert ks == 3 and all(c[n, 0] == 1 << 22 and (c[n, 1:] == 0).all() and b[n, 0] == n for n in range(16))    # identity


# ------------------------------------------------------------------ mdm_ingest_plan
def _c_plan(in_size, out_size, first, count):
    lib = _lib.load()
    ks = lib.mdm_ingest_plan(in_size, out_size, first, count, None, None)
    bounds, coeffs = np.full((count, 2), -1, dtype=np.int32), np.full((count, ks), -1, dtype=np.int32)
    assert lib.mdm_ingest_plan(in_size, out_size, first, count, bounds.ctypes.data, coeffs.ctypes.data) == ks
    return ks, bounds, coeffs


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_c_plan_equals_the_restatements_tables(name):
    h, w, _, size, _ = R.CASES[name]
    ow, oh, top, left = R.resize_crop_plan(h, w, size)
    for in_size, out_size, first in ((w, ow, left), (h, oh, top)):
        ks, bounds, coeffs = _c_plan(in_size, out_size, first, size)
        rks, rb, rc = R.plan(in_size, out_size, first, size)
        assert ks == rks and np.array_equal(bounds, rb) and np.array_equal(coeffs, rc), (name, in_size, out_size)
        hks, hb, hc = I.axis_plan(in_size, out_size, first, size)
        assert hks == ks and np.array_equal(hb, rb) and np.array_equal(hc, rc)
        assert (coeffs.sum(axis=1) - (1 << 22)).__abs__().max() <= ks           # normalised rows, one rounding per tap


def test_the_c_plan_over_a_sweep_of_sizes():
    for in_size in range(1, 200, 9):
        for out_size in (1, 5, 8, 33, 64, 150):
            ks, bounds, coeffs = _c_plan(in_size, out_size, 0, out_size)
            rks, rb, rc = R.plan(in_size, out_size)
            assert ks == rks and np.array_equal(bounds, rb) and np.array_equal(coeffs, rc), (in_size, out_size)
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= in_size).all() and (bounds[:, 1] <= ks).all()


@pytest.mark.parametrize("args,word", [((0, 8, 0, 8), "in_size"), ((8, 0, 0, 1), "out_size"), ((8, 8, 0, 0), "count"), ((8, 8, -1, 2), "first"),
                                       ((8, 8, 4, 5), "out_size")])
def test_the_plan_refuses(args, word):
    lib = _lib.load()
    assert lib.mdm_ingest_plan(*args, None, None) == -1
    text = lib.mdm_last_error().decode()
    assert text.startswith("ingest_plan:") and word in text
    b = np.zeros((8, 2), dtype=np.int32)
    assert lib.mdm_ingest_plan(8, 8, 0, 8, b.ctypes.data, None) == -1 and "coeffs" in lib.mdm_last_error().decode()


# ------------------------------------------------------------------ the fifth header and the five tables
def test_the_header_parses_to_exactly_the_two_names():
    structs, protos = _lib.parse_header(open(INGEST_HEADER).read())
    assert structs == {} and list(protos) == ["mdm_ingest_plan", "mdm_ingest_resize_crop", "mdm_ingest_launch_of"]
    assert [n for n, _ in protos["mdm_ingest_launch_of"][1]] == LAUNCH_OF_PARAMS and dict(protos["mdm_ingest_launch_of"][1])["out"] == "int32_t*"
    assert [n for n, _ in protos["mdm_ingest_plan"][1]] == PLAN_PARAMS
    assert [n for n, _ in protos["mdm_ingest_resize_crop"][1]] == RESIZE_PARAMS
    r = dict(protos["mdm_ingest_resize_crop"][1])
    assert (r["src"], r["src_stride"], r["hbounds"], r["dst"], r["M"], r["first"], r["S"]) == \
        ("uint8_t*", "int64_t", "int32_t*", "uint8_t*", "int64_t", "int64_t", "int")
    assert all(p[0] == "int" for p in protos.values())


def test_every_ingest_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_ingest_[a-z0-9_]+)\s*\(", open(INGEST_HEADER).read()))
    assert declared == set(_lib.INGEST_EXPORTS) == set(_lib.INGEST_PROTOS) == set(_lib.INGEST_PARAMS) and len(declared) == 3
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    for name in _lib.INGEST_EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.INGEST_PROTOS[name][0] and fn.restype is i32, name
    assert _lib.INGEST_PROTOS["mdm_ingest_plan"][0] == [i32, i32, i32, i32, vp, vp]
    assert _lib.INGEST_PROTOS["mdm_ingest_resize_crop"][0] == [vp, i64, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, i64, i64, i64, i32, vp]
    assert _lib.INGEST_PROTOS["mdm_ingest_launch_of"][0] == [i32, i32, i32, i32, vp]
    assert os.path.samefile(_lib.INGEST_HEADER_PATH, INGEST_HEADER)


def test_the_four_older_tables_are_unchanged():
    text = {n: open(os.path.join(ROOT, "include", n)).read() for n in ("mdm_hip.h", "mdm_vis.h", "mdm_data.h", "mdm_interp.h")}
    rows = [("mdm_hip.h", r"mdm_", _lib.EXPORTS, _lib._PROTOS, _lib._PARAMS, 92), ("mdm_vis.h", r"mdm_vis_", _lib.VIS_EXPORTS, _lib.VIS_PROTOS, _lib.VIS_PARAMS, 3),
            ("mdm_data.h", r"mdm_data_", _lib.DATA_EXPORTS, _lib.DATA_PROTOS, _lib.DATA_PARAMS, 2),
            ("mdm_interp.h", r"mdm_interp_", _lib.INTERP_EXPORTS, _lib.INTERP_PROTOS, _lib.INTERP_PARAMS, 3)]
    for header, prefix, exports, protos, params, count in rows:
        declared = re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text[header])
        assert set(exports) == set(protos) == set(params) == set(declared) and len(exports) == count, header
        assert not [n for n in exports if n.startswith("mdm_ingest_")] and "mdm_ingest" not in text[header], header


def test_call_and_recording_serve_the_ingest_table():
    kw = dict(zip(RESIZE_PARAMS, range(1, len(RESIZE_PARAMS) + 1)), stream=None)
    with _lib.Recording() as rec:
        _lib.call("mdm_ingest_resize_crop", **kw)
        with pytest.raises(TypeError, match="mdm_ingest_resize_crop"):
            _lib.call("mdm_ingest_resize_crop", src=1, stride=2)
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_ingest_resize_crop", tuple(range(1, len(RESIZE_PARAMS))))]


def test_every_ingest_symbol_has_a_test():
    assert set(COVERAGE) == set(_lib.INGEST_PROTOS)
    for sym, (mod, mention) in COVERAGE.items():
        text = open(os.path.join(TESTS, mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), f"{mod}.py does not mention {mention}"
    assert "pytest.mark.gpu" in open(os.path.join(TESTS, "test_ingest_gpu.py")).read()


# ------------------------------------------------------------------ refusals (host checks: nothing is launched, no device is needed)
P = [0x10000 * k for k in range(1, 8)]                                  # never dereferenced: every row fails a host check first
RESIZE_OK = dict(src=P[0], src_stride=37 * 53 * 3, K=2, h=37, w=53, C=3, hbounds=P[1], hcoeffs=P[2], ksh=11, vbounds=P[3], vcoeffs=P[4],
                 ksv=11, dst=P[5], dst_stride=192, M=4, first=1, S=8, stream=None)
RESIZE_REFUSALS = [("src", dict(src=None)), ("hbounds", dict(hbounds=None)), ("hcoeffs", dict(hcoeffs=None)), ("vbounds", dict(vbounds=None)),
                   ("vcoeffs", dict(vcoeffs=None)), ("dst", dict(dst=None)), ("C", dict(C=2)), ("C", dict(C=4)), ("C", dict(C=0)),
                   ("K", dict(K=0)), ("K", dict(K=-1)), ("h", dict(h=0)), ("w", dict(w=-3)), ("S", dict(S=0)), ("M", dict(M=0)),
                   ("ksh", dict(ksh=0)), ("ksv", dict(ksv=-1)), ("src_stride", dict(src_stride=37 * 53 * 3 - 1)),
                   ("dst_stride", dict(dst_stride=191)), ("first", dict(first=-1)), ("first", dict(first=3)), ("first", dict(first=4)),
                   ("h w C", dict(h=30000, w=30000, src_stride=2 ** 40)), ("C S S", dict(S=30000, dst_stride=2 ** 40)),
                   ("LDS", dict(w=20000, src_stride=2 ** 40))]


def test_refusals_name_the_argument():
    lib = _lib.load()
    assert list(RESIZE_OK) == _lib.INGEST_PARAMS["mdm_ingest_resize_crop"]
    for arg, change in RESIZE_REFUSALS:
        rc = lib.mdm_ingest_resize_crop(*dict(RESIZE_OK, **change).values())
        text = lib.mdm_last_error().decode()
        assert rc != 0 and text.startswith("ingest_resize_crop:") and re.search(r"(?<![\w])" + re.escape(arg) + r"(?![\w])", text), (change, text)


# ------------------------------------------------------------------ the launch geometries: GEOMETRY_CASES and mdm_ingest_launch_of
NJ_PAST_256 = ("preset128", "preset256", "grey264", "table_global_830", "tr7_33x40", "wide_12x9000")
NARROW = ("narrow_40x3_L", "narrow_9x5")
GEOMETRY_PLANS = {"preset128": (128, 146, 9, 0), "grey264": (282, 264, 0, 9), "tr7_33x40": (848, 700, 0, 74), "one_1x1": (4, 4, 0, 0)}
SHORT_LAST_TILE = {"table_global_830": 4, "wide_12x9000": 1}        # rows of the last tile where it is not a whole one


def _ksh(h, w, size):
    ow, _, _, left = R.resize_crop_plan(h, w, size)
    return _lib.load().mdm_ingest_plan(w, ow, left, size, None, None)


def _launch_of(w, C, S, ksh):
    """mdm_ingest_launch_of -> (TR, table in LDS, LDS bytes, workgroups per image), or the refusal's text"""
    lib = _lib.load()
    out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    if lib.mdm_ingest_launch_of(w, C, S, ksh, out) != 0:
        assert list(out) == [-1] * 4                                   # a refused query writes nothing
        return lib.mdm_last_error().decode()
    assert I.launch_of(w, C, S, ksh) == (out[0], bool(out[1]), out[2], out[3])
    return out[0], bool(out[1]), out[2], out[3]


@pytest.mark.parametrize("name", list(R.GEOMETRY_CASES))
def test_the_restatement_equals_live_pil_on_the_geometry_cases(name):
    h, w, C, size, _ = R.GEOMETRY_CASES[name]
    assert R.pil_allowed(h, w, C, size) == (name != "wide_12x9000")    # the one case PIL is not asked for
    assert not set(R.GEOMETRY_CASES) & set(R.CASES)
    src, out, pil = R.geometry_reference(name)
    assert src.shape == (h, w, C) and out.shape == (C, size, size) and out.dtype == np.uint8
    if pil is not None:
        assert int((out != pil).sum()) == 0
    if name == "one_1x1":
        assert all((out[c] == src[0, 0, c]).all() for c in range(C))


@pytest.mark.parametrize("name", list(R.GEOMETRY_CASES))
def test_the_c_plan_equals_the_restatements_tables_on_the_geometry_cases(name):
    h, w, _, size, _ = R.GEOMETRY_CASES[name]
    ow, oh, top, left = R.resize_crop_plan(h, w, size)
    for in_size, out_size, first in ((w, ow, left), (h, oh, top)):
        ks, bounds, coeffs = _c_plan(in_size, out_size, first, size)
        rks, rb, rc = R.plan(in_size, out_size, first, size)
        assert ks == rks and np.array_equal(bounds, rb) and np.array_equal(coeffs, rc), (name, in_size, out_size)
        hks, hb, hc = I.axis_plan(in_size, out_size, first, size)
        assert hks == ks and np.array_equal(hb, rb) and np.array_equal(hc, rc)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= in_size).all() and (bounds[:, 1] <= ks).all()


def test_the_geometry_cases_reach_what_they_are_there_for():
    """asked of the launcher's own geometry function, not restated: the row tile, where the table lies and the tiles of every case"""
    assert set(R.GEOMETRY_EXPECTED) == set(R.GEOMETRY_CASES)
    seen = []
    for name, (h, w, C, size, _) in R.GEOMETRY_CASES.items():
        tr, in_lds, lds, tiles = _launch_of(w, C, size, _ksh(h, w, size))
        assert (tr, in_lds, tiles) == R.GEOMETRY_EXPECTED[name] and tiles == -(-size // tr) and lds <= 65536, (name, tr, in_lds, lds, tiles)
        last = size - (tiles - 1) * tr
        assert last == SHORT_LAST_TILE.get(name, tr), (name, last)
        assert (size * C > 256) == (name in NJ_PAST_256), name
        assert (w * C < 16) == (name in NARROW or name == "one_1x1"), name
        seen.append((tr, in_lds, last < tr, size * C > 256, w * C < 16))
    for name, want in GEOMETRY_PLANS.items():
        h, w, _, size, _ = R.GEOMETRY_CASES[name]
        assert R.resize_crop_plan(h, w, size) == want, name
    assert _launch_of(10880, 3, 16, 3)[:3] == (1, False, 65512)         # edge_8x10880: 24 bytes below the limit
    # what the cases of CASES reach: one geometry
    for name, (h, w, C, size, _) in R.CASES.items():
        tr, in_lds, lds, tiles = _launch_of(w, C, size, _ksh(h, w, size))
        assert tr == min(size, 8) and in_lds and size * C <= 192 and w * C >= 16, name
        seen.append((tr, in_lds, size - (tiles - 1) * tr < tr, False, False))
    # between them: both instantiations, the shrunk tiles, a short last tile, NJ and the row on both sides of 256 and of 16 bytes
    assert {s[1] for s in seen} == {True, False} and {s[0] for s in seen} >= {1, 3, 7, 8}
    assert any(s[2] for s in seen) and {s[3] for s in seen} == {True, False} and {s[4] for s in seen} == {True, False}


def test_the_launch_query_fits_lds_and_is_monotone_in_the_table():
    for C in (1, 3):
        for w in (1, 5, 53, 1031, 4000, 9000, 10880 * 3 // C):
            for S in (1, 7, 8, 64, 128, 256, 700, 1024):
                got = [_launch_of(w, C, S, ksh) for ksh in (1, 3, 5, 40, 261, 4001)]
                if isinstance(got[0], str):
                    assert all(g == got[0] for g in got), (w, C, S)        # the table has no part in a refusal
                    continue
                for tr, in_lds, lds, tiles in got:
                    assert 1 <= tr <= min(S, 8) and tiles == -(-S // tr) and 0 < lds <= 65536, (w, C, S)
                    assert (tr, tiles) == got[0][::3]                       # nor in the row tile
                flags = [g[1] for g in got]
                assert flags == sorted(flags, reverse=True), (w, C, S, flags)   # a larger ksh never moves the table into LDS
                assert all(a[2] > b[2] for a, b in zip(got, got[1:]) if a[1] and not b[1])
                assert len({g[2] for g in got if not g[1]}) <= 1             # out of LDS, the table costs nothing
    assert _launch_of(10880, 3, 16, 3) == (1, False, 65512, 16)
    for w in (10881, 10886):
        text = _launch_of(w, 3, 16, 3)
        assert isinstance(text, str) and text.startswith("ingest_resize_crop:") and "LDS" in text and str(3 * w) in text, text


LAUNCH_OF_OK = dict(w=53, C=3, S=8, ksh=11)
LAUNCH_OF_REFUSALS = [("C", dict(C=2)), ("C", dict(C=0)), ("w", dict(w=0)), ("w", dict(w=-3)), ("S", dict(S=0)), ("ksh", dict(ksh=0)),
                      ("LDS", dict(w=20000)), ("LDS", dict(S=30000))]


def test_the_launch_query_refusals_name_the_argument():
    lib = _lib.load()
    assert list(LAUNCH_OF_OK) + ["out"] == _lib.INGEST_PARAMS["mdm_ingest_launch_of"] == LAUNCH_OF_PARAMS
    assert _launch_of(**LAUNCH_OF_OK) == (8, True, 1600, 1)
    for arg, change in LAUNCH_OF_REFUSALS:
        text = _launch_of(**dict(LAUNCH_OF_OK, **change))
        assert isinstance(text, str) and re.match(r"ingest_(launch_of|resize_crop):", text) and \
            re.search(r"(?<![\w])" + re.escape(arg) + r"(?![\w])", text), (change, text)
    assert lib.mdm_ingest_launch_of(*LAUNCH_OF_OK.values(), None) != 0 and "out" in lib.mdm_last_error().decode()


def test_the_launcher_and_the_query_refuse_alike():
    """the launcher with the never-dereferenced pointers of RESIZE_OK at geometries the query refuses: the same words"""
    lib = _lib.load()
    for change in (dict(w=10881, S=16, ksh=3), dict(w=10886, S=16, ksh=3), dict(w=20000), dict(w=32641, C=1, S=64), dict(S=6000)):
        kw = dict(RESIZE_OK, src_stride=2 ** 40, dst_stride=2 ** 40, **change)
        said = _launch_of(kw["w"], kw["C"], kw["S"], kw["ksh"])
        assert isinstance(said, str), change
        assert lib.mdm_ingest_resize_crop(*kw.values()) != 0
        assert lib.mdm_last_error().decode() == said, change


# ------------------------------------------------------------------ torchvision's sizes
def test_resize_crop_plan_gives_torchvisions_tuples():
    for name, want in R.EXPECTED_PLANS.items():
        h, w, _, size, _ = R.CASES[name]
        assert I.resize_crop_plan(h, w, size) == want, name
    assert I.resize_crop_plan(1024, 1024, 64) == (64, 64, 0, 0)
    assert I.resize_crop_plan(40, 17, 64) == (64, 150, 43, 0)              # the transposed case crops the other way
    assert I.resize_crop_plan(16, 18, 8) == (9, 8, 0, 0) and I.resize_crop_plan(16, 22, 8) == (11, 8, 0, 2)
    for h in range(1, 40):
        for w in range(1, 40):
            assert I.resize_crop_plan(h, w, 8) == R.resize_crop_plan(h, w, 8)
    with pytest.raises(ValueError):
        I.resize_crop_plan(0, 4, 8)
    import mdm
    assert mdm.resize_crop_plan is I.resize_crop_plan and mdm.get_dataset is I.get_dataset and mdm.image_folder is I.image_folder


# ------------------------------------------------------------------ ImageFolder
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_image_folder_orders_filters_and_follows_links(tmp_path):
    root = tmp_path / "set"
    for rel in ("b/2.png", "b/10.png", "b/sub/0.JPG", "a/z.jpeg", "a/y.TIFF", "a/notes.txt", "a/x.webp.bak", "c/deep/er/1.bmp",
                "c/0.ppm", "c/0.pgm", "c/k.tif", "c/k.gif"):
        _touch(str(root / rel))
    _touch(str(root / "top_level.png"))                                      # a file next to the classes is no class and no sample
    outside = tmp_path / "elsewhere"
    _touch(str(outside / "linked.png"))
    os.symlink(str(outside), str(root / "a" / "link"))                        # a linked directory is walked
    classes, class_to_idx, samples = I.image_folder(str(root))
    assert classes == ["a", "b", "c"] and class_to_idx == {"a": 0, "b": 1, "c": 2}
    rel = [(os.path.relpath(p, str(root)), l) for p, l in samples]
    assert rel == [("a/y.TIFF", 0), ("a/z.jpeg", 0), ("a/link/linked.png", 0),
                   ("b/10.png", 1), ("b/2.png", 1), ("b/sub/0.JPG", 1),
                   ("c/0.pgm", 2), ("c/0.ppm", 2), ("c/k.tif", 2), ("c/deep/er/1.bmp", 2)]
    os.makedirs(str(root / "d"))
    _touch(str(root / "d" / "readme.md"))
    with pytest.raises(FileNotFoundError, match="d"):
        I.image_folder(str(root))
    os.makedirs(str(tmp_path / "none"))
    with pytest.raises(FileNotFoundError):
        I.image_folder(str(tmp_path / "none"))


# ------------------------------------------------------------------ get_dataset: names, splits, errors
def test_get_dataset_names_splits_and_errors(tmp_path):
    p = str(tmp_path)
    assert I.folder_roots(p, "celeba_hq", "train") == [os.path.join(p, "celeba_hq", "train")]
    assert I.folder_roots(p, "CelebA_HQ", "all") == [os.path.join(p, "celeba_hq", "train"), os.path.join(p, "celeba_hq", "val")]
    assert I.folder_roots(p, "afhqv2", "all") == [os.path.join(p, "afhqv2", "train"), os.path.join(p, "afhqv2", "test")]
    assert I.folder_roots(p, "afhqv2", "test") == [os.path.join(p, "afhqv2", "test")]
    for name in ("metfaces", "stanfordcars"):
        assert I.folder_roots(p, name, "all") == I.folder_roots(p, name, "train") == [os.path.join(p, name)]
    for name in ("mnist", "CIFAR10", "flowers102", "lsun"):
        with pytest.raises(ValueError, match="download"):
            I.get_dataset(p, name, 32, "train")
    with pytest.raises(ValueError, match="unknown"):
        I.get_dataset(p, "imagenet", 32, "train")
    for name, split in (("celeba_hq", "test"), ("afhqv2", "val"), ("metfaces", "val")):
        with pytest.raises(ValueError, match="splits"):
            I.get_dataset(p, name, 32, split)
    with pytest.raises(FileNotFoundError):
        I.get_dataset(p, "metfaces", 32, "all")                              # the folder is not there
    for rel in ("afhqv2/train/cat/a.png", "afhqv2/train/dog/a.png", "afhqv2/train/wild/a.png", "afhqv2/test/cat/b.png",
                "afhqv2/test/dog/b.png", "afhqv2/test/wild/b.png"):
        _touch(os.path.join(p, rel))
    with pytest.raises(ValueError, match="num_data"):
        I.get_dataset(p, "afhqv2", 32, "all", True, 7)
    if not torch.cuda.is_available():
        state = torch.get_rng_state()
        with pytest.raises(TypeError, match="GPU"):                          # found, listed -- and nothing resizes off the GPU
            I.get_dataset(p, "afhqv2", 32, "all", True, 4)
        assert torch.equal(torch.get_rng_state(), state)                     # refused before anything is drawn
        with pytest.raises(TypeError, match="GPU"):
            I.ingest_arrays([np.zeros((4, 4, 3), dtype=np.uint8)], 2, device="cpu")


def test_the_decode_pool_is_sized_by_the_affinity_mask():
    assert 1 <= I.decode_threads() <= min(16, len(os.sched_getaffinity(0)))
    src = open(I.__file__).read()
    assert "cpu_count" not in src
