"""The presentation ABI without a GPU: include/mdm_vis.h parses and is bound next to the core header without entering its tables,
every `mdm_vis_*` symbol has a kernel-level test or launches nothing, the grid geometry of mdm_vis_grid_shape is torchvision's, the
host checks refuse what the header says they refuse, the reference of tests/_vis_ref.py passes a hand-computed case and `save_png`
round-trips a grid.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _vis_ref as VR
from mdm import _lib, visuals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
VIS_HEADER = os.path.join(ROOT, "include", "mdm_vis.h")
HOST = "host only"
_K = "test_vis_kernels_gpu"
COVERAGE = {"mdm_vis_grid_shape": HOST, "mdm_vis_range": (_K, "mdm_vis_range"), "mdm_vis_grid": (_K, "mdm_vis_grid")}


# ------------------------------------------------------------------ the second header and its tables
def test_the_header_parses_and_declares_only_vis_functions():
    structs, protos = _lib.parse_header(open(VIS_HEADER).read())
    assert structs == {} and list(protos) == ["mdm_vis_grid_shape", "mdm_vis_range", "mdm_vis_grid"]
    assert protos["mdm_vis_grid_shape"] == ("int", [(n, "int") for n in ("K", "C", "H", "W", "nrow", "padding")] + [("out", "int32_t*")])
    assert [n for n, _ in protos["mdm_vis_range"][1]] == ["x", "img_stride", "K", "E", "global", "lohi", "scratch", "stream"]
    assert [n for n, _ in protos["mdm_vis_grid"][1]] == ["x", "img_stride", "K", "C", "H", "W", "lohi", "mode", "nrow", "padding", "pad_value",
                                                        "grid_f32", "grid_u8", "stream"]
    assert dict(protos["mdm_vis_grid"][1])["img_stride"] == "int64_t" and dict(protos["mdm_vis_grid"][1])["pad_value"] == "float"


def test_every_vis_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_vis_[a-z0-9_]+)\s*\(", open(VIS_HEADER).read()))
    assert declared == set(_lib.VIS_EXPORTS) == set(_lib.VIS_PROTOS) and len(declared) == 3
    C = ctypes
    for name in _lib.VIS_EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.VIS_PROTOS[name][0] and fn.restype is C.c_int32, name
    assert _lib.VIS_PROTOS["mdm_vis_range"][0] == [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib.VIS_PROTOS["mdm_vis_grid"][0][10] is C.c_float


def test_the_core_tables_are_still_exactly_the_core_header():
    core = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    assert set(_lib.EXPORTS) == set(_lib._PROTOS) == set(re.findall(r"\b(mdm_[a-z0-9_]+)\s*\(", core))
    assert not [n for n in list(_lib.EXPORTS) + list(_lib._PARAMS) if n.startswith("mdm_vis_")]
    assert "mdm_vis" not in core and not set(_lib.VIS_EXPORTS) & set(_lib.EXPORTS)


def test_call_binds_vis_keywords_against_the_vis_header():
    """`_lib.call` and `Recording` serve both tables: a keyword call of a vis entry point records the positional tuple, a misspelt
    keyword is a TypeError that names it and records nothing"""
    with _lib.Recording() as rec:
        _lib.call("mdm_vis_grid", x=1, img_stride=2, K=3, C=4, H=5, W=6, lohi=None, mode=0, nrow=7, padding=8, pad_value=0.5, grid_f32=9,
                  grid_u8=None, stream=None)
        with pytest.raises(TypeError, match="mdm_vis_grid"):
            _lib.call("mdm_vis_grid", x=1, stride=2)
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_vis_grid", (1, 2, 3, 4, 5, 6, None, 0, 7, 8, 0.5, 9, None))]


def test_every_vis_symbol_has_a_kernel_test_or_is_host_only():
    """as tests/test_abi_coverage_cpu.py does for the core header"""
    assert set(COVERAGE) == set(_lib.VIS_PROTOS)
    for sym, where in COVERAGE.items():
        if where == HOST:
            continue
        mod, mention = where
        text = open(os.path.join(TESTS, mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), f"{mod}.py does not mention {mention}"
        assert "pytest.mark.gpu" in text


# ------------------------------------------------------------------ geometry
SHAPE_ROWS = [(K, nrow, p) for K, nrow in VR.GRID_KN + [(100, 10), (3, 1000)] for p in (0, 2, 3)]


@pytest.mark.parametrize("K,nrow,padding", SHAPE_ROWS)
def test_grid_shape_is_make_grids(K, nrow, padding):
    for C, H, W in VR.GRID_SHAPES:
        want = tuple(VR.make_grid_ref(torch.zeros(K, C, H, W), nrow, padding).shape)
        assert visuals.grid_shape(K, C, H, W, nrow, padding) == want == VR.grid_shape_ref(K, C, H, W, nrow, padding)
        out = (ctypes.c_int32 * 3)()
        assert _lib.load().mdm_vis_grid_shape(K, C, H, W, nrow, padding, out) == 0 and tuple(out) == want


def test_the_reference_grid_passes_a_hand_computed_case():
    """two 1 x 2 x 2 images, padding 1, pad value 9, written out by hand: side by side (nrow 2) and stacked (nrow 1)"""
    x = torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]], [[[5.0, 6.0], [7.0, 8.0]]]])
    side = torch.tensor([[9, 9, 9, 9, 9, 9, 9],
                         [9, 1, 2, 9, 5, 6, 9],
                         [9, 3, 4, 9, 7, 8, 9],
                         [9, 9, 9, 9, 9, 9, 9]], dtype=torch.float32)
    stacked = torch.tensor([[9, 9, 9, 9],
                            [9, 1, 2, 9],
                            [9, 3, 4, 9],
                            [9, 9, 9, 9],
                            [9, 5, 6, 9],
                            [9, 7, 8, 9],
                            [9, 9, 9, 9]], dtype=torch.float32)
    for nrow, plane in ((2, side), (8, side), (1, stacked)):
        g = VR.make_grid_ref(x, nrow, padding=1, pad_value=9.0)
        assert g.shape == (3,) + plane.shape and all(torch.equal(g[c], plane) for c in range(3)), nrow
    three = VR.make_grid_ref(torch.arange(3 * 2 * 1 * 2, dtype=torch.float32).reshape(3, 2, 1, 2), 2, padding=1, pad_value=-1.0)
    want = torch.tensor([[[-1, -1, -1, -1, -1, -1, -1], [-1, 0, 1, -1, 4, 5, -1], [-1, -1, -1, -1, -1, -1, -1], [-1, 8, 9, -1, -1, -1, -1],
                          [-1, -1, -1, -1, -1, -1, -1]],
                         [[-1, -1, -1, -1, -1, -1, -1], [-1, 2, 3, -1, 6, 7, -1], [-1, -1, -1, -1, -1, -1, -1], [-1, 10, 11, -1, -1, -1, -1],
                          [-1, -1, -1, -1, -1, -1, -1]]], dtype=torch.float32)
    assert torch.equal(three, want)                                  # two channels stay two; the unfilled cell is pad_value
    one = VR.make_grid_ref(x[:1], 5, padding=3, pad_value=9.0)
    assert one.shape == (3, 2, 2) and torch.equal(one[2], x[0, 0])   # a single image: no border, the channel three times


def test_the_reference_quantisation_is_save_images():
    """against torch's own sequence where torch defines it; k + 0.5 rounds up exactly at the edge; NaN is 0 by mdm_vis.h"""
    v = VR.quant_edges()
    fin = ~torch.isnan(v)
    want = v[fin].mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    got = VR.to_u8_ref(v[None, None, :])[0, :, 0]
    assert torch.equal(got[fin], want) and int(got[~fin].max()) == 0
    assert VR.to_u8_ref(torch.tensor([[[0.0, 1.0, 0.5, 2.0, -3.0]]]))[0, :, 0].tolist() == [0, 255, 128, 255, 0]


# ------------------------------------------------------------------ refusals (host checks: nothing is launched, no device is needed)
def _refused(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    text = lib.mdm_last_error().decode()
    return rc != 0 and text.startswith(name[4:]), text


def test_refusals_say_why():
    P, Q, R = 0x10000, 0x20000, 0x30000                              # never dereferenced: every row fails a host check first
    out = (ctypes.c_int32 * 3)()
    shape_ok = dict(K=4, C=3, H=8, W=8, nrow=2, padding=2)
    for k, v in (("K", 0), ("C", 0), ("H", -1), ("W", 0), ("nrow", 0), ("padding", -1)):
        a = dict(shape_ok, **{k: v})
        ok, text = _refused("mdm_vis_grid_shape", *a.values(), out)
        assert ok, (k, v, text)
        ok, text = _refused("mdm_vis_grid", P, 192, a["K"], a["C"], a["H"], a["W"], Q, 1, a["nrow"], a["padding"], 0.0, R, None, None)
        assert ok, (k, v, text)
    assert _refused("mdm_vis_grid_shape", *shape_ok.values(), None)[0]
    assert _refused("mdm_vis_grid_shape", 2 ** 31 - 1, 1, 2 ** 30, 1, 1, 0, out)[0]           # Hg past 2^31 - 1
    for args in ((None, 192, 4, 3, 8, 8, Q, 1, 2, 2, 0.0, R, None),        # x NULL
                 (P, 191, 4, 3, 8, 8, Q, 1, 2, 2, 0.0, R, None),           # img_stride < C H W
                 (P, 192, 4, 3, 8, 8, Q, 1, 2, 2, 0.0, None, None),        # both outputs NULL
                 (P, 192, 4, 3, 8, 8, Q, 3, 2, 2, 0.0, R, None),           # mode 3
                 (P, 192, 4, 3, 8, 8, Q, -1, 2, 2, 0.0, R, None),
                 (P, 192, 4, 3, 8, 8, None, 1, 2, 2, 0.0, R, None),        # mode 1 without lohi
                 (P, 192, 4, 3, 8, 8, None, 2, 2, 2, 0.0, None, R)):
        ok, text = _refused("mdm_vis_grid", *args, None)
        assert ok, (args, text)
    for args in ((None, 8, 2, 8, 0, Q, None), (P, 8, 2, 8, 0, None, None), (P, 8, 0, 8, 0, Q, None), (P, 8, 2, 0, 0, Q, None),
                 (P, 7, 2, 8, 0, Q, None),                                 # img_stride < E
                 (P, 8, 2, 8, 1, Q, None),                                 # a global range without scratch
                 (P, 8, 2, 8, 1, Q, R + 4)):                               # ... or with scratch that is not 16-byte aligned
        ok, text = _refused("mdm_vis_range", *args, None)
        assert ok, (args, text)


# ------------------------------------------------------------------ PNG
def test_save_png_round_trips_bit_for_bit(tmp_path):
    from PIL import Image
    g = torch.Generator().manual_seed(5)
    for shape in ((38, 56, 3), (1, 1, 3), (7, 5, 3)):
        u8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        path = tmp_path / f"g{shape[0]}.png"
        visuals.save_png(u8, str(path))
        back = np.asarray(Image.open(path))
        assert back.dtype == np.uint8 and back.shape == shape and np.array_equal(back, u8.numpy())
    with pytest.raises(ValueError):
        visuals.save_png(torch.zeros(4, 4, dtype=torch.uint8), str(tmp_path / "bad.png"))


def test_make_grid_refuses_what_it_cannot_read():
    """host-side argument checks of the Python layer: they raise before anything is launched"""
    with pytest.raises(TypeError):
        visuals.make_grid(torch.zeros(2, 3, 4, 4), 2)                                # not on the device
    with pytest.raises(ValueError):
        visuals.make_grid(torch.zeros(3, 4, 4), 2)
    with pytest.raises(ValueError):
        visuals.make_grid(torch.zeros(2, 3, 4, 4), 2, normalization="batch")
