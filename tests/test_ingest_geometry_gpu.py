"""Every launch geometry of `mdm_ingest_resize_crop` (include/mdm_ingest.h, csrc/ingest.hip) on the device, through the C ABI.
tests/test_ingest_gpu.py runs the kernel at S <= 64, where the launcher always picks one shape: a row tile of min(S, 8) rows, the
horizontal table in LDS, at most 192 (channel, column) pairs for the 256 lanes.  The cases of `_ingest_ref.GEOMETRY_CASES` reach the
rest -- the instantiation that reads the table from global memory, the row tiles 7, 3 and 1, the second and later trips of the lane
loops at the 128- and 256-pixel presets, rows shorter than 16 bytes, the widest row that still fits -- and tests/test_ingest_cpu.py
proves through `mdm_ingest_launch_of` that they do.  The contract is PIL's bytes: 0 differing bytes against the numpy restatement
(tests/_ingest_ref.py) and, wherever PIL can build the resized image, against the installed PIL.

Every operand sits inside guard bands (`_guard_bufs`): the source and the four tables must come back bit for bit, the destination
starts as a sentinel, its guards and every byte the header does not name must still hold it, and a second launch into a second
buffer with the same prefill must give the same bytes.  No table here is out of range: nothing is made to fault."""
import os

import numpy as np
import pytest
import torch

import _ingest_ref as R
from _guard_bufs import ByteBuf, Int32Buf
from mdm import _lib
from mdm import data as D
from mdm import ingest as I

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, SRC_GAP = 0xAB, 0x5C


def _plans(h, w, size, pitch=None):
    """host tables of mdm_ingest_plan for an h x w source at `size` -> (ksh, hbounds, hcoeffs, ksv, vbounds, vcoeffs); `pitch`
    re-lays both coefficient tables at that many words per row, zeros behind the real taps"""
    ow, oh, top, left = R.resize_crop_plan(h, w, size)
    out = []
    for in_size, out_size, first in ((w, ow, left), (h, oh, top)):
        ks, bounds, coeffs = I.axis_plan(in_size, out_size, first, size)
        if pitch is not None:
            assert pitch > ks
            wide = np.zeros((size, pitch), dtype=np.int32)
            wide[:, :ks] = coeffs
            ks, coeffs = pitch, wide
        out += [ks, bounds, coeffs]
    return tuple(out)


def _run(imgs, size, *, first=0, M=None, src_gap=0, dst_gap=0, shift=0, pitch=None):
    """imgs [K][h][w][C] uint8 on the host -> the M destination images [M][C size size + dst_gap] of two launches that agree, with
    every guard and every input checked; image k of the source starts at byte k (h w C + src_gap) of a buffer `shift` bytes off
    16-byte alignment"""
    K, h, w, C = imgs.shape
    M = K if M is None else M
    E, Dn = h * w * C, C * size * size
    src_stride, dst_stride = E + src_gap, Dn + dst_gap
    flat = torch.full((K, src_stride), SRC_GAP, dtype=torch.uint8)
    flat[:, :E] = torch.from_numpy(np.array(imgs)).reshape(K, E)             # a copy: the shared references are read-only
    sb = ByteBuf(flat, DEV, shift=shift)
    assert sb.t.data_ptr() % 16 == shift
    ksh, hb, hc, ksv, vb, vc = _plans(h, w, size, pitch)
    tb = [Int32Buf(torch.from_numpy(t), DEV) for t in (hb, hc, vb, vc)]
    outs = []
    for _ in range(2):
        db = ByteBuf(torch.full((M * dst_stride,), SENTINEL, dtype=torch.uint8), DEV)
        _lib.call("mdm_ingest_resize_crop", src=sb.t.data_ptr(), src_stride=src_stride, K=K, h=h, w=w, C=C, hbounds=tb[0].t.data_ptr(),
                  hcoeffs=tb[1].t.data_ptr(), ksh=ksh, vbounds=tb[2].t.data_ptr(), vcoeffs=tb[3].t.data_ptr(), ksv=ksv,
                  dst=db.t.data_ptr(), dst_stride=dst_stride, M=M, first=first, S=size, stream=_lib.stream())
        torch.cuda.synchronize()
        assert db.guards_intact(), "a byte outside the destination was written"
        outs.append(db.t.cpu())
    assert sb.intact(), "the source was modified"
    assert all(t.intact() for t in tb), "a table was modified"
    assert torch.equal(outs[0], outs[1]), "two launches differ"
    got = outs[0].numpy().reshape(M, dst_stride)
    untouched = [m for m in range(M) if not first <= m < first + K]
    assert (got[untouched] == SENTINEL).all() and (got[:, Dn:] == SENTINEL).all(), "a byte outside the K images was written"
    return got[:, :Dn].reshape(M, C, size, size)


def _geometry(name, pitch=None):
    h, w, C, size, _ = R.GEOMETRY_CASES[name]
    return I.launch_of(w, C, size, _plans(h, w, size, pitch)[0])


def _differing(got, want):
    return int((got != want).sum())


# ------------------------------------------------------------------ the global table first: the cheapest case that reaches <false>
def test_the_global_table_at_a_wider_pitch_gives_the_same_bits():
    """preset256's own tables re-laid at 40 words a row: the table no longer fits LDS, the kernel reads it where it lies, row x at
    x * 40 -- and the pixels are those of the 5-word tables in LDS"""
    name = "preset256"
    h, w, C, size, _ = R.GEOMETRY_CASES[name]
    src, want, pil = R.geometry_reference(name)
    assert _geometry(name)[:2] == (8, True) and _geometry(name, pitch=40)[:2] == (8, False)
    narrow = _run(src[None], size)
    wide = _run(src[None], size, pitch=40)
    print(f"{name}: {_differing(wide, narrow)} bytes differ between the tables in LDS and at pitch 40 in global memory")
    assert _differing(wide, narrow) == 0
    assert _differing(narrow[0], want) == 0 and _differing(wide[0], pil) == 0


# ------------------------------------------------------------------ byte for byte
@pytest.mark.parametrize("name", list(R.GEOMETRY_CASES))
def test_the_kernel_equals_pil_byte_for_byte_at_every_geometry(name):
    h, w, C, size, _ = R.GEOMETRY_CASES[name]
    src, want, pil = R.geometry_reference(name)
    tr, in_lds, _, tiles = _geometry(name)
    assert (tr, in_lds, tiles) == R.GEOMETRY_EXPECTED[name]
    got = _run(src[None], size)[0]
    for what, ref in (("restatement", want), ("live PIL", pil)):
        if ref is not None:
            print(f"{name} (TR {tr}, table in {'LDS' if in_lds else 'global memory'}): {_differing(got, ref)} bytes differ from the {what}")
            assert _differing(got, ref) == 0, (name, what)
    assert pil is not None or name == "wide_12x9000"


# ------------------------------------------------------------------ several images, padded strides, a window of the destination
_WINDOW = {}


def _window_problem(name):
    """three images of the case's shape (the case's own source first) and their references, made once"""
    if name not in _WINDOW:
        h, w, C, size, _ = R.GEOMETRY_CASES[name]
        rng = np.random.RandomState(len(name) + h)
        imgs = np.stack([R.geometry_reference(name)[0]] + [rng.randint(0, 256, size=(h, w, C)).astype(np.uint8) for _ in range(2)])
        _WINDOW[name] = (imgs, [R.resize_crop(im, size) for im in imgs], [R.pil_resize_crop(im, size) for im in imgs])
    return _WINDOW[name]


@pytest.mark.parametrize("name", ("preset128", "table_global_830", "tr7_33x40"))
def test_several_images_and_a_window_on_the_new_routes(name):
    """K = 3 images h w C + 5 bytes apart -- every image and row at another of the 16 alignments -- into images 2, 3, 4 of six
    C S S + 7 bytes apart: images 0, 1 and 5 and the 7-byte gaps keep the sentinel (`_run` holds them to it)"""
    h, w, C, size, _ = R.GEOMETRY_CASES[name]
    imgs, want, pil = _window_problem(name)
    got = _run(imgs, size, first=2, M=6, src_gap=5, dst_gap=7)
    for k in range(3):
        assert _differing(got[2 + k], want[k]) == 0 and _differing(got[2 + k], pil[k]) == 0, (name, k)


# ------------------------------------------------------------------ rows without an aligned middle, at every alignment
@pytest.mark.parametrize("name", ("narrow_40x3_L", "narrow_9x5"))
def test_narrow_rows_at_every_alignment_of_the_source(name):
    h, w, C, size, _ = R.GEOMETRY_CASES[name]
    src, want, pil = R.geometry_reference(name)
    assert w * C < 16
    for shift in range(16):
        got = _run(src[None], size, shift=shift)[0]
        assert _differing(got, want) == 0 and _differing(got, pil) == 0, (name, shift)


# ------------------------------------------------------------------ the host pipeline at a preset size
def test_ingest_arrays_at_a_preset_size_in_several_launches(monkeypatch):
    """shapes A A A B A' at size 128 with room for two A in a chunk: A A | A | B | A', four launches, every image PIL's"""
    rng = np.random.RandomState(21)
    A = (150, 131, 3)
    arrays = [rng.randint(0, 256, size=s).astype(np.uint8) for s in (A, A, A, (140, 200, 3), (131, 150, 3))]
    launches, real = [], I.resize_crop

    def counted(src, K, *a, **kw):
        launches.append(K)
        return real(src, K, *a, **kw)

    monkeypatch.setattr(I, "resize_crop", counted)
    data = I.ingest_arrays(arrays, 128, device=DEV, chunk_bytes=2 * 150 * 131 * 3 + 7)
    assert launches == [2, 1, 1, 1] and data.dtype == torch.uint8 and tuple(data.shape) == (5, 3, 128, 128)
    for k, arr in enumerate(arrays):
        assert _differing(data[k].cpu().numpy(), R.pil_resize_crop(arr, 128)) == 0, k


def test_a_folder_of_files_at_a_preset_size(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(22)
    files = [("cat/a.png", "RGB", (150, 131)), ("cat/b.png", "L", (140, 200)), ("dog/a.png", "RGB", (131, 135))]
    for rel, mode, (h, w) in files:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        Image.fromarray(rng.randint(0, 256, size=(h, w) + ((3,) if mode == "RGB" else ())).astype(np.uint8)).save(str(tmp_path / rel))
    size = 128
    want = []
    for rel, _, _ in files:
        im = Image.open(str(tmp_path / rel)).convert("RGB")
        ow, oh, top, left = I.resize_crop_plan(im.height, im.width, size)
        want.append(np.asarray(im.resize((ow, oh), Image.BILINEAR))[top:top + size, left:left + size].transpose(2, 0, 1))
    ds = D.DeviceDataset.from_folder(str(tmp_path), size, num_timesteps=4, device=DEV)
    assert ds.data.dtype == torch.uint8 and ds.data.is_cuda and (ds.M, ds.C, ds.H, ds.W) == (3, 3, size, size)
    assert _differing(ds.data.cpu().numpy(), np.stack(want)) == 0
    assert ds.label.cpu().tolist() == [0.0, 0.0, 1.0]
