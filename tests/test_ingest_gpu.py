"""The ingest kernel on the device (include/mdm_ingest.h, csrc/ingest.hip): `mdm_ingest_resize_crop` byte for byte against the
PIL-made fixture (tests/golden/ingest.npz), the numpy restatement (tests/_ingest_ref.py) and the installed PIL on every case of
`_ingest_ref.CASES` -- each the smallest input that reaches one way of going wrong -- then padded strides and a destination window,
tables that are wrong on purpose (the kernel clamps: wrong pixels, its own images only), the chunking of the host pipeline, and one
folder of files end to end through `DeviceDataset.from_folder` and a `DeviceLoader`.  0 differing bytes everywhere."""
import os

import numpy as np
import pytest
import torch

import _ingest_ref as R
from mdm import _lib
from mdm import data as D
from mdm import ingest as I

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("ingest")


def _launch(src_dev, K, h, w, C, tables, dst, first, size, src_stride):
    ksh, hb, hc, ksv, vb, vc = tables
    _lib.call("mdm_ingest_resize_crop", src=src_dev.data_ptr(), src_stride=src_stride, K=K, h=h, w=w, C=C, hbounds=hb.data_ptr(),
              hcoeffs=hc.data_ptr(), ksh=ksh, vbounds=vb.data_ptr(), vcoeffs=vc.data_ptr(), ksv=ksv, dst=dst.data_ptr(),
              dst_stride=C * size * size, M=dst.shape[0], first=first, S=size, stream=_lib.stream())


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_kernel_equals_pil_byte_for_byte(fixture, name):
    h, w, C, size, _ = R.CASES[name]
    src = R.case_source(name)
    dst = torch.full((1, C, size, size), 0xAB, dtype=torch.uint8, device=DEV)
    _launch(torch.from_numpy(src).to(DEV), 1, h, w, C, I.device_plans(h, w, size, DEV), dst, 0, size, h * w * C)
    got = dst[0].cpu().numpy()
    for what, want in (("fixture", fixture[name + "/out"]), ("restatement", R.resize_crop(src, size)), ("live PIL", R.pil_resize_crop(src, size))):
        differing = int((got != want).sum())
        print(f"{name}: {differing} bytes differ from the {what}")
        assert differing == 0, (name, what)


def test_padded_source_stride_and_a_window_of_the_destination():
    """K = 3 images 5 bytes apart in a 6-image destination prefilled with 0xAB, first = 2: images 0, 1 and 5 stay 0xAB"""
    h, w, C, size = 37, 53, 3, 8
    rng = np.random.RandomState(11)
    imgs = rng.randint(0, 256, size=(3, h, w, C)).astype(np.uint8)
    stride = h * w * C + 5
    flat = np.full(3 * stride, 0x5C, dtype=np.uint8)
    for k in range(3):
        flat[k * stride:k * stride + h * w * C] = imgs[k].reshape(-1)
    dst = torch.full((6, C, size, size), 0xAB, dtype=torch.uint8, device=DEV)
    _launch(torch.from_numpy(flat).to(DEV), 3, h, w, C, I.device_plans(h, w, size, DEV), dst, 2, size, stride)
    got = dst.cpu().numpy()
    for k in range(3):
        assert int((got[2 + k] != R.pil_resize_crop(imgs[k], size)).sum()) == 0, k
    assert (got[[0, 1, 5]] == 0xAB).all()


def _clamped_reference(src, size, hb, hc, ksh, vb, vc, ksv):
    """What the header says a table of any content gives: a first index is clamped into the image, a tap count into [0, ks], a
    column past the last one reads the last one, a row past the last one is dropped"""
    h, w, C = src.shape
    wide = src.astype(np.int64)
    tmp = np.empty((h, size, C), dtype=np.int64)
    for x in range(size):
        lo, cnt = int(np.clip(hb[x, 0], 0, w - 1)), int(np.clip(hb[x, 1], 0, ksh))
        acc = np.full((h, C), 1 << 21, dtype=np.int64)
        for i in range(cnt):
            acc += wide[:, min(lo + i, w - 1)] * int(hc[x, i])
        tmp[:, x] = np.clip(acc.astype(np.int32) >> 22, 0, 255)
    out = np.empty((size, size, C), dtype=np.uint8)
    for y in range(size):
        lo, cnt = int(np.clip(vb[y, 0], 0, h - 1)), int(np.clip(vb[y, 1], 0, ksv))
        acc = np.full((size, C), 1 << 21, dtype=np.int64)
        for i in range(cnt):
            if lo + i < h:
                acc += tmp[lo + i] * int(vc[y, i])
        out[y] = np.clip(acc.astype(np.int32) >> 22, 0, 255)
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def test_a_wrong_plan_gives_wrong_pixels_and_writes_only_its_own_images():
    """first indices of -7 and past the end, tap counts below 0 and past ks: the launch completes, the result is what the clamps
    define, and the images around its two stay as they were.  Nothing is made to fault: the indices never leave the image."""
    h, w, C, size = 37, 53, 3, 8
    rng = np.random.RandomState(12)
    imgs = rng.randint(0, 256, size=(2, h, w, C)).astype(np.uint8)
    ow, oh, top, left = R.resize_crop_plan(h, w, size)
    ksh, hb, hc = (np.array(v) if isinstance(v, np.ndarray) else v for v in R.plan(w, ow, left, size))
    ksv, vb, vc = (np.array(v) if isinstance(v, np.ndarray) else v for v in R.plan(h, oh, top, size))
    hb[0] = (-7, ksh); hb[1] = (w + 100, 3); hb[2] = (w - 2, ksh + 50); hb[3] = (5, -4); hb[4] = (2 ** 31 - 1, 2 ** 31 - 1)
    vb[0] = (-7, ksv); vb[1] = (h + 100, 3); vb[2] = (h - 2, ksv + 50); vb[3] = (5, -4); vb[7] = (-2 ** 31, 2 ** 31 - 1)
    tables = (ksh, torch.from_numpy(hb).to(DEV), torch.from_numpy(hc).to(DEV), ksv, torch.from_numpy(vb).to(DEV), torch.from_numpy(vc).to(DEV))
    dst = torch.full((4, C, size, size), 0xAB, dtype=torch.uint8, device=DEV)
    _launch(torch.from_numpy(imgs).to(DEV), 2, h, w, C, tables, dst, 1, size, h * w * C)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[[0, 3]] == 0xAB).all()
    for k in range(2):
        assert int((got[1 + k] != _clamped_reference(imgs[k], size, hb, hc, ksh, vb, vc, ksv)).sum()) == 0, k
        assert int((got[1 + k] != R.pil_resize_crop(imgs[k], size)).sum()) > 0          # wrong pixels, as promised


def test_a_launch_gives_the_same_bits_twice_and_many_row_tiles():
    """size 20 is three row tiles of 8, 8 and 4 rows; K = 5 images; two launches, one result"""
    h, w, C, size = 45, 61, 3, 20
    imgs = np.random.RandomState(13).randint(0, 256, size=(5, h, w, C)).astype(np.uint8)
    src = torch.from_numpy(imgs).to(DEV)
    a = torch.zeros((5, C, size, size), dtype=torch.uint8, device=DEV)
    b = torch.full((5, C, size, size), 255, dtype=torch.uint8, device=DEV)
    I.resize_crop(src, 5, h, w, C, I.device_plans(h, w, size, DEV), a, 0, size)
    I.resize_crop(src, 5, h, w, C, I.device_plans(h, w, size, DEV), b, 0, size)
    assert torch.equal(a, b)
    for k in range(5):
        assert int((a[k].cpu().numpy() != R.pil_resize_crop(imgs[k], size)).sum()) == 0, k


def test_mixed_shapes_flush_the_chunk_and_full_chunks_split():
    """shapes A A A B A with room for two A in a chunk: A A | A | B | A, four launches, every image right"""
    rng = np.random.RandomState(14)
    A, B = (30, 22, 3), (19, 41, 3)
    arrays = [rng.randint(0, 256, size=s).astype(np.uint8) for s in (A, A, A, B, A)]
    chunks = I._Chunks(5, 3, 8, DEV, chunk_bytes=2 * 30 * 22 * 3 + 7)
    for arr in arrays:
        chunks.add(arr)
    data = chunks.finish()
    assert chunks.launches == 4 and data.dtype == torch.uint8 and tuple(data.shape) == (5, 3, 8, 8)
    for k, arr in enumerate(arrays):
        assert int((data[k].cpu().numpy() != R.pil_resize_crop(arr, 8)).sum()) == 0, k
    grey = [rng.randint(0, 256, size=(28, 28)).astype(np.uint8) for _ in range(3)]
    one = I.ingest_arrays(grey, 32, C=1, device=DEV)
    for k, arr in enumerate(grey):
        assert int((one[k].cpu().numpy() != R.pil_resize_crop(arr[:, :, None], 32)).sum()) == 0, k
    with pytest.raises(ValueError):
        I.ingest_arrays([np.zeros((4, 4, 4), dtype=np.uint8)], 2, device=DEV)


def test_a_folder_of_files_end_to_end(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(15)
    files = [("cat/a.png", "RGB", (23, 31)), ("cat/b.jpg", "RGB", (40, 33)), ("cat/c.png", "L", (17, 29)),
             ("dog/a.png", "RGBA", (26, 16)), ("dog/b.png", "RGB", (64, 9)), ("dog/sub/c.PNG", "RGB", (12, 50))]
    for rel, mode, (h, w) in files:
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        bands = {"L": (), "RGB": (3,), "RGBA": (4,)}[mode]
        Image.fromarray(rng.randint(0, 256, size=(h, w) + bands).astype(np.uint8)).save(str(tmp_path / rel))
    size = 8
    want = []
    for rel, _, _ in files:
        im = Image.open(str(tmp_path / rel)).convert("RGB")
        ow, oh, top, left = I.resize_crop_plan(im.height, im.width, size)
        out = np.asarray(im.resize((ow, oh), Image.BILINEAR))[top:top + size, left:left + size]
        want.append(out.transpose(2, 0, 1))
    want = torch.from_numpy(np.stack(want))

    torch.manual_seed(3)
    ds = D.DeviceDataset.from_folder(str(tmp_path), size, num_timesteps=4, device=DEV)
    state = torch.get_rng_state()
    torch.manual_seed(3)
    rnd = torch.FloatTensor(6, 4).uniform_(-1.0, 1.0)                        # drawn where upstream draws it; reading items draws nothing
    assert torch.equal(torch.get_rng_state(), state)
    assert ds.data.dtype == torch.uint8 and ds.data.is_cuda and (ds.M, ds.C, ds.H, ds.W, ds.R) == (6, 3, size, size, 4)
    assert int((ds.data.cpu() != want).sum()) == 0
    assert ds.label.cpu().tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0] and torch.equal(ds.random.cpu(), rnd)
    lut = D.normalize_lut()
    assert torch.equal(ds.lut_host, lut)
    for i in range(6):
        x, l, r = ds[i]
        assert torch.equal(x, lut[want[i].long()]) and float(l) == float(i // 3) and torch.equal(r, rnd[i])
    batches = [(x.cpu().clone(), l.cpu().clone(), r.cpu().clone()) for x, l, r in D.DeviceLoader(ds, 4, shuffle=False, drop_last=False)]
    assert [len(b[0]) for b in batches] == [4, 2]
    assert torch.equal(torch.cat([b[0] for b in batches]), lut[want.long()])
    assert torch.cat([b[1] for b in batches]).tolist() == ds.label.cpu().tolist() and torch.equal(torch.cat([b[2] for b in batches]), rnd)
    first = D.DeviceDataset.from_folder(str(tmp_path), size, num_data=2, device=DEV)
    assert len(first) == 2 and int((first.data.cpu() != want[:2]).sum()) == 0
