"""The readers of mdm/rawsets.py and the routing of `get_dataset` without a GPU: IDX, CIFAR-10's pickled batches and Flowers102's
.mat files in torchvision's on-disk layouts, every file written here into `tmp_path` (tests/_rawsets_files.py).  No kernel is
launched and nothing outside `tmp_path` is read."""
import gzip
import os
import sys

import numpy as np
import pytest
import torch

import _rawsets_files as F
import mdm
from mdm import ingest as I
from mdm import rawsets as S


# ------------------------------------------------------------------ read_idx
def test_read_idx_round_trips_a_non_square_block_and_a_vector(tmp_path):
    rng = np.random.RandomState(1)
    block = rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8)                 # 7 x 3: swapped height and width would show
    labels = rng.randint(0, 10, size=5).astype(np.uint8)
    F.write_idx(str(tmp_path / "block"), block)
    F.write_idx(str(tmp_path / "labels"), labels)
    got = S.read_idx(str(tmp_path / "block"))
    assert got.dtype == np.uint8 and got.shape == (5, 7, 3) and np.array_equal(got, block)
    got = S.read_idx(tmp_path / "labels")
    assert got.dtype == np.uint8 and got.shape == (5,) and np.array_equal(got, labels)
    assert mdm.read_idx is S.read_idx


def test_read_idx_reads_gz_and_plain_and_the_plain_file_wins(tmp_path):
    a = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    b = a[::-1].copy()
    f = str(tmp_path / "x-idx3-ubyte")
    F.write_idx(f, a, gz=True)
    assert not os.path.exists(f) and os.path.exists(f + ".gz")
    assert np.array_equal(S.read_idx(f), a) and np.array_equal(S.read_idx(f + ".gz"), a)       # either name finds it
    F.write_idx(f, b)
    assert np.array_equal(S.read_idx(f), b) and np.array_equal(S.read_idx(f + ".gz"), b)       # both exist: the plain one
    os.remove(f + ".gz")
    assert np.array_equal(S.read_idx(f + ".gz"), b)
    with pytest.raises(FileNotFoundError):
        S.read_idx(str(tmp_path / "absent"))


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("what", ["magic", "type", "truncated", "overlong", "header"])
def test_read_idx_refuses_and_names_the_file(tmp_path, what, gz):
    a = np.arange(30, dtype=np.uint8).reshape(2, 3, 5)
    raw = {"magic": F.idx_bytes(a, magic=(0, 1)), "type": F.idx_bytes(a, type_byte=0x0D), "truncated": F.idx_bytes(a)[:-1],
           "overlong": F.idx_bytes(a) + b"\0", "header": F.idx_bytes(a)[:9]}[what]
    f = str(tmp_path / f"bad_{what}") + (".gz" if gz else "")
    with (gzip.open(f, "wb") if gz else open(f, "wb")) as fh:
        fh.write(raw)
    with pytest.raises(ValueError, match=f"bad_{what}"):
        S.read_idx(f)


# ------------------------------------------------------------------ mnist_arrays
def test_mnist_arrays_splits_order_and_labels(tmp_path):
    want = F.make_mnist(tmp_path, seed=2)
    for split, n in (("train", 5), ("test", 3), ("all", 8)):
        x, y = S.mnist_arrays(str(tmp_path), split)
        assert x.dtype == np.uint8 and x.shape == (n, 28, 28) and y.dtype == np.int64 and y.shape == (n,)
        assert np.array_equal(x, want[split][0]) and np.array_equal(y, want[split][1]), split
    with pytest.raises(ValueError, match="splits"):
        S.mnist_arrays(str(tmp_path), "val")
    assert mdm.mnist_arrays is S.mnist_arrays


def test_mnist_arrays_takes_the_image_shape_from_the_header(tmp_path):
    want = F.make_mnist(tmp_path, seed=3, shape=(5, 9), gz=())
    x, y = S.mnist_arrays(tmp_path, "all")
    assert x.shape == (8, 5, 9) and np.array_equal(x, want["all"][0]) and np.array_equal(y, want["all"][1])


def test_mnist_arrays_refuses_a_count_mismatch_and_missing_files(tmp_path):
    F.make_mnist(tmp_path, seed=4, gz=())
    raw = os.path.join(str(tmp_path), "MNIST", "raw")
    F.write_idx(os.path.join(raw, "train-labels-idx1-ubyte"), np.zeros(4, dtype=np.uint8))
    with pytest.raises(ValueError, match="5 images.*4 labels"):
        S.mnist_arrays(str(tmp_path), "train")
    S.mnist_arrays(str(tmp_path), "test")                                         # the other pair is whole
    os.remove(os.path.join(raw, "t10k-images-idx3-ubyte"))
    for split in ("test", "all"):
        with pytest.raises(ValueError, match="download") as e:
            S.mnist_arrays(str(tmp_path), split)
        assert raw in str(e.value)
    with pytest.raises(ValueError, match="download") as e:
        S.mnist_arrays(str(tmp_path / "nowhere"), "train")
    assert os.path.join(str(tmp_path / "nowhere"), "MNIST", "raw") in str(e.value)


# ------------------------------------------------------------------ cifar10_arrays
@pytest.mark.parametrize("keys", [str, bytes])
def test_cifar10_arrays_order_layout_and_both_key_types(tmp_path, keys):
    want = F.make_cifar10(tmp_path, seed=5, keys=keys)
    for split, n in (("train", 10), ("test", 3), ("all", 13)):
        x, y = S.cifar10_arrays(str(tmp_path), split)
        assert x.dtype == np.uint8 and x.shape == (n, 32, 32, 3) and x.flags.c_contiguous and y.dtype == np.int64 and y.shape == (n,)
        assert np.array_equal(x, want[split][0]) and np.array_equal(y, want[split][1]), split
    x, _ = S.cifar10_arrays(str(tmp_path), "all")
    for i in range(13):                                                          # plane c of image i is one constant, R G B last
        for c in range(3):
            assert (x[i, :, :, c] == (7 + 3 * i + c) % 256).all(), (i, c)
    with pytest.raises(ValueError, match="splits"):
        S.cifar10_arrays(str(tmp_path), "val")
    assert mdm.cifar10_arrays is S.cifar10_arrays


def test_cifar10_arrays_missing_files(tmp_path):
    F.make_cifar10(tmp_path, seed=6)
    root = os.path.join(str(tmp_path), "CIFAR", "cifar-10-batches-py")
    os.remove(os.path.join(root, "data_batch_3"))
    assert len(S.cifar10_arrays(str(tmp_path), "test")[0]) == 3
    for split in ("train", "all"):
        with pytest.raises(ValueError, match="download") as e:
            S.cifar10_arrays(str(tmp_path), split)
        assert root in str(e.value)


def test_a_cifar_file_that_names_a_foreign_global_runs_nothing(tmp_path):
    F.make_cifar10(tmp_path, seed=7)
    root = os.path.join(str(tmp_path), "CIFAR", "cifar-10-batches-py")
    marker = str(tmp_path / "it_ran")
    # protocol-0 pickle of os.system(": > marker"), a shell builtin: GLOBAL, MARK, STRING, TUPLE, REDUCE, STOP
    evil = b"cos\nsystem\n(S" + repr(f": > {marker}").encode() + b"\ntR."
    with open(os.path.join(root, "test_batch"), "wb") as fh:
        fh.write(evil)
    with pytest.raises(ValueError, match="system") as e:
        S.cifar10_arrays(str(tmp_path), "test")
    assert "test_batch" in str(e.value) and not os.path.exists(marker)
    import pickle
    pickle.loads(evil)                                                           # the same bytes through the stock unpickler DO run
    assert os.path.exists(marker)
    with open(os.path.join(root, "test_batch"), "wb") as fh:                      # a class of the standard library is no better
        pickle.dump({"data": np.zeros((1, 3072), dtype=np.uint8), "labels": [0], "when": __import__("datetime").date(2020, 1, 1)}, fh, protocol=2)
    with pytest.raises(ValueError, match="datetime"):
        S.cifar10_arrays(str(tmp_path), "test")


# ------------------------------------------------------------------ flowers102_samples
def test_flowers102_samples_follow_the_mat_order_with_labels_minus_one(tmp_path):
    root, labels = F.make_flowers102(tmp_path, seed=8, images=False)
    for split in ("train", "val", "test"):
        got = S.flowers102_samples(str(tmp_path), split)
        assert got == [(os.path.join(root, "jpg", f"image_{i:05d}.jpg"), int(labels[i - 1]) - 1) for i in F.FLOWER_IDS[split]], split
        assert all(isinstance(l, int) for _, l in got)
    every = S.flowers102_samples(str(tmp_path), "all")
    assert every == S.flowers102_samples(str(tmp_path), "train") + S.flowers102_samples(str(tmp_path), "val") + \
        S.flowers102_samples(str(tmp_path), "test")
    assert [int(os.path.basename(f)[6:11]) for f, _ in every] == [7, 2, 5, 9, 1, 4]
    with pytest.raises(ValueError, match="splits"):
        S.flowers102_samples(str(tmp_path), "valid")
    with pytest.raises(ValueError, match="download") as e:
        S.flowers102_samples(str(tmp_path / "nowhere"), "train")
    assert os.path.join(str(tmp_path / "nowhere"), "flowers102", "flowers-102") in str(e.value)
    assert mdm.flowers102_samples is S.flowers102_samples


def test_flowers102_samples_without_scipy_says_so(tmp_path, monkeypatch):
    F.make_flowers102(tmp_path, seed=9, images=False)
    for name in [m for m in sys.modules if m == "scipy" or m.startswith("scipy.")]:
        monkeypatch.setitem(sys.modules, name, None)                             # `import scipy...` now raises ImportError
    monkeypatch.setitem(sys.modules, "scipy", None)
    with pytest.raises(ImportError, match="scipy"):
        S.flowers102_samples(str(tmp_path), "train")


# ------------------------------------------------------------------ get_dataset
def test_get_dataset_routes_checks_in_order(tmp_path):
    empty = tmp_path / "empty"
    os.makedirs(str(empty))
    where = {"mnist": ("MNIST", "raw"), "cifar10": ("CIFAR", "cifar-10-batches-py"), "flowers102": ("flowers102", "flowers-102")}
    state = torch.get_rng_state()
    for name, sub in where.items():
        for spelled in (name, name.upper()):
            with pytest.raises(ValueError, match="download") as e:               # before any GPU check, on every machine
                I.get_dataset(str(empty), spelled, 32, "train")
            assert os.path.join(str(empty), *sub) in str(e.value)
    with pytest.raises(ValueError, match="download"):
        I.get_dataset(str(empty), "lsun", 32, "train")
    assert I.DOWNLOADS == ("mnist", "cifar10", "flowers102", "lsun")
    with pytest.raises(ValueError, match="download"):
        I.folder_roots(str(empty), "mnist", "train")
    F.make_mnist(tmp_path, seed=10)
    F.make_cifar10(tmp_path, seed=10)
    F.make_flowers102(tmp_path, seed=10, images=False)
    for name, split in (("mnist", "val"), ("cifar10", "val"), ("flowers102", "valid")):
        with pytest.raises(ValueError, match="splits"):
            I.get_dataset(str(tmp_path), name, 32, split)
    for name, total in (("mnist", 8), ("cifar10", 13), ("flowers102", 6)):
        for num in (0, total + 1):
            with pytest.raises(ValueError, match=f"num_data = {num} of {total} items"):
                I.get_dataset(str(tmp_path), name, 32, "all", True, num)
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("name", ["mnist", "cifar10", "flowers102"])
def test_get_dataset_with_the_files_and_no_gpu_refuses_before_it_draws(tmp_path, name):
    {"mnist": F.make_mnist, "cifar10": F.make_cifar10, "flowers102": F.make_flowers102}[name](tmp_path, seed=11)
    assert len(I.get_dataset.__defaults__) == 2 and mdm.get_dataset is I.get_dataset
    if torch.cuda.is_available():                                                # (with a GPU: tests/test_rawsets_gpu.py)
        return
    state = torch.get_rng_state()
    with pytest.raises(TypeError, match="GPU"):
        I.get_dataset(str(tmp_path), name, 32, "all", num_timesteps=4)
    with pytest.raises(TypeError, match="GPU"):
        I.get_dataset(str(tmp_path), name, 32, "train", True, 2)
    assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(TypeError, match="GPU"):
        I.ingest_block(np.zeros((2, 4, 4), dtype=np.uint8), 2, device="cpu")
    assert mdm.ingest_block is I.ingest_block


def test_ingest_block_refuses_what_is_no_block():
    for bad in (np.zeros((2, 4, 4), dtype=np.float32), np.zeros((4, 4), dtype=np.uint8), np.zeros((2, 4, 4, 2), dtype=np.uint8),
                np.zeros((0, 4, 4), dtype=np.uint8), np.zeros((2, 4, 4, 3, 1), dtype=np.uint8)):
        with pytest.raises(ValueError, match="block"):
            I.ingest_block(bad, 2, device="cpu")
