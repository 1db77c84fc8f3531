"""Synthetic MNIST / CIFAR-10 / Flowers102 trees in torchvision's on-disk layouts, written by the tests that read them
(tests/test_rawsets_cpu.py, tests/test_rawsets_gpu.py).  Nothing is committed and nothing is fetched: IDX files are written by
hand, CIFAR batches with `pickle.dump(protocol=2)`, the .mat files with `scipy.io.savemat`, the JPEGs by PIL."""
import gzip
import os
import pickle
import struct

import numpy as np


def idx_bytes(arr, type_byte=0x08, magic=(0, 0)):
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    return bytes(magic) + bytes([type_byte, arr.ndim]) + b"".join(struct.pack(">I", d) for d in arr.shape) + arr.tobytes()


def write_idx(file, arr, gz=False, **kw):
    os.makedirs(os.path.dirname(file), exist_ok=True)
    with (gzip.open(file + ".gz", "wb") if gz else open(file, "wb")) as fh:
        fh.write(idx_bytes(arr, **kw))


def make_mnist(path, seed=0, shape=(28, 28), gz=("t10k-images-idx3-ubyte",)):
    """5 train and 3 test images under path/MNIST/raw (the files named in `gz` compressed) -> {split: (images, labels)}"""
    rng = np.random.RandomState(seed)
    root = os.path.join(str(path), "MNIST", "raw")
    out = {}
    for split, stem, n in (("train", "train", 5), ("test", "t10k", 3)):
        x = rng.randint(0, 256, size=(n,) + shape).astype(np.uint8)
        y = rng.randint(0, 10, size=n).astype(np.uint8)
        for name, arr in ((f"{stem}-images-idx3-ubyte", x), (f"{stem}-labels-idx1-ubyte", y)):
            write_idx(os.path.join(root, name), arr, gz=name in gz)
        out[split] = (x, y.astype(np.int64))
    out["all"] = (np.concatenate([out["train"][0], out["test"][0]]), np.concatenate([out["train"][1], out["test"][1]]))
    return out


def make_cifar10(path, seed=0, keys=str, planes="constant"):
    """Five train batches of 2 images and a test batch of 3 under path/CIFAR/cifar-10-batches-py, keys as `str` or `bytes`
    -> {split: (images [M, 32, 32, 3], labels)}.  planes 'constant': plane c of image i holds (7 + 3 i + c) % 256 everywhere, so a
    wrong transpose or channel order cannot pass; 'random': seeded bytes."""
    rng = np.random.RandomState(seed)
    root = os.path.join(str(path), "CIFAR", "cifar-10-batches-py")
    os.makedirs(root, exist_ok=True)
    k = (lambda s: s.encode()) if keys is bytes else (lambda s: s)
    files = [f"data_batch_{i}" for i in range(1, 6)] + ["test_batch"]
    planar, labels, i = [], [], 0
    for name in files:
        n = 3 if name == "test_batch" else 2
        if planes == "constant":
            data = np.stack([np.repeat(np.array([(7 + 3 * (i + j) + c) % 256 for c in range(3)], dtype=np.uint8), 1024) for j in range(n)])
        else:
            data = rng.randint(0, 256, size=(n, 3072)).astype(np.uint8)
        lab = [int(v) for v in rng.randint(0, 10, size=n)]
        with open(os.path.join(root, name), "wb") as fh:
            pickle.dump({k("data"): data, k("labels"): lab, k("batch_label"): k(name)}, fh, protocol=2)
        planar.append(data); labels += lab; i += n
    x = np.concatenate(planar).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    y = np.array(labels, dtype=np.int64)
    return {"train": (x[:10], y[:10]), "test": (x[10:], y[10:]), "all": (x, y)}


FLOWER_IDS = {"train": [7, 2], "val": [5], "test": [9, 1, 4]}           # out of numeric order on purpose
FLOWER_SHAPES = {1: (23, 31), 2: (40, 33), 4: (17, 29), 5: (26, 16), 7: (64, 9), 9: (12, 50)}      # h, w


def make_flowers102(path, seed=0, images=True):
    """setid.mat / imagelabels.mat (10 labels, 1-based) and, with `images`, the six JPEGs of FLOWER_IDS under
    path/flowers102/flowers-102 -> (root, labels as stored)"""
    from scipy.io import savemat
    rng = np.random.RandomState(seed)
    root = os.path.join(str(path), "flowers102", "flowers-102")
    os.makedirs(os.path.join(root, "jpg"), exist_ok=True)
    labels = rng.randint(1, 103, size=10).astype(np.uint8)
    savemat(os.path.join(root, "setid.mat"), {"trnid": np.array([FLOWER_IDS["train"]], dtype=np.uint16),
                                              "valid": np.array([FLOWER_IDS["val"]], dtype=np.uint16),
                                              "tstid": np.array([FLOWER_IDS["test"]], dtype=np.uint16)})
    savemat(os.path.join(root, "imagelabels.mat"), {"labels": labels[None, :]})
    if images:
        from PIL import Image
        for i, (h, w) in FLOWER_SHAPES.items():
            Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(root, "jpg", f"image_{i:05d}.jpg"))
    return root, labels.astype(np.int64)
