"""MNIST, CIFAR-10 and Flowers102 from the files torchvision keeps under its `root` -- host code, no GPU, no network.

Upstream's `get_dataset` (utils/mydataset.py:86-127) builds these three with `download=True`, which fetches nothing when the files
already lie under `root`: on a machine that holds them torchvision reads them locally, and that is what is here.  The on-disk layouts
are torchvision's, taken from its published source (torchvision is not a dependency: the layouts are *parity unpinned*, DESIGN
finding 69); nothing is fetched, and torchvision's md5 check of the files is not reproduced.

    mnist       path/MNIST/raw/{train,t10k}-{images-idx3,labels-idx1}-ubyte[.gz]          IDX, `read_idx`
    cifar10     path/CIFAR/cifar-10-batches-py/{data_batch_1..5,test_batch}               pickled dicts, `cifar10_arrays`
    flowers102  path/flowers102/flowers-102/{setid.mat,imagelabels.mat,jpg/image_#####.jpg} `flowers102_samples`

`mdm.ingest.get_dataset` stages what these return into a `DeviceDataset`.  lsun needs lmdb and stays refused.
"""
from __future__ import annotations

import gzip
import io
import os
import pickle

import numpy as np

RAW_SETS = {"mnist": ("train", "test", "all"), "cifar10": ("train", "test", "all"), "flowers102": ("train", "val", "test", "all")}
MNIST_FILES = {"train": ("train-images-idx3-ubyte", "train-labels-idx1-ubyte"), "test": ("t10k-images-idx3-ubyte", "t10k-labels-idx1-ubyte")}
CIFAR10_FILES = {"train": tuple(f"data_batch_{i}" for i in range(1, 6)), "test": ("test_batch",)}
FLOWERS102_KEYS = {"train": "trnid", "val": "valid", "test": "tstid"}


def raw_root(path, name):
    """The directory torchvision reads `name` from when upstream hands it `path` (mydataset.py:89, 104, 119)"""
    sub = {"mnist": ("MNIST", "raw"), "cifar10": ("CIFAR", "cifar-10-batches-py"), "flowers102": ("flowers102", "flowers-102")}[name]
    return os.path.join(os.fspath(path), *sub)


def _parts(name, split):
    """`split` as the list of single splits upstream concatenates, in its order ('all' is every one of them)"""
    if split not in RAW_SETS[name]:
        raise ValueError(f"get_dataset: '{name}' has the splits {', '.join(RAW_SETS[name])}, not '{split}'")
    return [s for s in RAW_SETS[name] if s != "all"] if split == "all" else [split]


def _missing(name, root, files):
    return ValueError(f"get_dataset: the files of '{name}' ({', '.join(files)}) are not in {root}; upstream would download them "
                      "there; downloads are not built -- put the files there")


# ------------------------------------------------------------------ IDX (MNIST)
def _idx_file(file):
    """The file `read_idx` reads for `file`: the plain one when it exists (the one torchvision reads), else the .gz, else None"""
    file = os.fspath(file)
    plain = file[:-3] if file.endswith(".gz") else file
    for f in (plain, plain + ".gz"):
        if os.path.isfile(f):
            return f
    return None


def read_idx(file):
    """An IDX file of unsigned bytes -> ndarray of the header's shape.  The header is two zero bytes, the type byte (0x08) and
    the number of dimensions, then one big-endian uint32 per dimension.  `file` is the plain name or the same with .gz; when
    both exist the plain file is read.  A bad magic number, another type, and a payload shorter or longer than the header says are
    ValueError naming the file."""
    found = _idx_file(file)
    if found is None:
        raise FileNotFoundError(f"read_idx: neither {os.fspath(file)} nor its .gz twin exists")
    with (gzip.open(found, "rb") if found.endswith(".gz") else open(found, "rb")) as fh:
        raw = fh.read()
    if len(raw) < 4 or raw[0] != 0 or raw[1] != 0:
        raise ValueError(f"read_idx: {found} does not start with the two zero bytes of an IDX file")
    if raw[2] != 0x08:
        raise ValueError(f"read_idx: {found} has the type byte 0x{raw[2]:02x}; only 0x08 (unsigned byte) is read")
    nd = raw[3]
    if nd < 1 or len(raw) < 4 + 4 * nd:
        raise ValueError(f"read_idx: {found} announces {nd} dimensions and ends inside its header")
    shape = tuple(int(v) for v in np.frombuffer(raw, dtype=">u4", count=nd, offset=4))
    want, have = int(np.prod(shape, dtype=np.int64)), len(raw) - 4 - 4 * nd
    if have != want:
        raise ValueError(f"read_idx: {found} holds {have} payload bytes, its header {shape} says {want}")
    return np.frombuffer(raw, dtype=np.uint8, count=want, offset=4 + 4 * nd).reshape(shape).copy()


def mnist_arrays(path, split):
    """torchvision's `MNIST(path, train=...)` without the images -> (uint8 [M, h, w], int64 [M]); h x w comes from the header (28 x 28
    in the real files).  'all' is train followed by test (mydataset.py:95-98)."""
    root = raw_root(path, "mnist")
    images, labels = [], []
    parts = _parts("mnist", split)
    names = [f for part in parts for f in MNIST_FILES[part]]
    if None in [_idx_file(os.path.join(root, f)) for f in names]:
        raise _missing("mnist", root, names)
    for part in parts:
        files = [os.path.join(root, f) for f in MNIST_FILES[part]]
        x, y = read_idx(files[0]), read_idx(files[1])
        if x.ndim != 3 or y.ndim != 1:
            raise ValueError(f"mnist_arrays: {files[0]} is {x.shape} and {files[1]} is {y.shape}; images are [M, h, w], labels [M]")
        if len(x) != len(y):
            raise ValueError(f"mnist_arrays: {files[0]} holds {len(x)} images, {files[1]} holds {len(y)} labels")
        images.append(x)
        labels.append(y.astype(np.int64))
    return (images[0], labels[0]) if len(images) == 1 else (np.concatenate(images), np.concatenate(labels))


# ------------------------------------------------------------------ pickled batches (CIFAR-10)
def _np_multiarray():
    return np._core.multiarray if hasattr(np, "_core") else np.core.multiarray


class _ArrayUnpickler(pickle.Unpickler):
    """Admits the globals a pickled numpy array needs and no other: dicts, lists, strings and numbers are opcodes and ask for
    none, so a data file can name nothing that runs."""

    def find_class(self, module, name):
        import _codecs
        ok = {("numpy", "ndarray"): np.ndarray, ("numpy", "dtype"): np.dtype, ("_codecs", "encode"): _codecs.encode}
        for mod in ("numpy.core.multiarray", "numpy._core.multiarray"):
            ok[(mod, "_reconstruct")] = _np_multiarray()._reconstruct
            ok[(mod, "scalar")] = _np_multiarray().scalar
        if (module, name) not in ok:
            raise ValueError(f"a data file may not name {module}.{name}")
        return ok[(module, name)]


def load_batch(file):
    """One CIFAR batch file -> its dict, loaded with `encoding="latin1"` as torchvision loads it but through `_ArrayUnpickler`"""
    with open(file, "rb") as fh:
        raw = fh.read()
    try:
        entry = _ArrayUnpickler(io.BytesIO(raw), encoding="latin1").load()
    except ValueError as e:
        raise ValueError(f"cifar10_arrays: {file}: {e}") from None
    if not isinstance(entry, dict):
        raise ValueError(f"cifar10_arrays: {file} holds a {type(entry).__name__}, not a dict")
    return {k.decode("latin1") if isinstance(k, bytes) else k: v for k, v in entry.items()}


def cifar10_arrays(path, split):
    """torchvision's `CIFAR10(path/CIFAR, train=...)` without the images -> (uint8 [M, 32, 32, 3], int64 [M]).  Each file is a
    pickle of a dict with `data` ([n, 3072] uint8, planar R G B) and `labels`, keys as str or bytes; the images come back in the
    interleaved layout PIL sees.  'all' is train then test.  The files are read through an unpickler that admits only what a numpy
    array needs: another global is ValueError, and nothing of it runs.  torchvision's md5 check is NOT reproduced: a file that
    unpickles to the right shapes is taken as it is."""
    root = raw_root(path, "cifar10")
    names = [f for part in _parts("cifar10", split) for f in CIFAR10_FILES[part]]
    if not all(os.path.isfile(os.path.join(root, f)) for f in names):
        raise _missing("cifar10", root, names)
    images, labels = [], []
    for f in names:
        entry = load_batch(os.path.join(root, f))
        if "data" not in entry or "labels" not in entry:
            raise ValueError(f"cifar10_arrays: {os.path.join(root, f)} has the keys {sorted(entry)}, not 'data' and 'labels'")
        data, lab = np.asarray(entry["data"]), np.asarray(entry["labels"], dtype=np.int64).reshape(-1)
        if data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != 3072 or len(data) != len(lab):
            raise ValueError(f"cifar10_arrays: {os.path.join(root, f)}: data is {data.dtype} {data.shape} with {len(lab)} labels; "
                             "a batch is uint8 [n, 3072] with n labels")
        images.append(data.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
        labels.append(lab)
    return np.ascontiguousarray(np.concatenate(images)), np.concatenate(labels)


# ------------------------------------------------------------------ Flowers102
def flowers102_samples(path, split):
    """torchvision's `Flowers102(path/flowers102, split=...)` without the images -> [(file, label)]: the ids of `setid.mat`
    (`trnid`, `valid`, `tstid`) in the order they stand there, `jpg/image_{id:05d}.jpg`, label = `imagelabels.mat`'s 1-based
    `labels[id - 1]` minus 1.  'all' is train, val, test (mydataset.py:123-127).  Needs scipy for the two .mat files."""
    root = raw_root(path, "flowers102")
    parts = _parts("flowers102", split)
    mats = ("setid.mat", "imagelabels.mat")
    if not all(os.path.isfile(os.path.join(root, f)) for f in mats):
        raise _missing("flowers102", root, mats + ("jpg/",))
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError(f"flowers102_samples: setid.mat and imagelabels.mat are read with scipy.io.loadmat, and scipy is not "
                          f"importable ({e})") from None
    ids = loadmat(os.path.join(root, "setid.mat"), squeeze_me=True)
    labels = np.atleast_1d(loadmat(os.path.join(root, "imagelabels.mat"), squeeze_me=True)["labels"]).astype(np.int64) - 1
    samples = []
    for part in parts:
        for i in np.atleast_1d(ids[FLOWERS102_KEYS[part]]).tolist():
            if not 1 <= int(i) <= len(labels):
                raise ValueError(f"flowers102_samples: setid.mat names image {i}, imagelabels.mat has {len(labels)} labels")
            samples.append((os.path.join(root, "jpg", f"image_{int(i):05d}.jpg"), int(labels[int(i) - 1])))
    return samples
