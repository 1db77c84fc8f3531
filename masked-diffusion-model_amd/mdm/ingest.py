"""Image folders into the device data set (include/mdm_ingest.h, csrc/ingest.hip).

Upstream's `get_dataset` (utils/mydataset.py:63-210) reads celeba_hq, afhqv2, metfaces and stanfordcars with torchvision's
`ImageFolder` and the transform `Resize(size)`, `CenterCrop(size)`, `ToTensor()`, `Normalize([0.5], [0.5])`, and `MyDataset.__init__`
(:245-265) runs that chain over the whole set at the start of every run.  Here the files are decoded by host threads
(`Image.open(f).convert("RGB")`, ImageFolder's loader), consecutive images of one shape are collected in a pinned staging chunk,
and each chunk is ONE asynchronous copy and ONE `mdm_ingest_resize_crop` launch that resizes as PIL does (antialiased bilinear, 22-bit
fixed point, a uint8 rounding between the horizontal and the vertical pass), keeps the centre crop and writes planar uint8 straight
into the tensor that becomes `DeviceDataset.data`.  `ToTensor` + `Normalize` stay the 256-entry table of `mdm.data.normalize_lut()`,
so `ds[i]` and every gathered batch hold upstream's values bit for bit.

mnist, cifar10 and flowers102 -- the sets upstream builds with torchvision's `download=True`, which reads the files under `root` when
they are already there -- are read from those local files by mdm/rawsets.py and come through the same kernel: MNIST and CIFAR-10 are
one block of same-shape images each, and `ingest_block` stages such a block a chunk at a time (one host copy, one asynchronous
copy and one launch per chunk) where `ingest_arrays` would copy 60 000 arrays one by one; Flowers102 is a list of JPEG files and
takes the folder path.  MNIST gives a one-channel data set (PIL mode L, as torchvision hands it to the transform).

What is not built: any fetching (files that are not there are an error that says where they were looked for), torchvision's md5
check, lsun (it needs lmdb; `get_dataset` names it and says so), and `use_augment`: upstream's `MyDataset` never passes it on to
`get_dataset` (mydataset.py:245), and its own `self.transform(sample)` (:275-276) names an undefined variable and raises NameError.
`DeviceLoader(hflip=p)` is the flip there is.

There is no fallback: without a GPU nothing is resized, and the call says so.
"""
from __future__ import annotations

import collections
import functools
import os

import numpy as np
import torch

from . import _lib, rawsets
from ._lib import call, ptr, stream
from .data import DeviceDataset

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
DOWNLOADS = ("mnist", "cifar10", "flowers102", "lsun")
# name -> {split: sub-directories of path/name, in upstream's order}; () is path/name itself
FOLDER_SETS = {
    "celeba_hq": {"train": ("train",), "val": ("val",), "all": ("train", "val")},           # female 0, male 1
    "afhqv2": {"train": ("train",), "test": ("test",), "all": ("train", "test")},           # cat 0, dog 1, wild 2
    "metfaces": {"all": ("",), "train": ("",)},
    "stanfordcars": {"all": ("",), "train": ("",)},
}
CHUNK_BYTES = 64 << 20


def resize_crop_plan(h, w, size):
    """What torchvision's `Resize(size)` + `CenterCrop(size)` make of an h x w image -> (ow, oh, top, left): the shorter side
    becomes `size`, the longer `int(size * long / short)`; the crop starts at Python's `round` of half the excess (halves go to
    even)."""
    h, w, size = int(h), int(w), int(size)
    if min(h, w, size) < 1:
        raise ValueError(f"resize_crop_plan: h, w, size must be positive ({h}, {w}, {size})")
    if w <= h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    return ow, oh, int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))


def image_folder(root):
    """torchvision's `ImageFolder(root)` without the images -> (classes, class_to_idx, samples): the classes are the sorted
    sub-directories, `samples` the `(path, class index)` of every file with an image extension (any letter case) found by a sorted
    walk of each class that follows links.  No sub-directory, or a class without a file, is FileNotFoundError as there."""
    root = os.path.expanduser(os.fspath(root))
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
    class_to_idx = {c: i for i, c in enumerate(classes)}
    samples, found = [], set()
    for c in classes:
        for d, _, names in sorted(os.walk(os.path.join(root, c), followlinks=True)):
            for name in sorted(names):
                if name.lower().endswith(IMG_EXTENSIONS):
                    samples.append((os.path.join(d, name), class_to_idx[c]))
                    found.add(c)
    empty = [c for c in classes if c not in found]
    if empty:
        raise FileNotFoundError(f"Found no valid file for the classes {', '.join(empty)}. Supported extensions are: "
                                f"{', '.join(IMG_EXTENSIONS)}")
    return classes, class_to_idx, samples


def pil_loader(path):
    """ImageFolder's default loader as a [h][w][3] uint8 array"""
    from PIL import Image
    with open(path, "rb") as f:
        return np.asarray(Image.open(f).convert("RGB"))


def decode_threads():
    """Threads of the decode pool: the CPUs this process may run on, 16 at the most (never the machine's count)"""
    return max(1, min(16, len(os.sched_getaffinity(0))))


# ------------------------------------------------------------------ plans
@functools.lru_cache(maxsize=None)
def axis_plan(in_size, out_size, first, count):
    """`mdm_ingest_plan` -> (ks, bounds [count][2] int32, coeffs [count][ks] int32) as host arrays, cached"""
    lib = _lib.load()
    ks = lib.mdm_ingest_plan(in_size, out_size, first, count, None, None)
    if ks < 1:
        _lib.check(ks, "mdm_ingest_plan")
    bounds, coeffs = np.zeros((count, 2), dtype=np.int32), np.zeros((count, ks), dtype=np.int32)
    rc = lib.mdm_ingest_plan(in_size, out_size, first, count, bounds.ctypes.data, coeffs.ctypes.data)
    if rc != ks:
        _lib.check(rc, "mdm_ingest_plan")
    return ks, bounds, coeffs


@functools.lru_cache(maxsize=None)
def _device_axis_plan(in_size, out_size, first, count, device):
    ks, bounds, coeffs = axis_plan(in_size, out_size, first, count)
    return ks, torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device)


def device_plans(h, w, size, device):
    """The two tables of an h x w source at `size` on `device` -> (ksh, hbounds, hcoeffs, ksv, vbounds, vcoeffs): horizontal for
    the kept columns [left, left + size), vertical for the kept rows [top, top + size); uploaded once per shape."""
    ow, oh, top, left = resize_crop_plan(h, w, size)
    return _device_axis_plan(w, ow, left, size, torch.device(device)) + _device_axis_plan(h, oh, top, size, torch.device(device))


def launch_of(w, C, size, ksh):
    """The launch `mdm_ingest_resize_crop` would make, without making it (`mdm_ingest_launch_of`, host arithmetic) -> (rows of a
    workgroup's tile, whether the horizontal table is in LDS, LDS bytes of a workgroup, workgroups per image); None for what
    the launcher refuses -- `mdm_last_error` then says why."""
    import ctypes
    out = (ctypes.c_int32 * 4)()
    if _lib.load().mdm_ingest_launch_of(int(w), int(C), int(size), int(ksh), out) != 0:
        return None
    return out[0], bool(out[1]), out[2], out[3]


def resize_crop(src, K, h, w, C, plans, dst, first, size, src_stride=None):
    """One `mdm_ingest_resize_crop` launch on the current stream: K images [h][w][C] at `src` (uint8 device tensor, image k at
    byte k src_stride) -> images first .. first + K - 1 of `dst` ([M, C, size, size] uint8, contiguous, on the device)."""
    ksh, hb, hc, ksv, vb, vc = plans
    call("mdm_ingest_resize_crop", src=ptr(src), src_stride=int(h * w * C if src_stride is None else src_stride), K=int(K), h=int(h),
         w=int(w), C=int(C), hbounds=ptr(hb), hcoeffs=ptr(hc), ksh=ksh, vbounds=ptr(vb), vcoeffs=ptr(vc), ksv=ksv, dst=ptr(dst),
         dst_stride=int(C * size * size), M=int(dst.shape[0]), first=int(first), S=int(size), stream=stream())


# ------------------------------------------------------------------ the pipeline
class _Chunks:
    """Decoded images in, chunks out: consecutive images of one shape fill a pinned buffer (two of them take turns, so the host
    fills one while the copy of the other runs); a shape change, a full buffer or the end flushes: one async copy, one launch."""

    def __init__(self, M, C, size, device, chunk_bytes):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError(f"mdm.ingest: the images are resized by the kernel of mdm_ingest.h, which needs a GPU, not {self.device}")
        self.data = torch.empty(M, C, size, size, dtype=torch.uint8, device=self.device)
        self.C, self.size, self.chunk_bytes = C, size, int(chunk_bytes)
        self.host, self.free, self.dev = [None, None], [None, None], None
        self.cur, self.shape, self.count, self.first, self.done = 0, None, 0, 0, 0
        self.launches = 0

    def _buffers(self, nbytes):
        cap = max(self.chunk_bytes, nbytes)
        if self.host[self.cur] is None or self.host[self.cur].numel() < cap:
            self.host[self.cur] = torch.empty(cap, dtype=torch.uint8).pin_memory()
        if self.dev is None or self.dev.numel() < cap:
            self.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)      # stream order keeps the old one alive for its kernel
        if self.free[self.cur] is not None:
            self.free[self.cur].synchronize()                                       # the copy out of this buffer has finished
        return cap

    def add(self, arr):
        arr = np.asarray(arr)
        if arr.ndim == 2:
            arr = arr[:, :, None]
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != self.C or 0 in arr.shape:
            raise ValueError(f"mdm.ingest: a decoded image is uint8 [h][w][{self.C}], got {arr.dtype} {arr.shape}")
        if self.done + self.count >= self.data.shape[0]:
            raise ValueError(f"mdm.ingest: more than the {self.data.shape[0]} images announced")
        nbytes = arr.size
        if self.shape is not None and (arr.shape != self.shape or (self.count + 1) * nbytes > self.cap):
            self.flush()
        if self.shape is None:
            self.cap, self.shape, self.count = self._buffers(nbytes), arr.shape, 0
            self.view = self.host[self.cur].numpy()
        self.view[self.count * nbytes:(self.count + 1) * nbytes] = arr.reshape(-1)
        self.count += 1

    def add_block(self, block):
        """`block`: uint8 [K][h][w][C] -> its images in chunks of at most `chunk_bytes` (one image at the least): one host copy
        into the pinned buffer, then `flush`, per chunk"""
        K, h, w, C = block.shape
        if C != self.C:
            raise ValueError(f"mdm.ingest: the block has {C} channels, the data set {self.C}")
        self.flush()
        if self.done + K > self.data.shape[0]:
            raise ValueError(f"mdm.ingest: more than the {self.data.shape[0]} images announced")
        nbytes = h * w * C
        per = max(1, self.chunk_bytes // nbytes)
        for lo in range(0, K, per):
            n = min(per, K - lo)
            self.cap, self.shape, self.count = self._buffers(n * nbytes), (h, w, C), n
            np.copyto(self.host[self.cur].numpy()[:n * nbytes].reshape(n, h, w, C), block[lo:lo + n])
            self.flush()

    def flush(self):
        if self.shape is None:
            return
        h, w, C = self.shape
        n = self.count * h * w * C
        with torch.cuda.device(self.device):
            self.dev[:n].copy_(self.host[self.cur][:n], non_blocking=True)
            self.free[self.cur] = torch.cuda.Event()
            self.free[self.cur].record()
            resize_crop(self.dev, self.count, h, w, C, device_plans(h, w, self.size, self.device), self.data, self.done, self.size)
        self.launches += 1
        self.done += self.count
        self.cur, self.shape, self.count = 1 - self.cur, None, 0

    def finish(self):
        self.flush()
        if self.done != self.data.shape[0]:
            raise ValueError(f"mdm.ingest: {self.done} images arrived, {self.data.shape[0]} were announced")
        return self.data


def ingest_arrays(arrays, size, *, C=3, device=None, chunk_bytes=CHUNK_BYTES):
    """Decoded images (a sequence of uint8 [h][w][C] arrays, [h][w] for C = 1; shapes may differ) -> uint8 device tensor
    [M, C, size, size]: each resized and centre-cropped as `Resize(size)` + `CenterCrop(size)` do on the PIL image."""
    arrays = list(arrays)
    if not arrays:
        raise ValueError("mdm.ingest: no images")
    chunks = _Chunks(len(arrays), C, int(size), _device(device), chunk_bytes)
    for arr in arrays:
        chunks.add(arr)
    return chunks.finish()


def ingest_block(block, size, *, device=None, chunk_bytes=CHUNK_BYTES):
    """A block of same-shape decoded images (uint8 [K, h, w], or [K, h, w, C] with C 1 or 3; any strides) -> uint8 device tensor
    [K, C, size, size], the bytes `ingest_arrays` gives for the same images.  The block is cut into chunks of at most
    `chunk_bytes`; each is ONE host copy into the pinned buffer (the two buffers take turns), one asynchronous copy and one
    `mdm_ingest_resize_crop` launch.  At `size == h == w` the plans are the identity tables and the kernel writes the source
    bytes, planar."""
    block = np.asarray(block)
    if block.ndim == 3:
        block = block[:, :, :, None]
    if block.dtype != np.uint8 or block.ndim != 4 or block.shape[3] not in (1, 3) or 0 in block.shape:
        raise ValueError(f"mdm.ingest: a block is a non-empty uint8 [K][h][w] or [K][h][w][C] with C 1 or 3, got {block.dtype} {block.shape}")
    chunks = _Chunks(block.shape[0], block.shape[3], int(size), _device(device), chunk_bytes)
    chunks.add_block(block)
    return chunks.finish()


def ingest_files(paths, size, *, device=None, chunk_bytes=CHUNK_BYTES, loader=pil_loader, threads=None):
    """Image files -> uint8 device tensor [M, 3, size, size], in the order of `paths`.  `loader(path)` runs on a pool of
    `decode_threads()` host threads, at most four files per thread ahead of the one being staged, so the decoded images held at
    once are bounded whatever the size of the set."""
    from concurrent.futures import ThreadPoolExecutor
    paths = list(paths)
    if not paths:
        raise ValueError("mdm.ingest: no files")
    chunks = _Chunks(len(paths), 3, int(size), _device(device), chunk_bytes)
    threads = decode_threads() if threads is None else max(1, min(int(threads), decode_threads()))
    with ThreadPoolExecutor(max_workers=threads) as pool:
        ahead, todo = collections.deque(), iter(paths)
        for p in todo:
            ahead.append(pool.submit(loader, p))
            if len(ahead) >= 4 * threads:
                chunks.add(ahead.popleft().result())
        while ahead:
            chunks.add(ahead.popleft().result())
    return chunks.finish()


def _device(device):
    if device is None:
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def _need_gpu(device):
    device = _device(device)
    if device.type != "cuda":
        raise TypeError(f"mdm.ingest: the images are resized by the kernel of mdm_ingest.h, which needs a GPU, not {device}")
    return device


def dataset_from_samples(samples, size, *, num_timesteps=1, device=None, chunk_bytes=CHUNK_BYTES, **kw):
    """`(path, label)` pairs -> DeviceDataset, as `MyDataset.__init__` materialises them (mydataset.py:246-265): `random` is
    drawn first from the default host generator, then every item is read once -- reading draws nothing, there or here.  The
    uint8 tensor the kernel filled IS the data set's `data`; `lut` stays `normalize_lut()` unless `lut=` says otherwise."""
    samples = list(samples)
    if not samples:
        raise ValueError("mdm.ingest: the data set is empty")
    device = _need_gpu(device)
    random = torch.FloatTensor(len(samples), int(num_timesteps)).uniform_(-1.0, 1.0)
    data = ingest_files([p for p, _ in samples], size, device=device, chunk_bytes=chunk_bytes)
    return DeviceDataset(data, torch.tensor([float(l) for _, l in samples]), random, device=device, **kw)


def folder_roots(path, name, split):
    """The ImageFolder roots upstream's `get_dataset` reads for `(name, split)`, in its order of concatenation"""
    key = str(name).lower()
    if key in DOWNLOADS:
        raise ValueError(f"get_dataset: '{name}' is one of the data sets upstream downloads ({', '.join(DOWNLOADS)}), not an image "
                         "folder; downloads are not built -- get_dataset reads the local files of mnist, cifar10 and flowers102 "
                         "(mdm/rawsets.py); lsun needs lmdb: decode it yourself and give the tensor to DeviceDataset")
    if key not in FOLDER_SETS:
        raise ValueError(f"get_dataset: unknown data set '{name}'; the folder-backed ones are {', '.join(FOLDER_SETS)}")
    if split not in FOLDER_SETS[key]:
        raise ValueError(f"get_dataset: '{name}' has the splits {', '.join(FOLDER_SETS[key])}, not '{split}'")
    return [os.path.join(path, key, sub) if sub else os.path.join(path, key) for sub in FOLDER_SETS[key][split]]


def _first(items, data_subset, num_data):
    """`Subset(dataset, range(0, num_data))` of upstream's MyDataset: the number of leading items that are kept"""
    if not data_subset:
        return len(items)
    if not 0 < int(num_data) <= len(items):
        raise ValueError(f"get_dataset: num_data = {num_data} of {len(items)} items")
    return int(num_data)


def dataset_from_block(images, labels, size, *, num_timesteps=1, device=None, chunk_bytes=CHUNK_BYTES, **kw):
    """A block of same-shape decoded images (see `ingest_block`) and their labels -> DeviceDataset, as `MyDataset.__init__`
    materialises them: refused without a GPU before anything is drawn, then `random` from the default host generator, then the
    images.  The channel count is the block's: 1 for [M, h, w]."""
    device = _need_gpu(device)
    random = torch.FloatTensor(len(images), int(num_timesteps)).uniform_(-1.0, 1.0)
    data = ingest_block(images, size, device=device, chunk_bytes=chunk_bytes)
    return DeviceDataset(data, torch.as_tensor(np.asarray(labels, dtype=np.float32)), random, device=device, **kw)


def get_dataset(path, name, size, split, data_subset=False, num_data=0, *, num_timesteps=1, device=None, **kw):
    """Upstream's `MyDataset(path, name, size, split, data_subset, num_data, num_timesteps=...)` as a DeviceDataset: the directory
    layout, the `split` words ('all' concatenates in upstream's order) and the labels are upstream's.
    celeba_hq, afhqv2, metfaces, stanfordcars: image folders (celeba_hq female 0 / male 1, afhqv2 cat 0 / dog 1 / wild 2: the
    sorted class folders of every root).  mnist (one channel), cifar10, flowers102: torchvision's local files (mdm/rawsets.py);
    when they are not under `path` the call says where it looked -- upstream would download them there, and downloads are not
    built.  lsun raises.  `data_subset` keeps the first `num_data` items (`Subset(dataset, range(0, num_data))`); only those are
    staged or decoded.  `use_augment` is not a parameter: upstream's MyDataset never passes it on to its get_dataset, and its own
    flip branch raises NameError."""
    key = str(name).lower()
    if key in ("mnist", "cifar10"):
        images, labels = (rawsets.mnist_arrays if key == "mnist" else rawsets.cifar10_arrays)(path, split)
        n = _first(images, data_subset, num_data)
        return dataset_from_block(images[:n], labels[:n], size, num_timesteps=num_timesteps, device=device, **kw)
    if key == "flowers102":
        samples = rawsets.flowers102_samples(path, split)
    else:
        samples = []
        for root in folder_roots(path, name, split):
            samples += image_folder(root)[2]
    samples = samples[:_first(samples, data_subset, num_data)]
    return dataset_from_samples(samples, size, num_timesteps=num_timesteps, device=device, **kw)
