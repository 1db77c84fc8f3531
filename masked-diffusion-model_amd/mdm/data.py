"""The data set in device memory and the loader that gathers a batch with one launch (include/mdm_data.h, csrc/data.hip).

`DeviceDataset` is upstream's `MyDataset` (utils/mydataset.py:235-278): the whole set as one tensor plus a label and a row of
`random` per image -- here uploaded once, as uint8 or fp32.  `DeviceLoader` is what `get_dataloader` builds around it
(main_train_masked.py:92-102: `DataLoader(shuffle=True, drop_last=True, pin_memory=True)` with workers): it visits the indices a
`torch.utils.data.DataLoader` with the same arguments visits and draws from the same host generators, but a batch is ONE
`mdm_data_gather` launch on the current stream that writes `(x0, label, random)` into device buffers -- nothing is indexed,
collated, pinned or copied on the host per step.  `Trainer` binds the loader to `TrainStep.x0`, so the batch lands where the
captured step reads it and the step runs with `x0=None`.

There is no fallback: a data set that is not on a GPU cannot be gathered and says so.
"""
from __future__ import annotations

import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler

from ._lib import call, ptr, stream

KIND_F32, KIND_U8 = 0, 1


def normalize_lut():
    """The 256 values of upstream's `ToTensor()` + `Normalize([0.5], [0.5])` of a uint8 pixel, computed by torch as torchvision
    computes them: 0 -> -1, 255 -> 1."""
    u = torch.arange(256, dtype=torch.uint8)
    return (u.float().div(255) - 0.5) / 0.5


class DeviceDataset:
    """`data`: uint8 or float32 tensor / ndarray [M, C, H, W], uploaded once.  `label` [M] defaults to zeros; `random`
    [M, num_timesteps] defaults to `torch.FloatTensor(M, num_timesteps).uniform_(-1, 1)`, drawn from the default host generator
    where upstream draws it (mydataset.py:261).  uint8 data is read through `lut` (256 floats; default `normalize_lut()`).

    `len(ds)` and `ds[i] -> (data, label, random)` as CPU tensors (fp32 data, after the table) make it a map-style data set:
    `Tester` and `evaluate` read it like upstream's."""

    def __init__(self, data, label=None, random=None, *, lut=None, num_timesteps=1, device=None):
        data = torch.as_tensor(data)
        if data.dim() != 4 or data.dtype not in (torch.uint8, torch.float32) or data.shape[0] == 0:
            raise ValueError(f"DeviceDataset: data must be a non-empty uint8 or float32 [M, C, H, W], got {data.dtype} {tuple(data.shape)}")
        M = data.shape[0]
        if random is None:
            random = torch.FloatTensor(M, int(num_timesteps)).uniform_(-1.0, 1.0)
        random = torch.as_tensor(random, dtype=torch.float32).reshape(M, -1)
        label = torch.zeros(M) if label is None else torch.as_tensor(label, dtype=torch.float32).reshape(M)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.kind = KIND_U8 if data.dtype == torch.uint8 else KIND_F32
        if self.kind == KIND_U8:
            lut = normalize_lut() if lut is None else torch.as_tensor(lut, dtype=torch.float32).reshape(-1)
            if lut.numel() != 256:
                raise ValueError(f"DeviceDataset: lut has {lut.numel()} entries, a uint8 table has 256")
        elif lut is not None:
            raise ValueError("DeviceDataset: lut is the table of uint8 data; float32 data is stored as it is")
        self.lut_host = None if lut is None else lut.contiguous()
        self.lut = None if lut is None else self.lut_host.to(self.device)
        self.data = data.contiguous().to(self.device)
        self.label, self.random = label.contiguous().to(self.device), random.contiguous().to(self.device)
        self.M, self.C, self.H, self.W = (int(v) for v in data.shape)
        self.R = int(random.shape[1])
        self.img_stride = self.C * self.H * self.W

    @classmethod
    def from_dataset(cls, dataset, *, num_timesteps=1, device=None, **kw):
        """Materialise a map-style data set of `(image, label)` items the way `MyDataset.__init__` does (mydataset.py:246-265):
        `random` is drawn first, then every item is read once.  uint8 images stay uint8 (and go through `lut`)."""
        M = len(dataset)
        random = torch.FloatTensor(M, int(num_timesteps)).uniform_(-1.0, 1.0)
        first = torch.as_tensor(dataset[0][0])
        data = torch.zeros((M,) + tuple(first.shape), dtype=torch.uint8 if first.dtype == torch.uint8 else torch.float32)
        label = torch.zeros(M)
        for i in range(M):
            item = dataset[i]
            data[i] = torch.as_tensor(item[0])
            label[i] = float(item[1])
        return cls(data, label, random, device=device, **kw)

    @classmethod
    def from_folder(cls, root, size, *, num_data=None, num_timesteps=1, device=None, **kw):
        """An `ImageFolder(root)` of image files under upstream's transform (`Resize(size)`, `CenterCrop(size)`, `ToTensor()`,
        `Normalize([0.5], [0.5])`), materialised as `MyDataset.__init__` does: see mdm/ingest.py.  The files are decoded on host
        threads and resized and cropped on the device, byte for byte as PIL does; labels are the sorted class folders' indices;
        `num_data` keeps the first items and decodes only those."""
        from . import ingest
        samples = ingest.image_folder(root)[2]
        if num_data is not None:
            if not 0 < int(num_data) <= len(samples):
                raise ValueError(f"DeviceDataset.from_folder: num_data = {num_data} of {len(samples)} items")
            samples = samples[:int(num_data)]
        return ingest.dataset_from_samples(samples, size, num_timesteps=num_timesteps, device=device, **kw)

    def __len__(self):
        return self.M

    def __getitem__(self, i):
        i = int(i)
        if not -self.M <= i < self.M:
            raise IndexError(f"DeviceDataset index {i} out of range for {self.M} images")
        i %= self.M
        row = self.data[i].cpu()
        return (row if self.kind == KIND_F32 else self.lut_host[row.long()]), self.label[i].cpu(), self.random[i].cpu()

    def _on_gpu(self, what):
        if self.data.device.type != "cuda":
            raise TypeError(f"DeviceDataset.{what}: the data set is on {self.data.device}, the kernels of mdm_data.h need it on a GPU")

    def gather(self, index, first, N, x0, flip=None, label_out=None, random_out=None):
        """One `mdm_data_gather` launch on the current stream: `x0[n]` = image `index[first + n]` for n < N (`index`: int64 device
        tensor), mirrored along W where `flip[n]` (uint8 device tensor) is non-zero; labels and `random` rows with it."""
        self._on_gpu("gather")
        call("mdm_data_gather", src=ptr(self.data), kind=self.kind, img_stride=self.img_stride, M=self.M, C=self.C, H=self.H,
             W=self.W, lut=ptr(self.lut), index=ptr(index), first=int(first), N=int(N), flip=ptr(flip), x0=ptr(x0),
             label=ptr(self.label), random=ptr(self.random), R=self.R, label_out=ptr(label_out), random_out=ptr(random_out),
             stream=stream())

    def tensor(self):
        """The whole set as fp32 [M, C, H, W] on the device: one gather over arange(M)."""
        self._on_gpu("tensor")
        out = torch.empty(self.M, self.C, self.H, self.W, dtype=torch.float32, device=self.device)
        self.gather(torch.arange(self.M, dtype=torch.int64, device=self.device), 0, self.M, out)
        return out

    def means(self, per_channel=False):
        """`mdm_data_means`: fp32 [M, C] means over H W (`per_channel`) or [M, 1] means over C H W, on the device."""
        self._on_gpu("means")
        out = torch.empty(self.M, self.C if per_channel else 1, dtype=torch.float32, device=self.device)
        call("mdm_data_means", src=ptr(self.data), kind=self.kind, img_stride=self.img_stride, M=self.M, C=self.C, H=self.H,
             W=self.W, lut=ptr(self.lut), per_channel=int(bool(per_channel)), out=ptr(out), stream=stream())
        return out


class DeviceLoader:
    """Iterable over a `DeviceDataset`: yields `(x0, label, random)`, all three on the device, one `mdm_data_gather` launch each.

    THE YIELDED TENSORS ARE THE LOADER'S OWN BUFFERS: they are valid until the next batch is fetched, which overwrites them
    (in stream order).  Clone what has to live longer.  After `bind(buffer)` the images are written into `buffer` and `buffer` is
    what is yielded (`Trainer` binds `TrainStep.x0`).

    Order: made on the host once per epoch and uploaded as one int64 vector.  It is, index for index, what
    `torch.utils.data.DataLoader(ds, batch_size, shuffle=shuffle, drop_last=drop_last, generator=generator)` visits, and the
    host generators are left as that loader leaves them: creating the iterator draws the int64 base seed from `generator` (the
    default generator when None); torch's own `RandomSampler` / `BatchSampler` then draw the permutation.

    `world > 1`: rank r takes batches r, r + world, ... of that sequence, and a round of `world` batches is dealt only when it
    is complete (accelerate's `BatchSamplerShard(split_batches=False)` over a `drop_last=True` batch sampler).  Every rank must
    draw the same permutation, i.e. seed its generator alike (upstream seeds every rank with 0); nothing is broadcast.
    `Accelerator.prepare` sets `rank` / `world`.

    `hflip=p`: every image is mirrored along W with probability p -- one `torch.rand(1) < p` per image from the default host
    generator when its batch is fetched, as torchvision's `RandomHorizontalFlip` draws in a loader without workers; the flags
    are uploaded with the batch.  The default 0 draws nothing.  This is an option with torch's semantics, not parity with
    upstream: its own augment branch (mydataset.py:275-276) names an undefined variable and cannot run."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=True, generator=None, hflip=0.0, rank=0, world=1):
        if not isinstance(dataset, DeviceDataset):
            raise TypeError(f"DeviceLoader reads a DeviceDataset, not {type(dataset).__name__}")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size={batch_size}")
        if not 0.0 <= float(hflip) <= 1.0:
            raise ValueError(f"hflip={hflip} is not a probability")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.generator, self.hflip, self.rank, self.world = generator, float(hflip), int(rank), int(world)
        self.sampler = RandomSampler(range(len(dataset)), generator=generator) if self.shuffle else SequentialSampler(range(len(dataset)))
        self.batch_sampler = BatchSampler(self.sampler, self.batch_size, self.drop_last)
        self.x0 = self.label = self.random = None

    def _check_shard(self):
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {self.rank} of world {self.world}")
        if self.world > 1 and not self.drop_last:
            raise ValueError("DeviceLoader: sharding over ranks (world > 1) needs drop_last=True")

    def __len__(self):
        self._check_shard()
        n = len(self.batch_sampler)
        return n if self.world == 1 else n // self.world

    def epoch_indices(self):
        """This rank's batches of one epoch as a host list of index lists; does the epoch's draws."""
        self._check_shard()
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)          # the DataLoader iterator's base seed
        batches = list(self.batch_sampler)
        if self.world == 1:
            return batches
        rounds = len(batches) // self.world
        return [batches[k * self.world + self.rank] for k in range(rounds)]

    def bind(self, x0_buffer):
        """Gather the images into `x0_buffer` ([batch_size, C, H, W] fp32, contiguous, on the data set's device) from now on."""
        d = self.dataset
        want = (self.batch_size, d.C, d.H, d.W)
        if tuple(x0_buffer.shape) != want or x0_buffer.dtype != torch.float32 or not x0_buffer.is_contiguous() or \
                x0_buffer.device != d.data.device:
            raise ValueError(f"DeviceLoader.bind: need a contiguous float32 {want} on {d.data.device}, got {x0_buffer.dtype} "
                             f"{tuple(x0_buffer.shape)} on {x0_buffer.device}")
        self.x0 = x0_buffer
        return self

    def __iter__(self):
        d, B = self.dataset, self.batch_size
        d._on_gpu("DeviceLoader")
        dev = d.data.device
        if self.x0 is None:
            self.x0 = torch.empty(B, d.C, d.H, d.W, dtype=torch.float32, device=dev)
        if self.label is None:
            self.label, self.random = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, d.R, dtype=torch.float32, device=dev)
        batches = self.epoch_indices()
        if not batches:
            return
        index = torch.tensor([i for b in batches for i in b], dtype=torch.int64).to(dev)
        first = 0
        for b in batches:
            n = len(b)
            flip = None
            if self.hflip > 0.0:
                flip = torch.tensor([bool(torch.rand(1) < self.hflip) for _ in range(n)], dtype=torch.uint8).to(dev)
            d.gather(index, first, n, self.x0, flip, self.label, self.random)
            first += n
            yield (self.x0, self.label, self.random) if n == B else (self.x0[:n], self.label[:n], self.random[:n])
