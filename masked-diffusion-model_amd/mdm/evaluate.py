"""Evaluation caller: what runs right after the sampler -- same names and semantics as the reference.

Mirrors reference tester.py (`Tester.train` :57-134: sample with the EMA weights until `data_subset_num` unique images
exist; `remove_duplicates_in_batches` :148-160, `remove_duplicates_across_batches` :163-183, `get_nearest_neighbor_idx`
:186-201, `_compute_similarity` :140-145), sampler.py `get_nearest_neighbor` (:487-518), utils/datautils.py `normalize01`
(:211-222) and the data-mean histogram that feeds `sample_latent_shape='data'` (main_train_masked.py:60-87).

The reference compares images one pair at a time in Python loops (B x M cosine similarities, each its own kernel launch
and host sync).  Here every comparison of a batch is ONE fp32 contraction on the GPU -- unit-length rows (mdm_unit_rows)
times unit-length rows (mdm_gemm, exact-fp32 MFMA) -- and the greedy keep/drop decisions, which depend on the order of the
images, walk the resulting matrix on the host in the reference's order.  Image grids / plots are out of scope.

`NeighborBank` serves every nearest-neighbour call (include/mdm_neighbor.h): the data set's unit-length feature rows -- 32 x 32 after
normalize01 for `Sampler.get_nearest_neighbor`, full resolution for `Tester` -- are built by `mdm_nn_rows` straight from the
`DeviceDataset` storage, uint8 or fp32 as stored, and searched chunk by chunk by `mdm_nn_col_argmax`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import F32, call, ptr, stream

COSINE_TH = 0.9          # tester.py:54


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("mdm.evaluate needs a GPU and libmdm_hip.so; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def normalize01(data):
    """Per-image min-max normalisation, NaN -> 0 (utils/datautils.py:211-222)."""
    x = data.to(_dev(), torch.float32).contiguous()
    n = x.shape[0]
    y = torch.empty_like(x)
    call("mdm_normalize01", ptr(x), ptr(y), n, x.numel() // n, stream())
    return y


def cosine_similarity_matrix(source, target):
    """-> S[M][B], S[m][b] = cos(target[m], source[b]) over the flattened images (`_compute_similarity`, tester.py:140-145).
    B and M are padded to multiples of 4 / kept as they are by zero rows (dropped again on return)."""
    dev = _dev()
    src = source.to(dev, torch.float32).reshape(source.shape[0], -1)
    tgt = target.to(dev, torch.float32).reshape(target.shape[0], -1)
    B, D = src.shape
    M = tgt.shape[0]
    assert tgt.shape[1] == D
    Dp, Bp = (D + 3) // 4 * 4, (B + 3) // 4 * 4
    a = torch.zeros(M, Dp, device=dev)
    b = torch.zeros(Bp, Dp, device=dev)
    a[:, :D] = tgt
    b[:B, :D] = src
    au, bu = torch.empty_like(a), torch.empty_like(b)
    call("mdm_unit_rows", ptr(a), ptr(au), M, Dp, 1e-8, stream())
    call("mdm_unit_rows", ptr(b), ptr(bu), Bp, Dp, 1e-8, stream())
    S = torch.empty(M, Bp, device=dev)
    ops.matmul(F32, 0, M, Bp, Dp, au, Dp, bu, Dp, S, Bp)
    return S[:, :B]


def col_argmax(S):
    """(values, indices) of the column maxima of S[M][B]; ties -> the first row, like `score.max(dim=0)`."""
    S = S.contiguous()
    M, B = S.shape
    val = torch.empty(B, device=S.device)
    idx = torch.empty(B, dtype=torch.int64, device=S.device)
    call("mdm_col_argmax", ptr(S), M, B, ptr(val), ptr(idx), stream())
    return val, idx


def _dataset_tensor(dataset):
    if torch.is_tensor(dataset):
        return dataset
    return torch.stack([dataset[i][0] for i in range(len(dataset))])


def nn_plan(n_in, n_out, antialias):
    """(first [n_out] int32, count [n_out] int32, weight [n_out][taps] float32, taps): the one-axis tap table of
    `F.interpolate(mode="bilinear", align_corners=False, antialias=antialias)` as `mdm_nn_plan` states it (host arrays)."""
    lib = _lib.load()
    taps = lib.mdm_nn_plan(int(n_in), int(n_out), int(bool(antialias)), None, None, None, 0)
    if taps < 1:
        _lib.check(taps, "mdm_nn_plan")
    first, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    weight = np.zeros((n_out, taps), np.float32)
    got = lib.mdm_nn_plan(int(n_in), int(n_out), int(bool(antialias)), first.ctypes.data, count.ctypes.data, weight.ctypes.data, taps)
    if got != taps:
        _lib.check(-1, "mdm_nn_plan")
    return first, count, weight, taps


def neighbor_flip_rows(M, B):
    """The draws of upstream's `RandomHorizontalFlip()` over a `DataLoader(dataset, batch_size=B, shuffle=False)` pass
    (sampler.py:491-492, 504): the transform sees each batch as ONE tensor, so it is one `torch.rand(1) < 0.5` from the default host
    generator per batch, in data order.  -> uint8 [M] on the host: 1 on the rows of the batches that flip."""
    rows = torch.zeros(int(M), dtype=torch.uint8)
    for i in range(0, int(M), int(B)):
        if bool(torch.rand(1) < 0.5):
            rows[i:i + int(B)] = 1
    return rows


def _as_device_dataset(dataset):
    """`dataset` as a `DeviceDataset` on the GPU; a tensor or a map-style set is uploaded once (no draw from a host generator)."""
    from .data import DeviceDataset
    if isinstance(dataset, DeviceDataset):
        if dataset.data.device.type != "cuda":
            raise TypeError(f"NeighborBank: the data set is on {dataset.data.device}, the kernels of mdm_neighbor.h need it on a GPU")
        return dataset
    data = _dataset_tensor(dataset)
    if data.dtype != torch.uint8:
        data = data.to(torch.float32)
    return DeviceDataset(data, random=torch.zeros(data.shape[0], 1), device=_dev())


class NeighborBank:
    """The unit-length feature rows of a data set, and every nearest-neighbour query against them.

    `dataset`: a `DeviceDataset`, a tensor [M, C, H, W] or a map-style set (the last two are uploaded once).  A row is the image
    `normalize01`-ed (`normalize`), resized to `size` x `size` by the tap tables of `F.interpolate(mode="bilinear", antialias=...)`
    -- torchvision's tensor `Resize` -- or kept at full resolution (`size=None`, `Tester`'s comparison), and divided by its norm:
    one `mdm_nn_rows` launch per `chunk` images, reading the storage as it is (uint8 through the data set's table).  The rows stay
    for later queries when M x row_ld x 4 <= `cache_bytes`; otherwise every query rebuilds them chunk by chunk and one chunk of rows
    is all that is ever live.  Source images go through the same kernel (kind 0, not normalised, as upstream leaves them); a
    similarity is `ops.matmul` per chunk, the search `mdm_nn_col_argmax` with carry."""

    EPS = 1e-8            # torch.nn.functional.cosine_similarity's

    def __init__(self, dataset, size=32, antialias=True, normalize=True, chunk=4096, cache_bytes=1 << 30):
        self.dataset = d = _as_device_dataset(dataset)
        self.size, self.antialias, self.normalize = (None if size is None else int(size)), bool(antialias), bool(normalize)
        if self.size is not None and self.size < 1:
            raise ValueError(f"NeighborBank: size={size}")
        self.chunk = max(1, min(int(chunk), d.M))
        self.D = d.C * (self.size ** 2 if self.size else d.H * d.W)
        self.row_ld = (self.D + 3) // 4 * 4
        self._tables = {}
        self.cached = d.M * self.row_ld * 4 <= int(cache_bytes)
        self.rows = None
        if self.cached:
            self.rows = torch.empty(d.M, self.row_ld, dtype=torch.float32, device=d.device)
            for first in range(0, d.M, self.chunk):
                self._data_rows(first, min(self.chunk, d.M - first), self.rows[first:])
        else:
            self._chunk_rows = torch.empty(self.chunk, self.row_ld, dtype=torch.float32, device=d.device)

    def _axis(self, n_in):
        """the device copy of the tap table n_in -> size: (first, count, weight, taps)"""
        if n_in not in self._tables:
            first, count, weight, taps = nn_plan(n_in, self.size, self.antialias)
            dev = self.dataset.device
            self._tables[n_in] = (torch.from_numpy(first).to(dev), torch.from_numpy(count).to(dev), torch.from_numpy(weight).to(dev), taps)
        return self._tables[n_in]

    def _launch(self, src, kind, img_stride, M, C, H, W, lut, first, R, normalize, flip, out):
        S = self.size or 0
        (hf, hc, hw, ht), (vf, vc, vw, vt) = (self._axis(W), self._axis(H)) if S else ((None, None, None, 0),) * 2
        call("mdm_nn_rows", src=ptr(src), kind=kind, img_stride=img_stride, M=M, C=C, H=H, W=W, lut=ptr(lut), first=int(first), R=int(R),
             normalize=int(normalize), flip=int(flip), S=S, hfirst=ptr(hf), hcount=ptr(hc), hweight=ptr(hw), htaps=ht,
             vfirst=ptr(vf), vcount=ptr(vc), vweight=ptr(vw), vtaps=vt, eps=self.EPS, rows=ptr(out), row_ld=self.row_ld, stream=stream())

    def _data_rows(self, first, R, out):
        d = self.dataset
        self._launch(d.data, d.kind, d.img_stride, d.M, d.C, d.H, d.W, d.lut, first, R, self.normalize, False, out)

    def _chunks(self):
        """(first, R, rows of the images [first, first + R)) over the set: slices of the kept rows, or the one chunk buffer rebuilt"""
        d = self.dataset
        for first in range(0, d.M, self.chunk):
            R = min(self.chunk, d.M - first)
            if self.cached:
                yield first, R, self.rows[first:first + R]
            else:
                self._data_rows(first, R, self._chunk_rows)
                yield first, R, self._chunk_rows

    def source_rows(self, source, flip=False):
        """-> (rows [Bp][row_ld] with Bp = B padded to a multiple of 4 by zero rows, B): the unit rows of the source images, as
        they are (upstream does not normalise the source), mirrored along W with `flip`"""
        d = self.dataset
        src = source.to(d.device, torch.float32).contiguous()
        if src.dim() != 4 or src.shape[1] != d.C or (not self.size and tuple(src.shape[2:]) != (d.H, d.W)):
            raise ValueError(f"NeighborBank: source {tuple(source.shape)} does not match the data set's images {(d.C, d.H, d.W)}")
        B, C, H, W = (int(v) for v in src.shape)
        out = torch.zeros((B + 3) // 4 * 4, self.row_ld, dtype=torch.float32, device=d.device)
        self._launch(src, 0, C * H * W, B, C, H, W, None, 0, B, False, flip, out)
        return out, B

    def similarity(self, source, flip=False):
        """S [M][B], S[m][b] = cos(row of data image m, row of source[b]) (`_compute_similarity`, sampler.py:521-526); `flip`: against
        the mirrored source -- the similarity with the mirrored data up to rounding, the tables being symmetric"""
        d = self.dataset
        b, B = self.source_rows(source, flip)
        Bp = b.shape[0]
        S = torch.empty(d.M, Bp, dtype=torch.float32, device=d.device)
        for first, R, rows in self._chunks():
            ops.matmul(F32, 0, R, Bp, self.row_ld, rows, self.row_ld, b, self.row_ld, S[first:], Bp)
        return S[:, :B]

    def nearest_idx(self, source, augment_rows=None, with_val=False):
        """int64 [B] on the device: the data image with the largest similarity to each source image, `score.max(dim=0)` of
        sampler.py:512.  `augment_rows` (uint8 [M], see `neighbor_flip_rows`): the rows whose score is the larger of the similarity
        and the similarity with the mirrored image (sampler.py:503-508)."""
        d = self.dataset
        b, B = self.source_rows(source)
        Bp = b.shape[0]
        aug = b_aug = S_aug = None
        if augment_rows is not None:
            aug = torch.as_tensor(augment_rows).to(torch.uint8).reshape(-1).to(d.device)
            if aug.numel() != d.M:
                raise ValueError(f"NeighborBank: augment_rows has {aug.numel()} entries for {d.M} images")
            b_aug = self.source_rows(source, flip=True)[0]
            S_aug = torch.empty(self.chunk, Bp, dtype=torch.float32, device=d.device)
        S = torch.empty(self.chunk, Bp, dtype=torch.float32, device=d.device)
        val = torch.empty(B, dtype=torch.float32, device=d.device)
        idx = torch.empty(B, dtype=torch.int64, device=d.device)
        for first, R, rows in self._chunks():
            ops.matmul(F32, 0, R, Bp, self.row_ld, rows, self.row_ld, b, self.row_ld, S, Bp)
            if aug is not None:
                ops.matmul(F32, 0, R, Bp, self.row_ld, rows, self.row_ld, b_aug, self.row_ld, S_aug, Bp)
            call("mdm_nn_col_argmax", S=ptr(S), S_aug=ptr(S_aug), row_aug=None if aug is None else aug.data_ptr() + first, M=R, B=B,
                 ld=Bp, row0=first, carry=int(first > 0), val=ptr(val), idx=ptr(idx), stream=stream())
        return (val, idx) if with_val else idx

    def nearest(self, source, augment_rows=None):
        """fp32 [B, C, H, W] on the device: the stored (un-normalised) nearest data images, one `mdm_data_gather`"""
        d = self.dataset
        idx = self.nearest_idx(source, augment_rows)
        out = torch.empty(idx.numel(), d.C, d.H, d.W, dtype=torch.float32, device=d.device)
        d.gather(idx, 0, idx.numel(), out)
        return out

    def moments(self):
        """The fp64 moments of the bank's rows (mdm.moments.SetMoments, include/mdm_moment.h), streamed through `_chunks()` -- an
        uncached bank folds one rebuilt chunk at a time -- made once and kept on the bank."""
        from .moments import SetMoments
        if getattr(self, "_moments", None) is None:
            m = SetMoments(self.D, self.dataset.device)
            for first, R, rows in self._chunks():
                m.update(rows[:R])
            self._moments = m
        return self._moments

    def source_moments(self, source, into=None):
        """Fold the rows of the source images [B, C, H, W] into `into` (a new `SetMoments` when None) and return it.  The source goes
        through the SAME map as the data -- the bank's `normalize`, `size` and `antialias` -- because a set distance needs both
        sides in one feature space.  (`source_rows`, which leaves the source un-normalised as upstream does, serves the search.)"""
        from .moments import SetMoments
        d = self.dataset
        if not isinstance(source, torch.Tensor) or source.dim() != 4 or source.shape[1] != d.C or \
                (not self.size and tuple(source.shape[2:]) != (d.H, d.W)):
            raise ValueError(f"source: {tuple(getattr(source, 'shape', ()))} does not match the data set's images {(d.C, d.H, d.W)}")
        if into is None:
            into = SetMoments(self.D, d.device)
        elif not isinstance(into, SetMoments) or into.d != self.D:
            raise ValueError(f"into: a SetMoments of d = {self.D} is needed")
        src = source.to(d.device, torch.float32).contiguous()
        B, C, H, W = (int(v) for v in src.shape)
        out = torch.zeros(B, self.row_ld, dtype=torch.float32, device=d.device)
        self._launch(src, 0, C * H * W, B, C, H, W, None, 0, B, self.normalize, False, out)
        return into.update(out)


def _full_bank(dataset):
    """the full-resolution bank of a `DeviceDataset` on a GPU, made once and kept on the data set object; None for anything else"""
    from .data import DeviceDataset
    if not isinstance(dataset, DeviceDataset) or dataset.data.device.type != "cuda":
        return None
    bank = getattr(dataset, "_nn_bank_full", None)
    if bank is None:
        bank = dataset._nn_bank_full = NeighborBank(dataset, size=None)
    return bank


def get_nearest_neighbor_idx(source, dataset):
    """Index of the data image with the largest cosine similarity to each source image; data images are
    normalize01-ed first (tester.py:186-201).  A `DeviceDataset` on a GPU is searched through its full-resolution `NeighborBank`,
    made once and kept on the data set: nothing of the set is copied per call."""
    bank = _full_bank(dataset)
    if bank is not None:
        return bank.nearest_idx(source)
    data = normalize01(_dataset_tensor(dataset))
    return col_argmax(cosine_similarity_matrix(source, data))[1]


def get_nearest_neighbor(source, dataset):
    """The nearest data image (un-normalised, as stored) for every source image, compared at full resolution as
    `get_nearest_neighbor_idx` compares.  (Upstream's `Sampler.get_nearest_neighbor`, which compares 32 x 32 resizes, is
    `mdm.Sampler.get_nearest_neighbor`.)"""
    bank = _full_bank(dataset)
    if bank is not None:
        return bank.nearest(source).to(source.device)
    data = _dataset_tensor(dataset)
    idx = get_nearest_neighbor_idx(source, data)
    return data.to(source.device)[idx.to(source.device)]


def get_similar_neighbor(generated, img_set, idx, th=COSINE_TH):
    """tester.py:209-223: generated image i joins `img_set[idx[i]]` -- the list of its nearest data image -- unless a member of that
    list, an image added earlier in this call included, is more similar to it than `th`.  One similarity matrix per call (the
    members of the touched lists and the generated images against the generated images), then a host walk in upstream's order."""
    n = len(generated)
    if n == 0:
        return img_set
    idx = [int(i) for i in idx]
    members, stored = {}, []
    for k in sorted(set(idx)):
        members[k] = list(range(len(stored), len(stored) + img_set[k].shape[0]))
        stored.extend(img_set[k][j] for j in range(img_set[k].shape[0]))
    base = len(stored)
    gen = generated.cpu()
    target = torch.cat((torch.stack(stored).to(gen.dtype), gen), dim=0) if stored else gen
    S = cosine_similarity_matrix(generated, target).cpu()                # [base + n][n]
    added = {k: [] for k in members}
    for i in range(n):
        k = idx[i]
        if not any(bool(S[m, i] > th) for m in members[k]):
            members[k].append(base + i)
            added[k].append(i)
    for k, rows in added.items():
        if rows:
            img_set[k] = torch.cat((img_set[k], gen[rows]), dim=0)
    return img_set


def remove_duplicates_in_batches(current_batch, th=COSINE_TH):
    """Greedy, in order: an image is kept unless some ALREADY KEPT image of the batch has cosine similarity >= th
    (tester.py:148-160)."""
    S = cosine_similarity_matrix(current_batch, current_batch).cpu()
    kept = [0]
    for i in range(1, current_batch.shape[0]):
        if not bool((S[kept, i] >= th).any()):
            kept.append(i)
    return current_batch[kept]


def remove_duplicates_across_batches(unique_in_batch, previous_images, th=COSINE_TH):
    """Keep the images whose similarity to EVERY previously collected image is <= th (tester.py:163-183)."""
    if unique_in_batch.shape[0] == 0 or previous_images.shape[0] == 0:
        return unique_in_batch
    S = cosine_similarity_matrix(unique_in_batch, previous_images)        # [M prev][B]
    keep = ~(S > th).any(dim=0)
    return unique_in_batch[keep.to(unique_in_batch.device)]


def data_mean_histogram(dataset, args):
    """[hist_shape, hist_bin_edges, hist_mean_cum_sum] of the per-image (image-wise) or per-channel (channel-wise) means
    of the data set, `sample_num` bins per axis (main_train_masked.py:60-87); what `Sampler(dataset, args, Scheduler,
    dataset_hist)` takes for `sample_latent_shape='data'`.  Host arithmetic like upstream (once per run)."""
    if args.sample_latent_shape.lower() != "data":
        return [None, None, None]
    if args.mean_area not in ("channel-wise", "image-wise"):
        raise UnboundLocalError("mean_area")
    from .data import DeviceDataset
    if isinstance(dataset, DeviceDataset):         # the means are taken where the data is (mdm_data_means); only [M, d] comes back
        means = dataset.means(per_channel=args.mean_area == "channel-wise").cpu()
    else:
        data = _dataset_tensor(dataset).to("cpu", torch.float32)
        means = data.mean(dim=[2, 3]) if args.mean_area == "channel-wise" else data.mean(dim=[1, 2, 3]).unsqueeze(-1)
    hist, edges = torch.histogramdd(means, bins=args.sample_num, density=True)
    shape = hist.shape
    hist = torch.ravel(hist)
    hist = hist / torch.sum(hist)
    return [shape, edges, torch.cumsum(hist, dim=0)]


class Tester:
    """tester.py `Tester`: sample with the EMA weights until `args.data_subset_num` mutually distinct images exist."""

    def __init__(self, args, dataloader, dataset, model, ema_model, optimizer, lr_scheduler, accelerator):
        from .sampler import Sampler
        from .scheduler import Scheduler
        self.args, self.dataloader, self.dataset = args, dataloader, dataset
        self.model, self.ema_model, self.accelerator = model, ema_model, accelerator
        self.Scheduler = Scheduler(args, device=model.device)
        self.Sampler = Sampler(self.dataset, self.args, self.Scheduler, getattr(args, "dataset_hist", [None] * 3))
        self.cosine_similarity_th = COSINE_TH
        self.timesteps_used_epoch = None

    def train(self, epoch_start, epoch_length, resume_step, global_step, dirs, visualizer, max_rounds=1000):
        a = self.args
        a.updated_ddpm_num_steps = self.Scheduler.update_ddpm_num_steps(a.ddpm_num_steps)
        self.timesteps_used_epoch = self.Scheduler.get_timesteps_epoch(1, 10)          # tester.py:61
        total = torch.empty(0, a.out_channel, a.data_size, a.data_size)
        self.num_total_unique_images = []
        self.nearest_idx = []
        n_sets = len(self.dataset) if self.dataset is not None else a.data_subset_num
        self.img_set = [torch.empty(0, a.out_channel, a.data_size, a.data_size) for _ in range(n_sets)]          # tester.py:83
        for _ in range(max_rounds):
            if len(total) >= a.data_subset_num:
                break
            self.ema_model.store(None)
            self.ema_model.copy_to(None)
            # (the plan is fetched behind copy_to: a bf16 model's sampling plan copies the weights it finds; see Trainer)
            net = self.model.sampling_plan(self.Sampler.local_sample_num(), getattr(a, "sample_precision", "f32_split")).eval()
            generated, _ = self.Sampler.sample(net, self.timesteps_used_epoch)
            self.ema_model.restore(None)
            uniq = remove_duplicates_in_batches(generated, self.cosine_similarity_th)
            uniq = remove_duplicates_across_batches(uniq, total, self.cosine_similarity_th)
            total = torch.cat((total, uniq.cpu()), dim=0)
            self.num_total_unique_images.append(total.shape[0])
            if uniq.shape[0] and self.dataset is not None:
                self.nearest_idx.append(get_nearest_neighbor_idx(uniq, self.dataset).cpu())
                self.img_set = get_similar_neighbor(uniq.cpu(), self.img_set, self.nearest_idx[-1], self.cosine_similarity_th)   # :119-120
        self.model.train()
        self.total_unique_images = total
        return total
