"""Set-level sample quality (include/mdm_moment.h): the first and second moments of a set of feature rows, summed in fp64 on the
device, and the Frechet distance between the two Gaussians that two such sets define.

With pixel rows -- an image batch viewed as rows, a `DeviceDataset` read in place, the 32 x 32 rows of a `NeighborBank` -- this is a
PIXEL-SPACE Frechet distance.  It is NOT FID: FID is this distance on the pool features of an Inception network, which is not part
of this package and is not fetched.  With feature rows from an extractor the caller brings, `SetMoments.update` and
`frechet_distance` are the two calls of FID, and `SetMoments.save` / `load` the stats file FID tools keep for a data set.

Upstream has no counterpart (its FID import is commented out, sampler.py:13, 41-44).

The device work is `mdm_moment_accumulate` (two launches per call, carried across calls, no host read).  The distance is host fp64:
two `numpy.linalg.eigh` calls, which dominate the device work at d = 3072 (measured in DESIGN.md finding 73).
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

MomentPlan = collections.namedtuple("MomentPlan", "tile tiles splits rows_per_split grid lds_bytes ws_bytes")
FrechetResult = collections.namedtuple("FrechetResult", "distance mean_term trace_a trace_b cross_term clipped n_a n_b d rank_deficient")


def moment_plan(R, d):
    """`mdm_moment_plan` and `mdm_moment_ws_bytes` for R rows of d values: host code, no device needed.  -> MomentPlan(tile = the edge
    of a tile of outputs, tiles = those of the upper triangle, splits, rows_per_split, grid = (workgroups of the tile launch, of the
    combining launch), lds_bytes = (of either launch), ws_bytes)."""
    lib = _lib.load()
    tile, splits = _lib.i32(), _lib.i32()
    tiles, rps = _lib.i64(), _lib.i64()
    grid, lds = (_lib.i64 * 2)(), (_lib.i32 * 2)()
    ref = ctypes.byref
    _lib.check(lib.mdm_moment_plan(int(R), int(d), ref(tile), ref(tiles), ref(splits), ref(rps), grid, lds), "mdm_moment_plan")
    return MomentPlan(tile.value, tiles.value, splits.value, rps.value, tuple(grid), tuple(lds), lib.mdm_moment_ws_bytes(int(R), int(d)))


def moment_tile_of(d, tile):
    """`mdm_moment_tile_of`: (I, J), J >= I, the place of tile `tile` of d columns in the upper triangle, as both launches map it."""
    I, J = _lib.i32(), _lib.i32()
    _lib.check(_lib.load().mdm_moment_tile_of(int(d), int(tile), ctypes.byref(I), ctypes.byref(J)), "mdm_moment_tile_of")
    return I.value, J.value


class SetMoments:
    """n, sum = sum_r x_r and outer = sum_r x_r x_r^T of the rows seen so far: `n` a host int, `sum` [d] and `outer` [d, d] fp64
    tensors on `device` (the current GPU by default).  Rows are folded in by `update` / `update_dataset` where they lie, with carry:
    a set streamed in chunks, or a sampler run in rounds, accumulates without its rows ever being together.  Every element stays
    inside gamma(n + splits + calls) sum |x x| of the exact value (mdm_moment.h); `outer` is bit-symmetric."""

    def __init__(self, d, device=None):
        d = int(d)
        if d < 1:
            raise ValueError(f"d: {d}, a positive row length is needed")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:                     # "cuda" is the current GPU: tensors name theirs by index
            device = torch.device("cuda", torch.cuda.current_device())
        self.d, self.n, self.device = d, 0, device
        self._empty = True                                                     # nothing folded in or given yet: the next call overwrites
        self.sum = torch.zeros(d, dtype=torch.float64, device=self.device)
        self.outer = torch.zeros(d, d, dtype=torch.float64, device=self.device)
        self._ws = None

    @classmethod
    def from_arrays(cls, n, sum, outer, device="cpu"):
        """From host arrays (no device is needed with device="cpu"): n rows with these fp64 totals."""
        s, o = np.asarray(sum, np.float64), np.asarray(outer, np.float64)
        if s.ndim != 1 or o.shape != (s.size, s.size):
            raise ValueError(f"outer: shape {o.shape}, {(s.size, s.size)} to go with sum is needed")
        if int(n) < 0:
            raise ValueError(f"n: {n}")
        m = cls(s.size, device)
        m.n, m._empty = int(n), False
        m.sum.copy_(torch.from_numpy(s.copy()))
        m.outer.copy_(torch.from_numpy(o.copy()))
        return m

    @classmethod
    def from_rows(cls, rows, device="cpu"):
        """The host fp64 statement: the moments of a host array [R, d] by numpy (tests and small sets; nothing is launched)."""
        x = np.asarray(rows, np.float64)
        if x.ndim != 2:
            raise ValueError(f"rows: shape {x.shape}, [R, d] is needed")
        return cls.from_arrays(x.shape[0], x.sum(0), x.T @ x, device)

    # ---- the device fold ------------------------------------------------------------------------------------------------
    def _accumulate(self, rows_ptr, kind, lut, row_ld, R):
        if self.device.type != "cuda":
            raise RuntimeError(f"SetMoments: these moments are on {self.device}, mdm_moment_accumulate needs them on a GPU; there is no CPU fallback")
        need = _lib.load().mdm_moment_ws_bytes(int(R), self.d)
        if need < 0:
            _lib.check(-1, "mdm_moment_ws_bytes")
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty(need // 8, dtype=torch.float64, device=self.device)
        call("mdm_moment_accumulate", rows=rows_ptr, kind=kind, lut=ptr(lut), row_ld=int(row_ld), R=int(R), d=self.d, carry=int(not self._empty),
             sum=ptr(self.sum), outer=ptr(self.outer), outer_ld=self.d, ws=ptr(self._ws), ws_bytes=self._ws.numel() * 8, stream=stream())
        self.n += int(R)
        self._empty = False

    def update(self, rows):
        """Fold in fp32 rows on this object's device: [R, ld] with ld >= d, of which the first d values of a row count (the padded
        rows of a `NeighborBank`, a column slice), or an image batch [R, C, H, W] viewed as rows with d = C H W.  Read in place."""
        if not isinstance(rows, torch.Tensor):
            raise TypeError(f"rows: a torch.Tensor is needed, not {type(rows).__name__}")
        if rows.dtype != torch.float32:
            raise TypeError(f"rows: dtype {rows.dtype}, float32 is needed")
        if rows.device != self.device:
            raise ValueError(f"rows: on {rows.device}, the moments are on {self.device}")
        if rows.dim() == 4:
            if not rows.is_contiguous() or rows[0].numel() != self.d:
                raise ValueError(f"rows: image batch {tuple(rows.shape)}, contiguous with C H W = d = {self.d} is needed")
            R, ld = rows.shape[0], self.d
        elif rows.dim() == 2:
            R, ld = rows.shape[0], rows.stride(0)
            if rows.shape[1] < self.d or (rows.shape[1] > 1 and rows.stride(1) != 1) or (R > 1 and ld < rows.shape[1]):
                raise ValueError(f"rows: shape {tuple(rows.shape)} with strides {tuple(rows.stride())}, [R, ld >= d = {self.d}] with unit "
                                 "stride along a row is needed")
            ld = max(ld, rows.shape[1])
        else:
            raise ValueError(f"rows: shape {tuple(rows.shape)}, [R, ld >= d] or an image batch [R, C, H, W] is needed")
        if R == 0:
            return self
        self._accumulate(rows.data_ptr(), 0, None, ld, R)
        return self

    def update_dataset(self, dataset, chunk=4096):
        """Fold in a whole `DeviceDataset` where it is stored -- uint8 through its table or fp32, d = C H W -- `chunk` images per
        call, with carry.  No fp32 copy of a uint8 set ever exists."""
        from .data import DeviceDataset
        if not isinstance(dataset, DeviceDataset):
            raise TypeError(f"dataset: a DeviceDataset is needed, not {type(dataset).__name__}")
        if dataset.data.device != self.device:
            raise ValueError(f"dataset: on {dataset.data.device}, the moments are on {self.device}")
        if dataset.img_stride != self.d:
            raise ValueError(f"dataset: images of C H W = {dataset.img_stride} values, d = {self.d} is needed")
        if int(chunk) < 1:
            raise ValueError(f"chunk: {chunk}")
        step = dataset.data.element_size() * dataset.img_stride
        for first in range(0, dataset.M, int(chunk)):
            self._accumulate(dataset.data.data_ptr() + first * step, dataset.kind, dataset.lut, dataset.img_stride,
                             min(int(chunk), dataset.M - first))
        return self

    # ---- plumbing: fp64 adds in torch -------------------------------------------------------------------------------------
    def merge(self, other):
        """Add the moments of a second object of the same d (moved to this device)."""
        if not isinstance(other, SetMoments) or other.d != self.d:
            raise ValueError(f"other: SetMoments of d = {self.d} is needed")
        self.n += other.n
        self._empty = self._empty and other._empty
        self.sum += other.sum.to(self.device)
        self.outer += other.outer.to(self.device)
        return self

    def all_reduce(self, group=None):
        """Sum over the ranks of `group`: every rank then holds the moments of all rows."""
        import torch.distributed as dist
        n = torch.tensor([self.n], dtype=torch.int64, device=self.device)
        for t in (n, self.sum, self.outer):
            dist.all_reduce(t, group=group)
        self.n = int(n)
        return self

    # ---- host statistics --------------------------------------------------------------------------------------------------
    def mean(self):
        """numpy fp64 [d]: sum / n"""
        if self.n < 1:
            raise ValueError("SetMoments.mean: no rows yet")
        return self.sum.cpu().numpy() / self.n

    def cov(self, ddof=1):
        """numpy fp64 [d, d]: (outer - n mu mu^T) / (n - ddof), `np.cov(rows, rowvar=False, ddof=ddof)`"""
        if self.n - int(ddof) < 1:
            raise ValueError(f"SetMoments.cov: n = {self.n} rows with ddof = {ddof}")
        mu = self.mean()
        return (self.outer.cpu().numpy() - self.n * np.outer(mu, mu)) / (self.n - int(ddof))

    def save(self, path):
        """Write n, sum and outer as an .npz: the stats file of a data set."""
        with open(path, "wb") as f:
            np.savez(f, n=np.int64(self.n), sum=self.sum.cpu().numpy(), outer=self.outer.cpu().numpy())

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path) as z:
            return cls.from_arrays(int(z["n"]), z["sum"], z["outer"], device)


def _sqrt_psd(S):
    """S^{1/2} of a symmetric matrix, its negative eigenvalues taken as 0"""
    w, V = np.linalg.eigh(S)
    return (V * np.sqrt(np.maximum(w, 0.0))) @ V.T


def frechet_distance(a, b):
    """The Frechet distance between N(mu_a, S_a) and N(mu_b, S_b) of two `SetMoments` (S = cov(ddof=1)):
        |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^{1/2} S_b S_a^{1/2})^{1/2}
    in host fp64, in the symmetric form: S_a = V diag(w) V^T, M = S_a^{1/2} S_b S_a^{1/2} symmetrised, cross = sum sqrt(max(eig(M), 0))
    -- the eigenvalues of M are those of S_a S_b, whose square root pytorch-fid takes by scipy.linalg.sqrtm.  -> FrechetResult(distance,
    mean_term, trace_a, trace_b, cross_term, clipped = the negative eigenvalue mass of M that was set to 0, n_a, n_b, d,
    rank_deficient).

    On pixel rows this is a pixel-space distance, NOT FID; on the features of an extractor the caller brings it is FID.
    `rank_deficient` is min(n_a, n_b) <= d: a covariance of fewer rows than dimensions is singular.  Nothing is raised; the number is
    defined but biased upward (the traces count directions the cross term cannot see), so compare it only at equal n.  The
    n-dimensional form for n < d is not implemented.  The two `eigh` calls dominate (DESIGN.md finding 73)."""
    for name, m in (("a", a), ("b", b)):
        if not isinstance(m, SetMoments):
            raise TypeError(f"{name}: a SetMoments is needed, not {type(m).__name__}")
        if m.n < 2:
            raise ValueError(f"{name}: n = {m.n} rows, a covariance needs 2")
    if a.d != b.d:
        raise ValueError(f"b: d = {b.d}, a has d = {a.d}")
    mu_a, mu_b, S_a, S_b = a.mean(), b.mean(), a.cov(), b.cov()
    root = _sqrt_psd(S_a)
    M = root @ S_b @ root
    ev = np.linalg.eigvalsh((M + M.T) * 0.5)
    cross = float(np.sqrt(np.maximum(ev, 0.0)).sum())
    diff = mu_a - mu_b
    mean_term, tr_a, tr_b = float(diff @ diff), float(np.trace(S_a)), float(np.trace(S_b))
    return FrechetResult(mean_term + tr_a + tr_b - 2.0 * cross, mean_term, tr_a, tr_b, cross, float(-ev[ev < 0].sum()), a.n, b.n, a.d,
                         min(a.n, b.n) <= a.d)


def dataset_moments(dataset):
    """the pixel moments of a `DeviceDataset` on a GPU, read in place once and kept on the data set object"""
    from .data import DeviceDataset
    if not isinstance(dataset, DeviceDataset) or dataset.data.device.type != "cuda":
        raise TypeError("reference: the default reference is the moments of a DeviceDataset on a GPU; this Sampler's data set is "
                        f"{type(dataset).__name__}")
    m = getattr(dataset, "_set_moments", None)
    if m is None:
        m = dataset._set_moments = SetMoments(dataset.img_stride, dataset.data.device).update_dataset(dataset)
    return m
