"""Image quality on the device (include/mdm_metric.h): MSE, PSNR and SSIM of samples against held-out originals, over the whole image
and over the hole of an inpainting run.  A batch or a whole sampler history is reduced where it lives to eight numbers per image; no
image and no number comes to the host unless the caller reads the result.

Upstream has no counterpart (its FID import is commented out, sampler.py:13, 41-44).  The SSIM is Wang et al. 2004 with an 11 x 11
Gaussian window of sigma 1.5 over the valid region -- the defaults of torchmetrics' structural_similarity_index_measure and of skimage's
structural_similarity(gaussian_weights=True, use_sample_covariance=False); parity with either is UNPINNED, neither was available to
compare against.
"""
from __future__ import annotations

import collections
import ctypes

import torch

from . import _lib
from ._lib import call, ptr, stream

ImageMetrics = collections.namedtuple("ImageMetrics", "mse psnr ssim mse_hole psnr_hole ssim_hole hole_count hole_windows")
MetricPlan = collections.namedtuple("MetricPlan", "tile_h tile_w tiles_y tiles_x grid lds_bytes window ws_bytes")


def plan(R, C, H, W):
    """`mdm_metric_plan` and `mdm_metric_ws_bytes` for R rows of [C, H, W]: host code, no device needed.  -> MetricPlan(tile_h, tile_w,
    tiles_y, tiles_x, grid = (workgroups of the tile launch, of the combining launch), lds_bytes, window = the 11 float weights,
    ws_bytes)."""
    lib = _lib.load()
    th, tw, ty, tx, lds = (_lib.i32() for _ in range(5))
    grid, win = (_lib.i64 * 2)(), (_lib.f32 * 11)()
    ref = ctypes.byref
    _lib.check(lib.mdm_metric_plan(R, C, H, W, ref(th), ref(tw), ref(ty), ref(tx), grid, ref(lds), win), "mdm_metric_plan")
    return MetricPlan(th.value, tw.value, ty.value, tx.value, tuple(grid), lds.value, tuple(win), lib.mdm_metric_ws_bytes(R, C, H, W))


def _check(name, t, dev=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch.Tensor is needed, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: dtype {t.dtype}, float32 is needed")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name}: on {t.device}, pred is on {dev}")


def image_metrics(pred, truth, keep=None, data_range=2.0, clamp=(-1.0, 1.0)):
    """-> ImageMetrics(mse, psnr, ssim, mse_hole, psnr_hole, ssim_hole, hole_count, hole_windows) of device tensors with `pred`'s
    leading shape.  `pred` [N, C, H, W] or a history [T + 1, N, C, H, W] (read in place), `truth` [N, C, H, W], `keep` None or
    [N, 1 or C, H, W]: an element is HOLE where keep == 0, everything with keep None; all fp32, contiguous, on one device.
    `pred` is clamped to `clamp` first (what save_image shows; None: as it is), `truth` never.  The slots are those of
    include/mdm_metric.h: `*_hole` over the hole elements / the SSIM positions centred on one, NaN where there is none.
    Two launches (tiles, then one wave per image adding them in a fixed order) and no host read."""
    _check("pred", pred)
    _check("truth", truth, pred.device)
    if pred.dim() not in (4, 5) or truth.dim() != 4 or tuple(pred.shape[-4:]) != tuple(truth.shape):
        raise ValueError(f"pred: shape {tuple(pred.shape)}, [T + 1,] {tuple(truth.shape)} like truth is needed")
    N, Ch, H, W = truth.shape
    if keep is not None:
        _check("keep", keep, pred.device)
        if keep.dim() != 4 or (keep.shape[0], *keep.shape[2:]) != (N, H, W) or keep.shape[1] not in (1, Ch):
            raise ValueError(f"keep: shape {tuple(keep.shape)}, {(N, 1, H, W)} or {(N, Ch, H, W)} is needed")
    lo, hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
    if clamp is not None and not lo < hi:
        raise ValueError(f"clamp: {clamp!r}, (lo, hi) with lo < hi or None is needed")
    lead = tuple(pred.shape[:-3])
    R = 1
    for s in lead:
        R *= s
    need = _lib.load().mdm_metric_ws_bytes(R, Ch, H, W)
    if need < 0:
        _lib.check(-1, "mdm_metric_ws_bytes")
    ws = torch.empty(need // 8, dtype=torch.float64, device=pred.device)
    out = torch.empty(R, 8, dtype=torch.float32, device=pred.device)
    call("mdm_metric_image", pred=ptr(pred), truth=ptr(truth), keep=ptr(keep), Ck=keep.shape[1] if keep is not None else 0, R=R, N=N,
         C=Ch, H=H, W=W, clamp_lo=lo, clamp_hi=hi, data_range=float(data_range), ws=ptr(ws), ws_bytes=need, out=ptr(out), stream=stream())
    return ImageMetrics(*(out[:, k].reshape(lead) for k in range(8)))


def mean_fill_baseline(truth, keep, mean_area="image-wise"):
    """keep ? truth : the mean of the given values, built on the device (`mdm_inpaint_start`): the image a "known_mean" run starts
    from with its given pixels put back, and the trivial completion any quality number is to be read against.  The mean is taken
    per image ('image-wise') or per channel ('channel-wise'), in fp32 as mdm_inpaint.h states it; where nothing is given it is 0."""
    _check("truth", truth)
    _check("keep", keep, truth.device)
    if mean_area not in ("image-wise", "channel-wise"):
        raise ValueError(f"mean_area={mean_area!r}: 'image-wise' or 'channel-wise'")
    N, Ch, H, W = truth.shape
    if keep.dim() != 4 or (keep.shape[0], *keep.shape[2:]) != (N, H, W) or keep.shape[1] not in (1, Ch):
        raise ValueError(f"keep: shape {tuple(keep.shape)}, {(N, 1, H, W)} or {(N, Ch, H, W)} is needed")
    out = torch.empty_like(truth)
    fallback = torch.zeros(N, Ch, device=truth.device)
    call("mdm_inpaint_start", known=ptr(truth), keep=ptr(keep), keep_C=keep.shape[1], fallback=ptr(fallback),
         per_channel=int(mean_area == "channel-wise"), N=N, C=Ch, HW=H * W, x_start=ptr(out), mu=None, unknown=None, stream=stream())
    return out
