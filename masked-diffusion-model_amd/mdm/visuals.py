"""Image grids built on the device (include/mdm_vis.h, csrc/vis.hip).

Upstream draws a batch with `normalize01` / `normalize01_global` (utils/datautils.py:211-229), torchvision's `make_grid` and
`save_image` (sampler.py:369-387): three or four torch passes, K narrow copies and a float -> uint8 conversion on the host.  Here a
grid is one range launch (the min / max the normalisation needs) and one grid launch that normalises, places and quantises; what
crosses to the host is the uint8 image.  Nothing in here synchronises with the host or copies the images.

An image batch is a float32 device tensor [K, C, H, W] whose images are contiguous; the images themselves may lie any distance
apart (`x.stride(0)`), so `hist[1:, n]` of a time-major sampler history [T+1, N, C, H, W] is read in place.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call, ptr, stream

MODES = {None: 0, "image": 1, "global": 2}
_scratch = {}


def grid_shape(K, C_, H, W, nrow, padding=2):
    """(Cg, Hg, Wg) of the grid of K images [C, H, W] (mdm_vis_grid_shape; host only)."""
    out = (_lib.i32 * 3)()
    _lib.check(_lib.load().mdm_vis_grid_shape(K, C_, H, W, nrow, padding, out), "mdm_vis_grid_shape")
    return tuple(out)


def _images(x):
    """-> (x, image stride in elements): a float32 device batch [K, C, H, W] as the kernels read it -- the data pointer of the view
    and the distance between its images."""
    if x.dim() != 4:
        raise ValueError(f"an image batch is [K, C, H, W], not {tuple(x.shape)}")
    if x.dtype != torch.float32 or not x.is_cuda:
        raise TypeError(f"an image batch is a float32 device tensor, not {x.dtype} on {x.device}")
    E = x[0].numel() if x.shape[0] else 0
    if x.shape[0] == 0 or E == 0:
        raise ValueError(f"an empty image batch {tuple(x.shape)}")
    if not x[0].is_contiguous() or (x.shape[0] > 1 and x.stride(0) < E):
        raise ValueError("the images of a batch must be contiguous and must not overlap (strides %s)" % (tuple(x.stride()),))
    return x, (x.stride(0) if x.shape[0] > 1 else E)


def _range_scratch(dev):
    """The four words a global range counts in: zeroed once, left zero by the kernel; one block per (device, stream)."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _scratch:
        _scratch[key] = torch.zeros(4, dtype=torch.float32, device=dev)
    return _scratch[key]


def image_range(x, per_image=True):
    """{min, max} of every image -> [K, 2], or of the whole batch -> [1, 2] (mdm_vis_range; torch's amin / amax: a NaN makes both
    words NaN).  One launch."""
    x, stride = _images(x)
    K, E = x.shape[0], x[0].numel()
    lohi = torch.empty(K if per_image else 1, 2, dtype=torch.float32, device=x.device)
    call("mdm_vis_range", ptr(x), stride, K, E, 0 if per_image else 1, ptr(lohi), None if per_image else ptr(_range_scratch(x.device)),
         stream())
    return lohi


def make_grid(x, nrow=8, normalization=None, padding=2, pad_value=0.0, out="f32"):
    """torchvision's `make_grid(x, nrow, padding, pad_value, normalize=False)` of upstream's `normalize01(x)` ('image'),
    `normalize01_global(x)` ('global') or x itself (None).  out: 'f32' -> the grid [Cg, Hg, Wg] float32, 'u8' -> [Hg, Wg, Cg] uint8
    as `save_image` quantises it, 'both' -> (f32, u8); all on the device.  One range launch (none for None) and one grid launch."""
    if normalization not in MODES:
        raise ValueError(f"normalization={normalization!r} is not None, 'image' or 'global'")
    if out not in ("f32", "u8", "both"):
        raise ValueError(f"out={out!r} is not 'f32', 'u8' or 'both'")
    x, stride = _images(x)
    K, Cn, H, W = x.shape
    Cg, Hg, Wg = grid_shape(K, Cn, H, W, nrow, padding)
    mode = MODES[normalization]
    lohi = image_range(x, per_image=mode == 1) if mode else None
    f = torch.empty(Cg, Hg, Wg, dtype=torch.float32, device=x.device) if out != "u8" else None
    u = torch.empty(Hg, Wg, Cg, dtype=torch.uint8, device=x.device) if out != "f32" else None
    call("mdm_vis_grid", x=ptr(x), img_stride=stride, K=K, C=Cn, H=H, W=W, lohi=ptr(lohi), mode=mode, nrow=nrow, padding=padding,
         pad_value=pad_value, grid_f32=ptr(f), grid_u8=ptr(u), stream=stream())
    return (f, u) if out == "both" else f if out == "f32" else u


def save_png(u8_hwc, path):
    """Write a uint8 grid [Hg, Wg, 3] (a one-channel batch is already three channels in its grid) as a PNG."""
    from PIL import Image
    a = u8_hwc.detach().cpu().contiguous().numpy() if isinstance(u8_hwc, torch.Tensor) else u8_hwc
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.dtype.name != "uint8":
        raise ValueError(f"a PNG takes a uint8 [H, W, 3 | 4] image, not {a.dtype} {a.shape}")
    Image.fromarray(a).save(path, format="PNG")
