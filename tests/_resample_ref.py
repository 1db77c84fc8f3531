"""Reference side of the resample_with_conv=False tests (helpers only, no test functions).

The unet6 U-Net with parameter-free resampling -- nn.AvgPool2d(2) in place of every level's stride-2 convolution (reference
unet6.py:441-442) and a bare nn.Upsample(scale_factor=2, mode="nearest") with no convolution behind it (unet6.py:472-475) -- composed
from oracle/unet_ref.py's own blocks: no new arithmetic, only `F.avg_pool2d(h, 2)` and `F.interpolate(.., mode="nearest")` at the seams.
"""
import torch
import torch.nn.functional as F

from oracle.unet_ref import _conv, _gn, attn_block, param_shapes, random_params, res_block, timestep_embedding

NET3 = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2, 2], num_res_blocks=1, apply_attn=[False, True, False])


def resample_keys(cfg):
    """The keys resample_with_conv=False removes: downsamples.level_l.{nres}.1 (l < levels - 1), upsamples.level_l.{nres + 1}.1 (l > 0)."""
    levels, nres = len(cfg["ch_multipliers"]), cfg["num_res_blocks"]
    pre = [f"downsamples.level_{l}.{nres}.1" for l in range(levels - 1)] + [f"upsamples.level_{l}.{nres + 1}.1" for l in range(1, levels)]
    return {p + s for p in pre for s in (".weight", ".bias")}


def param_shapes_noconv(cfg):
    drop = resample_keys(cfg)
    return {k: v for k, v in param_shapes(cfg).items() if k not in drop}


def random_params_noconv(cfg, seed=1234):
    """oracle.unet_ref.random_params(cfg, seed) restricted to the kept keys (same recipe, same draws for every kept key)."""
    drop = resample_keys(cfg)
    return {k: v for k, v in random_params(cfg, seed).items() if k not in drop}


def unet_forward_noconv(p, cfg, x, t):
    """oracle.unet_ref.unet_forward with the two seams replaced (unet6.py:478-506 with resample_with_conv=False)."""
    hid, mult, nres, attn = cfg["hid_channels"], cfg["ch_multipliers"], cfg["num_res_blocks"], cfg["apply_attn"]
    levels = len(mult)
    temb = timestep_embedding(t, hid).to(p["embed.0.weight"].dtype)
    temb = F.linear(temb, p["embed.0.weight"], p["embed.0.bias"])
    temb = F.linear(F.silu(temb), p["embed.2.weight"], p["embed.2.bias"])

    def block(h, pre, a):
        if a:
            return attn_block(res_block(h, temb, p, pre + ".0"), p, pre + ".1")
        return res_block(h, temb, p, pre)

    hs = [_conv(x, p, "in_conv", padding=1)]
    for l in range(levels):
        for j in range(nres):
            hs.append(block(hs[-1], f"downsamples.level_{l}.{j}", attn[l]))
        if l != levels - 1:
            hs.append(F.avg_pool2d(hs[-1], 2))
    h = res_block(hs[-1], temb, p, "middle.0")
    h = attn_block(h, p, "middle.1")
    h = res_block(h, temb, p, "middle.2")
    for l in range(levels - 1, -1, -1):
        for j in range(nres + 1):
            h = block(torch.cat([h, hs.pop()], dim=1), f"upsamples.level_{l}.{j}", attn[l])
        if l != 0:
            h = F.interpolate(h, scale_factor=2, mode="nearest")
    h = F.silu(_gn(h, p, "out_conv.0"))
    return _conv(h, p, "out_conv.2", padding=1)


class UNetNoConvRef(torch.nn.Module):
    """nn.Module wrapper like oracle.unet_ref.UNetRef: `model(x, t).sample`, `.device`, `.parameters()`; dtype=torch.float64 is the
    yardstick option (the same network in double precision, never a target)."""

    class _Out:
        def __init__(self, sample):
            self.sample = sample

    def __init__(self, cfg, params=None, seed=1234, dtype=torch.float32):
        super().__init__()
        self.cfg = {k: v for k, v in cfg.items() if k != "resample_with_conv"}
        self.dtype = dtype
        params = params if params is not None else random_params_noconv(self.cfg, seed)
        self.keys = list(params.keys())
        self.plist = torch.nn.ParameterList([torch.nn.Parameter(params[k].clone().to(dtype)) for k in self.keys])

    @property
    def device(self):
        return self.plist[0].device

    def pdict(self):
        return {k: v for k, v in zip(self.keys, self.plist)}

    def forward(self, x, t):
        return UNetNoConvRef._Out(unet_forward_noconv(self.pdict(), self.cfg, x.to(self.dtype), t))
