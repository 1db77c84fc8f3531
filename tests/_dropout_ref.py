"""Reference side of the residual-block dropout tests (helpers only, no test functions).

(a) `keep_mask`: the dropout keep mask of csrc/norm.hip restated in numpy -- Philox4x32-10 as csrc/common.h writes it (`Philox`,
    `philox_at`), stream id 5, one call per 8 elements, 16-bit lanes, low half first.
(b) `unet_forward_dropout`: the forward of oracle/unet_ref.py, built from that module's own pieces, with a residual block that
    multiplies silu(gn2(h)) by a GIVEN mask times `scale` before conv2 (reference unet6.py:354, 360 with the mask made explicit).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.unet_ref import _conv, _gn, attn_block, same_pad_stride2, timestep_embedding

DROPOUT_STREAM = 5
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, ctr_lo, ctr_hi):
    """-> uint32 [len(ctr_lo), 4]; key / ctr_hi: Python ints (64 bit), ctr_lo: uint64 array.  csrc/common.h `Philox::operator()`."""
    ctr_lo = np.asarray(ctr_lo, dtype=np.uint64)
    c0, c1 = ctr_lo & _M32, ctr_lo >> np.uint64(32)
    c2 = np.full_like(c0, int(ctr_hi) & 0xFFFFFFFF)
    c3 = np.full_like(c0, (int(ctr_hi) >> 32) & 0xFFFFFFFF)
    a, b = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0            # < 2^64: both factors are below 2^32
        p1 = np.uint64(0xCD9E8D57) * c2
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(a), l1, h0 ^ c3 ^ np.uint64(b), l0
        a, b = (a + 0x9E3779B9) & 0xFFFFFFFF, (b + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def ctl_words(rate):
    """(thr, scale): thr = clamp(round(rate * 65536), 0, 65535), scale = 65536 / (65536 - thr)."""
    thr = max(0, min(65535, int(round(float(rate) * 65536))))
    return thr, 65536.0 / (65536 - thr)


def keep_mask(seed_key, offset, base, n, rate):
    """bool [n]: element i (global index g = base + i) is kept iff the 16-bit lane g & 7 of philox_at(rng, 5, g >> 3) is >= thr,
    with rng = {seed_key, offset}: key = seed_key, counter = {g >> 3, offset * 8 + 5} (csrc/sched.hip `philox_at`)."""
    thr, _ = ctl_words(rate)
    base, n = int(base), int(n)
    v0, v1 = base >> 3, (base + n + 7) >> 3
    words = philox4x32_10(seed_key, np.arange(v0, v1, dtype=np.uint64), (int(offset) * 8 + DROPOUT_STREAM) & 0xFFFFFFFFFFFFFFFF)
    lanes = np.stack([words & np.uint32(0xFFFF), words >> np.uint32(16)], axis=2).reshape(-1)      # lane j = half j & 1 of word j >> 1
    lo = base - (v0 << 3)
    return lanes[lo:lo + n] >= thr


def site_mask_nchw(seed_key, offset, base, N, H, W, C, rate):
    """The keep mask of one dropout site (NHWC [N][P][C] on the device) as a float NCHW tensor."""
    k = keep_mask(seed_key, offset, base, N * H * W * C, rate).reshape(N, H, W, C)
    return torch.from_numpy(np.ascontiguousarray(k.transpose(0, 3, 1, 2))).float()


def res_block_dropout(x, temb, p, pre, mask, scale):
    """oracle.unet_ref.res_block with dropout made explicit: silu(gn2(h)) * mask * scale in front of conv2."""
    skip = _conv(x, p, pre + ".skip") if (pre + ".skip.weight") in p else x
    h = _conv(F.silu(_gn(x, p, pre + ".norm1")), p, pre + ".conv1", padding=1)
    h = h + F.linear(F.silu(temb), p[pre + ".fc.weight"], p[pre + ".fc.bias"])[:, :, None, None]
    h = F.silu(_gn(h, p, pre + ".norm2")) * mask * scale
    h = _conv(h, p, pre + ".conv2", padding=1)
    return h + skip


def unet_forward_dropout(p, cfg, x, t, masks, scale):
    """oracle.unet_ref.unet_forward with `masks[pre]` (NCHW, 0 / 1, `pre` = the residual block's key prefix) applied in every block."""
    hid, mult, nres, attn = cfg["hid_channels"], cfg["ch_multipliers"], cfg["num_res_blocks"], cfg["apply_attn"]
    levels = len(mult)
    temb = timestep_embedding(t, hid).to(p["embed.0.weight"].dtype)
    temb = F.linear(temb, p["embed.0.weight"], p["embed.0.bias"])
    temb = F.linear(F.silu(temb), p["embed.2.weight"], p["embed.2.bias"])

    def res(h, pre):
        return res_block_dropout(h, temb, p, pre, masks[pre], scale)

    def block(h, pre, a):
        if a:
            return attn_block(res(h, pre + ".0"), p, pre + ".1")
        return res(h, pre)

    hs = [_conv(x, p, "in_conv", padding=1)]
    for l in range(levels):
        for j in range(nres):
            hs.append(block(hs[-1], f"downsamples.level_{l}.{j}", attn[l]))
        if l != levels - 1:
            hs.append(_conv(same_pad_stride2(hs[-1]), p, f"downsamples.level_{l}.{nres}.1", stride=2))
    h = res(hs[-1], "middle.0")
    h = attn_block(h, p, "middle.1")
    h = res(h, "middle.2")
    for l in range(levels - 1, -1, -1):
        for j in range(nres + 1):
            h = block(torch.cat([h, hs.pop()], dim=1), f"upsamples.level_{l}.{j}", attn[l])
        if l != 0:
            h = F.interpolate(h, scale_factor=2, mode="nearest")
            h = _conv(h, p, f"upsamples.level_{l}.{nres + 1}.1", padding=1)
    h = F.silu(_gn(h, p, "out_conv.0"))
    return _conv(h, p, "out_conv.2", padding=1)


def block_prefixes(cfg):
    """Key prefixes of the residual blocks in forward order (= the order of the dropout sites)."""
    mult, nres, attn = cfg["ch_multipliers"], cfg["num_res_blocks"], cfg["apply_attn"]
    levels = len(mult)
    out = []
    for l in range(levels):
        out += [f"downsamples.level_{l}.{j}" + (".0" if attn[l] else "") for j in range(nres)]
    out += ["middle.0", "middle.2"]
    for l in range(levels - 1, -1, -1):
        out += [f"upsamples.level_{l}.{j}" + (".0" if attn[l] else "") for j in range(nres + 1)]
    return out
