"""Residual-block dropout (unet6 `drop_rate`) without a GPU: the oracle with explicit masks against the reference's own run, the
statistics of the mask definition, the launch plan of a dropout net, and the three new C-ABI symbols."""
import math
import os
import re

import numpy as np
import pytest
import torch

import mdm
from mdm.unet import _AttnCore, _Conv, _Norm, _Temb
from oracle.unet_ref import random_params, unet_forward

from _dropout_ref import block_prefixes, ctl_words, keep_mask, unet_forward_dropout
from golden.make_golden import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.from_numpy(np.asarray(a))


# ----------------------------------------------------------------------------- 1 / 2: the oracle with explicit masks
def test_all_ones_masks_are_the_plain_oracle_bit_for_bit():
    p = random_params(TINY)
    g = torch.Generator().manual_seed(3)
    x, t = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1, torch.tensor([4.0, 90.0])
    ones = {pre: torch.ones(()) for pre in block_prefixes(TINY)}
    with torch.no_grad():
        assert torch.equal(unet_forward_dropout(p, TINY, x, t, ones, 1.0), unet_forward(p, TINY, x, t))


def test_oracle_with_the_references_masks_matches_the_reference(golden):
    """The reference's unet6.UNet(drop_rate=0.3) in train mode (tests/golden/make_dropout_golden.py) against the oracle replaying its
    masks: the same arithmetic plus one multiply, so the fp32 bounds of test_oracle_golden.test_unet_tiny_forward_backward."""
    g = golden("unet_dropout")
    p = {k: v.requires_grad_(True) for k, v in random_params(TINY, int(g["seed"])).items()}
    sites = [str(s) for s in g["sites"]]
    assert sorted(sites) == sorted(block_prefixes(TINY))
    masks = {}
    for s in sites:
        shp = tuple(int(v) for v in g["shape::" + s])
        masks[s] = T(np.unpackbits(g["mask::" + s])[:math.prod(shp)].reshape(shp)).float()
    kept = sum(float(m.sum()) for m in masks.values()) / sum(m.numel() for m in masks.values())
    assert abs(kept - (1 - float(g["rate"]))) < 0.02                  # 14 k elements: sigma = 0.004
    y = unet_forward_dropout(p, TINY, T(g["x"]), T(g["t"]), masks, float(g["scale"]))
    assert np.allclose(y.detach().numpy(), g["y"], rtol=1e-4, atol=2e-5)
    (y * T(g["gy"])).sum().backward()
    n = 0
    for k in g.files:
        if k.startswith("grad::"):
            want, got = g[k], p[k.split("::")[1]].grad.numpy()
            assert np.allclose(got, want, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(want).max())), k
            n += 1
    assert n == 3


# ----------------------------------------------------------------------------- 3: statistics of the mask definition
N_STAT = 1 << 20
SEED_A, SEED_B = 11, 12         # fixed seeds at which the restatement sits inside 4 sigma (checked below): 5 sigma then hides nothing


def _sigmas(frac, q, n):
    return abs(frac - q) / math.sqrt(q * (1 - q) / n)


@pytest.mark.parametrize("seed", [SEED_A, SEED_B])
def test_mask_statistics(seed):
    rate = 0.1
    thr, scale = ctl_words(rate)
    q = 1 - thr / 65536
    assert thr == 6554 and scale == 65536 / (65536 - 6554)
    a = keep_mask(seed, 1, 0, N_STAT, rate)
    other_site = keep_mask(seed, 1, N_STAT, N_STAT, rate)
    next_offset = keep_mask(seed, 2, 0, N_STAT, rate)
    qa = q * q + (1 - q) * (1 - q)
    figs = dict(keep=_sigmas(a.mean(), q, N_STAT), sites=_sigmas((a == other_site).mean(), qa, N_STAT),
                offsets=_sigmas((a == next_offset).mean(), qa, N_STAT))
    print(figs)
    assert all(v < 4.0 for v in figs.values()), figs          # the choice of seeds (5 sigma is the bar of the definition)
    assert all(v < 5.0 for v in figs.values()), figs
    assert keep_mask(seed, 1, 0, 4096, 0.0).all()
    # a site that does not start on a vector boundary reads the same lanes
    assert np.array_equal(keep_mask(seed, 1, 5, 100, rate), a[5:105])


# ----------------------------------------------------------------------------- 4: the plan
def _planned(cfg, **kw):
    net = mdm.UNet(cfg, 32, 32, 32, dtype=mdm.BF16, _dry=True, **kw)
    net._plan()
    return net


def _decisions(net, skip=()):
    """Every decision of the plan, spec by spec (links as names); `skip`: names of norms to leave out together with the links to them."""
    nm = lambda s: None if s is None or s.name in skip else s.name
    out = []
    for s in net.specs:
        if isinstance(s, _Conv):
            out.append((s.name, s.fwd_in_pair, nm(s.fwd_mate), nm(s.gn_fwd), s.sums, s.wgrad, s.dgrad, tuple(sorted(s.grad_exact.items())),
                        nm(s.gn_bwd), nm(s.bwd_mate), s.bwd_in_pair))
        elif isinstance(s, _Norm):
            if s.name not in skip:
                out.append((s.name, s.fwd_fused, s.bwd_fused, nm(s.sums_for), s.drop_base))
        elif isinstance(s, _AttnCore):
            out.append(("attn", s.mode))
        elif isinstance(s, _Temb):
            out.append(("temb", s.skinny))
    return out


def test_plan_of_a_dropout_net():
    cfg0, cfg = mdm.unet6_config(32), mdm.unet6_config(32, drop_rate=0.1)
    assert "drop_rate" not in cfg0 and cfg["drop_rate"] == 0.1 and {k: v for k, v in cfg.items() if k != "drop_rate"} == cfg0
    plain, drop = _planned(cfg0), _planned(cfg)
    sites = [b.norm2 for b in drop.blocks]
    assert len(sites) == 22 and all(not s.fwd_fused and not s.bwd_fused for s in sites)
    assert any(b.norm2.fwd_fused for b in plain.blocks) and any(b.norm2.bwd_fused for b in plain.blocks)     # what the rule gives up
    assert all(b.conv1.gn_fwd is None and b.conv2.gn_bwd is None for b in drop.blocks)
    bases = [s.drop_base for s in sites]
    assert bases[0] == 0 and all(b % 8 == 0 for b in bases) and all(y > x for x, y in zip(bases, bases[1:]))
    assert [y - x for x, y in zip(bases, bases[1:])] == [s.out.N * s.out.P * s.out.C for s in sites[:-1]]
    assert drop.dropout_sites() == [(s.name, s.drop_base, s.out.N * s.out.P * s.out.C) for s in sites] and plain.dropout_sites() == []
    # no decision of any other spec differs
    names = {s.name for s in sites}
    assert _decisions(drop, names) == _decisions(plain, names)
    # sums_for still rides on the standalone backward of every site
    assert all(b.norm2.sums_for is b.conv1 and b.conv1.sums == "norm" for b in drop.blocks)
    # drop_rate = 0 is the plan of a cfg without the key; a uniform_t plan of a dropout cfg is the drop_rate = 0 plan
    assert _decisions(_planned(dict(cfg0, drop_rate=0.0))) == _decisions(plain)
    assert _decisions(_planned(cfg, uniform_t=True)) == _decisions(_planned(cfg0, uniform_t=True))
    assert _planned(cfg, uniform_t=True).dropout_sites() == []
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="drop_rate"):
            mdm.UNet(dict(cfg0, drop_rate=bad), 1, 32, 32, _dry=True)


# ----------------------------------------------------------------------------- 5: the C ABI
DROP_FIELDS = ("rng", "drop_base", "ctl")       # of mdm_gn_desc: non-null rng selects the dropout kernels of both GroupNorm entry points


def test_header_declares_and_library_exports_the_new_symbols():
    from mdm import _lib
    header = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    lib = _lib.load()
    assert re.search(r"^int mdm_dropout_mask\(", header, re.M)
    assert "mdm_dropout_mask" in _lib.EXPORTS and lib.mdm_dropout_mask is not None
    struct = re.search(r"typedef struct mdm_gn_desc \{(.*?)\} mdm_gn_desc;", header, re.S).group(1)
    fields = dict(_lib.GnDesc._fields_)
    decls = (r"const uint64_t\* rng;", r"uint64_t drop_base;", r"const uint32_t\* ctl;")
    for name, ctype, decl in zip(DROP_FIELDS, (_lib.vp, _lib.u64, _lib.vp), decls):
        assert re.search(r"^\s*" + decl, struct, re.M), name
        assert fields[name] is ctype, name
    for name in ("mdm_groupnorm_fwd", "mdm_groupnorm_bwd"):
        assert re.search(r"^int " + name + r"\(const mdm_gn_desc\* desc_host, void\* stream\);", header, re.M), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
