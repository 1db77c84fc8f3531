"""unet6 `resample_with_conv=False` (average-pool downsampling, bare nearest upsampling) without a GPU: the parameter table against
the reference's own state_dict key list, the config helper, the CPU restatement against the reference's run, the launch plan, the
two new C-ABI symbols."""
import math
import os
import re

import numpy as np
import pytest
import torch

import mdm
from mdm.unet import _Conv, _Norm, _Resample
from oracle.unet_ref import param_shapes, random_params, unet6_config as oracle_config

from _resample_ref import NET3, UNetNoConvRef, param_shapes_noconv, random_params_noconv, resample_keys, unet_forward_noconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET3_POOL = dict(NET3, resample_with_conv=False)


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_param_table_is_the_references_key_set_in_its_order(golden):
    g = golden("unet_resample")
    keys = [str(k) for k in g["keys"]]
    net = mdm.UNet(NET3_POOL, 1, 16, 16, _dry=True)
    assert net.reference_param_order() == keys
    table = mdm.UNet.param_table(NET3_POOL, 16, 16)
    assert set(table) == set(keys) and len(table) == len(keys) == len(param_shapes(NET3)) - 8
    want = param_shapes_noconv(NET3)
    assert list(want) == keys and {k: tuple(v) for k, v in table.items()} == {k: tuple(v) for k, v in want.items()}
    assert not any(k in table for k in resample_keys(NET3))
    # the conv model is what it was
    assert dict(mdm.UNet.param_table(NET3, 16, 16)) == {k: tuple(v) for k, v in param_shapes(NET3).items()}


def test_preset_loses_12_tensors_and_3097984_parameters():
    count = lambda tab: sum(math.prod(v) for v in tab.values())
    conv, pool = mdm.UNet.param_table(mdm.unet6_config(32)), mdm.UNet.param_table(mdm.unet6_config(32, resample_with_conv=False))
    assert len(conv) - len(pool) == 12 and count(conv) == 35746307 and count(conv) - count(pool) == 3097984
    assert set(conv) - set(pool) == resample_keys(mdm.unet6_config(32)) and not set(pool) - set(conv)


def test_config_helper_and_flag_validation():
    assert mdm.unet6_config(32) == oracle_config(32) and "resample_with_conv" not in mdm.unet6_config(32)
    assert mdm.unet6_config(32, resample_with_conv=True) == oracle_config(32)
    cfg = mdm.unet6_config(128, resample_with_conv=False)
    assert cfg["resample_with_conv"] is False and {k: v for k, v in cfg.items() if k != "resample_with_conv"} == oracle_config(128)
    both = mdm.unet6_config(32, drop_rate=0.1, resample_with_conv=False)
    assert both["drop_rate"] == 0.1 and both["resample_with_conv"] is False
    for bad in (0, 1, "False", None, 0.0):
        with pytest.raises(ValueError, match="resample_with_conv"):
            mdm.UNet(dict(NET3, resample_with_conv=bad), 1, 16, 16, _dry=True)
    assert mdm.UNet(dict(NET3, resample_with_conv=True), 1, 16, 16, _dry=True).reference_shapes() == mdm.UNet.param_table(NET3, 16, 16)


def test_restatement_reproduces_the_reference(golden):
    """The reference's unet6.UNet(resample_with_conv=False) in train mode (tests/golden/make_resample_golden.py) against the forward
    composed from oracle/unet_ref.py's blocks: the fp32 bounds of test_oracle_golden.test_unet_tiny_forward_backward (bit-equal is
    what one host gives; another host's oneDNN may order a sum differently)."""
    g = golden("unet_resample")
    p = {k: v.requires_grad_(True) for k, v in random_params_noconv(NET3, int(g["seed"])).items()}
    assert list(p) == [str(k) for k in g["keys"]]
    full = random_params(NET3, int(g["seed"]))
    assert all(torch.equal(p[k].detach(), full[k]) for k in p)                     # the same draws for every kept key
    y = unet_forward_noconv(p, NET3, T(g["x"]), T(g["t"]))
    print("max |y - ref|", float(np.abs(y.detach().numpy() - g["y"]).max()))
    assert np.allclose(y.detach().numpy(), g["y"], rtol=1e-4, atol=2e-5)
    (y * T(g["gy"])).sum().backward()
    n = 0
    for k in g.files:
        if k.startswith("grad::"):
            want, got = g[k], p[k.split("::")[1]].grad.numpy()
            assert np.allclose(got, want, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(want).max())), k
            n += 1
    assert n == 4
    # the module wrapper is the same function
    m = UNetNoConvRef(NET3_POOL, {k: v.detach() for k, v in p.items()})
    with torch.no_grad():
        assert torch.equal(m(T(g["x"]), T(g["t"])).sample, y.detach())


@pytest.mark.parametrize("uniform_t", [False, True])
@pytest.mark.parametrize("mode", ["bf16", "f32", "f32_split", "f32_split_grads"])
@pytest.mark.parametrize("cfg,N,hw", [(NET3_POOL, 2, 16), (None, 4, 32)])
def test_dry_net_plans(cfg, N, hw, mode, uniform_t):
    cfg = cfg or mdm.unet6_config(32, resample_with_conv=False)
    kw = {"bf16": dict(dtype=mdm.BF16), "f32": dict(dtype=mdm.F32), "f32_split": dict(dtype=mdm.F32, f32_products="split"),
          "f32_split_grads": dict(dtype=mdm.F32, f32_products="split", grad_products="split")}[mode]
    net = mdm.UNet(cfg, N, hw, hw, _dry=True, uniform_t=uniform_t, **kw)
    net._plan()
    levels = len(cfg["ch_multipliers"])
    rs = [s for s in net.specs if isinstance(s, _Resample)]
    assert [s.kind for s in rs] == ["avgpool2"] * (levels - 1) + ["nearest2"] * (levels - 1)
    for s in rs:
        f = 2 if s.kind == "nearest2" else 1
        assert (s.out.H * 2 // f, s.out.W * 2 // f, s.out.C) == (s.src.H * f, s.src.W * f, s.src.C) and s.name is None
    convs = [s for s in net.specs if isinstance(s, _Conv)]
    assert not any(c.g.stride == 2 or c.g.ups for c in convs)
    # no fusion reaches across a seam: a norm that reads a resampled map is a launch of its own in the forward
    outs = {id(s.out) for s in rs}
    assert all(not s.fwd_fused for s in net.specs if isinstance(s, _Norm) and id(s.src0) in outs)
    # the gradient marks: a parameter-less spec inherits its successor's
    dry = mdm.UNet(cfg, N, hw, hw, _dry=True, **kw)
    for s, nxt in zip(dry.specs[1:], dry.specs[2:]):
        if isinstance(s, _Resample):
            assert s.param_lo == nxt.param_lo


def test_default_plan_is_untouched():
    cfg = mdm.unet6_config(32)
    net = mdm.UNet(cfg, 4, 32, 32, _dry=True)
    assert not any(isinstance(s, _Resample) for s in net.specs)
    assert sum(isinstance(s, _Conv) and (s.g.stride == 2 or s.g.ups == 1) for s in net.specs) == 6


NEW_SYMBOLS = ("mdm_avgpool2", "mdm_upsample2")


def test_header_declares_and_library_exports_the_new_symbols():
    from mdm import _lib
    header = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.mdm_version() == 1
