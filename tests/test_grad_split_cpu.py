"""Split-product gradients of fp32 training, host side (no GPU): the constructor contract, the C ABI symbols, and which cfg2
convolutions take split-product gradients."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mdm_split_shadow_t", "mdm_conv_wgrad_split", "mdm_conv_wgrad_split_plan", "mdm_wgrad_split_last_route")


@pytest.mark.parametrize("kw", [dict(dtype=1, grad_products="split"),
                                dict(dtype=1, f32_products="exact", grad_products="split"),
                                dict(dtype=0, grad_products="split"),
                                dict(dtype=0, f32_products="exact", grad_products="split"),
                                dict(dtype=0, f32_products="split", grad_products="bf16"),
                                dict(dtype=0, grad_products=None)])
def test_invalid_combinations_raise(kw):
    import mdm
    from golden.make_golden import TINY
    with pytest.raises(ValueError, match="grad_products"):
        mdm.UNet(TINY, N=4, H=16, W=16, **kw)


def test_new_symbols_declared_bound_and_exported():
    from mdm import _lib
    header = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    declared = set(re.findall(r"\b(mdm_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        getattr(lib, name)
    assert lib.mdm_wgrad_split_last_route().decode() == "none"


def test_split_plan_and_validation_without_a_device():
    """mdm_conv_wgrad_split_plan is host-only: the split rule (never more splits than the workspace holds, whole 32-pixel slabs,
    no split without a workspace) and the descriptor checks."""
    from mdm import _lib, ops
    g = ops.ConvGeom(N=32, IH=32, IW=32, C0=128, C1=0, Cout=128)
    f = ops.wgrad_fields(0, g, 16, 16, None, 16)
    f.pop("dbias")
    slab = 9 * 128 * 128 * 4
    sk, nb = _lib.wgrad_split_plan(**dict(f, ws=16, ws_bytes=1 << 40))
    assert sk > 1 and nb == sk * slab
    assert (32 * 32 * 32) % 32 == 0 and sk <= 32 * 32 * 32 // 32 // 8
    sk2, nb2 = _lib.wgrad_split_plan(**dict(f, ws=16, ws_bytes=3 * slab + 5))
    assert sk2 == 3 and nb2 == 3 * slab
    assert _lib.wgrad_split_plan(**dict(f, ws=None, ws_bytes=0)) == (1, 0)
    with pytest.raises(RuntimeError, match="wgrad_split"):
        _lib.wgrad_split_plan(**dict(f, dtype=1))                  # bf16 descriptors are mdm_gemm's
    with pytest.raises(RuntimeError, match="wgrad_split"):
        _lib.wgrad_split_plan(**dict(f, bias=16))


def test_cfg2_split_gradient_coverage():
    """Which gradients of the cfg2 network take split products: every weight gradient but those of the 8-channel ends, every data
    gradient but the stride-2 ones (and the ends)."""
    import mdm
    from mdm import ops
    net = mdm.UNet(mdm.unet6_config(32), 32, 32, 32, _dry=True)
    convs = [s for s in net.specs if type(s).__name__ == "_Conv"]
    why_w = [ops.split_grad_reason(c.g, "wgrad") for c in convs]
    why_d = [ops.split_grad_reason(c.g, "dgrad") for c in convs]
    assert sorted(w for w in why_w if w) == ["channels", "channels"]                # the first and the last convolution
    assert set(w for w in why_d if w) == {"channels", "stride2"}
    assert sum(c.g.stride == 2 for c in convs) == sum(w == "stride2" for w in why_d) == 3
    assert sum(w is None for w in why_d) == len(convs) - 5
