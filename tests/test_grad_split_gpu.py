"""Split-product gradients of fp32 training (UNet(dtype=F32, f32_products="split", grad_products="split")), kernel level:

  * the data gradient of a stride-1 3x3 / 1x1 convolution as a FORWARD convolution of dY through the flipped, per-tap transposed
    split shadow (mdm_split_shadow_t) on mdm_gemm's split forward routes (ops.conv_dgrad_split_fields);
  * the weight gradient on mdm_conv_wgrad_split (activations split in registers, split-K partial slabs summed in a fixed order).

Each against fp64 (tests/_bounds.py) with the per-element bound of the split-product routes, NaN guard bands around every output,
NaN-filled workspaces, and the rel-L2 bar of the split routes ("f32_split" in test_gemm_routes_gpu.py).  The geometries are those
of cfg2 (32x32, hid 128, [1, 2, 2, 2]) and of the decoder's concatenated inputs, folded upsamples and skip projections.
"""
import pytest
import torch

from _bounds import Buf, check, conv_dgrad_ref, conv_wgrad_ref, rne_bf16
from _notes import note

pytestmark = pytest.mark.gpu

F32_SPLIT_BAR = 1.8e-5        # REL_BAR["f32_split"] of test_gemm_routes_gpu.py


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _shadow_t(wt):
    """PsT of one filter wt[tap][Cout][Cin] (device fp32) through mdm_split_shadow_t: -> [tap][Cin][Cout] view."""
    from mdm import _lib
    T, Co, Ci = wt.shape
    P = wt.contiguous().reshape(-1)
    out = Buf((T * Ci * Co,), torch.float32, P.device)
    segs = torch.tensor([[0, T, Co, Ci]], dtype=torch.int64, device=P.device)
    _lib.call("mdm_split_shadow_t", P.data_ptr(), out.t.data_ptr(), segs.data_ptr(), 1, _lib.stream())
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.t.view(T, Ci, Co)


# name: (N, IH, IW, C0, C1, Cout, k, stride, pads (t, l, b, r), ups)
GEOMS = {
    "32x32_128_128": (2, 32, 32, 128, 0, 128, 3, 1, (1, 1, 1, 1), 0),
    "16x16_256_256": (2, 16, 16, 256, 0, 256, 3, 1, (1, 1, 1, 1), 0),
    "8x8_512_512": (4, 8, 8, 512, 0, 512, 3, 1, (1, 1, 1, 1), 0),
    "4x4_512_512": (4, 4, 4, 512, 0, 512, 3, 1, (1, 1, 1, 1), 0),
    "16x16_concat_384_256": (2, 16, 16, 256, 128, 256, 3, 1, (1, 1, 1, 1), 0),
    "upsample_8to16_256": (2, 8, 8, 256, 0, 256, 3, 1, (1, 1, 1, 1), 1),
    "skip1x1_concat_384_256": (2, 16, 16, 256, 128, 256, 1, 1, (0, 0, 0, 0), 0),
    "stride2_32to16_128": (2, 32, 32, 128, 0, 128, 3, 2, (0, 0, 1, 1), 0),
}


def _geom(name):
    from mdm.ops import ConvGeom
    N, IH, IW, C0, C1, Co, k, s, (pt, pl, pb, pr), ups = GEOMS[name]
    return ConvGeom(N=N, IH=IH, IW=IW, C0=C0, C1=C1, Cout=Co, KH=k, KW=k, stride=s, pad_t=pt, pad_l=pl, pad_b=pb, pad_r=pr, ups=ups)


def _operands(g, seed):
    dev = _dev()
    x0 = Buf((g.N, g.IH, g.IW, g.C0), torch.float32, dev, fill=_rand((g.N, g.IH, g.IW, g.C0), seed))
    x1 = Buf((g.N, g.IH, g.IW, g.C1), torch.float32, dev, fill=_rand((g.N, g.IH, g.IW, g.C1), seed + 1)) if g.C1 else None
    dy = Buf((g.N, g.OH, g.OW, g.Cout), torch.float32, dev, fill=_rand((g.N, g.OH, g.OW, g.Cout), seed + 2))
    wt = _rand((g.taps, g.Cout, g.Cin), seed + 3, scale=(1.0 / (g.taps * g.Cin)) ** 0.5).to(dev)
    return x0, x1, dy, wt


def _run_dgrad_split(g, dy, wsT, prior1=None):
    """split data gradient into NaN-filled guarded destinations (source 1, if any, accumulates onto prior1) -> (d0, d1, route)"""
    from mdm import _lib, ops
    dev = _dev()
    d0 = Buf((g.N, g.VH, g.VW, g.C0), torch.float32, dev)
    d1 = Buf((g.N, g.VH, g.VW, g.C1), torch.float32, dev, fill=prior1) if g.C1 else None
    _lib.gemm(**ops.conv_dgrad_split_fields(g, dy.t, wsT, d0.t, 0, d1.t if d1 else None, 1 if d1 else 0))
    route = _lib.last_route()
    torch.cuda.synchronize()
    return d0, d1, route


@pytest.mark.parametrize("name", [k for k in GEOMS if GEOMS[k][7] == 1])
def test_split_dgrad_vs_fp64(name):
    from mdm import ops
    g = _geom(name)
    assert ops.split_grad_reason(g, "dgrad") is None
    x0, x1, dy, wt = _operands(g, 11)
    wsT = _shadow_t(wt)
    prior1 = _rand((g.N, g.VH, g.VW, g.C1), 19) if g.C1 else None
    d0, d1, route = _run_dgrad_split(g, dy, wsT, prior1)
    assert "split" in route, route
    assert d0.guards_intact() and (d1 is None or d1.guards_intact()), d0.first_bad_guard()
    ref, mag = conv_dgrad_ref(dy.t, wt, g.VH, g.VW, g.Cin, g.KH, g.KW, 1, (g.pad_t, g.pad_l, g.pad_b, g.pad_r))
    y = d0.t if not g.C1 else torch.cat([d0.t, d1.t], -1)
    if g.C1:                                   # source 1 accumulated onto its prior value
        p = torch.cat([torch.zeros(g.N, g.VH, g.VW, g.C0, dtype=torch.float64), prior1.double()], -1)
        ref, mag = ref + p, mag + p.abs()
    ratio, rel = check(name, y, ref, mag, g.taps * g.Cout, "f32", split=True)
    note("grad_split_dgrad", dict(geom=name, route=route, rel_l2=rel, worst_err_over_bound=ratio))
    assert rel < F32_SPLIT_BAR, (name, rel)
    # not the exact kernel: the exact fp32 data gradient differs in its bits
    ex0 = torch.zeros_like(d0.t)
    ex1 = prior1.to(_dev()) if g.C1 else None
    ops.conv_dgrad(0, g, dy.t, wt, ex0, 0, ex1, 1 if g.C1 else 0)
    torch.cuda.synchronize()
    assert not torch.equal(ex0, d0.t)
    # two runs: the same bits
    e0, e1, route2 = _run_dgrad_split(g, dy, wsT, prior1)
    assert route2 == route and torch.equal(e0.t, d0.t) and (d1 is None or torch.equal(e1.t, d1.t))


def _run_wgrad_split(g, dy, x0, x1, ws_floats, acc=0, prior=None):
    from mdm import _lib, ops
    dev = _dev()
    dw = Buf((g.taps, g.Cout, g.Cin), torch.float32, dev, fill=prior if prior is not None else "nan")
    ws = Buf((ws_floats,), torch.float32, dev) if ws_floats else None
    ops.conv_wgrad_split(g, dy.t, x0.t, x1.t if x1 else None, dw.t, ws=ws.t if ws else None, acc=acc)
    route = _lib.wgrad_split_last_route()
    torch.cuda.synchronize()
    assert dw.guards_intact() and (ws is None or ws.guards_intact()), dw.first_bad_guard()
    return dw, route


def _wgrad_ws_floats(g):
    from mdm import _lib, ops
    f = ops.wgrad_fields(0, g, 16, 16, 16 if g.C1 else None, 16, ws=None)
    f.pop("dbias")
    f["ws"], f["ws_bytes"] = 16, 1 << 40                     # dummy pointer: plan only
    return _lib.wgrad_split_plan(**f)[1] // 4


@pytest.mark.parametrize("name", list(GEOMS))
def test_split_wgrad_vs_fp64(name):
    from mdm import ops
    g = _geom(name)
    assert ops.split_grad_reason(g, "wgrad") is None
    x0, x1, dy, _ = _operands(g, 23)
    nws = _wgrad_ws_floats(g)
    dw, route = _run_wgrad_split(g, dy, x0, x1, nws)
    assert route.startswith("wgrad_split<") and (route.endswith("+splitk") == (nws > 0)), (route, nws)
    ref, mag, _ = conv_wgrad_ref(dy.t, x0.t, x1.t if x1 else None, g.KH, g.KW, g.stride, (g.pad_t, g.pad_l, g.pad_b, g.pad_r), g.ups)
    ratio, rel = check(name, dw.t, ref, mag, g.N * g.OH * g.OW, "f32", split=True)
    note("grad_split_wgrad", dict(geom=name, route=route, rel_l2=rel, worst_err_over_bound=ratio))
    assert rel < F32_SPLIT_BAR, (name, rel)
    ex = torch.zeros_like(dw.t)
    ops.conv_wgrad(0, g, dy.t, x0.t, x1.t if x1 else None, ex, acc=0)
    torch.cuda.synchronize()
    assert not torch.equal(ex, dw.t)
    dw2, route2 = _run_wgrad_split(g, dy, x0, x1, nws)
    assert route2 == route and torch.equal(dw2.t, dw.t)


def test_split_wgrad_unsplit_accumulates():
    """Without a workspace the reduction is not split: one launch, D0 += dW."""
    g = _geom("16x16_concat_384_256")
    x0, x1, dy, _ = _operands(g, 31)
    prior = _rand((g.taps, g.Cout, g.Cin), 37)
    dw, route = _run_wgrad_split(g, dy, x0, x1, 0, acc=1, prior=prior)
    assert route == "wgrad_split<128>", route
    ref, mag, _ = conv_wgrad_ref(dy.t, x0.t, x1.t, 3, 3, 1, (1, 1, 1, 1), 0)
    ref, mag = ref + prior.double(), mag + prior.double().abs()
    _, rel = check("wgrad_acc", dw.t, ref, mag, g.N * g.OH * g.OW, "f32", split=True)
    assert rel < F32_SPLIT_BAR, rel


@pytest.mark.parametrize("name", ["16x16_256_256", "skip1x1_concat_384_256"])
def test_bf16_products_would_fail_the_bar(name):
    """The bar is meaningful: the same gradients from bf16-rounded operands (fp64 products) are ~100x further from fp64."""
    g = _geom(name)
    x0, x1, dy, wt = _operands(g, 41)
    pads = (g.pad_t, g.pad_l, g.pad_b, g.pad_r)
    b = lambda t: rne_bf16(t.double()).double() if t is not None else None
    ref, _ = conv_dgrad_ref(dy.t, wt, g.VH, g.VW, g.Cin, g.KH, g.KW, 1, pads)
    r16, _ = conv_dgrad_ref(b(dy.t), b(wt), g.VH, g.VW, g.Cin, g.KH, g.KW, 1, pads)
    assert float((r16 - ref).norm() / ref.norm()) > 10 * F32_SPLIT_BAR
    refw, _, _ = conv_wgrad_ref(dy.t, x0.t, x1.t if x1 else None, g.KH, g.KW, 1, pads, g.ups)
    w16, _, _ = conv_wgrad_ref(b(dy.t), b(x0.t), b(x1.t) if x1 else None, g.KH, g.KW, 1, pads, g.ups)
    assert float((w16 - refw).norm() / refw.norm()) > 10 * F32_SPLIT_BAR


def test_split_shadow_t_layout():
    """mdm_split_shadow_t against a torch restatement: taps flipped, each tap transposed to [Cin][Cout], every 32-element block
    of a row as 4 chunks of hi halves then 4 of lo halves, chunk g = pairs (element 4g+k, element 16+4g+k), k = 0..3."""
    from mdm import _lib
    dev = _dev()
    shapes = [(9, 64, 32), (1, 32, 96), (9, 96, 64)]
    offs, n = [], 0
    for T, Co, Ci in shapes:
        offs.append(n)
        n += (T * Co * Ci + 7) // 8 * 8
    P = _rand((n,), 51).to(dev)
    out = Buf((n,), torch.float32, dev)
    segs = torch.tensor([[o, T, Co, Ci] for o, (T, Co, Ci) in zip(offs, shapes)], dtype=torch.int64, device=dev)
    _lib.call("mdm_split_shadow_t", P.data_ptr(), out.t.data_ptr(), segs.data_ptr(), len(shapes), _lib.stream())
    torch.cuda.synchronize()
    assert out.guards_intact()
    Pc = P.cpu()
    for o, (T, Co, Ci) in zip(offs, shapes):
        w = Pc[o:o + T * Co * Ci].view(T, Co, Ci)
        wt = w.flip(0).transpose(1, 2).contiguous()          # [tap'][Cin][Cout]
        hi = wt.to(torch.bfloat16)
        lo = (wt - hi.float()).to(torch.bfloat16)
        def arrange(h):                                      # [..., Cout] bf16 -> per 32-block: chunk g = (4g+k, 16+4g+k) pairs
            b = h.view(torch.int16).reshape(T, Ci, Co // 32, 2, 4, 4)      # [.., half, g, k]
            return b.permute(0, 1, 2, 4, 5, 3).reshape(T, Ci, Co // 32, 32)
        want = torch.cat([arrange(hi), arrange(lo)], -1).reshape(-1)
        got = out.t[o:o + T * Co * Ci].cpu().view(torch.int16)
        assert torch.equal(got, want), (T, Co, Ci, int((got != want).sum()))
