"""The unet6 U-Net on libmdm_hip.so: parameter store, static launch plan, hipGraph replay.

Mirrors reference code/models/unet/unet6.py `UNet` (:365-506) behind the same call
contract `model(x[N,C,H,W], t[N]).sample` and the same state_dict key
grammar, but nothing here is an nn.Module: parameters live in ONE flat fp32 buffer
(plus flat grad / bf16-shadow buffers) and a forward or backward pass is a recorded
list of C-ABI launches over statically allocated NHWC activations.
"""
from __future__ import annotations

import math
import struct
from collections import OrderedDict
from types import SimpleNamespace

import os
import torch

from . import _lib, ops
from ._lib import BF16, F32


def unet6_config(image_size, in_channels=3, out_channels=3, drop_rate=0.0, resample_with_conv=True):
    """Presets of reference models_Unet.py:132-171 (`Model('unet6', C, H, W, out_C)`).  `drop_rate`: unet6's constructor argument of
    that name (unet6.py:378; the factory passes 0.0) -- a key of the dict only when it is not zero, so the default dict is unchanged.
    `resample_with_conv` (unet6.py:379; the factory passes True): likewise a key only when it is False."""
    if image_size in (32, 64):
        mult, attn = [1, 2, 2, 2], [False, False, True, False]
    elif image_size in (128, 256):
        mult, attn = [1, 1, 2, 2, 4, 4], [False, False, False, False, True, False]
    else:
        raise NotImplementedError("model selection error")
    cfg = dict(in_channels=in_channels, hid_channels=128, out_channels=out_channels, ch_multipliers=mult,
               num_res_blocks=2, apply_attn=attn)
    if drop_rate:
        cfg["drop_rate"] = float(drop_rate)
    if resample_with_conv is not True:
        cfg["resample_with_conv"] = resample_with_conv      # False; anything else is rejected by UNet
    return cfg


def _pad8(c):
    return (c + 7) // 8 * 8


# --------------------------------------------------------------------------- #
class Act:
    """A statically allocated NHWC activation and (lazily) its gradient."""

    def __init__(self, name, N, H, W, C, needs_grad=True):
        self.name, self.N, self.H, self.W, self.C = name, N, H, W, C
        self.data = None
        self.grad = None
        self.grad_written = False
        self.pending_add = None       # a gradient contribution (another activation's grad tensor) not yet folded into `grad`
        self.needs_grad = needs_grad
        self.norm_spec = None         # the _Norm that produced this activation (UNet._norm), if one did

    @property
    def P(self):
        return self.H * self.W


class ParamStore:
    """Flat fp32 master / grad buffers with named views.

    Internal layouts: conv weight `[tap][Cout_p][Cin_p]` (reference OIHW, unet6.py:196-199),
    linear `[out][in]` (unet6.py:157), vectors as is; `_p` = padded to a multiple of 8.
    All `fc.weight` (and `fc.bias`) are stored back to back so the 22 time-embedding
    projections of unet6.py:350,359 run as ONE contraction.
    """

    def __init__(self):
        self.entries = OrderedDict()     # name -> SimpleNamespace(off, ishape, rshape, kind)
        self.size = 0
        self.P = self.G = self.Pb = None
        self.PbT = self.tiles = None                     # bf16 stores: per-tap transposed shadow (allocate)
        self.Ps = self.split_segs = None                 # fp32 stores: enable_split
        self.PsT = self.split_t_segs = None              # fp32 stores: enable_split_t

    def declare(self, name, kind, rshape, ishape):
        assert name not in self.entries, name
        n = 1
        for d in ishape:
            n *= d
        self.entries[name] = SimpleNamespace(off=self.size, n=n, ishape=tuple(ishape), rshape=tuple(rshape), kind=kind)
        self.size += (n + 7) // 8 * 8          # keep every view 32-byte aligned

    def allocate(self, device, dtype):
        self.device, self.dtype = device, dtype
        self.P = torch.zeros(self.size, device=device, dtype=torch.float32)
        self.G = torch.zeros(self.size, device=device, dtype=torch.float32)
        self.Pb = torch.zeros(self.size, device=device, dtype=torch.bfloat16) if dtype == BF16 else None
        # second bf16 shadow with every conv filter transposed per tap ([tap][Cin][Cout]) for the data gradient
        if dtype == BF16:
            self.PbT = torch.zeros(self.size, device=device, dtype=torch.bfloat16)
            rows = []
            for e in self.entries.values():
                if e.kind not in ("conv", "convlin"):
                    continue
                taps, co, ci = e.ishape
                assert co % 8 == 0 and ci % 8 == 0
                for tp in range(taps):
                    for r0 in range(0, co, 64):           # 64 x 64 tiles (mdm_transpose_shadow_bf16)
                        for c0 in range(0, ci, 64):
                            rows.append((e.off + tp * co * ci, co, ci, r0, c0))
            self.tiles = torch.tensor(rows, dtype=torch.int64, device=device)

    def f(self, name):          # fp32 master view
        e = self.entries[name]
        return self.P[e.off:e.off + e.n].view(e.ishape)

    def g(self, name):          # fp32 gradient view
        e = self.entries[name]
        return self.G[e.off:e.off + e.n].view(e.ishape)

    def w(self, name):          # view the contraction kernels read (bf16 shadow or the master itself)
        if self.dtype == F32:
            return self.f(name)
        e = self.entries[name]
        return self.Pb[e.off:e.off + e.n].view(e.ishape)

    def wT(self, name):         # per-tap transposed bf16 filter [tap][Cin][Cout]
        e = self.entries[name]
        taps, co, ci = e.ishape
        return self.PbT[e.off:e.off + e.n].view(taps, ci, co)

    # -- fp32 stores: the filters once more as bf16 hi / lo pairs (mdm_gemm_desc.B_split, conv_halo_body<..., SPLIT>)
    def enable_split(self):
        """Allocate the split shadow `Ps` (same offsets as P) for every conv filter whose rows are whole 32-channel blocks."""
        if self.Ps is not None:
            return
        assert self.dtype == F32, "the split shadow belongs to an fp32 store"
        segs = [(e.off, e.n) for e in self.entries.values() if e.kind in ("conv", "convlin") and e.ishape[2] % 32 == 0]
        self.Ps = torch.zeros(self.size, device=self.device, dtype=torch.float32)
        self.split_segs = torch.tensor(segs, dtype=torch.int64, device=self.device)
        self.emit_split_shadow()

    def emit_split_shadow(self):
        if self.Ps is not None:
            _lib.call("mdm_split_shadow", _lib.ptr(self.P), _lib.ptr(self.Ps), _lib.ptr(self.split_segs),
                      int(self.split_segs.shape[0]), _lib.stream())

    def w_split(self, name):
        e = self.entries[name]
        if self.Ps is None or e.kind not in ("conv", "convlin") or e.ishape[2] % 32:
            return None
        return self.Ps[e.off:e.off + e.n].view(e.ishape)

    # -- split-product gradients: the filters once more, taps flipped and each tap transposed, as hi / lo pairs (mdm_split_shadow_t)
    def enable_split_t(self):
        """Allocate `PsT` (same offsets as P) for every conv filter whose Cout and Cin are whole 32-channel blocks: the data
        gradient of such a layer is a forward convolution of dY through it (ops.conv_dgrad_split_fields)."""
        if self.PsT is not None:
            return
        assert self.dtype == F32, "the split shadow belongs to an fp32 store"
        segs = [(e.off,) + tuple(e.ishape) for e in self.entries.values()
                if e.kind in ("conv", "convlin") and e.ishape[1] % 32 == 0 and e.ishape[2] % 32 == 0]
        self.PsT = torch.zeros(self.size, device=self.device, dtype=torch.float32)
        self.split_t_segs = torch.tensor(segs, dtype=torch.int64, device=self.device)
        self.emit_split_shadow_t()

    def emit_split_shadow_t(self):
        if self.PsT is not None:
            _lib.call("mdm_split_shadow_t", _lib.ptr(self.P), _lib.ptr(self.PsT), _lib.ptr(self.split_t_segs),
                      int(self.split_t_segs.shape[0]), _lib.stream())

    def ws_t(self, name):       # [tap][Cin][Cout] view of PsT (flipped taps), or None
        e = self.entries[name]
        if self.PsT is None or e.kind not in ("conv", "convlin") or e.ishape[1] % 32 or e.ishape[2] % 32:
            return None
        taps, co, ci = e.ishape
        return self.PsT[e.off:e.off + e.n].view(taps, ci, co)

    def emit_transposed_shadow(self):
        if self.PbT is not None:
            # from the bf16 shadow the optimizer (or sync_shadow's cast) has just written: a third less traffic than from P
            _lib.call("mdm_transpose_shadow_bf16", _lib.ptr(self.Pb), _lib.ptr(self.PbT), _lib.ptr(self.tiles),
                      int(self.tiles.shape[0]), _lib.stream())

    def emit_shadows(self):
        """The shadows derived from P (or from its bf16 shadow Pb), where the store has them: behind every change of the weights."""
        self.emit_transposed_shadow()
        self.emit_split_shadow()        # fp32 stores with split products: the filters' hi / lo shadow
        self.emit_split_shadow_t()      # ... and the flipped, transposed one of split-product gradients

    def sync_shadow(self):
        if self.Pb is not None:
            ops.cast_bf16(self.P, self.Pb)
        self.emit_shadows()

    # -- reference state_dict interchange
    def to_internal(self, name, t):
        e = self.entries[name]
        t = t.detach().to(torch.float32)
        assert tuple(t.shape) == e.rshape, (name, tuple(t.shape), e.rshape)
        if e.kind == "conv":
            o, i, kh, kw = e.rshape
            out = torch.zeros(e.ishape, dtype=torch.float32)
            out[:, :o, :i] = t.permute(2, 3, 0, 1).reshape(kh * kw, o, i)
            return out
        if e.kind == "convlin":            # an nn.Linear [out, in] run as a 1x1 convolution
            o, i = e.rshape
            out = torch.zeros(e.ishape, dtype=torch.float32)
            out[0, :o, :i] = t
            return out
        if e.kind == "vecpad":
            out = torch.zeros(e.ishape, dtype=torch.float32)
            out[:e.rshape[0]] = t
            return out
        return t.reshape(e.ishape)

    def to_reference(self, name, t):
        e = self.entries[name]
        t = t.detach().to("cpu", torch.float32)
        if e.kind == "conv":
            o, i, kh, kw = e.rshape
            return t[:, :o, :i].reshape(kh, kw, o, i).permute(2, 3, 0, 1).contiguous()
        if e.kind == "convlin":
            o, i = e.rshape
            return t[0, :o, :i].clone()
        if e.kind == "vecpad":
            return t[:e.rshape[0]].clone()
        return t.reshape(e.rshape).clone()

    def load_state_dict(self, sd):
        missing = [k for k in self.entries if k not in sd]
        extra = [k for k in sd if k not in self.entries]
        if missing or extra:
            raise KeyError(f"state_dict mismatch: missing={missing[:4]} unexpected={extra[:4]}")
        host = torch.zeros(self.size, dtype=torch.float32)
        for k, e in self.entries.items():
            host[e.off:e.off + e.n] = self.to_internal(k, sd[k]).reshape(-1)
        self.P.copy_(host)
        self.sync_shadow()

    def state_dict(self, order=None, src=None):
        src = self.P if src is None else src
        host = src.detach().to("cpu")
        keys = order or list(self.entries)
        return OrderedDict((k, self.to_reference(k, host[self.entries[k].off:self.entries[k].off + self.entries[k].n]
                                                 .view(self.entries[k].ishape))) for k in keys)

    def grad_dict(self):
        return self.state_dict(src=self.G)

    def flat_from_reference(self, sd, fill=0.0):
        """Host flat fp32 buffer (this store's layout) from a {reference key: tensor in reference shape} dict
        (optimizer moments of a checkpoint: same keys and shapes as the weights)."""
        host = torch.full((self.size,), float(fill), dtype=torch.float32)
        for k, e in self.entries.items():
            host[e.off:e.off + e.n] = self.to_internal(k, sd[k]).reshape(-1)
        return host


# --------------------------------------------------------------------------- #
class _ResBlock:
    """The members of one residual block (`skip`: its 1x1 projection, or None), shared by them as `spec.block`: which conv pairs
    with which, and whose sums ride on which norm, is read from this one record.  `paired`: the block may use launch pairs."""

    def __init__(self, skip, conv1, norm2, conv2, paired):
        self.skip, self.conv1, self.norm2, self.conv2, self.paired = skip, conv1, norm2, conv2, paired
        for s in (skip, conv1, norm2, conv2):
            if s is not None:
                s.block = self


class _Conv:
    def __init__(self, net, name, geom, src0, src1, out, rshape, fc_slot=None, resid=None):
        self.net, self.name, self.g, self.src0, self.src1, self.out = net, name, geom, src0, src1, out
        self.rshape, self.fc_slot, self.resid = rshape, fc_slot, resid
        self.block = self.param_lo = None
        # ---- decisions, fixed by UNet._plan() before anything is recorded; fwd() / bwd() only read them
        self.fwd_in_pair = False    # a skip projection: launched inside its block's conv1 pair
        self.fwd_mate = None        # conv1: the skip projection that shares its launch
        self.gn_fwd = None          # the _Norm right after this conv whose forward is this launch's epilogue
        self.sums = None            # bias / time-embedding sums: "colsum" | "wgrad" (ride on the weight gradient) | "norm" (block.norm2 emits them)
        self.wgrad = None           # "grouped" | "split" (mdm_conv_wgrad_split) | "single"
        self.dgrad = None           # "t" (transposed bf16 shadow) | "split" | "exact"; None: the input needs no gradient
        self.grad_exact = {}        # grad_products="split": {"wgrad" / "dgrad": "exact:<reason>"} of what stays exact fp32
        self.gn_bwd = None          # the _Norm that produced this conv's only input and whose backward is the data gradient's epilogue
        self.bwd_mate = None        # conv2: the skip projection whose whole backward runs here, data gradients in one launch
        self.bwd_in_pair = False    # that skip projection

    def declare(self, st):
        g = self.g
        rs = self.rshape
        st.declare(self.name + ".weight", "conv" if len(rs) == 4 else "convlin", rs, (g.taps, g.Cout, g.Cin))
        st.declare(self.name + ".bias", "vecpad", (rs[0],), (g.Cout,))

    def _fwd_fields(self):
        n, st, g = self.net, self.net.store, self.g
        rv, ld = (None, 0)
        if self.fc_slot is not None:
            rv, ld = n.T_all[:, self.fc_slot:], (0 if n.uniform_t else n.fc_total)     # uniform_t: ONE projection row for every image
        # 4x4 / 8x8 maps: this conv runs on whole-image tiles -> it normalises its own output (gnf_* epilogue; no GroupNorm launch)
        return ops.conv_fwd_fields(n.dt, g, self.src0.data, self.src1.data if self.src1 else None, st.w(self.name + ".weight"),
                                   st.f(self.name + ".bias"), self.out.data, rowvec=rv, rv_ld=ld,
                                   resid=self.resid.data if self.resid else None, ws=n.splitk_ws,
                                   gnf=self.gn_fwd.fwd_epilogue() if self.gn_fwd is not None else None,
                                   w_split=st.w_split(self.name + ".weight") if n.split_products else None,
                                   f32_split=int(n.split_products))

    def fwd(self):
        # A ResidualBlock's skip projection (1x1) only needs the block input, like conv1 only needs norm1's output: the two
        # run as ONE launch (mdm_gemm_pair) when conv1 is reached; conv2 consumes the projection afterwards.
        if self.fwd_in_pair:
            return
        if self.fwd_mate is not None:
            ops.conv_fwd_pair(self._fwd_fields(), self.fwd_mate._fwd_fields())
        else:
            _lib.gemm(**self._fwd_fields())

    def bwd(self, pair_a=None):
        """pair_a: descriptor fields of another conv's data gradient (the block's conv2) to launch TOGETHER with this one's.

        grad_products="split" (fp32 training): the data gradient of a stride-1 3x3 / 1x1 layer is a forward convolution of dY through
        the flipped, transposed split shadow (ops.conv_dgrad_split_fields; for a folded x2 upsample at the virtual resolution, then
        sumpool2'd as always), the weight gradient runs on mdm_conv_wgrad_split, the bias gradient stays on mdm_colsum.  Exact fp32
        remains, by design: stride-2 data gradients; both gradients of the 8-channel ends of the net (the first and last
        convolution: not whole 32-channel blocks); layers whose Cin is not a whole 64-channel tile (data gradient only); and
        everything that is not a convolution -- attention, GroupNorm, the time-embedding path, the loss and the optimizer."""
        n, st, g = self.net, self.net.store, self.g
        if self.bwd_in_pair and pair_a is None:         # a skip projection: its backward runs next to conv2's (bwd_mate)
            return
        dy = n.grad_for_read(self.out)
        r = self.resid
        per, ld = (None, 0)
        if self.fc_slot is not None:
            per, ld = n.dT_all[:, self.fc_slot:], n.fc_total
        s0, s1 = self.src0, self.src1
        fuse_bias = self.sums == "wgrad"            # bias sums ride along in the weight-gradient kernel
        if self.sums == "colsum":
            ops.colsum(n.dt, dy, g.N, g.OH * g.OW, g.Cout, per_img=per, ld=ld, acc_img=0, dbias=st.g(self.name + ".bias"))
        # Weight gradient.  It only READS dy and the layer input, and both stay in memory: on the bf16 path it is not
        # launched here but collected into the current GROUP (UNet._flush_wgrads: one launch for a whole stretch of the
        # backward, overwriting G -- no read of the zero-filled gradient).  dy must then stay untouched until the flush.
        wf = ops.wgrad_fields(n.dt, g, dy, s0.data, s1.data if s1 else None, st.g(self.name + ".weight"),
                              dbias=st.g(self.name + ".bias") if fuse_bias else None)
        grouped = self.wgrad == "grouped"
        if grouped:
            wf["acc0"] = 0
            n.overwritten.add(self.name + ".weight")     # this slot of G is stored, not accumulated: no zeroing needed
            wf["splitk"] = sk = ops.wgrad_group_split(g)
            if sk > 1:
                wf["ws"] = n.wgrad_slab(sk * g.taps * g.Cout * g.Cin)
                wf["ws_bytes"] = wf["ws"].numel() * 4
            n.pending_wgrads.append((self, wf))
        elif self.wgrad == "split":
            ops.conv_wgrad_split(g, dy, s0.data, s1.data if s1 else None, st.g(self.name + ".weight"), ws=n.splitk_ws)
            self._note_route("wgrad", _lib.wgrad_split_last_route)
        else:
            ops.conv_wgrad(n.dt, g, dy, s0.data, s1.data if s1 else None, st.g(self.name + ".weight"), ws=n.splitk_ws,
                           dbias=st.g(self.name + ".bias") if fuse_bias else None)
        if self.grad_exact:
            n.grad_routes.setdefault(self.name, {}).update(self.grad_exact)
        if r is not None and r.needs_grad:       # y = conv(..) + resid  (unet6.py:333, 362): d(resid) += dy
            if r.grad_written and not (grouped and r.pending_add is None):
                ops.add_(n.dt, r.grad, dy)
            elif grouped:
                r.pending_add = dy               # folded in by the next writer of r.grad (dst = dy + dx): dy stays intact
            else:
                r.grad, r.grad_written = dy, True      # alias: dy is dead after this op, later ops += into it
        if self.dgrad is None:
            assert pair_a is None
            return
        # bf16: the filters come from the per-tap transposed shadow so both operands are k-contiguous
        if self.dgrad == "t":
            wmat = st.wT(self.name + ".weight")
            dgrad = lambda *a: ops.conv_dgrad_t(*a, ws=n.splitk_ws)     # small maps split the taps over the grid
        elif self.dgrad == "split":
            # a forward convolution of dY through the flipped, transposed split shadow, on the split forward routes
            wmat = st.ws_t(self.name + ".weight")

            def dgrad(dt, g_, dy_, w_, d0, a0, d1=None, a1=0):
                _lib.gemm(**ops.conv_dgrad_split_fields(g_, dy_, w_, d0, a0, d1, a1))
                self._note_route("dgrad", _lib.last_route)
        else:
            dgrad, wmat = ops.conv_dgrad, st.w(self.name + ".weight")
        # conv2 of a ResidualBlock with a skip projection: the projection's whole backward runs HERE, its data gradient in
        # the same launch as this one's (both read this block's dY; they write different tensors)
        mate = self.bwd_mate

        def emit(fields):
            if pair_a is not None:
                _lib.gemm_pair(pair_a, fields)
            elif mate is not None:
                mate.bwd(pair_a=fields)
            else:
                _lib.gemm(**fields)
        nm = self.gn_bwd
        if nm is not None:
            # 4x4 / 8x8 maps: the data gradient runs on whole-image tiles, so the GroupNorm backward is its epilogue --
            # d(z) never goes to memory and the GroupNorm launch disappears (nm.bwd_fused)
            x = nm.src0
            gx, ax, addx = n.grad_for_write(x, want_add=2)
            emit(ops.conv_dgrad_t_fields(n.dt, g, dy, wmat, gx, ax, ws=n.splitk_ws,
                                         gnb=dict(x=x.data, stats=nm.stats, gamma=st.f(nm.name + ".weight"), beta=st.f(nm.name + ".bias"),
                                                  dgamma=st.g(nm.name + ".weight"), dbeta=st.g(nm.name + ".bias"), G=32, silu=nm.silu,
                                                  add=addx, **nm.sums_fields(ax, addx))))
        elif g.ups:
            tmp = n.scratch(g.N * g.VH * g.VW * g.Cin)
            dgrad(n.dt, g, dy, wmat, tmp, 0)
            g0, a0, _ = n.grad_for_write(s0)
            ops.sumpool2(n.dt, tmp, g0, a0, g.N, g.IH, g.IW, g.Cin)
        else:
            g0, a0, _ = n.grad_for_write(s0)
            g1, a1, _ = n.grad_for_write(s1) if s1 is not None else (None, 0, None)
            if self.dgrad == "t":
                emit(ops.conv_dgrad_t_fields(n.dt, g, dy, wmat, g0, a0, g1, a1, ws=n.splitk_ws))
            else:
                dgrad(n.dt, g, dy, wmat, g0, a0, g1, a1)

    def _note_route(self, which, route_fn):
        """Record, each time the plan runs, the route the split launch just issued took (UNet.grad_products_table).  A split data
        gradient reads only the split shadow: a route that is not a split one would compute garbage, so it is an error."""
        routes = self.net.grad_routes.setdefault(self.name, {})
        routes[which] = "pending"

        def fn():
            r = route_fn()
            if "split" not in r:
                raise RuntimeError(f"{self.name}: the split-product {which} took route {r!r}")
            routes[which] = r
        _lib.note(fn)


class _Norm:
    def __init__(self, net, name, src0, src1, out, silu, eps=1e-6):
        self.net, self.name, self.src0, self.src1, self.out, self.silu, self.eps = net, name, src0, src1, out, silu, eps
        self.block = self.param_lo = self.stats = None
        # ---- decisions (UNet._plan)
        self.fwd_fused = False      # the conv right before it normalises its own output (that conv's gn_fwd)
        self.bwd_fused = False      # its backward is the epilogue of its consumers' data gradients (their gn_bwd)
        self.sums_for = None        # norm2 of a ResidualBlock: conv1, whose bias / time-embedding sums this backward also emits
        # ---- set while the specs are built (UNet._resblock), not a decision of the plan
        self.drop_base = None       # norm2 of a ResidualBlock of a net with drop_rate > 0: first global element index of this dropout site

    def declare(self, st):
        c = self.out.C
        st.declare(self.name + ".weight", "vec", (c,), (c,))
        st.declare(self.name + ".bias", "vec", (c,), (c,))

    def fwd_epilogue(self):
        """This GroupNorm as the `gnf` epilogue of the conv before it (fwd_fused).  Called while that conv is recorded: `stats` is
        allocated there, which is where fwd() would have allocated it (a conv's fwd allocates nothing else)."""
        st = self.net.store
        self.stats = self.net.alloc((self.src0.N, 32, 2), torch.float32)
        return dict(out=self.out.data, gamma=st.f(self.name + ".weight"), beta=st.f(self.name + ".bias"), stats=self.stats, G=32,
                    silu=self.silu, eps=self.eps)

    def sums_fields(self, acc, add):
        """sum_* arguments of this norm's backward (own launch or epilogue): its dx is conv1's complete dY -- conv1's output has no
        other consumer and is nobody's residual (UNet._plan checks), so it is written, not accumulated, and nothing is pending."""
        n, prod = self.net, self.sums_for
        if prod is None:
            return {}
        assert acc == 0 and add is None, self.name
        return dict(sum_img=n.dT_all[:, prod.fc_slot:], sum_ld=n.fc_total, sum_all=n.store.g(prod.name + ".bias"))

    def fwd(self):
        n, st = self.net, self.net.store
        s0, s1 = self.src0, self.src1
        if self.fwd_fused:
            return
        self.stats = n.alloc((s0.N, 32, 2), torch.float32)
        if self.drop_base is not None:      # y = silu(GN(x)) * keep * scale (unet6.py:360), the mask drawn inside the kernel
            ops.groupnorm_fwd_dropout(n.dt, s0.data, s0.C, s0.N, s0.P, st.f(self.name + ".weight"), st.f(self.name + ".bias"), self.silu,
                                      self.out.data, self.stats, n.gn_ws, n.drop_rng.dev, self.drop_base, n.drop_ctl, eps=self.eps)
            return
        ops.groupnorm_fwd(n.dt, s0.data, s0.C, s1.data if s1 else None, s1.C if s1 else 0, s0.N, s0.P,
                          st.f(self.name + ".weight"), st.f(self.name + ".bias"), self.silu, self.out.data, self.stats, n.gn_ws,
                          eps=self.eps)

    def bwd(self):
        n, st = self.net, self.net.store
        s0, s1 = self.src0, self.src1
        if self.bwd_fused:
            return
        dyo = n.grad_for_read(self.out)
        g0, a0, add0 = n.grad_for_write(s0, want_add=2)
        if self.drop_base is not None:      # the same mask again, from the same counters, on dy as it is loaded
            ops.groupnorm_bwd_dropout(n.dt, s0.data, s0.C, s0.N, s0.P, st.f(self.name + ".weight"), st.f(self.name + ".bias"), self.silu,
                                      dyo, self.stats, g0, a0, st.g(self.name + ".weight"), st.g(self.name + ".bias"), n.gn_ws,
                                      n.drop_rng.dev, self.drop_base, n.drop_ctl, add0=add0, **self.sums_fields(a0, add0))
            return
        g1, a1, add1 = n.grad_for_write(s1, want_add=True) if s1 is not None else (None, 0, None)
        ops.groupnorm_bwd(n.dt, s0.data, s0.C, s1.data if s1 else None, s1.C if s1 else 0, s0.N, s0.P,
                          st.f(self.name + ".weight"), st.f(self.name + ".bias"), self.silu, dyo, self.stats,
                          g0, a0, g1, a1, st.g(self.name + ".weight"), st.g(self.name + ".bias"), n.gn_ws,
                          add0=add0, add1=add1, **self.sums_fields(a0, add0))


class _AttnCore:
    """softmax(q k^T / sqrt(C)) v over L = H*W tokens, one head (unet6.py:316-324)."""

    def __init__(self, net, qkv, out):
        self.net, self.qkv, self.out, self.name = net, qkv, out, None
        self.param_lo = self.lse = self.S = self.delta = None
        self.mode = None            # "fused" | "f32_small" (one exact-fp32 forward launch) | "unfused"   (UNet._plan)

    def declare(self, st):
        pass

    def fwd(self):
        n, q, o = self.net, self.qkv, self.out
        N, L, C = q.N, q.P, o.C
        if self.mode == "fused":     # one kernel, the scores never reach memory (csrc/attn.hip)
            self.lse = n.alloc((N, L), torch.float32)
            ops.attn_fwd(n.dt, q.data, o.data, self.lse, N, L, C, 1.0 / math.sqrt(C))
            return
        self.S = n.alloc((N, L, L), n.tdtype)
        d = q.data.view(N, L, 3 * C)
        sc = 1.0 / math.sqrt(C)
        if self.mode == "f32_small":                               # one exact-fp32 launch; S = the probabilities, as below
            ops.attn_f32_small_fwd(q.data, o.data, self.S, N, L, C, sc)
            return
        ops.matmul(n.dt, 0, L, L, C, d, 3 * C, d[:, :, C:], 3 * C, self.S, L, batch=N, sA=L * 3 * C, sB=L * 3 * C, sD=L * L, alpha=sc)
        ops.softmax_fwd(n.dt, self.S, N * L, L)
        ops.matmul(n.dt, 1, L, C, L, self.S, L, d[:, :, 2 * C:], 3 * C, o.data, C, batch=N, sA=L * L, sB=L * 3 * C, sD=L * C)

    def bwd(self):
        n, q, o = self.net, self.qkv, self.out
        N, L, C = q.N, q.P, o.C
        do = n.grad_for_read(o)
        dqkv, acc, _ = n.grad_for_write(q)
        assert acc == 0
        if self.mode == "fused":
            self.delta = n.alloc((N, L), torch.float32)
            ops.attn_bwd(n.dt, q.data, o.data, do, self.lse, self.delta, dqkv, N, L, C, 1.0 / math.sqrt(C))
            return
        d = q.data.view(N, L, 3 * C)
        g = dqkv.view(N, L, 3 * C)
        sc = 1.0 / math.sqrt(C)
        dP = n.alloc((N, L, L), n.tdtype)
        s3, sl, sc_ = L * 3 * C, L * L, L * C
        ops.matmul(n.dt, 2, L, C, L, self.S, L, do, C, g[:, :, 2 * C:], 3 * C, batch=N, sA=sl, sB=sc_, sD=s3)           # dV = P^T dO
        ops.matmul(n.dt, 0, L, L, C, do, C, d[:, :, 2 * C:], 3 * C, dP, L, batch=N, sA=sc_, sB=s3, sD=sl)               # dP = dO V^T
        ops.softmax_bwd(n.dt, self.S, dP, N * L, L)                                                                     # dS
        ops.matmul(n.dt, 1, L, C, L, dP, L, d[:, :, C:], 3 * C, g, 3 * C, batch=N, sA=sl, sB=s3, sD=s3, alpha=sc)        # dQ = dS K
        ops.matmul(n.dt, 2, L, C, L, dP, L, d, 3 * C, g[:, :, C:], 3 * C, batch=N, sA=sl, sB=s3, sD=s3, alpha=sc)        # dK = dS^T Q


class _Resample:
    """The parameter-free resampling of resample_with_conv=False: kind "avgpool2" = nn.AvgPool2d(2) in place of a level's stride-2
    convolution (unet6.py:441-442), "nearest2" = the bare nn.Upsample(scale_factor=2, mode="nearest") (unet6.py:472-475).  One
    streaming launch per direction; each is the other's backward (up to the pool's 0.25)."""

    def __init__(self, net, kind, src, out):
        assert kind in ("avgpool2", "nearest2"), kind
        self.net, self.kind, self.src, self.out, self.name = net, kind, src, out, None
        self.param_lo = None

    def declare(self, st):
        pass

    def fwd(self):
        n, s, o = self.net, self.src, self.out
        if self.kind == "avgpool2":
            ops.avgpool2(n.dt, s.data, o.data, 0, o.N, o.H, o.W, o.C)
        else:
            ops.upsample2(n.dt, s.data, o.data, 0, 1.0, s.N, s.H, s.W, s.C)

    def bwd(self):
        n, s, o = self.net, self.src, self.out
        if not s.needs_grad:
            return
        dy = n.grad_for_read(o)
        g, acc, _ = n.grad_for_write(s)
        if self.kind == "avgpool2":         # every pixel of the 2x2 block receives a quarter of the pooled pixel's gradient
            ops.upsample2(n.dt, dy, g, acc, 0.25, o.N, o.H, o.W, o.C)
        else:                               # the backward of nn.Upsample, as behind the folded x2 convolutions (_Conv.bwd)
            ops.sumpool2(n.dt, dy, g, acc, s.N, s.H, s.W, s.C)


class _Temb:
    """Sinusoidal embedding -> 2-layer MLP -> SiLU -> all 22 per-block projections in one
    contraction (unet6.py:18-34, 395-399, 350, 359).  fp32 throughout (rows = batch only)."""

    def __init__(self, net, hid, temb, fc_total, names=("embed.0", "embed.2"), variant=None):
        self.net, self.hid, self.temb, self.fc_total = net, hid, temb, fc_total
        self.l1, self.l2 = names
        self.variant = variant          # None: unet6.py:18-34; (flip_sin_to_cos, freq_shift): diffusers' Timesteps
        self.name = self.param_lo = None
        self.e = self.h1 = self.a1 = self.tm = self.st_ = None
        self.skinny = None              # the dedicated small-batch kernels, or the general contraction   (UNet._plan: _skinny())

    def declare(self, st):
        st.declare(self.l1 + ".weight", "lin", (self.temb, self.hid), (self.temb, self.hid))
        st.declare(self.l1 + ".bias", "vec", (self.temb,), (self.temb,))
        st.declare(self.l2 + ".weight", "lin", (self.temb, self.temb), (self.temb, self.temb))
        st.declare(self.l2 + ".bias", "vec", (self.temb,), (self.temb,))

    def _rows(self):
        """Rows of the time-embedding path: the batch -- or ONE when the plan was built for a timestep shared by the whole batch
        (`UNet(uniform_t=True)`: the reverse sampler; every image then reads projection row 0)."""
        return 1 if self.net.uniform_t else self.net.N

    def _skinny(self):
        """The dedicated small-batch kernels (mdm_skinny_*) take this path; larger batches use the general contraction."""
        N = self._rows()
        return (self.hid % 2 == 0 and ops.skinny_supported(N, self.temb, self.hid) and ops.skinny_supported(N, self.temb, self.temb)
                and ops.skinny_supported(N, self.fc_total, self.temb) and ops.skinny_supported(N, self.temb, self.fc_total))

    def fwd(self):
        n, st = self.net, self.net.store
        N, hid, te, ft = self._rows(), self.hid, self.temb, self.fc_total
        f = lambda *s: n.alloc(s, torch.float32)
        self.e, self.h1, self.a1, self.tm, self.st_ = f(N, hid), f(N, te), f(N, te), f(N, te), f(N, te)
        if self.skinny:         # 3 launches: embedding + Linear + SiLU, Linear + SiLU, the 22 projections
            ops.skinny_linear_fwd(None, st.f(self.l1 + ".weight"), st.f(self.l1 + ".bias"), N, te, hid, self.h1, act_out=self.a1,
                                  t=n.t_in, variant=self.variant, emb_out=self.e)
            ops.skinny_linear_fwd(self.a1, st.f(self.l2 + ".weight"), st.f(self.l2 + ".bias"), N, te, te, self.tm, act_out=self.st_)
            ops.skinny_linear_fwd(self.st_, n.fc_w, n.fc_b, N, ft, te, n.T_all)
            return
        ops.timestep_embedding(n.t_in, N, hid, self.e, self.variant)
        ops.matmul(F32, 0, N, te, hid, self.e, hid, st.f(self.l1 + ".weight"), hid, self.h1, te, bias=st.f(self.l1 + ".bias"))
        ops.silu_fwd(self.h1, self.a1, N * te)
        ops.matmul(F32, 0, N, te, te, self.a1, te, st.f(self.l2 + ".weight"), te, self.tm, te, bias=st.f(self.l2 + ".bias"))
        ops.silu_fwd(self.tm, self.st_, N * te)
        ops.matmul(F32, 0, N, ft, te, self.st_, te, n.fc_w, te, n.T_all, ft, bias=n.fc_b)

    def bwd(self):
        n, st = self.net, self.net.store
        assert not n.uniform_t, "a uniform_t plan is forward-only"
        N, hid, te, ft = n.N, self.hid, self.temb, self.fc_total
        f = lambda *s: n.alloc(s, torch.float32)
        d_st, d_tm, d_a1, d_h1 = f(N, te), f(N, te), f(N, te), f(N, te)
        if self.skinny:         # 6 launches: bias gradients ride on the weight gradients, silu' on the data gradients
            splits = max(s_ for s_ in range(1, 17) if (ft // 64) % s_ == 0)
            slabs = f(splits, N, te)
            # single writers of their weight-gradient slots: stored (acc=0), so those slots need no zeroing either
            n.overwritten.update(n.fc_weight_names + [self.l1 + ".weight", self.l2 + ".weight"])
            ops.matmul(F32, 2, ft, te, N, n.dT_all, ft, self.st_, te, n.fc_gw, te, acc=0, out_f32=1, dbias=n.fc_gb)
            ops.skinny_linear_bwd(n.dT_all, n.fc_w, N, te, ft, dx=d_tm, pre=self.tm, splits=splits, slabs=slabs)
            if splits > 1:
                ops.silu_bwd_sum(self.tm, slabs, splits, N * te, d_tm)
            ops.matmul(F32, 2, te, te, N, d_tm, te, self.a1, te, st.g(self.l2 + ".weight"), te, acc=0, out_f32=1, dbias=st.g(self.l2 + ".bias"))
            ops.skinny_linear_bwd(d_tm, st.f(self.l2 + ".weight"), N, te, te, dx=d_h1, pre=self.h1)
            ops.matmul(F32, 2, te, hid, N, d_h1, te, self.e, hid, st.g(self.l1 + ".weight"), hid, acc=0, out_f32=1, dbias=st.g(self.l1 + ".bias"))
            return
        ops.matmul(F32, 2, ft, te, N, n.dT_all, ft, self.st_, te, n.fc_gw, te, acc=1, out_f32=1)
        ops.colsum(F32, n.dT_all, 1, N, ft, dbias=n.fc_gb)
        # K = sum(Cout) ~ 5k against M = batch: split the reduction (partial slabs in the workspace, summed in a fixed order)
        ops.matmul(F32, 1, N, te, ft, n.dT_all, ft, n.fc_w, te, d_st, te, splitk=max(1, min(16, ft // 128)), ws=n.splitk_ws)
        ops.silu_bwd(self.tm, d_st, d_tm, 0, N * te)
        ops.matmul(F32, 2, te, te, N, d_tm, te, self.a1, te, st.g(self.l2 + ".weight"), te, acc=1, out_f32=1)
        ops.colsum(F32, d_tm, 1, N, te, dbias=st.g(self.l2 + ".bias"))
        ops.matmul(F32, 1, N, te, te, d_tm, te, st.f(self.l2 + ".weight"), te, d_a1, te)
        ops.silu_bwd(self.h1, d_a1, d_h1, 0, N * te)
        ops.matmul(F32, 2, te, hid, N, d_h1, te, self.e, hid, st.g(self.l1 + ".weight"), hid, acc=1, out_f32=1)
        ops.colsum(F32, d_h1, 1, N, te, dbias=st.g(self.l1 + ".bias"))


# --------------------------------------------------------------------------- #
class UNet:
    """HIP unet6.  `UNet(cfg, N, H, W, dtype=BF16)`; `model(x, t).sample`; `forward_plan` /
    `backward_plan` are `_lib.Recording`s that Trainer/Sampler splice into their own graphs."""

    def __init__(self, cfg, N, H, W, dtype=BF16, device=None, params=None, seed=1234, store=None, use_graph=True,
                 group_wgrads=True, wgrad_group_bytes=None, pair_convs=True, f32_products="exact", uniform_t=False, grad_products="exact",
                 drop_seed=0, _drop_parent=None, _dry=False):
        # grad_products="split": fp32 TRAINING with the backward's convolution products as hi / lo pairs too (data gradients through
        # the flipped, transposed split shadow PsT on the split forward routes, weight gradients on mdm_conv_wgrad_split); fp32
        # storage, accumulation and optimizer state.  Only with dtype=F32, f32_products="split"; "exact" (default) is today's path.
        if grad_products not in ("exact", "split") or (grad_products == "split" and not (dtype == F32 and f32_products == "split")):
            raise ValueError(f"grad_products={grad_products!r} needs dtype=F32 and f32_products='split' (got dtype={dtype}, "
                             f"f32_products={f32_products!r}); the default is 'exact'")
        self.grad_products = grad_products
        # uniform_t: the whole batch shares ONE timestep (the reverse sampler: sampler.py:137-145 passes a constant vector) -- the
        # time-embedding MLP and its 22 projections then run on one row and every image reads projection row 0.  Forward-only.
        self.uniform_t = bool(uniform_t)
        self.cfg = dict(cfg)
        # drop_rate (unet6.py:378): nn.Dropout between silu(norm2(.)) and conv2 of every ResidualBlock (:354, :360), here inside the
        # standalone GroupNorm kernels of those norm2 (csrc/norm.hip).  Forward-only plans (uniform_t, the fp32 sampling twins:
        # _drop_parent=False) are built without it and keep every fusion; a twin with dropout shares its parent's state (_drop_parent).
        rate = float(self.cfg.get("drop_rate", 0.0))
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"drop_rate={rate!r}: need 0 <= drop_rate < 1")
        self.drop_rate = 0.0 if (self.uniform_t or _drop_parent is False) else rate
        self.drop_seed = int(drop_seed)
        # resample_with_conv (unet6.py:379, 393): False = the parameter-free resampling of the original DDPM U-Net (_Resample)
        self.resample_with_conv = self.cfg.get("resample_with_conv", True)
        if not isinstance(self.resample_with_conv, bool):
            raise ValueError(f"resample_with_conv={self.resample_with_conv!r}: need True or False")
        self.drop_rng = self.drop_ctl = self._drop_ctl_modes = None
        self.N, self.H, self.W = N, H, W
        self.dt = dtype
        self.group_wgrads = group_wgrads            # weight gradients of the bf16 path run as grouped launches
        self.pair_convs = dtype == BF16 and pair_convs   # skip projections share a launch with conv1 / conv2's data gradient
        # fp32 storage with the FORWARD 3x3 convolutions' products on the bf16 matrix pipe as hi / lo pairs (~2^-16 per product
        # instead of 2^-24; mdm_gemm_desc.B_split).  "exact" (default) is the parity path; "split" is for the reverse sampler.
        assert f32_products in ("exact", "split") and (f32_products == "exact" or dtype == F32), f32_products
        self.split_products = f32_products == "split"
        if wgrad_group_bytes is None:
            # A group is one launch AND one gradient bucket (mdm/dist.py).  Under data parallelism ~32 MB groups let the exchange of one
            # bucket run under the backward of the next; a single process has nothing to exchange, and there one group over the whole
            # backward is faster (3.80 -> 3.73 ms/step at cfg2: every CU's share of the nine-tap weight-gradient launch is long).
            import torch.distributed as dist
            wgrad_group_bytes = (32 << 20) if (dist.is_available() and dist.is_initialized()) else (1 << 40)
        self.wgrad_group_bytes = wgrad_group_bytes  # a group is flushed once it covers this many bytes of fp32 gradient
        self._uniform_twin, self._batch_plans, self._sampling_plans = None, {}, {}
        if _dry:       # shape/parameter bookkeeping only (no device, no kernels): see `param_table`.  `_plan()` runs on request: it
            self.store = ParamStore()       # needs the library (host predicates only), the parameter table does not
            self._build_specs()
            self._declare_params()
            self._set_param_marks()
            return
        if not torch.cuda.is_available():
            raise RuntimeError("mdm.UNet needs a GPU and libmdm_hip.so; there is no CPU fallback")
        _lib.load()
        self.tdtype = _lib.torch_dtype(dtype)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.training = True
        self._bufs = []
        self._scratch = None
        self._scratch_n = 0
        self.use_graph = use_graph
        self.grad_routes = {}               # conv name -> {"dgrad": route, "wgrad": route} (grad_products_table)
        self.pending_wgrads = []
        self.wgrad_groups = []
        shared = store is not None
        self.store = store if shared else ParamStore()
        self._build_specs()
        if not shared:
            self._declare_params()
            self.store.allocate(self.device, dtype)
        else:
            assert store.dtype == dtype, "a shared parameter store must have the same compute dtype"
        if self.split_products:
            self.store.enable_split()
        if self.grad_products == "split":
            self.store.enable_split_t()
        self._set_param_marks()
        self._plan()
        self._materialize()
        if self.drop_rate > 0:
            self._init_dropout(_drop_parent)
        if not shared:
            if params is None:
                params = self._default_params(seed)
            self.load_state_dict(params)
        self.forward_plan = self._record(self._emit_fwd)
        self.overwritten = set()         # gradient slots the backward STORES (filled in while it is recorded)
        if self.uniform_t:
            self.backward_plan = None    # forward-only plan
            self.zero_table, self.zero_floats = None, 0
        else:
            self.backward_plan = self._record(self._emit_bwd)
            self._build_zero_table()
        self._graph_fwd = None

    def _init_dropout(self, parent):
        """The dropout state: a DeviceRng keyed by (drop_seed, data-parallel rank) whose offset the FIRST launch of forward_plan bumps
        (forward and backward of one step see one offset, every eager run / graph replay / micro-batch a new one), and the control
        words ctl = {thr, scale} the kernels read -- train() / eval() rewrite them on the device, in stream order, so they act on plans
        and graphs that are already recorded.  Plans over the same weights (with_batch, sampling_plan "model") share both."""
        if parent is not None:
            assert parent.drop_rate == self.drop_rate and parent.drop_rng is not None
            self.drop_rng, self.drop_ctl, self._drop_ctl_modes = parent.drop_rng, parent.drop_ctl, parent._drop_ctl_modes
            return
        from .scheduler import DeviceRng
        import torch.distributed as dist
        rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
        self.drop_rng = DeviceRng(self.device, self.drop_seed, rank)
        thr, scale = ops.dropout_ctl_words(self.drop_rate)
        bits = lambda f: struct.unpack("<i", struct.pack("<f", f))[0]
        self._drop_ctl_modes = torch.tensor([[0, bits(1.0)], [thr, bits(scale)]], dtype=torch.int32, device=self.device)    # eval, train
        self.drop_ctl = self._drop_ctl_modes[1].clone()

    def dropout_sites(self):
        """[(norm2 name, base, elements)] of the dropout sites in `specs` order ([] without dropout): element e of a site has the
        global index base + e in the mask definition of csrc/norm.hip."""
        return [(s.name, s.drop_base, s.out.N * s.out.P * s.out.C) for s in self.specs if isinstance(s, _Norm) and s.drop_base is not None]

    def _default_params(self, seed):
        from .init import xavier_like_params
        return xavier_like_params(self.reference_shapes(), seed)

    @staticmethod
    def param_table(cfg, H=32, W=32):
        """{reference key: reference shape} in flat-buffer order, computed on the host only."""
        return UNet(cfg, 1, H, W, _dry=True).reference_shapes()

    def _twin(self, N, **overrides):
        """Another launch plan of this architecture: same weights (store), dtype, products and timestep mode unless overridden.
        NOT inherited, here as before: group_wgrads, pair_convs and wgrad_group_bytes -- a twin always gets their defaults."""
        kw = dict(dtype=self.dt, device=self.device, store=self.store, use_graph=self.use_graph,
                  f32_products="split" if self.split_products else "exact", uniform_t=self.uniform_t, grad_products=self.grad_products,
                  drop_seed=self.drop_seed, _drop_parent=self if self.drop_rate > 0 else None)
        kw.update(overrides)
        return type(self)(self.cfg, N, self.H, self.W, **kw)

    def with_batch(self, N):
        """A second launch plan over the SAME weights for another batch size (e.g. sample_num)."""
        if N == self.N:
            return self
        if N not in self._batch_plans:
            self._batch_plans[N] = self._twin(N)
        return self._batch_plans[N]

    def with_uniform_t(self):
        """The forward-only twin of this plan for a timestep shared by the whole batch (same weights, batch, dtype, products): what
        `mdm.Sampler` runs -- the time-embedding path on one row instead of `sample_num` (0.125 -> ~0.04 ms of a 5.5 ms reverse step
        at sample_num = 100)."""
        if self.uniform_t:
            return self
        if self._uniform_twin is None:
            self._uniform_twin = self._twin(self.N, uniform_t=True)
        self._uniform_twin.training = self.training
        return self._uniform_twin

    def sampling_plan(self, N, precision="f32_split"):
        """The launch plan the reverse sampler should run on, with THIS model's current weights: `precision` =
        "f32_split" (default: fp32 storage, convolution products as bf16 hi / lo pairs -- the fastest mode whose 1000-step output stays
        within 1e-3 of the CPU reference, DESIGN finding 31), "f32" (exact fp32) or "model" (this model's own dtype: bf16 storage is
        3.1 s instead of 6 s per 1000 x 100 samples but 1e-2 away from the reference after 100 steps).
        An fp32 model shares its store with the plan; a bf16 model keeps a second, fp32 store of identical layout whose master
        weights are copied on the device from this model's fp32 masters at every call (143 MB at cfg2: ~0.1 ms)."""
        assert precision in ("f32_split", "f32", "model"), precision
        if precision == "model" or (precision == "f32" and self.dt == F32 and not self.split_products) or \
                (precision == "f32_split" and self.dt == F32 and self.split_products):
            net = self.with_batch(N)
            if net.split_products:
                net.store.emit_split_shadow()
            return net
        products = "split" if precision == "f32_split" else "exact"
        plans = self._sampling_plans
        key = (N, precision)
        if key not in plans:
            kw = dict(dtype=F32, f32_products=products, uniform_t=False, grad_products="exact", _drop_parent=False)     # forward-only: no dropout
            if self.dt == F32:
                plans[key] = self._twin(N, **kw)
            else:
                twin = next((v for (n2, p2), v in plans.items() if v.store is not self.store), None)
                plans[key] = self._twin(N, store=twin.store if twin is not None else None,
                                        params=None if twin is not None else self.state_dict(), **kw)
                if products == "split":
                    plans[key].store.enable_split()
        net = plans[key]
        if net.store is not self.store:
            assert net.store.size == self.store.size
            net.store.P.copy_(self.store.P)
            net.store.sync_shadow()
        elif net.split_products:
            # A shared fp32 store: the hi / lo filter shadow is refreshed by the optimizer tail only if it existed when that tail was
            # recorded (a TrainStep graph captured before the first sampling_plan call has no such launch).  One cheap launch here
            # makes "THIS model's current weights" true whatever was captured when.
            net.store.emit_split_shadow()
        net.training = self.training
        return net

    # ---- construction ---------------------------------------------------------
    def _act(self, name, H, W, C, needs_grad=True):
        a = Act(name, self.N, H, W, C, needs_grad)
        self.acts.append(a)
        return a

    # What a subclass with another assembly (UNet2D) changes about the shared builders below:
    down_pads = (0, 0, 1, 1)        # (top, left, bottom, right) of a stride-2 3x3 convolution: SamePad2d pads bottom / right only
    norm_eps = 1e-6
    res_names = ("skip", "fc")      # member names of a residual block's 1x1 projection and time-embedding projection
    pair_blocks = True              # residual blocks may use launch pairs (_ResBlock.paired)

    def _begin_specs(self, cin, cout):
        self.cin, self.cout, self.cin_p, self.cout_p = cin, cout, _pad8(cin), _pad8(cout)
        self.acts, self.specs, self.blocks, self.fc_slots = [], [], [], OrderedDict()
        self.fc_total = 0
        self._drop_elems = 0            # running element count of the dropout sites (64-bit on the host; every site a multiple of 8)

    def _conv(self, name, src0, src1, Cout, k=3, stride=1, ups=0, fc=None, resid=None, rshape=None):
        pads = (1, 1, 1, 1) if k == 3 and stride == 1 else self.down_pads if k == 3 else (0, 0, 0, 0)
        g = ops.ConvGeom(N=self.N, IH=src0.H, IW=src0.W, C0=src0.C, C1=src1.C if src1 else 0, Cout=Cout, KH=k, KW=k, stride=stride,
                         pad_t=pads[0], pad_l=pads[1], pad_b=pads[2], pad_r=pads[3], ups=ups)
        out = self._act(name, g.OH, g.OW, Cout)
        self.specs.append(_Conv(self, name, g, src0, src1, out, rshape or (Cout, g.Cin, k, k), fc_slot=fc, resid=resid))
        return out

    def _norm(self, name, src0, src1, silu):
        out = self._act(name, src0.H, src0.W, src0.C + (src1.C if src1 else 0))
        out.norm_spec = _Norm(self, name, src0, src1, out, silu, eps=self.norm_eps)
        self.specs.append(out.norm_spec)
        return out

    def _resample(self, kind, name, src):
        H, W = (src.H // 2, src.W // 2) if kind == "avgpool2" else (2 * src.H, 2 * src.W)
        out = self._act(name, H, W, src.C)
        self.specs.append(_Resample(self, kind, src, out))
        return out

    def _resblock(self, pre, x0, x1, Cout):               # ResidualBlock (unet6.py:336-362) / diffusers' ResnetBlock2D
        Cin = x0.C + (x1.C if x1 else 0)
        slot = self.fc_total
        self.fc_slots[f"{pre}.{self.res_names[1]}"] = (slot, Cout)
        self.fc_total += Cout
        skip = self._conv(f"{pre}.{self.res_names[0]}", x0, x1, Cout, k=1) if Cin != Cout else x0
        skip_spec = self.specs[-1] if Cin != Cout else None
        a = self._norm(pre + ".norm1", x0, x1, True)
        h = self._conv(pre + ".conv1", a, None, Cout, fc=slot)
        b = self._norm(pre + ".norm2", h, None, True)
        if self.drop_rate > 0:                            # a dropout site: nn.Dropout on silu(norm2(.)) (unet6.py:354, 360)
            b.norm_spec.drop_base = self._drop_elems
            self._drop_elems += b.N * b.P * b.C
        out = self._conv(pre + ".conv2", b, None, Cout, resid=skip)
        self.blocks.append(_ResBlock(skip_spec, self.specs[-3], self.specs[-2], self.specs[-1], self.pair_blocks))
        return out

    def _build_specs(self):
        cfg = self.cfg
        cin, hid, cout = cfg["in_channels"], cfg["hid_channels"], cfg["out_channels"]
        mult, nres, attn = cfg["ch_multipliers"], cfg["num_res_blocks"], cfg["apply_attn"]
        if isinstance(attn, bool):
            attn = [attn] * len(mult)
        temb = cfg.get("time_embedding_dim") or 4 * hid
        levels = len(mult)
        assert hid % 32 == 0, "GroupNorm(32) needs hid_channels % 32 == 0"
        assert self.H % (1 << (levels - 1)) == 0 and self.W % (1 << (levels - 1)) == 0
        self._begin_specs(cin, cout)
        conv, norm, res = self._conv, self._norm, self._resblock

        def att(pre, x):                                  # AttentionBlock (unet6.py:296-333)
            C = x.C
            nrm = norm(pre + ".norm", x, None, False)
            qkv = conv(pre + ".project_in", nrm, None, 3 * C, k=1)
            o = self._act(pre + ".attn", x.H, x.W, C)
            self.specs.append(_AttnCore(self, qkv, o))
            return conv(pre + ".project_out", o, None, C, k=1, resid=x)

        def block(pre, x0, x1, Cout, a):
            if a:
                return att(pre + ".1", res(pre + ".0", x0, x1, Cout))
            return res(pre, x0, x1, Cout)

        self.temb_dim = temb
        self.temb_spec = _Temb(self, hid, temb, 0)
        self.specs.append(self.temb_spec)
        self.x_in = self._act("x_in", self.H, self.W, self.cin_p, needs_grad=False)
        hs = [conv("in_conv", self.x_in, None, hid, rshape=(hid, cin, 3, 3))]
        for l in range(levels):                           # unet6.py:484-491
            cur = mult[l] * hid
            for j in range(nres):
                hs.append(block(f"downsamples.level_{l}.{j}", hs[-1], None, cur, attn[l]))
            if l != levels - 1 and self.resample_with_conv:
                hs.append(conv(f"downsamples.level_{l}.{nres}.1", hs[-1], None, cur, stride=2))
            elif l != levels - 1:                         # unet6.py:441-442
                hs.append(self._resample("avgpool2", f"downsamples.level_{l}.{nres}", hs[-1]))
        h = res("middle.0", hs[-1], None, hs[-1].C)       # unet6.py:494
        h = att("middle.1", h)
        h = res("middle.2", h, None, h.C)
        for l in range(levels - 1, -1, -1):               # unet6.py:497-503
            cur = mult[l] * hid
            for j in range(nres + 1):
                h = block(f"upsamples.level_{l}.{j}", h, hs.pop(), cur, attn[l])
            if l != 0 and self.resample_with_conv:
                h = conv(f"upsamples.level_{l}.{nres + 1}.1", h, None, cur, ups=1)
            elif l != 0:                                  # unet6.py:472-475
                h = self._resample("nearest2", f"upsamples.level_{l}.{nres + 1}", h)
        assert not hs
        h = norm("out_conv.0", h, None, True)             # unet6.py:505
        self.y_out = conv("out_conv.2", h, None, self.cout_p, rshape=(cout, hid, 3, 3))
        self.temb_spec.fc_total = self.fc_total

    def _plan(self):
        """Fix every launch decision before anything is recorded: each is a function of geometry, dtype and constructor flags alone
        (host predicates of the library on dummy non-null pointers -- no device, no allocation, so a `_dry` net can be planned too).
        fwd() / bwd() read these fields and assign none of them; the library checks every fused descriptor again at launch."""
        bf16, split = self.dt == BF16, self.grad_products == "split"
        convs = [s for s in self.specs if isinstance(s, _Conv)]
        readers = lambda act: [s for s in self.specs if isinstance(s, (_Conv, _Norm)) and
                               (s.src0 is act or s.src1 is act or (isinstance(s, _Conv) and s.resid is act))]
        # ---- forward
        for s in self.specs:
            if isinstance(s, _AttnCore):
                L, C = s.qkv.P, s.out.C
                s.mode = ("fused" if ops.attn_supported(self.dt, L, C) else
                          "f32_small" if self.dt == F32 and ops.attn_f32_small_supported(L, C) else "unfused")
            elif isinstance(s, _Temb):
                s.skinny = s._skinny()
        for prev, nm in zip(self.specs, self.specs[1:]):    # a norm as the epilogue of the conv right before it (4x4 / 8x8 maps)
            if (bf16 and isinstance(nm, _Norm) and nm.src1 is None and isinstance(prev, _Conv) and prev.out is nm.src0
                    and nm.drop_base is None            # a dropout site stays a launch: the conv epilogues know no dropout
                    and ops.conv_fwd_can_fuse_gn(self.dt, prev.g)):
                prev.gn_fwd, nm.fwd_fused = nm, True
        pairs = [b for b in self.blocks if self.pair_convs and b.paired and b.skip is not None]
        for b in pairs:                                     # skip projection + conv1 as one launch
            b.skip.fwd_in_pair, b.conv1.fwd_mate = True, b.skip
        if self.uniform_t:                                  # forward-only: no backward decisions
            return
        # ---- backward
        for c in convs:
            c.sums = "wgrad" if bf16 and c.fc_slot is None else "colsum"
            wf = ops.wgrad_fields(self.dt, c.g, 16, 16, 16 if c.src1 else None, 16, dbias=16 if c.sums == "wgrad" else None)
            reason = {w: ops.split_grad_reason(c.g, w) for w in ("wgrad", "dgrad")} if split else {}
            c.wgrad = ("grouped" if bf16 and self.group_wgrads and _lib.wgrad_group_accepts(**wf) else
                       "split" if split and reason["wgrad"] is None else "single")
            if c.src0.needs_grad:
                c.dgrad = "t" if bf16 else "split" if split and reason["dgrad"] is None else "exact"
                nm = c.src0.norm_spec
                if (bf16 and nm is not None and nm.src1 is None and c.src1 is None and not c.g.ups and nm.drop_base is None
                        and ops.conv_dgrad_t_can_fuse_gn_bwd(self.dt, c.g)):
                    c.gn_bwd, nm.bwd_fused = nm, True
            c.grad_exact = {w: "exact:" + reason[w] for w, how in (("wgrad", c.wgrad), ("dgrad", c.dgrad))
                            if split and how in ("single", "exact")}
        for b in self.blocks:                               # norm2's backward also emits conv1's bias / time-embedding sums
            assert readers(b.conv1.out) == [b.norm2] and b.norm2.src1 is None and b.conv1.fc_slot is not None, b.conv1.name
            b.conv1.sums, b.norm2.sums_for = "norm", b.conv1
        for b in pairs:                                     # the skip projection's backward inside conv2's, data gradients paired
            if not b.conv2.g.ups:
                b.skip.bwd_in_pair, b.conv2.bwd_mate = True, b.skip
        for c in convs:                                     # a norm with several consumers: fused into all of them or into none
            nm = c.src0.norm_spec
            assert nm is None or not nm.bwd_fused or c.gn_bwd is nm, c.name

    def _declare_params(self):
        st = self.store
        self.temb_spec.declare(st)
        te = self.temb_dim
        for name, (slot, co) in self.fc_slots.items():
            st.declare(name + ".weight", "lin", (co, te), (co, te))
        for name, (slot, co) in self.fc_slots.items():
            st.declare(name + ".bias", "vec", (co,), (co,))
        for s in self.specs[1:]:
            s.declare(st)

    def _set_param_marks(self):
        """spec.param_lo = lowest flat-buffer offset whose gradient is final once the backward of that
        spec (and of everything after it) has run; parameter-less specs inherit their successor's."""
        st, lo = self.store, self.store.size
        for s in reversed(self.specs[1:]):
            key = s.name
            if key is not None and key + ".weight" in st.entries:
                lo = st.entries[key + ".weight"].off
            s.param_lo = lo
        self.temb_spec.param_lo = 0

    def reference_shapes(self):
        return OrderedDict((k, e.rshape) for k, e in self.store.entries.items())

    def reference_param_order(self):
        """The 304 keys in the order `model.parameters()` yields them upstream = module registration order
        (unet6.py:395-415: embed, in_conv, downsamples.level_0.., middle, upsamples.level_0.., out_conv; inside a
        ResidualBlock norm1, conv1, fc, norm2, conv2, skip (:349-354); AttentionBlock norm, project_in, project_out
        (:307-310)).  torch.optim state dicts index parameters by this order."""
        top = {"embed": 0, "in_conv": 1, "downsamples": 2, "middle": 3, "upsamples": 4, "out_conv": 5}
        member = {"norm1": 0, "conv1": 1, "fc": 2, "norm2": 3, "conv2": 4, "skip": 5, "norm": 0, "project_in": 1, "project_out": 2}

        def rank(key):
            parts = key.split(".")
            r = [top[parts[0]]]
            for q in parts[1:]:
                if q.startswith("level_"):
                    r.append(int(q[6:]))
                elif q.isdigit():
                    r.append(int(q))
                elif q in member:
                    r.append(member[q])
                elif q in ("weight", "bias"):
                    r.append(0 if q == "weight" else 1)
                else:
                    raise KeyError(key)
            return r
        return sorted(self.store.entries, key=rank)

    def alloc(self, shape, dtype):
        t = torch.zeros(tuple(shape), device=self.device, dtype=dtype)
        self._bufs.append(t)
        return t

    def scratch(self, numel):
        if self._scratch is None or self._scratch_n < numel:
            self._scratch = self.alloc((numel,), self.tdtype)
            self._scratch_n = numel
        return self._scratch

    def grad_for_write(self, act, want_add=False):
        """-> (grad tensor, acc, add): the caller writes grad = (acc ? grad : 0) + (add or 0) + its contribution.  `add` is a
        pending contribution (the untouched dy of a residual join, see _Conv.bwd); only callers that can add a second
        tensor ask for it (want_add: 1 = instead of an accumulate, 2 = also next to one), for the others it is folded in
        by a separate launch first."""
        if act.grad is None:
            act.grad = self.alloc((act.N, act.H, act.W, act.C), self.tdtype)
        add = None
        if act.pending_add is not None:
            pend, act.pending_add = act.pending_add, None
            if want_add == 2 or (want_add and not act.grad_written):
                add = pend                  # want_add == 2: the caller can add it NEXT TO an accumulate (two addends)
            else:
                ops.add3(self.dt, act.grad, pend, act.grad if act.grad_written else None)
                act.grad_written = True
        acc = 1 if act.grad_written else 0
        act.grad_written = True
        return act.grad, acc, add

    def grad_for_read(self, act):
        """The complete gradient of `act` (every consumer has contributed by now), pending contribution included."""
        if act.pending_add is not None:
            pend, act.pending_add = act.pending_add, None
            if not act.grad_written:
                act.grad, act.grad_written = pend, True      # sole contribution: alias it (read-only from here on)
            else:
                ops.add_(self.dt, act.grad, pend)
        assert act.grad_written, act.name
        return act.grad

    def wgrad_slab(self, numel):
        """A slice of the split-K arena for one grouped weight gradient (fp32 elements); sized on first use."""
        off = (self._slab_off + 63) // 64 * 64
        self._slab_off = off + numel
        if self._slab_arena is None or self._slab_off > self._slab_arena.numel():
            raise RuntimeError("wgrad slab arena too small")       # sized by _materialize from the same split rule
        return self._slab_arena[off:off + numel]

    def _flush_wgrads(self):
        """Emit the pending weight gradients as ONE grouped launch (+ one launch summing their split-K slabs).
        (TrainStep lifts these calls out of the captured chain and issues them on a second stream, next to the
        data-gradient chain that follows.)  -> True if something was launched."""
        if not self.pending_wgrads:
            return False
        grp = _lib.WgradGroup([wf for _, wf in self.pending_wgrads], self.device)
        self.wgrad_groups.append(grp)
        self.pending_wgrads = []
        grp.launch()
        return True

    def _materialize(self):
        st = self.store
        for a in self.acts:
            a.data = self.alloc((a.N, a.H, a.W, a.C), self.tdtype)
        names = list(self.fc_slots)
        e0, e1 = st.entries[names[0] + ".weight"], st.entries[names[0] + ".bias"]
        ft, te = self.fc_total, self.temb_dim
        assert all(co % 8 == 0 for _, co in self.fc_slots.values())
        self.fc_w, self.fc_gw = st.P[e0.off:e0.off + ft * te].view(ft, te), st.G[e0.off:e0.off + ft * te].view(ft, te)
        self.fc_b, self.fc_gb = st.P[e1.off:e1.off + ft], st.G[e1.off:e1.off + ft]
        self.fc_weight_names = [nm + ".weight" for nm in names]
        self.T_all = self.alloc((1 if self.uniform_t else self.N, ft), torch.float32)
        self.dT_all = self.alloc((self.N, ft), torch.float32)
        self.t_in = self.alloc((self.N,), torch.float32)
        cmax = max(a.C for a in self.acts)
        self.gn_ws = self.alloc((self.N * (64 * 32 + 4 * cmax),), torch.float32)     # fp32 GroupNorm backward: per-image partial sums, 3 N C floats
        # (mdm_groupnorm_bwd_ws_floats; no other kernel reads it.  The size dates from the pixel-chunked launches, which nothing dispatches, and
        # stays: it is part of every plan's buffer layout)
        # split-K partial slabs of the weight-gradient contractions: room for 16 splits of the largest filter
        wmax = max(s.g.taps * s.g.Cout * s.g.Cin for s in self.specs if isinstance(s, _Conv))
        self.splitk_ws = self.alloc((16 * wmax,), torch.float32)
        # grouped weight gradients: every split layer gets its own slice of one arena for its fp32 partial slabs
        self._slab_arena, self._slab_off = None, 0
        if self.dt == BF16 and self.group_wgrads:
            need = 0
            for sp in self.specs:
                if isinstance(sp, _Conv):
                    sk = ops.wgrad_group_split(sp.g)
                    if sk > 1:
                        need += (sk * sp.g.taps * sp.g.Cout * sp.g.Cin + 63) // 64 * 64 + 64
            if need:
                self._slab_arena = self.alloc((need,), torch.float32)
        self.x_nchw = self.alloc((self.N, self.cin, self.H, self.W), torch.float32)
        self.y_nchw = self.alloc((self.N, self.cout, self.H, self.W), torch.float32)

    def _record(self, emit):
        with _lib.Recording() as rec:
            emit()
        return rec

    def _emit_fwd(self):
        if self.drop_rate > 0:
            self.drop_rng.advance()     # first launch of the plan: the masks of this run (its backward draws them again from the same offset)
        for s in self.specs:
            s.fwd()

    def _emit_bwd(self):
        """Backward of everything after `y_out.grad` has been written by the caller's loss kernel."""
        self.y_out.grad = self.alloc((self.N, self.H, self.W, self.cout_p), self.tdtype)
        self.y_out.grad_written = True
        # bwd_marks[i] = (#launches emitted so far, lowest flat-buffer offset whose gradient is final): parameters are
        # declared in forward order, so once the backward of spec j AND the group holding its weight gradient have run,
        # every gradient at or above spec j's first parameter is complete (mdm.dist.GradComm cuts buckets there).
        # Weight gradients are collected and flushed as a group whenever they cover ~wgrad_group_bytes of gradient;
        # marks exist only at those flush points.
        self.bwd_marks = []
        covered = 0
        for s in reversed(self.specs):
            s.bwd()
            if isinstance(s, _Conv):
                covered += 4 * s.g.taps * s.g.Cout * s.g.Cin
            if covered >= self.wgrad_group_bytes or s is self.specs[1]:
                self._flush_wgrads()
                self.bwd_marks.append((len(_lib._recording.calls), s.param_lo))
                covered = 0
        assert not self.pending_wgrads
        self.bwd_marks.append((len(_lib._recording.calls), 0))
        for a in self.acts:
            assert a.pending_add is None, a.name

    def grad_products_table(self):
        """{conv name: {"dgrad": route, "wgrad": route}} of a grad_products="split" model: the mdm_gemm route its split data gradient
        took and the mdm_conv_wgrad_split route of its weight gradient, as of the last run of the backward plan ("pending" before the
        first), or "exact:<reason>" (ops.split_grad_reason: "channels", "stride2", "geometry") where that gradient stays exact fp32.
        A convolution whose input needs no gradient (the first of the net) has no "dgrad" entry.  {} for grad_products="exact"."""
        return {k: dict(v) for k, v in self.grad_routes.items()}

    def census(self):
        """Leaf-op output elements of ONE forward under the counting rule of SURVEY 8(d) (every
        reference leaf op writes its output once, no credit for fusion): convs/linears, GroupNorm and
        SiLU separately, the residual / time-embedding adds, channel concats, x2 upsamples, SamePad
        copies, and the attention scores, softmax, both einsum outputs and the `.contiguous()` copy."""
        a_out = 0
        for s in self.specs:
            if isinstance(s, _Conv):
                g, o = s.g, s.out
                n = o.N * o.H * o.W * o.C
                a_out += n
                if s.resid is not None:
                    a_out += n                              # x + skip (unet6.py:333, 362)
                if s.fc_slot is not None:
                    a_out += n + o.N * o.C                  # x += fc(silu(t_emb)) and the fc output
                if g.ups:
                    a_out += g.N * g.VH * g.VW * g.Cin      # nn.Upsample output
                if g.stride == 2:
                    a_out += g.N * (g.IH + 1) * (g.IW + 1) * g.Cin   # SamePad2d output
            elif isinstance(s, _Norm):
                o = s.out
                n = o.N * o.H * o.W * o.C
                a_out += n * (2 if s.silu else 1)
                if s.src1 is not None:
                    a_out += n                              # torch.cat output (unet6.py:501), read by norm1 and skip
            elif isinstance(s, _AttnCore):
                N, L, C = s.qkv.N, s.qkv.P, s.out.C
                a_out += 2 * N * L * L + 2 * N * L * C
            elif isinstance(s, _Resample):
                a_out += s.out.N * s.out.P * s.out.C         # nn.AvgPool2d / nn.Upsample output
            elif isinstance(s, _Temb):
                a_out += self.N * (s.hid + 4 * s.temb)
        return a_out

    # ---- reference-compatible surface -------------------------------------------
    def load_state_dict(self, sd):
        self.store.load_state_dict(sd)

    def state_dict(self):
        """Reference key grammar, reference shapes, `model.parameters()` order."""
        return self.store.state_dict(order=self.reference_param_order())

    def parameters(self):
        return [self.store.P]

    def num_parameters(self):
        n = 0
        for e in self.store.entries.values():
            k = 1
            for d in e.rshape:
                k *= d
            n += k
        return n

    def train(self, mode=True):
        """PyTorch's semantics: a plan drops iff the model is in training mode when it RUNS -- the control words are rewritten on the
        device, in stream order and without a host synchronisation, so recorded plans and captured graphs follow."""
        self.training = bool(mode)
        if self.drop_ctl is not None:
            self.drop_ctl.copy_(self._drop_ctl_modes[1 if mode else 0])
        return self

    def eval(self):
        return self.train(False)

    def zero_grad(self):
        self.store.G.zero_()

    def _build_zero_table(self):
        """(offset, length) pieces of G that the recorded backward ACCUMULATES into (atomics / += : biases, GroupNorm scales,
        any weight gradient that is not a single stored launch): what `emit_zero_grad` clears before a step.  The slots in
        `overwritten` are written whole by exactly one launch per step."""
        rows = []
        for name, e in self.store.entries.items():
            if name in self.overwritten:
                continue
            size = (e.n + 7) // 8 * 8
            for o in range(0, size, 4096):
                rows.append((e.off + o, min(4096, size - o)))
        self.zero_table = torch.tensor(rows, dtype=torch.int64, device=self.device) if rows else None
        self.zero_floats = sum(r[1] for r in rows)

    def emit_zero_grad(self):
        """Clear the accumulated gradient slots (launch, recordable): the per-step `optimizer.zero_grad()`."""
        if self.zero_table is None or self.zero_floats * 2 > self.store.size:
            ops.fill(self.store.G, 0.0)
        else:
            ops.fill_segments(self.store.G, self.zero_table, 0.0)

    def run_forward(self):
        """x_in (NHWC, padded) and t_in must already hold the inputs."""
        if not self.use_graph:
            self.forward_plan.run()
            return
        if self._graph_fwd is None:
            self._graph_fwd = _lib.GraphExec(self.forward_plan)
        self._graph_fwd.launch()

    def run_backward(self):
        """y_out.grad must hold dL/dpred.  Gradient slots listed in `overwritten` (the grouped bf16 weight gradients, the
        time-embedding weights) are STORED by this pass, every other slot (biases, GroupNorm scales, ungrouped weights) is
        accumulated into and must have been cleared first (`emit_zero_grad`): two backward passes without an optimizer step
        in between do NOT add up -- gradient accumulation goes through TrainStep, which sums whole gradient buffers."""
        if self.backward_plan is None:
            raise RuntimeError("a uniform_t plan is forward-only")
        self.backward_plan.run()

    def forward(self, x, t):
        """x: [N,C,H,W] fp32 (any device), t: [N] -> object with `.sample` [N,C_out,H,W] fp32 on the GPU
        (reference contract: trainer_masked_mean_shift.py:140, sampler.py:145)."""
        assert tuple(x.shape) == (self.N, self.cin, self.H, self.W), (tuple(x.shape), (self.N, self.cin, self.H, self.W))
        if self.uniform_t:
            tt = t.reshape(-1)
            assert bool((tt == tt[0]).all()), "this plan was built for ONE timestep per batch (uniform_t)"
        self.x_nchw.copy_(x.to(torch.float32), non_blocking=True)
        self.t_in.copy_(t.reshape(-1).to(torch.float32), non_blocking=True)
        ops.nchw_to_nhwc(self.dt, self.x_nchw, self.x_in.data, self.N, self.cin, self.H, self.W, self.cin_p)
        self.run_forward()
        ops.nhwc_to_nchw(self.dt, self.y_out.data, self.y_nchw, self.N, self.cout, self.H, self.W, self.cout_p)
        return SimpleNamespace(sample=self.y_nchw.clone())

    __call__ = forward
