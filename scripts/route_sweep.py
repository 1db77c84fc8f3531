#!/usr/bin/env python3
"""Differential sweep of the host-side dispatch of mdm_gemm: what the library decides for a fixed grid of descriptors.

    python scripts/route_sweep.py [--out FILE] [--tree DIR]            # one line per case
    python scripts/route_sweep.py --reasons [--out FILE] [--tree DIR]  # ops.split_grad_reason over the sweep's conv geometries
    python scripts/route_sweep.py --launch [--out FILE] [--tree DIR]   # mdm_gemm_launch_of / _pair_launch_of: the planned geometry

One line per case: the case, `mdm_gemm_route_of`, `mdm_gemm_plan` (split count, workspace bytes), `mdm_gemm_can_fuse_gn_fwd` and
`_bwd` (G = 32); for a pair of convolutions `mdm_gemm_pair_route_of`.  Everything asked is host arithmetic on the descriptor: no GPU,
pointers are dummies.  MDM_LIB_PATH selects the library file, so the same script run on two builds gives two files that are
byte-identical where the two builds decide the same (`cmp a.txt b.txt`): does a refactor of the dispatch leave every choice as it
was?  The last line on stderr gives the case count, the sha256 of the output and the route names the sweep never saw
(tests/test_gemm_routes_cpu.py pins the digest).  `--tree DIR` imports `mdm` from another checkout.

The grid: dtype x the maps 4, 8, 16, 32, 64 (square), 12x12 and 64x32 x batch 1, 2, 4, 32, 100 x 1x1 / 3x3 / 3x3 stride 2 / folded
upsample / transposed shadow x source channels from CHANNELS (with and without a second source) x output channels drawn from
CHANNELS, each once with a workspace and no options and once with B_split, f32_split, ws, out_f32 and the fused GroupNorm epilogues
drawn; the layout-1 data gradient and the layout-2 weight gradient of the same sites; plain contractions in the three layouts; pairs
of a 3x3 and a 1x1 convolution.  Draws come from a fixed linear congruential generator, not from `random`.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import os
import sys

MAPS = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (12, 12), (64, 32)]
BATCHES = [1, 2, 4, 32, 100]
CHANNELS = [8, 16, 32, 64, 96, 128, 192, 256, 384, 512]
KINDS = ["k1", "k3", "k3s2", "ups", "t"]
PTR = 16                                     # a non-null pointer that is never dereferenced
NOT_FROM_MDM_GEMM = ("wgrad_group", "wgrad_taps_group")     # entry points of their own (mdm_wgrad_group_launch)


class Lcg:
    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        return (self.x >> 33) % n

    def pick(self, seq):
        return seq[self.below(len(seq))]


def geom(ops, kind, n, h, w, c0, c1, cout):
    """The ConvGeom of a site whose (virtual) input map is h x w."""
    if kind == "k1":
        return ops.ConvGeom(n, h, w, c0, c1, cout, KH=1, KW=1, pad_t=0, pad_l=0, pad_b=0, pad_r=0)
    if kind == "k3s2":
        return ops.ConvGeom(n, h, w, c0, c1, cout, stride=2, pad_t=0, pad_l=0)
    if kind == "ups":
        return ops.ConvGeom(n, h // 2, w // 2, c0, c1, cout, ups=1)
    return ops.ConvGeom(n, h, w, c0, c1, cout)


def geometries(ops):
    """(tag, kind, dtype, ConvGeom) of every convolution site of the grid, in a fixed order."""
    rng = Lcg(20251018)
    for dt in (1, 0):
        for h, w in MAPS:
            for n in BATCHES:
                for kind in KINDS:
                    for c0 in CHANNELS:
                        for c1 in (0, rng.pick(CHANNELS)):
                            if kind == "t" and c1:
                                continue                    # the transposed shadow has one source
                            cout = rng.pick(CHANNELS)
                            tag = f"{'bf16' if dt else 'f32'} {kind} {h}x{w} n{n} c{c0}+{c1}>{cout}"
                            yield tag, kind, dt, geom(ops, kind, n, h, w, c0, c1, cout)


def conv_cases(ops):
    """(tag, fields) / (tag, fields_a, fields_b) of the convolution descriptors."""
    rng = Lcg(3)
    for tag, kind, dt, g in geometries(ops):
        s1 = PTR if g.C1 else None
        if kind == "t":
            base = lambda: ops.conv_dgrad_t_fields(dt, g, PTR, PTR, PTR, 0)
        else:
            base = lambda: ops.conv_fwd_fields(dt, g, PTR, s1, PTR, PTR, PTR)
        f = base()
        f.update(ws=PTR, ws_bytes=1 << 40)
        yield f"{tag} ws", f
        f, opts = base(), []
        if rng.below(2):
            f.update(ws=PTR, ws_bytes=1 << 40); opts.append("ws")
        if rng.below(2) and not dt:
            f.update(B_split=PTR); opts.append("B_split")
        if rng.below(2) and not dt:
            f.update(f32_split=1); opts.append("f32_split")
        if rng.below(4) == 0:
            f.update(out_f32=1); opts.append("out_f32")
        if rng.below(3) == 0:
            G = rng.pick([32, 32, 8])
            if kind == "t":
                f.update(gnb_x=PTR, gnb_stats=PTR, gnb_gamma=PTR, gnb_beta=PTR, gnb_dgamma=PTR, gnb_dbeta=PTR, gnb_G=G, gnb_silu=1)
                opts.append(f"gnb{G}")
            else:
                f.update(gnf_out=PTR, gnf_gamma=PTR, gnf_beta=PTR, gnf_stats=PTR, gnf_G=G, gnf_silu=1, gnf_eps=1e-6)
                f.update(bias=None if rng.below(2) else PTR)
                opts.append(f"gnf{G}")
        yield f"{tag} {'+'.join(opts) or 'bare'}", f
        if kind in ("k1", "k3", "k3s2") and rng.below(3) == 0:
            # the data gradient through the untransposed filters (layout 1) and the weight gradient (layout 2) of the same site
            yield f"{tag} dgrad1", dict(dtype=dt, layout=1, M=g.N * g.VH * g.VW, N=g.Cin, K=g.taps * g.Cout, conv=1, OH=g.VH, OW=g.VW,
                                        IH=g.OH, IW=g.OW, KH=g.KH, KW=g.KW, stride=g.stride, pad_t=g.pad_t, pad_l=g.pad_l, transposed=1,
                                        C0=g.Cout, Ck=g.Cout, src0=PTR, ld0=g.Cout, B=PTR, ldb=g.Cin, wtap=g.Cout * g.Cin, D0=PTR,
                                        ldd0=g.C0, D1=s1, ldd1=g.C1, N0=g.C0)
        if kind != "t" and rng.below(3) == 0:
            f = ops.wgrad_fields(dt, g, PTR, PTR, s1, PTR, splitk=rng.pick([0, 0, 1, 4]))
            if rng.below(4):
                f.update(ws=PTR, ws_bytes=1 << 40)
            yield f"{tag} wgrad sk{f['splitk']}{' ws' if f['ws'] else ''}", f
        if kind == "k3" and not dt and rng.below(2):
            yield f"{tag} dgrad_split", ops.conv_dgrad_split_fields(g, PTR, PTR, PTR, 0, s1, 0)
        if kind in ("k3", "t") and rng.below(2):
            # a pair: this convolution next to the 1x1 convolution of the same source (forward), or of the same dY (backward)
            g1 = geom(ops, "k1", g.N, g.VH, g.VW, g.C0, g.C1, rng.pick([g.Cout, g.Cout, 64, 128]))
            if kind == "t":
                a, b = ops.conv_dgrad_t_fields(dt, g, PTR, PTR, PTR, 0), ops.conv_dgrad_t_fields(dt, g1, PTR, PTR, PTR, 0)
            else:
                a, b = base(), ops.conv_fwd_fields(dt, g1, PTR, s1, PTR, PTR, PTR)
            if rng.below(2):
                a.update(ws=PTR, ws_bytes=1 << 40); b.update(ws=PTR, ws_bytes=1 << 40)
            yield f"{tag} pair>{g1.Cout}{' ws' if a['ws'] else ''}", a, b
    # the fused GroupNorm epilogues (small maps, groups of 4 .. 64 channels) and the pairs of a residual block, bf16, in full
    for (h, w), n in ((m, n) for m in MAPS[:4] for n in BATCHES[2:]):
        for c0 in (64, 128, 256, 512):
            for cout in (64, 128, 256, 512):
                g = geom(ops, "k3", n, h, w, c0, 0, cout)
                for G in (32, 8, 4) if h <= 8 else ():
                    f = ops.conv_fwd_fields(1, g, PTR, None, PTR, PTR, PTR, ws=None,
                                            gnf=dict(out=PTR, gamma=PTR, beta=PTR, stats=PTR, G=G, silu=1))
                    yield f"bf16 k3 {h}x{w} n{n} c{c0}>{cout} gnf{G}", f
                    f = ops.conv_dgrad_t_fields(1, g, PTR, PTR, PTR, 0, gnb=dict(x=PTR, stats=PTR, gamma=PTR, beta=PTR, dgamma=PTR,
                                                                                 dbeta=PTR, G=G, silu=1))
                    yield f"bf16 t {h}x{w} n{n} c{c0}>{cout} gnb{G}", f
                for c1x1 in (64, 128, 256):
                    g1 = geom(ops, "k1", n, h, w, c0, 0, c1x1)
                    yield (f"bf16 k3 {h}x{w} n{n} c{c0}>{cout} pair>{c1x1}", ops.conv_fwd_fields(1, g, PTR, None, PTR, PTR, PTR),
                           ops.conv_fwd_fields(1, g1, PTR, None, PTR, PTR, PTR))


def plain_cases():
    rng = Lcg(7)
    for dt in (1, 0):
        for layout in (0, 1, 2):
            for M in (8, 32, 64, 104, 256, 4096):
                for N in (8, 64, 128, 512):
                    for K in (64, 128, 512, 2048):
                        for batch in (1, 4):
                            for splitk in (0, 1, 4):
                                lda, ldb = (K, K) if layout == 0 else (K, N) if layout == 1 else (M, N)
                                f = dict(dtype=dt, layout=layout, M=M, N=N, K=K, batch=batch, sA=M * K, sB=N * K, sD=M * N, A=PTR, lda=lda,
                                         B=PTR, ldb=ldb, D0=PTR, ldd0=N, N0=N, splitk=splitk)
                                opts = []
                                if rng.below(4):
                                    f.update(ws=PTR, ws_bytes=1 << 40); opts.append("ws")
                                if rng.below(2):
                                    f.update(out_f32=1); opts.append("out_f32")
                                if rng.below(2) and not dt:
                                    f.update(f32_split=1); opts.append("f32_split")
                                if rng.below(4) == 0:
                                    f.update(bias=PTR); opts.append("bias")
                                yield f"{'bf16' if dt else 'f32'} plain{layout} {M}x{N}x{K} b{batch} sk{splitk} {'+'.join(opts) or 'bare'}", f


def sweep(_lib, ops):
    """The output lines and the set of route names seen."""
    lib, seen, lines = _lib.load(), set(), []
    sk, nb = C.c_int32(), C.c_int64()

    def ask(fields):
        d = _lib._desc({k: v for k, v in fields.items() if k != "_flops"})
        route = lib.mdm_gemm_route_of(C.byref(d)).decode()
        plan = f"{sk.value},{nb.value}" if lib.mdm_gemm_plan(C.byref(d), C.byref(sk), C.byref(nb)) == 0 else "refused"
        seen.add(route)
        return d, f"{route} | {plan} | {lib.mdm_gemm_can_fuse_gn_fwd(C.byref(d), 32)}{lib.mdm_gemm_can_fuse_gn_bwd(C.byref(d), 32)}"

    cases = list(conv_cases(ops)) + list(plain_cases())
    for i, case in enumerate(cases):
        d, text = ask(case[1])
        if len(case) == 3:
            db, tb = ask(case[2])
            pair = lib.mdm_gemm_pair_route_of(C.byref(d), C.byref(db)).decode()
            seen.add(pair)
            text = f"{text} || {tb} || {pair}"
        lines.append(f"{i} {case[0]} | {text}")
    return lines, seen


def launches(_lib, ops):
    """One line per case of the sweep: the six numbers of `mdm_gemm_launch_of` (workgroups, grid z, threads, dynamic LDS bytes, tile
    rows, tile columns) or `refused`; for a pair those of `mdm_gemm_pair_launch_of`, or both members' where it runs as two launches."""
    show = lambda t: "refused" if t is None else " ".join(map(str, t))
    lines = []
    for i, case in enumerate(list(conv_cases(ops)) + list(plain_cases())):
        if len(case) == 3:
            t = _lib.pair_launch_of(dict(case[1]), dict(case[2]))
            text = show(t) if t is None or len(t) == 6 else f"two: {show(t[0])} || {show(t[1])}"
        else:
            text = show(_lib.launch_of(**case[1]))
        lines.append(f"{i} {case[0]} | {text}")
    return lines


def reasons(ops):
    """One line per distinct convolution geometry of the sweep: ops.split_grad_reason of its two gradients."""
    lines, done = [], set()
    for tag, kind, dt, g in geometries(ops):
        key = tag.split(" ", 1)[1]
        if kind != "t" and key not in done:
            done.add(key)
            lines.append(f"{key} | dgrad {ops.split_grad_reason(g, 'dgrad')} | wgrad {ops.split_grad_reason(g, 'wgrad')}")
    return lines


def digest(lines):
    return hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest()


def load(tree):
    sys.path.insert(0, os.path.join(os.path.abspath(tree), "masked-diffusion-model_amd"))
    from mdm import _lib, ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(tree)), ops.__file__
    return _lib, ops


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="write the lines here instead of stdout")
    ap.add_argument("--reasons", action="store_true", help="the split_grad_reason table instead of the routes")
    ap.add_argument("--launch", action="store_true", help="the planned launch geometry of every case instead of the routes")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import mdm from (default: the one this script lies in)")
    opt = ap.parse_args()
    _lib, ops = load(opt.tree)
    if opt.reasons:
        lines, note = reasons(ops), ""
    elif opt.launch:
        lines, note = launches(_lib, ops), ""
    else:
        lines, seen = sweep(_lib, ops)
        missing = [n for n in _lib.route_names() if n not in seen and n.split("+")[0] not in NOT_FROM_MDM_GEMM]
        note = f", {len(seen & set(_lib.route_names()))} route names seen, never seen: {missing}"
    out = open(opt.out, "w") if opt.out else sys.stdout
    out.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines, sha256 {digest(lines)}{note}", file=sys.stderr)


if __name__ == "__main__":
    main()
