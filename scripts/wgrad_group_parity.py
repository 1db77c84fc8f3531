#!/usr/bin/env python3
"""The schedule of grouped weight gradients over a fixed matrix of groups, as text and as one digest -- no GPU.

    python scripts/wgrad_group_parity.py [--out FILE] [--tree DIR]

Every group of the matrix is asked of `mdm_wgrad_group_schedule` at n_cu = 256 and n_cu = 8, with MDM_TAPS_MIN_SHARE unset and
forced to 0.  A case prints one header line (group, n_cu, min share, form, bytes of the device table, rows) and one line per
decoded table row (include/mdm_hip.h: queue, round, desc, kind, tile_or_item, k0, k1, slot).  The last line of the output is
the case count and the sha256 of everything before it; tests/test_wgrad_group_cpu.py pins both.

The groups:
  * `mixed240`: the 240 members of tests/test_kernels_gpu.py::test_grouped_weight_gradients_match_self_contained_ones (16 shapes,
    short items, more than 96 split members: the reduce table closes), `mixed16`: the 16 shapes once under the default split rule,
    `per_tap`: members no nine-tap kernel takes, `taps3`: three nine-tap members with cut tiles;
  * the per-flush groups of the bf16 nets of scripts/plan_fingerprint.py's matrix, from `_dry` nets: `UNet._plan()` says which
    convolutions are grouped, the flush rule of `UNet._emit_bwd` is restated below.  Pointers are dummies (never dereferenced).

MDM_LIB_PATH selects the library file, so a build of another commit that exports the same query can be compared: the digests of
two builds that plan alike are equal (profiles/r14_wgrad_group_plan.md).
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import os
import sys

PTR = 16
N_CUS = (256, 8)
MIN_SHARES = (None, 0)
# N, H, C0, C1, Cout, stride, ups: the shapes of test_grouped_weight_gradients_match_self_contained_ones
SHAPES = [(8, 8, 64, 0, 64, 1, 0), (8, 8, 64, 0, 128, 1, 0), (4, 16, 64, 64, 64, 1, 0), (4, 32, 128, 0, 128, 1, 0),
          (8, 16, 64, 0, 64, 2, 0), (4, 8, 64, 0, 64, 1, 1), (16, 4, 256, 0, 256, 1, 0),
          (4, 8, 64, 64, 128, 1, 0), (4, 16, 64, 64, 128, 1, 0), (2, 16, 128, 0, 128, 1, 1), (4, 4, 64, 0, 128, 1, 1),
          (2, 32, 64, 0, 256, 1, 0), (1, 64, 64, 64, 128, 1, 0), (2, 64, 128, 0, 128, 1, 0),
          (4, 16, 8, 0, 128, 1, 0), (4, 16, 128, 0, 8, 1, 0)]
TINY = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[False, True])
CFG4 = dict(in_channels=4, hid_channels=128, out_channels=4, ch_multipliers=[1, 2, 2, 2], num_res_blocks=2, apply_attn=[True] * 4)


def geom(ops, N, H, C0, C1, Cout, stride=1, ups=0, k=3):
    if k == 1:
        return ops.ConvGeom(N=N, IH=H, IW=H, C0=C0, C1=C1, Cout=Cout, KH=1, KW=1, pad_t=0, pad_l=0, pad_b=0, pad_r=0)
    pads = (1, 1, 1, 1) if stride == 1 else (0, 0, 1, 1)
    return ops.ConvGeom(N=N, IH=H, IW=H, C0=C0, C1=C1, Cout=Cout, stride=stride, pad_t=pads[0], pad_l=pads[1], pad_b=pads[2],
                        pad_r=pads[3], ups=ups)


def member(ops, g, splitk, acc=0, dbias=PTR):
    """Descriptor fields of one member on dummy pointers; a split member gets a workspace of its own."""
    wf = ops.wgrad_fields(1, g, PTR, PTR, PTR if g.C1 else None, PTR, dbias=dbias, acc=acc)
    wf["splitk"] = splitk
    if splitk > 1:
        wf["ws"], wf["ws_bytes"] = PTR, splitk * g.taps * g.Cout * g.Cin * 4
    return wf


def shape_groups(ops):
    mixed = []
    for rep in range(240):
        g = geom(ops, *SHAPES[rep % len(SHAPES)])
        mixed.append(member(ops, g, max(ops.wgrad_group_split(g, slabs_per_item=4), 1), acc=int(rep % 5 == 0)))
    yield "mixed240", mixed
    yield "mixed16", [member(ops, g, ops.wgrad_group_split(g)) for g in (geom(ops, *s) for s in SHAPES)]
    yield "per_tap", [member(ops, geom(ops, 4, 8, 64, 0, 64), 1), member(ops, geom(ops, 2, 16, 64, 0, 128, k=1), 1),
                      member(ops, geom(ops, 8, 16, 128, 0, 128), 4), member(ops, geom(ops, 8, 16, 64, 0, 64, stride=2), 2),
                      member(ops, geom(ops, 16, 4, 256, 0, 256), 1)]
    yield "taps3", [member(ops, geom(ops, 4, 8, 64, 64, 128), 1), member(ops, geom(ops, 2, 32, 64, 0, 256), 1),
                    member(ops, geom(ops, 4, 16, 8, 0, 128), 1)]


def net_groups(mdm, ops):
    """The groups `UNet._emit_bwd` flushes, from the plan of a `_dry` net (no device)."""
    from mdm.unet import _Conv
    from mdm.unet2d import UNet2D, my_model_config
    u6 = mdm.unet6_config
    nets = [("tiny_n4_16", mdm.UNet, TINY, 4, 16, {}), ("cfg2_n32", mdm.UNet, u6(32), 32, 32, {}),
            ("cfg2_n100", mdm.UNet, u6(32), 100, 32, {}), ("cfg3_n8", mdm.UNet, u6(64), 8, 64, {}),
            ("cfg4_n16", mdm.UNet, CFG4, 16, 32, {}), ("u128_n1", mdm.UNet, u6(128), 1, 128, {}),
            ("unet2d_n4", UNet2D, my_model_config(3, 32, num_attention=1), 4, 32, {}),
            ("cfg2_n32_32MiB", mdm.UNet, u6(32), 32, 32, dict(wgrad_group_bytes=32 << 20))]
    for name, cls, cfg, n, hw, kw in nets:
        net = cls(cfg, n, hw, hw, dtype=mdm.BF16, _dry=True, **kw)
        net._plan()
        pending, covered, k = [], 0, 0
        for s in reversed(net.specs):
            if isinstance(s, _Conv):
                if s.wgrad == "grouped":
                    pending.append(member(ops, s.g, ops.wgrad_group_split(s.g), dbias=PTR if s.sums == "wgrad" else None))
                covered += 4 * s.g.taps * s.g.Cout * s.g.Cin
            if covered >= net.wgrad_group_bytes or s is net.specs[1]:
                if pending:
                    yield f"{name}#{k}", pending
                    k += 1
                pending, covered = [], 0
        assert not pending, name


def groups(mdm, ops):
    yield from shape_groups(ops)
    yield from net_groups(mdm, ops)


@contextlib.contextmanager
def min_share(value):
    old = os.environ.get("MDM_TAPS_MIN_SHARE")
    if value is None:
        os.environ.pop("MDM_TAPS_MIN_SHARE", None)
    else:
        os.environ["MDM_TAPS_MIN_SHARE"] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MDM_TAPS_MIN_SHARE", None)
        else:
            os.environ["MDM_TAPS_MIN_SHARE"] = old


def sweep(_lib, mdm, ops):
    """-> (number of cases, output lines)"""
    lines, cases = [], 0
    for name, fields in groups(mdm, ops):
        for n_cu in N_CUS:
            for ms in MIN_SHARES:
                with min_share(ms):
                    rows, need, form = _lib.wgrad_group_schedule(fields, n_cu)
                cases += 1
                lines.append(f"{name} members={len(fields)} n_cu={n_cu} min_share={ms} form={form} need={need} rows={len(rows)}")
                lines += [" ".join(map(str, r)) for r in rows]
    return cases, lines


def digest(lines):
    return hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="write the lines here instead of stdout")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import mdm from (default: the one this script lies in)")
    opt = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(opt.tree), "masked-diffusion-model_amd"))
    import mdm
    from mdm import _lib, ops
    cases, lines = sweep(_lib, mdm, ops)
    tail = f"{cases} cases, {len(lines)} lines, sha256 {digest(lines)}"
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(tail)
    else:
        print("\n".join(lines + [tail]))


if __name__ == "__main__":
    main()
