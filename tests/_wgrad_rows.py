"""Rows of the weight-gradient bound tests (test_wgrad_bounds_cpu.py proves on the host that the rows reach what they claim,
test_wgrad_bounds_gpu.py runs them): the members of three grouped launches (mdm_wgrad_group_*: wgrad_taps_group_kernel /
wgrad_taps_body, tile_parts_reduce_kernel, the per-tap items that ride in its queues, wgrad_group_kernel,
splitk_reduce_batched_kernel) and the edges of mdm_conv_wgrad_split (wgrad_split_kernel<64> / <128>, splitk_reduce_kernel).

Helpers only.  Descriptors are built over ops.wgrad_fields, with tensors for a launch or with dummy non-null pointers for the host
questions (mdm_wgrad_group_schedule, mdm_conv_wgrad_split_plan never dereference a pointer).  References are conv_wgrad_ref and
epilogue_ref of tests/_bounds.py, the per-element bound is `check`'s:

    |y - ref| <= u |ref| + (1 + u) ((k_terms + 8) 2^-23 + [split] 2^-15) mag,   u = 2^-24, k_terms = N OH OW

(`mag` = the same sum over absolute values).  It does not depend on the order of summation, so it holds for a tile summed in one
pass, for one cut into slots, for the split-K slabs and for the fp32 atomics of the bias gradient alike.

`wgrad_flat` restates the nine-tap gradient the way the kernel indexes it -- pixels flat over (image, row, column), tap (ty, tx)
at flat offset (ty - 1) W + (tx - 1), masked at the image's edges -- in fp64, with a fault planted on request: what a wrong mask,
a dropped or doubled slab, a wrong source at a concat boundary or a wrong upsample row would compute.
"""
import torch

from _bounds import SPLIT_PRODUCT, U_F32, conv_wgrad_ref, epilogue_ref

F32_BF16_BAR = 1e-6           # REL_BAR["f32_bf16"] of test_gemm_routes_gpu.py
F32_SPLIT_BAR = 1.8e-5        # REL_BAR["f32_split"] of test_gemm_routes_gpu.py
Q, RND, DESC, KIND, ITEM, K0, K1, SLOT = range(8)          # a row of mdm_wgrad_group_schedule
GK_64, GK_128, GK_256x128, GK_TAPS = range(4)
TAPS_BM, TAPS_BN = 128, 64
SLOT_BYTES, PART_TILE_BYTES = 9 * TAPS_BM * TAPS_BN * 4, 48


def M(N, IH, IW, C0, C1, Co, k=3, stride=1, ups=0, dbias=0, acc=0, splitk=1):
    """One member: bf16, 3x3 stride 1 pad 1 unless said otherwise; splitk > 1 comes with a workspace of its own."""
    return dict(N=N, IH=IH, IW=IW, C0=C0, C1=C1, Co=Co, k=k, stride=stride, ups=ups, dbias=dbias, acc=acc, splitk=splitk)


GROUPS = {
    "edges": [M(2, 32, 32, 64, 0, 128), M(1, 16, 16, 64, 0, 128, ups=1), M(4, 16, 8, 40, 24, 128), M(16, 2, 32, 64, 0, 64),
              M(4, 16, 16, 8, 0, 128), M(4, 16, 16, 128, 0, 8, dbias=1), M(2, 16, 16, 64, 64, 256, dbias=1)],
    "wide": [M(1, 64, 64, 64, 0, 128), M(8, 2, 64, 64, 0, 128, dbias=1), M(8, 16, 8, 64, 0, 128)],
    "riders": [M(2, 32, 32, 64, 0, 128, dbias=1), M(2, 16, 16, 64, 0, 128, k=1), M(8, 16, 16, 64, 0, 64, stride=2),
               M(16, 4, 4, 256, 0, 256), M(4, 8, 8, 64, 0, 64, acc=1), M(8, 16, 16, 128, 0, 128, splitk=4, acc=1),
               M(4, 16, 16, 64, 0, 64, splitk=2)],
}
RIDERS_NINE_TAP = (0, 6)      # the members of `riders` the nine-tap kernel takes
# the per-tap form (wgrad_group_kernel + splitk_reduce_batched_kernel): `riders` without its nine-tap-eligible members, and all of
# `riders` below the default share (its split member 6 then keeps its two slabs: a batched reduce with acc0 = 0 beside acc0 = 1)
GROUPS["riders_per_tap"] = [m for i, m in enumerate(GROUPS["riders"]) if i not in RIDERS_NINE_TAP]
GROUPS["riders_all_per_tap"] = GROUPS["riders"]
# (group, queues of the persistent launch, route)
MERGED_RUNS = [("edges", 8, "wgrad_taps_group"), ("edges", 24, "wgrad_taps_group"), ("wide", 8, "wgrad_taps_group"),
               ("wide", 16, "wgrad_taps_group"), ("riders", 8, "wgrad_taps_group+splitk")]
PER_TAP_RUNS = [("riders_per_tap", "wgrad_group+splitk"), ("riders_all_per_tap", "wgrad_group+splitk")]


def geom(m):
    from mdm import ops
    k, s = m["k"], m["stride"]
    pads = (0, 0, 0, 0) if k == 1 else (0, 0, 1, 1) if s == 2 else (1, 1, 1, 1)
    return ops.ConvGeom(N=m["N"], IH=m["IH"], IW=m["IW"], C0=m["C0"], C1=m["C1"], Cout=m["Co"], KH=k, KW=k, stride=s,
                        pad_t=pads[0], pad_l=pads[1], pad_b=pads[2], pad_r=pads[3], ups=m["ups"])


def pads_of(g):
    return (g.pad_t, g.pad_l, g.pad_b, g.pad_r)


def ws_floats(m):
    g = geom(m)
    return m["splitk"] * g.taps * g.Cout * g.Cin if m["splitk"] > 1 else 0


def member_fields(m, dy=16, x0=16, x1=16, dw=16, db=16, ws=16):
    """Descriptor fields of member `m`: tensors, or the default dummy pointers (host questions only)."""
    from mdm import ops
    g = geom(m)
    f = ops.wgrad_fields(1, g, dy, x0, x1 if g.C1 else None, dw, splitk=m["splitk"], dbias=db if m["dbias"] else None, acc=m["acc"])
    if m["splitk"] > 1:
        f["ws"], f["ws_bytes"] = ws, ws_floats(m) * 4
    return f


def group_fields(name):
    return [member_fields(m) for m in GROUPS[name]]


def slabs(m):
    g = geom(m)
    return g.N * g.OH * g.OW // 64


def slabs_per_image(m):
    g = geom(m)
    return g.OH * g.OW / 64.0          # below 1: several images per slab


def tiles_of(rows):
    """{(desc, tile): the nine-tap parts of that tile in slab order}"""
    t = {}
    for r in rows:
        if r[DESC] >= 0 and r[KIND] == GK_TAPS:
            t.setdefault((r[DESC], r[ITEM]), []).append(r)
    for parts in t.values():
        parts.sort(key=lambda r: r[K0])
    return t


def cuts_of(rows):
    """{desc: sorted slab indices at which a tile of that member is cut}"""
    c = {}
    for (d, _), parts in tiles_of(rows).items():
        for r in parts[1:]:
            c.setdefault(d, set()).add(r[K0])
    return {d: sorted(v) for d, v in c.items()}


def slots_at(n_desc, rows, need, desc_size):
    """(offset, bytes) of the slot section of the device table, by the layout include/mdm_hip.h documents: descriptors | (flat
    items) | taps table | part tiles | slots, every section but the last padded to 256 bytes."""
    pad = lambda v: (v + 255) // 256 * 256
    cut = sum(len(p) > 1 for p in tiles_of(rows).values())
    nslots = max([r[SLOT] for r in rows] + [0])
    at = pad(n_desc * desc_size) + pad(len(rows) * 16) + pad(cut * PART_TILE_BYTES)
    assert at + nslots * SLOT_BYTES == need, (at, nslots, need)
    return at, nslots * SLOT_BYTES


# ------------------------------------------------------------------ operands and references (CPU, computed once per group)
_draws, _refs = {}, {}


def bound_of(ref, mag, k_terms, split=False):
    """The per-element bound tensor `check(..., k_terms, "f32", split)` of tests/_bounds.py holds y to."""
    gamma = (k_terms + 8) * 2.0 ** -23 + (SPLIT_PRODUCT if split else 0.0)
    return U_F32 * ref.double().abs() + (1 + U_F32) * gamma * mag.double()


def _draw(shape, gen, dtype):
    return torch.randn(*shape, generator=gen).to(dtype)


def member_draw(m, seed, dtype=torch.bfloat16):
    """dy, x0, x1 in `dtype`, the fp32 prior of dw (acc members) and of dbias (it accumulates), all on the CPU."""
    g = geom(m)
    gen = torch.Generator().manual_seed(seed)
    return dict(g=g, dy=_draw((g.N, g.OH, g.OW, g.Cout), gen, dtype), x0=_draw((g.N, g.IH, g.IW, g.C0), gen, dtype),
                x1=_draw((g.N, g.IH, g.IW, g.C1), gen, dtype) if g.C1 else None,
                prior=_draw((g.taps, g.Cout, g.Cin), gen, torch.float32) if m["acc"] else None,
                dbprior=_draw((g.Cout,), gen, torch.float32) if m["dbias"] else None)


def member_ref(m, d):
    """-> dict(dw=(ref, mag), db=(ref, mag) or None, K): fp64 references of what the launch leaves in dw / dbias, priors included."""
    g = d["g"]
    a, mg, (s, sa) = conv_wgrad_ref(d["dy"], d["x0"], d["x1"], g.KH, g.KW, g.stride, pads_of(g), g.ups)
    pr = d["prior"].reshape(-1, g.Cin) if d["prior"] is not None else None
    ref, mag = epilogue_ref(a.reshape(-1, g.Cin), mg.reshape(-1, g.Cin), prior=pr)
    out = dict(dw=(ref.reshape(a.shape), mag.reshape(a.shape)), db=None, K=g.N * g.OH * g.OW)
    if d["dbprior"] is not None:
        p = d["dbprior"].double()
        out["db"] = (s + p, sa + p.abs())
    return out


def group_draws(name):
    """The operands of a group: the same for every queue count it runs at."""
    base = {"riders_per_tap": "riders", "riders_all_per_tap": "riders"}.get(name, name)
    if base not in _draws:
        _draws[base] = [member_draw(m, 7000 + 100 * sorted(GROUPS).index(base) + i) for i, m in enumerate(GROUPS[base])]
    if name == "riders_per_tap":
        return [d for i, d in enumerate(_draws[base]) if i not in RIDERS_NINE_TAP]
    return _draws[base]


def group_refs(name):
    base = {"riders_per_tap": "riders", "riders_all_per_tap": "riders"}.get(name, name)
    if base not in _refs:
        _refs[base] = [member_ref(m, d) for m, d in zip(GROUPS[base], group_draws(base))]
    if name == "riders_per_tap":
        return [r for i, r in enumerate(_refs[base]) if i not in RIDERS_NINE_TAP]
    return _refs[base]


# ------------------------------------------------------------------ mdm_conv_wgrad_split rows
def S(geometry, route, plan, ws_bytes=0, splitk=0, **over):
    """geometry = (N, IH, IW, C0, C1, Cout[, k, stride, ups] as keywords of M); `over`: descriptor fields that are overridden
    (lda, ld0, ldd0 + dtap); ws_bytes: the workspace handed in, exactly."""
    return dict(m=geometry, route="wgrad_split" + route, plan=plan, ws_bytes=ws_bytes, splitk=splitk, over=over)


_W16 = M(4, 16, 16, 64, 0, 64)
_SLAB16 = 9 * 64 * 64 * 4
SPLIT_ROWS = {
    "bt64": S(M(3, 8, 8, 64, 0, 64), "<64>", (1, 0)),
    "bt64_ragged_splitk": S(M(4, 16, 16, 96, 0, 64), "<64>+splitk", (4, 884736), ws_bytes=884736),
    "k_tail_48": S(M(3, 4, 4, 64, 0, 64), "<64>", (1, 0)),
    "k_tail_80": S(M(5, 4, 4, 64, 0, 64), "<64>", (1, 0)),
    "k_16": S(M(1, 4, 4, 64, 0, 64), "<64>", (1, 0)),
    "k_16_1x1": S(M(1, 4, 4, 32, 0, 32, k=1), "<64>", (1, 0)),
    "bt128_ragged": S(M(2, 8, 8, 136, 0, 160), "<128>", (1, 0)),
    "concat_36_28": S(M(2, 8, 8, 36, 28, 64), "<64>", (1, 0)),
    "cin8": S(M(4, 8, 8, 8, 0, 64), "<64>", (1, 0)),
    "cout8": S(M(4, 8, 8, 64, 0, 8), "<64>", (1, 0)),
    "explicit3": S(M(5, 8, 8, 64, 0, 64), "<64>+splitk", (3, 442368), ws_bytes=442368, splitk=3),
    "ws_cap": S(_W16, "<64>+splitk", (2, 2 * _SLAB16), ws_bytes=2 * _SLAB16),
    "ws_below_two": S(_W16, "<64>", (1, 0), ws_bytes=2 * _SLAB16 - 4),
    "non_dense": S(_W16, "<64>", (1, 0), ws_bytes=4 * _SLAB16, ldd0=80, dtap=64 * 80),
    "stride2": S(M(3, 8, 8, 64, 0, 64, stride=2), "<64>", (1, 0)),
    "ups": S(M(3, 4, 4, 64, 0, 64, ups=1), "<64>", (1, 0)),
    "pitched_lda": S(M(3, 8, 8, 64, 0, 64), "<64>", (1, 0), lda=96),
    "pitched_ld0": S(M(3, 8, 8, 64, 0, 64), "<64>", (1, 0), ld0=72),
}
assert _SLAB16 * 2 == 294912


def split_fields(row, dy=16, x0=16, x1=16, dw=16, ws=16, acc=0):
    """Descriptor fields of mdm_conv_wgrad_split for a row: tensors, or the default dummy pointers (plan only)."""
    from mdm import ops
    g = geom(row["m"])
    f = ops.wgrad_fields(0, g, dy, x0, x1 if g.C1 else None, dw, splitk=row["splitk"], acc=acc)
    f.pop("dbias")
    f.pop("_flops")
    if row["ws_bytes"]:
        f["ws"], f["ws_bytes"] = ws, row["ws_bytes"]
    f.update(row["over"])
    return f


_split_refs = {}


def split_draw_and_ref(name):
    """(draw, {acc: (ref, mag)}, K) of a split row, fp32 operands; computed once."""
    if name not in _split_refs:
        m = SPLIT_ROWS[name]["m"]
        d = member_draw(dict(m, acc=1), 9000 + sorted(SPLIT_ROWS).index(name), torch.float32)
        g = d["g"]
        a, mg, _ = conv_wgrad_ref(d["dy"], d["x0"], d["x1"], g.KH, g.KW, g.stride, pads_of(g), g.ups)
        with_prior = epilogue_ref(a.reshape(-1, g.Cin), mg.reshape(-1, g.Cin), prior=d["prior"].reshape(-1, g.Cin))
        _split_refs[name] = (d, {0: (a, mg), 1: tuple(t.reshape(a.shape) for t in with_prior)}, g.N * g.OH * g.OW)
    return _split_refs[name]


# ------------------------------------------------------------------ the nine-tap gradient as the kernel indexes it, with faults
def wgrad_flat(dy, x0, x1, ups=0, fault=None, slab=1, part=(0, 1)):
    """fp64 (dW[9][Cout][Cin], dbias[Cout]) of a 3x3 stride-1 pad-1 convolution over flat pixels p = (image, row, column): tap
    (ty, tx) multiplies dy[p] with the (virtual) input at p + (ty - 1) W + (tx - 1) where that pixel lies in the same image row
    range, 0 elsewhere.  fault:
      x_mask         the left-neighbour taps (tx = 0) lose their x mask: column 0 reads the last pixel of the previous row
      y_mask         the up-neighbour taps (ty = 0) lose their y mask at the first row of every image but the first: they read the
                     last row of the previous image
      slab_dropped   the 64 pixels of slab `slab` are left out;  slab_twice: counted twice
      concat_source  the eight channels from C0 on are read from source 0 past its C0 channels (the next pixel's first eight)
      ups_row        the folded upsample reads physical row (vy + 1) >> 1 instead of vy >> 1
      dbias_part     the bias gradient misses the slabs [part[0], part[1])
    """
    dy, x0 = dy.double(), x0.double()
    x1 = x1.double() if x1 is not None else None
    N, IH, IW, C0 = x0.shape
    if fault == "concat_source":
        assert x1 is not None and x1.shape[-1] >= 8
        flat0 = torch.cat([x0.reshape(-1), torch.zeros(8, dtype=torch.float64)])
        at = (torch.arange(N * IH * IW) * C0 + C0)[:, None] + torch.arange(8)[None, :]
        x1 = x1.clone()
        x1[..., :8] = flat0[at].reshape(N, IH, IW, 8)
    x = torch.cat([x0, x1], -1) if x1 is not None else x0
    if ups:
        vy = torch.arange(2 * IH)
        py = ((vy + 1) >> 1).clamp(max=IH - 1) if fault == "ups_row" else vy >> 1
        x = x[:, py][:, :, torch.arange(2 * IW) >> 1]
    _, H, W, Ci = x.shape
    Co = dy.shape[-1]
    assert dy.shape[:3] == x.shape[:3]
    P = N * H * W
    p = torch.arange(P)
    ox, oy, img = p % W, (p // W) % H, p // (W * H)
    wgt = torch.ones(P, dtype=torch.float64)
    if fault == "slab_dropped":
        wgt[64 * slab:64 * slab + 64] = 0
    if fault == "slab_twice":
        wgt[64 * slab:64 * slab + 64] = 2
    dyf, xf = dy.reshape(P, Co) * wgt[:, None], x.reshape(P, Ci)
    dw = torch.zeros(9, Co, Ci, dtype=torch.float64)
    for ty in range(3):
        for tx in range(3):
            ok_x = (ox + tx - 1 >= 0) & (ox + tx - 1 < W)
            ok_y = (oy + ty - 1 >= 0) & (oy + ty - 1 < H)
            if fault == "x_mask" and tx == 0:
                ok_x = torch.ones(P, dtype=torch.bool)
            if fault == "y_mask" and ty == 0:
                ok_y = ok_y | ((oy == 0) & (img > 0))
            src = p + (ty - 1) * W + (tx - 1)
            ok = ok_x & ok_y & (src >= 0) & (src < P)
            xg = xf[src.clamp(0, P - 1)] * ok[:, None].double()
            dw[ty * 3 + tx] = dyf.t() @ xg
    bw = torch.ones(P, dtype=torch.float64)
    if fault == "dbias_part":
        bw[64 * part[0]:64 * part[1]] = 0
    return dw, (dy.reshape(P, Co) * bw[:, None]).sum(0)
