"""Row tables of the store (csrc/optim.hip), loss / sampler (csrc/sched.hip) and evaluation (csrc/eval.hip) kernel tests, what draws
a row's problem, and a numpy fp32 emulation of each kernel's arithmetic with the faults a wrong kernel could make.  Shared by
tests/test_store_kernels_gpu.py, tests/test_loss_sampler_kernels_gpu.py and tests/test_eval_kernels_gpu.py (which run the rows on the
GPU) and by tests/test_store_rows_cpu.py (which emulates them without one).  Helpers only, no test functions; importable without a
GPU.  The bounds and references are in tests/_bounds.py (the section on these kernels)."""
import numpy as np
import torch

from _bounds import sqnorm_geom

f32, f64 = np.float32, np.float64
NAN = float("nan")
INF = float("inf")


def fma32(a, b, c):
    """fmaf in numpy: the fp64 product of two fp32 values is exact, the fp64 sum rounds to 53 bits, then once more to fp32"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def wave_sum32(a):
    """a [..., 64] fp32 -> [...]: v += shfl_xor(v, o) for o = 32 .. 1 (every lane ends with the same value: fp32 + commutes)"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    assert a.dtype == f32
    return a[..., 0]


def block_sum32(acc):
    """acc [blocks][256] fp32 -> [blocks]: wave sums, then (p0 + p1) + (p2 + p3)"""
    p = wave_sum32(acc.reshape(acc.shape[0], 4, 64))
    return (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])


# ------------------------------------------------------------------ mdm_sqnorm
CAP4 = 1024 * 256                                   # float4 one trip of the capped grid covers
SQNORM_NS = (1, 3, 4, 7, 1023, 1024, 1025 * 4 + 2, CAP4 * 4, CAP4 * 4 + 4, CAP4 * 4 + 7)
SQNORM_FAULTS = ("no_tail", "no_last_float4", "no_second_trip", "final_reads_all")


def sqnorm_row(n):
    g = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=g) * 0.7


def onehot_positions(n):
    """first, last, first and last element of the tail, last element of the float4 body, first element of the second trip"""
    n4 = n // 4
    pos = {0, n - 1}
    if n % 4:
        pos |= {4 * n4, n - 1}
    if n4:
        pos.add(4 * n4 - 1)
    if n4 > CAP4:
        pos.add(4 * CAP4)
    return sorted(pos)


def onehot(n, p):
    x = torch.zeros(n)
    x[p] = 3.0
    return x


def emulate_sqnorm(g, partials=None, fault=None):
    """-> (the word mdm_sqnorm stores, the module's partials array behind the call).  `partials`: that array before the call (zero
    when the module is loaded)."""
    g = np.asarray(g, f32).reshape(-1)
    n = g.size
    n4, nb, T = sqnorm_geom(n)
    threads = nb * 256
    body4 = n4 - (1 if fault == "no_last_float4" and n4 else 0)
    trips = min(T, 1) if fault == "no_second_trip" else T
    acc = np.zeros(threads, f32)
    for tr in range(trips):
        v = np.zeros((threads, 4), f32)
        m = max(0, min(body4 - tr * threads, threads))
        v[:m] = g[4 * tr * threads:4 * (tr * threads + m)].reshape(-1, 4)
        for c in range(4):
            acc = fma32(v[:, c], v[:, c], acc)              # a lane without a float4 adds 0 * 0: exact
    if fault != "no_tail":
        for i in range(4 * n4, n):
            acc[0] = fma32(g[i], g[i], acc[0])
    partials = np.zeros(1024, f32) if partials is None else partials.copy()
    partials[:nb] = block_sum32(acc.reshape(nb, 256))
    nblk = 1024 if fault == "final_reads_all" else nb
    a = np.zeros(256, f32)
    for i in range(0, nblk, 256):
        chunk = np.zeros(256, f32)
        m = min(256, nblk - i)
        chunk[:m] = partials[i:i + m]
        a = a + chunk
    return block_sum32(a.reshape(1, 256))[0], partials


# ------------------------------------------------------------------ mdm_cast_bf16, mdm_fill_f32, mdm_fill_segments_f32
FLAT_NS = (1, 255, 257, 2048 * 256 + 5)             # the last: past the 2048-workgroup cap, the second trip of the grid-stride loop
FILL_VALUES = (-0.0, 1.5, float(np.float32(3.0e-39)))
# fp32 bit patterns with a known bf16 rounding: ties to even in both directions, +-0, subnormals, the largest finite value (-> inf),
# +-inf, NaN (stays NaN)
CAST_EDGES = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x00000001, 0x00008000,
              0x00018000, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC01234]


def cast_row(n):
    """random fp32 bit patterns of every exponent with the edges cycled over the first positions and the last one"""
    g = torch.Generator().manual_seed(n)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    e = torch.tensor(CAST_EDGES, dtype=torch.int64)
    e = torch.where(e >= 2 ** 31, e - 2 ** 32, e).to(torch.int32)
    k = min(n, len(CAST_EDGES))
    bits[:k] = e[:k]
    bits[-1] = e[(n - 1) % len(CAST_EDGES)]
    return bits.view(torch.float32)


def cast_want(x, fault=None):
    """torch's .to(bfloat16) (round to nearest even, NaN stays NaN) -> int16 bits; fault "truncate": the low 16 bits dropped"""
    if fault == "truncate":
        return (x.view(torch.int32) >> 16).to(torch.int16)
    return x.to(torch.bfloat16).view(torch.int16)


def cast_matches(got, want, src):
    """int16 bits against torch's: equal wherever the source is a number; a NaN source must give a NaN (torch's CPU conversion makes
    every NaN 0x7FC0, the hardware keeps the sign and quiets the payload: the contract is that NaN stays NaN)"""
    nan = torch.isnan(src)
    isnan16 = (got.to(torch.int32) & 0x7FFF) > 0x7F80
    return torch.equal(got[~nan], want[~nan]) and bool(isnan16[nan].all())


# (offset, length) rows into one buffer: lengths {4, 8, 1024, 1028, 4096}, offsets multiples of 4, adjacent and non-adjacent
FILL_SEGS = [(0, 4), (4, 8), (12, 1024), (1040, 1028), (2068, 4096), (6400, 4), (6408, 4096), (10504, 1028), (12000, 8)]
FILL_SEG_SIZE = 12100


def check_zero_table(rows, entries, overwritten):
    """the contract between UNet._build_zero_table and fill_segments_kernel: every row 16-byte aligned, a multiple of 4 and at most
    4096 long, the rows disjoint, and their union exactly the (8-padded) slots of the entries not in `overwritten`"""
    rows = [(int(o), int(n)) for o, n in rows]
    for o, n in rows:
        assert o % 4 == 0 and n % 4 == 0 and 0 < n <= 4096, (o, n)
    srt = sorted(rows)
    for (o0, n0), (o1, _) in zip(srt, srt[1:]):
        assert o0 + n0 <= o1, ("overlap", o0, n0, o1)
    want = sorted((e.off, (e.n + 7) // 8 * 8) for name, e in entries.items() if name not in overwritten)
    merged = []
    for o, n in srt:                                   # the pieces of one slot are adjacent: merge and compare slot by slot
        if merged and merged[-1][0] + merged[-1][1] == o:
            merged[-1][1] += n
        else:
            merged.append([o, n])
    wm = []
    for o, n in want:
        if wm and wm[-1][0] + wm[-1][1] == o:
            wm[-1][1] += n
        else:
            wm.append([o, n])
    assert merged == wm, "the zero table does not cover exactly the accumulated slots"


# ------------------------------------------------------------------ mdm_transpose_shadow_bf16
TRANSPOSE_FILTERS = [(1, 8, 8), (9, 8, 128), (9, 128, 8), (1, 40, 24), (9, 64, 64), (9, 72, 136), (1, 200, 72)]     # (taps, Cout, Cin)
TRANSPOSE_GAP_AFTER = 3                             # a non-filter gap of 40 elements behind filter 3
TRANSPOSE_FAULTS = ("tap0_offset", "skip_partial_tile")


def pack_filters(shapes, gap_after=None, gap=40):
    """back to back (8-padded like ParamStore.declare) -> ([(off, taps, Cout, Cin)], total elements)"""
    out, n = [], 0
    for i, (t, co, ci) in enumerate(shapes):
        out.append((n, t, co, ci))
        n += (t * co * ci + 7) // 8 * 8
        if gap_after is not None and i == gap_after:
            n += gap
    return out, n


def transpose_tiles(filters, fault=None):
    """the tile table as ParamStore.allocate builds it: (element offset of the tap matrix, Cout, Cin, row0, col0) per 64 x 64 tile"""
    rows = []
    for off, taps, co, ci in filters:
        for tp in range(taps):
            for r0 in range(0, co, 64):
                for c0 in range(0, ci, 64):
                    if fault == "skip_partial_tile" and (r0 + 64 > co or c0 + 64 > ci):
                        continue
                    rows.append((off + (0 if fault == "tap0_offset" else tp) * co * ci, co, ci, r0, c0))
    return rows


def emulate_transpose(Pb, PT, tiles):
    """transpose_shadow_bf16_kernel tile by tile on int16 bits (numpy arrays; PT is written in place)"""
    for off, co, ci, r0, c0 in tiles:
        r1, c1 = min(r0 + 64, co), min(c0 + 64, ci)
        src = Pb[off:off + co * ci].reshape(co, ci)
        PT[off:off + co * ci].reshape(ci, co)[c0:c1, r0:r1] = src[r0:r1, c0:c1].T
    return PT


# ------------------------------------------------------------------ mdm_split_shadow, mdm_split_shadow_t
SPLIT_FILTERS = [(9, 64, 96), (9, 256, 256), (1, 32, 32)]      # the middle one: 589 824 elements, the second trip of the grid-stride loop
SPLIT_TRIP = 64 * 256 * 8                           # elements one trip of mdm_split_shadow's grid covers per segment
SPLIT_GAP_AFTER = 0


def split_problem():
    filters, n = pack_filters(SPLIT_FILTERS, SPLIT_GAP_AFTER, gap=72)
    g = torch.Generator().manual_seed(77)
    P = torch.randn(n, generator=g) * torch.logspace(-5, 3, n)[torch.randperm(n, generator=g)]
    return filters, n, P


def emulate_split(P, segs, fault=None):
    """-> {off: int16 bits} as _bounds.split_want; fault "no_second_trip": what lies behind the first trip of a segment is never
    written and still holds the destination's NaN fill"""
    from _bounds import split_want
    out = split_want(P, segs)
    if fault == "no_second_trip":
        for off, ln in segs:
            if ln > SPLIT_TRIP:
                out[off] = out[off].clone()
                out[off][2 * SPLIT_TRIP:] = 0x7FC0                 # a NaN-filled destination is still there
    return out


# ------------------------------------------------------------------ mdm_loss_fwd_bwd
LOSS_SHAPES = [(3, 3, 5, 5), (5, 1, 37, 37), (2, 3, 192, 192)]          # tests/test_monitor_gpu.py::test_loss_mon_kernel's
LOSS_CCP = {(3, 3, 5, 5): [(3, 8), (3, 16)], (5, 1, 37, 37): [(1, 8)], (2, 3, 192, 192): [(3, 8)], (2, 8, 9, 9): [(8, 8)]}
LOSS_ROWS = [(N, C, H, W, Cp, dt, ws, ww)
             for (N, _, H, W), ccp in LOSS_CCP.items() for C, Cp in ccp for dt in ("f32", "bf16")
             for ws, ww in ((0, 0), (1, 0), (0, 1), (1, 1))]
LOSS_GSCALE = 0.5
LOSS_FAULTS = ("x0_s_swapped", "no_gscale")
TD = {"f32": torch.float32, "bf16": torch.bfloat16}


def loss_id(r):
    N, C, H, W, Cp, dt, ws, ww = r
    return f"{N}x{C}x{H}x{W}-Cp{Cp}-{dt}{'-s' if ws else ''}{'-w' if ww else ''}"


def loss_problem(r):
    """-> dict(pred NHWC [N][H][W][Cp] in the storage type with NaN in its pad channels, x_in, x0, s | None, w | None)"""
    N, C, H, W, Cp, dt, ws, ww = r
    g = torch.Generator().manual_seed(N * 1000 + H + Cp)
    rn = lambda *sz: torch.randn(*sz, generator=g)
    pred = (rn(N, H, W, Cp) * 0.5).to(TD[dt])
    pred[..., C:] = NAN
    T = dict(pred=pred, x_in=rn(N, C, H, W) + 0.3, x0=rn(N, C, H, W))
    T["s"] = rn(N, C, H, W) * 0.4 + 0.1 if ws else None
    T["w"] = torch.rand(N, generator=g) + 0.5 if ww else None
    return T


def emulate_loss(r, T, fault=None):
    """-> (loss word (python int, Q23.40), flag word, dpred NHWC in the storage type) as loss_kernel forms them: the residual in the
    kernel's order, per-thread fmaf chains over (trip, channel), waves, the workgroup's four partials, x inv_numel, one rounding to
    Q23.40 per workgroup, integer adds"""
    from _bounds import dpred_want, loss_geom, loss_residual32
    N, C, H, W, Cp, dt, ws, ww = r
    HW = H * W
    if fault == "x0_s_swapped" and T["s"] is not None:
        r32 = loss_residual32(T["pred"], T["x_in"], T["x0"], T["s"], C)
    else:
        r32 = loss_residual32(T["pred"], T["x_in"], T["s"], T["x0"], C)
    dp = dpred_want(r32, T["w"], Cp, 1.0 if fault == "no_gscale" else LOSS_GSCALE, TD[dt])
    grid, trips = loss_geom(N, HW)
    threads = grid * 256
    rr = np.zeros((trips * threads, C), f32)
    rr[:N * HW] = r32.permute(0, 2, 3, 1).reshape(N * HW, C).numpy()               # pixel-major: pix = n HW + p
    wn = np.ones(trips * threads, f32)
    if T["w"] is not None:
        wn[:N * HW] = np.repeat(T["w"].numpy().astype(f32), HW)
    local = np.zeros(threads, f32)
    for tr in range(trips):
        sl = slice(tr * threads, (tr + 1) * threads)
        for c in range(C):
            local = fma32(wn[sl] * rr[sl, c], rr[sl, c], local)
    inv_numel = f32(1.0) / (f32(N) * f32(C) * f32(HW))
    v = block_sum32(local.reshape(grid, 256)) * inv_numel
    assert v.dtype == f32
    word, flag = 0, 0
    for x in v:
        if abs(x) < 4194304.0:
            word += int(np.rint(f64(x) * 2.0 ** 40))
        else:
            flag += 1
    return word, flag, dp


# ------------------------------------------------------------------ mdm_sampler_x0, mdm_sampler_update
SAMPLER_SHAPES = [(1, 1, 5, 51, 8), (2, 3, 8, 16, 8), (1, 8, 16, 16, 8), (100, 3, 32, 32, 8)]      # total 255, 768, 2048, the bench shape
# (dt, s, pred_nchw, shifted0 given): each optional operand NULL in some rows and given in others
SAMPLER_FORMS = [("f32", 1, 1, 1), ("bf16", 1, 0, 1), ("f32", 0, 1, 0), ("bf16", 0, 0, 0), ("bf16", 1, 1, 0), ("f32", 1, 0, 0)]
UPDATE_FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]      # (momentum, diff given)
SAMPLER_FAULTS = ("x0_plus_s", "momentum_inverted")


def sampler_problem(shape, dt):
    N, C, H, W, Cp = shape
    g = torch.Generator().manual_seed(N + 10 * C + H * W)
    pred = (torch.randn(N, H, W, Cp, generator=g) * 0.5).to(TD[dt])
    pred[..., C:] = NAN
    return dict(pred=pred, x_in=torch.randn(N, C, H, W, generator=g) + 0.3, s=torch.randn(N, C, H, W, generator=g) * 0.4 + 0.1,
                d_t=torch.randn(N, C, H, W, generator=g), d_next=torch.randn(N, C, H, W, generator=g),
                x_t=torch.randn(N, C, H, W, generator=g) * 0.7 - 0.2)


def emulate_sampler_x0(T, C, with_s, fault=None):
    from _bounds import sampler_x0_want
    pv, sh0, x0h = sampler_x0_want(T["pred"], T["x_in"], T["s"] if with_s else None, C)
    if fault == "x0_plus_s" and with_s:
        x0h = sh0 + T["s"]
    return pv, sh0, x0h


def emulate_sampler_update(T, momentum, fault=None):
    from _bounds import sampler_update_want
    return sampler_update_want(T["d_t"], T["d_next"], T["x_t"], (not momentum) if fault == "momentum_inverted" else momentum)


# ------------------------------------------------------------------ mdm_normalize01
NORM_ES = (1, 63, 256, 257, 3072)
NORM_KINDS = ("plain", "max_last", "min_last", "negative", "constant", "inf", "nan")
NORM_FAULTS = ("batch_min",)


def normalize_problem(E):
    """one image per kind, [len(NORM_KINDS)][E]"""
    g = torch.Generator().manual_seed(E)
    x = torch.randn(len(NORM_KINDS), E, generator=g) * 2.0 + 0.5
    k = NORM_KINDS.index
    x[k("max_last"), -1] = 50.0
    x[k("min_last"), -1] = -50.0
    x[k("negative")] = -x[k("negative")].abs() - 1.0
    x[k("constant")] = 0.3
    x[k("inf"), E // 2] = INF
    x[k("nan"), (2 * E) // 3] = NAN
    return x


def emulate_normalize01(x, fault=None):
    """numpy fp32: min / max that hand a NaN on, (x - lo) / (hi - lo), NaN -> 0"""
    a = x.numpy().astype(f32)
    with np.errstate(all="ignore"):
        lo, hi = a.min(1, keepdims=True), a.max(1, keepdims=True)          # numpy's min / max propagate NaN like amin / amax
        if fault == "batch_min":
            lo = np.full_like(lo, np.nanmin(a))
        v = (a - lo) / (hi - lo)
    v[np.isnan(v)] = 0.0
    return torch.from_numpy(v)


# ------------------------------------------------------------------ mdm_unit_rows
UNIT_DS = (1, 4, 255, 256, 257, 3072, 49152)
UNIT_RS = (1, 5)
UNIT_EPS = 1e-8
UNIT_FAULTS = ("no_last_element", "no_eps")


def unit_problem(R, D):
    """random rows; with R = 5: row 1 zero, row 2 all 1e-10 (||x|| < eps up to D = 3072, above it at 49 152), row 3 scaled by 1e3"""
    g = torch.Generator().manual_seed(R * 100000 + D)
    x = torch.randn(R, D, generator=g)
    if R >= 5:
        x[1] = 0.0
        x[2] = 1e-10
        x[3] *= 1e3
    return x


def emulate_unit_rows(x, eps, fault=None):
    a = x.numpy().astype(f32)
    R, D = a.shape
    trips = -(-D // 256)
    pad = np.zeros((R, trips * 256), f32)
    pad[:, :D] = a
    if fault == "no_last_element":
        pad[:, D - 1] = 0
    acc = np.zeros((R, 256), f32)
    for tr in range(trips):
        v = pad[:, tr * 256:(tr + 1) * 256]
        acc = fma32(v, v, acc)
    nrm = np.sqrt(block_sum32(acc))
    assert nrm.dtype == f32
    with np.errstate(all="ignore"):
        inv = f32(1.0) / (nrm if fault == "no_eps" else np.maximum(nrm, f32(eps)))
        return torch.from_numpy(a * inv[:, None])


# ------------------------------------------------------------------ mdm_col_argmax
ARGMAX_MS = (1, 2, 255, 256, 257, 1000)
ARGMAX_BS = (1, 3, 100)
ARGMAX_FAULTS = ("last_of_equals", "finite_start")
BIG_IDX = 0x7FFFFFFF


def argmax_problem(M, B):
    """S [M][B] random in (-1, 1) with planted columns (as far as M and B have room; the column -> what it holds in `plan`):
    equal maxima 2.0 at rows (m, m + 256) -- the same lane's serial loop --, (m, m + 1), (5, 700), (70, 200) -- two waves --, an
    all-equal column, an all-negative one, an all -inf one, one NaN, two NaNs around a larger number, all NaN"""
    g = torch.Generator().manual_seed(M * 1000 + B)
    S = torch.rand(M, B, generator=g) * 2 - 1
    cols = []

    def ties(a, b):
        def f(c):
            c[a] = c[b] = 2.0
        return f if b < M else None

    def one_nan(c):
        c[0] = 5.0
        c[M // 2] = NAN

    def two_nan(c):
        c[(M // 3 + 1) % M] = 9.0
        c[M - 1] = NAN
        c[M // 3] = NAN

    plans = [("tie_same_lane", ties(3, 259)), ("tie_neighbours", ties(max(0, M // 2 - 1), max(0, M // 2 - 1) + 1)), ("tie_5_700", ties(5, 700)),
             ("tie_two_waves", ties(70, 200)), ("all_equal", lambda c: c.fill_(0.25)), ("all_negative", lambda c: c.copy_(-c.abs() - 1)),
             ("all_neg_inf", lambda c: c.fill_(-INF)), ("one_nan", one_nan), ("two_nan", two_nan), ("all_nan", lambda c: c.fill_(NAN))]
    plans = [(n, f) for n, f in plans if f is not None]
    if B < len(plans):                                           # no room for all: the plans rotate with M
        k = (3 * ARGMAX_MS.index(M)) % len(plans)
        plans = plans[k:] + plans[:k]
    plan = {}
    for b, (name, f) in zip(range(B - 1, -1, -1), plans):          # from the last column down: column 0 stays random when B has room
        col = S[:, b].clone()
        f(col)
        S[:, b] = col
        plan[name] = b
    return S, plan


def emulate_col_argmax(S, fault=None):
    """torch.max(dim=0)'s rule restated in numpy: a NaN beats every number, the first row among equals"""
    a = S.numpy().astype(f32)
    M, B = a.shape
    val, idx = np.zeros(B, f32), np.zeros(B, np.int64)
    for b in range(B):
        c = a[:, b]
        nan = np.isnan(c)
        if nan.any():
            if fault == "finite_start":                         # v > best || v == best never holds for a NaN: it is skipped
                c = np.where(nan, -INF, c)
            else:
                rows = np.nonzero(nan)[0]
                i = rows[-1] if fault == "last_of_equals" else rows[0]
                val[b], idx[b] = c[i], i
                continue
        mx = c.max()
        if fault == "finite_start" and not mx >= f32(-3.0e38):
            val[b], idx[b] = f32(-3.0e38), BIG_IDX
            continue
        rows = np.nonzero(c == mx)[0]
        i = rows[-1] if fault == "last_of_equals" else rows[0]
        val[b], idx[b] = c[i], i
    return torch.from_numpy(val), torch.from_numpy(idx)


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_f32(a, b):
    """bit equality of two fp32 tensors"""
    a, b = a.detach().cpu().float().contiguous(), b.detach().cpu().float().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def call(name, *args):
    """one entry point through the C ABI on the current stream, then a device synchronise"""
    from mdm import _lib
    _lib.call(name, *args, _lib.stream())
    torch.cuda.synchronize()


def refused(name, *args):
    """the entry point returns non-zero from its host checks (nothing is launched) and says why"""
    from mdm import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*args, _lib.stream())
    return rc != 0 and len(lib.mdm_last_error()) > 0


class IntBuf:
    """int64 words `.t` [n] inside guard bands of a sentinel no kernel writes, as _bounds.Buf is for floats; the words start as `fill`"""
    PAT = 0x5A5A5A5A5A5A5A5A

    def __init__(self, n, device, fill=0x7A7A7A7A7A7A7A7A, guard=1024):
        self.n, self.g = n, guard
        self.raw = torch.full((n + 2 * guard,), self.PAT, dtype=torch.int64, device=device)
        self.t = self.raw[guard:guard + n]
        self.t.fill_(fill)

    def guards_intact(self):
        return bool((self.raw[:self.g] == self.PAT).all()) and bool((self.raw[self.g + self.n:] == self.PAT).all())

    def first_bad_guard(self):
        return ((self.raw != self.PAT).nonzero().flatten()[:4] - self.g).tolist()


# ------------------------------------------------------------------ what a row's outputs are held to (GPU rows and emulation alike)
def check_sqnorm(name, got, g):
    """-> err / bound; an all-zero-but-one row (bound 9 x small) is also held to exactly 9.0 by its caller"""
    from _bounds import sqnorm_ref
    ref, bound = sqnorm_ref(g)
    err = abs(float(got) - ref)
    assert np.isfinite(float(got)) and err <= bound, (name, float(got), ref, bound)
    return err / bound if bound else 0.0


def check_loss(name, r, T, word, flag, dpred):
    """-> err / bound of the loss word; dpred bit for bit"""
    from _bounds import dpred_want, loss_ref, loss_residual32
    N, C, H, W, Cp, dt, ws, ww = r
    r32 = loss_residual32(T["pred"], T["x_in"], T["s"], T["x0"], C)
    ref, bound = loss_ref(r32, T["w"])
    got = word * 2.0 ** -40
    assert flag == 0, (name, flag)
    assert abs(got - ref) <= bound, (name, got, ref, bound)
    want = dpred_want(r32, T["w"], Cp, LOSS_GSCALE, TD[dt])
    d = dpred.detach().cpu()
    ity = torch.int32 if dt == "f32" else torch.int16
    assert d.dtype == want.dtype and torch.equal(d.contiguous().view(ity), want.view(ity)), f"{name}: dpred differs from the fp32 expression"
    assert bool((d[..., C:].contiguous().view(ity) == 0).all()), f"{name}: pad channels of dpred are not +0"
    return abs(got - ref) / bound


def check_unit_rows(name, y, x, eps):
    from _bounds import check_bound, unit_rows_ref
    ref, bound = unit_rows_ref(x, eps)
    zero = (x == 0).all(1)
    yc = y.detach().cpu()
    assert bool((yc[zero].contiguous().view(torch.int32) == 0).all()), f"{name}: a zero row is not +0"
    if bool((~zero).any()):
        return check_bound(name, yc[~zero], ref[~zero], bound[~zero])[0]
    return 0.0


def check_normalize01(name, y, x):
    from _bounds import normalize01_want
    assert same_f32(y, normalize01_want(x)), f"{name}: differs from nan_to_num((x - amin) / (amax - amin), nan=0)"


def check_col_argmax(name, val, idx, S):
    from _bounds import col_argmax_want
    wv, wi = col_argmax_want(S)
    i = idx.detach().cpu()
    assert bool(((i >= 0) & (i < S.shape[0])).all()), f"{name}: an index outside [0, M): {i[(i < 0) | (i >= S.shape[0])][:4].tolist()}"
    assert torch.equal(i, wi), (name, "indices", i.tolist()[:8], wi.tolist()[:8])
    if val is not None:
        assert same_f32(val, wv), (name, "values", val.detach().cpu().tolist()[:8], wv.tolist()[:8])


def raises(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False
