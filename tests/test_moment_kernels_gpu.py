"""mdm_moment_accumulate through the C ABI on the GPU (include/mdm_moment.h), at the smallest shapes where tiling, K stepping, split
edges and masks can go wrong -- d at both edges of an MFMA tile and of a workgroup tile and over three tile rows, R around the edges
of a K step and of a split, taken from mdm_moment_plan / mdm_moment_ws_bytes.  Every operand lies between NaN guard bands that are
checked after the call; the padding columns d .. row_ld and the rows past R hold NaN.  Exact-grid rows must come out BIT-EQUAL to the
int64 statement on every route, in one call and as three carried chunks; normal and uniform rows inside the header's bound against
math.fsum; `outer` bit-symmetric; two launches bit-identical; a NaN and an inf exactly where they belong; a refused call writes
nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _moment_ref as MM  # noqa: E402

GUARD = 64
DS = [1, 15, 16, 17, 63, 64, 65, 129]
R_KEYS = ["1", "3", "4", "5", "rps-1", "rps", "rps+1", "2rps+2"]
# a subset of the product: every d and every R at least once, the widest d with the longest R, one column with a split edge
SHAPES = [(1, "1"), (1, "2rps+2"), (15, "3"), (16, "4"), (17, "5"), (63, "rps-1"), (64, "rps"), (65, "rps+1"), (129, "2rps+2"), (129, "5"),
          (17, "2rps+2"), (65, "3")]
assert {d for d, _ in SHAPES} == set(DS) and {k for _, k in SHAPES} == set(R_KEYS)
# float rows 16-byte aligned with row_ld the next multiple of 4 (the 16-byte route), the same one float off, row_ld == d, row_ld == d + 3;
# uint8 the same three pitches (by 4 bytes where the pitch allows, else by 1)
ROUTES = ["f32_vec", "f32_off", "f32_ld0", "f32_ld3", "u8_vec", "u8_ld0", "u8_ld3"]


def _plan(R, d):
    import mdm
    return mdm.moment_plan(R, d)                                               # mdm_moment_plan and mdm_moment_ws_bytes


def _rows_of(key, d):
    rps = _plan(64, d).rows_per_split
    R = {"1": 1, "3": 3, "4": 4, "5": 5, "rps-1": rps - 1, "rps": rps, "rps+1": rps + 1, "2rps+2": 2 * rps + 2}[key]
    p = _plan(R, d)
    assert p.rows_per_split == rps and p.splits == -(-R // rps), "the plan of these small shapes splits at rows_per_split"
    return R, p


class Banded:
    """a device buffer of `n` elements between two guard bands of NaN (float types) or 0xA5 (bytes), `offset` elements off the
    allocation's alignment"""

    def __init__(self, n, dtype, offset=0):
        self.fill = float("nan") if dtype.is_floating_point else 0xA5
        self.buf = torch.full((2 * GUARD + n + offset,), self.fill, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD + offset:GUARD + offset + n]
        self.n, self.offset = n, offset

    def bands_intact(self):
        lo, hi = self.buf[:GUARD + self.offset], self.buf[GUARD + self.offset + self.n:]
        if self.buf.dtype.is_floating_point:
            return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


def _lut():
    """an exact table: byte b -> (b - 128) 2^-7, the grid of the exact tests"""
    return ((torch.arange(256, dtype=torch.float32) - 128) / 128).cuda()


def _place_rows(route, x, ints):
    """the rows on the device for a route -> (Banded, kind, lut, row_ld); x float32 [R][d] (ints: its grid integers, for uint8)"""
    R, d = x.shape
    if route.startswith("u8"):
        ld = d + 3 if route == "u8_ld3" else d if route == "u8_ld0" else (d + 3) // 4 * 4
        b = Banded(R * ld, torch.uint8)
        m = torch.full((R, ld), 0xA5, dtype=torch.uint8)
        m[:, :d] = torch.from_numpy((ints + 128).astype(np.uint8))
        b.view.copy_(m.reshape(-1).cuda())
        return b, 1, _lut(), ld
    ld = d + 3 if route == "f32_ld3" else d if route == "f32_ld0" else (d + 3) // 4 * 4
    b = Banded(R * ld, torch.float32, offset=1 if route == "f32_off" else 0)
    assert (b.view.data_ptr() % 16 == 0) == (route != "f32_off")
    m = torch.full((R, ld), float("nan"))
    m[:, :d] = torch.from_numpy(x)
    b.view.copy_(m.reshape(-1).cuda())
    return b, 0, None, ld


class Outputs:
    def __init__(self, d, R):
        """for calls of R rows and of the chunks of `_cuts(R)`: fewer rows may plan more splits and a larger workspace"""
        cuts = _cuts(R)
        self.d, self.ld = d, d + 3
        self.sum, self.outer = Banded(d, torch.float64), Banded(d * self.ld, torch.float64)
        self.ws_bytes = max(_plan(n, d).ws_bytes for n in [R] + [hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])])
        self.ws = Banded(self.ws_bytes // 8, torch.float64)

    def call(self, src, src_kind, src_lut, src_ld, n_rows, carry, first_row=0, **change):
        """mdm_moment_accumulate on the rows [first_row, first_row + n_rows) of `src`; `change` replaces parameters by the header's names"""
        from mdm import _lib
        elem = 1 if src_kind == 1 else 4
        kw = dict(rows=src.view.data_ptr() + first_row * src_ld * elem, kind=src_kind, lut=None if src_lut is None else src_lut.data_ptr(),
                  row_ld=src_ld, R=n_rows, d=self.d, carry=carry, sum=self.sum.view.data_ptr(), outer=self.outer.view.data_ptr(),
                  outer_ld=self.ld, ws=self.ws.view.data_ptr(), ws_bytes=self.ws_bytes, stream=_lib.stream())
        _lib.call("mdm_moment_accumulate", **dict(kw, **change))

    def read(self):
        """(sum [d], outer [d][d]) on the host after checking that the padding of outer and every guard band still hold NaN"""
        torch.cuda.synchronize()
        o = self.outer.view.view(self.d, self.ld).cpu().numpy()
        assert np.isnan(o[:, self.d:]).all(), "elements d .. outer_ld of a row were written"
        assert self.sum.bands_intact() and self.outer.bands_intact() and self.ws.bands_intact()
        return self.sum.view.cpu().numpy().copy(), o[:, :self.d].copy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _cuts(R):
    """three chunks of unequal length (fewer where R has fewer rows)"""
    return sorted({0, R // 3, R // 3 + 1 + R // 4, R}) if R >= 3 else [0, R]


def _check_exact(R, d, route):
    g = np.random.default_rng(100 * d + R)
    ints = MM.grid_ints(g, R + 2, d)                                            # two more rows: what lies past R must not count
    x = MM.grid_rows(ints)
    rows, kind, lut, ld = _place_rows(route, x, ints)
    if kind == 0:                                                               # the rows past R hold NaN (uint8 has none: 0xA5 bytes)
        rows.view.view(R + 2, ld)[R:] = float("nan")
    else:
        rows.view.view(R + 2, ld)[R:] = 0xA5
    want_s, want_o = MM.grid_moments(ints[:R])
    out = Outputs(d, R)
    out.call(rows, kind, lut, ld, R, carry=0)
    s1, o1 = out.read()
    assert _same_bits(s1, want_s) and _same_bits(o1, want_o), "one call"
    assert _same_bits(o1, o1.T)
    out.call(rows, kind, lut, ld, R, carry=0)                                   # two launches, the same bits (over the old values: carry 0 overwrites)
    s2, o2 = out.read()
    assert _same_bits(s1, s2) and _same_bits(o1, o2)
    cuts = _cuts(R)
    for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):                     # carried chunks of unequal length
        out.call(rows, kind, lut, ld, hi - lo, carry=int(k > 0), first_row=lo)
    s3, o3 = out.read()
    assert _same_bits(s3, want_s) and _same_bits(o3, want_o), f"chunks {cuts}"
    assert rows.bands_intact()


def _check_bound(R, d, dist, routes):
    """one call: s the plan's splits, no carried call; chunks: s the largest split count of the calls, c the calls after the first"""
    g = np.random.default_rng(7 * d + R)
    x = (g.normal(size=(R, d)) if dist == "normal" else g.uniform(-1, 1, size=(R, d))).astype(np.float32)
    ref_s, ref_o, mag_s, mag_o = MM.fsum_moments(x)
    cuts = _cuts(R)
    s_one = _plan(R, d).splits
    s_chunks = max(_plan(hi - lo, d).splits for lo, hi in zip(cuts[:-1], cuts[1:]))
    for route in routes:
        rows, kind, lut, ld = _place_rows(route, x, None)
        out = Outputs(d, R)
        out.call(rows, kind, lut, ld, R, carry=0)
        s, o = out.read()
        assert MM.inside(s, ref_s, MM.bound(R, s_one, 0, mag_s, ref_s)), route
        assert MM.inside(o, ref_o, MM.bound(R, s_one, 0, mag_o, ref_o)) and _same_bits(o, o.T), route
        for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            out.call(rows, kind, lut, ld, hi - lo, carry=int(k > 0), first_row=lo)
        s, o = out.read()
        assert MM.inside(s, ref_s, MM.bound(R, s_chunks, len(cuts) - 2, mag_s, ref_s)), route
        assert MM.inside(o, ref_o, MM.bound(R, s_chunks, len(cuts) - 2, mag_o, ref_o)) and _same_bits(o, o.T), route


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("d,rkey", SHAPES, ids=[f"d{d}-R{k}" for d, k in SHAPES])
def test_exact_grid_rows_are_bit_equal_to_the_int64_statement(d, rkey, route):
    _check_exact(_rows_of(rkey, d)[0], d, route)


# Splits of SEVERAL 16-row blocks with a ragged last one: the row-block loop past its first pass, the look-ahead loads and the
# re-staging behind the second barrier -- the loop every workload shape lives in.  d = 129 (6 tiles, 86 workgroups wanted each) with
# R = 2757 plans splits of 48 rows, 3 blocks, and a last split of 21; d = 2049 has 561 tiles and one split of 2, 3 and 4 blocks.
LONG = [(2757, 129), (17, 2049), (33, 2049), (50, 2049)]


def test_the_long_shapes_run_several_blocks_per_split():
    for R, d in LONG:
        p = _plan(R, d)
        last = R - (p.splits - 1) * p.rows_per_split
        assert min(p.rows_per_split, R) > 16 and last % 16 != 0, (R, d, p)      # more than one block, the last one ragged
    assert _plan(2757, 129).splits > 1 and _plan(50, 2049).splits == 1


@pytest.mark.parametrize("route", ["f32_vec", "f32_off", "f32_ld3", "u8_vec", "u8_ld3"])
@pytest.mark.parametrize("R,d", LONG, ids=[f"d{d}-R{R}" for R, d in LONG])
def test_exact_grid_rows_over_several_blocks_per_split(R, d, route):
    _check_exact(R, d, route)


@pytest.mark.parametrize("dist", ["normal", "uniform"])
@pytest.mark.parametrize("d,rkey", SHAPES, ids=[f"d{d}-R{k}" for d, k in SHAPES])
def test_float_rows_are_inside_the_bound(d, rkey, dist):
    _check_bound(_rows_of(rkey, d)[0], d, dist, ("f32_vec", "f32_off", "f32_ld0", "f32_ld3"))


@pytest.mark.parametrize("dist", ["normal", "uniform"])
def test_float_rows_over_several_blocks_per_split_are_inside_the_bound(dist):
    _check_bound(2757, 129, dist, ("f32_vec", "f32_off"))


def test_the_tile_map_covers_the_triangle_once():
    """mdm_moment_tile_of is the map both launches use (one function, compiled for host and device)"""
    import mdm
    for d in (1, 64, 65, 129, 700):
        p = _plan(4, d)
        T = -(-d // p.tile)
        pairs = [mdm.moment_tile_of(d, t) for t in range(p.tiles)]
        assert sorted(pairs) == [(i, j) for i in range(T) for j in range(i, T)] and pairs == sorted(pairs)


def test_uint8_rows_through_the_default_table_are_inside_the_bound():
    from mdm.data import normalize_lut
    d = 65
    R, p = _rows_of("2rps+2", d)
    g = np.random.default_rng(5)
    b = g.integers(0, 256, size=(R, d)).astype(np.uint8)
    lut = normalize_lut()
    x = lut.numpy()[b]
    ref_s, ref_o, mag_s, mag_o = MM.fsum_moments(x)
    rows = Banded(R * d, torch.uint8, offset=1)                                 # row_ld == d, odd: the byte route
    rows.view.copy_(torch.from_numpy(b).reshape(-1).cuda())
    out = Outputs(d, R)
    out.call(rows, 1, lut.cuda(), d, R, carry=0)
    s, o = out.read()
    assert MM.inside(s, ref_s, MM.bound(R, p.splits, 0, mag_s, ref_s)) and MM.inside(o, ref_o, MM.bound(R, p.splits, 0, mag_o, ref_o))
    assert _same_bits(o, o.T)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("route", ["f32_vec", "f32_ld3"])
def test_a_non_finite_value_reaches_its_column_sum_and_its_row_and_column_of_outer(bad, route):
    d = 129
    R, p = _rows_of("2rps+2", d)
    g = np.random.default_rng(9)
    x = g.uniform(0.25, 1.0, size=(R, d)).astype(np.float32)                    # positive: inf times it is inf, never inf - inf
    for r, c in ((R - 1, 70), (0, 0), (17, 128)):
        y = x.copy()
        y[r, c] = bad
        rows, kind, lut, ld = _place_rows(route, y, None)
        out = Outputs(d, R)
        out.call(rows, kind, lut, ld, R, carry=0)
        s, o = out.read()
        want_s = np.zeros(d, bool)
        want_s[c] = True
        want_o = np.zeros((d, d), bool)
        want_o[c, :] = want_o[:, c] = True
        assert np.array_equal(~np.isfinite(s), want_s) and np.array_equal(~np.isfinite(o), want_o), (r, c)
        x64 = x.astype(np.float64)
        x64[:, c] = 0
        ref_s, ref_o, mag_s, mag_o = MM.fsum_moments(x64)                       # and everything else is as if column c were not there
        keep = ~want_o
        assert MM.inside(o[keep], ref_o[keep], MM.bound(R, p.splits, 0, mag_o, ref_o)[keep])
        assert MM.inside(s[~want_s], ref_s[~want_s], MM.bound(R, p.splits, 0, mag_s, ref_s)[~want_s])


def test_every_refusal_names_its_argument_and_writes_nothing():
    from mdm import _lib
    lib = _lib.load()
    d, R = 17, 5
    x = np.ones((R, d), np.float32)
    rows, kind, lut, ld = _place_rows("f32_vec", x, None)
    out = Outputs(d, R)
    need = lib.mdm_moment_ws_bytes(R, d)
    assert need == out.ws_bytes == _plan(R, d).ws_bytes and lib.mdm_moment_ws_bytes(R, 8193) == -1
    assert lib.mdm_moment_plan(R, 0, None, None, None, None, None, None) == -1 and "d" in lib.mdm_last_error().decode()
    bad = [(dict(rows=None), "rows"), (dict(sum=None), "sum"), (dict(outer=None), "outer"), (dict(ws=None), "ws"), (dict(kind=2), "kind"),
           (dict(rows=rows.view.data_ptr() + 2), "4-byte"), (dict(kind=1), "lut"), (dict(R=0), "R"), (dict(d=0), "d"), (dict(d=8193), "d = 8193"), (dict(row_ld=d - 1), "row_ld"),
           (dict(outer_ld=d - 1), "outer_ld"), (dict(sum=out.sum.view.data_ptr() + 4), "sum"),
           (dict(outer=out.outer.view.data_ptr() + 4), "outer"), (dict(ws=out.ws.view.data_ptr() + 4), "ws"), (dict(ws_bytes=need - 8), "ws_bytes")]
    for change, word in bad:
        with pytest.raises(RuntimeError, match=word):
            out.call(rows, kind, lut, ld, R, carry=0, **change)
    torch.cuda.synchronize()
    for b in (out.sum, out.outer, out.ws):                                      # nothing was launched: every output still holds its NaN fill
        assert bool(torch.isnan(b.buf).all())
    out.call(rows, kind, lut, ld, R, carry=0)                                   # and the same operands, unchanged, are accepted
    s, o = out.read()
    assert _same_bits(s, np.full(d, float(R))) and _same_bits(o, np.full((d, d), float(R)))
