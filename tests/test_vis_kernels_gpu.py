"""mdm_vis_range and mdm_vis_grid (csrc/vis.hip) through the C ABI against tests/_vis_ref.py: torch's amin / amax / min / max, upstream's
two normalisations, torchvision's grid geometry and save_image's quantisation, all on the CPU.  fp32 results bit for bit (a NaN by its
position: the payload is free), uint8 byte for byte.

Every operand sits inside guard bands (`_bounds.Buf`; `ByteBuf` below for the uint8 grid), destinations start as the NaN pattern or a
byte sentinel, the gaps between strided images hold NaN (a read of one would poison the result), inputs must come back bit for bit
and a second launch must repeat the first.  The scratch words of a global range must be zero again after every launch."""
import pytest
import torch

import _store_rows as SR
import _vis_ref as VR
from _bounds import Buf
from _store_rows import call, refused, same_f32

pytestmark = pytest.mark.gpu
F32 = torch.float32
MODES = (None, "image", "global")          # mode 0, 1, 2


def _dev():
    return torch.device("cuda:0")


class ByteBuf:
    """uint8 `.t` [n] of a sentinel inside guard bands of another byte no kernel writes; `off`: misalign the data by that many bytes"""
    GUARD, FILL = 0xA5, 0x5C

    def __init__(self, n, device, off=0, guard=65536):
        self.n, self.g = n, guard + off
        self.raw = torch.full((n + 2 * guard + off,), self.GUARD, dtype=torch.uint8, device=device)
        self.t = self.raw[self.g:self.g + n]
        self.t.fill_(self.FILL)

    def guards_intact(self):
        return bool((self.raw[:self.g] == self.GUARD).all()) and bool((self.raw[self.g + self.n:] == self.GUARD).all())

    def first_bad_guard(self):
        return ((self.raw.cpu() != self.GUARD).nonzero().flatten()[:4] - self.g).tolist()


def _intact(bufs, inputs=()):
    for b in bufs:
        if b is not None:
            assert b.guards_intact(), b.first_bad_guard()
    for b, want in inputs:
        assert torch.equal(b.t.cpu().view(torch.int32), want.contiguous().view(torch.int32)), "an input was modified"


def _strided(x, extra, device):
    """x [K, E] -> (Buf [K, E + extra] whose gaps are NaN, what it must still hold afterwards)"""
    K, E = x.shape
    host = torch.full((K, E + extra), VR.NAN)
    host[:, :E] = x
    return Buf((K, E + extra), F32, device, host), host


# ------------------------------------------------------------------ mdm_vis_range
def _range(x, extra, glob):
    """-> lohi of two launches on fresh buffers (everything checked in between)"""
    K, E = x.shape
    outs = []
    sb = Buf((4,), F32, _dev(), torch.zeros(4))
    for _ in range(2):
        xb, host = _strided(x, extra, _dev())
        lb = Buf((1 if glob else K, 2), F32, _dev())
        call("mdm_vis_range", xb.t.data_ptr(), E + extra, K, E, glob, lb.t.data_ptr(), sb.t.data_ptr() if glob else None)
        _intact((xb, lb, sb), [(xb, host)])
        assert not bool(sb.t.view(torch.int32).any()), f"the scratch words are not zero after the launch: {sb.t.view(torch.int32).tolist()}"
        outs.append(lb.t.cpu())
    assert VR.same_grid(outs[1], outs[0]), "a second launch differs"
    return outs[0]


@pytest.mark.parametrize("K", VR.RANGE_KS)
@pytest.mark.parametrize("E", VR.RANGE_ES)
def test_range_is_torchs(E, K):
    """per image and over the batch, contiguous and img_stride = E + 7, every image kind: plain, the extremum in the last element, all
    negative, constant, one +inf, one NaN (both words NaN) -- and for the batch range also without the NaN image"""
    nk = len(SR.NORM_KINDS)
    for extra in VR.RANGE_STRIDE_EXTRA:
        for seed in (range(nk) if K == 1 else (0, 3)):
            x = VR.image_kinds(K, E, seed)
            for glob in (0, 1):
                got, want = _range(x, extra, glob), VR.range_ref(x, not glob)
                assert VR.same_grid(got, want), (E, K, extra, seed, glob, got.tolist(), want.tolist())
                for k in range(K if not glob else 0):
                    if SR.NORM_KINDS[(k + seed) % nk] == "nan":
                        assert bool(torch.isnan(got[k]).all()), "a NaN pixel must make both words NaN"
        x = VR.image_kinds(K, E, 1, VR.FINITE_KINDS)
        got, want = _range(x, extra, 1), VR.range_ref(x, False)
        assert same_f32(got, want), (E, K, extra, got.tolist(), want.tolist())


PART = 16384                               # RANGE_PART_ELEMS of csrc/vis.hip: what one workgroup of a global range takes of an image at least


@pytest.mark.parametrize("K,E", [(3, 2 * PART + 5), (1, 1024 * PART + 9), (1030, 3), (2000, 4099)])
def test_range_over_the_batch_in_parts(K, E):
    """the shapes at which a global range takes another path: an image in several parts (the last one short), more parts than the
    1024 workgroups allow, more images than workgroups, both; the extremes sit in the last element of the last image and in the first
    of the first, then a NaN in the last element"""
    g = torch.Generator().manual_seed(K + E)
    x = torch.randn(K, E, generator=g)
    x[0, 0], x[-1, -1] = -77.0, 88.0
    assert same_f32(_range(x, 0, 1), torch.tensor([[-77.0, 88.0]]))
    if K * E < 1 << 20:
        assert same_f32(_range(x, 5, 1), torch.tensor([[-77.0, 88.0]]))
        assert same_f32(_range(x, 0, 0), VR.range_ref(x, True))
    x[-1, -1] = VR.NAN
    assert bool(torch.isnan(_range(x, 0, 1)).all())


# ------------------------------------------------------------------ mdm_vis_grid
def _grid(xb, stride, shape, lohi, mode, nrow, padding, pad_value, outs, x_off=0, f_off=0, u_off=0):
    """one launch into fresh destinations -> (f32 grid | None, u8 grid | None) on the host; `outs`: 'f32' | 'u8' | 'both'"""
    K, C, H, W = shape
    Cg, Hg, Wg = VR.grid_shape_ref(K, C, H, W, nrow, padding)
    n = Cg * Hg * Wg
    fb = Buf((n + f_off,), F32, _dev()) if outs != "u8" else None
    ub = ByteBuf(n, _dev(), off=u_off) if outs != "f32" else None
    lb = Buf(tuple(lohi.shape), F32, _dev(), lohi) if lohi is not None else None
    call("mdm_vis_grid", xb.t.data_ptr() + 4 * x_off, stride, K, C, H, W, lb.t.data_ptr() if lb else None, mode, nrow, padding, pad_value,
         fb.t.data_ptr() + 4 * f_off if fb else None, ub.t.data_ptr() if ub else None)
    _intact((xb, fb, ub, lb), [(lb, lohi)] if lb else [])
    if fb is not None and f_off:
        assert bool((fb.t[:f_off].view(torch.int32) == fb.pat).all()), "written in front of a misaligned grid_f32"
    return (fb.t[f_off:].cpu().view(Cg, Hg, Wg) if fb else None), (ub.t.cpu().view(Hg, Wg, Cg) if ub else None)


def _check_grid(x, xb, host, stride, nrow, padding, pad_value, norm, forms=("both", "f32", "u8"), **off):
    """x [K, C, H, W] on the host (what the kernel reads from `xb`), normalisation `norm`: every output form against the reference,
    `lohi` taken from torch; the input comes back bit for bit"""
    mode = MODES.index(norm)
    lohi = VR.range_ref(x.flatten(1), mode == 1) if mode else None
    want_f, want_u = VR.grid_ref(x, nrow, norm, padding, pad_value)
    first = None
    for form in forms + forms[:1]:
        f, u = _grid(xb, stride, tuple(x.shape), lohi, mode, nrow, padding, pad_value, form, **off)
        assert torch.equal(xb.t.cpu().view(torch.int32), host.view(torch.int32)), "the input was modified"
        if f is not None:
            assert VR.same_grid(f, want_f), (norm, form, "f32", int((f.view(torch.int32) != want_f.view(torch.int32)).sum()))
        if u is not None:
            assert torch.equal(u, want_u), (norm, form, "u8", (u != want_u).nonzero()[:4].tolist())
        if first is None:
            first = (f, u)
    assert VR.same_grid(f, first[0]) and torch.equal(u, first[1]), "a second launch differs"
    return want_f


@pytest.mark.parametrize("row", VR.GRID_ROWS, ids=VR.grid_row_id)
def test_grid_is_make_grid_of_the_normalised_batch(row):
    """geometry x normalisation x output form; images of every kind (a NaN image: all 0 in mode 1, everything NaN in mode 2; a constant
    image: 0 in mode 1) and, so that mode 2 is compared on numbers, once more without the +inf and NaN kinds"""
    (C, H, W), (K, nrow), padding, pad_value = row
    seed = VR.GRID_ROWS.index(row)
    for kinds in (None, VR.FINITE_KINDS):
        x = VR.image_kinds(K, C * H * W, seed, kinds)
        xb, host = _strided(x, 0, _dev())
        for norm in MODES:
            want = _check_grid(x.view(K, C, H, W), xb, host, C * H * W, nrow, padding, pad_value, norm)
            if kinds is not None and norm == "global" and float(x.min()) != float(x.max()):
                assert not bool(torch.isnan(want).any())


def test_grid_reads_a_time_major_history_in_place():
    """[T+1, N, C, H, W] with T+1 = 4, N = 3: the frames of sample n are N C H W apart and start at hist[0, n]; no copy"""
    T1, N, C, H, W = 4, 3, 3, 16, 16
    hist = torch.randn(T1, N, C, H, W, generator=torch.Generator().manual_seed(11)) * 1.5
    hb = Buf((T1 * N, C * H * W), F32, _dev(), hist.view(T1 * N, -1))
    for n in range(N):
        for norm in MODES:
            _check_grid(hist[:, n].contiguous(), hb, hist.view(T1 * N, -1), N * C * H * W, 2, 2, 0.0, norm, forms=("both",), x_off=n * C * H * W)


@pytest.mark.parametrize("x_off,f_off,u_off", [(1, 0, 0), (0, 1, 1), (3, 2, 3), (2, 3, 2)])
def test_grid_at_any_alignment(x_off, f_off, u_off):
    """pointers that rule out the 16-byte loads, the 16-byte stores and the 4-byte stores; img_stride = E + 7 with NaN in the gaps"""
    K, C, H, W = 5, 3, 16, 16
    E = C * H * W
    x = VR.image_kinds(K, E, 2, VR.FINITE_KINDS)
    host = torch.full((K * (E + 7) + x_off,), VR.NAN)
    host[x_off:].view(K, E + 7)[:, :E] = x
    xb = Buf(tuple(host.shape), F32, _dev(), host)
    for norm in MODES:
        _check_grid(x.view(K, C, H, W), xb, host, E + 7, 3, 2, 0.5, norm, x_off=x_off, f_off=f_off, u_off=u_off)


def test_mode_1_is_normalize01_then_mode_0():
    """the per-image mode with the range kernel's own lohi is bit for bit mdm_normalize01 followed by the grid without normalisation --
    its constant and NaN-pixel images included"""
    K, C, H, W, nrow = 7, 3, 16, 16, 3
    E = C * H * W
    x = VR.image_kinds(K, E, 0)
    xb, host = _strided(x, 0, _dev())
    lb, yb = Buf((K, 2), F32, _dev()), Buf((K, E), F32, _dev())
    call("mdm_vis_range", xb.t.data_ptr(), E, K, E, 0, lb.t.data_ptr(), None)
    call("mdm_normalize01", xb.t.data_ptr(), yb.t.data_ptr(), K, E)
    _intact((xb, lb, yb), [(xb, host)])
    a = _grid(xb, E, (K, C, H, W), lb.t.cpu(), 1, nrow, 2, 0.0, "both")
    b = _grid(yb, E, (K, C, H, W), None, 0, nrow, 2, 0.0, "both")
    assert same_f32(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not bool(torch.isnan(a[0]).any())
    assert VR.same_grid(a[0], VR.grid_ref(x.view(K, C, H, W), nrow, "image")[0])


def test_quantisation_at_every_rounding_edge():
    """mode 0 on the fp32 neighbours (-2 .. +2 ulp) of every (k + 0.5) / 255, values below 0 and above 1, the infinities and NaN (-> 0):
    one image [1, 1, n], so the grid is the image three times"""
    v = VR.quant_edges()
    n = v.numel()
    xb, host = _strided(v[None], 0, _dev())
    f, u = _grid(xb, n, (1, 1, 1, n), None, 0, 8, 2, 0.0, "both")
    want = VR.to_u8_ref(v[None, None, :].expand(3, 1, n))
    assert torch.equal(u, want), (u != want).nonzero()[:6].tolist()
    assert VR.same_grid(f, v[None, None, :].expand(3, 1, n))
    fin = ~torch.isnan(v)
    assert torch.equal(u[0, :, 1][fin], v[fin].mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)) and int(u[0, :, 0][~fin].max()) == 0


def test_refusals_write_nothing():
    K, C, H, W = 4, 3, 8, 8
    E = C * H * W
    x = torch.ones(K, E)
    xb, lb = Buf((K, E), F32, _dev(), x), Buf((K, 2), F32, _dev(), torch.zeros(K, 2))
    fb, ub, sb = Buf((3 * 22 * 22,), F32, _dev()), ByteBuf(3 * 22 * 22, _dev()), Buf((4,), F32, _dev(), torch.zeros(4))
    X, L, F, U, S = (b.t.data_ptr() for b in (xb, lb, fb, ub, sb))
    ok = (X, E, K, C, H, W, L, 1, 2, 2, 0.0, F, U)
    for i, v in ((0, None), (1, E - 1), (2, 0), (3, 0), (4, 0), (5, -2), (7, 3), (7, -1), (8, 0), (9, -1), (6, None)):
        bad = list(ok)
        bad[i] = v
        assert refused("mdm_vis_grid", *bad), (i, v)
    assert refused("mdm_vis_grid", X, E, K, C, H, W, L, 1, 2, 2, 0.0, None, None)
    for bad in ((None, E, K, E, 0, F, None), (X, E, K, E, 0, None, None), (X, E, 0, E, 0, F, None), (X, E, K, 0, 0, F, None),
                (X, E - 1, K, E, 0, F, None), (X, E, K, E, 1, F, None), (X, E, K, E, 1, F, S + 4)):
        assert refused("mdm_vis_range", *bad), bad
    torch.cuda.synchronize()
    _intact((xb, lb, fb, ub, sb), [(xb, x), (lb, torch.zeros(K, 2)), (sb, torch.zeros(4))])
    assert bool((fb.t.view(torch.int32) == fb.pat).all()) and bool((ub.t == ByteBuf.FILL).all()), "a refused call wrote"
