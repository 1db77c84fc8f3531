"""The three kernels of csrc/restore.hip through the C ABI (include/mdm_restore.h).

mdm_restore_x0 bit for bit against numpy (tests/_restore_ref.x0_np: the group sum in the header's stated order, one division, two
fp32 operations) and every element inside the fp64-derived bound of tests/_restore_ref.project_ref, on the 16-byte route and the
scalar one (H W or W no multiple of 4 -- 2 x 6 has H W = 12 but rows 24 bytes apart --, or a pointer one float off a 16-byte
boundary), for fp32 and bf16 predictions, with and without a shift, with every combination of absent optional outputs; its
unprojected outputs against mdm_sampler_x0 on the same inputs; one case beyond one pass of the grid cap, twice.
mdm_restore_measure the same way; mdm_restore_start: `expand` exact given y, every mu inside the bound of mu_ref, two runs and
both alignments the same bits.  Every output is pre-filled with a sentinel and compared whole, with guard bands on both sides; a
refused call writes nothing.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _restore_ref as RR  # noqa: E402
from mdm import _lib  # noqa: E402

SENT, GUARD = -512.0, 8                          # (exact in bf16 too; 8 floats keep a 16-byte aligned view aligned)
# (k, H, W): k = 1 scalar (15) and 16-byte (16, 68); k = 2 scalar (W = 6: H W % 4 == 0 but rows unaligned) and 16-byte; k = 4 one
# group per plane, several, a row of five; k = 8 one group per plane and several (lane pairs)
SHAPES = [(1, 3, 5), (1, 4, 4), (1, 4, 17), (2, 2, 6), (2, 4, 4), (2, 6, 8), (4, 4, 4), (4, 8, 12), (4, 4, 20), (8, 8, 8), (8, 16, 24)]
CASES = [(k, H, W, C, gray) for k, H, W in SHAPES for C in (1, 3) for gray in (0, 1) if k * k * (C if gray else 1) > 1]
IDS = [f"k{k}-{H}x{W}-C{C}-gray{g}" for k, H, W, C, g in CASES]


def _buf(numel, dtype=torch.float32, skew=0, data=None):
    """(view of `numel` elements, the whole buffer): GUARD + skew sentinels in front of the view and GUARD behind it; the view holds
    sentinels too, or `data`.  skew = 1 puts the view one element off a 16-byte boundary."""
    whole = torch.full((GUARD + skew + numel + GUARD,), SENT, device="cuda", dtype=dtype)
    view = whole[GUARD + skew:GUARD + skew + numel]
    if data is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))
        assert (view.data_ptr() % 16 == 0) == (skew == 0)
    return view, whole


def _guards(whole, numel, skew=0, written=True):
    """the bands on both sides hold the sentinel -- and so does the view of an output that was not to be written"""
    h = whole.float().cpu().numpy()
    lo = GUARD + skew
    return (h[:lo] == SENT).all() and (h[lo + numel:] == SENT).all() and (written or (h == SENT).all())


def _call(name, **kw):
    _lib.call(name, stream=_lib.stream(), **kw)
    torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """bit for bit, a NaN matching any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _yshape(N, C, H, W, k, gray):
    return (N, 1 if gray else C, H // k, W // k)


# ------------------------------------------------------------------------------------------ x0
def _x0_case(N, C, H, W, k, gray, dtype, seed=0):
    g = np.random.default_rng(100000 * k + 1000 * C + 10 * H * W + gray + seed)
    Cp = 8
    pred = torch.from_numpy((g.random((N, H, W, Cp)) * 2 - 1).astype(np.float32)).to(_lib.torch_dtype(dtype))
    x_in, s = ((g.random((N, C, H, W)) * 2 - 1).astype(np.float32) for _ in range(2))
    y = (g.random(_yshape(N, C, H, W, k, gray)) * 2 - 1).astype(np.float32)
    return Cp, pred, x_in, s, y


OPERANDS = ("x_in", "s", "y", "pred_nchw", "shifted0", "x0_hat")


def _run_x0(Cp, pred, x_in, s, y, k, gray, dtype, outs=(True, True), skew=None):
    """-> (pred_nchw, shifted0, x0_hat) as numpy or None where absent, after checking every guard band.  `skew`: per-operand element
    offsets in the order of OPERANDS."""
    N, C, H, W = x_in.shape
    numel = x_in.size
    sk = dict(zip(OPERANDS, skew or (0,) * 6))
    d_pred = pred.cuda().contiguous()
    ins = {n: _buf(v.size, skew=sk[n], data=v) for n, v in (("x_in", x_in), ("s", s), ("y", y)) if v is not None}
    res = {n: _buf(numel, skew=sk[n]) for n in ("pred_nchw", "shifted0", "x0_hat")}
    has = dict(pred_nchw=outs[0], shifted0=outs[1], x0_hat=True)
    _call("mdm_restore_x0", dtype=dtype, pred_nhwc=d_pred.data_ptr(), Cp=Cp, x_in=ins["x_in"][0].data_ptr(),
          s=ins["s"][0].data_ptr() if s is not None else None, y=ins["y"][0].data_ptr(), k=k, gray=gray, N=N, C=C, H=H, W=W,
          **{n: (res[n][0].data_ptr() if has[n] else None) for n in res})
    for n, (view, whole) in res.items():
        assert _guards(whole, numel, sk[n], written=has[n]), n
    for n, v in (("x_in", x_in), ("s", s), ("y", y)):                          # the inputs are read only
        if v is not None:
            assert _guards(ins[n][1], v.size, sk[n]) and _same(ins[n][0].cpu().numpy(), v.reshape(-1)), n
    assert torch.equal(d_pred.cpu(), pred)
    return tuple(res[n][0].cpu().numpy().reshape(N, C, H, W) if has[n] else None for n in res)


@pytest.mark.parametrize("k,H,W,C,gray", CASES, ids=IDS)
def test_x0(k, H, W, C, gray):
    N = 3
    worst = 0.0
    for dtype, shift in itertools.product((_lib.F32, _lib.BF16), (True, False)):
        Cp, pred, x_in, s, y = _x0_case(N, C, H, W, k, gray, dtype)
        if not shift:
            s = None
        want = RR.x0_np(pred.float().numpy(), x_in, s, y, k, gray)
        for outs in itertools.product((True, False), repeat=2):                # every combination of absent optional outputs
            got = _run_x0(Cp, pred, x_in, s, y, k, gray, dtype, outs)
            for name, gv, wv in zip(("pred_nchw", "shifted0", "x0_hat"), got, want):
                assert gv is None or _same(gv, wv), (name, outs, dtype, shift)
        # the unprojected outputs are what mdm_sampler_x0 writes from the same inputs, and the projection starts from its x0_hat
        d_pred, d_x, d_s = pred.cuda().contiguous(), torch.from_numpy(x_in).cuda(), torch.from_numpy(s).cuda() if shift else None
        outs3 = [torch.full((x_in.size,), SENT, device="cuda") for _ in range(3)]
        _call("mdm_sampler_x0", dtype=dtype, pred_nhwc=d_pred.data_ptr(), Cp=Cp, x_in=d_x.data_ptr(), s=d_s.data_ptr() if shift else None,
              N=N, C=C, H=H, W=W, pred_nchw=outs3[0].data_ptr(), shifted0=outs3[1].data_ptr(), x0_hat=outs3[2].data_ptr())
        parent = [o.cpu().numpy().reshape(x_in.shape) for o in outs3]
        got = _run_x0(Cp, pred, x_in, s, y, k, gray, dtype)
        assert _same(got[0], parent[0]) and _same(got[1], parent[1])
        assert _same(got[2], RR.project_np(parent[2], y, k, gray)) and not _same(got[2], parent[2])
        ref, bound = RR.project_ref(parent[2], y, k, gray)
        err = np.abs(got[2].astype(np.float64) - ref)
        assert (err <= bound).all(), float((err - bound).max())
        worst = max(worst, float((err / bound).max()))
    print(f"mdm_restore_x0 k {k} {H} x {W} C {C} gray {gray}: largest |x0_hat - fp64| / bound = {worst:.3f}")


# one 16-byte-route case per k; (operand, ...) one float off alignment in turn, then all of them
SKEW_CASES = [(1, 4, 4, 3, 1), (2, 6, 8, 3, 0), (4, 8, 12, 3, 1), (8, 16, 24, 3, 0), (8, 16, 24, 3, 1)]


@pytest.mark.parametrize("k,H,W,C,gray", SKEW_CASES, ids=[f"k{c[0]}-gray{c[4]}" for c in SKEW_CASES])
def test_x0_bits_do_not_depend_on_pointer_alignment(k, H, W, C, gray):
    """the scalar route forms every sum in the order of the 16-byte route: the header's promise"""
    N = 3
    Cp, pred, x_in, s, y = _x0_case(N, C, H, W, k, gray, _lib.BF16, seed=5)
    want = RR.x0_np(pred.float().numpy(), x_in, s, y, k, gray)
    base = _run_x0(Cp, pred, x_in, s, y, k, gray, _lib.BF16)
    assert all(_same(gv, wv) for gv, wv in zip(base, want))
    for which in list(range(6)) + [None]:
        skew = (1,) * 6 if which is None else tuple(int(j == which) for j in range(6))
        got = _run_x0(Cp, pred, x_in, s, y, k, gray, _lib.BF16, skew=skew)
        assert all(_same(gv, bv) for gv, bv in zip(got, base)), which


@pytest.mark.parametrize("k,H,W", [(1, 4, 4), (2, 6, 8), (8, 16, 24)], ids=["k1", "k2", "k8"])
@pytest.mark.parametrize("C", [5, 8])
def test_x0_gray_over_more_channels_than_a_lane_of_the_16_byte_route_holds(k, H, W, C):
    """gray with C > 4 takes the scalar route whatever the alignment: the same statement, groups of up to 512 elements"""
    N = 2
    Cp, pred, x_in, s, y = _x0_case(N, C, H, W, k, 1, _lib.BF16, seed=3)
    want = RR.x0_np(pred.float().numpy(), x_in, s, y, k, 1)
    got = _run_x0(Cp, pred, x_in, s, y, k, 1, _lib.BF16)
    assert all(_same(gv, wv) for gv, wv in zip(got, want))
    ref, bound = RR.project_ref(RR.parent_np(pred.float().numpy(), x_in, s)[2], y, k, 1)
    assert (np.abs(got[2].astype(np.float64) - ref) <= bound).all()
    assert _same(_run_measure(x_in, k, 1), RR.measure_np(x_in, k, 1))          # (the 16-byte measure kernel holds nothing: any C)


def test_x0_beyond_one_pass_of_the_grid_cap():
    """2048 workgroups of 256 lanes take 524288 items of four columns by two rows in one pass; [11, 3, 384, 384] at k = 2 has 608256"""
    N, C, H, W, k, gray = 11, 3, 384, 384, 2, 0
    assert N * C * (H // k) * (W // 4) > 2048 * 256
    g = np.random.default_rng(77)
    pred = torch.from_numpy((g.random((N, H, W, 8), dtype=np.float32) * 2 - 1)).to(torch.bfloat16)
    x_in, s = (g.random((N, C, H, W), dtype=np.float32) * 2 - 1 for _ in range(2))
    y = g.random(_yshape(N, C, H, W, k, gray), dtype=np.float32) * 2 - 1
    want = RR.x0_np(pred.float().numpy(), x_in, s, y, k, gray)
    d_pred, d_x, d_s, d_y = pred.cuda(), torch.from_numpy(x_in).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    runs = []
    for _ in range(2):
        outs = [torch.full((x_in.size + 2 * GUARD,), SENT, device="cuda") for _ in range(3)]
        views = [o[GUARD:-GUARD] for o in outs]
        _call("mdm_restore_x0", dtype=_lib.BF16, pred_nhwc=d_pred.data_ptr(), Cp=8, x_in=d_x.data_ptr(), s=d_s.data_ptr(), y=d_y.data_ptr(),
              k=k, gray=gray, N=N, C=C, H=H, W=W, pred_nchw=views[0].data_ptr(), shifted0=views[1].data_ptr(), x0_hat=views[2].data_ptr())
        assert all(bool((o[:GUARD] == SENT).all()) and bool((o[-GUARD:] == SENT).all()) for o in outs)
        runs.append([v.cpu().numpy().reshape(x_in.shape) for v in views])
    for gv, wv, again in zip(runs[0], want, runs[1]):
        assert np.array_equal(_bits(gv), _bits(wv)) and np.array_equal(_bits(gv), _bits(again))


@pytest.mark.parametrize("skew", [0, 1], ids=["16-byte", "scalar"])
@pytest.mark.parametrize("k,gray", [(1, 1), (2, 0), (4, 1), (8, 0), (8, 1)])
def test_a_nan_reaches_its_own_group_and_nothing_else(k, gray, skew):
    N, C, H, W = 3, 3, 16, 24
    Cp, pred, x_in, s, y = _x0_case(N, C, H, W, k, gray, _lib.F32, seed=9)
    x_in[1, 2, 9, 13] = np.nan                                                 # in x: group (1, gray ? 0 : 2, 9 / k, 13 / k)
    y[2, 0, 0, (W // k) - 1] = np.nan                                          # in y: group (2, 0, 0, last)
    got = _run_x0(Cp, pred, x_in, s, y, k, gray, _lib.F32, skew=(skew,) * 6)
    want = np.zeros((N, C, H, W), bool)
    by, bx = 9 // k * k, 13 // k * k
    want[1, slice(None) if gray else 2, by:by + k, bx:bx + k] = True
    want[2, slice(None) if gray else 0, 0:k, W - k:] = True
    assert np.array_equal(np.isnan(got[2]), want) and _same(got[2], RR.x0_np(pred.numpy(), x_in, s, y, k, gray)[2])
    assert int(np.isnan(got[0]).sum()) == 0 and int(np.isnan(got[1]).sum()) == 1


# ------------------------------------------------------------------------------------------ measure
def _run_measure(x, k, gray, skew=0):
    N, C, H, W = x.shape
    ys = _yshape(N, C, H, W, k, gray)
    xb, yb = _buf(x.size, skew=skew, data=x), _buf(int(np.prod(ys)), skew=skew)
    _call("mdm_restore_measure", x=xb[0].data_ptr(), k=k, gray=gray, N=N, C=C, H=H, W=W, y=yb[0].data_ptr())
    assert _guards(yb[1], int(np.prod(ys)), skew) and _guards(xb[1], x.size, skew) and _same(xb[0].cpu().numpy(), x.reshape(-1))
    return yb[0].cpu().numpy().reshape(ys)


@pytest.mark.parametrize("k,H,W,C,gray", CASES, ids=IDS)
def test_measure(k, H, W, C, gray):
    N = 3
    g = np.random.default_rng(7 + 100 * k + H * W + 10 * C + gray)
    x = (g.random((N, C, H, W)) * 2 - 1).astype(np.float32)
    got = _run_measure(x, k, gray)
    assert _same(got, RR.measure_np(x, k, gray))
    ref, bound = RR.mean_ref(x, k, gray)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err - bound).max())
    print(f"mdm_restore_measure k {k} {H} x {W} C {C} gray {gray}: largest |y - fp64| / bound = {float((err / bound).max()):.3f}")
    assert _same(_run_measure(x, k, gray), got) and _same(_run_measure(x, k, gray, skew=1), got)
    x[0, 0, 0, 0] = np.nan                                                     # a NaN reaches its group's mean only
    nan = np.isnan(_run_measure(x, k, gray))
    assert nan[0, 0, 0, 0] and int(nan.sum()) == 1


# ------------------------------------------------------------------------------------------ start
def _run_start(y, k, gray, per_channel, C, outs=(True, True), skew=0):
    N, _, Hk, Wk = y.shape
    H, W = Hk * k, Wk * k
    yb, mu, ex = _buf(y.size, skew=skew, data=y), _buf(N * C), _buf(N * C * H * W, skew=skew)
    _call("mdm_restore_start", y=yb[0].data_ptr(), k=k, gray=gray, per_channel=per_channel, N=N, C=C, H=H, W=W,
          mu=mu[0].data_ptr() if outs[0] else None, expand=ex[0].data_ptr() if outs[1] else None)
    assert _guards(mu[1], N * C, 0, outs[0]) and _guards(ex[1], N * C * H * W, skew, outs[1])
    assert _guards(yb[1], y.size, skew) and _same(yb[0].cpu().numpy(), y.reshape(-1))
    return (mu[0].cpu().numpy().reshape(N, C) if outs[0] else None, ex[0].cpu().numpy().reshape(N, C, H, W) if outs[1] else None)


@pytest.mark.parametrize("k,H,W,C,gray", CASES + [(2, 64, 72, 3, 0), (1, 40, 40, 3, 1)], ids=IDS + ["k2-64x72-C3-gray0", "k1-40x40-C3-gray1"])
def test_start(k, H, W, C, gray):
    """(the two larger shapes give a thread of the mean several elements and every wave a share)"""
    N = 3
    g = np.random.default_rng(3 + 100 * k + H * W + 10 * C + gray)
    y = (g.random(_yshape(N, C, H, W, k, gray)) * 2 - 1).astype(np.float32)
    for per_channel in (0, 1):
        mu, ex = _run_start(y, k, gray, per_channel, C)
        assert _same(ex, RR.expand_np(y, k, gray, C))                          # exact given y
        ref, bound = RR.mu_ref(y, C, gray, per_channel)
        err = np.abs(mu.astype(np.float64) - ref)
        assert (err <= bound).all(), float((err - bound).max())
        if gray or not per_channel:
            assert (mu == mu[:, :1]).all()                                     # one value per image, repeated for every channel
        elif C > 1:
            assert not (mu == mu[:, :1]).all()
        for outs in itertools.product((True, False), repeat=2):                # ... and with both absent nothing is launched
            for skew in (0, 1):
                mo, eo = _run_start(y, k, gray, per_channel, C, outs, skew)
                assert (mo is None or _same(mo, mu)) and (eo is None or _same(eo, ex)), (outs, skew)
    y[0, 0, 0, 0] = np.nan
    mu, ex = _run_start(y, k, gray, 1, C)
    assert np.array_equal(np.isnan(ex), np.isnan(RR.expand_np(y, k, gray, C)))
    assert np.isnan(mu[0, 0]) and not np.isnan(mu[1:]).any() and (gray or C == 1 or not np.isnan(mu[0, 1:]).any())


def test_the_expansion_of_a_measurement_has_that_measurement():
    """measure(expand(y)) = y to the bound of the mean (every element of a group is y[g], the exact mean is y[g])"""
    g = np.random.default_rng(12)
    for k, gray in ((2, 0), (4, 1), (1, 1), (8, 0)):
        y = (g.random(_yshape(3, 3, 16, 24, k, gray)) * 2 - 1).astype(np.float32)
        ex = _run_start(y, k, gray, 0, 3, outs=(False, True))[1]
        back = _run_measure(ex, k, gray)
        assert (np.abs(back.astype(np.float64) - y) <= RR.mean_ref(ex, k, gray)[1]).all()


# ------------------------------------------------------------------------------------------ refusals
def _refusal_rows():
    x0 = dict(dtype=0, pred_nhwc="in", Cp=8, x_in="in", s="in", y="in", k=2, gray=0, N=2, C=3, H=4, W=4, pred_nchw="out",
              shifted0="out", x0_hat="out")
    measure = dict(x="in", k=2, gray=0, N=2, C=3, H=4, W=4, y="out")
    start = dict(y="in", k=2, gray=0, per_channel=0, N=2, C=3, H=4, W=4, mu="out", expand="out")
    groups = [dict(k=0), dict(k=3), dict(k=16), dict(k=-2), dict(k=4, H=6), dict(k=4, W=6), dict(k=8), dict(gray=2), dict(gray=-1),
              dict(k=1), dict(k=1, gray=1, C=1), dict(C=9), dict(N=0), dict(N=-1), dict(C=0), dict(H=0), dict(W=-4)]
    return [("mdm_restore_x0", x0, [dict(pred_nhwc=None), dict(x_in=None), dict(y=None), dict(x0_hat=None), dict(dtype=2),
                                    dict(dtype=-1), dict(Cp=2), dict(C=9, Cp=16)] + groups),
            ("mdm_restore_measure", measure, [dict(x=None), dict(y=None)] + groups),
            ("mdm_restore_start", start, [dict(y=None)] + groups)]


@pytest.mark.parametrize("name,ok,rows", _refusal_rows(), ids=[r[0] for r in _refusal_rows()])
def test_refusals_write_nothing(name, ok, rows):
    """every pointer is a real buffer, far larger than any row's extents ask for"""
    lib = _lib.load()
    assert list(ok) + ["stream"] == _lib.RESTORE_PARAMS[name]
    for change in rows:
        bufs = {"in": torch.zeros(4096, device="cuda"), "out": _buf(4096)[1]}
        args = [bufs[v].data_ptr() if isinstance(v, str) else v for v in dict(ok, **change).values()]
        rc = getattr(lib, name)(*args, _lib.stream())
        text = lib.mdm_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and text.startswith(name[4:] + ":"), (change, rc, text)
        assert bool((bufs["out"] == SENT).all()) and not bufs["in"].any(), change
    args = [bufs[v].data_ptr() if isinstance(v, str) else v for v in ok.values()]      # the row the changes start from is accepted
    assert getattr(lib, name)(*args, _lib.stream()) == 0
    torch.cuda.synchronize()


def test_a_start_without_outputs_launches_nothing():
    P = torch.zeros(64, device="cuda").data_ptr()
    assert _lib.load().mdm_restore_start(P, 2, 0, 0, 2, 3, 4, 4, None, None, _lib.stream()) == 0
    torch.cuda.synchronize()
