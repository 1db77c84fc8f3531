"""The two kernels of csrc/inpaint.hip through the C ABI (include/mdm_inpaint.h).

mdm_inpaint_x0 bit for bit against numpy (tests/_inpaint_ref.x0_np: two fp32 operations and a select) on the 16-byte route
(H W = 16, 4 x 17) and the scalar one (H W = 15, or a pointer one float off a 16-byte boundary), for fp32 and bf16 predictions, with
and without a shift, with every combination of absent optional outputs, keep values from {0, 1, 0.5, -0, NaN}; its unprojected
outputs against mdm_sampler_x0 on the same inputs.  mdm_inpaint_start: x_start and unknown exact given the mu it wrote, every mu
inside the fp64-derived bound of tests/_inpaint_ref.mean_given_ref, two runs the same bits.  Every output is pre-filled with a
sentinel and compared whole, with guard bands on both sides; a refused call writes nothing.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _inpaint_ref as PR  # noqa: E402
from mdm import _lib  # noqa: E402

SENT, GUARD = -512.0, 8                          # (exact in bf16 too; 8 floats keep a 16-byte aligned view aligned)
KEEP_VALUES = np.array([0.0, 1.0, 0.5, -0.0, np.nan], dtype=np.float32)
GIVEN = np.array([False, True, True, False, True])


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


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


# ------------------------------------------------------------------------------------------ x0
SHAPES = [(3, 5), (4, 4), (4, 17)]               # H W = 15 (scalar route), 16 and 68 (16-byte route)


def _x0_case(N, C, H, W, keep_C, dtype, seed=0):
    g = np.random.default_rng(1000 * C + 10 * H * W + keep_C + seed)
    Cp = 8
    pred = torch.from_numpy((g.random((N, H, W, Cp)) * 2 - 1).astype(np.float32)).to(_lib.torch_dtype(dtype))
    x_in, s, known = ((g.random((N, C, H, W)) * 2 - 1).astype(np.float32) for _ in range(3))
    idx = g.integers(0, len(KEEP_VALUES), (N, keep_C, H, W))
    idx.reshape(-1)[:len(KEEP_VALUES)] = np.arange(len(KEEP_VALUES))          # every value is in every case
    keep = KEEP_VALUES[idx]
    assert np.array_equal(PR.given_np(keep, keep_C), GIVEN[idx])              # -0 is not given, NaN is given
    known.reshape(-1)[::7] = np.nan                                           # a given NaN passes through; a hidden one does not leak
    return Cp, pred, x_in, s, known, keep


def _run_x0(Cp, pred, x_in, s, known, keep, dtype, outs=(True, True), skew=None):
    """-> (pred_nchw, shifted0, x0_hat) as numpy or None where absent, after checking every guard band.  `skew`: per-operand
    element offsets (x_in, s, known, keep, pred_nchw, shifted0, x0_hat)."""
    N, C, H, W = x_in.shape
    numel = x_in.size
    sk = dict(zip(("x_in", "s", "known", "keep", "pred_nchw", "shifted0", "x0_hat"), skew or (0,) * 7))
    d_pred = pred.cuda().contiguous()
    ins = {k: _buf(v.size, skew=sk[k], data=v) for k, v in (("x_in", x_in), ("s", s), ("known", known), ("keep", keep)) if v is not None}
    res = {k: _buf(numel, skew=sk[k]) for k in ("pred_nchw", "shifted0", "x0_hat")}
    has = dict(pred_nchw=outs[0], shifted0=outs[1], x0_hat=True)
    _call("mdm_inpaint_x0", dtype=dtype, pred_nhwc=d_pred.data_ptr(), Cp=Cp, x_in=ins["x_in"][0].data_ptr(),
          s=ins["s"][0].data_ptr() if s is not None else None, known=ins["known"][0].data_ptr(), keep=ins["keep"][0].data_ptr(),
          keep_C=keep.shape[1], N=N, C=C, H=H, W=W, **{k: (res[k][0].data_ptr() if has[k] else None) for k in res})
    for k, (view, whole) in res.items():
        assert _guards(whole, numel, sk[k], written=has[k]), k
    for k, v in (("x_in", x_in), ("s", s), ("known", known), ("keep", keep)):                  # the inputs are read only
        if v is not None:
            assert _guards(ins[k][1], v.size, sk[k]) and _same(ins[k][0].cpu().numpy(), v.reshape(-1)), k
    assert torch.equal(d_pred.cpu(), pred)
    return tuple(res[k][0].cpu().numpy().reshape(N, C, H, W) if has[k] else None for k in res)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda v: f"HW{v[0] * v[1]}")
@pytest.mark.parametrize("C,keep_C", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
@pytest.mark.parametrize("shift", [True, False])
def test_x0(hw, C, keep_C, dtype, shift):
    N, (H, W) = 3, hw
    Cp, pred, x_in, s, known, keep = _x0_case(N, C, H, W, keep_C, dtype)
    if not shift:
        s = None
    want = PR.x0_np(pred.float().numpy(), x_in, s, known, keep)
    given = PR.given_np(keep, C)
    assert given.any() and not given.all() and _same(want[2][given], known[given])
    for outs in itertools.product((True, False), repeat=2):                   # every combination of absent optional outputs
        got = _run_x0(Cp, pred, x_in, s, known, keep, dtype, outs)
        for name, gv, wv in zip(("pred_nchw", "shifted0", "x0_hat"), got, want):
            assert gv is None or _same(gv, wv), (name, outs)
    # the unprojected outputs are what mdm_sampler_x0 writes from the same inputs
    d_pred, d_x, d_s = pred.cuda().contiguous(), dev(x_in), dev(s) if shift else None
    outs3 = [torch.full((x_in.size,), SENT, device="cuda") for _ in range(3)]
    _call("mdm_sampler_x0", dtype=dtype, pred_nhwc=d_pred.data_ptr(), Cp=Cp, x_in=d_x.data_ptr(), s=d_s.data_ptr() if shift else None,
          N=N, C=C, H=H, W=W, pred_nchw=outs3[0].data_ptr(), shifted0=outs3[1].data_ptr(), x0_hat=outs3[2].data_ptr())
    got = _run_x0(Cp, pred, x_in, s, known, keep, dtype)
    parent = [o.cpu().numpy().reshape(x_in.shape) for o in outs3]
    assert _same(got[0], parent[0]) and _same(got[1], parent[1])
    assert _same(got[2][~given], parent[2][~given]) and _same(got[2][given], known[given])


@pytest.mark.parametrize("which", range(7), ids=["x_in", "s", "known", "keep", "pred_nchw", "shifted0", "x0_hat"])
def test_x0_on_the_scalar_route_of_an_unaligned_pointer(which):
    """H W = 16 with one operand one float off a 16-byte boundary: the 16-byte route must not be taken"""
    N, C, H, W = 3, 3, 4, 4
    Cp, pred, x_in, s, known, keep = _x0_case(N, C, H, W, 1, _lib.F32, seed=which)
    want = PR.x0_np(pred.numpy(), x_in, s, known, keep)
    got = _run_x0(Cp, pred, x_in, s, known, keep, _lib.F32, skew=tuple(int(k == which) for k in range(7)))
    assert all(_same(gv, wv) for gv, wv in zip(got, want))


def test_x0_with_every_pointer_unaligned():
    N, C, H, W = 3, 3, 4, 17
    Cp, pred, x_in, s, known, keep = _x0_case(N, C, H, W, 3, _lib.BF16)
    want = PR.x0_np(pred.float().numpy(), x_in, s, known, keep)
    got = _run_x0(Cp, pred, x_in, s, known, keep, _lib.BF16, skew=(1,) * 7)
    assert all(_same(gv, wv) for gv, wv in zip(got, want))


# ------------------------------------------------------------------------------------------ start
def _start_case(N, C, HW, keep_C, seed):
    g = np.random.default_rng(seed)
    known = (g.random((N, C, HW)) * 2 - 1).astype(np.float32)
    keep = KEEP_VALUES[g.integers(0, len(KEEP_VALUES), (N, keep_C, HW))]
    keep[1] = 0.0                                                             # image 1: nothing given -> the fallback
    keep[2] = np.float32(1.0)                                                 # image 2: everything given
    if keep_C == C and C > 1:
        keep[3, 0] = -0.0                                                     # image 3: nothing of channel 0, all of channel 1
        keep[3, 1] = np.nan
    fallback = (g.random((N, C)) * 2 - 1).astype(np.float32)
    return known, keep, fallback


def _run_start(known, keep, fallback, per_channel, outs=(True, True, True), skew=0):
    N, C, HW = known.shape
    kn, kp, fb = _buf(known.size, skew=skew, data=known), _buf(keep.size, skew=skew, data=keep), dev(fallback)
    x, mu, unk = _buf(known.size, skew=skew), _buf(N * C), _buf(N, dtype=torch.int32)
    _call("mdm_inpaint_start", known=kn[0].data_ptr(), keep=kp[0].data_ptr(), keep_C=keep.shape[1], fallback=fb.data_ptr(),
          per_channel=per_channel, N=N, C=C, HW=HW, x_start=x[0].data_ptr() if outs[0] else None, mu=mu[0].data_ptr() if outs[1] else None,
          unknown=unk[0].data_ptr() if outs[2] else None)
    assert _guards(x[1], known.size, skew, outs[0]) and _guards(mu[1], N * C, 0, outs[1]) and _guards(unk[1], N, 0, outs[2])
    assert _guards(kn[1], known.size, skew) and _guards(kp[1], keep.size, skew)
    assert _same(kn[0].cpu().numpy(), known.reshape(-1)) and _same(kp[0].cpu().numpy(), keep.reshape(-1))
    return (x[0].cpu().numpy().reshape(N, C, HW) if outs[0] else None, mu[0].cpu().numpy().reshape(N, C) if outs[1] else None,
            unk[0].cpu().numpy() if outs[2] else None)


@pytest.mark.parametrize("HW", [15, 16, 1028])
@pytest.mark.parametrize("C,keep_C", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("per_channel", [0, 1])
def test_start(HW, C, keep_C, per_channel):
    N = 4
    known, keep, fallback = _start_case(N, C, HW, keep_C, seed=HW + 10 * C + keep_C)
    x, mu, unk = _run_start(known, keep, fallback, per_channel)
    assert np.array_equal(unk, PR.unknown_np(keep)) and unk[1] == HW and unk[2] == 0
    assert _same(x, PR.start_np(known, keep, mu))                             # exact given the mu the kernel wrote
    ref, bound, none = PR.mean_given_ref(known, keep, fallback, per_channel)
    assert none[1].all() and not none[2].any() and _same(mu[none], fallback[none])
    if keep_C == C and C > 1:
        assert bool(none[3, 0]) == bool(per_channel) and not none[3, 1]
    err = np.abs(mu.astype(np.float64) - ref)
    assert (err <= bound).all(), (err - bound).max()
    frac = float((err[~none] / bound[~none]).max())
    print(f"mdm_inpaint_start HW {HW} C {C} keep_C {keep_C} per_channel {per_channel}: largest |mu - fp64| / bound = {frac:.3f}")
    if not per_channel:
        assert (mu == mu[:, :1])[~none].all()                                 # one value per image, replicated to every channel
    assert _same(x[2], known[2]) and _same(x[1], np.broadcast_to(fallback[1][:, None], (C, HW)))
    # the same bits on every run, on both routes, and with any subset of the outputs
    x2, mu2, unk2 = _run_start(known, keep, fallback, per_channel)
    assert _same(x2, x) and _same(mu2, mu) and np.array_equal(unk2, unk)
    xs, mus, unks = _run_start(known, keep, fallback, per_channel, skew=1)      # the scalar route: another order, the same bound
    assert np.array_equal(unks, unk) and _same(xs, PR.start_np(known, keep, mus))
    assert (np.abs(mus.astype(np.float64) - ref) <= bound).all() and _same(mus[none], fallback[none])
    for outs in itertools.product((True, False), repeat=3):
        xo, muo, unko = _run_start(known, keep, fallback, per_channel, outs)
        assert (xo is None or _same(xo, x)) and (muo is None or _same(muo, mu)) and (unko is None or np.array_equal(unko, unk)), outs


# ------------------------------------------------------------------------------------------ refusals
def _refusal_rows():
    x0 = dict(dtype=0, pred_nhwc="in", Cp=8, x_in="in", s="in", known="in", keep="in", keep_C=3, N=2, C=3, H=4, W=4, pred_nchw="out",
              shifted0="out", x0_hat="out")
    start = dict(known="in", keep="in", keep_C=3, fallback="in", per_channel=0, N=2, C=3, HW=16, x_start="out", mu="out", unknown="out")
    return [("mdm_inpaint_x0", x0, [dict(pred_nhwc=None), dict(x_in=None), dict(known=None), dict(keep=None), dict(x0_hat=None),
                                    dict(keep_C=2), dict(keep_C=0), dict(C=9, keep_C=9, Cp=16), dict(N=0), dict(N=-1), dict(C=0),
                                    dict(H=0), dict(W=-3), dict(dtype=2), dict(dtype=-1), dict(Cp=2)]),
            ("mdm_inpaint_start", start, [dict(known=None), dict(keep=None), dict(fallback=None), dict(keep_C=2), dict(keep_C=0),
                                          dict(C=9, keep_C=9), dict(N=0), dict(N=-2), dict(C=0), dict(HW=0), dict(HW=-16)])]


@pytest.mark.parametrize("name,ok,rows", _refusal_rows(), ids=[r[0] for r in _refusal_rows()])
def test_refusals_write_nothing(name, ok, rows):
    """every pointer is a real buffer, far larger than any row's extents ask for"""
    lib = _lib.load()
    assert list(ok) + ["stream"] == _lib.INPAINT_PARAMS[name]
    for change in rows:
        bufs = {"in": torch.zeros(4096, device="cuda"), "out": _buf(4096)[1]}
        args = [bufs[v].data_ptr() if isinstance(v, str) else v for v in dict(ok, **change).values()]
        rc = getattr(lib, name)(*args, _lib.stream())
        text = lib.mdm_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and text.startswith(name[4:] + ":"), (change, rc, text)
        assert bool((bufs["out"] == SENT).all()) and not bufs["in"].any(), change


def test_a_start_without_outputs_launches_nothing():
    P = torch.zeros(64, device="cuda").data_ptr()
    assert _lib.load().mdm_inpaint_start(P, P, 1, P, 0, 2, 3, 4, None, None, None, _lib.stream()) == 0
    torch.cuda.synchronize()
