"""The two kernels of csrc/metric.hip through the C ABI (include/mdm_metric.h): mdm_metric_image against the fp64 statement of
tests/_metric_ref.py, every one of the eight slots of every row inside the derived bound of tests/_metric_bounds.py, the two counts
exact.  The shapes come from mdm_metric_plan (one window, one past it, each tile edge - 1, exactly and + 1, one-row and one-column
maps, W a multiple of 4 and not, C 1 and 3, N 1 and 5, R = 3 N) and every shape runs with every pointer 16-byte aligned and with every
pointer one float off.  Every operand lies inside guard bands of a NaN pattern (`_bounds.Buf`, the float sibling of
tests/_guard_bufs.py): a write past an end shows in the bands, a read past an end that reaches a result turns it into NaN.  A NaN
planted in one row gives the header's NaN slots in the rows that read it and leaves the others bit for bit; two launches give the same
bits; a refused call names its argument and writes nothing.  The workspace size is mdm_metric_ws_bytes'.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _metric_bounds as MB  # noqa: E402
import _metric_ref as MR  # noqa: E402
from _bounds import Buf  # noqa: E402
from mdm import _lib  # noqa: E402


def _plan(R, C, H, W):
    import mdm
    return mdm.metrics.plan(R, C, H, W)


TH, TW = _plan(1, 1, 11, 11).tile_h, _plan(1, 1, 11, 11).tile_w
# (R, N, C, H, W)
SHAPES = [(3, 1, 1, 11, 11), (15, 5, 3, 11, 12), (3, 1, 3, 12, 11), (15, 5, 1, 12, 12),
          (3, 1, 1, TH + 9, TW + 9), (3, 1, 3, TH + 10, TW + 10), (3, 1, 1, TH + 11, TW + 11), (15, 5, 3, TH + 10, TW + 11),
          (3, 1, 3, 11, 40), (15, 5, 1, 40, 11), (6, 2, 3, 2 * TH + 5, TW + 20), (3, 1, 1, 96, 96)]
CLASSES = [(img, kp) for img in MR.IMAGE_KINDS for kp in ("none", "box")] + [("smooth", kp) for kp in MR.KEEP_KINDS] + \
          [("two_level", "random_c"), ("noise", "nan")]
BIG_CLASSES = [("noise", "random"), ("smooth", "box"), ("two_level", "none"), ("equal", "random_c"), ("near", "nan"), ("outside", "zeros")]


class FBuf:
    """fp32 `.t` [n] holding `values` (or the NaN pattern) inside `_bounds.Buf` guard bands; `shift` = 1 puts it one float off a
    16-byte boundary."""

    def __init__(self, n, values=None, shift=0):
        self.buf = Buf((n + shift,), torch.float32, "cuda", row=1)
        self.t = self.buf.t[shift:]
        self.shift = shift
        assert (self.t.data_ptr() % 16 == 0) == (shift == 0)
        self.want = None
        if values is not None:
            self.want = values.reshape(-1).clone()
            self.t.copy_(self.want)

    def ptr(self):
        return self.t.data_ptr()

    def _pattern(self, t):
        return bool((t.view(torch.int32) == self.buf.pat).all())

    def guards_intact(self):
        return self.buf.guards_intact() and self._pattern(self.buf.t[:self.shift])

    def intact(self):
        return self.guards_intact() and np.array_equal(self.t.cpu().numpy().view(np.uint32), self.want.numpy().view(np.uint32))

    def untouched(self):
        return self.guards_intact() and self._pattern(self.t)


def run(pred, truth, keep, shift=0, clamp=(-1.0, 1.0), L=2.0):
    """mdm_metric_image -> out [R, 8] on the host, after checking every guard band and that the inputs came back bit for bit"""
    lib = _lib.load()
    R, C, H, W = pred.shape
    N = truth.shape[0]
    need = lib.mdm_metric_ws_bytes(R, C, H, W)
    assert need == _plan(R, C, H, W).ws_bytes and need > 0 and need % 8 == 0
    ins = {k: FBuf(v.numel(), v, shift) for k, v in (("pred", pred), ("truth", truth), ("keep", keep)) if v is not None}
    ws, out = FBuf(need // 4 + 2 * shift, shift=shift), FBuf(R * 8, shift=shift)     # (the workspace holds doubles: 8-byte aligned)
    ws_ptr = ws.ptr() + 4 * shift
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    _lib.call("mdm_metric_image", pred=ins["pred"].ptr(), truth=ins["truth"].ptr(), keep=ins["keep"].ptr() if keep is not None else None,
              Ck=keep.shape[1] if keep is not None else 0, R=R, N=N, C=C, H=H, W=W, clamp_lo=lo, clamp_hi=hi, data_range=L, ws=ws_ptr,
              ws_bytes=need, out=out.ptr(), stream=_lib.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in ins.values()), "an input was written"
    assert ws.guards_intact() and out.guards_intact(), "a write past the workspace or the output"
    return out.t.cpu().reshape(R, 8)


def _bits(t):
    return t.numpy().view(np.uint32)


_REFS = {}


def _case(shape, img, kp):
    key = (shape, img, kp)
    if key not in _REFS:
        R, N, C, H, W = shape
        pred, truth = MR.draw_images(img, R, N, C, H, W)
        keep = MR.draw_keep(kp, N, C, H, W)
        ref = MR.reference(pred, truth, keep)
        _REFS[key] = (pred, truth, keep, ref["out"], MB.out_bound(ref, TH, TW))
    return _REFS[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_slot_inside_the_bound(shape):
    worst = 0.0
    for img, kp in (BIG_CLASSES if shape[3] * shape[4] > 4000 else CLASSES):
        pred, truth, keep, ref_out, bound = _case(shape, img, kp)
        assert bool(torch.isfinite(bound).all())
        outs = []
        for shift in (0, 1):
            got = run(pred, truth, keep, shift)
            worst = max(worst, MB.check(f"{shape} {img}/{kp} shift {shift}", got, ref_out, bound))
            outs.append(got)
        again = run(pred, truth, keep, 0)
        assert np.array_equal(_bits(again), _bits(outs[0])), "two launches differ"
        if img == "equal":
            assert bool((outs[0][:, 0] == 0).all()) and bool(torch.isinf(outs[0][:, 1]).all())
    print(f"mdm_metric_image {shape}: largest error / bound = {worst:.3f}")
    assert worst <= 1


def test_clamp_off_and_another_data_range():
    shape = (6, 2, 3, TH + 3, TW + 13)
    R, N, C, H, W = shape
    pred, truth = MR.draw_images("outside", R, N, C, H, W)
    keep = MR.draw_keep("random", N, C, H, W)
    for clamp, L in ((None, 2.0), ((-0.5, 0.25), 2.0), ((-1.0, 1.0), 1.0), ((1.0, -1.0), 255.0)):
        ref = MR.reference(pred, truth, keep, L, clamp)
        ratio = MB.check(f"clamp {clamp} L {L}", run(pred, truth, keep, 0, clamp, L), ref["out"], MB.out_bound(ref, TH, TW))
        print(f"clamp {clamp} L {L}: largest error / bound = {ratio:.3f}")
    a, b = MR.reference(pred, truth, keep, 2.0, None)["out"], MR.reference(pred, truth, keep, 2.0, (-1.0, 1.0))["out"]
    assert float((a[:, 0] - b[:, 0]).abs().min()) > 0.1                      # the clamp is not a no-op on this class


@pytest.mark.parametrize("where", ["pred", "truth"])
@pytest.mark.parametrize("in_hole", [True, False])
def test_a_nan_reaches_the_stated_slots_of_the_rows_that_read_it(where, in_hole):
    shape = (6, 2, 3, TH + 11, TW + 11)
    R, N, C, H, W = shape
    pred, truth = MR.draw_images("smooth", R, N, C, H, W)
    keep = torch.ones(N, 1, H, W)
    keep[:, :, 6:12, 6:12] = 0                                               # the hole: rows and columns 6 .. 11
    clean = run(pred, truth, keep)
    y, x = (8, 9) if in_hole else (H - 1, W - 1)                             # the far corner: no hole-centred window reaches it
    pred, truth = pred.clone(), truth.clone()
    if where == "pred":
        pred[3, 1, y, x] = math.nan
        rows = [3]
    else:
        truth[1, 2, y, x] = math.nan
        rows = [1, 3, 5]                                                      # r % N == 1
    got = run(pred, truth, keep)
    ref = MR.reference(pred, truth, keep)
    MB.check(f"NaN in {where}", got, ref["out"], MB.out_bound(ref, TH, TW))
    nan = torch.zeros(R, 8, dtype=torch.bool)
    for r in rows:
        nan[r, :3] = True
        nan[r, 3:6] = in_hole                                                 # the element is hole / a window centred in the hole holds it
    assert torch.equal(torch.isnan(got), nan)
    others = [r for r in range(R) if r not in rows]
    assert np.array_equal(_bits(got[others]), _bits(clean[others])) and np.array_equal(_bits(got[:, 6:]), _bits(clean[:, 6:]))
    assert bool((got[:, 6] == 3 * 36).all()) and bool((got[:, 7] == 3 * 36).all())


def test_a_nan_beside_the_hole_reaches_ssim_hole_only():
    """not a hole element, but inside the window of a hole-centred position: mse_hole and psnr_hole stay, ssim_hole goes"""
    R, N, C, H, W = 2, 2, 1, 20, 20
    pred, truth = MR.draw_images("noise", R, N, C, H, W)
    keep = torch.ones(N, 1, H, W)
    keep[:, :, 6:9, 6:9] = 0
    pred[1, 0, 12, 12] = math.nan
    got = run(pred, truth, keep)
    assert torch.isnan(got[1]).tolist() == [True, True, True, False, False, True, False, False] and not bool(torch.isnan(got[0]).any())
    ref = MR.reference(pred, truth, keep)
    MB.check("NaN beside the hole", got, ref["out"], MB.out_bound(ref, TH, TW))


# ------------------------------------------------------------------------------------------ refusals
OK = dict(pred="in", truth="in", keep="in", Ck=3, R=4, N=2, C=3, H=16, W=16, clamp_lo=-1.0, clamp_hi=1.0, data_range=2.0, ws="ws",
          ws_bytes=1 << 20, out="out")
REFUSALS = [(dict(pred=None), "pred"), (dict(truth=None), "truth"), (dict(out=None), "out"), (dict(ws=None), "ws"), (dict(R=0), "R"),
            (dict(R=-4), "R"), (dict(N=0), "N"), (dict(C=0, Ck=1), "C"), (dict(H=0), "H"), (dict(W=-16), "W"), (dict(R=5), "R"),
            (dict(H=10), "H"), (dict(W=10), "W"), (dict(Ck=2), "Ck"), (dict(Ck=0), "Ck"), (dict(data_range=0.0), "data_range"),
            (dict(data_range=-2.0), "data_range"), (dict(data_range=math.inf), "data_range"), (dict(data_range=math.nan), "data_range"),
            (dict(C=4, Ck=4, H=32768, W=32768), "C H W"), (dict(ws_bytes=4 * 3 * 48 - 1), "ws_bytes")]


def test_refusals_name_the_argument_and_write_nothing():
    lib = _lib.load()
    assert list(OK) + ["stream"] == _lib.METRIC_PARAMS["mdm_metric_image"]
    assert lib.mdm_metric_ws_bytes(4, 3, 16, 16) == 4 * 3 * 48                # one tile per channel: the last row asks for one byte less
    for change, word in REFUSALS:
        bufs = {"in": FBuf(8192, torch.zeros(8192)), "ws": FBuf(1 << 18), "out": FBuf(4096)}
        args = [bufs[v].ptr() if isinstance(v, str) else v for v in dict(OK, **change).values()]
        rc = lib.mdm_metric_image(*args, _lib.stream())
        text = lib.mdm_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and text.startswith("metric_image:") and word in text, (change, rc, text)
        assert bufs["out"].untouched() and bufs["ws"].untouched() and bufs["in"].intact(), change
    bufs = {"in": FBuf(8192, torch.zeros(8192)), "ws": FBuf(1 << 18), "out": FBuf(4096)}
    args = [bufs[v].ptr() if isinstance(v, str) else v for v in dict(OK, keep=None, Ck=7).values()]      # Ck is not read without keep
    assert lib.mdm_metric_image(*args, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert not bufs["out"].untouched() and bufs["out"].guards_intact()


def test_the_plan_is_the_launch():
    """mdm_metric_plan: the tiles cover the map, the grid is one workgroup per tile at these sizes and one per row"""
    for R, N, C, H, W in SHAPES:
        p = _plan(R, C, H, W)
        assert (p.tile_h, p.tile_w) == (TH, TW) and (p.tiles_y - 1) * TH < H - 10 <= p.tiles_y * TH and (p.tiles_x - 1) * TW < W - 10 <= p.tiles_x * TW
        assert p.grid == (R * C * p.tiles_y * p.tiles_x, R) and p.ws_bytes == p.grid[0] * 48
