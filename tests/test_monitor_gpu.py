"""Device-side training monitors: mdm_loss_fwd_bwd_mon / mdm_monitor_commit through the C ABI, then the step, the trainers and the
deferred-loss epoch on top of them (reference trainer_masked_mean_shift.py:61-64, 175-179, 249-250, 321-334).

THE SUMMATION BOUND used throughout (`_sum_bound`).  A monitor is mean(x) = sum(x) / numel, summed in fp32 as
    thread: k terms added serially            (k = C channels x the pixels one thread loops over)
    wave:   6 shuffle levels over 64 lanes
    block:  2 levels over the 4 waves         -> 8 levels above the thread
and each of the G workgroups rounds (its partial / numel) to Q23.40 once, half an ulp = 2^-41, before integer adds that are exact.
First-order error analysis of a summation tree (Higham, Accuracy and Stability, 4.2): every term passes through at most
k + 8 additions, each with relative error <= 2^-24, so |error of sum| <= (k + 8) 2^-24 sum|x|, i.e. for the mean
    |error| <= (k + 8) * 2^-24 * mean|x|  +  G * 2^-41.
(The multiplication by 1/numel is one more rounding of the same size class; it is inside the slack of counting k additions
for k terms.)  Nothing here is tuned to what the kernel returns.
"""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden.make_golden import TINY, base_args, seed_all  # noqa: E402

Q40 = 2.0 ** -40
NAMES = ["train_loss", "inverse_reconstruct_train_mean", "reconstruct_train_mean", "shifted_degrade_img_mean", "degraded_train_mean"]


def _grid(npix):
    return min(256, max(1, -(-npix // 256)))


def _sum_bound(absmean, N, C, H, W):
    npix = N * H * W
    G = _grid(npix)
    k = C * -(-npix // (G * 256))
    return (k + 8) * 2.0 ** -24 * absmean + G * 2.0 ** -41


def _check_norm(col, opt):
    """Column 6 is the IEEE correctly rounded fp32 square root (`__fsqrt_rn`) of the word the optimizer's clip read, so it equals
    numpy's fp32 sqrt of that word bit for bit -- and `optimizer.grad_norm()`, which is torch's sqrt of the same word."""
    want = np.sqrt(np.float32(opt.sqnorm.item()))
    gn = opt.grad_norm()
    print(f"grad norm: ring {float(col)!r} sqrt(sqnorm) {float(want)!r} grad_norm() {gn!r}")
    assert np.float32(col) == want, (float(col), float(want))
    assert float(col) == gn, (float(col), gn)


def T(a):
    return torch.from_numpy(np.asarray(a))


# ------------------------------------------------------------------------------------------ kernel level
def _run_loss(mon, dt, pred, x_in, s, x0, w, x_t, shape, gscale=0.5):
    from mdm import _lib
    from mdm._lib import call, ptr, stream
    N, C, H, W = shape
    dpred = torch.full_like(pred, 7.0)                       # sentinel: every element (pad channels too) must be written
    loss = torch.zeros(2, device="cuda", dtype=torch.int64)
    head = (dt, ptr(pred), ptr(x_in), ptr(s), ptr(x0), ptr(w), N, C, H, W, pred.shape[-1], gscale, ptr(dpred), ptr(loss))
    if not mon:
        call("mdm_loss_fwd_bwd", *head, stream())
        torch.cuda.synchronize()
        return dpred, loss, None
    acc = torch.zeros(6, device="cuda", dtype=torch.int64)
    call("mdm_loss_fwd_bwd_mon", *head, ptr(x_t), ptr(acc), stream())
    torch.cuda.synchronize()
    return dpred, loss, acc


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("shape", [(3, 3, 5, 5), (5, 1, 37, 37), (2, 3, 192, 192)])
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("with_s,with_w", [(False, False), (True, False), (False, True), (True, True)])
def test_loss_mon_kernel(shape, dt, with_s, with_w):
    """75 pixels (tail lanes of one workgroup, Cp = 8 padding) / 6845 pixels, 27 workgroups, one real channel of 8 / 73728 pixels:
    more than 256 x 256, so the 256-workgroup cap makes threads loop."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(N * 1000 + H)
    rn = lambda *sz: torch.randn(*sz, generator=g)
    tdt = torch.float32 if dt == 0 else torch.bfloat16
    pred = (rn(N, H, W, 8) * 0.5).to(tdt).cuda()             # NHWC, Cp = 8; the pad channels hold garbage on purpose
    x_in, x0, x_t = (rn(N, C, H, W) + 0.3).cuda(), rn(N, C, H, W).cuda(), (rn(N, C, H, W) * 0.7 - 0.2).cuda()
    s = (rn(N, C, H, W) * 0.4 + 0.1).cuda() if with_s else None
    w = (torch.rand(N, generator=g) + 0.5).cuda() if with_w else None
    d0, l0, _ = _run_loss(False, dt, pred, x_in, s, x0, w, x_t, shape)
    d1, l1, m1 = _run_loss(True, dt, pred, x_in, s, x0, w, x_t, shape)
    d2, l2, m2 = _run_loss(True, dt, pred, x_in, s, x0, w, x_t, shape)
    assert torch.equal(_bits(d0), _bits(d1)) and torch.equal(l0, l1), "dpred / loss words differ from mdm_loss_fwd_bwd"
    assert torch.equal(_bits(d1), _bits(d2)) and torch.equal(l1, l2)
    assert torch.equal(m1, m2), (m1.tolist(), m2.tolist())                     # integer atomics: same words run to run
    m = m1.tolist()
    assert m[4] == 0 and m[5] == 0 and l1[1].item() == 0
    # fp64 mean of the same fp32 expression over the same bits (pred as stored; IEEE fp32 add / sub are the same on the CPU)
    pv = pred.float().cpu()[..., :C].permute(0, 3, 1, 2).contiguous()
    rec = x_in.cpu() + pv
    inv = rec - s.cpu() if with_s else rec
    for q, (name, ten) in enumerate((("inverse", inv), ("recon", rec), ("x_in", x_in.cpu()), ("x_t", x_t.cpu()))):
        want = float(ten.double().mean())
        got = m[q] * Q40
        bound = _sum_bound(float(ten.double().abs().mean()), N, C, H, W)
        print(f"{name}: got {got:.10e} want {want:.10e} err {abs(got - want):.3e} bound {bound:.3e}")
        assert abs(got - want) <= bound, (name, got, want, bound)


def test_loss_mon_flags_a_partial_that_is_not_finite():
    """One inf in x_t: the workgroup that holds it bumps mon_q40[4] and adds nothing to that sum; loss, dpred and the other
    three sums are what they are without it."""
    shape = N, C, H, W = (2, 3, 24, 24)                        # 1152 pixels: 5 workgroups
    g = torch.Generator().manual_seed(9)
    pred = torch.randn(N, H, W, 8, generator=g).cuda()
    x_in, x0, x_t = (torch.randn(N, C, H, W, generator=g).cuda() for _ in range(3))
    _, l0, m0 = _run_loss(True, 0, pred, x_in, None, x0, None, x_t, shape)
    bad = x_t.clone()
    bad[0, 0, 0, 0] = float("inf")
    _, l1, m1 = _run_loss(True, 0, pred, x_in, None, x0, None, bad, shape)
    assert torch.equal(l0, l1) and torch.equal(m0[:3], m1[:3])
    assert m0[4].item() == 0 and m1[4].item() == 1 and m1[5].item() == 0
    # the other four workgroups' x_t partials are there: pixels 256 .. 1151
    rest = x_t.cpu().permute(0, 2, 3, 1).reshape(N * H * W, C)[256:].double().sum().item() / x_t.numel()
    assert abs(m1[3].item() * Q40 - rest) <= _sum_bound(float(x_t.abs().mean()), N, C, H, W)


def test_monitor_commit_kernel():
    from mdm import MonitorRing
    from mdm._lib import call, ptr, stream
    ring = MonitorRing("cuda", 3)
    q = lambda v: int(round(v * 2.0 ** 40))
    loss = torch.tensor([q(0.75), 0], device="cuda", dtype=torch.int64)
    vals = [0.5, -0.25, 1.5, 2.0 ** -40]
    gsq = torch.tensor([9.0], device="cuda")

    def fill(flags=3):
        ring.mon_q40.copy_(torch.tensor([q(v) for v in vals] + [flags, 0], dtype=torch.int64))

    def commit(gn):
        call("mdm_monitor_commit", ptr(loss), ptr(ring.mon_q40), ptr(gn), ptr(ring.ctr), ptr(ring.ring), ring.cap, stream())
        torch.cuda.synchronize()
    ring.ctr.fill_(4)                                          # row 4 % 3 = 1
    ring.cursor = ring.issued = 4
    fill()
    commit(gsq)
    rows = ring.ring.cpu().numpy()
    assert np.array_equal(rows[1], np.array([0.75, 0.5, -0.25, 1.5, 2.0 ** -40, 3.0, 3.0, 0.0], dtype=np.float32))
    assert not rows[0].any() and not rows[2].any()             # only its own row
    assert ring.ctr.item() == 5 and not ring.mon_q40.cpu().numpy().any()          # counter advanced, accumulators cleared
    assert loss.tolist() == [q(0.75), 0]                       # the loss words are only read
    fill(0)
    commit(None)                                               # a micro-step without an update: no norm
    row = ring.ring[2].cpu().numpy()
    assert np.isnan(row[5]) and row[0] == np.float32(0.75) and row[6] == 0 and ring.ctr.item() == 6
    loss[1] = 2                                                # the loss flag word
    fill(0)
    commit(gsq)
    row = ring.ring[0].cpu().numpy()                           # 6 % 3
    assert np.isnan(row[0]) and row[1] == 0.5 and row[5] == 3.0 and ring.ctr.item() == 7
    got, dropped = ring.read()
    assert dropped == 0 and got.shape == (3, 8) and got[0, 4] == np.float32(2.0 ** -40) and np.isnan(got[1, 5]) and np.isnan(got[2, 0])


# ------------------------------------------------------------------------------------------ step level
def _make_trainer(name, a, dt, loader=None, accum=1, n=4, ema=False):
    """As tests/test_path_gpu.py::_make_trainer builds them."""
    import mdm
    from oracle.unet_ref import random_params
    model = mdm.UNet(TINY, N=n, H=16, W=16, dtype=dt, params=random_params(TINY), use_graph=getattr(a, "use_graph", True))
    opt = mdm.AdamW(model, lr=1e-3)
    lr_s = mdm.get_lr_scheduler("constant", opt, 0, 10)
    acc = mdm.Accelerator(gradient_accumulation_steps=accum)
    e = mdm.EMA(model) if ema else None
    if name == "base":
        tr = mdm.BaseTrainer(a, loader, None, model, e, opt, lr_s, acc)
    else:
        tr = mdm.Trainer(a, loader, None, [None] * 3, model, e, opt, lr_s, acc)
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(a.ddpm_num_steps)
    tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    return tr, model


def _cfg(v):
    return [None if str(x) == "None" else str(x) for x in v]


def _fixture_args(g, name, **kw):
    st, sel, ch, kind, lw = _cfg(g[f"step_{name}_cfg"])
    return base_args(data_size=16, ddpm_schedule=kind, ddpm_num_steps=10, select_degrade_pixel=sel, degrade_channel=ch,
                     shift_type=st, loss_weight_use=(lw == "True"), batch_size=4, **kw)


@pytest.mark.parametrize("name", ["ms", "ms_w", "base"])
@pytest.mark.parametrize("dt", [0, 1])
def test_monitors_vs_reference(golden, name, dt):
    """The five attributes after one `_run_batch` against the reference's own (tests/golden/train_monitors.npz, written by
    make_monitor_golden.py from the reference run that also produced train_step.npz's `step_*`)."""
    g, gm = golden("train_step"), golden("train_monitors")
    assert np.array_equal(gm["mon_x0"], g["step_x0"]) and list(gm["mon_names"]) == NAMES
    a = _fixture_args(g, name, monitor=True)
    tr, model = _make_trainer(name, a, dt)
    assert tr.loss_names == NAMES and tr.mean_names == ["ema_sample_mean"]
    seed_all(500)
    r = tr._run_batch(0, (T(g["step_x0"]), None, None), 0, 1, 0, None, None)
    assert np.array_equal(tr.step.x_in.cpu().numpy(), g[f"step_{name}_xin"])           # same draws as the reference run
    want, absmean = gm[f"mon_{name}"], gm[f"mon_{name}_absmean"]
    got = [getattr(tr, k) for k in NAMES]
    assert all(isinstance(v, float) for v in got)
    assert (r if isinstance(r, float) else r[0]) == tr.train_loss
    for k, v, wv in zip(NAMES, got, want):
        print(f"{name} dt={dt} {k}: got {v:.9e} want {wv:.9e} diff {abs(v - wv):.3e}")
    loss_bar = (2e-5 if dt == 0 else 3e-2) * max(1.0, want[0])                          # test_train_step_vs_reference's
    assert abs(got[0] - want[0]) < loss_bar, (got[0], want[0])
    rel = 2e-4 if dt == 0 else 8e-2                                                     # the same test's bar on `pred`
    for q in (1, 2):            # through the network: pred may be rel * ||pred_ref|| away, so its mean rel * rms(pred_ref)
        bound = rel * float(gm[f"mon_{name}_pred_rms"]) + _sum_bound(absmean[q - 1], 4, 3, 16, 16)
        assert abs(got[q] - want[q]) <= bound, (NAMES[q], got[q], want[q], bound)
    f64 = gm[f"mon_{name}_f64"]     # fp64 means of the reference's own fp32 tensors: free of the reference's summation error
    for q in (3, 4):            # not through the network: bit-equal inputs, summation order only
        bound = _sum_bound(absmean[q - 1], 4, 3, 16, 16)
        print(f"{NAMES[q]}: vs fp64 mean {abs(got[q] - f64[q - 1]):.3e} bound {bound:.3e}")
        assert abs(got[q] - want[q]) <= bound, (NAMES[q], got[q], want[q], bound)
        assert abs(got[q] - f64[q - 1]) <= bound, (NAMES[q], got[q], f64[q - 1], bound)
    assert list(tr.get_current_losses().keys()) == NAMES
    assert list(tr.get_current_losses().values()) == got
    row = tr.step.mon.last()
    assert row[6] == 0 and row[7] == 0
    _check_norm(row[5], tr.optimizer)


def _device_args(**kw):
    return base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation",
                     rng_mode="device", seed=3, batch_size=4, use_ema=True, loss_weight_use=True, **kw)


def _names(rec):
    return [c[0] for c in rec.calls]


@pytest.mark.parametrize("form", ["eager", "graph", "cut"])
def test_monitor_on_does_not_change_the_step(form):
    """fp32, seeded device RNG, three steps: loss words, weights and EMA shadow bit-equal with `monitor` on and off; column 6 is
    the optimizer's pre-clip gradient norm; and the recorded launch list with monitors differs from the one without only by the
    loss entry's name and the trailing commit."""
    g = torch.Generator().manual_seed(78)
    x0 = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1
    outs = {}
    for mon in (False, True):
        kw = dict(use_graph=form != "eager", cut_step_graph=form == "cut")
        if mon:
            kw["monitor"] = True
        tr, model = _make_trainer("ms", _device_args(**kw), 0, ema=True)
        assert (tr.step.mon is not None) == mon
        words, norms = [], []
        for _ in range(3):
            loss = tr._run_batch(0, (x0, None, None), 0, 1, 0, None, None)
            words.append(tr.step.loss.raw.tolist())
            if mon:
                row = tr.step.mon.last()
                _check_norm(row[5], tr.optimizer)
                assert loss == float(np.float32(words[-1][0] * Q40)) and row[6] == 0
            norms.append(tr.optimizer.grad_norm())
        outs[mon] = (words, norms, model.store.P.clone(), tr.ema_model.shadow.clone(), tr.step._graphs)
    assert outs[False][0] == outs[True][0] and outs[False][1] == outs[True][1]
    assert torch.equal(outs[False][2], outs[True][2]) and torch.equal(outs[False][3], outs[True][3])
    gr_off, gr_on = outs[False][4], outs[True][4]
    assert gr_off[0] == gr_on[0] == ("cut" if form == "cut" else "whole")
    rec = (lambda x: x.rec) if form != "eager" else (lambda x: x)
    if form == "cut":
        off = _names(rec(gr_off[1])) + _names(rec(gr_off[4]))          # front + tail; the backward pieces come from one plan
        on = _names(rec(gr_on[1])) + _names(rec(gr_on[4]))
        assert [len(rec(p).calls) if p is not None else 0 for p, _ in gr_off[2]] == [len(rec(p).calls) if p is not None else 0 for p, _ in gr_on[2]]
    else:
        off, on = _names(rec(gr_off[1])), _names(rec(gr_on[1]))
    assert off.count("mdm_loss_fwd_bwd") == 1 and "mdm_monitor_commit" not in off and "mdm_loss_fwd_bwd_mon" not in off
    assert on == [("mdm_loss_fwd_bwd_mon" if n == "mdm_loss_fwd_bwd" else n) for n in off] + ["mdm_monitor_commit"]


def _loader(n_batches, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 3, 16, 16, generator=g) * 2 - 1, None, None) for _ in range(n_batches)]


def test_deferred_epoch_returns_the_undeferred_losses():
    """`_run_epoch` over 6 batches: monitor / monitor + defer / the same with a 4-row ring (mid-epoch read) -- one list, exactly."""
    runs = []
    for kw in (dict(), dict(defer_loss=True), dict(defer_loss=True, monitor_cap=4)):
        tr, model = _make_trainer("ms", _device_args(monitor=True, **kw), 0, loader=_loader(6), ema=True)
        losses = tr._run_epoch(0, 1, 0, None, None)
        assert len(losses) == 6 and all(isinstance(v, float) and np.isfinite(v) for v in losses)
        assert tr.step.mon.cap == kw.get("monitor_cap", 4096)
        assert tr.train_loss == losses[-1]                      # the attributes hold the last step's values either way
        runs.append((losses, model.store.P.clone()))
    assert runs[0][0] == runs[1][0] == runs[2][0], [r[0] for r in runs]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])
    assert len(set(runs[0][0])) == 6


def test_deferred_handles_and_a_ring_left_unread_past_cap():
    import mdm
    a = _device_args(monitor=True, defer_loss=True, monitor_cap=4)
    tr, model = _make_trainer("ms", a, 0, ema=True)
    hs = [tr._run_batch(i, b, 0, 1, 0, None, None) for i, b in enumerate(_loader(6))]
    assert not any(isinstance(h, float) for h in hs)
    assert float(hs[5]) == hs[5].item() and np.isfinite(float(hs[2]))
    with pytest.raises(RuntimeError, match="overwritten"):
        float(hs[0])                                            # rows 0 and 1 are gone
    with pytest.raises(RuntimeError, match="overwritten"):
        hs[1].item()
    rows, dropped = tr.step.mon.read()
    assert dropped == 2 and rows.shape == (4, 8) and [float(r[0]) for r in rows] == [float(h) for h in hs[2:]]
    # ... and an epoch whose ring overran raises instead of returning a short list
    tr.dataloader = _loader(3)
    real_read = tr.step.mon.read
    tr.step.mon.read = lambda: (real_read()[0], 1)
    with pytest.raises(RuntimeError, match="overran"):
        tr._run_epoch(0, 1, 0, None, None)
    with pytest.raises(ValueError):
        _make_trainer("ms", _device_args(defer_loss=True), 0)   # defer needs monitor


@pytest.mark.parametrize("mode", ["replay", "device"])
def test_gradient_accumulation_one_row_per_micro_step(mode):
    kw = dict(rng_mode="device", seed=3) if mode == "device" else {}
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", batch_size=4,
                  monitor=True, gradient_accumulation_steps=2, **kw)
    tr, model = _make_trainer("ms", a, 0, loader=_loader(4), accum=2)
    seed_all(11)
    losses = tr._run_epoch(0, 1, 0, None, None)
    rows, dropped = tr.step.mon.read()
    assert dropped == 0 and rows.shape == (4, 8) and tr.global_step == 2
    assert [float(v) for v in rows[:, 0]] == losses
    assert np.isnan(rows[0, 5]) and np.isnan(rows[2, 5])        # micro-steps that do not sync: no update, no norm
    assert np.isfinite(rows[1, 5]) and np.isfinite(rows[3, 5]) and rows[1, 5] > 0
    _check_norm(rows[3, 5], tr.optimizer)
    assert not rows[:, 6].any() and np.isfinite(rows[:, :5]).all()


def test_visualizer_gets_the_reference_losses_once_per_epoch(tmp_path):
    import os
    calls = []

    class Vis:
        def plot_current_losses(self, epoch, losses, kind):
            calls.append((epoch, losses, kind))
    d = {k: str(tmp_path / k) for k in ("train_loss", "checkpoint", "ema_sample_img")}
    for v in d.values():
        os.makedirs(v, exist_ok=True)
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", batch_size=4,
                  rng_mode="device", seed=3, monitor=True)
    tr, model = _make_trainer("ms", a, 1, loader=_loader(2))
    tr.train(0, 2, 0, 0, types.SimpleNamespace(list_dir=d), Vis())
    assert [c[0] for c in calls] == [0, 1] and all(c[2] == "value" for c in calls)
    for _, losses, _ in calls:
        assert list(losses.keys()) == NAMES and all(isinstance(v, float) and np.isfinite(v) for v in losses.values())
    assert calls[1][1] == tr.get_current_losses()
    tr.ema_sample_mean = torch.tensor(0.25)
    assert dict(tr.get_current_mean()) == {"ema_sample_mean": 0.25}


@pytest.mark.parametrize("dt", [0, 1])
def test_base_trainer_returns_the_same_three_numbers_without_the_layout_kernel(golden, dt, monkeypatch):
    from mdm import ops
    g = golden("train_step")
    x0 = T(g["step_x0"])
    tr0, _ = _make_trainer("base", _fixture_args(g, "base"), dt)
    seed_all(500)
    want = tr0._run_batch(0, (x0, None, None), 0, 1, 0, None, None)
    recon_abs = float(tr0.reconstructed_img.abs().mean())
    xt_abs = float(tr0.step.x_t.abs().mean())
    n_calls = []
    real = ops.nhwc_to_nchw
    monkeypatch.setattr(ops, "nhwc_to_nchw", lambda *a, **k: (n_calls.append(1), real(*a, **k))[1])
    tr1, _ = _make_trainer("base", _fixture_args(g, "base", monitor=True), dt)
    seed_all(500)
    got = tr1._run_batch(0, (x0, None, None), 0, 1, 0, None, None)
    assert not n_calls, "the monitored base trainer still launches nhwc_to_nchw"
    assert len(got) == 3 and all(isinstance(v, float) for v in got)
    print("base", dt, want, got)
    # the ring's loss column is the fp32 rounding of the same Q23.40 word LossCell converts in fp64: equal after that rounding
    assert got[0] == float(np.float32(want[0])) and torch.equal(tr0.step.loss.raw, tr1.step.loss.raw)
    assert abs(got[1] - want[1]) <= _sum_bound(recon_abs, 4, 3, 16, 16), (got[1], want[1])
    assert abs(got[2] - want[2]) <= _sum_bound(xt_abs, 4, 3, 16, 16), (got[2], want[2])
    assert got[1] == tr1.reconstruct_train_mean and got[2] == tr1.degraded_train_mean
