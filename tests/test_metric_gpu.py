"""The Python surface of the image metrics on the GPU (mdm/metrics.py, mdm.Sampler.evaluate_inpaint): `image_metrics` on a batch and on
a history view equals the kernel-level call bit for bit, `clamp=None` works, `mean_fill_baseline` equals its torch statement bit for
bit, and `evaluate_inpaint` on the trained 16 x 16 fixture net measures every start from the same draws, keeps the hole bookkeeping
(given pixels come out bit-equal to `known`, so the squared error of the whole image is the squared error of the hole), returns
T_run + 1 trajectory rows whose last is the `sample_0` row, and leaves the generator and Philox states as it found them.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _metric_bounds as MB  # noqa: E402
import _metric_ref as MR  # noqa: E402
from golden.make_golden import TINY, base_args, seed_all  # noqa: E402
from golden.make_trained_tiny import smooth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HW, T = 4, 16, 40


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _kernel_call(pred, truth, keep, clamp=(-1.0, 1.0), L=2.0):
    from mdm import _lib
    R, (n, C, H, W) = pred.numel() // truth[0].numel(), truth.shape
    need = _lib.load().mdm_metric_ws_bytes(R, C, H, W)
    ws, out = torch.empty(need // 8, dtype=torch.float64, device="cuda"), torch.empty(R, 8, device="cuda")
    _lib.call("mdm_metric_image", pred=pred.data_ptr(), truth=truth.data_ptr(), keep=keep.data_ptr() if keep is not None else None,
              Ck=keep.shape[1] if keep is not None else 0, R=R, N=n, C=C, H=H, W=W, clamp_lo=clamp[0], clamp_hi=clamp[1], data_range=L,
              ws=ws.data_ptr(), ws_bytes=need, out=out.data_ptr(), stream=_lib.stream())
    return out


def test_image_metrics_is_the_kernel_call():
    import mdm
    pred, truth = MR.draw_images("outside", 3 * N, N, 3, 20, 24)
    keep = MR.draw_keep("random", N, 3, 20, 24)
    d_pred, d_truth, d_keep = pred.cuda(), truth.cuda(), keep.cuda()
    hist = mdm.image_metrics(d_pred.view(3, N, 3, 20, 24), d_truth, d_keep)
    want = _kernel_call(d_pred, d_truth, d_keep)
    assert isinstance(hist, mdm.ImageMetrics) and hist._fields == MR.SLOTS
    for k, t in enumerate(hist):
        assert t.is_cuda and tuple(t.shape) == (3, N) and np.array_equal(_bits(t.reshape(-1)), _bits(want[:, k])), MR.SLOTS[k]
    batch = mdm.image_metrics(d_pred[N:2 * N], d_truth, d_keep)               # one slot of the history as a batch
    for k, t in enumerate(batch):
        assert tuple(t.shape) == (N,) and np.array_equal(_bits(t), _bits(hist[k][1])), MR.SLOTS[k]
    # against the fp64 statement, and with the clamp off, another range, no keep
    ref = MR.reference(pred, truth, keep)
    p = mdm.metrics.plan(3 * N, 3, 20, 24)
    MB.check("image_metrics", torch.stack([t.reshape(-1) for t in hist], 1), ref["out"], MB.out_bound(ref, p.tile_h, p.tile_w))
    off = mdm.ImageMetrics(*(t.reshape(-1) for t in mdm.image_metrics(d_pred.view(3, N, 3, 20, 24), d_truth, None, data_range=1.0, clamp=None)))
    ref = MR.reference(pred, truth, None, 1.0, None)
    MB.check("clamp=None", torch.stack(list(off), 1), ref["out"], MB.out_bound(ref, p.tile_h, p.tile_w))
    assert np.array_equal(_bits(torch.stack(list(off), 1)), _bits(_kernel_call(d_pred, d_truth, None, (0.0, 0.0), 1.0)))
    assert float((off.mse - hist.mse.reshape(-1)).abs().min()) > 0.1 and bool((off.hole_count == 3 * 20 * 24).all())


def test_image_metrics_refusals():
    import mdm
    pred, truth = (t.cuda() for t in MR.draw_images("noise", N, N, 3, 16, 16))
    keep = torch.ones(N, 1, 16, 16, device="cuda")
    for kw, err, word in ((dict(pred=pred[:, :2].contiguous()), ValueError, "pred"), (dict(pred=pred.double()), TypeError, "pred"),
                          (dict(truth=truth.cpu()), ValueError, "truth"), (dict(keep=keep[:2]), ValueError, "keep"),
                          (dict(keep=keep.expand(N, 3, 16, 16)), ValueError, "keep"), (dict(clamp=(1.0, -1.0)), ValueError, "clamp"),
                          (dict(pred=pred[:, :, :10].contiguous(), truth=truth[:, :, :10].contiguous(), keep=None), RuntimeError, "H = 10"),
                          (dict(data_range=0.0), RuntimeError, "data_range")):
        with pytest.raises(err, match=word):
            mdm.image_metrics(**dict(dict(pred=pred, truth=truth, keep=keep), **kw))


@pytest.mark.parametrize("mean_area", ["image-wise", "channel-wise"])
def test_mean_fill_baseline_is_its_torch_statement(mean_area):
    import mdm
    from mdm import _lib
    truth = smooth_images(N, torch.Generator().manual_seed(5)).cuda()
    keep = mdm.inpaint_keep("random", N, HW, HW, p=0.4, generator=torch.Generator().manual_seed(3)).cuda()
    keep[3] = 0                                                               # nothing given: the fill is 0
    got = mdm.metrics.mean_fill_baseline(truth, keep, mean_area)
    mu = torch.empty(N, 3, device="cuda")                                     # the fp32 mean as mdm_inpaint.h states it ...
    _lib.call("mdm_inpaint_start", known=truth.data_ptr(), keep=keep.data_ptr(), keep_C=1, fallback=torch.zeros(N, 3, device="cuda").data_ptr(),
              per_channel=int(mean_area == "channel-wise"), N=N, C=3, HW=HW * HW, x_start=None, mu=mu.data_ptr(), unknown=None,
              stream=_lib.stream())
    want = torch.where(keep != 0, truth, mu[:, :, None, None])                # ... selected by torch
    assert np.array_equal(_bits(got), _bits(want)) and not bool(got[3].any())
    given = (keep != 0).expand(N, 3, HW, HW)
    dims = (1, 2) if mean_area == "channel-wise" else (0, 1, 2)
    for n in range(3):                                                        # and that mean is the mean of the given values
        m64 = (truth[n].double() * given[n]).sum(dims) / given[n].sum(dims)
        assert float((mu[n].double() - m64).abs().max()) < 1e-5
    assert torch.equal(mdm.mean_fill_baseline(truth, keep, mean_area), got)


def _trained_model(n):
    import mdm
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_tiny.npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    return mdm.UNet(TINY, N=n, H=HW, W=HW, dtype=mdm.F32, params=params).eval()


def _setup(history):
    import mdm
    a = base_args(data_size=HW, ddpm_schedule="linear", ddpm_num_steps=T, shift_type="noise_with_perturbation",
                  sampling_mask_dependency="dependent_prev", momentum_adaptive="base_sampling", sample_num=N, sample_latent_shape="uniform",
                  sample_history=history, rng_mode="device", seed=11)
    s = mdm.Scheduler(a)
    s.update_ddpm_num_steps(T)
    return s, mdm.Sampler(None, a, s, [None] * 3), s.get_timesteps_epoch(0, 1)


@pytest.fixture(scope="module")
def problem():
    import mdm
    truth = smooth_images(N, torch.Generator().manual_seed(777)).contiguous().cuda()       # (the training drew from seed 2024)
    keep = mdm.inpaint_keep("box", N, HW, HW, top=5, left=4, height=6, width=7).cuda()
    return _trained_model(N), truth, keep


def test_evaluate_inpaint(problem):
    import mdm
    model, truth, keep = problem
    s, smp, ts = _setup(False)
    assert len(ts) == T
    seed_all(21)
    host0, dev0 = torch.get_rng_state(), s.dev_rng.dev.clone()
    res = smp.evaluate_inpaint(model, ts, truth, keep)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), host0) and torch.equal(s.dev_rng.dev, dev0)
    assert list(res) == ["latent", "known_mean", "matched"] and set(smp.inpaint_steps_run) == set(res)
    j = mdm.inpaint_start_index(s.ratio_list, ts, 42 / 256)
    assert smp.inpaint_steps_run == {"latent": T, "known_mean": T, "matched": j + 1} and j + 1 < T
    CHW = 3 * HW * HW
    for start, m in res.items():
        assert isinstance(m, mdm.ImageMetrics) and all(t.is_cuda and tuple(t.shape) == (N,) for t in m)
        assert bool((m.hole_count == 3 * 42).all()) and bool((m.hole_windows == 3 * 6 * 6).all())     # every map position of a 16 x 16
        assert bool(torch.isfinite(torch.stack(list(m))).all()), start                                # image is centred in rows 5 .. 10
        # given pixels are bit-equal to `known`: all of the squared error lies in the hole.  Both means are within
        # gamma(3) + 2^-24 (+ the double sums) of their exact values (tests/_metric_bounds.py): 2 (4 2^-24) relative covers the pair
        total, hole = m.mse.double() * CHW, m.mse_hole.double() * m.hole_count.double()
        assert bool(((total - hole).abs() <= 8 * 2.0 ** -24 * total).all()), (start, total, hole)
        assert bool((m.mse > 0).all()) and bool((m.psnr_hole < m.psnr).all())
    # the same draws: run again alone from the same states, the same bits
    seed_all(21)
    alone = smp.evaluate_inpaint(model, ts, truth, keep, starts=("matched",))
    for a, b in zip(alone["matched"], res["matched"]):
        assert np.array_equal(_bits(a), _bits(b))
    # and it is sample_inpaint's sample_0 that was measured
    seed_all(21)
    x0, _ = smp.sample_inpaint(model, ts, truth, keep, "known_mean")
    direct = mdm.image_metrics(x0, truth, keep)
    s.dev_rng.dev.copy_(dev0)
    for a, b in zip(direct, res["known_mean"]):
        assert np.array_equal(_bits(a), _bits(b))
    base = mdm.image_metrics(mdm.mean_fill_baseline(truth, keep), truth, keep)
    print("psnr_hole per start:", {k: [round(float(v), 2) for v in m.psnr_hole] for k, m in res.items()},
          "mean fill:", [round(float(v), 2) for v in base.psnr_hole])


def test_evaluate_inpaint_trajectory(problem):
    model, truth, keep = problem
    s, smp, ts = _setup("device")
    seed_all(21)
    host0, dev0 = torch.get_rng_state(), s.dev_rng.dev.clone()
    traj = smp.evaluate_inpaint(model, ts, truth, keep, trajectory=True)
    assert torch.equal(torch.get_rng_state(), host0) and torch.equal(s.dev_rng.dev, dev0)
    seed_all(21)
    last = smp.evaluate_inpaint(model, ts, truth, keep)
    for start, m in traj.items():
        steps = smp.inpaint_steps_run[start]
        assert steps == (T if start != "matched" else smp.inpaint_steps_run["matched"]) and 1 <= steps <= T
        for a, b in zip(m, last[start]):
            assert tuple(a.shape) == (steps + 1, N) and np.array_equal(_bits(a[-1]), _bits(b)), start
        assert bool((m.hole_count == 3 * 42).all())
    assert traj["matched"].mse.shape[0] < T + 1
    s2, smp2, _ = _setup(False)
    with pytest.raises(ValueError, match="sample_history"):
        smp2.evaluate_inpaint(model, ts, truth, keep, trajectory=True)
