"""The latent-interpolation sampler on the GPU (mdm.Sampler.sample_interpolation and the two Scheduler methods under it).

Replay mode against the reference's own trajectories (tests/golden/sampler_interp.npz): shifts, masks and mu bit for bit, the other
lists within the bounds test_path_gpu.py::test_sampler_trajectories_vs_reference uses for its flat-input ('1-d_constant') cases --
every start image here is one constant colour, the same ill-conditioned GroupNorm regime.  Device mode: the one-graph-per-step
loop against the host-driven loop bit for bit, the row mask shared by the batch, and two shards against the whole batch.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _interp_ref as IR  # noqa: E402
from golden.make_golden import TINY, base_args, seed_all  # noqa: E402

NAMES = IR.INTERP_HISTORY_NAMES
RTOL, ATOL = 2e-4, 1e-4               # of test_sampler_trajectories_vs_reference: 20 ATOL scale per element, 5 RTOL rel-L2


def _params():
    from oracle.unet_ref import random_params
    return random_params(TINY)


def _sampler(a, T=6):
    import mdm
    s = mdm.Scheduler(a)
    s.update_ddpm_num_steps(T)
    return s, mdm.Sampler(None, a, s, [None] * 3), s.get_timesteps_epoch(0, 1)


# ------------------------------------------------------------------------------------------ replay mode against the reference
@pytest.fixture(scope="module")
def fp32_model():
    import mdm
    return mdm.UNet(TINY, N=4, H=16, W=16, dtype=0, params=_params()).eval()


@pytest.mark.parametrize("i", range(4))
def test_trajectories_vs_reference(golden, fp32_model, i):
    g = golden("sampler_interp")
    assert int(g["interp_n"]) == 4
    a, shift = IR.fixture_args(g[f"interp{i}_cfg"], base_args)
    s, smp, ts = _sampler(a)
    assert ts == list(g[f"interp{i}_ts"])
    T = len(ts)
    seed_all(int(g[f"interp{i}_seed"]))
    x0, mu, hist = smp.sample_interpolation(fp32_model, ts, shift)
    ref = IR.fixture_hist(g, i, smp._get_latent_initial_interpolation(shift)[0].numpy())
    assert len(hist) == 10 and all(tuple(h.shape) == (T + 1, 4, 3, 16, 16) and not h.is_cuda for h in hist)
    assert mu.shape == (4, 1, 1, 1) and np.array_equal(mu.numpy(), g[f"interp{i}_mu"])
    for k in ("shift", "degraded_mask"):
        assert np.array_equal(hist[NAMES.index(k)].numpy(), ref[NAMES.index(k)]), (i, k)
    for j, k in enumerate(NAMES):
        h, r = hist[j].numpy(), ref[j]
        assert not h[0].any(), (i, k, "slot 0")
        if k in ("sample_t", "degraded_mask", "degraded_t", "difference", "degraded_next_t"):
            assert not h[T].any(), (i, k, "slot T")
        scale = max(1.0, float(np.abs(r).max()))
        err, l2 = float(np.abs(h - r).max()), float(np.linalg.norm(h - r))
        print(f"case {i} {k}: max |diff| {err:.3e} (scale {scale:.2f}), rel-L2 {l2 / max(np.linalg.norm(r), 1e-6):.3e}")
        assert err < 20 * ATOL * scale, (i, k, err, scale)
        assert l2 <= 5 * RTOL * max(np.linalg.norm(r), 1e-6) + 1e-7, (i, k)
    rel = np.linalg.norm(x0.cpu().numpy() - g[f"interp{i}_x0"]) / np.linalg.norm(g[f"interp{i}_x0"])
    print(f"case {i} x0: rel-L2 {rel:.3e}")
    assert rel < 1e-3, (i, rel)
    if str(g[f"interp{i}_cfg"][5]) == "indexing":
        assert not hist[NAMES.index("degraded_mask")].any()          # counts >= 1 > u: upstream's all-zero mask, kept


def test_failing_configurations_raise_what_the_reference_raises(golden, fp32_model):
    g = golden("sampler_interp")
    for j in range(int(g["interp_nfail"])):
        row = g[f"interp_fail{j}"]
        a, shift = IR.fixture_args(row[:-1], base_args)
        s, smp, ts = _sampler(a)
        with pytest.raises(Exception) as ei:
            smp.sample_interpolation(fp32_model, ts, shift)
        torch.cuda.synchronize()
        assert type(ei.value).__name__ == str(row[-1]), (j, type(ei.value).__name__, str(row[-1]))


def test_replay_draw_order():
    """'dependent' consumes sample_num randperm(HW) before the loop, any other value nothing; then one FloatTensor(1, HW) per i > 0"""
    import mdm
    model = mdm.UNet(TINY, N=4, H=16, W=16, dtype=0, params=_params()).eval()
    for dep, perms in (("dependent", 4), ("independent", 0), ("anything", 0)):
        a = base_args(data_size=16, ddpm_num_steps=6, sample_num=4, sampling_mask_dependency=dep, sample_history=False)
        s, smp, ts = _sampler(a)
        seed_all(77)
        smp.sample_interpolation(model, ts, 0.3)
        after = torch.rand(3)
        seed_all(77)
        for _ in range(perms):
            torch.randperm(256)
        for _ in range(len(ts) - 1):
            torch.FloatTensor(1, 256).uniform_(0, 1)
        assert torch.equal(after, torch.rand(3)), dep


def test_any_callable_model_and_the_step_hook():
    """A model that is no fused `UNet` goes through the same step body (the oracle runs the same callable on the CPU), and
    `step_hook(i, slot, x_t)` is called at the top of every step and may overwrite x_t in place."""
    import types
    net = lambda x, t: types.SimpleNamespace(sample=-0.5 * x + 0.01 * t[:, None, None, None])
    a = base_args(data_size=16, ddpm_schedule="exponential", ddpm_num_steps=6, sample_num=4, mean_option="degraded_area",
                  mean_area="channel-wise")
    s, smp, ts = _sampler(a)
    ref_s = IR.InterpSchedulerRef(a)
    ref_s.update_ddpm_num_steps(6)
    seed_all(21)
    rx0, rmu, rhist = IR.InterpSamplerRef(None, a, ref_s, [None] * 3)._sample_interpolation(net, ts, -0.4)
    seed_all(21)
    x0, mu, hist = smp.sample_interpolation(net, ts, -0.4)
    assert torch.equal(mu, rmu)
    for k in ("shift", "degraded_mask"):
        assert torch.equal(hist[NAMES.index(k)], rhist[NAMES.index(k)]), k
    # elementwise fp32 arithmetic on both sides; only the fills are sums (768 terms of size <= 2, another order), and a fill
    # enters every later step once: 6 steps x 768 x 2^-23 x 2
    tol = 6 * 768 * 2.0 ** -23 * 2
    for j, k in enumerate(NAMES):
        assert float((hist[j] - rhist[j]).abs().max()) <= tol, (k, float((hist[j] - rhist[j]).abs().max()))
    assert float((x0.cpu() - rx0).abs().max()) <= tol
    calls = []

    def hook(i, slot, x_t):
        calls.append((i, slot, tuple(x_t.shape), x_t.is_cuda))
        if i == 2:
            x_t.fill_(0.125)                                                 # teacher forcing: the step then starts from this x_t
    smp.step_hook = hook
    seed_all(21)
    _, _, forced = smp.sample_interpolation(net, ts, -0.4)
    T = len(ts)
    assert calls == [(i, T - i, (4, 3, 16, 16), True) for i in range(T - 1, -1, -1)]
    sh, shifted = forced[NAMES.index("shift")], forced[NAMES.index("shifted")]
    assert torch.equal(shifted[T - 2], 0.125 + sh[T - 2]) and torch.equal(shifted[1], hist[NAMES.index("shifted")][1])


# ------------------------------------------------------------------------------------------ the two Scheduler methods
def test_shift_method_is_the_emitter_and_the_formula():
    N = 5
    a = base_args(data_size=8, ddpm_schedule="exponential", ddpm_num_steps=10)
    s, _, _ = _sampler(a, 10)
    ref = IR.InterpSchedulerRef(a)
    ref.update_ddpm_num_steps(10)
    time = torch.tensor([1.0, 3.0, 10.0, 7.0, 10.0])
    mu = torch.tensor([-1.0, -0.2, 0.9, 0.4, float("nan")])[:, None, None, None]
    for shift in (0.3, -0.4, 0.0):
        got = s.get_schedule_shift_time_interpolation(time.cuda(), mu.squeeze().cuda(), shift)
        want = ref.get_schedule_shift_time_interpolation(time, mu.squeeze(), shift)
        assert got.shape == (N, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
        assert torch.equal(got.cpu()[:4], want[:4]) and bool(torch.isnan(got[4]).all()) and bool(torch.isnan(want[4]).all())
        ratio = torch.index_select(s.ratio_dev, 0, time.int().cuda() - 1).contiguous()
        x_t = (torch.rand(N, 3, 8, 8) * 2 - 1).cuda()
        sb, xb = torch.full_like(x_t, 9.0), torch.full_like(x_t, 9.0)
        s.emit_shift_interp(x_t, mu.reshape(N).cuda().contiguous(), ratio, shift, sb, xb)
        torch.cuda.synchronize()
        assert torch.equal(sb[:4], got[:4].expand(4, 3, 8, 8)) and torch.equal(xb[:4], x_t[:4] + got[:4])
        assert bool(torch.isnan(sb[4]).all()) and bool(torch.isnan(xb[4]).all())
    clamped = ref.get_schedule_shift_time_interpolation(time, mu.squeeze(), 0.3)[:4].reshape(4)
    plain = ((torch.ones(4) * 0.3) * ref.ratio_list[time.long() - 1][:4]).float()
    assert (clamped != plain).any() and (clamped == plain).any()       # both regimes are in the case


@pytest.mark.parametrize("mean_option", [0.25, "degraded_area", "non_degraded_area", "whatever"])
@pytest.mark.parametrize("sel", ["thresholding", "indexing"])
def test_degrade_method_is_the_emitters_and_the_formula(mean_option, sel):
    N, C, H = 3, 3, 8
    a = base_args(data_size=H, ddpm_schedule="log" if sel == "indexing" else "linear", ddpm_num_steps=10, select_degrade_pixel=sel,
                  degrade_channel="1-channel" if sel == "thresholding" else None)
    s, _, _ = _sampler(a, 10)
    ref = IR.InterpSchedulerRef(a)
    steps = ref.update_ddpm_num_steps(10)
    time = torch.tensor([3.0, float(steps // 2), float(steps - 1)])       # ratios >= 0.2 over 64 pixels: no mask without a degraded pixel
    amount = ref.get_black_area_num_pixels_time(time)
    g = torch.Generator().manual_seed(3)
    img = torch.rand(N, C, H, H, generator=g) * 2 - 1
    seed_all(55)
    want = ref.degrade_interpolation_sampling(amount, img, mean_option=mean_option, mean_area="channel-wise")
    seed_all(55)
    got = s.degrade_interpolation_sampling(s.get_black_area_num_pixels_time(time.cuda()), img.cuda(), mean_option=mean_option,
                                           mean_area="channel-wise")
    assert all(t.is_cuda and tuple(t.shape) == (N, C, H, H) for t in got)
    assert torch.equal(got[1].cpu(), want[1].contiguous())                                      # the mask, bit for bit
    # the fill is a mean of up to C H W fp32 terms of size <= 1, summed in another order: 2^-23 per term at worst
    tol = C * H * H * 2.0 ** -23
    assert float((got[0].cpu() - want[0]).abs().max()) <= tol and float((got[2].cpu() - want[2]).abs().max()) <= tol
    if isinstance(mean_option, str):                             # ANY string: the image-wise mean of the degraded area
        gone = 1 - want[1]
        mean = (img * gone).sum(dim=(1, 2, 3)) / gone.sum(dim=(1, 2, 3))
        assert float((got[2].cpu() - mean[:, None, None, None]).abs().max()) <= tol
    if sel == "indexing":
        assert amount.dtype == torch.int64 and int(amount.min()) >= 1 and not got[1].any()      # counts: the all-zero mask
    else:
        assert 0 < float(got[1].mean()) < 1
    # the emitters over caller-owned buffers give the same mask
    seed_all(55)
    mask = torch.full((N, C, H, H), 9.0, device="cuda")
    s.emit_row_mask(amount.to("cuda", torch.float64), mask, u_row=s.host_uniform_row(H * H))
    torch.cuda.synchronize()
    assert torch.equal(mask, got[1])


def test_degrade_method_without_a_mean_option_is_a_type_error():
    a = base_args(data_size=8, ddpm_num_steps=10)
    s, _, _ = _sampler(a, 10)
    with pytest.raises(TypeError):
        s.degrade_interpolation_sampling(torch.tensor([0.5, 0.5]), torch.zeros(2, 3, 8, 8))


# ------------------------------------------------------------------------------------------ device mode
def _device_run(mode, n, rows=None, rank=0, hist=False, graph=True, dtype=1, seed=5):
    import mdm
    model = mdm.UNet(TINY, N=n if rows is None else rows[1] - rows[0], H=16, W=16, dtype=dtype, params=_params()).eval()
    # (exponential: the smallest ratio is 0.1, so no row of 256 pixels is without a degraded pixel and no fill is 0 / 0)
    a = base_args(data_size=16, ddpm_schedule="exponential", ddpm_num_steps=8, sample_num=n, momentum_adaptive=mode, mean_option="degraded_area",
                  mean_area="channel-wise", sample_history=hist, rng_mode="device", seed=seed, rng_rank=rank, sampler_graph=graph)
    s, smp, ts = _sampler(a, 8)
    x0, mu, h = smp._sample_interpolation(model, ts, 0.3, rows=rows) if rows is not None else smp.sample_interpolation(model, ts, 0.3)
    torch.cuda.synchronize()
    return smp, s, x0, mu, h


@pytest.mark.parametrize("mode", ["base_momentum", "base_sampling"])
def test_one_graph_per_step_equals_the_host_driven_loop(mode):
    outs = []
    for flag in (False, True):
        smp, s, x0, mu, h = _device_run(mode, 4, graph=flag)
        assert h == [] and bool(torch.isfinite(x0).all()) and mu.shape == (4, 1, 1, 1)
        assert hasattr(smp, "_graph_keep") == flag              # the graph loop ran exactly where it was asked for
        outs.append(x0.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1]), np.abs(outs[0] - outs[1]).max()


def test_the_row_mask_is_shared_by_the_batch_and_follows_the_ratio():
    smp, s, x0, mu, h = _device_run("base_momentum", 4, hist="device")
    assert all(t.is_cuda for t in h)
    m = h[NAMES.index("degraded_mask")].cpu().numpy()
    T, ratio = 8, s.ratio_list.numpy()
    assert not m[0].any() and not m[T].any()
    for slot in range(1, T):
        t = T - slot + 1                                         # the step's timestep; the row is thresholded at ratio[t - 2]
        assert (m[slot] == m[slot][:1, :1]).all(), slot          # one row for every sample and channel
        r, frac = ratio[t - 2], float(m[slot][0, 0].mean())
        # 256 independent pixels kept with probability 1 - r: five binomial standard deviations and one pixel
        assert abs(frac - (1 - r)) <= 5 * np.sqrt(r * (1 - r) / 256) + 1 / 256, (slot, frac, 1 - r)
    rows = [m[slot][0, 0] for slot in range(1, T)]
    assert not any(np.array_equal(rows[i], rows[i + 1]) for i in range(len(rows) - 1))        # a new row every step


def test_two_shards_are_the_whole_batch():
    """rows [0, 2) under rng_rank 0 and rows [2, 4) under rng_rank 1 against all four rows in one process: the row mask drops the
    rank half of the key, so both shards threshold the row the whole batch thresholds"""
    _, _, x0, mu, full = _device_run("base_momentum", 4, hist="device", dtype=0)
    parts = [_device_run("base_momentum", 4, rows=(lo, lo + 2), rank=rank, hist="device", dtype=0) for rank, lo in ((0, 0), (1, 2))]
    for k in ("degraded_mask", "shift"):
        j = NAMES.index(k)
        got = torch.cat([p[4][j] for p in parts], 1)
        assert tuple(got.shape) == tuple(full[j].shape) and torch.equal(got, full[j]), k
    assert all(torch.equal(p[3], mu) for p in parts) and mu.shape == (4, 1, 1, 1)              # mu is the full grid on every shard
    got = torch.cat([p[2] for p in parts], 0)
    rel = float((got - x0).norm() / x0.norm())
    print(f"two shards vs the whole batch: x0 rel-L2 {rel:.3e}")
    assert rel < 1e-3, rel


def test_sample_still_ignores_interpolation_shift():
    import mdm
    model = mdm.UNet(TINY, N=2, H=16, W=16, dtype=0, params=_params()).eval()
    outs = []
    for kw in ({}, dict(interpolation_shift=0.3)):
        a = base_args(data_size=16, ddpm_num_steps=6, sample_num=2, sample_latent_shape="uniform", shift_type="1-d_constant")
        s, smp, ts = _sampler(a)
        seed_all(9)
        x0, hist = smp.sample(model, ts, **kw)
        outs.append((x0.cpu(), hist))
    assert torch.equal(outs[0][0], outs[1][0]) and len(outs[1][1]) == 11
    assert all(torch.equal(p, q) for p, q in zip(outs[0][1], outs[1][1]))
