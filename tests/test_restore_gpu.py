"""The restoration sampler on the GPU (mdm.Sampler.sample_restore, evaluate_restore, mdm.restore_measure / restore_expand).

Upstream has no counterpart, so parity is against the restatement of tests/_restore_ref.py (itself the pinned oracle bit for bit when
the projection is skipped, tests/test_restore_cpu.py).  Replay mode: masks and shifts bit for bit, the other lists within the bounds
test_path_gpu.py::test_sampler_trajectories_vs_reference applies.  The result has the measurement to the kernel's bound; the
one-graph-per-step loop equals the host-driven one; a step with the projection records as many launches as one without; two shards
are the whole batch; `evaluate_restore` leaves both RNG states as it found them.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _restore_ref as RR  # noqa: E402
from golden.make_golden import TINY, base_args, seed_all  # noqa: E402
from oracle.scheduler_ref import SchedulerRef  # noqa: E402
from oracle.unet_ref import UNetRef, random_params  # noqa: E402

NAMES = RR.HISTORY_NAMES
RTOL, ATOL = 2e-4, 1e-4               # of test_sampler_trajectories_vs_reference: 20 ATOL scale per element, 5 RTOL rel-L2
N, HW, T = 4, 16, 6


def _params():
    return random_params(TINY)


def _sampler(a, steps=T):
    import mdm
    s = mdm.Scheduler(a)
    s.update_ddpm_num_steps(steps)
    return s, mdm.Sampler(None, a, s, [None] * 3), s.get_timesteps_epoch(0, 1)


def _truth(n=N, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, HW, HW, generator=g) * 2 - 1


def _measurement(pool, gray, n=N):
    """on the host, in fp64 rounded once: what the restatement and the device run are both given"""
    return RR.measure_t(_truth(n), pool, gray).contiguous()


@pytest.fixture(scope="module")
def fp32_model():
    import mdm
    return mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=0, params=_params()).eval()


@pytest.fixture(scope="module")
def ref_net():
    return UNetRef(TINY, _params()).eval()


def _args(dep, mode, extra, **kw):
    return base_args(**{**dict(data_size=HW, ddpm_num_steps=T, sample_num=N, sample_latent_shape="uniform", sampling_mask_dependency=dep,
                               momentum_adaptive=mode), **extra, **kw})


# ------------------------------------------------------------------------------------------ replay mode against the restatement
# (sampling_mask_dependency, momentum_adaptive, start, pool, gray, further args).  'dependent_t' runs for 'degraded_area' fills only; the
# exponential table keeps its smallest ratio at 0.1, so no image of 256 pixels is without a degraded pixel and no fill is 0 / 0.
CASES = [
    ("independent", "base_momentum", "latent", 2, False, {}),
    ("dependent_prev", "base_sampling", "measured", 4, True, dict(mean_area="channel-wise")),
    ("dependent_t", "base_momentum", "measured", 1, True, dict(mean_option="degraded_area", ddpm_schedule="exponential")),
    ("independent", "base_sampling", "measured", 2, False, dict(mean_area="channel-wise")),
    ("dependent_prev", "base_momentum", "latent", 1, True, {}),
    ("dependent_t", "base_sampling", "latent", 4, True, dict(mean_option="degraded_area", ddpm_schedule="exponential")),
    ("independent", "base_momentum", "measured", 8, False, dict(select_degrade_pixel="indexing", degrade_channel=None, ddpm_schedule="log")),
]


def _reference(a, ref_net, y, pool, gray, start, seed):
    s = SchedulerRef(a)
    s.update_ddpm_num_steps(a.ddpm_num_steps)
    ts = s.get_timesteps_epoch(0, 1)
    seed_all(seed)
    return ts, RR.RestoreSamplerRef(None, a, s, [None] * 3).sample_restore(ref_net, ts, y, pool, gray, start)


def _within(tag, hist, x0, rhist, rx0):
    for k in ("shift", "degraded_mask", "degraded_mask_next"):
        j = NAMES.index(k)
        assert np.array_equal(hist[j].numpy().view(np.uint32), rhist[j].numpy().view(np.uint32)), (tag, k)
    for j, k in enumerate(NAMES):
        h, r = hist[j].numpy(), rhist[j].numpy()
        assert h.shape == r.shape and np.isfinite(r).all(), (tag, k)
        scale = max(1.0, float(np.abs(r).max()))
        err, l2 = float(np.abs(h - r).max()), float(np.linalg.norm(h - r))
        print(f"{tag} {k}: max |diff| {err:.3e} (scale {scale:.2f}), rel-L2 {l2 / max(np.linalg.norm(r), 1e-6):.3e}")
        assert err < 20 * ATOL * scale, (tag, k, err, scale)
        assert l2 <= 5 * RTOL * max(np.linalg.norm(r), 1e-6) + 1e-7, (tag, k)
    rel = float(np.linalg.norm(x0.cpu().numpy() - rx0.numpy()) / np.linalg.norm(rx0.numpy()))
    print(f"{tag} x0: rel-L2 {rel:.3e}")
    assert rel < 1e-3, (tag, rel)


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-pool{c[3]}-gray{int(c[4])}" for c in CASES])
def test_trajectories_vs_restatement(fp32_model, ref_net, case):
    dep, mode, start, pool, gray, extra = case
    a = _args(dep, mode, extra)
    y = _measurement(pool, gray)
    s, smp, ts = _sampler(a)
    rts, (rx0, rhist) = _reference(a, ref_net, y, pool, gray, start, seed=40)
    assert ts == rts
    seed_all(40)
    x0, hist = smp.sample_restore(fp32_model, ts, y.cuda(), pool, gray, start)
    assert len(hist) == 11 and all(tuple(h.shape) == (len(ts) + 1, N, 3, HW, HW) and not h.is_cuda for h in hist)
    _within("-".join(map(str, case[:5])), hist, x0, rhist, rx0)
    first = hist[NAMES.index("sample_t")][1]
    assert bool((first == first[:, :, :1, :1]).all())                         # both starts are constant images
    if start == "measured":
        want, bound = RR.mu_ref(y.numpy(), 3, gray, a.mean_area == "channel-wise")
        assert (np.abs(first[:, :, 0, 0].double().numpy() - want) <= bound).all()


# ------------------------------------------------------------------------------------------ the result has the measurement
def _bits_equal(a, b):
    return np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pool,gray", [(2, False), (4, True), (1, True), (8, False)])
def test_the_result_has_the_measurement(dtype, pool, gray):
    """every sample_0 of the history is a projected image: its measurement (`restore_measure`, the kernel's own mean) lies within
    the mean's bound Em of its exact group mean, and that within the projection's per-element bound of y"""
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=dtype, params=_params()).eval()
    a = _args("independent", "base_momentum", {}, sample_history="device", rng_mode="device", seed=9)
    s, smp, ts = _sampler(a)
    y = mdm.restore_measure(_truth().cuda(), pool, gray)
    assert tuple(y.shape) == (N, 1 if gray else 3, HW // pool, HW // pool)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), RR.measure_np(_truth().numpy(), pool, int(gray)).view(np.uint32))
    x0, hist = smp.sample_restore(model, ts, y, pool, gray, "measured")
    torch.cuda.synchronize()
    h0 = hist[NAMES.index("sample_0")]
    assert not bool(h0[0].any()) and _bits_equal(h0[len(ts)], x0) and bool(torch.isfinite(x0).all())
    yn = y.cpu().numpy()
    sh0, sft = hist[NAMES.index("shifted_result")].cpu().numpy(), hist[NAMES.index("shift")].cpu().numpy()
    for slot in range(1, len(ts) + 1):
        img = h0[slot].cpu().numpy()
        x = (sh0[slot] - sft[slot]).astype(np.float32)                         # what mdm_sampler_x0 would have written: the unprojected x
        assert np.array_equal(img.view(np.uint32), RR.project_np(x, yn, pool, int(gray)).view(np.uint32)), slot
        ref, bound = RR.project_ref(x, yn, pool, int(gray))
        assert (np.abs(img.astype(np.float64) - ref) <= bound).all(), slot
        # the exact group mean of `ref` is y, so that of img lies within the largest bound of the group, and the fp32 mean within Em
        back = mdm.restore_measure(h0[slot].contiguous(), pool, gray).cpu().numpy().astype(np.float64)
        _, Em = RR.mean_ref(img, pool, int(gray))
        err = np.abs(back - yn)
        assert (err <= Em + RR.to_groups(bound, pool, int(gray)).max(-1)).all(), (slot, float(err.max()))
    assert float((x0 - _truth().cuda()).abs().max()) > 1e-3                    # (and it is not the truth: an untrained net)


# ------------------------------------------------------------------------------------------ the graph loop
def _device_run(start, graph, pool, gray, dtype=1, mode="base_momentum", dep="independent"):
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=dtype, params=_params()).eval()
    a = _args(dep, mode, {}, rng_mode="device", seed=5, sample_history=False, sampler_graph=graph)
    s, smp, ts = _sampler(a)
    seed_all(2)
    x0, hist = smp.sample_restore(model, ts, _measurement(pool, gray).cuda(), pool, gray, start)
    torch.cuda.synchronize()
    assert hist == [] and hasattr(smp, "_graph_keep") == graph                # the graph loop ran exactly where it was asked for
    return smp, ts, x0.cpu().clone()


@pytest.mark.parametrize("start,pool,gray", [("latent", 2, False), ("measured", 4, True), ("measured", 1, True)])
@pytest.mark.parametrize("mode", ["base_momentum", "base_sampling"])
def test_one_graph_per_step_equals_the_host_driven_loop(start, pool, gray, mode):
    (_, _, host), (smp, ts, graph) = (_device_run(start, flag, pool, gray, mode=mode) for flag in (False, True))
    assert _bits_equal(host, graph) and bool(torch.isfinite(host).all())
    assert smp._graph_keep[0][1].tolist() == ts                               # what mdm_sampler_step_params walks: every step
    other = _device_run("latent" if start == "measured" else "measured", True, pool, gray, mode=mode)[2]
    assert not _bits_equal(other, graph)                                      # the start is read


def test_a_step_with_the_projection_records_as_many_launches():
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=1, params=_params()).eval()
    recs = []
    for restore in (False, True):
        a = _args("independent", "base_momentum", {}, rng_mode="device", seed=5, sample_history=False)
        s, smp, ts = _sampler(a)
        if restore:
            smp.sample_restore(model, ts, _measurement(2, False).cuda(), 2)
        else:
            smp.sample(model, ts)
        torch.cuda.synchronize()
        recs.append([[name for name, _, _ in g.rec.calls] for g in smp._graph_keep[1:]])      # the body graph and the last graph
    swap = lambda names: ["mdm_restore_x0" if n == "mdm_sampler_x0" else n for n in names]
    for plain, proj in zip(*recs):
        assert len(plain) == len(proj) and swap(plain) == proj
        assert plain.count("mdm_sampler_x0") == 1 and proj.count("mdm_restore_x0") == 1 and "mdm_restore_x0" not in plain


# ------------------------------------------------------------------------------------------ sharding
@pytest.mark.parametrize("start", RR.STARTS)
def test_two_shards_are_the_whole_batch(fp32_model, start):
    """rows [0, 2) and rows [2, 4) against all four rows in one process, in replay mode (every host draw is the full batch's, sliced)"""
    import mdm
    half = mdm.UNet(TINY, N=2, H=HW, W=HW, dtype=0, params=_params()).eval()
    y = _measurement(2, True).cuda()
    a = _args("dependent_prev", "base_momentum", {})
    s, smp, ts = _sampler(a)
    seed_all(3)
    x0, full = smp.sample_restore(fp32_model, ts, y, 2, True, start)
    parts = []
    for lo in (0, 2):
        s, smp, ts = _sampler(a)
        seed_all(3)
        parts.append(smp._sample_restore(half, ts, y, 2, True, start, rows=(lo, lo + 2)))
        assert smp.args is a and s.replay_rows is None
    for k in ("shift", "degraded_mask"):
        j = NAMES.index(k)
        got = torch.cat([p[1][j] for p in parts], 1)
        assert tuple(got.shape) == tuple(full[j].shape) and torch.equal(got, full[j]), k
    j = NAMES.index("sample_t")                                               # the start rows are the whole batch's, bit for bit
    assert torch.equal(torch.cat([p[1][j][1] for p in parts], 0), full[j][1])
    got = torch.cat([p[0] for p in parts], 0)
    rel = float((got - x0).norm() / x0.norm())
    print(f"two shards vs the whole batch ({start}): x0 rel-L2 {rel:.3e}")
    assert rel < 1e-3, rel


# ------------------------------------------------------------------------------------------ evaluate_restore
@pytest.mark.parametrize("pool,gray", [(2, False), (1, True)])
def test_evaluate_restore(pool, gray):
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=1, params=_params()).eval()
    a = _args("independent", "base_momentum", {}, rng_mode="device", seed=4, sample_history=False)
    s, smp, ts = _sampler(a)
    truth = _truth().cuda()
    seed_all(17)
    host_state, dev_state = torch.get_rng_state().clone(), s.dev_rng.dev.clone()
    out = smp.evaluate_restore(model, ts, truth, pool, gray)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), host_state) and torch.equal(s.dev_rng.dev, dev_state)   # both states as found
    assert list(out) == ["latent", "measured", "expand"] and all(isinstance(v, mdm.ImageMetrics) for v in out.values())
    y = mdm.restore_measure(truth, pool, gray)
    want = mdm.image_metrics(mdm.restore_expand(y, 3, pool, gray), truth)
    for got, ref in zip(out["expand"], want):
        assert tuple(got.shape) == (N,) and got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint32), ref.cpu().numpy().view(np.uint32))
    # every start ran from the states found: the "latent" entry is a plain sample_restore from them
    x0, _ = smp.sample_restore(model, ts, y, pool, gray, "latent")
    torch.set_rng_state(host_state); s.dev_rng.dev.copy_(dev_state)
    lat = mdm.image_metrics(x0, truth)
    assert _bits_equal(out["latent"].psnr, lat.psnr) and not _bits_equal(out["latent"].psnr, out["measured"].psnr)
    assert bool(torch.isfinite(out["expand"].psnr).all())
    only = smp.evaluate_restore(model, ts, truth, pool, gray, starts=("measured",))
    assert list(only) == ["measured", "expand"] and _bits_equal(only["measured"].ssim, out["measured"].ssim)


def test_evaluate_restore_trajectory():
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=1, params=_params()).eval()
    a = _args("independent", "base_momentum", {}, rng_mode="device", seed=4, sample_history="device")
    s, smp, ts = _sampler(a)
    out = smp.evaluate_restore(model, ts, _truth().cuda(), 4, True, trajectory=True)
    assert tuple(out["latent"].psnr.shape) == (len(ts) + 1, N) and tuple(out["expand"].psnr.shape) == (N,)
    a.sample_history = False
    with pytest.raises(ValueError, match="trajectory"):
        smp.evaluate_restore(model, ts, _truth().cuda(), 4, True, trajectory=True)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_argument(fp32_model):
    a = _args("independent", "base_momentum", {})
    s, smp, ts = _sampler(a)
    y = _measurement(2, False).cuda()
    bad = [
        (dict(measurement=y[:3].contiguous()), ValueError, "measurement"), (dict(measurement=y[:, :1].contiguous()), ValueError, "measurement"),
        (dict(measurement=y, gray=True), ValueError, "measurement"), (dict(measurement=y, pool=4), ValueError, "measurement"),
        (dict(measurement=y.double()), TypeError, "measurement"), (dict(measurement=y.transpose(2, 3)), ValueError, "measurement"),
        (dict(measurement=y.cpu()), ValueError, "measurement"), (dict(measurement=y.cpu().numpy()), TypeError, "measurement"),
        (dict(pool=3), ValueError, "pool"), (dict(pool=1), ValueError, "pool=1"), (dict(gray=2), ValueError, "gray"),
        (dict(start="matched"), ValueError, "start"), (dict(start="known_mean"), ValueError, "start"), (dict(start=None), ValueError, "start"),
    ]
    for change, err, word in bad:
        kw = dict(dict(measurement=y, pool=2, gray=False, start="latent"), **change)
        seed_all(0)
        with pytest.raises(err, match=word):
            smp.sample_restore(fp32_model, ts, kw["measurement"], kw["pool"], kw["gray"], kw["start"])
        assert torch.equal(torch.rand(2), (seed_all(0), torch.rand(2))[1])   # refused before any host draw
    with pytest.raises(ValueError, match="inpaint and restore"):
        smp._sample_mean_shift_momentum(fp32_model, ts, inpaint=(y, y), restore=(y, 2, 0))
    # what `sample` refuses stays refused, with the same exception
    for extra in (dict(sampling_mask_dependency="dependent"), dict(momentum_adaptive="momentum"),
                  dict(sampling_mask_dependency="dependent_t", mean_option=0)):
        b = _args("independent", "base_momentum", extra)
        s, smp, ts = _sampler(b)
        raised = []
        for f in (lambda: smp.sample(fp32_model, ts), lambda: smp.sample_restore(fp32_model, ts, y, 2)):
            with pytest.raises(Exception) as ei:
                f()
            raised.append(type(ei.value))
        torch.cuda.synchronize()
        assert raised[0] is raised[1], (extra, raised)
