"""The inpainting sampler on the GPU (mdm.Sampler.sample_inpaint).

Upstream has no counterpart, so parity is against the restatement of tests/_inpaint_ref.py (itself the pinned oracle bit for bit when
nothing is given, tests/test_inpaint_cpu.py).  Replay mode: masks and shifts bit for bit, the other lists within the bounds
test_path_gpu.py::test_sampler_trajectories_vs_reference applies.  Given pixels come out bit-equal to `known`; with nothing given
the run is `sample` bit for bit in every loop; the one-graph-per-step loop equals the host-driven one; a step with the projection
records as many launches as one without; a 'matched' run walks exactly the steps `inpaint_start_index` names; two shards are the
whole batch.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _inpaint_ref as PR  # noqa: E402
from golden.make_golden import TINY, base_args, seed_all  # noqa: E402
from oracle.scheduler_ref import SchedulerRef  # noqa: E402
from oracle.unet_ref import UNetRef, random_params  # noqa: E402

NAMES = PR.HISTORY_NAMES
RTOL, ATOL = 2e-4, 1e-4               # of test_sampler_trajectories_vs_reference: 20 ATOL scale per element, 5 RTOL rel-L2
N, HW, T = 4, 16, 6


def _params():
    return random_params(TINY)


def _sampler(a, steps=T):
    import mdm
    s = mdm.Scheduler(a)
    s.update_ddpm_num_steps(steps)
    return s, mdm.Sampler(None, a, s, [None] * 3), s.get_timesteps_epoch(0, 1)


def _known(n=N, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, HW, HW, generator=g) * 2 - 1


def _keep(kind, ck=1, n=N):
    import mdm
    if kind == "box":
        k = mdm.inpaint_keep("box", n, HW, HW, top=4, left=4, height=8, width=8)              # 25 % unknown
    elif kind == "random":
        k = mdm.inpaint_keep("random", n, HW, HW, p=0.4, generator=torch.Generator().manual_seed(3))
    else:
        k = torch.zeros(n, 1, HW, HW) if kind == "none" else torch.ones(n, 1, HW, HW)
    if ck == 3:                         # per-channel: channel 1 keeps other pixels than channels 0 and 2
        k = torch.cat((k, k.flip(-1), k), 1)
    return k.contiguous()


@pytest.fixture(scope="module")
def fp32_model():
    import mdm
    return mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=0, params=_params()).eval()


@pytest.fixture(scope="module")
def ref_net():
    return UNetRef(TINY, _params()).eval()


# ------------------------------------------------------------------------------------------ replay mode against the restatement
# (sampling_mask_dependency, momentum_adaptive, start, mask, Ck, further args).  'dependent_t' runs for 'degraded_area' fills only; the
# exponential table keeps its smallest ratio at 0.1, so no image of 256 pixels is without a degraded pixel and no fill is 0 / 0.
CASES = [
    ("independent", "base_momentum", "latent", "box", 1, {}),
    ("dependent_prev", "base_sampling", "known_mean", "random", 3, dict(mean_area="channel-wise")),
    ("dependent_t", "base_momentum", "matched", "box", 1, dict(mean_option="degraded_area", ddpm_schedule="exponential")),
    ("independent", "base_sampling", "latent", "random", 1, dict(select_degrade_pixel="indexing", degrade_channel=None, ddpm_schedule="log")),
    ("independent", "base_momentum", "matched", "random", 3, dict(mean_area="channel-wise")),
    ("dependent_prev", "base_momentum", "known_mean", "box", 1, {}),
    ("dependent_t", "base_sampling", "latent", "random", 3, dict(mean_option="degraded_area", ddpm_schedule="exponential")),
]


def _args(dep, mode, extra, **kw):
    return base_args(**{**dict(data_size=HW, ddpm_num_steps=T, sample_num=N, sample_latent_shape="uniform", sampling_mask_dependency=dep,
                               momentum_adaptive=mode), **extra, **kw})


def _reference(a, ref_net, known, keep, start, seed):
    s = SchedulerRef(a)
    s.update_ddpm_num_steps(a.ddpm_num_steps)
    ts = s.get_timesteps_epoch(0, 1)
    seed_all(seed)
    return ts, PR.InpaintSamplerRef(None, a, s, [None] * 3).sample_inpaint(ref_net, ts, known, keep, start)


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


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-Ck{c[4]}" for c in CASES])
def test_trajectories_vs_restatement(fp32_model, ref_net, case):
    dep, mode, start, mask, ck, extra = case
    a = _args(dep, mode, extra)
    known, keep = _known(), _keep(mask, ck)
    s, smp, ts = _sampler(a)
    rts, (rx0, rhist) = _reference(a, ref_net, known, keep, start, seed=40)
    assert ts == rts
    seed_all(40)
    x0, hist = smp.sample_inpaint(fp32_model, ts, known.cuda(), keep.cuda(), start)
    assert len(hist) == 11 and all(tuple(h.shape) == (len(ts) + 1, N, 3, HW, HW) and not h.is_cuda for h in hist)
    _within("-".join(map(str, case[:5])), hist, x0, rhist, rx0)
    given = (keep != 0).expand(N, 3, HW, HW)
    assert torch.equal(x0.cpu()[given], known[given])
    if start == "matched":
        steps = PR.start_index(s.ratio_list, ts, float((~given).any(1).sum((1, 2)).max()) / (HW * HW)) + 1
        assert 1 <= steps < len(ts) and all(not h[steps + 1:].any() for h in hist) and hist[NAMES.index("sample_0")][steps].any()


# ------------------------------------------------------------------------------------------ exactness
def _bits_equal(a, b):
    return np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("start", PR.STARTS)
def test_given_pixels_come_out_bit_equal(dtype, start):
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=dtype, params=_params()).eval()
    a = _args("independent", "base_momentum", {}, sample_history="device", rng_mode="device", seed=9)
    s, smp, ts = _sampler(a)
    known, keep = _known().cuda(), _keep("random", 3).cuda()
    known[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1e-40, -1.0])              # a signed zero and a denormal pass through too
    keep[0, 0, 0, :4] = 1
    x0, hist = smp.sample_inpaint(model, ts, known, keep, start)
    torch.cuda.synchronize()
    given = keep != 0
    assert bool(given.any()) and not bool(given.all()) and _bits_equal(x0[given], known[given])
    assert not _bits_equal(x0[~given], known[~given]) and bool(torch.isfinite(x0).all())
    h0 = hist[NAMES.index("sample_0")]
    filled = [k for k in range(h0.shape[0]) if bool(h0[k].any())]
    assert filled == list(range(1, len(filled) + 1)) and (len(filled) == len(ts) or start == "matched")
    for k in filled:
        assert _bits_equal(h0[k][given], known[given]), k
    assert _bits_equal(h0[filled[-1]], x0)


# ------------------------------------------------------------------------------------------ nothing given: `sample`
@pytest.mark.parametrize("loop", ["replay", "device", "graph"])
def test_nothing_given_is_sample_bit_for_bit(loop):
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=1 if loop != "replay" else 0, params=_params()).eval()
    kw = {} if loop == "replay" else dict(rng_mode="device", seed=7, sample_history=False, sampler_graph=loop == "graph")
    outs = []
    for inpaint in (False, True):
        a = _args("dependent_prev", "base_momentum", {}, **kw)
        s, smp, ts = _sampler(a)
        seed_all(23)
        if inpaint:
            x0, hist = smp.sample_inpaint(model, ts, _known().cuda(), _keep("none").cuda())
        else:
            x0, hist = smp.sample(model, ts)
        torch.cuda.synchronize()
        assert hasattr(smp, "_graph_keep") == (loop == "graph")
        outs.append((x0.cpu().clone(), [h.clone() for h in hist], torch.rand(3)))
    (x0, hist, after), (y0, yhist, yafter) = outs
    assert _bits_equal(x0, y0) and torch.equal(after, yafter) and bool(torch.isfinite(x0).all())
    assert len(hist) == len(yhist) == (11 if loop == "replay" else 0)
    for k, h, y in zip(NAMES, hist, yhist):
        assert _bits_equal(h, y), k


# ------------------------------------------------------------------------------------------ the graph loop
def _device_run(start, graph, keep, dtype=1, mode="base_momentum", dep="independent"):
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=dtype, params=_params()).eval()
    a = _args(dep, mode, {}, rng_mode="device", seed=5, sample_history=False, sampler_graph=graph)
    s, smp, ts = _sampler(a)
    seed_all(2)
    x0, hist = smp.sample_inpaint(model, ts, _known().cuda(), keep.cuda(), start)
    torch.cuda.synchronize()
    assert hist == [] and hasattr(smp, "_graph_keep") == graph                # the graph loop ran exactly where it was asked for
    return smp, ts, x0.cpu().clone()


@pytest.mark.parametrize("start", ["latent", "matched"])
@pytest.mark.parametrize("mode", ["base_momentum", "base_sampling"])
def test_one_graph_per_step_equals_the_host_driven_loop(start, mode):
    keep = _keep("box")
    (_, _, host), (smp, ts, graph) = (_device_run(start, flag, keep, mode=mode) for flag in (False, True))
    assert _bits_equal(host, graph) and bool(torch.isfinite(host).all())
    given = (keep != 0).expand(N, 3, HW, HW)
    assert _bits_equal(graph[given], _known()[given])
    ts_dev = smp._graph_keep[0][1]                                           # what mdm_sampler_step_params walks
    assert ts_dev.tolist() == (ts[:3] if start == "matched" else ts)         # a quarter box on the linear table: three steps


def test_a_step_with_the_projection_records_as_many_launches():
    import mdm
    model = mdm.UNet(TINY, N=N, H=HW, W=HW, dtype=1, params=_params()).eval()
    recs = []
    for inpaint in (False, True):
        a = _args("independent", "base_momentum", {}, rng_mode="device", seed=5, sample_history=False)
        s, smp, ts = _sampler(a)
        if inpaint:
            smp.sample_inpaint(model, ts, _known().cuda(), _keep("box").cuda())
        else:
            smp.sample(model, ts)
        torch.cuda.synchronize()
        recs.append([[name for name, _, _ in g.rec.calls] for g in smp._graph_keep[1:]])      # the body graph and the last graph
    swap = lambda names: ["mdm_inpaint_x0" if n == "mdm_sampler_x0" else n for n in names]
    for plain, proj in zip(*recs):
        assert len(plain) == len(proj) and swap(plain) == proj
        assert plain.count("mdm_sampler_x0") == 1 and proj.count("mdm_inpaint_x0") == 1 and "mdm_inpaint_x0" not in plain


# ------------------------------------------------------------------------------------------ 'matched'
def _hooked(smp):
    calls = []
    smp.step_hook = lambda i, slot, x_t: calls.append((i, slot))
    return calls


def test_matched_runs_the_steps_the_start_index_names(fp32_model):
    import mdm
    a = _args("independent", "base_momentum", {})
    s, smp, ts = _sampler(a)
    keep = _keep("box")
    j = mdm.inpaint_start_index(s.ratio_list, ts, 0.25)
    assert ts == [1, 2, 3, 4, 5, 6] and j == 2
    calls = _hooked(smp)
    seed_all(1)
    x0, hist = smp.sample_inpaint(fp32_model, ts, _known().cuda(), keep.cuda(), "matched")
    assert calls == [(2, 1), (1, 2), (0, 3)]
    for k, h in zip(NAMES, hist):
        assert tuple(h.shape) == (T + 1, N, 3, HW, HW) and not h[0].any() and not h[j + 2:].any(), k
    for k in ("sample_t", "shifted", "mask", "sample_0"):
        assert all(hist[NAMES.index(k)][slot].any() for slot in (1, 2, 3)), k
    # the start is keep ? known : mean, and it is what the first step read
    given = (keep != 0).expand(N, 3, HW, HW)
    start = hist[NAMES.index("sample_t")][1]
    assert torch.equal(start[given], _known()[given])
    mean = torch.stack([_known()[n][given[n]].double().mean() for n in range(N)])
    fill = start[~given].reshape(N, -1)                                      # (every image has the same number of unknown elements)
    # one constant per image; its distance from the fp64 mean is bounded in test_inpaint_kernels_gpu.py (576 terms below 1: < 1e-4)
    assert bool((fill == fill[:, :1]).all()) and float((fill - mean[:, None]).abs().max()) < 1e-4


def test_matched_uses_the_largest_hole_of_the_batch(fp32_model):
    import mdm
    a = _args("independent", "base_momentum", {}, sample_history=False)
    small = mdm.inpaint_keep("box", N, HW, HW, top=6, left=6, height=4, width=4)              # 16 / 256 everywhere ...
    mixed = small.clone()
    mixed[2] = _keep("box")[2]                                                # ... and 64 / 256 in one image
    want = {}
    for name, keep in (("small", small), ("mixed", mixed)):
        s, smp, ts = _sampler(a)
        calls = _hooked(smp)
        seed_all(1)
        smp.sample_inpaint(fp32_model, ts, _known().cuda(), keep.cuda(), "matched")
        want[name] = len(calls)
    assert want == {"small": mdm.inpaint_start_index(s.ratio_list, ts, 16 / 256) + 1, "mixed": 3} and want["small"] < 3


# ------------------------------------------------------------------------------------------ sharding
@pytest.mark.parametrize("start", PR.STARTS)
def test_two_shards_are_the_whole_batch(fp32_model, start):
    """rows [0, 2) and rows [2, 4) against all four rows in one process, in replay mode (every host draw is the full batch's, sliced);
    the larger hole lies in row 3, so the first shard of a 'matched' run must take its start index from the other shard's image"""
    import mdm
    half = mdm.UNet(TINY, N=2, H=HW, W=HW, dtype=0, params=_params()).eval()
    known = _known().cuda()
    keep = mdm.inpaint_keep("box", N, HW, HW, top=6, left=6, height=4, width=4)
    keep[3] = _keep("box")[3]
    keep = keep.cuda()
    a = _args("dependent_prev", "base_momentum", {})
    s, smp, ts = _sampler(a)
    seed_all(3)
    x0, full = smp.sample_inpaint(fp32_model, ts, known, keep, start)
    parts = []
    for lo in (0, 2):
        s, smp, ts = _sampler(a)
        calls = _hooked(smp)
        seed_all(3)
        parts.append(smp._sample_inpaint(half, ts, known, keep, start, rows=(lo, lo + 2)))
        assert len(calls) == (3 if start == "matched" else len(ts)), (lo, calls)
        assert smp.args is a and s.replay_rows is None
    for k in ("shift", "degraded_mask"):
        j = NAMES.index(k)
        got = torch.cat([p[1][j] for p in parts], 1)
        assert tuple(got.shape) == tuple(full[j].shape) and torch.equal(got, full[j]), k
    got = torch.cat([p[0] for p in parts], 0)
    given = (keep != 0).expand(N, 3, HW, HW)
    assert _bits_equal(got[given], known[given])
    rel = float((got - x0).norm() / x0.norm())
    print(f"two shards vs the whole batch ({start}): x0 rel-L2 {rel:.3e}")
    assert rel < 1e-3, rel


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_argument(fp32_model):
    a = _args("independent", "base_momentum", {})
    s, smp, ts = _sampler(a)
    known, keep = _known().cuda(), _keep("box").cuda()
    bad = [
        (dict(known=known[:3].contiguous()), ValueError, "known"), (dict(known=known[:, :2].contiguous()), ValueError, "known"),
        (dict(known=torch.zeros(N, 3, HW, 8, device="cuda")), ValueError, "known"),
        (dict(keep=torch.ones(N, 2, HW, HW, device="cuda")), ValueError, "keep"), (dict(keep=keep[:2].contiguous()), ValueError, "keep"),
        (dict(keep=torch.ones(N, 1, HW, 8, device="cuda")), ValueError, "keep"), (dict(keep=torch.ones(N, HW, HW, device="cuda")), ValueError, "keep"),
        (dict(known=known.double()), TypeError, "known"), (dict(keep=keep.bool()), TypeError, "keep"),
        (dict(known=known.transpose(2, 3)), ValueError, "known"), (dict(keep=keep.expand(N, 3, HW, HW)), ValueError, "keep"),
        (dict(known=known.cpu()), ValueError, "known"), (dict(keep=keep.cpu()), ValueError, "keep"),
        (dict(known=known.cpu().numpy()), TypeError, "known"),
        (dict(start="mean"), ValueError, "start"), (dict(start=None), ValueError, "start"),
    ]
    for change, err, word in bad:
        kw = dict(dict(known=known, keep=keep, start="latent"), **change)
        seed_all(0)
        with pytest.raises(err, match=word):
            smp.sample_inpaint(fp32_model, ts, kw["known"], kw["keep"], kw["start"])
        assert torch.equal(torch.rand(2), (seed_all(0), torch.rand(2))[1])   # refused before any host draw
    # what `sample` refuses stays refused, with the same exception
    for extra in (dict(sampling_mask_dependency="dependent"), dict(momentum_adaptive="momentum"), dict(momentum_adaptive="boosting"),
                  dict(sampling_mask_dependency="dependent_t", mean_option=0)):
        b = _args("independent", "base_momentum", extra)
        s, smp, ts = _sampler(b)
        raised = []
        for f in (lambda: smp.sample(fp32_model, ts), lambda: smp.sample_inpaint(fp32_model, ts, known, keep)):
            with pytest.raises(Exception) as ei:
                f()
            raised.append(type(ei.value))
        torch.cuda.synchronize()
        assert raised[0] is raised[1], (extra, raised)
