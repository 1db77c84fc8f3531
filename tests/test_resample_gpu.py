"""unet6 `resample_with_conv=False` on the GPU: the two streaming kernels bit for bit and inside guard bands, the 3-level net against
the reference's own run (tests/golden/unet_resample.npz) and the CPU restatement, graph / eager / determinism, the uniform_t twin, one
train step and a short sampler run against the oracles, and the combination with drop_rate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _bounds import U_BF16, U_F32, Buf  # noqa: E402
from _resample_ref import NET3, UNetNoConvRef, random_params_noconv, resample_keys  # noqa: E402
from golden.make_golden import base_args, seed_all  # noqa: E402

DT = {"f32": 0, "bf16": 1}
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
NET3_POOL = dict(NET3, resample_with_conv=False)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ----------------------------------------------------------------------------- 1: the kernels
SHAPES = [(2, 1, 1, 8), (3, 3, 5, 40), (2, 16, 16, 128)]        # (N, H, W, C) of the SMALL map


def _up2(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_avgpool2(dt, shape):
    from mdm import ops
    N, H, W, C = shape
    dev, td = _dev(), TD[dt]
    g = torch.Generator().manual_seed(sum(shape))
    big = (torch.randn(N, 2 * H, 2 * W, C, generator=g) * 1.5 + 0.2).to(td)
    prior = torch.randn(N, H, W, C, generator=g).to(td)
    src = Buf(big.shape, td, dev, fill=big)
    out, sp, accd = Buf(shape, td, dev), Buf(shape, td, dev), Buf(shape, td, dev, fill=prior)
    ops.avgpool2(DT[dt], src.t, out.t, 0, N, H, W, C)
    ops.sumpool2(DT[dt], src.t, sp.t, 0, N, H, W, C)
    ops.avgpool2(DT[dt], src.t, accd.t, 1, N, H, W, C)
    torch.cuda.synchronize()
    for b in (src, out, sp, accd):
        assert b.guards_intact(), b.first_bad_guard()
    assert _same_bits(src.t, big.to(dev))
    y = out.t.cpu()
    assert bool(torch.isfinite(y.float()).all())
    # 0.25 x the sum pool of the same input, bit for bit (a power of two commutes with the rounding to storage)
    assert _same_bits(y, (sp.t.cpu().float() * 0.25).to(td))
    # against float64: three fp32 adds and one rounding to storage
    b64 = big.double()
    taps = [b64[:, 0::2, 0::2], b64[:, 0::2, 1::2], b64[:, 1::2, 0::2], b64[:, 1::2, 1::2]]
    ref = F.avg_pool2d(b64.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    bound = 3 * U_F32 * 0.25 * sum(t.abs() for t in taps) + (U_BF16 if dt == "bf16" else U_F32) * ref.abs()
    err = (y.double() - ref).abs()
    print("avgpool2", dt, shape, "worst err / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    # accumulate: torch's (dst.float() + contribution).to(storage) with the taps summed in the kernel's order
    f = big.float()
    contrib = 0.25 * (((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2])
    assert _same_bits(accd.t.cpu(), (prior.float() + contrib).to(td))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_upsample2(dt, shape):
    from mdm import ops
    N, H, W, C = shape
    dev, td = _dev(), TD[dt]
    g = torch.Generator().manual_seed(7 + sum(shape))
    small = (torch.randn(shape, generator=g) * 1.5 - 0.1).to(td)
    prior = torch.randn(N, 2 * H, 2 * W, C, generator=g).to(td)
    src = Buf(shape, td, dev, fill=small)
    one, quarter, accd = Buf(prior.shape, td, dev), Buf(prior.shape, td, dev), Buf(prior.shape, td, dev, fill=prior)
    ops.upsample2(DT[dt], src.t, one.t, 0, 1.0, N, H, W, C)
    ops.upsample2(DT[dt], src.t, quarter.t, 0, 0.25, N, H, W, C)
    ops.upsample2(DT[dt], src.t, accd.t, 1, 0.25, N, H, W, C)
    torch.cuda.synchronize()
    for b in (src, one, quarter, accd):
        assert b.guards_intact(), b.first_bad_guard()
    assert _same_bits(src.t, small.to(dev))
    up = _up2(small)
    assert _same_bits(one.t.cpu(), up)                                       # a bit copy of src[:, y // 2, x // 2]
    assert _same_bits(quarter.t.cpu(), (up.float() * 0.25).to(td))
    assert _same_bits(accd.t.cpu(), (prior.float() + 0.25 * up.float()).to(td))
    # and it is the backward of the average pool: <avgpool2(a), b> == <a, upsample2(0.25)(b)> up to rounding
    if dt == "f32":
        a = torch.randn(prior.shape, generator=g)
        pooled = torch.empty(shape, device=dev)
        ops.avgpool2(0, a.to(dev), pooled, 0, N, H, W, C)
        torch.cuda.synchronize()
        lhs = float((pooled.cpu().double() * small.double()).sum())
        rhs = float((a.double() * quarter.t.cpu().double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((a.double().abs() * quarter.t.cpu().double().abs()).sum())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_channel_count_must_be_a_multiple_of_8(dt):
    from mdm import ops
    dev, td = _dev(), TD[dt]
    a, b = torch.zeros(256, device=dev, dtype=td), torch.zeros(256, device=dev, dtype=td)
    with pytest.raises(RuntimeError, match="avgpool2"):
        ops.avgpool2(DT[dt], a, b, 0, 1, 1, 1, 12)
    with pytest.raises(RuntimeError, match="upsample2"):
        ops.upsample2(DT[dt], a, b, 0, 1.0, 1, 1, 1, 12)
    with pytest.raises(RuntimeError, match="avgpool2"):
        ops.avgpool2(DT[dt], a, b, 0, 1, 0, 1, 8)
    torch.cuda.synchronize()
    assert float(b.float().abs().sum()) == 0.0


# ----------------------------------------------------------------------------- 2: the whole net
_ORACLE = {}


def _oracle(g):
    """The CPU restatement's forward and every gradient on the fixture's inputs, in fp32 and -- the YARDSTICK -- fp64: how far the
    reference's own fp32 arithmetic is from the exact result (tests/test_path_gpu.py scales its bars the same way).  Computed once."""
    if not _ORACLE:
        params = random_params_noconv(NET3, int(g["seed"]))
        x, t, gy = (torch.from_numpy(g[k]) for k in ("x", "t", "gy"))
        for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            m = UNetNoConvRef(NET3_POOL, params, dtype=dtype)
            y = m(x, t).sample
            (y * gy.to(dtype)).sum().backward()
            _ORACLE[name] = (y.detach(), {k: p.grad for k, p in zip(m.keys, m.plist)})
        cat = lambda d: torch.cat([d[k].reshape(-1).double() for k in params])
        a, b = cat(_ORACLE["f32"][1]), cat(_ORACLE["f64"][1])
        _ORACLE["yard"] = float((a - b).norm() / b.norm())
        _ORACLE["params"] = params
    return _ORACLE


def _net(dt, g, N=2, **kw):
    from mdm import unet as U
    mode = dict(bf16=dict(dtype=1), f32=dict(dtype=0), f32_split=dict(dtype=0, f32_products="split"))[dt]
    return U.UNet(NET3_POOL, N=N, H=16, W=16, params=random_params_noconv(NET3, int(g["seed"])), **mode, **kw)


def _fwd_bwd(net, g):
    from mdm import ops
    x, t, gy = (torch.from_numpy(g[k]) for k in ("x", "t", "gy"))
    y = net(x, t).sample
    net.zero_grad()
    ops.nchw_to_nhwc(net.dt, gy.to(net.device), net.y_out.grad, 2, 3, 16, 16, net.cout_p)
    net.run_backward()
    torch.cuda.synchronize()
    return y.cpu(), net.store.grad_dict()


# the bars of tests/test_unet_gpu.py::test_unet_tiny_forward_backward; split products in the forward keep the fp32 bars (as the
# teacher-forced sampler test does)
@pytest.mark.parametrize("dt,tol_y,tol_g", [("f32", 2e-4, 2e-3), ("f32_split", 2e-4, 2e-3), ("bf16", 3e-2, 8e-2)])
def test_net3_forward_backward_vs_the_reference(golden, dt, tol_y, tol_g):
    g = golden("unet_resample")
    o = _oracle(g)
    f = max(1.0, 5.0 * o["yard"] / 2e-4)
    net = _net(dt, g)
    y, grads = _fwd_bwd(net, g)
    want = o["f32"][1]
    assert set(want) == set(grads) == {str(k) for k in g["keys"]}
    print("rel_l2_y", _rel(y, g["y"]), "yardstick", o["yard"])
    assert _rel(y, g["y"]) < tol_y
    rms = float(torch.cat([w.reshape(-1) for w in want.values()]).pow(2).mean().sqrt())

    def err(a, b):
        a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
        return float((a - b).norm() / (b.norm() + 1e-2 * rms * b.numel() ** 0.5))
    med = sorted(float(w.norm()) for w in want.values())[len(want) // 2]
    keys = [k for k in want if dt != "bf16" or float(want[k].norm()) > 1e-2 * med]
    assert len(keys) > 0.8 * len(want)
    worst = max((err(grads[k], want[k]), k) for k in keys)
    allg = torch.cat([grads[k].reshape(-1) for k in want]), torch.cat([want[k].reshape(-1) for k in want])
    print("worst", worst, "all", _rel(*allg))
    assert worst[0] < tol_g * f, worst
    assert _rel(*allg) < tol_g / 2 * f
    n = 0
    for k in g.files:
        if k.startswith("grad::"):
            print(k, err(grads[k.split("::")[1]], g[k]))
            assert err(grads[k.split("::")[1]], g[k]) < tol_g * f, k
            n += 1
    assert n == 4


def test_state_dict_round_trip_and_mismatched_dicts(golden):
    from mdm import unet as U
    from oracle.unet_ref import random_params
    g = golden("unet_resample")
    p = random_params_noconv(NET3, 5)
    net = U.UNet(NET3_POOL, N=1, H=16, W=16, dtype=1, params=p)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]] == list(p)
    assert all(torch.equal(sd[k], p[k]) for k in p)
    assert net.num_parameters() == sum(v.numel() for v in p.values())
    before = net.store.P.clone()
    full = random_params(NET3, 6)
    with pytest.raises(KeyError, match="downsamples.level_0.1.1.weight"):
        net.load_state_dict(full)                                           # a conv-model dict: unexpected keys, nothing loaded
    assert torch.equal(net.store.P, before)
    conv = U.UNet(NET3, N=1, H=16, W=16, dtype=1, params=full)
    before = conv.store.P.clone()
    with pytest.raises(KeyError, match="missing.*downsamples.level_0.1.1.weight"):
        conv.load_state_dict(p)
    assert torch.equal(conv.store.P, before)
    assert set(conv.state_dict()) - set(sd) == resample_keys(NET3)


# ----------------------------------------------------------------------------- 3: graph, eager, determinism, twins
def test_graph_equals_eager_and_the_fp32_backward_is_reproducible(golden):
    g = golden("unet_resample")
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    eager, graph = _net("f32", g, use_graph=False), _net("f32", g, use_graph=True)
    ye = eager(x, t).sample.clone()
    yg1 = graph(x, t).sample.clone()
    yg2 = graph(x, t).sample.clone()                                        # a replay of the captured graph
    assert _same_bits(ye, yg1) and _same_bits(ye, yg2)
    _, _ = _fwd_bwd(graph, g)
    G1 = graph.store.G.clone()
    _, _ = _fwd_bwd(graph, g)
    assert torch.equal(_bits(G1), _bits(graph.store.G)) and float(G1.abs().sum()) > 0
    _, _ = _fwd_bwd(eager, g)
    assert torch.equal(_bits(G1), _bits(eager.store.G))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_uniform_t_twin_is_bit_equal(golden, dt):
    g = golden("unet_resample")
    net = _net(dt, g).eval()
    x, t = torch.from_numpy(g["x"]), torch.full((2,), 41.0)
    y = net(x, t).sample.clone()
    twin = net.with_uniform_t()
    assert twin is not net and twin.uniform_t and twin.backward_plan is None and twin.resample_with_conv is False
    assert _same_bits(twin(x, t).sample, y)
    assert net.with_batch(3).resample_with_conv is False


def test_sampling_plans_of_a_bf16_model_build_and_run(golden):
    g = golden("unet_resample")
    net = _net("bf16", g).eval()
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    want = _net("f32", g).eval()(x, t).sample.clone()
    for prec, tol in (("f32_split", 5e-5), ("f32", 2e-6)):                # the bars of test_sampling_plan_follows_the_models_weights
        plan = net.sampling_plan(2, prec).eval()
        assert plan.dt == 0 and plan.resample_with_conv is False
        got = plan(x, t).sample.clone()
        torch.cuda.synchronize()
        assert _rel(got, want.cpu()) < tol, (prec, _rel(got, want.cpu()))


# ----------------------------------------------------------------------------- 4: one train step, then the captured graph
def test_train_step_vs_the_trainer_oracle_then_graph_steps():
    import mdm
    from oracle.scheduler_ref import SchedulerRef
    from oracle.trainer_ref import train_step_ref
    n, hw, T = 4, 16, 20
    a = base_args(data_size=hw, ddpm_num_steps=T, batch_size=n)            # mean-shift, thresholding / 1-channel, host RNG replay
    params = random_params_noconv(NET3, 1234)
    x0 = torch.rand(n, 3, hw, hw, generator=torch.Generator().manual_seed(11)) * 2 - 1
    model = mdm.UNet(NET3_POOL, N=n, H=hw, W=hw, dtype=mdm.F32, params=params)
    opt = mdm.AdamW(model, lr=1e-3)
    tr = mdm.Trainer(a, None, None, [None] * 3, model, None, opt, mdm.get_lr_scheduler("constant", opt, 0, 1), mdm.Accelerator())
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(T)
    used = tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    seed_all(7)
    loss = float(tr.step.run_replay(x0, used))
    got = model.state_dict()

    ref = UNetNoConvRef(NET3_POOL, params)
    assert list(ref.keys) == model.reference_param_order()
    ropt = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    rs = SchedulerRef(a)
    rs.update_ddpm_num_steps(T)
    seed_all(7)
    r = train_step_ref(ref, ropt, rs, a, x0, used, rs.rng)
    assert torch.equal(r["mask"], tr.step.mask.cpu()) and torch.equal(r["x_t"], tr.step.x_t.cpu())      # the same draws
    assert float((r["x_in"] - tr.step.x_in.cpu()).abs().max()) <= 1e-6      # z * ratio re-rounded (tests/test_device_path_gpu.py)
    want_loss = float(r["loss"])
    print("loss", loss, want_loss)
    assert abs(loss - want_loss) < 2e-5 * max(1.0, want_loss), (loss, want_loss)
    # weights after the AdamW step, where the oracle's gradient is well conditioned (tests/test_path_gpu.py, fp32: 2e-5)
    grads = {k: p.grad.numpy() for k, p in ref.pdict().items()}
    trms = {k: float(np.sqrt((v ** 2).mean())) for k, v in grads.items()}
    med = sorted(trms.values())[len(trms) // 2]
    checked = 0
    for k, v in ref.pdict().items():
        if trms[k] < 1e-3 * med:
            continue
        ok = np.abs(grads[k]) > 1e-3 * trms[k]
        d = np.abs(got[k].numpy() - v.detach().numpy())[ok]
        checked += int(ok.sum())
        assert d.max() <= 2e-5, (k, float(d.max()), int(ok.sum()))
    assert checked > 1000, checked
    # three steps of the device-RNG step as ONE captured graph, every one from the same Philox state (the same timesteps, masks and
    # shifts on the same batch): the loss cell must not rise
    start = tr.Scheduler.dev_rng.dev.clone()
    losses = []
    for _ in range(3):
        tr.Scheduler.dev_rng.dev.copy_(start)
        losses.append(float(tr.step.run_device(x0, used)))
    torch.cuda.synchronize()
    print("graph losses", losses)
    assert tr.step._graphs[0] == "whole" and np.isfinite(losses).all()
    assert losses[1] <= losses[0] and losses[2] <= losses[1], losses
    assert bool(torch.isfinite(model.store.P).all())


# ----------------------------------------------------------------------------- 5: the sampler
def test_sampler_10_steps_vs_the_sampler_oracle():
    import mdm
    from oracle.sampler_ref import SamplerRef
    from oracle.scheduler_ref import SchedulerRef
    n, hw, T = 4, 16, 10
    a = base_args(data_size=hw, ddpm_num_steps=T, sampling_mask_dependency="independent", momentum_adaptive="base_sampling",
                  sample_num=n, sample_latent_shape="uniform", sample_history=False)
    params = random_params_noconv(NET3, 1234)
    model = mdm.UNet(NET3_POOL, N=n, H=hw, W=hw, dtype=mdm.F32, params=params).eval()
    s = mdm.Scheduler(a)
    s.update_ddpm_num_steps(T)
    ts = s.get_timesteps_epoch(0, 1)
    seed_all(4310)
    x0, _ = mdm.Sampler(None, a, s, [None] * 3).sample(model, ts)
    torch.cuda.synchronize()
    rs = SchedulerRef(a)
    rs.update_ddpm_num_steps(T)
    seed_all(4310)
    with torch.no_grad():
        want, _ = SamplerRef(None, a, rs, [None] * 3).sample(UNetNoConvRef(NET3_POOL, params), ts)
    rel = _rel(x0, want)
    print("sampler rel-L2", rel)
    assert bool(torch.isfinite(x0).all()) and rel < 1e-3, rel                # north_star: within 1e-3 rel-L2


# ----------------------------------------------------------------------------- 6: with drop_rate
def test_with_drop_rate_a_step_runs_and_eval_ignores_it(golden):
    import mdm
    g = golden("unet_resample")
    params = random_params_noconv(NET3, int(g["seed"]))
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    drop = mdm.UNet(dict(NET3_POOL, drop_rate=0.3), N=2, H=16, W=16, dtype=mdm.F32, params=params, drop_seed=4)
    plain = mdm.UNet(NET3_POOL, N=2, H=16, W=16, dtype=mdm.F32, params=params)
    assert len(drop.dropout_sites()) == 11
    y_train = drop(x, t).sample.clone()
    drop.eval(); plain.eval()
    y_eval, y_plain = drop(x, t).sample.clone(), plain(x, t).sample.clone()
    assert _same_bits(y_eval, y_plain) and not torch.equal(y_train, y_plain)
    drop.train()
    n = 4
    a = base_args(data_size=16, ddpm_num_steps=20, batch_size=n, rng_mode="device", seed=5)
    m = mdm.UNet(dict(NET3_POOL, drop_rate=0.3), N=n, H=16, W=16, dtype=mdm.BF16, params=params, drop_seed=4)
    opt = mdm.AdamW(m, lr=1e-3)
    tr = mdm.Trainer(a, None, None, [None] * 3, m, None, opt, mdm.get_lr_scheduler("constant", opt, 0, 1), mdm.Accelerator())
    tr.Scheduler.update_ddpm_num_steps(20)
    tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    before = m.store.P.clone()
    x0 = torch.rand(n, 3, 16, 16, generator=torch.Generator().manual_seed(3)) * 2 - 1
    loss = float(tr._run_batch(0, (x0, None, None), 0, 1, 0, None, None))
    torch.cuda.synchronize()
    assert np.isfinite(loss) and loss > 0 and not torch.equal(m.store.P, before) and bool(torch.isfinite(m.store.P).all())
