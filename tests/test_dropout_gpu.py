"""Residual-block dropout (unet6 `drop_rate`) on the GPU: the mask against its numpy restatement, the dropout GroupNorm kernels
against torch, the whole net against the CPU oracle with the same masks, modes / determinism / graphs, TrainStep + checkpoint, sampler."""
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _dropout_ref import ctl_words, keep_mask, site_mask_nchw, unet_forward_dropout  # noqa: E402
from golden.make_golden import TINY, base_args  # noqa: E402

DT = {"f32": 0, "bf16": 1}


# ---- helpers of tests/test_kernels_gpu.py (test_groupnorm_fwd_bwd)
def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _q(x, dt):
    return x.bfloat16().float() if dt == "bf16" else x


def _up(x, dt):
    return x.to(_dev(), torch.bfloat16 if dt == "bf16" else torch.float32).contiguous()


def _tol(dt, scale=1.0):
    return (2e-2 if dt == "bf16" else 2e-4) * scale


def _relerr(a, b):
    return float((a.float().cpu() - b).norm() / (b.norm() + 1e-12))


def _rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


def _rng(key, offset):
    return torch.tensor([key, offset], dtype=torch.int64, device=_dev())


def _ctl(rate):
    thr, scale = ctl_words(rate)
    return torch.tensor([thr, struct.unpack("<i", struct.pack("<f", scale))[0]], dtype=torch.int32, device=_dev())


# ----------------------------------------------------------------------------- 1: mask parity
@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("offset", [1, (1 << 33) + 7])
@pytest.mark.parametrize("base", [0, 8 * 12345])
def test_mask_matches_the_numpy_restatement(base, offset, rate):
    from mdm import ops
    n, key = 4096 + 8, 0x1234ABCD | (3 << 32)
    keep = torch.full((n + 16,), 7, dtype=torch.uint8, device=_dev())
    ops.dropout_mask(_rng(key, offset), base, _ctl(rate), n, keep[8:])
    torch.cuda.synchronize()
    got = keep.cpu().numpy()
    assert (got[:8] == 7).all() and (got[8 + n:] == 7).all()                 # nothing outside [0, n)
    want = keep_mask(key, offset, base, n, rate)
    assert np.array_equal(got[8:8 + n].astype(bool), want) and 0 < want.sum() < n
    ops.dropout_mask(_rng(key, offset), base, _ctl(0.0), n, keep[8:])      # an eval ctl keeps everything
    torch.cuda.synchronize()
    assert bool((keep[8:8 + n] == 1).all())


# ----------------------------------------------------------------------------- 2: GroupNorm parity
GN_DROPOUT_ROUTES = {      # (C, HW): {storage type: (forward, backward)}
    (128, 64): {"bf16": ("fwd_reg<1,256>", "bwd_reg<1,256>"), "f32": ("fwd_reg<1,256>", "bwd+reduce")},
    (256, 16): {"bf16": ("fwd_reg<1,256>", "bwd_reg<1,256>"), "f32": ("fwd_reg<1,256>", "bwd+reduce")},
    (128, 1024): {"bf16": ("fwd_reg<4,512>", "bwd_reg<4,512>"), "f32": ("fwd_reg<8,512>", "bwd+reduce")},
    (32, 4096): {"bf16": ("fwd", "bwd"), "f32": ("fwd", "bwd+reduce")},
}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,HW", [(128, 64), (256, 16), (128, 1024), (32, 4096)])
def test_groupnorm_dropout_fwd_bwd(dt, C, HW):
    """The register kernels at one vector per lane and at 8 - 16, and the generic kernels; every fp32 backward is the generic
    kernel.  A dropout site runs on the kernel its plain GroupNorm runs on."""
    from mdm import _lib, ops
    N, G, rate, silu = 3, 32, 0.3, True
    key, offset, base = 77 | (1 << 32), 5, 8 * 1000
    fwd, bwd = GN_DROPOUT_ROUTES[C, HW][dt]
    for fields in (dict(), dict(rng=16, ctl=16, drop_base=base)):
        shape = dict(dtype=DT[dt], N=N, P=HW, G=G, C0=C, C1=0, **fields)
        assert (_lib.gn_route_of(0, **shape), _lib.gn_route_of(1, **shape)) == (fwd, bwd)
    g = torch.Generator().manual_seed(C + HW)
    x = _q(torch.randn(N, C, HW, generator=g) * 1.5 + 0.3, dt).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g)).requires_grad_(True)
    _, scale = ctl_words(rate)
    keep = keep_mask(key, offset, base, N * HW * C, rate).reshape(N, HW, C)
    mask = torch.from_numpy(keep).permute(0, 2, 1).float()                  # [N, C, HW]
    y = F.silu(F.group_norm(x, G, gamma, beta, eps=1e-6)) * mask * float(np.float32(scale))
    gy = _q(torch.randn(y.shape, generator=g), dt)
    y.backward(gy)
    dev = _dev()
    xh = _up(x.detach().permute(0, 2, 1), dt)                               # [N, HW, C]
    out = torch.empty(N, HW, C, device=dev, dtype=xh.dtype)
    stats = torch.empty(N, G, 2, device=dev)
    ws = torch.empty(N * (64 * G + 4 * C), device=dev)
    gd, bd = gamma.detach().to(dev), beta.detach().to(dev)
    rng, ctl, ev = _rng(key, offset), _ctl(rate), _ctl(0.0)
    ops.groupnorm_fwd_dropout(DT[dt], xh, C, N, HW, gd, bd, silu, out, stats, ws, rng, base, ctl)
    torch.cuda.synchronize()
    assert _relerr(out, y.detach().permute(0, 2, 1)) < _tol(dt, 0.5)
    assert float(out.float().cpu()[~torch.from_numpy(keep)].abs().max()) == 0.0          # dropped elements: exact zeros
    gyh = _up(gy.permute(0, 2, 1), dt)
    d0 = torch.empty_like(xh)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ops.groupnorm_bwd_dropout(DT[dt], xh, C, N, HW, gd, bd, silu, gyh, stats, d0, 0, dg, db, ws, rng, base, ctl)
    torch.cuda.synchronize()
    gx = x.grad.permute(0, 2, 1)
    assert _relerr(d0, gx) < _tol(dt)
    assert _relerr(dg, gamma.grad) < _tol(dt, 0.25)
    assert _relerr(db, beta.grad) < _tol(dt, 0.25)
    if (C, HW) == (128, 64):        # fused column sums of dx, as tests/test_kernels_gpu.py checks them
        per = torch.zeros(N, C + 8, device=dev)
        tot = torch.full((C,), 2.0, device=dev)
        dg2, db2 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        ops.groupnorm_bwd_dropout(DT[dt], xh, C, N, HW, gd, bd, silu, gyh, stats, d0, 0, dg2, db2, ws, rng, base, ctl,
                                  sum_img=per[:, 8:], sum_ld=C + 8, sum_all=tot)
        torch.cuda.synchronize()
        sc = float(gx.abs().sum(1).mean())
        assert float((per[:, 8:].cpu() - gx.sum(1)).abs().max()) < _tol(dt, 0.5) * sc and float(per[:, :8].abs().sum()) == 0
        assert float(((tot - 2.0).cpu() - gx.sum((0, 1))).abs().max()) < _tol(dt, 0.5) * sc * N
    # an eval ctl: the bits of the plain entry points (fp32 sums have a fixed order; bf16 dgamma / dbeta go through float atomics
    # across the images, so there only y and dx are compared bit for bit)
    o1, o2, s1, s2 = torch.empty_like(out), torch.empty_like(out), torch.empty_like(stats), torch.empty_like(stats)
    ops.groupnorm_fwd_dropout(DT[dt], xh, C, N, HW, gd, bd, silu, o1, s1, ws, rng, base, ev)
    ops.groupnorm_fwd(DT[dt], xh, C, None, 0, N, HW, gd, bd, silu, o2, s2, ws)
    e1, e2 = torch.empty_like(xh), torch.empty_like(xh)
    g1, b1, g2, b2 = (torch.zeros(C, device=dev) for _ in range(4))
    ops.groupnorm_bwd_dropout(DT[dt], xh, C, N, HW, gd, bd, silu, gyh, s1, e1, 0, g1, b1, ws, rng, base, ev)
    ops.groupnorm_bwd(DT[dt], xh, C, None, 0, N, HW, gd, bd, silu, gyh, s2, e2, 0, None, 0, g2, b2, ws)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(s1, s2) and torch.equal(e1, e2)
    if dt == "f32":
        assert torch.equal(g1, g2) and torch.equal(b1, b2)


# ----------------------------------------------------------------------------- 3: the whole net
def _masks_of(net, rng_words, rate):
    key, offset = (int(v) for v in rng_words)
    out = {}
    for name, base, n in net.dropout_sites():
        spec = next(s for s in net.specs if s.name == name)
        o = spec.out
        assert n == o.N * o.H * o.W * o.C
        out[name[:-len(".norm2")]] = site_mask_nchw(key & 0xFFFFFFFFFFFFFFFF, offset, base, o.N, o.H, o.W, o.C, rate)
    return out


@pytest.mark.parametrize("dt,tol_y,tol_g", [(0, 2e-4, 2e-3), (1, 3e-2, 8e-2)])
def test_unet_tiny_dropout_forward_backward(dt, tol_y, tol_g):
    """One eager forward + backward of the tiny net with drop_rate = 0.3 against the CPU oracle under the SAME masks (rebuilt from the
    net's rng words and site bases); the tolerances of test_unet_gpu.test_unet_tiny_forward_backward for this net without dropout."""
    from mdm import ops
    from mdm import unet as U
    from oracle.unet_ref import random_params
    rate, N, HW = 0.3, 4, 16
    cfg = dict(TINY, drop_rate=rate)
    params = random_params(TINY)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(N, 3, HW, HW, generator=g) * 2 - 1
    t = torch.tensor([3.0, 41.0, 250.0, 999.0])
    gy = torch.randn(N, 3, HW, HW, generator=g)
    net = U.UNet(cfg, N=N, H=HW, W=HW, dtype=dt, params=params, use_graph=False, drop_seed=9)
    assert len(net.dropout_sites()) == 8
    y = net(x, t).sample
    net.zero_grad()
    ops.nchw_to_nhwc(dt, gy.to(net.device), net.y_out.grad, N, 3, HW, HW, net.cout_p)
    net.run_backward()
    torch.cuda.synchronize()
    words = net.drop_rng.dev.cpu().tolist()
    assert words == [9, 1]                                                  # key = (drop_seed, rank 0); ONE advance per forward
    grads = net.store.grad_dict()
    masks = _masks_of(net, words, rate)
    frac = sum(float(m.sum()) for m in masks.values()) / sum(m.numel() for m in masks.values())
    assert abs(frac - 0.7) < 0.01
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    yo = unet_forward_dropout(p, TINY, x, t, masks, float(np.float32(ctl_words(rate)[1])))
    (yo * gy).sum().backward()
    want = {k: v.grad for k, v in p.items()}
    print("rel_l2_y", _rel(y, yo.detach()))
    assert _rel(y, yo.detach()) < tol_y
    rms = float(torch.cat([w.reshape(-1) for w in want.values()]).pow(2).mean().sqrt())

    def err(a, b):
        a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
        return float((a - b).norm() / (b.norm() + 1e-2 * rms * b.numel() ** 0.5))
    med = sorted(float(w.norm()) for w in want.values())[len(want) // 2]
    keys = [k for k in want if dt == 0 or float(want[k].norm()) > 1e-2 * med]
    assert set(want) == set(grads) and len(keys) > 0.8 * len(want)
    worst = max((err(grads[k], want[k]), k) for k in keys)
    allg = torch.cat([grads[k].reshape(-1) for k in want]), torch.cat([want[k].reshape(-1) for k in want])
    print("worst", worst, "all", _rel(*allg))
    assert worst[0] < tol_g, worst
    assert _rel(*allg) < tol_g / 2


# ----------------------------------------------------------------------------- 4: modes and determinism
def test_modes_determinism_and_graph_replay():
    from mdm import unet as U
    from oracle.unet_ref import random_params, unet_forward
    N, HW = 4, 16
    cfg = dict(TINY, drop_rate=0.3)
    params = random_params(TINY)
    g = torch.Generator().manual_seed(22)
    x = torch.rand(N, 3, HW, HW, generator=g) * 2 - 1
    t = torch.tensor([3.0, 41.0, 250.0, 999.0])
    eager = U.UNet(cfg, N=N, H=HW, W=HW, dtype=0, params=params, use_graph=False)
    graph = U.UNet(cfg, N=N, H=HW, W=HW, dtype=0, params=params, use_graph=True)
    start = eager.drop_rng.dev.clone()
    y1 = eager(x, t).sample.clone()
    y2 = eager(x, t).sample.clone()
    assert not torch.equal(y1, y2)                                          # the offset advanced
    eager.drop_rng.dev.copy_(start)
    assert torch.equal(eager(x, t).sample, y1) and torch.equal(eager(x, t).sample, y2)       # same state, same bits
    g1 = graph(x, t).sample.clone()                                         # captured here: every replay bumps the offset itself
    g2 = graph(x, t).sample.clone()
    assert torch.equal(g1, y1) and torch.equal(g2, y2)
    graph.eval()
    e1, e2 = graph(x, t).sample.clone(), graph(x, t).sample.clone()
    assert torch.equal(e1, e2)
    with torch.no_grad():
        ref = unet_forward(params, TINY, x, t)
    assert _rel(e1, ref) < 2e-4
    graph.train()                                                           # nothing re-recorded: the same graph drops again
    graph.drop_rng.dev.copy_(start)
    assert torch.equal(graph(x, t).sample, y1)
    # a batch twin shares the state and the mode
    twin = graph.with_batch(2)
    assert twin.drop_rng is graph.drop_rng and twin.drop_ctl is graph.drop_ctl and len(twin.dropout_sites()) == 8
    assert graph.with_uniform_t().dropout_sites() == [] and graph.with_uniform_t().drop_rng is None


# ----------------------------------------------------------------------------- 5: TrainStep and checkpoint
def _trainer(params, x0, rate=0.2):
    import mdm
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=20, batch_size=4, rng_mode="device", seed=5)
    m = mdm.UNet(dict(TINY, drop_rate=rate), N=4, H=16, W=16, dtype=mdm.F32, params=params, drop_seed=3)
    o = mdm.AdamW(m, lr=1e-3)
    tr = mdm.Trainer(a, None, None, [None] * 3, m, None, o, mdm.get_lr_scheduler("constant", o, 0, 1), mdm.Accelerator())
    tr.Scheduler.update_ddpm_num_steps(20)
    tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    return tr, m, o


def test_train_steps_resume_bit_exactly_from_a_checkpoint(tmp_path):
    from mdm import checkpoint
    from oracle.unet_ref import random_params
    params = random_params(TINY)
    x0 = torch.rand(4, 3, 16, 16, generator=torch.Generator().manual_seed(3)) * 2 - 1
    step = lambda tr: float(tr._run_batch(0, (x0, None, None), 0, 1, 0, None, None))
    tr, m, _ = _trainer(params, x0)
    losses = [step(tr) for _ in range(3)]
    torch.cuda.synchronize()
    w3 = m.store.P.clone()
    key, offset3 = m.drop_rng.dev.cpu().tolist()
    assert key == 3 and offset3 >= 3 and len(set(losses)) == 3             # key = (drop_seed, rank 0); every step advanced the offset
    tr, m, o = _trainer(params, x0)
    first = [step(tr) for _ in range(2)]
    assert first == losses[:2]
    checkpoint.save_state(str(tmp_path), m, optimizer=o, scheduler=tr.Scheduler)
    st = torch.load(str(tmp_path / "random_states_0.pkl"), map_location="cpu", weights_only=False)
    assert st["mdm_dropout_philox"] == m.drop_rng.dev.cpu().tolist() and 2 <= st["mdm_dropout_philox"][1] < offset3
    tr2, m2, o2 = _trainer(random_params(TINY, 99), x0)                     # fresh model / optimizer / scheduler
    checkpoint.load_state(str(tmp_path), m2, optimizer=o2, scheduler=tr2.Scheduler)
    assert step(tr2) == losses[2]
    torch.cuda.synchronize()
    assert torch.equal(m2.store.P, w3)
    # drop_rate = 0: no such key
    import mdm
    plain = mdm.UNet(TINY, N=4, H=16, W=16, dtype=mdm.F32, params=params)
    checkpoint.save_state(str(tmp_path / "plain"), plain)
    assert "mdm_dropout_philox" not in torch.load(str(tmp_path / "plain" / "random_states_0.pkl"), map_location="cpu", weights_only=False)


# ----------------------------------------------------------------------------- 6: the sampler
def test_sampler_in_eval_mode_ignores_dropout():
    import mdm
    from oracle.unet_ref import random_params
    params = random_params(TINY)
    outs = []
    for cfg in (dict(TINY, drop_rate=0.3), TINY):
        a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, sample_num=4, sample_latent_shape="normal",
                      rng_mode="device", seed=8, sample_history=False)
        S = mdm.Scheduler(a)
        S.update_ddpm_num_steps(10)
        ts = S.get_timesteps_epoch(0, 1)
        model = mdm.UNet(cfg, N=4, H=16, W=16, dtype=mdm.F32, params=params).eval()
        torch.manual_seed(31)
        x0, _ = mdm.Sampler(None, a, S, [None] * 3).sample(model, ts)
        torch.cuda.synchronize()
        outs.append(x0.clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
