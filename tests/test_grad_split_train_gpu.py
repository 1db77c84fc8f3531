"""Split-product gradients of fp32 training, model level: UNet(dtype=F32, f32_products="split", grad_products="split") through the
mean-shift trainer against the reference's own fp32 step (tests/golden/train_grads.npz) and trajectory (train_traj.npz), its
bit-reproducibility, and the sampler after an update (the hi / lo filter shadows follow the weights)."""
import numpy as np
import pytest
import torch

from _notes import note

pytestmark = pytest.mark.gpu

from golden.make_golden import TINY, base_args, seed_all  # noqa: E402

SPLIT = dict(dtype=0, f32_products="split", grad_products="split")


def T(a):
    return torch.from_numpy(np.asarray(a))


def _trainer(a, **kw):
    import mdm
    from oracle.unet_ref import random_params
    model = mdm.UNet(TINY, N=4, H=16, W=16, params=random_params(TINY), **SPLIT, **kw)
    opt = mdm.AdamW(model, lr=1e-3)
    tr = mdm.Trainer(a, None, None, [None] * 3, model, None, opt, mdm.get_lr_scheduler("constant", opt, 0, 10), mdm.Accelerator())
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(a.ddpm_num_steps)
    tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    return tr, model


def test_gradient_tensors_vs_reference(golden):
    """All 128 gradient tensors of one reference `_run_batch` (captured before clipping) and the clip norm -- the setup of
    test_path_gpu.py::test_train_step_gradient_tensors_vs_reference -- and the route of every convolution's gradients."""
    from mdm import ops
    g = golden("train_grads")
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", loss_weight_use=True,
                  batch_size=4)
    tr, model = _trainer(a)
    seed_all(501)
    loss = tr._run_batch(0, (T(g["tg_x0"]), None, None), 0, 1, 0, None, None)
    assert np.array_equal(tr.step.x_in.cpu().numpy(), g["tg_xin"])
    want_loss = float(g["tg_loss"])
    grads = model.store.grad_dict()
    want = {k.split("::")[1]: g[k] for k in g.files if k.startswith("tg_g::")}
    assert set(want) == set(grads) and len(want) == 128
    a_ = np.concatenate([grads[k].numpy().reshape(-1) for k in want])
    b_ = np.concatenate([want[k].reshape(-1) for k in want])
    rel = np.linalg.norm(a_ - b_) / np.linalg.norm(b_)
    rms = float(np.sqrt((b_ ** 2).mean()))
    worst_t = max(float(np.abs(grads[k].numpy() - want[k]).max() / (np.abs(want[k]).max() + rms)) for k in want)
    norm_rel = abs(tr.optimizer.grad_norm() - float(g["tg_norm"])) / float(g["tg_norm"])
    note("grad_split_train_grads", dict(rel_l2=float(rel), loss=loss, ref_loss=want_loss, clip_norm_rel=norm_rel, worst_tensor=worst_t))
    # bars at ~4x the MI355X's figures (loss 2.8e-7 relative, gradients 1.54e-5 rel-L2, clip norm 6.0e-7): the exact fp32 path's
    # bars of the same fixture are 2e-5 / 2e-4 / 2e-4, bf16's gradient bar is 6e-2
    assert abs(loss - want_loss) < 1.2e-6 * max(1.0, want_loss), (loss, want_loss)
    assert rel < 6e-5, rel
    for k in want:
        assert np.allclose(grads[k].numpy(), want[k], rtol=3e-3, atol=3e-2 * rms), k
    assert norm_rel < 2.4e-6, norm_rel
    # every eligible convolution ran both gradients with split products, the rest say why not
    tab = model.grad_products_table()
    convs = [s for s in model.specs if type(s).__name__ == "_Conv"]
    assert set(tab) == {c.name for c in convs}
    n_split = 0
    for c in convs:
        for which in ("dgrad", "wgrad"):
            if which not in tab[c.name]:
                assert which == "dgrad" and not c.src0.needs_grad, (c.name, tab[c.name])
                continue
            why = ops.split_grad_reason(c.g, which)
            r = tab[c.name][which]
            if why is None:
                assert "split" in r and not r.startswith("exact"), (c.name, which, r)
                n_split += 1
            else:
                assert r == "exact:" + why, (c.name, which, r)
    assert n_split >= 20, tab


@pytest.mark.parametrize("gas", [1, 2])
def test_trainer_trajectory_vs_reference(golden, tmp_path, gas):
    """`Trainer.train()` in replay mode, 2 epochs x 3 batches (tests/golden/train_traj.npz), in split-gradient mode: per-batch
    losses and final weights against the reference's fp32 run."""
    import mdm
    from oracle.unet_ref import random_params
    from test_device_path_gpu import _dirs
    from test_oracle_golden import live_gradient_keys
    from torch.utils.data import DataLoader, TensorDataset
    g = golden("train_traj")
    tag = f"traj_g{gas}"
    data = torch.from_numpy(g["traj_data"])
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", loss_weight_use=True,
                  batch_size=4, sample_num=2, sample_latent_shape="zero", use_ema=False, scheduler_num_scale_timesteps=2,
                  save_images_epochs=10, gradient_accumulation_steps=gas)
    seed_all(0)
    model = mdm.UNet(TINY, N=4, H=16, W=16, params=random_params(TINY), **SPLIT)
    opt = mdm.AdamW(model, lr=1e-3)
    lr_s = mdm.optim.LambdaLR(opt, lambda k: 1.0 / (1.0 + 0.25 * k))
    loader = DataLoader(TensorDataset(data, torch.zeros(12)), batch_size=4, shuffle=False)
    acc = mdm.Accelerator(gradient_accumulation_steps=gas)
    model, opt, loader, lr_s = acc.prepare(model, opt, loader, lr_s)
    tr = mdm.Trainer(a, loader, None, [None] * 3, model, None, opt, lr_s, acc)
    losses = []
    ob = tr._run_batch
    tr._run_batch = lambda *aa, **kk: (lambda r: (losses.append(r), r)[-1])(ob(*aa, **kk))
    seed_all(900 + gas)
    tr.train(0, 2, 0, 0, _dirs(tmp_path), None)
    torch.cuda.synchronize()
    ref_losses = np.asarray(g[tag + "_losses"], dtype=np.float64)
    loss_rel = float(np.max(np.abs(np.asarray(losses) - ref_losses) / np.abs(ref_losses)))
    sd = model.state_dict()
    worst, worst_frac = 0.0, 0.0
    for k in live_gradient_keys(golden("train_step")):
        d = np.abs(sd[k].numpy() - g[tag + "_w::" + k])
        worst = max(worst, float(d.max()))
        worst_frac = max(worst_frac, float((d > 3e-4).mean()))
    note("grad_split_trajectory", dict(gas=gas, loss_rel=loss_rel, worst_weight_diff=worst, worst_frac_over_3em4=worst_frac))
    # ~4x the MI355X's figures (losses 1.1e-5 relative, largest weight difference 1.2e-3, elements beyond 3e-4: 8.1e-5); the exact
    # fp32 trajectory test allows 1e-4 / 1.2e-2 / 5e-3 (a near-zero gradient may flip sign: ~2 lr per step)
    assert loss_rel < 4.5e-5, (losses, list(ref_losses))
    assert worst_frac < 3.3e-4 and worst < 4.8e-3, (worst_frac, worst)


def _device_step_model(seed):
    import mdm
    from oracle.unet_ref import random_params
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation",
                  rng_mode="device", seed=seed, batch_size=4, use_ema=True)
    model = mdm.UNet(TINY, N=4, H=16, W=16, params=random_params(TINY), **SPLIT)
    opt = mdm.AdamW(model, lr=1e-3)
    ema = mdm.EMA(model)
    tr = mdm.Trainer(a, None, None, [None] * 3, model, ema, opt, mdm.get_lr_scheduler("constant", opt, 0, 10), mdm.Accelerator())
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(10)
    tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    return tr, model, ema


def test_split_gradient_step_is_bit_reproducible():
    """Two freshly built models, the same device-RNG train steps (one hipGraph each): loss, G, P and the EMA are the same bits."""
    outs = []
    for _ in range(2):
        tr, model, ema = _device_step_model(3)
        g = torch.Generator().manual_seed(78)
        x0 = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1
        ls = [tr._run_batch(0, (x0, None, None), 0, 1, 0, None, None) for _ in range(3)]
        outs.append((ls, model.store.G.clone(), model.store.P.clone(), ema.shadow.clone()))
    assert outs[0][0] == outs[1][0], (outs[0][0], outs[1][0])
    assert all(np.isfinite(outs[0][0]))
    for u, v in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(u, v), float((u - v).abs().max())


def test_sampler_after_an_update_matches_a_fresh_model():
    """After one split-gradient optimizer step (inside the step's hipGraph), sampling_plan("f32_split") of the model samples
    exactly what a fresh split model loaded from its state_dict() samples: the filter shadows were refreshed by the update."""
    import mdm
    tr, model, _ = _device_step_model(5)
    g = torch.Generator().manual_seed(79)
    x0 = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1
    p0 = model.store.P.clone()
    tr._run_batch(0, (x0, None, None), 0, 1, 0, None, None)
    torch.cuda.synchronize()
    assert not torch.equal(p0, model.store.P)
    fresh = mdm.UNet(TINY, N=4, H=16, W=16, dtype=0, f32_products="split", params=model.state_dict())
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", sample_num=2,
                  sample_latent_shape="normal", noise_mean=0.1)
    outs = []
    for m in (model, fresh):
        net = m.sampling_plan(2, "f32_split")
        assert net.store is m.store
        s = mdm.Scheduler(a)
        s.update_ddpm_num_steps(10)
        ts = s.get_timesteps_epoch(0, 1)
        seed_all(610)
        xs, _ = mdm.Sampler(None, a, s, [None] * 3).sample(net, ts)
        outs.append(xs.clone())
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
