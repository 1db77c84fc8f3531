"""The visuals surface on the GPU (mdm/visuals.py, mdm.Sampler's grid methods, the trainers' `get_current_visuals` and `args.visuals`)
against tests/_vis_ref.py on the CPU: TINY net, 16 x 16, N = 4, as smoke() runs it.  Grids are compared bit for bit (a NaN by position),
PNGs and uint8 grids byte for byte."""
import os
import types

import numpy as np
import pytest
import torch

import _vis_ref as VR
from golden.make_golden import TINY, base_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS_NAMES = ["input", "degraded_img", "degrade_binary_masks", "degradation_mask", "mean_pixel", "shift", "shifted_degrade_img",
            "reconstructed_img", "inverse_shift_reconstructed_img", "mask"]                  # trainer_masked_mean_shift.py:58
BASE_NAMES = ["input", "degraded_img", "degradation_mask", "mask", "mean_pixel", "degrade_binary_masks", "reconstructed_img"]   # trainer_masked.py:58
SAMPLE_NAMES = ["ema_sample_result_normalize_global", "ema_sample_result_normalize_local"]   # :59


def _png(path):
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path)).copy())


def _sampler():
    import mdm
    a = base_args(data_size=16)
    return mdm.Sampler(None, a, mdm.Scheduler(a, device=DEV), [None] * 3)


def _batch(n, c=3, seed=0):
    return torch.randn(n, c, 16, 16, generator=torch.Generator().manual_seed(seed)) * 1.7 + 0.2


# ------------------------------------------------------------------ Sampler
@pytest.mark.parametrize("n,c", [(4, 3), (5, 1), (1, 3)])
def test_save_image_grid_is_upstreams(tmp_path, n, c):
    """sampler.py:369-387: nrow = ceil(sqrt(batch)), both normalisations (and none for any other word), the PNG = the uint8 grid"""
    S, x = _sampler(), _batch(n, c, seed=n)
    nrow = int(np.ceil(np.sqrt(n)))
    for norm, ref_norm in (("global", "global"), ("image", "image"), ("none", None)):
        want_f, want_u = VR.grid_ref(x, nrow, ref_norm)
        g = S._save_image_grid(x.to(DEV), normalization=norm)
        assert g.is_cuda and g.dtype == torch.float32 and VR.same_grid(g, want_f), norm
        g2 = S._save_image_grid(x, norm, str(tmp_path), f"{norm}.png")                       # a host batch is moved to the device
        assert VR.same_grid(g2, want_f) and torch.equal(_png(tmp_path / f"{norm}.png"), want_u), norm
    assert VR.same_grid(S._save_image_grid(x.to(DEV)), VR.grid_ref(x, nrow, "global")[0])    # 'global' is the default
    assert S._save_image_grid(torch.zeros(0, 3, 16, 16, device=DEV)) is None
    assert S._save_image_grid(torch.zeros(0, 3, 16, 16), "image", str(tmp_path), "empty.png") is None
    assert not os.path.exists(tmp_path / "empty.png")
    const = torch.full((2, 3, 16, 16), 0.25)
    assert bool(torch.isnan(S._save_image_grid(const.to(DEV), "global")[:, 2:18, 2:18]).all())      # 0 / 0, as upstream
    assert not bool(S._save_image_grid(const.to(DEV), "image").any())


def test_save_multi_index_image_grid_on_a_device_history():
    """sampler.py:390-417 on a 5-step history kept on the device: one grid per sample over its frames, read in place from the
    time-major tensor; 'skip_first' drops frame 0; upstream's [N, T', C, H, W] gives the same grids"""
    S = _sampler()
    T1, N = 6, 4
    hist = torch.randn(T1, N, 3, 16, 16, generator=torch.Generator().manual_seed(3))
    hd = hist.to(DEV)
    before = hd.clone()
    for option, frames in (("skip_first", hist[1:]), (None, hist)):
        nrow = int(np.ceil(np.sqrt(T1)))
        for norm in ("global", "image", None):
            want = [VR.grid_ref(frames[:, i], nrow, norm)[0] for i in range(N)]
            got = S._save_multi_index_image_grid(hd, normalization=norm, option=option, time_major=True)
            up = S._save_multi_index_image_grid(hd.transpose(0, 1).contiguous(), normalization=norm, option=option)
            assert len(got) == len(up) == N
            for g, u, w in zip(got, up, want):
                assert g.is_cuda and VR.same_grid(g, w) and VR.same_grid(u, w), (option, norm)
    got = S._save_multi_index_image_grid(hd, nrow=2, option="skip_first", time_major=True)
    assert VR.same_grid(got[3], VR.grid_ref(hist[1:, 3], 2, "global")[0])
    assert torch.equal(hd, before)
    with pytest.raises(UnboundLocalError):
        S._save_multi_index_image_grid(hd, normalization="batch", time_major=True)


def test_save_image_pair_grid(tmp_path):
    """sampler.py:474-484: interleaved, normalize01 per image, nrow = 2 ceil(sqrt(batch)); upstream's second, batch-wide min-max
    pass is the identity here (no image is constant), which the reference below applies to show it"""
    S = _sampler()
    a, b = _batch(5, seed=1), _batch(5, seed=2)
    data = torch.zeros(10, 3, 16, 16)
    for i in range(5):
        data[2 * i], data[2 * i + 1] = a[i], b[i]
    norm = VR.normalize01(data)
    lo, hi = norm.min(), norm.max()
    again = (norm.clamp(lo, hi) - lo) / max(float(hi - lo), 1e-5)                             # make_grid(normalize=True)'s norm_ip
    assert float(lo) == 0.0 and float(hi) == 1.0 and torch.equal(again, norm)
    want_f = VR.make_grid_ref(again, 6)
    g = S._save_image_pair_grid(a.to(DEV), b, str(tmp_path), "pair.png")
    assert VR.same_grid(g, want_f) and torch.equal(_png(tmp_path / "pair.png"), VR.to_u8_ref(want_f))


# ------------------------------------------------------------------ trainers
def _make_trainer(name, a, dt, loader=None, n=4, ema=False):
    import mdm
    from oracle.unet_ref import random_params
    model = mdm.UNet(TINY, N=n, H=16, W=16, dtype=dt, params=random_params(TINY), use_graph=getattr(a, "use_graph", True))
    opt = mdm.AdamW(model, lr=1e-3)
    lr_s = mdm.get_lr_scheduler("constant", opt, 0, 10)
    e = mdm.EMA(model) if ema else None
    if name == "base":
        tr = mdm.BaseTrainer(a, loader, None, model, e, opt, lr_s, mdm.Accelerator())
    else:
        tr = mdm.Trainer(a, loader, None, [None] * 3, model, e, opt, lr_s, mdm.Accelerator())
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(a.ddpm_num_steps)
    tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    return tr, model


def _loader(n_batches, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 3, 16, 16, generator=g) * 2 - 1, None, None) for _ in range(n_batches)]


@pytest.mark.parametrize("name,dt,mode", [("ms", 0, "replay"), ("ms", 1, "device"), ("base", 0, "replay"), ("base", 1, "device")])
def test_visual_tensors_and_current_visuals_after_one_batch(name, dt, mode):
    """the five tensors the step does not keep equal their definitions recomputed on the CPU from the step's buffers (single fp32
    additions and products: bit for bit); `get_current_visuals` has upstream's keys in upstream's order, every value the reference
    grid of the trainer's own attribute; the whole call is one mdm_sampler_x0, then per grid one range and one grid launch"""
    from mdm import _lib
    kw = dict(rng_mode="device", seed=3) if mode == "device" else {}
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", batch_size=4, **kw)
    tr, model = _make_trainer(name, a, dt)
    names = MS_NAMES if name == "ms" else BASE_NAMES
    assert tr.train_visual_names == names and tr.sample_visual_names == SAMPLE_NAMES and tr.visuals is False
    with pytest.raises(RuntimeError):
        tr.get_current_visuals(0)                                                            # no step has run
    torch.manual_seed(7)
    tr._run_batch(0, _loader(1)[0], 0, 1, 0, None, None)
    with pytest.raises(AttributeError):
        tr.get_current_visuals(0)                                                            # as upstream: no EMA sample drawn yet
    tr.ema_sample_result_normalize_global = torch.full((3, 4, 4), 0.5, device=DEV)
    tr.ema_sample_result_normalize_local = torch.full((3, 4, 4), 0.25, device=DEV)
    vis = tr.get_current_visuals(0)
    torch.cuda.synchronize()

    s = tr.step
    x_in, sh, keep, mp = s.x_in.cpu(), s.s.cpu(), s.mask.cpu(), s.mean_pixel.cpu()[:, :, None, None]
    y = model.y_out.data.reshape(4, 16, 16, model.cout_p)[..., :3].permute(0, 3, 1, 2).float().cpu().contiguous()
    same = lambda t, w: t.is_cuda and t.dtype == torch.float32 and VR.same_grid(t, w)
    assert same(tr.mask, y)
    assert same(tr.reconstructed_img, x_in + y)                                              # ms:142
    assert same(tr.inverse_shift_reconstructed_img, (x_in + y) - sh)                         # ms:145
    assert same(tr.degradation_mask, (1 - keep) * mp + keep)                                 # scheduler.py:320
    assert same(tr.mean_pixel, torch.ones_like(keep) * mp)                                   # scheduler.py:321
    assert same(tr.shift, sh) and (name == "ms" or not bool(sh.any()))                       # no shift: the zero tensor
    assert tr.input is s.x0 and tr.degraded_img is s.x_t and tr.degrade_binary_masks is s.mask
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0

    assert isinstance(vis, dict) and type(vis).__name__ == "OrderedDict"
    assert list(vis) == [n + sfx for n in names for sfx in ("_normalize_global", "_normalize_local")] + SAMPLE_NAMES
    for n in names:
        x = getattr(tr, n).cpu()
        assert same(vis[n + "_normalize_global"], VR.grid_ref(x, 2, "global")[0]), n
        assert same(vis[n + "_normalize_local"], VR.grid_ref(x, 2, "image")[0]), n
    assert vis[SAMPLE_NAMES[0]] is tr.ema_sample_result_normalize_global and vis[SAMPLE_NAMES[1]] is tr.ema_sample_result_normalize_local

    with _lib.Recording() as rec:                                                            # what the call issues, by name
        tr.get_current_visuals(0)
    assert [c[0] for c in rec.calls] == ["mdm_sampler_x0"] + ["mdm_vis_range", "mdm_vis_grid"] * (2 * len(names))


def _upstream_save_epochs(a, epoch_start, epoch_length):
    """trainer_masked_mean_shift.py:252"""
    return [e for e in range(epoch_start, epoch_start + epoch_length)
            if (e > 0 and (e + 1) % a.save_images_epochs == 0) or e == epoch_start + epoch_length - 1
            or (e + 1) % (epoch_length / a.scheduler_num_scale_timesteps) == 0]


def _dirs(tmp_path):
    d = {k: str(tmp_path / k) for k in ("train_loss", "checkpoint", "ema_sample_img")}
    for v in d.values():
        os.makedirs(v, exist_ok=True)
    return types.SimpleNamespace(list_dir=d)


def _train_args(**kw):
    return base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", batch_size=4,
                     rng_mode="device", seed=3, use_ema=True, sampling="momentum", sample_num=4, sample_history=False,
                     save_images_epochs=1, **kw)


def test_train_shows_upstreams_22_grids_and_writes_the_png(tmp_path):
    calls = []

    class Vis:
        def reset(self):
            calls.append(("reset",))

        def plot_current_losses(self, epoch, losses, kind):
            calls.append(("losses", epoch))

        def display_current_results(self, epoch, visuals):
            calls.append(("display", epoch, visuals))
    a = _train_args(visuals=True, monitor=True)
    tr, model = _make_trainer("ms", a, 1, loader=_loader(2), ema=True)
    dirs = _dirs(tmp_path)
    tr.train(0, 2, 0, 0, dirs, Vis())
    torch.cuda.synchronize()
    saved = _upstream_save_epochs(a, 0, 2)
    assert saved == [1]
    want_calls = []
    for e in (0, 1):
        want_calls += ["reset", "losses"] + (["display"] if e in saved else [])
    assert [c[0] for c in calls] == want_calls                                               # reset once per epoch, at its top
    shown = [c for c in calls if c[0] == "display"]
    assert [c[1] for c in shown] == saved
    vis = shown[-1][2]
    assert list(vis) == [n + sfx for n in MS_NAMES for sfx in ("_normalize_global", "_normalize_local")] + SAMPLE_NAMES and len(vis) == 22
    assert all(v.is_cuda and v.dtype == torch.float32 and v.dim() == 3 and v.shape[0] == 3 for v in vis.values())
    out = dirs.list_dir["ema_sample_img"]
    assert sorted(os.listdir(out)) == [f"ema_sample_{e:05d}.{ext}" for e in saved for ext in ("png", "pt")]
    smp = tr.ema_sample.cpu()
    assert torch.equal(torch.load(os.path.join(out, "ema_sample_00001.pt")), smp) and tuple(smp.shape) == (4, 3, 16, 16)
    want_f, want_u = VR.grid_ref(smp, 2, "global")
    assert torch.equal(_png(os.path.join(out, "ema_sample_00001.png")), want_u)
    assert VR.same_grid(vis[SAMPLE_NAMES[0]], want_f) and VR.same_grid(vis[SAMPLE_NAMES[1]], VR.grid_ref(smp, 2, "image")[0])
    assert VR.same_grid(vis["input_normalize_global"], VR.grid_ref(tr.step.x0.cpu(), 2, "global")[0])


def test_train_without_visuals_is_what_it_was(tmp_path):
    """`visuals` unset and a visualizer that has only `plot_current_losses` (tests/test_monitor_gpu.py's): it finishes, is asked for
    losses alone and no PNG is written"""
    calls = []

    class Vis:
        def plot_current_losses(self, epoch, losses, kind):
            calls.append(epoch)
    tr, model = _make_trainer("ms", _train_args(monitor=True), 1, loader=_loader(2), ema=True)
    dirs = _dirs(tmp_path)
    tr.train(0, 2, 0, 0, dirs, Vis())
    torch.cuda.synchronize()
    assert calls == [0, 1] and tr.visuals is False and not hasattr(tr, "ema_sample_result_normalize_global")
    assert sorted(os.listdir(dirs.list_dir["ema_sample_img"])) == ["ema_sample_00001.pt"]
