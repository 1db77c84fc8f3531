"""Image metrics on one MI355X (DESIGN finding 71).

timing:  `mdm_metric_image` on [100, 3, 64, 64] and [100, 3, 256, 256] against one `truth`, and on a [1001, 100, 3, 64, 64] history in
         place; `mdm_data_means` over the same number of bytes in the same run (the yardstick of finding 68); the same metrics stated in
         torch on the device (F.conv2d with the 11-tap windows).  The project's device events around `reps` back-to-back calls, the
         median of 5 windows after two warm calls.
quality: the trained 16 x 16 fixture net (tests/golden/trained_tiny.npz) completing 64 held-out smooth images under the `box`, `half`
         and `random` holes of `inpaint_keep`, from the three starts, next to `mean_fill_baseline`: psnr_hole and ssim_hole, mean and
         standard deviation over the images, and the reverse steps each start ran.

    python scripts/prof_metrics.py [out.json] [timing|quality|all]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "masked-diffusion-model_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mdm  # noqa: E402
from mdm import _lib  # noqa: E402

PEAK = 8.0e12
dev = torch.device("cuda:0")
lib = _lib.load()
out = {}
what = sys.argv[2] if len(sys.argv) > 2 else "all"


def timed(fn, reps):
    """seconds per call: device events (mdm_event_*) around `reps` calls, the median of 5 windows after two warm calls"""
    st = _lib.stream()
    fn(); fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
        _lib.check(lib.mdm_event_create(ctypes.byref(a))); _lib.check(lib.mdm_event_create(ctypes.byref(b)))
        _lib.check(lib.mdm_event_record(a, st))
        for _ in range(reps):
            fn()
        _lib.check(lib.mdm_event_record(b, st))
        _lib.check(lib.mdm_event_elapsed_ms(a, b, ctypes.byref(ms)))
        lib.mdm_event_destroy(a); lib.mdm_event_destroy(b)
        ts.append(ms.value * 1e-3 / reps)
    return sorted(ts)[2], ts


def torch_metrics(pred, truth, keep, L=2.0):
    """the same eight numbers in torch on the device, fp32: separable F.conv2d with the plan's window"""
    R, C, H, W = pred.shape
    w = torch.tensor(mdm.metrics.plan(R, C, H, W).window, device=pred.device)
    t = truth.repeat(R // truth.shape[0], 1, 1, 1)
    hole = (keep == 0).expand(truth.shape).repeat(R // truth.shape[0], 1, 1, 1)
    p = pred.clamp(-1.0, 1.0)
    win = lambda x: F.conv2d(F.conv2d(x.reshape(R * C, 1, H, W), w.view(1, 1, 1, 11)), w.view(1, 1, 11, 1)).reshape(R, C, H - 10, W - 10)
    mp, mt = win(p), win(t)
    vp, vt, cv = win(p * p) - mp * mp, win(t * t) - mt * mt, win(p * t) - mp * mt
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    smap = ((2 * mp * mt + C1) * (2 * cv + C2)) / ((mp * mp + mt * mt + C1) * (vp + vt + C2))
    sq = (p - t) ** 2
    hc = hole[:, :, 5:H - 5, 5:W - 5]
    mse, mse_h = sq.mean((1, 2, 3)), (sq * hole).sum((1, 2, 3)) / hole.sum((1, 2, 3))
    return torch.stack((mse, 10 * torch.log10(L * L / mse), smap.mean((1, 2, 3)), mse_h, 10 * torch.log10(L * L / mse_h),
                        (smap * hc).sum((1, 2, 3)) / hc.sum((1, 2, 3))), 1)


def timing():
    g = torch.Generator(device=dev).manual_seed(1)
    for name, lead, N, H, reps in (("batch_64", (100,), 100, 64, 200), ("batch_256", (100,), 100, 256, 40), ("history_64", (1001, 100), 100, 64, 2)):
        C = 3
        R = int(np.prod(lead))
        try:
            pred = torch.rand(*lead, C, H, H, device=dev, generator=g) * 2.4 - 1.2
        except torch.cuda.OutOfMemoryError:
            out[name] = "does not fit"
            continue
        truth = torch.rand(N, C, H, H, device=dev, generator=g) * 2 - 1
        keep = mdm.inpaint_keep("box", N, H, H, top=H // 4, left=H // 4, height=H // 2, width=H // 2).to(dev)
        need = lib.mdm_metric_ws_bytes(R, C, H, H)
        ws, res = torch.empty(need // 8, dtype=torch.float64, device=dev), torch.empty(R, 8, device=dev)
        def kernel():
            _lib.call("mdm_metric_image", pred=pred.data_ptr(), truth=truth.data_ptr(), keep=keep.data_ptr(), Ck=1, R=R, N=N, C=C, H=H, W=H,
                      clamp_lo=-1.0, clamp_hi=1.0, data_range=2.0, ws=ws.data_ptr(), ws_bytes=need, out=res.data_ptr(), stream=_lib.stream())
        nbytes = (pred.numel() + truth.numel() + keep.numel()) * 4
        t, ts = timed(kernel, reps)
        p = mdm.metrics.plan(R, C, H, H)
        row = dict(shape=list(pred.shape), bytes_read_once=nbytes, workspace_bytes=need, tile_workgroups=p.grid[0], seconds=t, all=ts,
                   bytes_per_s=nbytes / t, frac_hbm_peak=nbytes / t / PEAK)
        t, ts = timed(lambda: mdm.image_metrics(pred, truth, keep), reps)
        row["python_surface_seconds"] = t
        # the yardstick: mdm_data_means over as many bytes of float images
        M = nbytes // (4 * C * H * H)
        src, means = torch.empty(M * C * H * H, device=dev).uniform_(-1, 1), torch.empty(M, device=dev)
        def yard():
            _lib.call("mdm_data_means", src=src.data_ptr(), kind=0, img_stride=C * H * H, M=M, C=C, H=H, W=H, lut=None, per_channel=0,
                      out=means.data_ptr(), stream=_lib.stream())
        ty, tys = timed(yard, reps)
        row["data_means"] = dict(bytes=M * C * H * H * 4, seconds=ty, all=tys, bytes_per_s=M * C * H * H * 4 / ty)
        row["seconds_over_data_means"] = row["seconds"] / ty
        del src
        if len(lead) == 1:                      # the statement in torch on the device (its intermediates do not fit for the history)
            want = torch_metrics(pred, truth, keep)
            kernel()
            row["max_abs_diff_vs_torch_fp32"] = float((res[:, :6] - want).abs().max())
            tt, tts = timed(lambda: torch_metrics(pred, truth, keep), max(1, reps // 10))
            row["torch_on_device"] = dict(seconds=tt, all=tts, over_kernel=tt / row["seconds"])
        out[name] = row
        print(name, json.dumps(row), flush=True)
        del pred, truth, keep, ws, res
        torch.cuda.empty_cache()


def quality(n=64, hw=16, T=1000):
    from golden.make_golden import TINY, base_args, seed_all
    from golden.make_trained_tiny import smooth_images
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_tiny.npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    model = mdm.UNet(TINY, N=n, H=hw, W=hw, dtype=mdm.F32, params=params).eval()
    truth = smooth_images(n, torch.Generator().manual_seed(31337)).contiguous().to(dev)       # the training drew from seed 2024
    holes = dict(box=mdm.inpaint_keep("box", n, hw, hw, top=4, left=4, height=8, width=8), half=mdm.inpaint_keep("half", n, hw, hw, side="right"),
                 random=mdm.inpaint_keep("random", n, hw, hw, p=0.5, generator=torch.Generator().manual_seed(9)))
    stat = lambda t: dict(mean=float(t.double().mean()), std=float(t.double().std()))
    rows = []
    for dep, mode in (("dependent_prev", "base_sampling"), ("dependent_prev", "base_momentum")):
        for hole, keep in holes.items():
            keep = keep.to(dev)
            a = base_args(data_size=hw, ddpm_schedule="linear", ddpm_num_steps=T, shift_type="noise_with_perturbation",
                          sampling_mask_dependency=dep, momentum_adaptive=mode, sample_num=n, sample_latent_shape="uniform",
                          sample_history=False, rng_mode="device", seed=3)
            s = mdm.Scheduler(a)
            s.update_ddpm_num_steps(T)
            smp = mdm.Sampler(None, a, s, [None] * 3)
            seed_all(17)
            res = smp.evaluate_inpaint(model, s.get_timesteps_epoch(0, 1), truth, keep)
            res["mean_fill_baseline"] = mdm.image_metrics(mdm.mean_fill_baseline(truth, keep), truth, keep)
            for start, m in res.items():
                row = dict(sampler=f"{dep}/{mode}", hole=hole, start=start, steps=smp.inpaint_steps_run.get(start, 0), images=n,
                           hole_elements=float(m.hole_count.mean()), psnr_hole=stat(m.psnr_hole), ssim_hole=stat(m.ssim_hole),
                           psnr=stat(m.psnr), ssim=stat(m.ssim))
                rows.append(row)
                print(json.dumps(row), flush=True)
    out["quality"] = rows


if what in ("timing", "all"):
    timing()
if what in ("quality", "all"):
    quality()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
