"""The restoration sampler on one MI355X (DESIGN finding 72).

timing:  `mdm_restore_x0` on [100, 3, 64, 64] and [100, 3, 256, 256] for (k, gray) = (4, 0), (1, 1), (8, 1), next to `mdm_inpaint_x0`
         and `mdm_sampler_x0` on the same operands in the same run: a bf16 NHWC prediction with Cp = 8, a shift, no history outputs
         (what a reverse step of the graph loop launches).  The project's device events around `reps` back-to-back calls; 7 windows
         per kernel, the kernels taking turns window by window; median, smallest and largest.  Bytes are the algorithm's: every
         operand once.
quality: the trained 16 x 16 fixture net (tests/golden/trained_tiny.npz) restoring 64 held-out smooth images from their pool 2 and
         pool 4 colour measurements and their pool 1 grey one, from both starts, next to the `expand` baseline: PSNR and SSIM, mean
         and standard deviation over the images.

    python scripts/prof_restore.py [out.json] [timing|quality|all]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "masked-diffusion-model_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mdm  # noqa: E402
from mdm import _lib  # noqa: E402

PEAK = 8.0e12
dev = torch.device("cuda:0")
lib = _lib.load()
out = {}
what = sys.argv[2] if len(sys.argv) > 2 else "all"


def window(fn, reps):
    """seconds per call: device events (mdm_event_*) around `reps` calls"""
    st = _lib.stream()
    a, b, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
    _lib.check(lib.mdm_event_create(ctypes.byref(a))); _lib.check(lib.mdm_event_create(ctypes.byref(b)))
    _lib.check(lib.mdm_event_record(a, st))
    for _ in range(reps):
        fn()
    _lib.check(lib.mdm_event_record(b, st))
    _lib.check(lib.mdm_event_elapsed_ms(a, b, ctypes.byref(ms)))
    lib.mdm_event_destroy(a); lib.mdm_event_destroy(b)
    return ms.value * 1e-3 / reps


def timing():
    g = torch.Generator(device=dev).manual_seed(1)
    N, C, Cp = 100, 3, 8
    for H, reps in ((64, 400), (256, 60)):
        img = lambda: torch.rand(N, C, H, H, device=dev, generator=g) * 2 - 1
        pred = (torch.rand(N, H, H, Cp, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
        x_in, s, known, x0 = img(), img(), img(), img()
        keep = mdm.inpaint_keep("box", N, H, H, top=H // 4, left=H // 4, height=H // 2, width=H // 2).to(dev)
        common = dict(dtype=_lib.BF16, pred_nhwc=pred.data_ptr(), Cp=Cp, x_in=x_in.data_ptr(), s=s.data_ptr(), N=N, C=C, H=H, W=H,
                      pred_nchw=None, shifted0=None, x0_hat=x0.data_ptr())
        plane = N * C * H * H * 4
        base = pred.numel() * 2 * C // Cp + 3 * plane          # the C channels of the prediction, x_in, s, x0_hat
        fns = {"mdm_sampler_x0": (lambda: _lib.call("mdm_sampler_x0", stream=_lib.stream(), **common), base),
               "mdm_inpaint_x0": (lambda: _lib.call("mdm_inpaint_x0", known=known.data_ptr(), keep=keep.data_ptr(), keep_C=1,
                                                    stream=_lib.stream(), **common), base + plane + keep.numel() * 4)}
        ys = {}
        for k, gray in ((4, 0), (1, 1), (8, 1)):
            ys[k, gray] = mdm.restore_measure(known, k, bool(gray))
            fns[f"mdm_restore_x0 k={k} gray={gray}"] = (
                lambda k=k, gray=gray: _lib.call("mdm_restore_x0", y=ys[k, gray].data_ptr(), k=k, gray=gray, stream=_lib.stream(), **common),
                base + ys[k, gray].numel() * 4)
        for fn, _ in fns.values():
            fn(); fn()
        torch.cuda.synchronize()
        times = {name: [] for name in fns}
        for _ in range(7):                                      # the kernels take turns: a drift of the machine meets all of them
            for name, (fn, _) in fns.items():
                times[name].append(window(fn, reps))
        rows = {}
        for name, (_, nbytes) in fns.items():
            ts = sorted(times[name])
            rows[name] = dict(bytes=nbytes, seconds=ts[3], smallest=ts[0], largest=ts[-1], bytes_per_s=nbytes / ts[3],
                              frac_hbm_peak=nbytes / ts[3] / PEAK)
        for name in rows:
            rows[name]["over_inpaint_x0"] = rows[name]["seconds"] / rows["mdm_inpaint_x0"]["seconds"]
        out[f"x0_{H}"] = rows
        print(f"x0_{H}", json.dumps(rows), flush=True)
        del pred, x_in, s, known, x0, keep, ys
        torch.cuda.empty_cache()


def quality(n=64, hw=16, T=1000):
    from golden.make_golden import TINY, base_args, seed_all
    from golden.make_trained_tiny import smooth_images
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_tiny.npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    model = mdm.UNet(TINY, N=n, H=hw, W=hw, dtype=mdm.F32, params=params).eval()
    truth = smooth_images(n, torch.Generator().manual_seed(31337)).contiguous().to(dev)       # the training drew from seed 2024
    stat = lambda t: dict(mean=float(t.double().mean()), std=float(t.double().std()))
    rows = []
    for dep, mode in (("dependent_prev", "base_sampling"), ("dependent_prev", "base_momentum")):
        for pool, gray in ((2, False), (4, False), (1, True)):
            a = base_args(data_size=hw, ddpm_schedule="linear", ddpm_num_steps=T, shift_type="noise_with_perturbation",
                          sampling_mask_dependency=dep, momentum_adaptive=mode, sample_num=n, sample_latent_shape="uniform",
                          sample_history=False, rng_mode="device", seed=3)
            s = mdm.Scheduler(a)
            s.update_ddpm_num_steps(T)
            smp = mdm.Sampler(None, a, s, [None] * 3)
            seed_all(17)
            res = smp.evaluate_restore(model, s.get_timesteps_epoch(0, 1), truth, pool, gray)
            for start, m in res.items():
                row = dict(sampler=f"{dep}/{mode}", pool=pool, gray=gray, start=start, images=n, psnr=stat(m.psnr), ssim=stat(m.ssim),
                           psnr_gain_over_expand=stat(m.psnr - res["expand"].psnr), ssim_gain_over_expand=stat(m.ssim - res["expand"].ssim))
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
