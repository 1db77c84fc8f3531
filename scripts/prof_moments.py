"""Set moments on one MI355X (DESIGN finding 73).

`mdm_moment_accumulate` (carry 0) on [30 000 x 3072] float rows, on the same set as uint8 read in place through the table, on
[100 x 3072] (one sampler round) and on [4096 x 192]; in the same run `X.double().T @ X.double()` in torch on the device and
`mdm_data_means` over the same bytes; and the host `eigh` pair of `frechet_distance` at d = 3072.  The project's device events around
`reps` back-to-back calls, the median of 5 windows after two warm calls.  The fp64 matrix rate the kernel is held against comes from a
calibration loop of the same instruction, scripts/micro/mfma_f64_rate (run first, as a child process, when it has been built).

    python scripts/prof_moments.py [out.json] [noeigh]"""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "masked-diffusion-model_amd")]
out = {}
CAL = os.path.join(ROOT, "scripts", "micro", "mfma_f64_rate")
if os.path.exists(CAL):                          # before this process opens the device
    r = subprocess.run([CAL], capture_output=True, text=True, timeout=120)
    out["calibration"] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 and r.stdout.strip() else f"failed ({r.returncode})"
    print("calibration", out["calibration"], flush=True)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mdm  # noqa: E402
from mdm import _lib  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
rate = max(out["calibration"]["tflops_4_waves"], out["calibration"]["tflops_8_waves"]) * 1e12 if isinstance(out.get("calibration"), dict) else None


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


def case(name, R, d, kind, reps, C=3):
    g = torch.Generator(device=dev).manual_seed(1)
    if kind == 1:
        rows = torch.randint(0, 256, (R, d), dtype=torch.uint8, device=dev, generator=g)
        lut = mdm.data.normalize_lut().to(dev)
    else:
        rows, lut = torch.rand(R, d, device=dev, generator=g) * 2 - 1, None
    p = mdm.moment_plan(R, d)
    ws = torch.empty(p.ws_bytes // 8, dtype=torch.float64, device=dev)
    s, o = torch.empty(d, dtype=torch.float64, device=dev), torch.empty(d, d, dtype=torch.float64, device=dev)
    def kernel():
        _lib.call("mdm_moment_accumulate", rows=rows.data_ptr(), kind=kind, lut=_lib.ptr(lut), row_ld=d, R=R, d=d, carry=0, sum=s.data_ptr(),
                  outer=o.data_ptr(), outer_ld=d, ws=ws.data_ptr(), ws_bytes=p.ws_bytes, stream=_lib.stream())
    t, ts = timed(kernel, reps)
    done = 2.0 * R * p.tiles * p.tile * p.tile              # the FLOPs the tiles of the triangle run, masked columns included
    row = dict(shape=[R, d], kind=("float", "uint8")[kind], plan=p._asdict(), seconds=t, all=ts, flops_run=done, flops_per_s=done / t,
               useful_flops_per_s=float(R) * d * (d + 1) / t, row_bytes=rows.numel() * rows.element_size())
    if rate:
        row["frac_of_calibrated_f64_matrix_rate"] = done / t / rate
    x = rows.float() if kind == 0 else lut[rows.long()]
    if R * d * 8 <= 2 << 30:                               # the statement in torch on the device: an fp64 copy, then the product
        want = x.double().T @ x.double()
        kernel()
        row["max_abs_diff_vs_torch_f64"] = float((o - want).abs().max())
        row["bit_symmetric"] = bool(torch.equal(o, o.T))
        del want
        tt, tts = timed(lambda: x.double().T @ x.double(), max(1, reps // 2))
        row["torch_f64_on_device"] = dict(seconds=tt, all=tts, over_kernel=tt / t)
        xd = x.double()
        tt2, _ = timed(lambda: xd.T @ xd, max(1, reps // 2))
        row["torch_f64_on_device"]["product_alone_seconds"] = tt2
        del xd
    if d % C == 0 and int(round((d // C) ** 0.5)) ** 2 == d // C:      # the yardstick: mdm_data_means over the same bytes
        H = int(round((d // C) ** 0.5))
        means = torch.empty(R, device=dev)
        def yard():
            _lib.call("mdm_data_means", src=rows.data_ptr(), kind=kind, img_stride=d, M=R, C=C, H=H, W=H, lut=_lib.ptr(lut), per_channel=0,
                      out=means.data_ptr(), stream=_lib.stream())
        ty, tys = timed(yard, reps)
        row["data_means"] = dict(seconds=ty, all=tys, bytes_per_s=row["row_bytes"] / ty)
        row["seconds_over_data_means"] = t / ty
    out[name] = row
    print(name, json.dumps(row), flush=True)
    del rows, ws, s, o, x
    torch.cuda.empty_cache()


case("set_30000x3072_float", 30000, 3072, 0, 3)
case("set_30000x3072_uint8", 30000, 3072, 1, 3)
case("round_100x3072_float", 100, 3072, 0, 20)
case("bank_4096x192_float", 4096, 192, 0, 50)

if "noeigh" not in sys.argv[2:]:
    g = np.random.default_rng(0)
    n, d = 4000, 3072
    xa, xb = g.normal(size=(n, d)), g.normal(size=(n, d)) * 1.1 + 0.05
    a, b = mdm.SetMoments.from_rows(xa), mdm.SetMoments.from_rows(xb)
    t0 = time.perf_counter()
    r = mdm.frechet_distance(a, b)
    out["frechet_host_d3072"] = dict(seconds=time.perf_counter() - t0, threads=torch.get_num_threads(), distance=r.distance, clipped=r.clipped)
    print("frechet_host_d3072", json.dumps(out["frechet_host_d3072"]), flush=True)

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
