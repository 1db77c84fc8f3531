#!/usr/bin/env python3
"""Where the time of an image-folder ingest goes on the device side, against PIL on the host (DESIGN finding 67).

Synthetic decoded images already in memory -- no files, no data set, no decoder:
    case 1: K = 256 images of 1024 x 1024 x 3 -> 64
    case 2: K = 256 images of  512 x  512 x 3 -> 32
For each case: the pinned-to-device copy of the K images (HIP events), `mdm_ingest_resize_crop` over them (HIP events, the median
of `--reps` launches after a warm one), the images/s of copy + kernel, and `PIL.Image.resize((S, S), BILINEAR)` over the same bytes
on a pool of `mdm.ingest.decode_threads()` threads (PIL releases the GIL in its resampler).  The result of the launch is compared
with PIL's on the first and the last image before anything is reported.  One JSON line on stdout, also written to `--out`.

Not measured here: decoding (JPEG / PNG), the host memcpy into the staging chunk, files of mixed shapes.

    python scripts/prof_ingest.py [--k 256] [--reps 5] [--pil-images 64] [--out profiles/ingest.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "masked-diffusion-model_amd"))

from mdm import ingest as I  # noqa: E402

CASES = [(1024, 1024, 3, 64), (512, 512, 3, 32)]


def _events_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def run_case(h, w, C, size, K, reps, pil_images, dev):
    from PIL import Image
    rng = np.random.default_rng(h)
    host = torch.empty(K * h * w * C, dtype=torch.uint8).pin_memory()
    view = host.numpy().reshape(K, h, w, C)
    base = rng.integers(0, 256, size=(8, h, w, C), dtype=np.uint8)          # eight different images, repeated: the bytes do not matter
    for k in range(K):
        view[k] = base[k % 8]
    src = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
    dst = torch.empty(K, C, size, size, dtype=torch.uint8, device=dev)
    plans = I.device_plans(h, w, size, dev)
    copy_ms = _events_ms(lambda: src.copy_(host, non_blocking=True), reps + 1)[1:]
    kern_ms = _events_ms(lambda: I.resize_crop(src, K, h, w, C, plans, dst, 0, size), reps + 1)[1:]
    got = dst.cpu().numpy()
    for k in (0, K - 1):
        want = np.asarray(Image.fromarray(view[k]).resize((size, size), Image.BILINEAR)).transpose(2, 0, 1)
        assert np.array_equal(got[k], want), f"image {k} differs from PIL"
    threads = I.decode_threads()
    n = min(pil_images, K)
    with ThreadPoolExecutor(max_workers=threads) as pool:
        t0 = time.perf_counter()
        list(pool.map(lambda k: Image.fromarray(view[k]).resize((size, size), Image.BILINEAR), range(n)))
        pil_s = time.perf_counter() - t0
    copy, kern = statistics.median(copy_ms), statistics.median(kern_ms)
    in_bytes = K * h * w * C
    return {"shape": [h, w, C], "size": size, "K": K, "copy_ms": round(copy, 3), "copy_GBps": round(in_bytes / copy / 1e6, 1),
            "kernel_ms": round(kern, 3), "kernel_ms_all": [round(v, 3) for v in kern_ms], "kernel_source_GBps": round(in_bytes / kern / 1e6, 1),
            "device_images_per_s": round(K / ((copy + kern) / 1e3)), "pil_threads": threads, "pil_images": n,
            "pil_images_per_s": round(n / pil_s, 1), "device_over_pil": round(K / ((copy + kern) / 1e3) / (n / pil_s), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pil-images", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_ingest.py needs a GPU"
    dev = torch.device("cuda", 0)
    import PIL
    res = {"what": "ingest: copy + mdm_ingest_resize_crop against PIL.Image.resize on the host", "pil": PIL.__version__,
           "device": torch.cuda.get_device_name(0), "cases": [run_case(*c, args.k, args.reps, args.pil_images, dev) for c in CASES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
