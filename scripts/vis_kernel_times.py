"""Kernel times of the image-grid kernels (csrc/vis.hip) at the size DESIGN section 7 quotes: K = 100 images of 3 x 64 x 64, nrow 10.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/vis_kernel_times.py --run
    python scripts/vis_kernel_times.py --parse OUT

`--run` issues, per variant below, WARM launches that are not counted and then REPS launches, first on one batch (warm: the 4.9 MB
input stays in the last-level cache) and then rotating over NBUF batches (cold: 64 x 4.9 MB = 315 MB, more than the 256 MB cache).
`--parse` reads the dispatches of the three kernels back from the trace in issue order and prints, per variant, the median and the
fastest time and the bytes the algorithm needs (input read once, every output element written once) over the median.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "masked-diffusion-model_amd"))

K, C, H, W, NROW = 100, 3, 64, 64, 10
WARM, REPS, NBUF = 5, 30, 64
KERNELS = ("range_image_kernel", "range_global_kernel", "grid_kernel")
# (name, kernel, normalisation, output form)
VARIANTS = [("range per image", "range", "image", None), ("range over the batch", "range", "global", None),
            ("grid mode 1 -> f32", "grid", "image", "f32"), ("grid mode 2 -> f32", "grid", "global", "f32"),
            ("grid mode 2 -> f32 + u8", "grid", "global", "both"), ("grid mode 2 -> u8", "grid", "global", "u8")]


def variant_bytes(kernel, form):
    from mdm import visuals
    cg, hg, wg = visuals.grid_shape(K, C, H, W, NROW)
    rd = K * C * H * W * 4
    if kernel == "range":
        return rd
    return rd + cg * hg * wg * ((4 if form != "u8" else 0) + (1 if form != "f32" else 0))


def run():
    import torch
    from mdm import _lib, visuals
    from mdm._lib import call, ptr, stream
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    bufs = [torch.randn(K, C, H, W, device=dev, generator=g) for _ in range(NBUF)]
    cg, hg, wg = visuals.grid_shape(K, C, H, W, NROW)
    f32 = torch.empty(cg, hg, wg, device=dev)
    u8 = torch.empty(hg, wg, cg, dtype=torch.uint8, device=dev)
    lohi = {"image": visuals.image_range(bufs[0], True), "global": visuals.image_range(bufs[0], False)}
    scratch = torch.zeros(4, device=dev)
    E = C * H * W

    def launch(kernel, norm, form, x):
        if kernel == "range":
            call("mdm_vis_range", ptr(x), E, K, E, int(norm == "global"), ptr(lohi[norm]), ptr(scratch), stream())
        else:
            call("mdm_vis_grid", ptr(x), E, K, C, H, W, ptr(lohi[norm]), visuals.MODES[norm], NROW, 2, 0.0,
                 ptr(f32) if form != "u8" else None, ptr(u8) if form != "f32" else None, stream())
    torch.cuda.synchronize()
    for _, kernel, norm, form in VARIANTS:
        for rotate in (False, True):
            for i in range(WARM + REPS):
                launch(kernel, norm, form, bufs[i % NBUF] if rotate else bufs[0])
            torch.cuda.synchronize()
    print("issued", len(VARIANTS) * 2 * (WARM + REPS), "launches")


def parse(out_dir):
    rows = []
    for path in sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                if any(k in r["Kernel_Name"] for k in KERNELS):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    rows = rows[2:]                                        # the two launches that fill `lohi` before the timed sequence
    per = WARM + REPS
    assert len(rows) == len(VARIANTS) * 2 * per, (len(rows), len(VARIANTS) * 2 * per)
    out = []
    for v, (name, kernel, norm, form) in enumerate(VARIANTS):
        for c, cache in enumerate(("warm", "cold")):
            chunk = rows[(2 * v + c) * per:(2 * v + c + 1) * per][WARM:]
            assert all(("range" in kn) == (kernel == "range") for _, _, kn in chunk), name
            us = [(e - s) / 1e3 for s, e, _ in chunk]
            med, nb = statistics.median(us), variant_bytes(kernel, form)
            out.append(dict(variant=name, cache=cache, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                            bytes=nb, gb_per_s=round(nb / med / 1e3, 1)))
            print(json.dumps(out[-1]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parse", metavar="DIR")
    a = ap.parse_args()
    if a.run:
        run()
    if a.parse:
        parse(a.parse)
