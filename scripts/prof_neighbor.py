"""The nearest-neighbour bank on one MI355X (DESIGN finding 68): bank build (`mdm_nn_rows`) and one 100-image query on a uint8 set of
M images of 3 x 256 x 256, `mdm_data_means` over the same storage for comparison, the full-resolution search, and the path before the
bank -- normalize01(dataset.tensor()) + cosine_similarity_matrix + col_argmax -- at the largest M that fits.  Device events, the
median of 3 after a warm call.      python scripts/prof_neighbor.py [M] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "masked-diffusion-model_amd")]
import torch  # noqa: E402

import mdm  # noqa: E402
from mdm import evaluate as E  # noqa: E402

PEAK = 8.0e12
dev = torch.device("cuda:0")
out = {}


def timed(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)[len(ts) // 2], ts


def dataset(M, size=256):
    g = torch.Generator(device=dev).manual_seed(M)
    data = torch.randint(0, 256, (M, 3, size, size), dtype=torch.uint8, device=dev, generator=g)
    return mdm.DeviceDataset(data, random=torch.zeros(M, 1), device=dev)


M = int(sys.argv[1]) if len(sys.argv) > 1 else 30000
ds = dataset(M)
E_img = 3 * 256 * 256
src = torch.rand(100, 3, 256, 256, device=dev)

t, ts = timed(lambda: ds.means(per_channel=False))
out["data_means"] = dict(M=M, seconds=t, all=ts, images_per_s=M / t, bytes_per_s=M * E_img / t, frac_hbm_peak=M * E_img / t / PEAK)

bank = None
def build():
    global bank
    bank = E.NeighborBank(ds, size=32, antialias=True)
t, ts = timed(build)
traffic = M * (2 * E_img + 3 * 3072 * 4)                      # the storage twice, the row written, read back and written again
out["bank_build"] = dict(M=M, seconds=t, all=ts, images_per_s=M / t, storage_bytes_per_s=M * E_img / t, traffic_bytes_per_s=traffic / t,
                         frac_hbm_peak=traffic / t / PEAK, vs_data_means=out["data_means"]["seconds"] / t * 2)

t, ts = timed(lambda: bank.nearest_idx(src))
out["query_100_cached"] = dict(M=M, seconds=t, all=ts, images_per_s=M / t)
chunked = E.NeighborBank(ds, size=32, antialias=True, cache_bytes=0)
t, ts = timed(lambda: chunked.nearest_idx(src))
out["query_100_rebuilt"] = dict(M=M, seconds=t, all=ts, images_per_s=M / t)
t, ts = timed(lambda: bank.source_rows(src))
out["source_rows_100"] = dict(seconds=t, all=ts)
idx_new = bank.nearest_idx(src).cpu()
del bank, chunked

# Tester's full-resolution comparison through the bank, rows rebuilt per query (they do not fit the default cache at this size)
full = E.NeighborBank(ds, size=None, chunk=1024)
t, ts = timed(lambda: full.nearest_idx(src), reps=2)
out["query_100_full_resolution"] = dict(M=M, cached=full.cached, seconds=t, all=ts, images_per_s=M / t)
idx_full = full.nearest_idx(src).cpu()
del full
torch.cuda.empty_cache()

# the parent commit's path: normalize01(dataset.tensor()) + cosine_similarity_matrix + col_argmax, at the largest M that fits
Mp = M
while Mp >= 1000:
    try:
        dp = ds if Mp == M else dataset(Mp)
        def parent():
            data = E.normalize01(dp.tensor())
            return E.col_argmax(E.cosine_similarity_matrix(src, data))[1]
        t, ts = timed(parent, reps=2)
        out["parent_path"] = dict(M=Mp, seconds=t, all=ts, images_per_s=Mp / t)
        if Mp == M:
            out["parent_path"]["same_idx_as_full_resolution_bank"] = bool(torch.equal(parent().cpu(), idx_full))
        break
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        out.setdefault("parent_oom_at", []).append(Mp)
        Mp //= 2

if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out, indent=1))
