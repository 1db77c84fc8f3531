"""bench.py's plain run on the GPU: it times exactly `--steps` steps, prints the headline line without the `--full` legs, and
`--dump-outputs DIR` writes one step of the timed path run from the seeded initial state -- the same inputs on every run, whatever
`--steps` / `--warmup` were."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8


def _bench_dump(out_dir, steps, warmup):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--batch", str(N), "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_bench_plain_run_and_dump_outputs(tmp_path):
    runs = [_bench_dump(tmp_path / f"run{k}", steps, warmup) for k, (steps, warmup) in enumerate(((3, 1), (5, 2)))]
    for (line, d), (steps, warmup) in zip(runs, ((3, 1), (5, 2))):
        assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-3)
        assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        # the --full legs stay out of a plain run
        assert line["roofline"] is None and line["step_hbm"] is None and line["cpu_baseline"] is None and line["sampler"] is None
        assert "extras" not in line and line["windows"]["n"] == 1
        assert set(d) == {"loss", "t", "shift", "x_in", "pred", "params", "ema"}, sorted(d)
        assert all(a.dtype in (np.float32, np.float64) for a in d.values())
        assert sum(a.nbytes for a in d.values()) <= 64 << 20
        assert d["loss"].shape == (1,) and np.isfinite(d["loss"]).all()
        for k in ("shift", "x_in", "pred"):
            assert d[k].shape == (N, 3, 32, 32) and np.isfinite(d[k]).all(), k
        assert d["params"].shape == d["ema"].shape == (1 << 22,) and np.isfinite(d["params"]).all()
        # pred is the prediction of the dumped step: its loss = mean(((x_in + pred) - s - x0)^2), x0 = bench's batch
        x0 = (torch.rand(N, 3, 32, 32, generator=torch.Generator().manual_seed(100)) * 2 - 1).double().numpy()
        want = float(np.mean(((d["x_in"].astype(np.float64) + d["pred"]) - d["shift"] - x0) ** 2))
        assert abs(float(d["loss"][0]) - want) <= 1e-4 * want, (float(d["loss"][0]), want)
    (_, a), (_, b) = runs
    # the dumped step starts from the same state on every run: timesteps, shifts and the degraded input agree bit for bit,
    # what the step computes from them to the rounding of its float-atomic sums
    for k in ("t", "shift", "x_in"):
        assert np.array_equal(a[k], b[k]), k
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= 1e-6 * float(b["loss"][0]), (a["loss"], b["loss"])
    for k in ("pred", "params", "ema"):
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        assert np.linalg.norm(x - y) <= 1e-6 * np.linalg.norm(y), (k, float(np.abs(x - y).max()))
