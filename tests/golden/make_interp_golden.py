#!/usr/bin/env python3
"""Generate tests/golden/sampler_interp.npz by RUNNING THE REFERENCE's `Sampler._sample_interpolation` (sampler.py:264-366).

    python tests/golden/make_interp_golden.py

Needs the reference checkout like make_golden.py, whose stubs and helpers it uses.  Only settings, inputs and outputs are stored.
Of the ten history lists five are stored as they come (tests/_interp_ref.py FIXTURE_LISTS), `shift` as its one value per
sample, and four are left out because they are single fp32 operations of stored tensors -- this script asserts that
`fixture_hist` rebuilds all ten bit for bit from what it stores before it writes the file.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
from _interp_ref import FIXTURE_LISTS, INTERP_HISTORY_NAMES, fixture_args, fixture_hist  # noqa: E402

# dependency, momentum_adaptive, mean_option, mean_area, select, channel, schedule, interpolation_shift
CASES = [("independent", "base_momentum", 0, "image-wise", "thresholding", "1-channel", "linear", -0.4),
         ("dependent", "base_momentum", "degraded_area", "channel-wise", "thresholding", "1-channel", "exponential", 0.3),
         ("independent", "base_sampling", "non_degraded_area", "image-wise", "thresholding", "1-channel", "exponential", 0.0),
         ("independent", "base_momentum", 0.25, "image-wise", "indexing", None, "log", -0.4)]
FAILS = [("independent", "momentum", 0, "image-wise", "thresholding", "1-channel", "linear", 0.3),
         ("independent", "base_momentum", None, "image-wise", "thresholding", "1-channel", "linear", 0.3)]


def _cfg(row):
    dep, mode, mo, ma, sel, ch, kind, shift = row
    return np.array([dep, mode, str(mo), type(mo).__name__, ma, sel, str(ch), kind, repr(shift)])


def _run(scheduler_mod, sampler_mod, unet6, cfg, seed):
    a, shift = fixture_args(cfg, G.base_args)
    s = scheduler_mod.Scheduler(a)
    s.update_ddpm_num_steps(a.ddpm_num_steps)
    ts = s.get_timesteps_epoch(0, 1)
    smp = sampler_mod.Sampler(None, a, s, [None] * 3)
    model = G._Wrap(G.build_ref_unet(unet6, G.TINY)).eval()
    G.seed_all(seed)
    return ts, smp, smp._sample_interpolation(model, ts, shift)


def main():
    G._stub_modules()
    sys.path.insert(0, G.REF)
    import scheduler as scheduler_mod
    import sampler as sampler_mod
    from models.unet import unet6
    torch.set_num_threads(4)
    out = {}
    for i, row in enumerate(CASES):
        cfg, seed = _cfg(row), 1100 + i
        ts, smp, (x0, mu, hist) = _run(scheduler_mod, sampler_mod, unet6, cfg, seed)
        hist = np.stack([G.npy(h) for h in hist])
        assert np.isfinite(hist).all() and np.isfinite(G.npy(x0)).all(), i
        out[f"interp{i}_cfg"], out[f"interp{i}_seed"], out[f"interp{i}_ts"] = cfg, np.array(seed), np.array(ts)
        out[f"interp{i}_x0"], out[f"interp{i}_mu"] = G.npy(x0), G.npy(mu)
        sh = hist[INTERP_HISTORY_NAMES.index("shift")]
        assert (sh == sh[:, :, :1, :1, :1]).all()                                  # one value per sample and step
        out[f"interp{i}_shift"] = sh[:, :, 0, 0, 0].copy()
        for k in FIXTURE_LISTS:
            out[f"interp{i}_{k}"] = hist[INTERP_HISTORY_NAMES.index(k)]
        latent = G.npy(smp._get_latent_initial_interpolation(float(cfg[-1]))[0])
        assert np.array_equal(fixture_hist(out, i, latent), hist), f"case {i}: the stored lists do not rebuild the reference's ten"
    out["interp_n"] = np.array(len(CASES))
    for j, row in enumerate(FAILS):
        try:
            _run(scheduler_mod, sampler_mod, unet6, _cfg(row), 1200 + j)
            err = "none"
        except Exception as e:          # noqa: BLE001
            err = type(e).__name__
        out[f"interp_fail{j}"] = np.append(_cfg(row), err)
    out["interp_nfail"] = np.array(len(FAILS))
    path = os.path.join(HERE, "sampler_interp.npz")
    np.savez_compressed(path, **out)
    print(f"sampler_interp: {len(out)} arrays -> {path} ({os.path.getsize(path) / 1024:.0f} KiB); failures "
          f"{[str(out[f'interp_fail{j}'][-1]) for j in range(len(FAILS))]}")


if __name__ == "__main__":
    main()
