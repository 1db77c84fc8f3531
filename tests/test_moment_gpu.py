"""The Python surface of the set moments on the GPU (mdm/moments.py, NeighborBank.moments / source_moments, Sampler.evaluate_frechet):
`SetMoments.update` is the kernel call bit for bit, `update_dataset` reads a uint8 `DeviceDataset` in place and equals the fold of its
fp32 copy, the bank's moments are the fold of its rows cached or not, the source goes through the bank's own map, `frechet_distance`
of device-made objects is the same function on host copies, and `evaluate_frechet` on the trained 16 x 16 fixture net is the fold of
explicit `sample` calls from the same generator and Philox states.  No ordering or quality claim is asserted."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _moment_ref as MM  # noqa: E402
from golden.make_golden import TINY, base_args, seed_all  # noqa: E402
from golden.make_trained_tiny import smooth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HW, T = 4, 16, 10


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint64)


def _same(a, b):
    return a.n == b.n and a.d == b.d and np.array_equal(_bits(a.sum), _bits(b.sum)) and np.array_equal(_bits(a.outer), _bits(b.outer))


def _kernel_call(rows2d, d, carry_into=None):
    """mdm_moment_accumulate on fp32 rows [R][ld] -> (sum, outer) device tensors"""
    from mdm import _lib
    R, ld = rows2d.shape[0], rows2d.stride(0)
    need = _lib.load().mdm_moment_ws_bytes(R, d)
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    s, o = carry_into if carry_into is not None else (torch.empty(d, dtype=torch.float64, device="cuda"),
                                                       torch.empty(d, d, dtype=torch.float64, device="cuda"))
    _lib.call("mdm_moment_accumulate", rows=rows2d.data_ptr(), kind=0, lut=None, row_ld=ld, R=R, d=d, carry=int(carry_into is not None),
              sum=s.data_ptr(), outer=o.data_ptr(), outer_ld=d, ws=ws.data_ptr(), ws_bytes=need, stream=_lib.stream())
    return s, o


def _inside(m, x, chunks):
    """the moments `m` against math.fsum over the host rows x [R][d], folded in by calls of `chunks` rows each: the header's bound with
    s the largest split count of those calls and c the calls after the first"""
    import mdm
    assert sum(chunks) == x.shape[0] == m.n
    ref_s, ref_o, mag_s, mag_o = MM.fsum_moments(x)
    splits = max(mdm.moment_plan(c, x.shape[1]).splits for c in chunks)
    return MM.inside(m.sum.cpu().numpy(), ref_s, MM.bound(x.shape[0], splits, len(chunks) - 1, mag_s, ref_s)) and \
        MM.inside(m.outer.cpu().numpy(), ref_o, MM.bound(x.shape[0], splits, len(chunks) - 1, mag_o, ref_o))


def test_update_on_an_image_batch_is_the_kernel_call():
    import mdm
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(9, 3, 5, 7, generator=g) * 2 - 1).cuda()
    m = mdm.SetMoments(105)
    assert m.update(x) is m and m.n == 9 and m.sum.is_cuda and m.outer.dtype == torch.float64
    s, o = _kernel_call(x.view(9, 105), 105)
    assert np.array_equal(_bits(m.sum), _bits(s)) and np.array_equal(_bits(m.outer), _bits(o))
    # carried: a second batch, and rows [R, ld > d] of which the first d count
    y = (torch.rand(6, 120, generator=g) * 2 - 1).cuda()
    y[:, 105:] = float("nan")
    m.update(y)
    s, o = _kernel_call(y, 105, (s, o))
    assert m.n == 15 and np.array_equal(_bits(m.sum), _bits(s)) and np.array_equal(_bits(m.outer), _bits(o))
    assert _inside(m, np.concatenate([x.view(9, 105).cpu().numpy(), y[:, :105].cpu().numpy()]), [9, 6])
    # "cuda" names the current GPU; totals given with n = 0 are carried, not overwritten
    named = mdm.SetMoments(105, "cuda").update(x)
    assert named.device == x.device and np.array_equal(_bits(named.outer), _bits(_kernel_call(x.view(9, 105), 105)[1]))
    given = mdm.SetMoments.from_arrays(0, np.ones(105), np.eye(105), device="cuda").update(x)
    plain = mdm.SetMoments(105).update(x)
    assert given.n == 9 and torch.equal(given.sum, 1.0 + plain.sum) and torch.equal(given.outer, torch.eye(105, dtype=torch.float64, device="cuda") + plain.outer)
    with pytest.raises(ValueError, match="rows"):
        m.update(x.cpu())
    with pytest.raises(TypeError, match="rows"):
        m.update(x.double())
    assert m.n == 15


def test_update_dataset_reads_a_uint8_set_in_place():
    import mdm
    g = np.random.default_rng(2)
    data = g.integers(0, 256, size=(50, 3, 5, 5)).astype(np.uint8)
    exact = (torch.arange(256, dtype=torch.float32) - 128) / 128
    ds = mdm.DeviceDataset(data, random=torch.zeros(50, 1), lut=exact)
    a = mdm.SetMoments(75).update_dataset(ds, chunk=16)                        # 16, 16, 16, 2 images with carry
    rows = ds.tensor().view(50, 75)
    b = mdm.SetMoments(75)
    for first in range(0, 50, 16):
        b.update(rows[first:first + 16])
    assert a.n == 50 and _same(a, b)
    ints = data.reshape(50, 75).astype(np.int64) - 128                        # and both are the int64 statement: the table is exact
    want_s, want_o = MM.grid_moments(ints)
    assert np.array_equal(a.sum.cpu().numpy(), want_s) and np.array_equal(a.outer.cpu().numpy(), want_o)
    assert _same(mdm.SetMoments(75).update_dataset(ds), mdm.SetMoments(75).update(rows))          # one chunk
    # the default table (0 -> -1, 255 -> 1) is not exact: inside the bound
    dflt = mdm.DeviceDataset(data, random=torch.zeros(50, 1))
    c = mdm.SetMoments(75).update_dataset(dflt, chunk=16)
    assert _inside(c, dflt.lut_host.numpy()[data.reshape(50, 75)], [16, 16, 16, 2])
    # an fp32 set is read in place too
    f = mdm.DeviceDataset(rows.view(50, 3, 5, 5).cpu(), random=torch.zeros(50, 1))
    assert _same(mdm.SetMoments(75).update_dataset(f, chunk=16), a)
    with pytest.raises(ValueError, match="dataset"):
        mdm.SetMoments(74).update_dataset(ds)


@pytest.fixture(scope="module")
def image_set():
    import mdm
    imgs = smooth_images(40, torch.Generator().manual_seed(31)).contiguous()
    u8 = ((imgs.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8)
    return mdm.DeviceDataset(u8, random=torch.zeros(40, 1))


def test_bank_moments_are_the_fold_of_its_rows_cached_or_not(image_set):
    import mdm
    cached = mdm.NeighborBank(image_set, size=8, chunk=16)
    stream = mdm.NeighborBank(image_set, size=8, chunk=16, cache_bytes=0)
    assert cached.cached and not stream.cached and cached.D == 192
    m = cached.moments()
    assert m is cached.moments() and m.n == 40 and m.d == 192                  # made once
    want = mdm.SetMoments(192)
    for first in range(0, 40, 16):
        want.update(cached.rows[first:first + 16])
    assert _same(m, want) and _same(stream.moments(), want)
    assert _inside(m, cached.rows[:, :192].cpu().numpy(), [16, 16, 8])
    tr = float(torch.diagonal(m.outer).sum())                                   # unit rows: the trace of outer is the number of rows
    assert abs(tr - 40) < 1e-4


def test_source_moments_applies_the_banks_own_map(image_set):
    import mdm
    bank = mdm.NeighborBank(image_set, size=8, chunk=16)
    data = image_set.tensor()
    got = bank.source_moments(data)
    assert got.n == 40 and _inside(got, bank.rows[:, :192].cpu().numpy(), [40])      # a source equal to the data: the data's moments
    raw = mdm.SetMoments(192).update(bank.source_rows(data)[0][:40])           # upstream's un-normalised source rows are another set
    assert not _inside(raw, bank.rows[:, :192].cpu().numpy(), [40])
    twice = bank.source_moments(data[:10], into=got)                           # `into` carries
    assert twice is got and got.n == 50
    with pytest.raises(ValueError, match="source"):
        bank.source_moments(data[:, :2])
    with pytest.raises(ValueError, match="into"):
        bank.source_moments(data, into=mdm.SetMoments(191))


def test_frechet_of_device_objects_is_frechet_of_their_host_copies(image_set):
    import mdm
    g = torch.Generator().manual_seed(4)
    a = mdm.SetMoments(75).update((torch.rand(200, 75, generator=g) * 2 - 1).cuda())
    b = mdm.SetMoments(75).update((torch.randn(90, 75, generator=g) * 0.5 + 0.1).cuda())
    host = [mdm.SetMoments.from_arrays(m.n, m.sum.cpu().numpy(), m.outer.cpu().numpy()) for m in (a, b)]
    r, h = mdm.frechet_distance(a, b), mdm.frechet_distance(*host)
    assert isinstance(r, mdm.FrechetResult) and r == h and (r.n_a, r.n_b, r.d, r.rank_deficient) == (200, 90, 75, False)
    assert r.distance > 0 and mdm.frechet_distance(a, mdm.SetMoments(75).update((torch.rand(60, 75, generator=g)).cuda())).rank_deficient


def _trained_model(n):
    import mdm
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_tiny.npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    return mdm.UNet(TINY, N=n, H=HW, W=HW, dtype=mdm.F32, params=params).eval()


def _setup(dataset):
    import mdm
    a = base_args(data_size=HW, ddpm_schedule="linear", ddpm_num_steps=T, shift_type="noise_with_perturbation",
                  sampling_mask_dependency="dependent_prev", momentum_adaptive="base_sampling", sample_num=N, sample_latent_shape="uniform",
                  sample_history=False, rng_mode="device", seed=11)
    s = mdm.Scheduler(a)
    s.update_ddpm_num_steps(T)
    return s, mdm.Sampler(dataset, a, s, [None] * 3), s.get_timesteps_epoch(0, 1)


def test_evaluate_frechet_is_the_fold_of_explicit_sample_calls(image_set, monkeypatch):
    import mdm
    model = _trained_model(N)
    s, smp, ts = _setup(image_set)
    assert len(ts) == T
    seed_all(21)
    host0, dev0 = torch.get_rng_state(), s.dev_rng.dev.clone()
    want = mdm.SetMoments(3 * HW * HW)
    batches = []
    for _ in range(2):
        x0, _ = smp.sample(model, ts)
        want.update(x0)
        batches.append(x0.clone())
    torch.cuda.synchronize()
    host1, dev1 = torch.get_rng_state(), s.dev_rng.dev.clone()
    assert not torch.equal(host0, host1) and not torch.equal(batches[0], batches[1])
    # pixels, default reference: the data set's moments, read in place once and kept on the data set object
    torch.set_rng_state(host0)
    s.dev_rng.dev.copy_(dev0)
    assert getattr(image_set, "_set_moments", None) is None
    res = smp.evaluate_frechet(model, ts, rounds=2)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), host1) and torch.equal(s.dev_rng.dev, dev1)      # left where two sample calls leave them
    ref = image_set._set_moments
    assert _same(ref, mdm.SetMoments(3 * HW * HW).update_dataset(image_set)) and ref.n == 40
    assert isinstance(res, mdm.FrechetResult) and res == mdm.frechet_distance(want, ref)
    assert (res.n_a, res.n_b, res.d, res.rank_deficient) == (2 * N, 40, 3 * HW * HW, True) and np.isfinite(res.distance)
    # an explicit reference; the default one is not computed again
    torch.set_rng_state(host0)
    s.dev_rng.dev.copy_(dev0)
    again = smp.evaluate_frechet(model, ts, rounds=2, reference=mdm.SetMoments.from_arrays(ref.n, ref.sum.cpu().numpy(), ref.outer.cpu().numpy()))
    assert again == res and image_set._set_moments is ref
    # features="bank": both sides are rows of the 32 x 32 bank; the host eigh pair at d = 3072 is not run here, the two sets are taken
    seen = {}
    monkeypatch.setattr(mdm.moments, "frechet_distance", lambda a, b: seen.update(a=a, b=b) or "result")
    torch.set_rng_state(host0)
    s.dev_rng.dev.copy_(dev0)
    assert smp.evaluate_frechet(model, ts, rounds=2, features="bank") == "result"
    bank = smp._nn_bank
    assert seen["b"] is bank.moments() and bank.size == 32 and seen["b"].n == 40 and seen["a"].d == 3072
    rows64 = bank.rows[:, :3072].double()                                      # 40 rows in one split of three blocks: against torch's fp64 product
    ref, mag = rows64.T @ rows64, rows64.abs().T @ rows64.abs()
    assert bool(((seen["b"].outer - ref).abs() <= 2 * MM.gamma(40 + 1) * mag).all()) and torch.equal(seen["b"].outer, seen["b"].outer.T)
    folded = bank.source_moments(batches[1], into=bank.source_moments(batches[0]))
    assert _same(seen["a"], folded) and torch.equal(torch.get_rng_state(), host1) and torch.equal(s.dev_rng.dev, dev1)
    for kw, err, word in ((dict(features="inception"), ValueError, "features"), (dict(rounds=0), ValueError, "rounds"),
                          (dict(reference=np.zeros(3)), TypeError, "reference")):
        with pytest.raises(err, match=word):
            smp.evaluate_frechet(model, ts, **kw)
    assert torch.equal(torch.get_rng_state(), host1)                           # refused before any draw
