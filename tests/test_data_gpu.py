"""The device-resident data set on the GPU (include/mdm_data.h, mdm/data.py): mdm_data_gather and mdm_data_means against torch indexing
and fp64 means on the CPU, `DeviceLoader` against a host `torch.utils.data.DataLoader` batch for batch, `data_mean_histogram` over a
`DeviceDataset` against its host path, and a `Trainer` fed by a `DeviceLoader` against one fed by the host loader, bit for bit.
Every case is a few tiny launches."""
import math

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from golden.make_golden import TINY, base_args, seed_all
from mdm import _lib
from mdm import data as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_F, SENTINEL_U = 777.0, 255            # what the gaps between strided images hold; the data never holds it


def _gather(src, kind, stride, M, C, H, W, lut, index, first, N, flip, x0, label=None, random=None, R=0, label_out=None, random_out=None):
    p = _lib.ptr
    _lib.call("mdm_data_gather", p(src), kind, stride, M, C, H, W, p(lut), p(index), first, N, p(flip), p(x0), p(label), p(random), R,
              p(label_out), p(random_out), _lib.stream())


def _means(src, kind, stride, M, C, H, W, lut, per_channel, out):
    p = _lib.ptr
    _lib.call("mdm_data_means", p(src), kind, stride, M, C, H, W, p(lut), int(per_channel), p(out), _lib.stream())


def _images(kind, M, C, H, W, seed):
    """-> (stored images on the host, their fp32 values on the host, the table or None)"""
    g = torch.Generator().manual_seed(seed)
    if kind == 0:
        x = torch.randn(M, C, H, W, generator=g)
        return x, x, None
    u = torch.randint(0, 200, (M, C, H, W), generator=g, dtype=torch.uint8)
    lut = D.normalize_lut()
    return u, lut[u.long()], lut


def _stored(img, stride, off):
    """The images on the device at `stride` elements from one another behind `off` leading elements, every gap holding the sentinel
    -> (the buffer, the view that starts at image 0)"""
    M, E = img.shape[0], img[0].numel()
    sent = SENTINEL_U if img.dtype == torch.uint8 else SENTINEL_F
    buf = torch.full((off + M * stride + 3,), sent, dtype=img.dtype)
    buf[off:off + M * stride].view(M, stride)[:, :E] = img.reshape(M, E)
    buf = buf.to(DEV)
    return buf, buf[off:]


# ------------------------------------------------------------------ gather, exact
GATHER_SHAPES = [(7, 3, 5, 7, 4), (3, 1, 1, 1, 5), (9, 4, 8, 8, 9), (5, 3, 32, 32, 32)]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("M,C,H,W,N", GATHER_SHAPES)
def test_gather_is_indexing(kind, M, C, H, W, N):
    """x0 = values[index[first : first + N]] bit for bit, for a packed and a padded layout, every pointer alignment, inside a larger
    NaN buffer whose margins stay NaN; labels and `random` rows with it"""
    E = C * H * W
    img, val, lut = _images(kind, M, C, H, W, seed=M)
    lut_d = None if lut is None else lut.to(DEV)
    g = torch.Generator().manual_seed(100 + M)
    idx = torch.randint(0, M, (N,), generator=g)                   # N > M or N close to M: with repeats
    if N >= M:
        assert len(set(idx.tolist())) < N
    first = 3
    index = torch.cat([torch.full((first,), M + 5), idx, torch.full((2,), -7)]).to(torch.int64).to(DEV)
    label = torch.randn(M, generator=g)
    want = val[idx]
    assert not bool((want == (SENTINEL_F if kind == 0 else float(D.normalize_lut()[SENTINEL_U]))).any())
    margin = 8
    for stride in (E, E + 5):
        for s_off in ((0, 1) if kind == 0 else (0, 1, 2, 3)):
            buf, src = _stored(img, stride, s_off)
            for x_off in (0, 1):
                for R in (1, 3):
                    rnd = torch.randn(M, R, generator=g)
                    out = torch.full((margin + x_off + N * E + margin,), float("nan"), device=DEV)
                    x0 = out[margin + x_off:margin + x_off + N * E]
                    lo, ro = torch.full((N + 2,), float("nan"), device=DEV), torch.full((N * R + 2,), float("nan"), device=DEV)
                    _gather(src, kind, stride, M, C, H, W, lut_d, index, first, N, None, x0, label.to(DEV), rnd.to(DEV), R, lo, ro)
                    where = (stride, s_off, x_off, R)
                    assert torch.equal(x0.cpu().view(N, C, H, W), want), where
                    head, tail = out[:margin + x_off].cpu(), out[margin + x_off + N * E:].cpu()
                    assert bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all()), where
                    assert torch.equal(lo[:N].cpu(), label[idx]) and bool(torch.isnan(lo[N:]).all()), where
                    assert torch.equal(ro[:N * R].cpu().view(N, R), rnd[idx]) and bool(torch.isnan(ro[N * R:]).all()), where
    # without the optional outputs, onto an aligned buffer
    buf, src = _stored(img, E, 0)
    x0 = torch.empty(N, C, H, W, device=DEV)
    _gather(src, kind, E, M, C, H, W, lut_d, index, first, N, None, x0)
    assert torch.equal(x0.cpu(), want)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("W", [1, 7, 32])
def test_gather_mirrors_along_w(kind, W):
    M, C, H, N = 4, 2, 3, 6
    E = C * H * W
    img, val, lut = _images(kind, M, C, H, W, seed=W)
    lut_d = None if lut is None else lut.to(DEV)
    idx = torch.tensor([0, 3, 3, 1, 2, 0])
    flags = torch.tensor([1, 0, 7, 0, 1, 255], dtype=torch.uint8)
    want = torch.stack([torch.flip(val[i], dims=[2]) if f else val[i] for i, f in zip(idx.tolist(), flags.tolist())])
    for s_off in (0, 1):
        buf, src = _stored(img, E, s_off)
        for x_off in (0, 1):
            out = torch.full((4 + x_off + N * E + 4,), float("nan"), device=DEV)
            x0 = out[4 + x_off:4 + x_off + N * E]
            _gather(src, kind, E, M, C, H, W, lut_d, idx.to(DEV), 0, N, flags.to(DEV), x0)
            assert torch.equal(x0.cpu().view(N, C, H, W), want), (s_off, x_off)
            assert bool(torch.isnan(out[:4 + x_off]).all()) and bool(torch.isnan(out[4 + x_off + N * E:]).all())


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("C,H,W", [(3, 5, 7), (3, 8, 8)])
def test_a_bad_index_is_a_nan_row_and_reads_nothing(kind, C, H, W):
    M, R = 6, 2
    img, val, lut = _images(kind, M, C, H, W, seed=9)
    lut_d = None if lut is None else lut.to(DEV)
    idx = torch.tensor([1, -1, 0, M, 2 ** 40, 5, -2 ** 40])
    N = len(idx)
    bad = torch.tensor([False, True, False, True, True, False, True])
    g = torch.Generator().manual_seed(4)
    label, rnd = torch.randn(M, generator=g), torch.randn(M, R, generator=g)
    flags = torch.tensor([0, 1, 1, 0, 1, 0, 0], dtype=torch.uint8)
    for flip in (None, flags):
        buf, src = _stored(img, C * H * W, 0)
        x0, lo, ro = torch.zeros(N, C, H, W, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, R, device=DEV)
        _gather(src, kind, C * H * W, M, C, H, W, lut_d, idx.to(DEV), 0, N, None if flip is None else flip.to(DEV), x0, label.to(DEV),
                rnd.to(DEV), R, lo, ro)
        x0, lo, ro = x0.cpu(), lo.cpu(), ro.cpu()
        assert bool(torch.isnan(x0[bad]).all()) and bool(torch.isnan(lo[bad]).all()) and bool(torch.isnan(ro[bad]).all())
        good = idx[~bad]
        want = val[good] if flip is None else torch.stack([torch.flip(val[i], dims=[2]) if f else val[i]
                                                           for i, f in zip(good.tolist(), flags[~bad].tolist())])
        assert torch.equal(x0[~bad], want) and torch.equal(lo[~bad], label[good]) and torch.equal(ro[~bad], rnd[good])


def test_gather_past_two_to_the_31():
    """uint8, 700 000 images of 3 x 32 x 32: image 699 051 starts just past byte 2^31.  The buffer is left uninitialised but for
    the three rows that are read."""
    M, C, H, W = 700_000, 3, 32, 32
    rows = [0, 699_051, 699_999]
    assert (rows[1] - 1) * C * H * W < 2 ** 31 < rows[1] * C * H * W + 4096
    src = torch.empty(M, C, H, W, dtype=torch.uint8, device=DEV)
    u = torch.randint(0, 256, (3, C, H, W), generator=torch.Generator().manual_seed(31), dtype=torch.uint8)
    for k, r in enumerate(rows):
        src[r] = u[k].to(DEV)
    lut = D.normalize_lut()
    x0 = torch.empty(3, C, H, W, device=DEV)
    _gather(src, 1, C * H * W, M, C, H, W, lut.to(DEV), torch.tensor(rows, dtype=torch.int64, device=DEV), 0, 3, None, x0)
    assert torch.equal(x0.cpu(), lut[u.long()])
    out = torch.empty(1, 3, device=DEV)
    _means(src[rows[1]:], 1, C * H * W, 1, C, H, W, lut.to(DEV), 1, out)
    ref = lut[u[1].long()].double().mean(dim=[1, 2])
    assert float((out.cpu()[0].double() - ref).abs().max()) <= 2.0 ** -23
    del src


# ------------------------------------------------------------------ means
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("per_channel", [0, 1])
@pytest.mark.parametrize("M,C,H,W", [(5, 3, 5, 7), (2, 1, 1, 1), (3, 3, 64, 64)])
def test_means_within_one_rounding_of_fp64(kind, per_channel, M, C, H, W):
    """|got - ref| <= 2^-24 |ref| + E 2^-52 mean|x|: one rounding to fp32 of an fp64 sum of E terms taken in any order; two runs
    give the same bits"""
    E = C * H * W
    img, val, lut = _images(kind, M, C, H, W, seed=17 + M)
    lut_d = None if lut is None else lut.to(DEV)
    v64 = val.double()
    if per_channel:
        ref, mabs, terms = v64.mean(dim=[2, 3]), v64.abs().mean(dim=[2, 3]), H * W
    else:
        ref, mabs, terms = v64.mean(dim=[1, 2, 3]).unsqueeze(-1), v64.abs().mean(dim=[1, 2, 3]).unsqueeze(-1), E
    bound = 2.0 ** -24 * ref.abs() + terms * 2.0 ** -52 * mabs
    for stride, s_off in ((E, 0), (E, 1), (E + 5, 0), (E + 5, 3 if kind else 1)):
        buf, src = _stored(img, stride, s_off)
        outs = []
        for _ in range(2):
            out = torch.full((M * (C if per_channel else 1) + 2,), float("nan"), device=DEV)
            _means(src, kind, stride, M, C, H, W, lut_d, per_channel, out)
            outs.append(out.cpu())
        assert torch.equal(outs[0][:-2], outs[1][:-2]) and bool(torch.isnan(outs[0][-2:]).all())
        got = outs[0][:-2].view(M, -1).double()
        err = (got - ref).abs()
        print(f"means kind {kind} per_channel {per_channel} {(M, C, H, W)} stride {stride} off {s_off}: "
              f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (stride, s_off, float((err - bound).max()))


# ------------------------------------------------------------------ DeviceDataset, histogram
def _const_images(M):
    """3 x 8 x 8 images constant per channel, values k / 64 with the three k of an image k0 - d, k0, k0 + d: the channel means and the
    image mean k0 / 64 are exact in fp32 and fp64 whatever the order of the sum -> (k as uint8 [M, 3, 8, 8])"""
    g = torch.Generator().manual_seed(64)
    k0 = torch.randint(40, 200, (M,), generator=g)
    d = torch.randint(0, 40, (M,), generator=g)
    k = torch.stack([k0 - d, k0, k0 + d], dim=1)
    return k.to(torch.uint8)[:, :, None, None].expand(M, 3, 8, 8).contiguous()


@pytest.mark.parametrize("storage", ["f32", "u8"])
@pytest.mark.parametrize("area", ["image-wise", "channel-wise"])
def test_histogram_over_a_device_dataset_is_the_host_paths(storage, area):
    from mdm import evaluate
    k = _const_images(37)
    table = torch.arange(256, dtype=torch.float32) / 64
    host = table[k.long()]
    ds = D.DeviceDataset(host, device=DEV) if storage == "f32" else D.DeviceDataset(k, lut=table, device=DEV)
    a = base_args(sample_latent_shape="data", mean_area=area, sample_num=4)
    want, got = evaluate.data_mean_histogram(host, a), evaluate.data_mean_histogram(ds, a)
    assert tuple(got[0]) == tuple(want[0]) == ((4,) if area == "image-wise" else (4, 4, 4))
    assert len(got[1]) == len(want[1]) and all(torch.equal(x, y) for x, y in zip(got[1], want[1]))
    assert torch.equal(got[2], want[2]) and got[2].device.type == "cpu"
    means = ds.means(per_channel=area == "channel-wise").cpu()
    assert torch.equal(means, host.mean(dim=[2, 3]) if area == "channel-wise" else host.mean(dim=[1, 2, 3]).unsqueeze(-1))
    a.sample_latent_shape = "zero"
    assert evaluate.data_mean_histogram(ds, a) == [None, None, None]


def test_the_data_set_reads_back_what_it_stores():
    u = torch.randint(0, 256, (6, 3, 4, 5), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    lut = D.normalize_lut()
    for stored, val in ((u, lut[u.long()]), (lut[u.long()], lut[u.long()])):
        ds = D.DeviceDataset(stored, torch.arange(6.0), num_timesteps=3, device=DEV)
        t = ds.tensor()
        assert t.is_cuda and t.dtype == torch.float32 and torch.equal(t.cpu(), val)
        x, l, r = ds[4]
        assert not x.is_cuda and torch.equal(x, val[4]) and float(l) == 4.0 and torch.equal(r, ds.random[4].cpu())
        from mdm import evaluate
        assert torch.equal(evaluate._dataset_tensor(ds), val)


# ------------------------------------------------------------------ DeviceLoader
@pytest.mark.parametrize("storage", ["f32", "u8"])
def test_loader_yields_the_host_dataloaders_batches(storage):
    M, B = 50, 8
    g = torch.Generator().manual_seed(50)
    u = torch.randint(0, 256, (M, 3, 8, 8), generator=g, dtype=torch.uint8)
    val = D.normalize_lut()[u.long()] if storage == "u8" else torch.randn(M, 3, 8, 8, generator=g)
    label, rnd = torch.arange(float(M)), torch.rand(M, 2, generator=g) * 2 - 1
    ds = D.DeviceDataset(u if storage == "u8" else val, label, rnd, device=DEV)
    host = DataLoader(TensorDataset(val, label, rnd), batch_size=B, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(6))
    ours = D.DeviceLoader(ds, B, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(6))
    assert len(ours) == len(host) == 6
    for epoch in range(2):
        n = 0
        for got, want in zip(ours, host, strict=True):
            assert all(t.is_cuda for t in got) and got[0] is ours.x0
            assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want, strict=True)), (epoch, n)
            n += 1
        assert n == 6
    assert torch.equal(ours.generator.get_state(), host.generator.get_state())
    # the last, short batch of drop_last=False and the natural order
    host = DataLoader(TensorDataset(val, label, rnd), batch_size=B, shuffle=False, drop_last=False)
    ours = D.DeviceLoader(ds, B, shuffle=False, drop_last=False)
    got = [tuple(t.cpu().clone() for t in b) for b in ours]
    assert len(got) == len(ours) == len(host) == 7 and got[-1][0].shape[0] == 2
    assert all(torch.equal(a, b) for g_, w in zip(got, host, strict=True) for a, b in zip(g_, w, strict=True))
    # a bound buffer is what is yielded
    buf = torch.zeros(B, 3, 8, 8, device=DEV)
    ours = D.DeviceLoader(ds, B, shuffle=False).bind(buf)
    b = next(iter(ours))
    assert b[0] is buf and torch.equal(buf.cpu(), val[:B])
    with pytest.raises(ValueError):
        ours.bind(torch.zeros(B, 3, 8, 8))                                # not on the device


def test_loader_hflip_draws_like_random_horizontal_flip():
    M, B = 12, 4
    val = torch.randn(M, 3, 4, 6, generator=torch.Generator().manual_seed(12))
    ds = D.DeviceDataset(val, device=DEV)
    ours = D.DeviceLoader(ds, B, shuffle=True, generator=torch.Generator().manual_seed(1), hflip=0.5)
    order = D.DeviceLoader(ds, B, shuffle=True, generator=torch.Generator().manual_seed(1)).epoch_indices()
    torch.manual_seed(33)
    got = [b[0].cpu().clone() for b in ours]
    state = torch.get_rng_state()
    torch.manual_seed(33)
    flags = [[bool(torch.rand(1) < 0.5) for _ in b] for b in order]       # one draw per image, batch by batch
    assert torch.equal(torch.get_rng_state(), state) and any(f for fs in flags for f in fs) and not all(f for fs in flags for f in fs)
    for x, b, fs in zip(got, order, flags, strict=True):
        assert torch.equal(x, torch.stack([torch.flip(val[i], dims=[2]) if f else val[i] for i, f in zip(b, fs)]))
    every = next(iter(D.DeviceLoader(ds, B, shuffle=False, hflip=1.0)))[0].cpu()
    assert torch.equal(every, torch.flip(val[:B], dims=[3]))


# ------------------------------------------------------------------ Trainer
def _trainer(a, loader, accum):
    import mdm
    from oracle.unet_ref import random_params
    model = mdm.UNet(TINY, N=4, H=32, W=32, dtype=mdm.F32, params=random_params(TINY))
    opt = mdm.AdamW(model, lr=1e-3)
    acc = mdm.Accelerator(gradient_accumulation_steps=accum)
    tr = mdm.Trainer(a, acc.prepare(loader), None, [None] * 3, model, None, opt, mdm.get_lr_scheduler("constant", opt, 0, 10), acc)
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(a.ddpm_num_steps)
    return tr, model


@pytest.fixture(scope="module")
def train_set():
    g = torch.Generator().manual_seed(14)
    x = torch.rand(14, 3, 32, 32, generator=g) * 2 - 1                    # 14 images, batch 4, drop_last: 3 batches an epoch
    return x, torch.arange(14.0), torch.rand(14, 1, generator=g) * 2 - 1


@pytest.mark.parametrize("variant", ["device_rng", "accumulate", "replay", "monitor_defer"])
def test_trainer_on_a_device_loader_is_the_trainer_on_the_host_loader(train_set, variant):
    """fp32 is bit-reproducible: two epochs of three batches give the same losses and the same weights whichever loader feeds them"""
    x, label, rnd = train_set
    kw = dict(data_size=32, ddpm_schedule="linear", ddpm_num_steps=10, shift_type="noise_with_perturbation", batch_size=4, seed=3)
    if variant != "replay":
        kw["rng_mode"] = "device"
    if variant == "monitor_defer":
        kw.update(monitor=True, defer_loss=True)
    accum = 2 if variant == "accumulate" else 1
    kw["gradient_accumulation_steps"] = accum
    runs = []
    for which in ("host", "device"):
        gen = torch.Generator().manual_seed(77)
        if which == "host":
            loader = DataLoader(TensorDataset(x, label, rnd), batch_size=4, shuffle=True, drop_last=True, generator=gen)
        else:
            loader = D.DeviceLoader(D.DeviceDataset(x, label, rnd, device=DEV), 4, shuffle=True, drop_last=True, generator=gen)
        tr, model = _trainer(base_args(**kw), loader, accum)
        assert len(loader) == 3
        if which == "device":
            assert loader.x0 is tr.step.x0
        seed_all(21)
        losses = []
        for epoch in range(2):
            losses += tr._run_epoch(epoch, 2, 0, None, None)
        assert len(losses) == 6 and all(isinstance(v, float) and math.isfinite(v) for v in losses)
        runs.append((losses, model.store.P.clone(), tr.global_step, torch.get_rng_state()))
        if which == "device":
            b = next(iter(loader))
            assert b[0] is tr.step.x0 and b[0].data_ptr() == tr.step.x0.data_ptr()
    (l0, p0, s0, r0), (l1, p1, s1, r1) = runs
    print(f"{variant}: host losses {l0}\n{variant}: device losses {l1}")
    assert l0 == l1 and len(set(l0)) == 6
    assert torch.equal(p0, p1) and s0 == s1 == (4 if accum == 2 else 6) and torch.equal(r0, r1)


def test_trainer_refuses_a_loader_of_another_batch_size(train_set):
    x, label, rnd = train_set
    loader = D.DeviceLoader(D.DeviceDataset(x, label, rnd, device=DEV), 2)
    with pytest.raises(ValueError, match="batch"):
        _trainer(base_args(data_size=32, batch_size=4, rng_mode="device", seed=3), loader, 1)
