"""MNIST / CIFAR-10 / Flowers102 from local files into the device data set, and one channel through every layer.

`ingest_block` and `get_dataset` byte for byte against the installed PIL (`Image.fromarray` in mode L or RGB, `Resize(size)` +
`CenterCrop(size)` through tests/_ingest_ref.py): exact integer arithmetic, 0 differing bytes.  Then the train step of upstream's
mnist preset -- `unet6_config(32, in_channels=1, out_channels=1)`, ddpm_num_steps 64, Adam at lr 1e-4 -- fed by a `DeviceLoader`
over the synthetic MNIST set through `Trainer`, against `oracle.trainer_ref.train_step_ref` on the CPU with the same batches and
host draws, and a one-channel reverse sampler as one graph per step.  Every file is written into a temporary directory
(tests/_rawsets_files.py)."""
import numpy as np
import pytest
import torch

import _ingest_ref as R
import _rawsets_files as F
from mdm import data as D
from mdm import ingest as I

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from golden.make_golden import base_args, seed_all  # noqa: E402


def _chw(img, size):
    """What PIL makes of one decoded image ([h][w] or [h][w][3] uint8) under Resize(size) + CenterCrop(size) -> [C][size][size]"""
    return R.pil_resize_crop(img[:, :, None] if img.ndim == 2 else img, size)


def _to_tensor_normalize(u8):
    """torchvision's ToTensor() + Normalize([0.5], [0.5]) of a uint8 array, as they compute it"""
    return (torch.from_numpy(np.ascontiguousarray(u8)).float().div(255) - 0.5) / 0.5


# ------------------------------------------------------------------ ingest_block
def _block(name):
    rng = np.random.RandomState({"grey28": 21, "grey5x9": 22, "rgb32": 23}[name])
    if name == "grey28":
        return rng.randint(0, 256, size=(7, 28, 28)).astype(np.uint8)
    if name == "grey5x9":
        return rng.randint(0, 256, size=(7, 5, 9)).astype(np.uint8)
    planar = rng.randint(0, 256, size=(5, 3072)).astype(np.uint8)              # CIFAR's layout: the block is a strided view of it
    return planar.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)


@pytest.mark.parametrize("three_per_chunk", [False, True], ids=["default_chunk", "three_per_chunk"])
@pytest.mark.parametrize("name,size", [("grey28", 32), ("grey28", 28), ("grey28", 16), ("grey5x9", 4), ("rgb32", 32), ("rgb32", 16)])
def test_ingest_block_equals_pil_byte_for_byte(name, size, three_per_chunk, monkeypatch):
    block = _block(name)
    K, h, w = block.shape[:3]
    C = 1 if block.ndim == 3 else 3
    launches = []
    launch = I.resize_crop
    monkeypatch.setattr(I, "resize_crop", lambda src, k, *a, **kw: (launches.append(int(k)), launch(src, k, *a, **kw))[1])
    kw = dict(chunk_bytes=3 * h * w * C) if three_per_chunk else {}
    got = I.ingest_block(block, size, device=DEV, **kw)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (K, C, size, size)
    assert launches == ([3] * (K // 3) + [K % 3] if three_per_chunk else [K])     # 7 images: 3 + 3 + 1, three launches
    want = np.stack([_chw(block[k], size) for k in range(K)])
    differing = int((got.cpu().numpy() != want).sum())
    print(f"{name} at {size}: {differing} bytes differ from PIL")
    assert differing == 0
    if size == h == w:                                                            # PIL returns a copy there: the source, planar
        assert np.array_equal(got.cpu().numpy(), block.reshape(K, h, w, C).transpose(0, 3, 1, 2))
    assert torch.equal(got, I.ingest_arrays([block[k] for k in range(K)], size, C=C, device=DEV))
    assert torch.equal(got, I.ingest_block(block, size, device=DEV, **kw))        # the same call twice: the same bits
    if name == "grey5x9":
        assert R.resize_crop_plan(h, w, size)[2:] != (0, 0)                       # the crop offsets are live


# ------------------------------------------------------------------ get_dataset
def _check_dataset(path, name, size, images, labels):
    """`images`: the decoded images of split 'all' in upstream's order, as PIL sees them"""
    M, T = len(images), 5
    want = np.stack([_chw(im, size) for im in images])
    C = want.shape[1]
    torch.manual_seed(31)
    ds = I.get_dataset(str(path), name, size, "all", num_timesteps=T, device=DEV)
    state = torch.get_rng_state()
    torch.manual_seed(31)
    rnd = torch.FloatTensor(M, T).uniform_(-1.0, 1.0)                            # drawn first, where upstream draws it; nothing else is
    assert torch.equal(torch.get_rng_state(), state)
    assert isinstance(ds, D.DeviceDataset) and len(ds) == M and (ds.M, ds.C, ds.H, ds.W, ds.R) == (M, C, size, size, T)
    assert ds.data.dtype == torch.uint8 and ds.data.is_cuda and torch.equal(ds.lut_host, D.normalize_lut())
    differing = int((ds.data.cpu().numpy() != want).sum())
    print(f"{name} at {size}: {differing} bytes differ from PIL")
    assert differing == 0
    assert ds.label.dtype == torch.float32 and ds.label.cpu().tolist() == [float(l) for l in labels]
    assert torch.equal(ds.random.cpu(), rnd)
    x_all = _to_tensor_normalize(want)
    for i in range(M):
        x, l, r = ds[i]
        assert x.dtype == torch.float32 and torch.equal(x, x_all[i]) and float(l) == float(labels[i]) and torch.equal(r, rnd[i])
    torch.manual_seed(32)
    sub = I.get_dataset(str(path), name.upper(), size, "all", True, 4, num_timesteps=T, device=DEV)
    torch.manual_seed(32)
    assert len(sub) == 4 and int((sub.data.cpu().numpy() != want[:4]).sum()) == 0
    assert sub.label.cpu().tolist() == [float(l) for l in labels[:4]] and torch.equal(sub.random.cpu(), torch.FloatTensor(4, T).uniform_(-1.0, 1.0))
    order = D.DeviceLoader(ds, 4, shuffle=True, generator=torch.Generator().manual_seed(33)).epoch_indices()
    x, l, r = next(iter(D.DeviceLoader(ds, 4, shuffle=True, generator=torch.Generator().manual_seed(33))))
    assert sorted(order[0]) != order[0] or sorted(order[-1]) != order[-1]
    assert torch.equal(x.cpu(), x_all[order[0]]) and l.cpu().tolist() == [float(labels[i]) for i in order[0]] and torch.equal(r.cpu(), rnd[order[0]])
    return ds


def test_get_dataset_mnist(tmp_path):
    want = F.make_mnist(tmp_path, seed=41)
    ds = _check_dataset(tmp_path, "mnist", 32, list(want["all"][0]), want["all"][1])
    assert ds.C == 1
    test = I.get_dataset(str(tmp_path), "MNIST", 32, "test", device=DEV)
    assert len(test) == 3 and torch.equal(test.data, ds.data[5:]) and torch.equal(test.label, ds.label[5:])
    same = I.get_dataset(str(tmp_path), "mnist", 28, "train", device=DEV)         # size == h == w: the source bytes
    assert np.array_equal(same.data.cpu().numpy()[:, 0], want["train"][0])


def test_get_dataset_cifar10(tmp_path):
    want = F.make_cifar10(tmp_path, seed=42, planes="random")
    ds = _check_dataset(tmp_path, "cifar10", 32, list(want["all"][0]), want["all"][1])
    assert ds.C == 3 and np.array_equal(ds.data.cpu().numpy(), want["all"][0].transpose(0, 3, 1, 2))
    train = I.get_dataset(str(tmp_path), "cifar10", 16, "train", device=DEV)
    assert len(train) == 10 and int((train.data.cpu().numpy() != np.stack([_chw(im, 16) for im in want["train"][0]])).sum()) == 0


def test_get_dataset_flowers102(tmp_path):
    from PIL import Image
    root, labels = F.make_flowers102(tmp_path, seed=43)
    ids = F.FLOWER_IDS["train"] + F.FLOWER_IDS["val"] + F.FLOWER_IDS["test"]
    images = [np.asarray(Image.open(f"{root}/jpg/image_{i:05d}.jpg").convert("RGB")) for i in ids]
    assert len({im.shape for im in images}) == 6
    ds = _check_dataset(tmp_path, "flowers102", 8, images, [int(labels[i - 1]) - 1 for i in ids])
    assert ds.C == 3
    val = I.get_dataset(str(tmp_path), "flowers102", 8, "val", device=DEV)
    assert len(val) == 1 and torch.equal(val.data, ds.data[2:3])


# ------------------------------------------------------------------ one channel through every layer
LR, STEPS = 1e-4, 64          # the mnist launch scripts: optim adam, lr 1e-4; ddpm_num_steps 64 with data_size 32


def _mnist_args(**kw):
    return base_args(data_size=32, in_channel=1, out_channel=1, ddpm_schedule="linear", ddpm_num_steps=STEPS, updated_ddpm_num_steps=STEPS,
                     select_degrade_pixel="thresholding", degrade_channel="1-channel", shift_type="noise_reduction", noise_mean=0.1,
                     batch_size=4, **kw)


@pytest.fixture(scope="module")
def mnist_step(tmp_path_factory):
    """The synthetic MNIST set on the device, its two shuffled batches of one epoch, and the oracle's two steps on them (CPU,
    fp32, computed once): loss and unclipped gradients of step 1, weights after step 2."""
    import mdm
    from oracle.scheduler_ref import SchedulerRef
    from oracle.trainer_ref import train_step_ref
    from oracle.unet_ref import UNetRef, random_params
    path = tmp_path_factory.mktemp("mnist")
    F.make_mnist(path, seed=51)
    torch.manual_seed(52)
    ds = I.get_dataset(str(path), "mnist", 32, "all", num_timesteps=STEPS, device=DEV)
    cfg = mdm.unet6_config(32, in_channels=1, out_channels=1)
    params = random_params(cfg)
    batches = [b[0].cpu().clone() for b in D.DeviceLoader(ds, 4, generator=torch.Generator().manual_seed(53))]
    assert len(batches) == 2 and tuple(batches[0].shape) == (4, 1, 32, 32)
    a = _mnist_args()
    rs = SchedulerRef(a)
    rs.update_ddpm_num_steps(STEPS)
    used = rs.get_timesteps_epoch(0, 1)
    ref = UNetRef(cfg, params)
    ropt = torch.optim.Adam(ref.parameters(), lr=LR)
    seed_all(500)
    r1 = train_step_ref(ref, ropt, rs, a, batches[0], used, rs.rng)
    sc = min(1.0, 1.0 / (float(r1["grad_norm"]) + 1e-6))                          # undo the in-place clip (make_golden.py)
    g1 = {k: (p.grad / sc).numpy().copy() for k, p in ref.pdict().items()}
    r2 = train_step_ref(ref, ropt, rs, a, batches[1], used, rs.rng)
    sc = min(1.0, 1.0 / (float(r2["grad_norm"]) + 1e-6))
    g2 = {k: (p.grad / sc).numpy().copy() for k, p in ref.pdict().items()}
    w2 = {k: p.detach().numpy().copy() for k, p in ref.pdict().items()}
    return dict(ds=ds, cfg=cfg, params=params, used=used, loss=(float(r1["loss"]), float(r2["loss"])), x_in=r1["x_in"], g1=g1, g2=g2, w2=w2,
                norm=float(r1["grad_norm"]))


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_one_channel_train_step_vs_the_oracle(mnist_step, dt):
    """Loss and every gradient tensor of step 1, the weights after step 2.  fp32: the bars of
    test_path_gpu.py::test_train_step_vs_reference -- per tensor rtol 3e-3, atol 3e-2 rms (rms over all gradients); the weights
    as their MOVE since the start under the same pair (rms over the oracle's moves), where both steps' oracle gradients are well
    conditioned (that test's rule: an Adam step has the size lr whatever |g| is, so an element below the noise moves by +-lr on
    rounding alone, on both sides).  bf16: that test's bf16 bars -- loss 3e-2, gradients 8e-2 rel-L2 over all tensors, and at most
    2 % of the well-conditioned weights further than 2.1 lr per step from the oracle's."""
    import mdm
    m = mnist_step
    a = _mnist_args()
    model = mdm.UNet(m["cfg"], N=4, H=32, W=32, dtype=dt, params=m["params"])
    assert (model.cin, model.cout, model.cin_p, model.cout_p) == (1, 1, 8, 8)
    opt = mdm.Adam(model, lr=LR)
    loader = D.DeviceLoader(m["ds"], 4, generator=torch.Generator().manual_seed(53))
    tr = mdm.Trainer(a, loader, m["ds"], [None] * 3, model, None, opt, mdm.get_lr_scheduler("constant", opt, 0, 10), mdm.Accelerator())
    assert loader.x0 is tr.step.x0 and tuple(tr.step.x0.shape) == (4, 1, 32, 32)
    a.updated_ddpm_num_steps = tr.Scheduler.update_ddpm_num_steps(STEPS)
    tr.timesteps_used_epoch = tr.Scheduler.get_timesteps_epoch(0, 1)
    assert tr.timesteps_used_epoch == m["used"]
    w0 = model.state_dict()
    it = iter(loader)
    batch = next(it)
    assert batch[0] is tr.step.x0
    seed_all(500)
    loss1 = tr._run_batch(0, batch, 0, 1, 0, None, None)
    x_in = tr.step.x_in.cpu()
    grads = model.store.grad_dict()
    gnorm = tr.optimizer.grad_norm()
    loss2 = tr._run_batch(1, next(it), 0, 1, 0, None, None)
    sd = model.state_dict()
    assert torch.equal(x_in, m["x_in"])                                           # the batch, the mask and the shift: bit for bit

    want = m["g1"]
    assert set(want) == set(grads) == set(sd)
    a_ = np.concatenate([grads[k].numpy().reshape(-1) for k in want])
    b_ = np.concatenate([want[k].reshape(-1) for k in want])
    grel = float(np.linalg.norm(a_ - b_) / np.linalg.norm(b_))
    rms = float(np.sqrt((b_ ** 2).mean()))
    print(f"dtype {dt}: loss {loss1:.7f} / {loss2:.7f}, oracle {m['loss'][0]:.7f} / {m['loss'][1]:.7f}; gradients rel-L2 {grel:.3e}; "
          f"norm {gnorm:.6f}, oracle {m['norm']:.6f}")
    worst = max((float((np.abs(grads[k].numpy() - want[k]) - 3e-3 * np.abs(want[k])).max()) / rms, k) for k in want)
    print(f"dtype {dt}: worst gradient excess over rtol, in rms: {worst[0]:.3e} ({worst[1]}) against 3e-2")
    # the weights: elements whose oracle gradient is well conditioned in both steps
    trms = {k: float(np.sqrt((v ** 2).mean())) for k, v in want.items()}
    med = sorted(trms.values())[len(trms) // 2]
    floor = 1e-3 if dt == 0 else 2e-1
    moves, refs, far = [], [], {}
    for k in want:
        if trms[k] < 1e-3 * med:
            continue
        ok = (np.abs(want[k]) > floor * trms[k]) & (np.abs(m["g2"][k]) > floor * trms[k])
        got_move, ref_move = (sd[k] - w0[k]).numpy()[ok], (m["w2"][k] - w0[k].numpy())[ok]
        moves.append(got_move); refs.append(ref_move)
        far[k] = float((np.abs(got_move - ref_move) > 2 * 2.1 * LR).mean()) if ok.any() else 0.0
    moves, refs = np.concatenate(moves), np.concatenate(refs)
    mrms = float(np.sqrt((refs ** 2).mean()))
    excess = float((np.abs(moves - refs) - 3e-3 * np.abs(refs)).max())
    print(f"dtype {dt}: {len(refs)} weights compared, rms move {mrms:.3e}, worst excess over rtol {excess:.3e} against {3e-2 * mrms:.3e}; "
          f"worst far fraction {max(far.values()):.3e}")
    assert len(refs) > 1000
    if dt == 0:
        assert np.isclose(loss1, m["loss"][0], rtol=3e-3, atol=0) and np.isclose(loss2, m["loss"][1], rtol=3e-3, atol=0)
        for k in want:
            assert np.allclose(grads[k].numpy(), want[k], rtol=3e-3, atol=3e-2 * rms), k
        assert abs(gnorm - m["norm"]) <= 3e-3 * m["norm"]
        assert np.allclose(moves, refs, rtol=3e-3, atol=3e-2 * mrms)
    else:
        for got, ref in zip((loss1, loss2), m["loss"]):
            assert abs(got - ref) < 3e-2 * max(1.0, ref), (got, ref)
        assert grel < 8e-2, grel
        assert max(far.values()) < 0.02, far


def test_one_channel_sampler_one_graph_per_step_equals_the_host_driven_loop():
    """tests/test_path_gpu.py::test_sampler_one_graph_per_step_equals_the_host_driven_loop at one channel: device RNG, history off,
    4 reverse steps of the mnist preset's net; 'noise_reduction' is a shift upstream can run at C = 1."""
    import mdm
    from oracle.unet_ref import random_params
    cfg = mdm.unet6_config(32, in_channels=1, out_channels=1)
    params = random_params(cfg)
    outs = []
    for flag in (False, True):
        model = mdm.UNet(cfg, N=4, H=32, W=32, dtype=1, params=params).eval()
        a = _mnist_args(sampling_mask_dependency="independent", momentum_adaptive="base_momentum", sample_num=4,
                        sample_latent_shape="uniform", sample_history=False, rng_mode="device", seed=5, sampler_graph=flag)
        a.ddpm_num_steps = 4
        s = mdm.Scheduler(a)
        s.update_ddpm_num_steps(4)
        smp = mdm.Sampler(None, a, s, [None] * 3)
        seed_all(401)
        x0, hist = smp.sample(model, s.get_timesteps_epoch(0, 1))
        torch.cuda.synchronize()
        assert hist == [] and tuple(x0.shape) == (4, 1, 32, 32) and bool(torch.isfinite(x0).all())
        assert hasattr(smp, "_graph_keep") == flag
        outs.append(x0.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
