"""The nearest-neighbour host layer on the GPU (mdm/evaluate.py `NeighborBank`, `Sampler.get_nearest_neighbor`, `get_similar_neighbor`,
`Tester.img_set`) against upstream's method restated with torch on the CPU (tests/_neighbor_ref.py: `F.interpolate` +
`F.cosine_similarity` + `max(dim=0)`, sampler.py:487-518; tester.py:209-223).

Data: M = 48 images (40 at 256 x 256), each a random 4 x 4 x C grid bilinearly upsampled plus 0.05 randn; sources are normalize01 of
six of them plus 0.05 randn.  Every test first asserts on the CPU reference that the best and the second-best similarity of every
column are at least 0.01 apart, so that an index is a property of the method and not of a rounding."""
import types

import numpy as np
import pytest
import torch

import _neighbor_ref as NR

pytestmark = pytest.mark.gpu
SIZES = (48, 64, 100, 128, 256)
PICKS = [3, 7, 11, 20, 33, 39]
GAP = 0.01


def _set(size, kind):
    """(what is stored -- uint8 or fp32 [M][3][size][size] --, its fp32 values, the sources), drawn once per (size, kind)"""
    key = (size, kind)
    if key not in _SETS:
        from mdm.data import normalize_lut
        x = NR.host_set(40 if size == 256 else 48, 3, size, seed=size)
        if kind == "u8":
            stored = NR.as_bytes(x)
            values = normalize_lut()[stored.long()]
        else:
            stored = values = x
        _SETS[key] = (stored, values, NR.host_sources(values, PICKS))
    return _SETS[key]


_SETS, _REFS = {}, {}


def _reference(size, kind, antialias):
    """score [M][B] of upstream's method on the CPU, its gap asserted"""
    key = (size, kind, antialias)
    if key not in _REFS:
        _, values, src = _set(size, kind)
        _REFS[key] = _gapped(NR.scores_torch(src, values, antialias))
    return _REFS[key]


def _gapped(score):
    top = score.topk(2, dim=0).values
    assert float((top[0] - top[1]).min()) >= GAP, f"the reference's own gap is {float((top[0] - top[1]).min())}: the case decides nothing"
    return score


def _sampler(dataset, antialias=True):
    import mdm
    return mdm.Sampler(dataset, types.SimpleNamespace(nn_antialias=antialias), None, [None] * 3)


@pytest.mark.parametrize("antialias", (True, False))
@pytest.mark.parametrize("kind", ("u8", "f32"))
@pytest.mark.parametrize("size", SIZES)
def test_sampler_get_nearest_neighbor_returns_the_references_images(size, kind, antialias):
    import mdm
    stored, values, src = _set(size, kind)
    want = _reference(size, kind, antialias).argmax(dim=0)
    assert want.tolist() == PICKS
    smp = _sampler(mdm.DeviceDataset(stored, random=torch.zeros(len(stored), 1)), antialias)
    got = smp.get_nearest_neighbor(src)
    assert got.shape == src.shape and got.device == src.device and got.dtype == src.dtype
    assert torch.equal(got, values[want]), "not dataset[idx][0] of the reference's indices"
    bank = smp._nn_bank
    assert smp.get_nearest_neighbor(src.cuda()).is_cuda and smp._nn_bank is bank, "the bank is made once per Sampler"
    assert bank.size == 32 and bank.antialias == antialias and bank.D == 3072 and bank.cached


@pytest.mark.parametrize("size, kind, antialias", [(64, "u8", True), (100, "f32", False), (256, "u8", True), (256, "f32", True)])
def test_bank_similarity_is_within_the_bound_of_the_reference(size, kind, antialias):
    """Both unit rows are off by at most the norm of their per-element bound (tests/_neighbor_ref.py), their product -- an fp32
    contraction over D = 3072 products of unit rows -- by (D + 8) 2^-23 (the allowance tests/_bounds.py gives mdm_gemm); the
    reference matrix is fp32 arithmetic of the same length and gets the same allowance: twice the sum."""
    import mdm
    stored, values, src = _set(size, kind)
    bank = mdm.NeighborBank(mdm.DeviceDataset(stored, random=torch.zeros(len(stored), 1)), size=32, antialias=antialias)
    S = bank.similarity(src).cpu()
    ref = _reference(size, kind, antialias)
    ea = max(np.linalg.norm(NR.row_ref(values[m].numpy(), 1, 0, 32, antialias)[1]) for m in range(0, len(values), 5))
    eb = max(np.linalg.norm(NR.row_ref(src[b].numpy(), 0, 0, 32, antialias)[1]) for b in range(len(src)))
    tol = 2 * (ea + eb + (3072 + 8) * 2.0 ** -23)
    assert S.shape == ref.shape and float((S - ref).abs().max()) <= tol, (float((S - ref).abs().max()), tol)
    Sf = bank.similarity(torch.flip(src, dims=[-1])).cpu()
    assert float((bank.similarity(src, flip=True).cpu() - Sf).abs().max()) <= tol, "flip=True is not the mirrored source"


def _planted(antialias):
    """a 64 x 64 set in which the 32 x 32 neighbour and the full-resolution neighbour differ: decoy B carries a one-pixel
    checkerboard, and so does the source made of image A -- at full resolution the shared checkerboard decides, under either
    resize to 32 x 32 it averages out"""
    A, B = 11, 29
    values = NR.host_set(48, 3, 64, seed=64).clone()
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    checker = ((yy + xx) % 2).float() * 2 - 1
    values[B] += 1.5 * checker
    src = NR.normalize01_torch(values[[A]]) + 0.6 * checker + 0.05 * torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    small, full = _gapped(NR.scores_torch(src, values, antialias)), _gapped(NR.scores_torch(src, values, antialias, size=None))
    assert int(small.argmax(dim=0)) == A and int(full.argmax(dim=0)) == B
    return values, src, A, B


@pytest.mark.parametrize("antialias", (True, False))
def test_the_32x32_neighbour_comes_back_where_full_resolution_differs(antialias):
    import mdm
    values, src, A, B = _planted(antialias)
    ds = mdm.DeviceDataset(values, random=torch.zeros(48, 1))
    assert torch.equal(_sampler(ds, antialias).get_nearest_neighbor(src), values[[A]]), "upstream compares 32 x 32 resizes"
    assert mdm.evaluate.get_nearest_neighbor_idx(src, ds).tolist() == [B]          # Tester's comparison stays at full resolution
    assert mdm.evaluate.get_nearest_neighbor_idx(src, values).tolist() == [B]


@pytest.mark.parametrize("size, seed, mirrored", [(64, 3, [0, 2, 4]), (100, 11, [0, 2])])
def test_augment_equals_the_reference_run_with_the_same_seed(size, seed, mirrored):
    """mirrored plants: some sources are made of MIRRORED data images, so only the similarity with a flipped batch finds them.  (The
    plants sit in batches that the seed flips: a mirrored source whose batch stays has no neighbour that stands out, and the gap
    assertion would say so.)"""
    import mdm
    stored, values, src = _set(size, "u8")
    src = src.clone()
    src[mirrored] = torch.flip(src[mirrored], dims=[-1])
    torch.manual_seed(seed)
    ref = _gapped(NR.scores_torch(src, values, True, augment=True))
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    flips = NR.flip_draws(len(values), len(src))
    assert any(flips) and not all(flips), "the seed must flip some batches and leave others"
    plain = NR.scores_torch(src, values, True).argmax(dim=0)
    assert plain.tolist() != ref.argmax(dim=0).tolist(), "the mirrored plants must change an answer"
    smp = _sampler(mdm.DeviceDataset(stored, random=torch.zeros(len(stored), 1)))
    torch.manual_seed(seed)
    got = smp.get_nearest_neighbor(src, augment=True)
    assert torch.equal(torch.get_rng_state(), state), "the host generator is not where upstream leaves it"
    assert torch.equal(got, values[ref.argmax(dim=0)])
    state = torch.get_rng_state()
    smp.get_nearest_neighbor(src)
    assert torch.equal(torch.get_rng_state(), state), "augment=False draws"


def test_metric_other_than_cosine_is_upstreams_error():
    import mdm
    stored, values, src = _set(48, "f32")
    with pytest.raises(UnboundLocalError):
        _sampler(mdm.DeviceDataset(stored, random=torch.zeros(48, 1))).get_nearest_neighbor(src, metric="l2")


@pytest.mark.parametrize("size, kind", [(64, "u8"), (48, "f32")])
def test_chunked_equals_cached(size, kind):
    import mdm
    stored, values, src = _set(size, kind)
    ds = mdm.DeviceDataset(stored, random=torch.zeros(len(stored), 1))
    cached, chunked = mdm.NeighborBank(ds), mdm.NeighborBank(ds, chunk=16, cache_bytes=0)
    assert cached.cached and cached.rows.shape == (48, 3072) and not chunked.cached and chunked.rows is None
    assert chunked._chunk_rows.shape == (16, 3072), "no more than one chunk of rows is live"
    mask = torch.zeros(48, dtype=torch.uint8)
    mask[12:30] = 1
    for rows in (None, mask):
        v0, i0 = cached.nearest_idx(src, rows, with_val=True)
        v1, i1 = chunked.nearest_idx(src, rows, with_val=True)
        assert torch.equal(i0, i1) and (rows is not None or i0.tolist() == PICKS)
        assert float((v0 - v1).abs().max()) <= (3072 + 8) * 2.0 ** -23
    assert float((cached.similarity(src) - chunked.similarity(src)).abs().max()) <= (3072 + 8) * 2.0 ** -23
    assert torch.equal(chunked.nearest(src).cpu(), values[PICKS])


@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_get_nearest_neighbor_idx_on_a_device_dataset_equals_the_tensor_path(kind):
    import mdm
    from mdm import evaluate as E
    stored, values, src = _set(48, kind)
    _gapped(NR.scores_torch(src, values, True, size=None))
    ds = mdm.DeviceDataset(stored, random=torch.zeros(48, 1))
    want = E.get_nearest_neighbor_idx(src, values)
    assert want.tolist() == PICKS
    assert torch.equal(E.get_nearest_neighbor_idx(src, ds), want)
    bank = ds._nn_bank_full
    assert bank.size is None and bank.D == 3 * 48 * 48
    assert torch.equal(E.get_nearest_neighbor(src, ds), values[PICKS]) and ds._nn_bank_full is bank, "the bank is kept on the data set"
    assert torch.equal(E.get_nearest_neighbor(src, values), values[PICKS])


def _similar_problem():
    """12 generated images: 0..5 distinct, 6..8 near copies of 0, 1, 2 (similarity > 0.9), 9..11 distinct again; three of the
    lists already hold a member: one a near copy of a generated image, two unrelated"""
    g = torch.Generator().manual_seed(9)
    base = torch.randn(9, 3, 16, 16, generator=g)
    gen = torch.cat((base[:6], base[:3] + 0.1 * torch.randn(3, 3, 16, 16, generator=g), base[6:]))
    idx = [4, 1, 4, 0, 1, 5, 4, 1, 2, 0, 5, 4]
    img_set = [torch.empty(0, 3, 16, 16) for _ in range(6)]
    img_set[0] = torch.randn(1, 3, 16, 16, generator=g)
    img_set[1] = (gen[4] + 0.1 * torch.randn(3, 16, 16, generator=g)).unsqueeze(0)
    img_set[3] = torch.randn(2, 3, 16, 16, generator=g)
    S = torch.nn.functional.cosine_similarity(gen.flatten(1)[None], torch.cat([gen] + img_set).flatten(1)[:, None], dim=2)
    assert float((S - 0.9).abs().min()) > 0.01, "a pair sits at the threshold"
    return gen, idx, img_set


def test_get_similar_neighbor_equals_the_restatement():
    from mdm import evaluate as E
    gen, idx, img_set = _similar_problem()
    want = NR.similar_neighbor_ref(gen, [t.clone() for t in img_set], idx, 0.9)
    got = E.get_similar_neighbor(gen, [t.clone() for t in img_set], torch.tensor(idx), 0.9)
    assert [t.shape[0] for t in want] == [3, 2, 1, 2, 3, 2] and len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    again = E.get_similar_neighbor(gen, [t.clone() for t in got], torch.tensor(idx), 0.9)       # a second round adds nothing
    for a, b in zip(again, want):
        assert torch.equal(a, b)


def test_tester_keeps_img_set():
    """`Tester.train` (tester.py:83, 119-120): the rounds' unique images and nearest indices, replayed through the restatement"""
    import mdm
    from golden.make_golden import TINY, base_args
    from mdm.evaluate import Tester
    from oracle.unet_ref import random_params
    a = base_args(data_size=16, ddpm_schedule="linear", ddpm_num_steps=8, shift_type="noise_with_perturbation", sample_num=4,
                  sampling_mask_dependency="independent", momentum_adaptive="base_momentum", sample_latent_shape="uniform",
                  sample_history=False, rng_mode="device", seed=8, data_subset_num=6)
    model = mdm.UNet(TINY, N=4, H=16, W=16, dtype=mdm.BF16, params=random_params(TINY))
    data = mdm.DeviceDataset(torch.rand(10, 3, 16, 16) * 2 - 1, random=torch.zeros(10, 1))
    tst = Tester(a, None, data, model, mdm.EMA(model), None, None, mdm.Accelerator())
    total = tst.train(0, 1, 0, 0, None, None, max_rounds=6)
    want = [torch.empty(0, 3, 16, 16) for _ in range(10)]
    start, rounds = 0, iter(tst.nearest_idx)
    for end in tst.num_total_unique_images:
        if end > start:
            want = NR.similar_neighbor_ref(total[start:end], want, next(rounds).tolist(), 0.9)
        start = end
    assert len(tst.img_set) == 10 and sum(t.shape[0] for t in tst.img_set) == sum(t.shape[0] for t in want) > 0
    for a_, b_ in zip(tst.img_set, want):
        assert torch.equal(a_, b_)
    assert hasattr(data, "_nn_bank_full"), "a Tester round searches the DeviceDataset through its bank"
