"""The data ABI without a GPU: include/mdm_data.h parses and is bound next to the core and the presentation header without entering
their tables, every `mdm_data_*` symbol has a kernel-level test, the host checks refuse what the header says they refuse and name the
argument, `DeviceLoader.epoch_indices()` visits what a `torch.utils.data.DataLoader` visits and leaves the host generators as it leaves
them, the shards are accelerate's, and the uint8 table is torchvision's Normalize.  No kernel is launched."""
import ctypes
import os
import re

import pytest
import torch
from torch.utils.data import BatchSampler, DataLoader, RandomSampler, SequentialSampler, TensorDataset

from mdm import _lib
from mdm import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
DATA_HEADER = os.path.join(ROOT, "include", "mdm_data.h")
_K = "test_data_gpu"
COVERAGE = {"mdm_data_gather": (_K, "mdm_data_gather"), "mdm_data_means": (_K, "mdm_data_means")}
GATHER_PARAMS = ["src", "kind", "img_stride", "M", "C", "H", "W", "lut", "index", "first", "N", "flip", "x0", "label", "random", "R",
                 "label_out", "random_out", "stream"]
MEANS_PARAMS = ["src", "kind", "img_stride", "M", "C", "H", "W", "lut", "per_channel", "out", "stream"]


# ------------------------------------------------------------------ the third header and its tables
def test_the_header_parses_and_declares_only_the_two_data_functions():
    structs, protos = _lib.parse_header(open(DATA_HEADER).read())
    assert structs == {} and list(protos) == ["mdm_data_gather", "mdm_data_means"]
    assert [n for n, _ in protos["mdm_data_gather"][1]] == GATHER_PARAMS
    assert [n for n, _ in protos["mdm_data_means"][1]] == MEANS_PARAMS
    g = dict(protos["mdm_data_gather"][1])
    assert (g["src"], g["img_stride"], g["M"], g["first"], g["N"], g["index"], g["flip"]) == \
        ("void*", "int64_t", "int64_t", "int64_t", "int", "int64_t*", "uint8_t*")
    assert protos["mdm_data_gather"][0] == protos["mdm_data_means"][0] == "int"


def test_every_data_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mdm_data_[a-z0-9_]+)\s*\(", open(DATA_HEADER).read()))
    assert declared == set(_lib.DATA_EXPORTS) == set(_lib.DATA_PROTOS) == set(_lib.DATA_PARAMS) and len(declared) == 2
    C = ctypes
    for name in _lib.DATA_EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.DATA_PROTOS[name][0] and fn.restype is C.c_int32, name
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.DATA_PROTOS["mdm_data_gather"][0] == [vp, i32, i64, i64, i32, i32, i32, vp, vp, i64, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    assert _lib.DATA_PROTOS["mdm_data_means"][0] == [vp, i32, i64, i64, i32, i32, i32, vp, i32, vp, vp]
    assert _lib.DATA_PARAMS["mdm_data_gather"] == GATHER_PARAMS


def test_the_core_and_vis_tables_are_still_exactly_their_headers():
    core = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    vis = open(os.path.join(ROOT, "include", "mdm_vis.h")).read()
    assert set(_lib.EXPORTS) == set(_lib._PROTOS) == set(re.findall(r"\b(mdm_[a-z0-9_]+)\s*\(", core)) and len(_lib.EXPORTS) == 92
    assert set(_lib.VIS_EXPORTS) == set(_lib.VIS_PROTOS) == set(re.findall(r"\b(mdm_vis_[a-z0-9_]+)\s*\(", vis)) and len(_lib.VIS_EXPORTS) == 3
    for table in (_lib.EXPORTS, _lib._PARAMS, _lib.VIS_EXPORTS, _lib.VIS_PARAMS):
        assert not [n for n in table if n.startswith("mdm_data_")]
    assert "mdm_data" not in core and "mdm_data" not in vis


def test_call_binds_data_keywords_against_the_data_header():
    """`_lib.call` and `Recording` serve the third table as they serve the other two"""
    kw = dict(src=1, kind=0, img_stride=2, M=3, C=4, H=5, W=6, lut=None, per_channel=1, out=7, stream=None)
    with _lib.Recording() as rec:
        _lib.call("mdm_data_means", **kw)
        with pytest.raises(TypeError, match="mdm_data_means"):
            _lib.call("mdm_data_means", src=1, stride=2)
    assert [(n, a) for n, _, a in rec.calls] == [("mdm_data_means", (1, 0, 2, 3, 4, 5, 6, None, 1, 7))]


def test_every_data_symbol_has_a_kernel_test():
    """as tests/test_abi_coverage_cpu.py does for the core header"""
    assert set(COVERAGE) == set(_lib.DATA_PROTOS)
    for sym, (mod, mention) in COVERAGE.items():
        text = open(os.path.join(TESTS, mod + ".py")).read()
        assert re.search(r"(?<![\w.])" + re.escape(mention) + r"\b", text), f"{mod}.py does not mention {mention}"
        assert "pytest.mark.gpu" in text


# ------------------------------------------------------------------ refusals (host checks: nothing is launched, no device is needed)
P = [0x10000 * k for k in range(1, 10)]                                # never dereferenced: every row fails a host check first
GATHER_OK = dict(src=P[0], kind=1, img_stride=192, M=10, C=3, H=8, W=8, lut=P[1], index=P[2], first=0, N=4, flip=None, x0=P[3],
                 label=P[4], random=P[5], R=2, label_out=P[6], random_out=P[7], stream=None)
MEANS_OK = dict(src=P[0], kind=1, img_stride=192, M=10, C=3, H=8, W=8, lut=P[1], per_channel=1, out=P[3], stream=None)
STORAGE_REFUSALS = [("src", dict(src=None)), ("kind", dict(kind=2)), ("kind", dict(kind=-1)), ("lut", dict(lut=None)),
                    ("M", dict(M=0)), ("M", dict(M=-5)), ("C", dict(C=0)), ("H", dict(H=-1)), ("W", dict(W=0)),
                    ("C H W", dict(C=2048, H=1024, W=1024, img_stride=2 ** 40)), ("img_stride", dict(img_stride=191))]
GATHER_REFUSALS = STORAGE_REFUSALS + [("index", dict(index=None)), ("x0", dict(x0=None)), ("N", dict(N=0)), ("N", dict(N=-1)),
                                      ("first", dict(first=-1)), ("label", dict(label=None)), ("random", dict(random=None)),
                                      ("R", dict(R=0)), ("R", dict(R=-2))]
MEANS_REFUSALS = STORAGE_REFUSALS + [("out", dict(out=None))]


def _refused(name, args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args.values())
    return rc, lib.mdm_last_error().decode()


@pytest.mark.parametrize("name,ok,rows", [("mdm_data_gather", GATHER_OK, GATHER_REFUSALS), ("mdm_data_means", MEANS_OK, MEANS_REFUSALS)])
def test_refusals_name_the_argument(name, ok, rows):
    assert list(ok) == _lib.DATA_PARAMS[name]
    for arg, change in rows:
        rc, text = _refused(name, dict(ok, **change))
        assert rc != 0 and text.startswith(name[4:] + ":") and re.search(r"(?<![\w])" + re.escape(arg) + r"(?![\w])", text), (change, text)


def test_what_is_optional_is_not_refused_for_being_absent():
    """kind 0 needs no table and the label / random pair may be left out together: such a call passes every host check (it is then
    refused by a later one here, so that nothing is launched)"""
    for change in (dict(kind=0, lut=None), dict(label=None, label_out=None), dict(random=None, random_out=None, R=0)):
        rc, text = _refused("mdm_data_gather", dict(GATHER_OK, x0=None, **change))
        assert rc != 0 and "x0" in text, (change, text)
    rc, text = _refused("mdm_data_means", dict(MEANS_OK, kind=0, lut=None, out=None))
    assert rc != 0 and "out" in text


# ------------------------------------------------------------------ the epoch's order and the host generators
def _host_epoch(dl):
    return [b[0].tolist() for b in dl]


@pytest.mark.parametrize("M", [11, 50])
@pytest.mark.parametrize("batch", [3, 8])
@pytest.mark.parametrize("drop_last", [True, False])
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("given", [False, True])
def test_epoch_indices_are_the_dataloaders(M, batch, drop_last, shuffle, given):
    ds = D.DeviceDataset(torch.zeros(M, 1, 1, 1), device="cpu")
    gen_a, gen_b = (torch.Generator().manual_seed(21), torch.Generator().manual_seed(21)) if given else (None, None)
    host = DataLoader(TensorDataset(torch.arange(M)), batch_size=batch, shuffle=shuffle, drop_last=drop_last, generator=gen_a)
    ours = D.DeviceLoader(ds, batch, shuffle=shuffle, drop_last=drop_last, generator=gen_b)
    assert len(ours) == len(host)
    torch.manual_seed(5)
    want = [_host_epoch(host) for _ in range(2)]
    want_state = torch.get_rng_state()
    torch.manual_seed(5)
    got = [ours.epoch_indices() for _ in range(2)]
    assert got == want and all(len(e) == len(host) for e in got)
    assert torch.equal(torch.get_rng_state(), want_state)
    if given:
        assert torch.equal(gen_a.get_state(), gen_b.get_state())
    if shuffle:
        assert got[0] != got[1]
    if not drop_last:
        assert sorted(i for b in got[0] for i in b) == list(range(M))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("M,batch", [(11, 3), (50, 8), (50, 3)])
def test_shards_are_accelerates(world, M, batch):
    from accelerate.data_loader import BatchSamplerShard
    ds = D.DeviceDataset(torch.zeros(M, 1, 1, 1), device="cpu")
    seen = []
    for rank in range(world):
        ours = D.DeviceLoader(ds, batch, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(9), rank=rank, world=world)
        bs = BatchSampler(RandomSampler(range(M), generator=torch.Generator().manual_seed(9)), batch, True)
        shard = BatchSamplerShard(bs, num_processes=world, process_index=rank, split_batches=False)
        for _ in range(2):
            torch.empty((), dtype=torch.int64).random_(generator=bs.sampler.generator)      # the base seed a DataLoader iterator draws
            want = list(shard)
            got = ours.epoch_indices()
            assert got == want and len(ours) == len(want) == (M // batch) // world
        seen.append(got)
    flat = [i for s in seen for b in s for i in b]
    assert len(set(flat)) == len(flat)                                   # the ranks' batches are disjoint
    with pytest.raises(ValueError):
        len(D.DeviceLoader(ds, batch, drop_last=False, world=world))
    with pytest.raises(ValueError):
        D.DeviceLoader(ds, batch, rank=world, world=world).epoch_indices()


def test_prepare_sets_the_shard_and_returns_the_loader():
    import mdm
    ds = D.DeviceDataset(torch.zeros(8, 1, 1, 1), device="cpu")
    dl = D.DeviceLoader(ds, 2, rank=5, world=7)
    acc = mdm.Accelerator(device="cpu")
    other = [torch.zeros(2)]
    out = acc.prepare(dl, other)
    assert out[0] is dl and out[1] is other and (dl.rank, dl.world) == (0, 1)
    assert mdm.DeviceLoader is D.DeviceLoader and mdm.DeviceDataset is D.DeviceDataset


# ------------------------------------------------------------------ the table and the host side of the data set
def test_the_normalize_table_is_torchvisions():
    u = torch.arange(256, dtype=torch.uint8)
    lut = D.normalize_lut()
    assert lut.dtype == torch.float32 and torch.equal(lut, (u.float().div(255) - 0.5) / 0.5)
    assert float(lut[0]) == -1.0 and float(lut[255]) == 1.0
    ds = D.DeviceDataset(torch.zeros(2, 1, 2, 2, dtype=torch.uint8), device="cpu")
    assert torch.equal(ds.lut_host, lut) and ds.kind == 1


def test_the_data_set_is_map_style_on_the_host_side():
    g = torch.Generator().manual_seed(2)
    u8 = torch.randint(0, 256, (5, 3, 4, 6), generator=g, dtype=torch.uint8)
    label = torch.arange(5.0)
    torch.manual_seed(3)
    ds = D.DeviceDataset(u8.numpy(), label, num_timesteps=4, device="cpu")
    torch.manual_seed(3)
    rnd = torch.FloatTensor(5, 4).uniform_(-1, 1)                        # drawn where upstream draws it
    assert len(ds) == 5 and (ds.M, ds.C, ds.H, ds.W, ds.R) == (5, 3, 4, 6, 4)
    for i in (0, 4, -1):
        x, l, r = ds[i]
        assert x.dtype == torch.float32 and torch.equal(x, D.normalize_lut()[u8[i].long()]) and float(l) == float(label[i])
        assert torch.equal(r, rnd[i])
    with pytest.raises(IndexError):
        ds[5]
    f = D.DeviceDataset(torch.ones(2, 1, 2, 2), device="cpu")
    assert f.kind == 0 and f.lut is None and torch.equal(f.label, torch.zeros(2)) and torch.equal(f[1][0], torch.ones(1, 2, 2))

    class Items(torch.utils.data.Dataset):
        def __len__(self):
            return 5

        def __getitem__(self, i):
            return u8[i], int(i) * 2
    torch.manual_seed(3)
    m = D.DeviceDataset.from_dataset(Items(), num_timesteps=4, device="cpu")
    assert torch.equal(m.data, u8) and torch.equal(m.label, 2 * label) and torch.equal(m.random, rnd)
    for bad in (torch.zeros(2, 3, 4), torch.zeros(2, 1, 2, 2, dtype=torch.float64), torch.zeros(0, 1, 2, 2)):
        with pytest.raises(ValueError):
            D.DeviceDataset(bad, device="cpu")
    with pytest.raises(ValueError):
        D.DeviceDataset(torch.zeros(2, 1, 2, 2), lut=torch.zeros(256), device="cpu")


def test_a_data_set_off_the_gpu_launches_nothing():
    ds = D.DeviceDataset(torch.zeros(4, 1, 2, 2), device="cpu")
    for fn in (ds.tensor, ds.means, lambda: next(iter(D.DeviceLoader(ds, 2)))):
        with pytest.raises(TypeError, match="GPU"):
            fn()
    with pytest.raises(TypeError):
        D.DeviceLoader(TensorDataset(torch.zeros(4)), 2)
    with pytest.raises(ValueError):
        D.DeviceLoader(ds, 2).bind(torch.zeros(3, 1, 2, 2))
