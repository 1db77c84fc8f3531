"""Grouped weight gradients on the GPU: the table mdm_wgrad_group_create uploaded is the one mdm_wgrad_group_schedule describes,
and the launch computes what one mdm_gemm call per layer computes.  Small real tensors; every group owns its operands."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# dev_buf (include/mdm_hip.h): descriptors | flat items (per-tap form) | taps table (merged form) | part tiles | slots, sections padded
# to 256 bytes.  Item word {x, y, z, w}: x = descriptor (-1: padding), w = kind (3: nine-tap); per-tap: y = item, z = tiles per tap and
# k-split; nine-tap: y = tile | (slot + 1) << 12, z = k0 | k1 << 16.
TILE_BITS, K_BITS, GK_TAPS = 12, 16, 3
# N, H, C0, C1, Cout, stride, ups, kernel, splitk, accumulate
GROUP_A = [(4, 8, 64, 0, 64, 1, 0, 3, 1, 0), (2, 16, 64, 0, 128, 1, 0, 1, 1, 0), (8, 16, 128, 0, 128, 1, 0, 3, 4, 1)]
GROUP_B = [(4, 8, 64, 64, 128, 1, 0, 3, 1, 0), (2, 32, 64, 0, 256, 1, 0, 3, 1, 0), (4, 16, 8, 0, 128, 1, 0, 3, 1, 0)]
# the 16 shapes of test_kernels_gpu.test_grouped_weight_gradients_match_self_contained_ones, once: at Q_CUT queues some tiles are cut
# (partial slots + tile_parts_reduce_kernel), which the three short layers of GROUP_B are not
GROUP_D = [s + (3, 0, 0) for s in
           [(8, 8, 64, 0, 64, 1, 0), (8, 8, 64, 0, 128, 1, 0), (4, 16, 64, 64, 64, 1, 0), (4, 32, 128, 0, 128, 1, 0), (8, 16, 64, 0, 64, 2, 0),
            (4, 8, 64, 0, 64, 1, 1), (16, 4, 256, 0, 256, 1, 0), (4, 8, 64, 64, 128, 1, 0), (4, 16, 64, 64, 128, 1, 0),
            (2, 16, 128, 0, 128, 1, 1), (4, 4, 64, 0, 128, 1, 1), (2, 32, 64, 0, 256, 1, 0), (1, 64, 64, 64, 128, 1, 0),
            (2, 64, 128, 0, 128, 1, 0), (4, 16, 8, 0, 128, 1, 0), (4, 16, 128, 0, 8, 1, 0)]]
Q_CUT = 32          # queues of "d_merged_cut_tiles": GROUP_D then has cut tiles (26 parts in slots) on any device of >= 32 CUs
CASES = {"a_per_tap": (GROUP_A, None, None, 0), "b_merged": (GROUP_B, 0, None, 1), "c_merged_reserve32": (GROUP_B, 0, 32, 1),
         "d_merged_cut_tiles": (GROUP_D, 0, None, 1)}


def pad256(v):
    return (v + 255) // 256 * 256


def build(members, dev):
    """-> (fields of the group, [(gw, gb, reference gw, reference gb, initial value of gw or None)]): the references are one
    self-contained mdm_gemm call per layer on the same operands."""
    from mdm import _lib, ops
    g = torch.Generator().manual_seed(1234)
    fields, outs, keep = [], [], []
    for N, H, C0, C1, Cout, stride, ups, k, splitk, acc in members:
        if k == 1:
            geom = ops.ConvGeom(N=N, IH=H, IW=H, C0=C0, C1=C1, Cout=Cout, KH=1, KW=1, pad_t=0, pad_l=0, pad_b=0, pad_r=0)
        else:
            pads = (1, 1, 1, 1) if stride == 1 else (0, 0, 1, 1)
            geom = ops.ConvGeom(N=N, IH=H, IW=H, C0=C0, C1=C1, Cout=Cout, stride=stride, pad_t=pads[0], pad_l=pads[1], pad_b=pads[2],
                                pad_r=pads[3], ups=ups)
        rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev, torch.bfloat16).contiguous()
        x0, x1, gy = rnd(N, H, H, C0), (rnd(N, H, H, C1) if C1 else None), rnd(N, geom.OH, geom.OW, Cout)
        ws = torch.empty(max(ops.conv_wgrad_ws_bytes(1, geom) // 4, 16), device=dev)
        ref_w, ref_b = torch.full((geom.taps, Cout, geom.Cin), 0.5, device=dev), torch.zeros(Cout, device=dev)
        ops.conv_wgrad(1, geom, gy, x0, x1, ref_w, ws=ws, dbias=ref_b, acc=1)
        gw, gb = torch.full((geom.taps, Cout, geom.Cin), 0.5, device=dev), torch.zeros(Cout, device=dev)
        wf = ops.wgrad_fields(1, geom, gy, x0, x1, gw, dbias=gb, acc=acc)
        assert _lib.wgrad_group_accepts(**wf)
        wf["splitk"] = splitk if splitk else max(ops.wgrad_group_split(geom), 1)
        if wf["splitk"] > 1:
            gws = torch.full((wf["splitk"] * geom.taps * Cout * geom.Cin,), float("nan"), device=dev)
            wf["ws"], wf["ws_bytes"] = gws, gws.numel() * 4
        fields.append(wf)
        outs.append((gw, gb, ref_w if acc else ref_w - 0.5, ref_b, acc))
        keep += [x0, x1, gy, ws]
    return fields, outs, keep


def decode(table, n, n_rows, form, n_cu):
    """The uploaded item table as the rows of mdm_wgrad_group_schedule, by the documented layout."""
    from mdm import _lib
    raw = table.cpu().numpy().tobytes()
    at = pad256(n * ctypes.sizeof(_lib.GemmDesc))       # form 0: the flat items follow the descriptors; form 1: that section is empty
    words = torch.frombuffer(bytearray(raw[at:at + 16 * n_rows]), dtype=torch.int32).view(n_rows, 4).tolist()
    queues, rows = (n_cu if form else 8), []
    for i, (x, y, z, w) in enumerate(words):
        if x < 0:
            rows.append((i % queues, i // queues, -1, 0, 0, 0, 0, 0))
        elif w == GK_TAPS:
            rows.append((i % queues, i // queues, x, w, y & ((1 << TILE_BITS) - 1), z & ((1 << K_BITS) - 1), (z & 0xFFFFFFFF) >> K_BITS,
                         y >> TILE_BITS))
        else:
            rows.append((i % queues, i // queues, x, w, y, z, 0, 0))
    return rows


@pytest.mark.parametrize("name", list(CASES))
def test_group_table_and_gradients(name, monkeypatch):
    from mdm import _lib
    members, min_share, reserve, want_form = CASES[name]
    dev = torch.device("cuda:0")
    if name == "d_merged_cut_tiles":        # the persistent launch is planned for Q_CUT queues whatever the device's CU count
        assert torch.cuda.get_device_properties(dev).multi_processor_count >= Q_CUT
        reserve = torch.cuda.get_device_properties(dev).multi_processor_count - Q_CUT
    for var, val in (("MDM_TAPS_MIN_SHARE", min_share), ("MDM_WGRAD_RESERVE_CUS", reserve)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    fields, outs, keep = build(members, dev)
    n_cu = max(8, torch.cuda.get_device_properties(dev).multi_processor_count - (reserve or 0))
    rows, need, form = _lib.wgrad_group_schedule(fields, n_cu)
    assert form == want_form
    grp = _lib.WgradGroup(fields, dev)
    assert grp.table.numel() == need
    assert decode(grp.table, len(fields), len(rows), form, n_cu) == rows
    if name == "d_merged_cut_tiles":
        assert n_cu == Q_CUT and any(r[7] > 0 for r in rows)
    runs = []
    for _ in range(2):
        for gw, gb, _, _, _ in outs:
            gw.fill_(0.5)
            gb.zero_()
        grp.launch()
        torch.cuda.synchronize()
        for gw, gb, ref_w, ref_b, _ in outs:
            # the tolerance of test_grouped_weight_gradients_match_self_contained_ones
            assert float((gw - ref_w).abs().max()) <= 1e-5 * float(ref_w.abs().max()) + 2e-6
            assert float((gb - ref_b).abs().max()) <= 1e-5 * float(ref_b.abs().max()) + 1e-5
            assert float(ref_w.abs().max()) > 0.1
        runs.append([gw.clone() for gw, *_ in outs])
    # plain stores and sums in a fixed order: the weight gradients are the same bits on every run (the bias gradients are fp32
    # atomics of several workgroups -- mdm_gemm_desc.dbias -- and are held to the tolerance above, not to bit equality)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
