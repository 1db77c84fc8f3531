"""MonitorRing's host side (decode, cursor, wrap-around, dropped rows) against a hand-filled buffer, and the two monitor entry
points in the header and the ctypes table.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _commit(ring, n):
    """What n mdm_monitor_commit launches leave in `ring.buf`: row k holds k + column / 10 in every column."""
    buf = ring.buf.numpy()
    rows = buf[8:].view(np.float32).reshape(ring.cap, 8)
    ctr = int(buf[0])
    for k in range(ctr, ctr + n):
        rows[k % ring.cap] = k + np.arange(8, dtype=np.float32) / 10
    buf[0] = ctr + n


def test_columns_are_the_reference_names_then_norm_and_flags():
    from mdm import MonitorRing
    assert MonitorRing.COLUMNS == ("train_loss", "inverse_reconstruct_train_mean", "reconstruct_train_mean",
                                   "shifted_degrade_img_mean", "degraded_train_mean", "grad_norm", "flags", "reserved")


def test_layout_one_buffer_counter_then_rows():
    from mdm import MonitorRing
    r = MonitorRing("cpu", 5)
    assert r.buf.dtype == torch.int32 and r.buf.numel() == 8 + 5 * 8
    assert r.ring.shape == (5, 8) and r.ring.dtype == torch.float32 and r.mon_q40.shape == (6,) and r.mon_q40.dtype == torch.int64
    assert r.ctr.data_ptr() == r.buf.data_ptr() and r.ring.data_ptr() == r.buf.data_ptr() + 32      # views: one copy reads both
    rows, dropped = r.read()
    assert rows.shape == (0, 8) and dropped == 0
    with pytest.raises(RuntimeError):
        r.last()
    with pytest.raises(ValueError):
        MonitorRing("cpu", 0)


def test_read_is_oldest_first_and_moves_the_cursor():
    from mdm import MonitorRing
    r = MonitorRing("cpu", 4)
    _commit(r, 3)
    rows, dropped = r.read()
    assert dropped == 0 and rows.dtype == np.float32 and rows.shape == (3, 8)
    assert np.array_equal(rows[:, 0], [0, 1, 2]) and np.allclose(rows[1], 1 + np.arange(8) / 10)
    assert np.array_equal(r.last(), rows[-1])
    rows, dropped = r.read()
    assert len(rows) == 0 and dropped == 0                        # nothing new
    _commit(r, 3)                                                 # commits 3, 4, 5: rows 3, 0, 1 -- wraps
    rows, dropped = r.read()
    assert dropped == 0 and np.array_equal(rows[:, 0], [3, 4, 5])
    assert r.last()[0] == 5
    _commit(r, 4)                                                 # exactly cap unread rows: all still there
    rows, dropped = r.read()
    assert dropped == 0 and np.array_equal(rows[:, 0], [6, 7, 8, 9])


def test_dropped_rows_are_counted_not_hidden():
    from mdm import MonitorRing
    r = MonitorRing("cpu", 4)
    _commit(r, 2)
    r.read()
    _commit(r, 7)                                                 # commits 2..8, the ring keeps 5..8
    rows, dropped = r.read()
    assert dropped == 3 and np.array_equal(rows[:, 0], [5, 6, 7, 8])
    rows, dropped = r.read()
    assert dropped == 0 and len(rows) == 0
    assert r.row(8)[0] == 8 and r.row(5)[0] == 5
    with pytest.raises(RuntimeError):
        r.row(4)                                                  # overwritten


def test_deferred_handle_reads_its_own_row():
    from mdm import MonitorRing
    from mdm.train_step import DeferredLoss
    r = MonitorRing("cpu", 4)
    _commit(r, 3)
    r.issued = 3
    h = DeferredLoss(r, 1)
    assert float(h) == 1.0 and h.item() == 1.0 and float(DeferredLoss(r, 2, 4)) == np.float32(2.4)
    _commit(r, 3)
    r.issued = 6
    with pytest.raises(RuntimeError):
        float(h)


def test_counter_is_read_modulo_2_32():
    from mdm import MonitorRing
    r = MonitorRing("cpu", 4)
    r.buf[0] = -2                                                 # 2^32 - 2 as the device's unsigned counter
    r.cursor = 2 ** 32 - 2
    rows = r.buf.numpy()[8:].view(np.float32).reshape(4, 8)
    rows[(2 ** 32 - 2) % 4] = 7.0
    rows[(2 ** 32 - 1) % 4] = 8.0
    r.buf[0] = 0                                                  # two commits later the counter has wrapped
    got, dropped = r.read()
    assert dropped == 0 and np.array_equal(got[:, 0], [7.0, 8.0])


def test_counter_wrap_with_a_cap_that_does_not_divide_2_32():
    """The device indexes with (uint32 counter) % cap: across the wrap the rows are NOT consecutive for cap = 3."""
    from mdm import MonitorRing
    r = MonitorRing("cpu", 3)
    rows = r.buf.numpy()[8:].view(np.float32).reshape(3, 8)
    r.cursor = 2 ** 32 - 2
    for k, v in ((2 ** 32 - 2, 7.0), (2 ** 32 - 1, 8.0), (0, 9.0)):
        rows[k % 3] = v                                           # 2^32 - 2 -> row 2, 2^32 - 1 -> row 0, 0 -> row 0 again
    r.buf[0] = 1                                                  # three commits later
    got, dropped = r.read()
    assert dropped == 0 and np.array_equal(got[:, 0], [rows[(2 ** 32 - 2) % 3, 0], rows[(2 ** 32 - 1) % 3, 0], rows[0, 0]])
    assert got[0, 0] == 7.0 and got[2, 0] == 9.0


def test_entry_points_are_declared_and_bound():
    from mdm import _lib
    hdr = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    for name, nargs in (("mdm_loss_fwd_bwd_mon", 17), ("mdm_monitor_commit", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in _lib._PROTOS and name in _lib.EXPORTS
        assert len(_lib._PROTOS[name][0]) == nargs, name
    assert len(_lib._PROTOS["mdm_loss_fwd_bwd_mon"][0]) == len(_lib._PROTOS["mdm_loss_fwd_bwd"][0]) + 2

