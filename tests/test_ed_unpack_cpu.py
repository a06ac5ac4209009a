"""The decoder of the window-alignment results a batch delivers with HAO_DELIVER_ED (hao_unpack_ed, include/hao.h) is a pure host function of the two views of
the batch: here both views are built by hand - overlaps in their 32-byte wire form, per-read pair offsets, one error byte and one 16-bit pattern end per
pair - and the decoder must rebuild the pairs helpers.ed_tasks_grid_all forms from the same overlaps, in the same order, with the results widened
(0xff -> INT32_MAX, 0xffff -> -1).  No GPU involved: the device side is checked by tests/test_gpu_ed_deliver.py."""
import ctypes as C

import numpy as np
import pytest

from hifiasm_amd import api
from helpers import ed_tasks_grid_all

NOALN = 2**31 - 1
U64_MAX = 2**64 - 1


def _views(lengths, ols, rid_lo, window, thre, seed=5):
    """ols[i] = hao_ovlp_t rows (uint32 [n, 12]) of read rid_lo + i -> (Delivery, EdDelivery, keep-alive, expected tasks per read, stored err / pe per read)"""
    rng = np.random.default_rng(seed)
    n = len(ols)
    ol_off = np.zeros(n + 1, dtype=np.uint64)
    ol_off[1:] = np.cumsum([o.shape[0] for o in ols])
    allo = np.concatenate(ols).reshape(-1, 12) if n else np.zeros((0, 12), np.uint32)
    wire = np.zeros((max(1, allo.shape[0]), 8), dtype=np.uint32)      # hao_ovlp_wire_t: y | strand << 31, x_pos_s, x_pos_e, y_pos_s, y_pos_e, shared_seed, nhe, fc_len
    if allo.shape[0]:
        wire[:allo.shape[0]] = np.stack([allo[:, 4] | (allo[:, 7] << 31), allo[:, 1], allo[:, 2], allo[:, 5], allo[:, 6], allo[:, 8], allo[:, 10], allo[:, 11]], axis=1)
    want = [ed_tasks_grid_all(lengths, [o], rid_lo + i, window, thre) for i, o in enumerate(ols)]
    ed_off = np.zeros(n + 1, dtype=np.uint64)
    ed_off[1:] = np.cumsum([w.shape[0] for w in want])
    T = int(ed_off[-1])
    err = rng.integers(0, thre + 1, size=T + 1).astype(np.uint8)
    pe = rng.integers(0, window + 2 * thre, size=T + 1).astype(np.uint16)
    none = rng.random(T + 1) < 0.3
    err[none] = 0xFF; pe[none] = 0xFFFF                                # no alignment within thre
    d = api.Delivery()
    d.rid_lo, d.n_reads, d.n_ol = rid_lo, n, allo.shape[0]
    d.ol_off, d.ol = ol_off.ctypes.data, wire.ctypes.data
    e = api.EdDelivery()
    e.n_pairs, e.window, e.thre = T, window, thre
    e.ed_off, e.err, e.pe = ed_off.ctypes.data, err.ctypes.data, pe.ctypes.data
    keep = [ol_off, wire, ed_off, err, pe]
    stored = [(err[int(ed_off[i]):int(ed_off[i + 1])], pe[int(ed_off[i]):int(ed_off[i + 1])]) for i in range(n)]
    return d, e, keep, want, stored


def _ovl(x_id, xs, xe, y_id, ys, ye, rev):
    return np.array([x_id, xs, xe, 0, y_id, ys, ye, rev, 17, 0, 3, 2], dtype=np.uint32)


def _batch():
    rng = np.random.default_rng(11)
    lengths = rng.integers(900, 3200, size=14).astype(np.uint32)
    lengths[6] = 1500
    rid_lo = 4
    ols = []
    for r in range(rid_lo, rid_lo + 5):
        if r == 6:      # a read without overlaps
            ols.append(np.zeros((0, 12), dtype=np.uint32)); continue
        rows = []
        for _ in range(int(rng.integers(2, 7))):
            y = int(rng.integers(0, 14))
            if y == r:
                y = (y + 1) % 14
            L, Ly = int(lengths[r]), int(lengths[y])
            xs = int(rng.integers(0, L // 2)); span = int(rng.integers(100, min(L - xs, Ly)))
            ys = int(rng.integers(0, Ly - span + 1)) if rng.random() < 0.7 else int(rng.integers(0, 8))      # (some start at the target's first bases: abs_diag > 0)
            rows.append(_ovl(r, xs, xs + span - 1, y, ys, min(Ly - 1, ys + span - 1), int(rng.integers(0, 2))))
        ols.append(np.stack(rows))
    return lengths, rid_lo, ols


def _unpack(e, d, lengths, rid, cap, fill=0x5A):
    t = np.full((max(cap, 1), 10), fill, dtype=np.uint32); r = np.full((max(cap, 1), 2), fill, dtype=np.int32)
    n = api.lib().hao_unpack_ed(C.byref(e), C.byref(d), np.ascontiguousarray(lengths, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), rid,
                                t.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), cap)
    return int(n), t, r


@pytest.mark.parametrize("window,thre", [(375, 15), (375, 3), (100, 40), (775, 70)])
def test_unpack_rebuilds_the_grid_pairs(window, thre):
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, window, thre)
    total = 0
    for i in range(len(ols)):
        wt = want[i]
        n, t, r = _unpack(e, d, lengths, rid_lo + i, wt.shape[0] + 3)
        assert n == wt.shape[0]
        assert (t[:n] == wt).all()
        er, pe = stored[i]
        assert (r[:n, 0] == np.where(er == 0xFF, NOALN, er.astype(np.int32))).all()
        assert (r[:n, 1] == np.where(pe == 0xFFFF, -1, pe.astype(np.int32))).all()
        assert ((r[:n, 0] == NOALN) == (r[:n, 1] == -1)).all()      # (absent alignment: both fields)
        total += n
    assert total == e.n_pairs and total > 20
    assert (np.concatenate([s[0] for s in stored]) == 0xFF).any()      # some pairs without an alignment were decoded


def test_unpack_cap_too_small_writes_nothing():
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, 375, 15)
    i = max(range(len(ols)), key=lambda k: want[k].shape[0])
    m = want[i].shape[0]
    assert m > 2
    n, t, r = _unpack(e, d, lengths, rid_lo + i, m - 1)
    assert n == m and (t == 0x5A).all() and (r == 0x5A).all()
    n, t, r = _unpack(e, d, lengths, rid_lo + i, m)
    assert n == m and (t == want[i]).all()


def test_unpack_reads_outside_the_batch_and_without_overlaps():
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, 375, 15)
    for rid in (0, rid_lo - 1, rid_lo + len(ols), 13, 10**9):
        n, t, r = _unpack(e, d, lengths, rid, 100)
        assert n == 0 and (t == 0x5A).all(), rid
    n, t, r = _unpack(e, d, lengths, 6, 100)      # read 6 of the batch has no overlaps, hence no pairs
    assert n == 0 and int(e.n_pairs) > 0 and (t == 0x5A).all()


def test_unpack_with_lengths_of_another_read_set_is_refused():
    """the tasks are rebuilt from the lengths the caller passes: lengths that do not give the delivered pair count are an error (UINT64_MAX), not wrong tasks"""
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, 375, 15)
    i = max(range(len(ols)), key=lambda k: want[k].shape[0])
    other = lengths.copy(); other[rid_lo + i] += 4 * 375      # four more windows: the overlaps still cover the same ones, so make the targets shorter too
    other[[int(y) for y in ols[i][:, 4]]] = 120
    n, t, r = _unpack(e, d, other, rid_lo + i, 10_000)
    assert n == U64_MAX
