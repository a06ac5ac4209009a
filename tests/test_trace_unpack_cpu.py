"""The decoder of the traceback a batch delivers with HAO_DELIVER_TRACE (hao_unpack_trace, include/hao.h) is a pure host function of the three views of the batch:
here they are built by hand - the overlap and ED views of test_ed_unpack_cpu.py, plus per-read cigar offsets, a 16-bit ps and entry count per pair and the
entries - and the decoder must rebuild the pairs helpers.ed_tasks_grid_all forms, widen the results (ps 0xffff -> -1; ts = 0, te = t_len - 1) and hand out
the read's cigars in CSR form.  No GPU involved: the device side is checked by tests/test_gpu_trace_grid.py."""
import ctypes as C

import numpy as np
import pytest

from hifiasm_amd import api
from test_ed_unpack_cpu import _views, _batch, NOALN, U64_MAX


def _trace_view(d, e, keep, want, stored, seed=9):
    """a TraceDelivery over the same pairs: a random subset of the aligned pairs traced, with random cigars"""
    rng = np.random.default_rng(seed)
    n = len(want)
    ps, nc, cig, cg_off = [], [], [], np.zeros(n + 1, dtype=np.uint64)
    per = []
    for i in range(n):
        er, _ = stored[i]
        m = er.shape[0]
        tr = (er != 0xFF) & (rng.random(m) < 0.7)
        p = np.where(tr, rng.integers(0, 40, size=m), 0xFFFF).astype(np.uint16)
        k = np.where(tr, rng.integers(1, 9, size=m), 0).astype(np.uint16)
        c = rng.integers(0, 1 << 16, size=int(k.sum())).astype(np.uint16)
        ps.append(p); nc.append(k); cig.append(c); per.append((p, k, c))
        cg_off[i + 1] = cg_off[i] + c.shape[0]
    ps = np.concatenate(ps + [np.zeros(1, np.uint16)]); nc = np.concatenate(nc + [np.zeros(1, np.uint16)]); cig = np.concatenate(cig + [np.zeros(1, np.uint16)])
    t = api.TraceDelivery()
    t.n_traced, t.n_cigar = int((ps[:-1] != 0xFFFF).sum()), int(cg_off[-1])
    t.cg_off, t.ps, t.n_cig, t.cigar = cg_off.ctypes.data, ps.ctypes.data, nc.ctypes.data, cig.ctypes.data
    keep += [cg_off, ps, nc, cig]
    return t, per


def _unpack(t, e, d, lengths, rid, cap, ccap, fill=0x5A):
    tk = np.full((max(cap, 1), 10), fill, dtype=np.uint32); r = np.full((max(cap, 1), 6), fill, dtype=np.int32)
    off = np.full(max(cap, 1) + 1, fill, dtype=np.uint64); cg = np.full(max(ccap, 1), fill, dtype=np.uint16)
    n = api.lib().hao_unpack_trace(C.byref(t), C.byref(e), C.byref(d), np.ascontiguousarray(lengths, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), rid,
                                   tk.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_uint64)), cg.ctypes.data_as(C.c_void_p),
                                   cap, ccap)
    return int(n), tk, r, off, cg


@pytest.mark.parametrize("window,thre", [(375, 15), (100, 40), (775, 70)])
def test_unpack_rebuilds_tasks_results_and_cigars(window, thre):
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, window, thre)
    t, per = _trace_view(d, e, keep, want, stored)
    total = traced = 0
    for i in range(len(ols)):
        wt = want[i]; p, k, c = per[i]
        n, tk, r, off, cg = _unpack(t, e, d, lengths, rid_lo + i, wt.shape[0] + 2, c.shape[0] + 2)
        assert n == wt.shape[0] and (tk[:n] == wt).all()
        er, pe = stored[i]
        assert (r[:n, 0] == np.where(er == 0xFF, NOALN, er.astype(np.int32))).all()
        assert (r[:n, 2] == np.where(pe == 0xFFFF, -1, pe.astype(np.int32))).all()
        assert (r[:n, 1] == np.where(p == 0xFFFF, -1, p.astype(np.int32))).all()
        assert (r[:n, 3] == 0).all() and (r[:n, 4] == wt[:, 6].astype(np.int32) - 1).all() and (r[:n, 5] == k).all()
        assert off[0] == 0 and (np.diff(off[:n + 1]).astype(np.int64) == k).all()
        assert (cg[:c.shape[0]] == c).all() and (cg[c.shape[0]:] == 0x5A).all()
        total += n; traced += int((p != 0xFFFF).sum())
    assert total == e.n_pairs and traced == t.n_traced and traced > 3


def test_unpack_caps_too_small_write_nothing():
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, 375, 15)
    t, per = _trace_view(d, e, keep, want, stored)
    i = max(range(len(ols)), key=lambda q: per[q][2].shape[0])
    m, mc = want[i].shape[0], per[i][2].shape[0]
    assert m > 2 and mc > 2
    for cap, ccap in ((m - 1, mc), (m, mc - 1)):
        n, tk, r, off, cg = _unpack(t, e, d, lengths, rid_lo + i, cap, ccap)
        assert n == m and (tk == 0x5A).all() and (r == 0x5A).all() and (off == 0x5A).all() and (cg == 0x5A).all()
    n, tk, r, off, cg = _unpack(t, e, d, lengths, rid_lo + i, m, mc)
    assert n == m and (tk == want[i]).all() and (cg == per[i][2]).all()


def test_unpack_reads_outside_the_batch():
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, 375, 15)
    t, per = _trace_view(d, e, keep, want, stored)
    for rid in (0, rid_lo - 1, rid_lo + len(ols), 13, 10**9):
        n, tk, r, off, cg = _unpack(t, e, d, lengths, rid, 100, 100)
        assert n == 0 and (tk == 0x5A).all() and (cg == 0x5A).all(), rid
    n, tk, r, off, cg = _unpack(t, e, d, lengths, 6, 100, 100)      # read 6 of the batch has no overlaps: no pairs, an empty cigar range
    assert n == 0 and off[0] == 0 and (cg == 0x5A).all()


def test_unpack_with_mismatched_lengths_or_counts_is_refused():
    lengths, rid_lo, ols = _batch()
    d, e, keep, want, stored = _views(lengths, ols, rid_lo, 375, 15)
    t, per = _trace_view(d, e, keep, want, stored)
    i = max(range(len(ols)), key=lambda q: want[q].shape[0])
    other = lengths.copy(); other[rid_lo + i] += 4 * 375
    other[[int(y) for y in ols[i][:, 4]]] = 120
    n, *_ = _unpack(t, e, d, other, rid_lo + i, 10_000, 10_000)
    assert n == U64_MAX
    # entry counts that do not add up to the read's delivered range
    nc = np.frombuffer((C.c_uint16 * (int(e.n_pairs) + 1)).from_address(t.n_cig), dtype=np.uint16)
    p0 = int(np.frombuffer((C.c_uint64 * (len(ols) + 1)).from_address(e.ed_off), dtype=np.uint64)[i])
    nc[p0] += 1
    n, *_ = _unpack(t, e, d, lengths, rid_lo + i, 10_000, 10_000)
    assert n == U64_MAX
