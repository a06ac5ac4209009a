"""Reference placement of the window grid, the parts that need no GPU (include/hao.h: "REFERENCE PLACEMENT"):
  * the oracle (hao_or_window_ed, hao_or_window_trace) equals the REAL reference on every task of tests/golden/refgrid.npz (tasks formed by
    tests/refgrid_model.py, results from ref_harness: make_golden_refgrid.py), and the model still forms those tasks;
  * the host decoder of a reference-placed HAO_DELIVER_ED batch (hao_unpack_ed with placement = HAO_PLACE_REF: hao_ref_shift + hao_ref_pair, the functions the
    kernels use) rebuilds the model's tasks from wire bytes built by hand as tests/test_ed_unpack_cpu.py builds them - overlaps in their 32-byte wire form AND
    their fake cigars in the packed and the raw wire form - for the oracle's overlaps of two scenarios and for hand-made overlaps that init_waln refuses or clips;
  * the threshold table equals int(q_l * e_rate), Adjust_Threshold, min 31 for q_l = 0 .. 775 at both rates."""
import ctypes as C
import os

import numpy as np
import pytest

from hifiasm_amd import api
from helpers import scenario_reads, scenario_oracle
import refgrid_model as M

NOALN = 2**31 - 1
U64_MAX = 2**64 - 1
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refgrid.npz"))
CONFIGS = {"hifi": (775, 0.04), "nn": (775, 0.04), "edge": (775, 0.04), "ont": (375, 0.07)}
FIXTURE = {"hifi": ("hifi", 775, 0.04), "nn": ("nn", 775, 0.04), "edge": ("edge", 775, 0.04), "ont": ("ont", 375, 0.07), "hifi375": ("hifi", 375, 0.07)}      # (hifi375: the case with a pair init_waln refuses)


@pytest.mark.parametrize("key", sorted(FIXTURE))
def test_oracle_equals_the_reference_on_the_fixture(key):
    name, wl, e_rate = FIXTURE[key]
    assert tuple(GOLD[key + "_cfg"]) == (wl, e_rate)
    rs, _ = scenario_reads(name)
    o = scenario_oracle(name)
    t, res = GOLD[key + "_tasks"], GOLD[key + "_res"]
    want = np.concatenate([M.read_tasks(*o.lchain(int(r))[:3], rs.lengths, wl, e_rate) for r in GOLD[key + "_reads"]])
    if key == "hifi375":
        infos = [f for r in GOLD[key + "_reads"] for _, _, f in M.read_tasks(*o.lchain(int(r))[:3], rs.lengths, wl, e_rate, with_info=True)[1]]
        assert sum(f["refused"] for f in infos) >= 1 and len(infos) == t.shape[0] + sum(f["refused"] for f in infos)      # the refused window left no task
    assert t.shape == want.shape and (t == want).all()                      # the model forms the fixture's tasks from the oracle's overlaps and fake cigars
    assert t.shape[0] > 6000 and len(set(t[:, 8].tolist())) > 5              # per-window thresholds
    got = o.window_ed(t)
    assert (got == res).all(), np.flatnonzero((got != res).any(axis=1))[:10]
    sidx, sres, scig = GOLD[key + "_sidx"], GOLD[key + "_sres"], GOLD[key + "_scig"]
    tr, cg = o.window_trace(t[sidx], cap=80, mode=3)
    assert (tr == sres).all(), np.flatnonzero((tr != sres).any(axis=1))[:10]
    assert int(sres[:, 5].max()) <= 80
    flat = np.concatenate([cg[i, :tr[i, 5]] for i in range(tr.shape[0])]) if tr.shape[0] else np.zeros(0, np.uint16)
    assert flat.size == scig.size and (flat == scig).all()


@pytest.mark.parametrize("e_rate", [0.04, 0.07])
def test_threshold_table(e_rate):
    for wl in (775, 375):
        tab = api.ref_thresholds(wl, e_rate)
        assert tab.shape == (wl + 1,)
        for q_l in range(wl + 1):
            t = int(q_l * e_rate)
            if t == 0 and q_l >= 4:
                t = 1
            assert int(tab[q_l]) == min(t, 31) == M.threshold(q_l, e_rate), (wl, q_l)
    assert int(api.ref_thresholds(775, 0.04)[775]) == 31 and int(api.ref_thresholds(375, 0.04)[375]) == 15 and list(api.ref_thresholds(775, 0.04)[:5]) == [0, 0, 0, 0, 1]


def _wire_cigar(xs, fc, raw):
    """the words of one fake cigar on the wire (hao_deliver.cuh): packed = 4 bytes per entry after the first (site step | zigzag(shift step) << 20, from (x_pos_s, 0)),
    raw = 2 words per entry; -> (words, raw?)"""
    if not raw and len(fc) and M.fake_gap_pos(fc[0]) == xs and M.fake_gap_shift(fc[0]) == 0:
        words, site, sh, ok = [], xs, 0, True
        for e in fc[1:]:
            ds, dh = M.fake_gap_pos(e) - site, M.fake_gap_shift(e) - sh
            zz = (dh << 1) if dh >= 0 else ((-dh) << 1) - 1
            if ds < 0 or ds >= (1 << 20) or zz >= (1 << 12):
                ok = False; break
            words.append(ds | (zz << 20)); site += ds; sh += dh
        if ok:
            return words, False
    return [w for e in fc for w in (int(e) & 0xFFFFFFFF, int(e) >> 32)], True


def _views(lengths, reads, rid_lo, window, e_rate, seed=5):
    """reads[i] = (ol uint32 [n,12], fc uint64, fc_off [n+1]) of read rid_lo + i -> (Delivery, EdDelivery, keep-alive, expected tasks per read, stored err / pe per read)"""
    rng = np.random.default_rng(seed)
    n = len(reads)
    ols = [r[0] for r in reads]
    ol_off = np.zeros(n + 1, dtype=np.uint64)
    ol_off[1:] = np.cumsum([o.shape[0] for o in ols])
    allo = np.concatenate(ols).reshape(-1, 12) if n else np.zeros((0, 12), np.uint32)
    wire = np.zeros((max(1, allo.shape[0]), 8), dtype=np.uint32)
    if allo.shape[0]:
        wire[:allo.shape[0]] = np.stack([allo[:, 4] | (allo[:, 7] << 31), allo[:, 1], allo[:, 2], allo[:, 5], allo[:, 6], allo[:, 8], allo[:, 10], allo[:, 11]], axis=1)
    words, fc_off, j, n_raw = [], [], 0, 0
    for ol, fc, fo in reads:
        for i in range(ol.shape[0]):
            e = fc[int(fo[i]):int(fo[i + 1])]
            assert len(e) == int(ol[i, 11])
            w, raw = _wire_cigar(int(ol[i, 1]), e, raw=(j % 3 == 2))
            fc_off.append(len(words) | ((1 << 63) if raw else 0)); words += w; j += 1; n_raw += raw
    fc_off.append(len(words))
    fcw = np.array(words + [0], dtype=np.uint32); fco = np.array(fc_off, dtype=np.uint64)
    want = [M.read_tasks(ol, fc, fo, lengths, window, e_rate) for ol, fc, fo in reads]
    ed_off = np.zeros(n + 1, dtype=np.uint64)
    ed_off[1:] = np.cumsum([w.shape[0] for w in want])
    T = int(ed_off[-1])
    err = rng.integers(0, 32, size=T + 1).astype(np.uint8)
    pe = rng.integers(0, window + 62, size=T + 1).astype(np.uint16)
    none = rng.random(T + 1) < 0.3
    err[none] = 0xFF; pe[none] = 0xFFFF
    d = api.Delivery()
    d.rid_lo, d.n_reads, d.n_ol, d.n_fc = rid_lo, n, allo.shape[0], len(words)
    d.ol_off, d.ol, d.fc_off, d.fc = ol_off.ctypes.data, wire.ctypes.data, fco.ctypes.data, fcw.ctypes.data
    e = api.EdDelivery()
    e.n_pairs, e.window, e.thre, e.placement, e.e_rate = T, window, int(api.ref_thresholds(window, e_rate)[window]), api.PLACE_REF, e_rate
    e.ed_off, e.err, e.pe = ed_off.ctypes.data, err.ctypes.data, pe.ctypes.data
    keep = [ol_off, wire, fcw, fco, ed_off, err, pe]
    stored = [(err[int(ed_off[i]):int(ed_off[i + 1])], pe[int(ed_off[i]):int(ed_off[i + 1])]) for i in range(n)]
    return d, e, keep, want, stored, n_raw


def _unpack(e, d, lengths, rid, cap, fill=0x5A):
    t = np.full((max(cap, 1), 10), fill, dtype=np.uint32); r = np.full((max(cap, 1), 2), fill, dtype=np.int32)
    n = api.lib().hao_unpack_ed(C.byref(e), C.byref(d), np.ascontiguousarray(lengths, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), rid,
                                t.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), cap)
    return int(n), t, r


def _check(lengths, reads, rid_lo, window, e_rate):
    d, e, keep, want, stored, n_raw = _views(lengths, reads, rid_lo, window, e_rate)
    total = 0
    for i in range(len(reads)):
        wt = want[i]
        n, t, r = _unpack(e, d, lengths, rid_lo + i, wt.shape[0] + 3)
        assert n == wt.shape[0], (i, n, wt.shape[0])
        assert (t[:n] == wt).all(), (i, np.flatnonzero((t[:n] != wt).any(axis=1))[:5])
        er, pe = stored[i]
        assert (r[:n, 0] == np.where(er == 0xFF, NOALN, er.astype(np.int32))).all()
        assert (r[:n, 1] == np.where(pe == 0xFFFF, -1, pe.astype(np.int32))).all()
        total += n
    assert total == e.n_pairs
    return total, n_raw, want


@pytest.mark.parametrize("name", ["hifi", "ont"])
def test_unpack_rebuilds_the_reference_placed_pairs(name):
    wl, e_rate = CONFIGS[name]
    rs, _ = scenario_reads(name)
    o = scenario_oracle(name)
    lo, hi = 3, 27
    reads = [o.lchain(r)[:3] for r in range(lo, hi)]
    total, n_raw, want = _check(rs.lengths, reads, lo, wl, e_rate)
    T = np.concatenate(want).astype(np.int64)
    assert total > 1500 and n_raw > 50
    assert (T[:, 9] > 0).any() and (T[:, 8] < T[:, 8].max()).any()          # clipped at the target's start; thresholds below the full window's
    # the shift matters: the diagonal start differs on many pairs
    sh = sum(f["shift"] != 0 for ol, fc, fo in reads for _, _, f in M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate, with_info=True)[1])
    assert sh > 100


def _ovl(x_id, xs, xe, y_id, ys, ye, rev, n_fc):
    return np.array([x_id, xs, xe, 0, y_id, ys, ye, rev, 17, 0, 3, n_fc], dtype=np.uint32)


def _fc(entries):
    return np.array([(s << 32) | (((-h) << 1) | 1 if h < 0 else h << 1) for s, h in entries], dtype=np.uint64)


def test_unpack_refused_clipped_and_unresolved_windows():
    """hand-made overlaps: a shifted start before the target's first base or past its last (init_waln refuses), a target too short by more than 31 bases
    (refused) and by less (aux_end > 0), a start inside the first `thre` bases (aux_beg > 0), a 3-base last window (threshold 0), a cigar that does not reach
    the window (unresolved: no pair), a site equal to the last entry's"""
    lengths = np.array([5000, 900, 3000, 3000, 760, 3000, 3000, 3000], dtype=np.uint32)
    wl, e_rate = 775, 0.04
    rows, fcs = [], []

    def add(xs, xe, y, ys, rev, entries):
        rows.append(_ovl(0, xs, xe, y, ys, ys + (xe - xs), rev, len(entries))); fcs.append(_fc(entries))
    add(100, 2400, 2, 5, 0, [(100, 0), (800, -20), (1600, 3), (2400, 3)])          # window 2 (from 1550) takes the entry at 800: shift -20; window 0 starts at target base 5 < thre: aux_beg
    add(0, 1552, 2, 10, 1, [(0, -30), (1552, -30)])                                 # window 0: 10 - 30 < 0: refused
    add(50, 2000, 1, 0, 0, [(50, 0), (775, 200), (2000, 200)])                      # target of 900 bases: window 1 starts at 925 >= 900: refused; window 2 too
    add(0, 1500, 4, 0, 0, [(0, 0), (1500, 0)])                                      # target of 760 bases: window 0 short by 15 + 62 - ... : aux_end > 0; window 1 refused
    add(20, 1552, 3, 400, 0, [(20, 0), (1552, 0)])                                  # last window [1550, 1552]: 3 bases, threshold 0
    add(700, 2300, 5, 100, 0, [(775, 4), (2300, 4)])                                # window 0 starts at 700 < the first site: unresolved
    add(0, 1550, 6, 30, 0, [(0, 0), (1550, 7)])                                     # window 2 starts AT the last site: takes the last shift
    ol = np.stack(rows); fc = np.concatenate(fcs); fo = np.concatenate([[0], np.cumsum([len(f) for f in fcs])]).astype(np.uint64)
    T, infos = M.read_tasks(ol, fc, fo, lengths, wl, e_rate, with_info=True)
    by = {(i, w): f for i, w, f in infos}
    assert by[(1, 0)]["refused"] and by[(2, 1)]["refused"] and by[(2, 2)]["refused"] and by[(3, 1)]["refused"]
    assert by[(0, 0)]["aux_beg"] > 0 and by[(3, 0)]["aux_end"] > 0 and not by[(3, 0)]["refused"]
    assert by[(4, 2)]["thre"] == 0 and by[(4, 2)]["q_l"] == 3
    assert by[(5, 0)]["unresolved"] and by[(6, 2)]["shift"] == 7 and by[(0, 2)]["shift"] == -20 and by[(0, 1)]["shift"] == 0
    total, n_raw, want = _check(lengths, [(ol, fc, fo)], 0, wl, e_rate)
    assert total == T.shape[0] == len(infos) - sum(f["refused"] or f["unresolved"] for _, _, f in infos) and total >= 10


def test_unpack_without_the_cigars_or_with_other_lengths_is_refused():
    rs, _ = scenario_reads("hifi")
    o = scenario_oracle("hifi")
    reads = [o.lchain(r)[:3] for r in range(4, 9)]
    d, e, keep, want, stored, _ = _views(rs.lengths, reads, 4, 775, 0.04)
    i = max(range(len(reads)), key=lambda k: want[k].shape[0])
    m = want[i].shape[0]
    n, t, r = _unpack(e, d, rs.lengths, 4 + i, m - 1)
    assert n == m and (t == 0x5A).all()                                       # cap too small: nothing written
    other = rs.lengths.copy(); other[[int(y) for y in reads[i][0][:, 4]]] = 120
    assert _unpack(e, d, other, 4 + i, 10_000)[0] == U64_MAX
    d.fc = None
    assert _unpack(e, d, rs.lengths, 4 + i, 10_000)[0] == U64_MAX              # the decoder needs the delivered fake cigars
    for rid in (0, 3, 9, 10**9):
        assert _unpack(e, d, rs.lengths, rid, 100)[0] == 0
