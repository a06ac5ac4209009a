"""The decoder of the delivered window lists (hao_unpack_wlist, include/hao.h) is a pure host function of four views of a batch.  Here the views are built by
hand - overlaps in their wire form, the rescue stage's per-overlap records, record offsets, 16-byte window records, entry offsets, entries - from what
tests/wlist_model.py gives over the oracle for a range of reads, and the decoder must hand back the model's lists read by read.  Then its argument errors and
every check that refuses views that do not belong together.  No GPU involved: the device side is checked by tests/test_gpu_wlist.py."""
import ctypes as C

import numpy as np
import pytest

from hifiasm_amd import api
from helpers import scenario_reads, scenario_oracle
import rescue_model as RM
import wlist_model as WM

U64_MAX = 2**64 - 1
WL, ER = 775, 0.004
LO, HI = 20, 36


def _views(lo, hi):
    rs, _ = scenario_reads("hifi")
    o = scenario_oracle("hifi")
    align, trace = RM.oracle_aligner(o), WM.oracle_tracer(o)
    ols, per = [], []
    for r in range(lo, hi):
        ol, fc, fo, _ = o.lchain(r)
        T = RM.M.read_tasks(ol, fc, fo, rs.lengths, WL, ER)
        res = o.window_ed(T) if T.shape[0] else np.zeros((0, 2), dtype=np.int32)
        ols.append(ol); per.append(WM.read_wlist(ol, fc, fo, rs.lengths, WL, ER, res, align, trace))
    n = hi - lo
    ol_off = np.zeros(n + 1, dtype=np.uint64); ol_off[1:] = np.cumsum([o_.shape[0] for o_ in ols])
    allo = np.concatenate(ols).reshape(-1, 12)
    wire = np.stack([allo[:, 4] | (allo[:, 7] << 31), allo[:, 1], allo[:, 2], allo[:, 5], allo[:, 6], allo[:, 8], allo[:, 10], allo[:, 11]], axis=1).astype(np.uint32).copy()
    rflat = [w for p in per for w in p[0]]; wflat = [w for p in per for w in p[1]]
    ov = np.zeros(len(rflat), dtype=api.RESCUE_OVLP)
    for i, w in enumerate(rflat):
        ov[i] = (w["verdict"], w["flags"], w["exit_win"], w["align_length"], w["n_rescued"])
    woff = np.zeros(len(wflat) + 1, dtype=np.uint64); raws, coff, cig = [], [0], []
    for i, (W, cs, ev, sw, nt) in enumerate(wflat):
        raw = np.zeros((W.shape[0], 4), dtype=np.uint32)
        raw[:, 0] = W[:, 1].astype(np.int32).view(np.uint32); raw[:, 1] = W[:, 2].astype(np.int32).view(np.uint32); raw[:, 2] = W[:, 0]
        raw[:, 3] = W[:, 3] | (W[:, 4] << 8) | (W[:, 5] << 16) | (W[:, 6] << 18) | (W[:, 7] << 19)
        raws.append(raw); woff[i + 1] = woff[i] + W.shape[0]
        for c in cs:
            cig.extend(c); coff.append(len(cig))
    wins = np.concatenate(raws + [np.zeros((1, 4), dtype=np.uint32)]); coff = np.array(coff, dtype=np.uint64); cig = np.array(cig + [0], dtype=np.uint16)
    d = api.Delivery(); d.rid_lo, d.n_reads, d.n_ol = lo, n, allo.shape[0]; d.ol_off, d.ol = ol_off.ctypes.data, wire.ctypes.data
    e = api.EdDelivery(); e.window, e.placement, e.e_rate = WL, api.PLACE_REF, ER
    r = api.RescueDelivery(); r.n_ol, r.ovlp = len(rflat), ov.ctypes.data
    w = api.WlistDelivery(); w.n_ol, w.n_wins, w.n_cigar = len(wflat), int(woff[-1]), int(coff[-1])
    w.win_off, w.wins, w.cig_off, w.cigars = woff.ctypes.data, wins.ctypes.data, coff.ctypes.data, cig.ctypes.data
    return rs, d, e, r, w, per, dict(ol_off=ol_off, wire=wire, ov=ov, woff=woff, wins=wins, coff=coff, cig=cig)


@pytest.fixture(scope="module")
def views():
    return _views(LO, HI)


def test_unpack_returns_the_models_lists(views):
    rs, d, e, r, w, per, keep = views
    n_w = n_c = 0
    for k, rid in enumerate(range(LO, HI)):
        got = api.unpack_wlist(d, e, r, w, rs.lengths, rid)
        assert len(got) == len(per[k][1])
        for (gw, gc), (ww, wc, ev, sw, nt) in zip(got, per[k][1]):
            assert gw.shape == ww.shape and (gw == ww).all(), rid
            assert len(gc) == len(wc) and all(tuple(int(x) for x in a) == tuple(b) for a, b in zip(gc, wc)), rid
            n_w += gw.shape[0]; n_c += sum(len(c) for c in gc)
    assert n_w == w.n_wins > 200 and n_c == w.n_cigar > n_w


def test_unpack_argument_errors_and_refusals(views):
    rs, d, e, r, w, per, keep = views
    L = np.ascontiguousarray(rs.lengths, dtype=np.uint32)
    lp = L.ctypes.data_as(C.POINTER(C.c_uint32))
    f = api.lib().hao_unpack_wlist
    rid = LO + 3
    lists = per[3][1]
    n = len(lists); m = sum(x[0].shape[0] for x in lists); k = sum(len(c) for x in lists for c in x[1])
    assert n > 0 and m > 0 and k > 0
    wo = np.full(n + 1, 7, dtype=np.uint64); wi = np.full((m, 4), 0x5A5A5A5A, dtype=np.uint32); co = np.full(m + 1, 7, dtype=np.uint64); cg = np.full(k, 0x5A5A, dtype=np.uint16)
    u64p = C.POINTER(C.c_uint64)
    args = (wo.ctypes.data_as(u64p), wi.ctypes.data_as(C.c_void_p), co.ctypes.data_as(u64p), cg.ctypes.data_as(C.c_void_p))
    V = (C.byref(d), C.byref(e), C.byref(r), C.byref(w), lp)
    for i in range(5):                                                                       # a NULL view or no lengths
        bad = list(V); bad[i] = None
        assert f(*bad, rid, *args, n, m, k) == U64_MAX
    assert f(*V, LO - 1, *args, n, m, k) == 0 and f(*V, HI, *args, n, m, k) == 0             # reads outside the batch
    untouched = lambda: (wo == 7).all() and (wi == 0x5A5A5A5A).all() and (co == 7).all() and (cg == 0x5A5A).all()
    for caps in ((n - 1, m, k), (n, m - 1, k), (n, m, k - 1)):                              # caps too small: the count, nothing written
        assert f(*V, rid, *args, *caps) == n and untouched()
    for i in range(4):                                                                       # a NULL output
        ptrs = list(args); ptrs[i] = None
        assert f(*V, rid, *ptrs, n, m, k) == n and untouched()
    assert f(*V, rid, *args, n, m, k) == n and int(wo[0]) == 0 and int(wo[n]) == m and int(co[0]) == 0 and int(co[m]) == k

    def refused(rid_=rid):
        return f(*V, rid_, None, None, None, None, 0, 0, 0) == U64_MAX
    assert not refused()
    e2 = api.EdDelivery(); e2.window, e2.placement = WL, api.PLACE_DIAG                     # a diagonal-placed ED view
    assert f(C.byref(d), C.byref(e2), C.byref(r), C.byref(w), lp, rid, *args, n, m, k) == U64_MAX
    for view, field in ((r, "n_ol"), (w, "n_ol")):                                           # overlap counts that differ
        old = getattr(view, field); setattr(view, field, old - 1)
        try:
            assert refused()
        finally:
            setattr(view, field, old)
    for field in ("n_wins", "n_cigar"):                                                      # totals that the offsets do not add up to
        old = getattr(w, field); setattr(w, field, old + 1)
        try:
            assert refused()
        finally:
            setattr(w, field, old)
    woff, wins, coff, ov, ol_off = keep["woff"], keep["wins"], keep["coff"], keep["ov"], keep["ol_off"]
    o0 = int(ol_off[3]); i = o0 + int(np.flatnonzero(np.diff(woff[o0:int(ol_off[4]) + 1].astype(np.int64)) > 1)[0]); g = int(woff[i])      # an overlap of the read with two records or more

    def poke(arr, idx, val):
        old = arr[idx].copy(); arr[idx] = val
        try:
            assert refused()
        finally:
            arr[idx] = old
    poke(woff, i + 1, int(woff[i]) - 1 if int(woff[i]) else int(woff[-1]) + 5)                # record offsets that do not ascend / run past the total
    poke(woff, i + 1, int(woff[-1]) + 5)
    poke(coff, g + 1, int(coff[g + 2]) + 1)                                                  # entry offsets that do not ascend
    poke(coff, g + 1, int(coff[-1]) + 5)
    poke(wins, (g, 2), 10_000)                                                               # a record in a window its overlap does not cover
    poke(wins, (g + 1, 2), int(wins[g, 2]))                                                  # windows that do not ascend
    vold = ov["verdict"][i]; ov["verdict"][i] = 0                                            # a record in an overlap whose delivered verdict is 0
    try:
        assert refused()
    finally:
        ov["verdict"][i] = vold
    Ls = L.copy(); Ls[rid] = 1                                                               # lengths of another read set: the record lies beyond the read's grid
    assert f(C.byref(d), C.byref(e), C.byref(r), C.byref(w), Ls.ctypes.data_as(C.POINTER(C.c_uint32)), rid, None, None, None, None, 0, 0, 0) == U64_MAX
    assert not refused()
