"""The decoder of the rescue stage's delivered results (hao_unpack_rescue, include/hao.h) is a pure host function of three views of a batch.  Here the views
are built by hand - overlaps in their 32-byte wire form, a 16-byte record per overlap, record offsets, 16-byte window records - from what tests/rescue_model.py
gives over the oracle for a range of reads, and the decoder must hand back the model's records read by read.  Then its argument errors and the checks
that refuse views that do not belong together.  No GPU involved: the device side is checked by tests/test_gpu_rescue.py."""
import ctypes as C

import numpy as np
import pytest

from hifiasm_amd import api
from helpers import scenario_reads, scenario_oracle
import rescue_model as RM

U64_MAX = 2**64 - 1
WL, ER = 775, 0.004


def _views(lo, hi):
    rs, _ = scenario_reads("hifi")
    o = scenario_oracle("hifi")
    align = RM.oracle_aligner(o)
    ols, per = [], []
    for r in range(lo, hi):
        ol, fc, fo, _ = o.lchain(r)
        T = RM.M.read_tasks(ol, fc, fo, rs.lengths, WL, ER)
        res = o.window_ed(T) if T.shape[0] else np.zeros((0, 2), dtype=np.int32)
        ols.append(ol); per.append(RM.read_rescue(ol, fc, fo, rs.lengths, WL, ER, res, align))
    n = hi - lo
    ol_off = np.zeros(n + 1, dtype=np.uint64); ol_off[1:] = np.cumsum([o_.shape[0] for o_ in ols])
    allo = np.concatenate(ols).reshape(-1, 12)
    wire = np.stack([allo[:, 4] | (allo[:, 7] << 31), allo[:, 1], allo[:, 2], allo[:, 5], allo[:, 6], allo[:, 8], allo[:, 10], allo[:, 11]], axis=1).astype(np.uint32).copy()
    flat = [w for p in per for w in p]
    ov = np.zeros(len(flat), dtype=api.RESCUE_OVLP)
    woff = np.zeros(len(flat) + 1, dtype=np.uint64)
    raws = []
    for i, w in enumerate(flat):
        ov[i] = (w["verdict"], w["flags"], w["exit_win"], w["align_length"], w["n_rescued"])
        W = w["wins"]
        raw = np.zeros((W.shape[0], 4), dtype=np.uint32)
        raw[:, 0] = W[:, 1].astype(np.int32).view(np.uint32); raw[:, 1] = W[:, 2].astype(np.int32).view(np.uint32); raw[:, 2] = W[:, 0]
        raw[:, 3] = W[:, 3] | (W[:, 4] << 8) | (W[:, 5] << 16) | (W[:, 6] << 18)
        raws.append(raw); woff[i + 1] = woff[i] + W.shape[0]
    wins = np.concatenate(raws + [np.zeros((1, 4), dtype=np.uint32)])
    d = api.Delivery(); d.rid_lo, d.n_reads, d.n_ol = lo, n, allo.shape[0]; d.ol_off, d.ol = ol_off.ctypes.data, wire.ctypes.data
    e = api.EdDelivery(); e.window, e.placement, e.e_rate = WL, api.PLACE_REF, ER
    r = api.RescueDelivery(); r.n_ol, r.n_wins, r.n_rescued = len(flat), int(woff[-1]), int(ov["n_rescued"].sum())
    r.ovlp, r.win_off, r.wins = ov.ctypes.data, woff.ctypes.data, wins.ctypes.data
    return rs, d, e, r, per, [ol_off, wire, ov, woff, wins]


@pytest.fixture(scope="module")
def views():
    return _views(20, 36)


def test_unpack_returns_the_models_records(views):
    rs, d, e, r, per, keep = views
    n_w = 0
    for k, rid in enumerate(range(20, 36)):
        ov, wins = api.unpack_rescue(d, e, r, rs.lengths, rid)
        assert ov.shape[0] == len(per[k]) == len(wins)
        for i, w in enumerate(per[k]):
            assert tuple(int(x) for x in ov[i]) == (w["verdict"], w["flags"], w["exit_win"], w["align_length"], w["n_rescued"]), (rid, i)
            assert wins[i].shape == w["wins"].shape and (wins[i] == w["wins"]).all(), (rid, i)
            n_w += wins[i].shape[0]
    assert n_w == r.n_wins and n_w > 50


def test_unpack_argument_errors_and_refusals(views):
    rs, d, e, r, per, keep = views
    L = np.ascontiguousarray(rs.lengths, dtype=np.uint32)
    lp = L.ctypes.data_as(C.POINTER(C.c_uint32))
    f = api.lib().hao_unpack_rescue
    n = len(per[3]); m = sum(w["wins"].shape[0] for w in per[3])
    assert n > 0 and m > 0
    ov = np.full(n, 0x5A, dtype=np.uint8).repeat(16).view(api.RESCUE_OVLP); wo = np.full(n + 1, 7, dtype=np.uint64); wi = np.full((m, 4), 0x5A5A5A5A, dtype=np.uint32)
    args = (ov.ctypes.data_as(C.c_void_p), wo.ctypes.data_as(C.POINTER(C.c_uint64)), wi.ctypes.data_as(C.c_void_p))
    for bad in ((None, C.byref(e), C.byref(r), lp), (C.byref(d), None, C.byref(r), lp), (C.byref(d), C.byref(e), None, lp), (C.byref(d), C.byref(e), C.byref(r), None)):
        assert f(*bad, 23, *args, n, m) == U64_MAX                                          # a NULL view or no lengths
    assert f(C.byref(d), C.byref(e), C.byref(r), lp, 19, *args, n, m) == 0                  # reads outside the batch
    assert f(C.byref(d), C.byref(e), C.byref(r), lp, 36, *args, n, m) == 0
    for caps, ptrs in (((n - 1, m), args), ((n, m - 1), args), ((n, m), (None, args[1], args[2])), ((n, m), (args[0], None, args[2])), ((n, m), (args[0], args[1], None))):
        assert f(C.byref(d), C.byref(e), C.byref(r), lp, 23, *ptrs, *caps) == n             # too small or NULL outputs: the count, nothing written
        assert (wo == 7).all() and (wi == 0x5A5A5A5A).all() and (ov.view(np.uint8) == 0x5A).all()
    assert f(C.byref(d), C.byref(e), C.byref(r), lp, 23, *args, n, m) == n and int(wo[n]) == m and int(wo[0]) == 0
    e2 = api.EdDelivery(); e2.window, e2.placement = WL, api.PLACE_DIAG                    # a diagonal-placed ED view
    assert f(C.byref(d), C.byref(e2), C.byref(r), lp, 23, *args, n, m) == U64_MAX
    r2 = api.RescueDelivery(); r2.n_ol, r2.n_wins, r2.ovlp, r2.win_off, r2.wins = r.n_ol - 1, r.n_wins, r.ovlp, r.win_off, r.wins      # another batch's overlap count
    assert f(C.byref(d), C.byref(e), C.byref(r2), lp, 23, *args, n, m) == U64_MAX
    woff = keep[3]; first = int(np.flatnonzero(np.diff(woff.astype(np.int64)) > 0)[0]); rid_bad = 20 + int(np.searchsorted(keep[0], first, side="right")) - 1
    wins = keep[4]; old = int(wins[int(woff[first]), 2])
    wins[int(woff[first]), 2] = 10_000                                                      # a record in a window its overlap does not cover
    try:
        assert f(C.byref(d), C.byref(e), C.byref(r), lp, rid_bad, None, None, None, 0, 0) == U64_MAX
    finally:
        wins[int(woff[first]), 2] = old
    Ls = L.copy(); Ls[rid_bad] = 1                                                          # lengths of another read set: the record lies beyond the read's grid
    assert f(C.byref(d), C.byref(e), C.byref(r), Ls.ctypes.data_as(C.POINTER(C.c_uint32)), rid_bad, None, None, None, 0, 0) == U64_MAX
