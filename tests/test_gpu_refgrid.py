"""The window grid in REFERENCE placement on the device (include/hao.h: hao_window_ed_ref, hao_fetch_ed_ovlp, hao_deliver_ed_config_ref): the fake-cigar shift
of a window's target start, one threshold per window, init_waln's admission and clipping.  For every read and every pair of each read set, none left out:
  * blocking: task count, tasks and order equal tests/refgrid_model.py over the batch's overlaps and fake cigars; (err, pe) equal the oracle run live on the same
    tasks and tests/golden/refgrid.npz (the real reference) on the sampled reads; no unresolved window; the per-overlap summaries equal a reduction of the results;
  * streaming (HAO_DELIVER_OL | HAO_DELIVER_ED after hao_deliver_ed_config_ref, batches of 64 and 257 reads): the tasks hao_unpack_ed rebuilds from the delivered
    overlaps and fake cigars, the results and the summaries equal the blocking path's (whose results the blocking test holds against the oracle, every read); a batch without the part and a batch after switching back to
    hao_deliver_ed_config have the byte counts and contents of diagonal placement;
  * the traced stage is not built in reference placement: HAO_DELIVER_TRACE fails with HAO_EUNSUPP on a reference-placed context;
  * argument errors."""
import os

import numpy as np
import pytest

from helpers import ed_tasks_grid_all, scenario_reads, scenario_oracle
import refgrid_model as M

pytestmark = pytest.mark.gpu
NOALN = 2**31 - 1
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refgrid.npz"))
CONFIGS = {"hifi": (775, 0.04), "ont": (375, 0.07), "rr": (775, 0.04), "nn": (775, 0.04), "edge": (775, 0.04), "hifi_15k": (775, 0.04)}
# (read set, window, e_rate, first read, reads left off the end, fixture key).  Every read of every set at its own configuration; then hifi at the ONT
# configuration - the one case in which init_waln refuses a pair of a chained overlap (read 114), so that a refused slot goes through the generators, the
# alignment kernel and the summary kernel - and a batch that does not start at read 0
CASES = [(n, *CONFIGS[n], 0, 0, n if n != "rr" and n != "hifi_15k" else None) for n in CONFIGS] + [("hifi", 375, 0.07, 0, 0, "hifi375"), ("hifi", 775, 0.04, 7, 5, "hifi")]


def _engine(name):
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads(name)
    e = Engine(0, **okw)
    e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
    return e, rs


def _blocking(e, rs, lo, hi, wl, e_rate):
    """-> per read: (overlaps, model tasks, device results, device summaries), after checking tasks, order and count against the model"""
    e.overlap_batch(lo, hi)
    n, unres = e.window_ed_ref(wl, e_rate)
    assert unres == 0
    got_t, got_r = e.fetch_ed_grid(n)
    per, k = {}, 0
    for r in range(lo, hi):
        ol, fc, fo, _ = e.h_ec_lchain(r)
        want = M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate)
        m = want.shape[0]
        assert k + m <= n and (got_t[k:k + m] == want).all(), (r, np.flatnonzero((got_t[k:k + m] != want).any(axis=1))[:5])
        s = e.fetch_ed_ovlp(r)
        assert s.shape == (ol.shape[0], 4)
        assert (s == M.summaries(ol, fc, fo, rs.lengths, wl, e_rate, got_r[k:k + m])).all(), r
        per[r] = (ol, want, got_r[k:k + m], s)
        k += m
    assert k == n
    return per, got_t, got_r


@pytest.mark.parametrize("name,wl,e_rate,first,cut,gold", CASES)
def test_reference_placed_pairs_blocking(name, wl, e_rate, first, cut, gold):
    e, rs = _engine(name)
    o = scenario_oracle(name)
    try:
        lo, hi = first, rs.n - cut
        per, T, R = _blocking(e, rs, lo, hi, wl, e_rate)
        assert T.shape[0] > 200
        want_r = o.window_ed(T)
        assert (R == want_r).all(), np.flatnonzero((R != want_r).any(axis=1))[:10]
        if gold is not None:                                   # the real reference on the sampled reads
            gt, gr, k, seen = GOLD[gold + "_tasks"], GOLD[gold + "_res"], 0, 0
            for r in GOLD[gold + "_reads"]:
                r = int(r)
                m = M.read_tasks(*o.lchain(r)[:3], rs.lengths, wl, e_rate).shape[0]
                if lo <= r < hi:
                    assert (per[r][1] == gt[k:k + m]).all() and (per[r][2] == gr[k:k + m]).all(), r
                    seen += 1
                k += m
            assert k == gt.shape[0] and (seen == len(GOLD[gold + "_reads"]) or first or cut)
        if gold == "hifi375":                                  # the refused pair went through the device: a covered window without a pair, counted by the summary only
            n_win = sum(int(per[r][3][:, 0].sum()) for r in range(lo, hi))
            assert n_win > T.shape[0] and int(per[114][3][:, 0].sum()) > per[114][1].shape[0]
        if T.shape[0] < 60_000:
            assert (e.window_ed_batch(T) == R).all()           # the upload path on the same tasks
        ti = T.astype(np.int64)
        print(f"[ref grid] {name} ({wl}, {e_rate}): {T.shape[0]} pairs, {int((R[:, 0] != NOALN).sum())} aligned, thresholds {sorted(set(ti[:, 8].tolist()))[:4]} .. {int(ti[:, 8].max())}, "
              f"{int((ti[:, 9] > 0).sum())} with aux_beg, {int((ti[:, 2] + ti[:, 9] < ti[:, 6] + 2 * ti[:, 8]).sum())} with aux_end")
    finally:
        e.close()


@pytest.mark.parametrize("name,bs,cfg", [("hifi", 64, None), ("ont", 64, None), ("rr", 257, None), ("nn", 64, None), ("edge", 257, None), ("hifi_15k", 257, None), ("hifi", 64, (375, 0.07))])
def test_reference_placed_pairs_streamed(name, bs, cfg):
    from hifiasm_amd.api import DELIVER_OL, DELIVER_ED, PLACE_REF
    wl, e_rate = cfg or CONFIGS[name]
    e, rs = _engine(name)
    try:
        e.deliver_ed_config_ref(wl, e_rate)
        cuts = list(range(0, rs.n, bs)) + [rs.n]
        got, pending = {}, None

        def consume(slot, lo, hi):
            d = e.deliver_wait(slot)
            assert (d.rid_lo, d.n_reads) == (lo, hi - lo) and d.ed is not None
            assert (d.ed.window, d.ed.placement, d.ed.e_rate, d.ed.unresolved) == (wl, PLACE_REF, e_rate, 0)
            n = 0
            for r in range(lo, hi):
                t, res = e.delivered_ed(d, r)
                got[r] = (t, res, e.delivered_ed_ovlp(d, r)); n += t.shape[0]
            assert n == d.ed.n_pairs
            return d

        for lo, hi in zip(cuts[:-1], cuts[1:]):
            slot = e.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED)
            if pending:
                consume(*pending)
            pending = (slot, lo, hi)
        consume(*pending)
        total = 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):                # the blocking path over the same ranges
            per, T, R = _blocking(e, rs, lo, hi, wl, e_rate)
            for r in range(lo, hi):
                assert got[r][0].shape == per[r][1].shape and (got[r][0] == per[r][1]).all() and (got[r][1] == per[r][2]).all() and (got[r][2] == per[r][3]).all(), r
            total += T.shape[0]
        assert total > 200
        if cfg:                                                # (the case with a refused pair: delivered summaries count a window that has no pair)
            assert sum(int(got[r][2][:, 0].sum()) for r in got) > sum(got[r][0].shape[0] for r in got)
    finally:
        e.close()


def test_other_batches_keep_their_bytes():
    """a batch without the ED part, and a batch after switching back to hao_deliver_ed_config, have the byte counts and contents of diagonal placement; a
    reference-placed batch adds the offsets, 3 bytes per pair and 16 bytes per overlap"""
    from hifiasm_amd.api import DELIVER_OL, DELIVER_CL, DELIVER_ED, PLACE_DIAG
    e, rs = _engine("hifi")
    lo, hi = 2, rs.n - 1
    keys = ["rid_lo", "n_reads", "n_ol", "n_fc", "n_chains", "n_cl", "n_exc", "n_codes", "n_pos", "bytes"]
    try:
        def run(parts):
            d = e.deliver_wait(e.overlap_batch_async(lo, hi, parts=parts))
            return d, {k: int(getattr(d, k)) for k in keys}, [e.delivered_read(d, r) for r in range(lo, hi)]
        d0, f0, r0 = run(DELIVER_OL | DELIVER_CL)
        e.deliver_ed_config_ref(775, 0.04)
        d1, f1, r1 = run(DELIVER_OL | DELIVER_CL)                              # without the part
        assert f1 == f0 and d1.ed is None
        d2, f2, r2 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED)                 # reference placement
        assert f2["bytes"] == f0["bytes"] + (hi - lo + 1) * 8 + 3 * int(d2.ed.n_pairs) + 16 * f0["n_ol"] and int(d2.ed.n_pairs) > 200
        e.deliver_ed_config(375, 15)                                           # switched back: diagonal placement as before
        d3, f3, r3 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED)
        assert (d3.ed.placement, d3.ed.window, d3.ed.thre, d3.ed.e_rate) == (PLACE_DIAG, 375, 15, 0.0) and not d3.ed.ovlp
        assert f3["bytes"] == f0["bytes"] + (hi - lo + 1) * 8 + 3 * int(d3.ed.n_pairs)
        T = []
        for r in range(lo, hi):
            t, res = e.delivered_ed(d3, r)
            want = ed_tasks_grid_all(rs.lengths, [r0[r - lo][0]], r, 375, 15)
            assert t.shape == want.shape and (t == want).all(), r
            T.append((t, res))
        e.overlap_batch(lo, hi)
        n = e.window_ed_grid(375, 15)
        bt, br = e.fetch_ed_grid(n)
        assert (bt == np.concatenate([x[0] for x in T])).all() and (br == np.concatenate([x[1] for x in T])).all()
        for rr in (r1, r2, r3):
            for a, b in zip(r0, rr):
                assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
    finally:
        e.close()


def test_traced_stage_is_refused_in_reference_placement():
    from hifiasm_amd.api import HaoError, DELIVER_OL, DELIVER_ED, DELIVER_TRACE
    e, rs = _engine("hifi")
    try:
        e.deliver_ed_config_ref(775, 0.04)
        with pytest.raises(HaoError, match=r"\(-4\)"):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE)
        assert not hasattr(e, "window_trace_ref")                              # (no reference-placed form of hao_window_trace_grid exists)
        e.deliver_ed_config(375, 15)                                           # diagonal placement: the traced part runs as before
        d = e.deliver_wait(e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE))
        assert d.tr is not None and d.tr.n_traced > 100
    finally:
        e.close()


def test_argument_errors():
    from hifiasm_amd.api import HaoError
    e, rs = _engine("hifi")
    try:
        e.overlap_batch(0, rs.n)
        for w, er in ((0, 0.04), (65535 - 62, 0.04), (70000, 0.04), (775, 0.0), (775, 1.0), (775, -0.1), (775, float("nan"))):
            with pytest.raises(HaoError, match=r"\(-2\)"):
                e.window_ed_ref(w, er)
            with pytest.raises(HaoError, match=r"\(-2\)"):
                e.deliver_ed_config_ref(w, er)
        n, u = e.window_ed_ref(65535 - 63, 0.04)                               # the largest window
        assert n > 0 and u == 0
        n, u = e.window_ed_ref(775, 0.04)
        s = e.fetch_ed_ovlp(3)
        assert s.shape[0] == e.h_ec_lchain(3)[0].shape[0]
        with pytest.raises(HaoError):
            e.fetch_ed_ovlp(rs.n)
        e.overlap_batch(1, rs.n)                                               # a new batch: the summaries belong to the old one
        with pytest.raises(HaoError):
            e.fetch_ed_ovlp(3)
    finally:
        e.close()
