"""f3 with traceback on the device grid (hao_window_trace_grid / hao_fetch_trace_grid, HAO_DELIVER_TRACE): the grid pairs hao_window_ed_grid forms, in the same
order, with the distance-only (err, pe), and - for the pairs that aligned and whose band covers the pattern - the semi-global traced alignment
(ed_band_cal_semi_64_w_absent_diag_trace + gen_trace).  Traced pairs must equal the oracle (bands of one and two words) and the host-fed path
(hao_window_trace_batch(HAO_ALIGN_SEMI), every band; its wide bands are pinned to the reference's *_infi_* functions by test_gpu_zz_new.py::test_wide_bands_trace);
aligned pairs outside that domain keep their distance-only result without a cigar.  The streamed part must equal the blocking path over the same range bit
for bit, with both slots in flight over batches that do not start at read 0.  Then the contract's edges."""
import numpy as np
import pytest

from helpers import ed_tasks_grid_all, scenario_reads, scenario_oracle, scenario_engine, MANY_SLICES

pytestmark = pytest.mark.gpu
NOALN = 2**31 - 1
CASES = [("hifi", 375, 15), ("hifi", 375, 40), ("nn", 375, 15), ("rr", 375, 15), ("hifi", 775, 70), ("nn", 775, 100), ("edge", 100, 3), ("rr", 775, 100)]


def _engine(name, env=None):
    e, rs = scenario_engine(name, env)
    e.ha_ft_gen(); e.ha_pt_gen()
    return e, rs


def _semi_domain(t):
    ti = t.astype(np.int64)
    ai = ti[:, 2] - ti[:, 6] + ti[:, 9]
    return (ai >= 0) & (ai <= 2 * ti[:, 8]) & (ti[:, 6] > ti[:, 9])


def _blocking(e, lo, hi, window, thre):
    e.overlap_batch(lo, hi)
    n, nt, nc, nu = e.window_trace_grid(window, thre)
    t, r, off, cg = e.fetch_trace_grid(n, nc)
    return (n, nt, nc, nu), t, r, off, cg


def _check_traced(e, o, t, r, off, cg, thre):
    """every traced pair against the host-fed path (and the oracle for one- and two-word bands); every untraced one has no cigar"""
    traced = r[:, 1] >= 0
    assert (r[~traced, 5] == 0).all() and (r[~traced, 1] == -1).all()
    assert ((off[1:] - off[:-1]).astype(np.int64) == r[:, 5]).all() and int(off[-1]) == cg.shape[0]
    assert (r[:, 3] == 0).all() and (r[:, 4] == t[:, 6].astype(np.int32) - 1).all()
    idx = np.flatnonzero(traced)
    if idx.size == 0:
        return 0
    cap = 2 * thre + 3
    tt = t[idx]
    refs = [e.window_trace_batch(tt, cap=cap, mode=3)]
    if thre <= 63:
        refs.append(o.window_trace(tt, cap=cap, mode=3))
    for hr, hc in refs:
        assert (r[idx] == hr).all(), idx[np.flatnonzero((r[idx] != hr).any(axis=1))[:10]]
        for j, i in enumerate(idx):
            k = int(r[i, 5])
            assert (cg[int(off[i]):int(off[i + 1])] == hc[j, :k]).all(), i
    return idx.size


def _grid_case(name, window, thre, env=None, min_traced=0):
    """min_traced: the pairs the oracle aligns inside the semi-global domain - the pairs of the sliced sweep - are at least that many (thre <= 63), asserted first"""
    e, rs = _engine(name, env)
    o = scenario_oracle(name)
    try:
        lo, hi = (0, rs.n) if name != "hifi" else (7, rs.n - 5)      # (a batch that does not start at read 0)
        e.overlap_batch(lo, hi)
        ols = [e.h_ec_lchain(q)[0] for q in range(lo, hi)]
        want_t = ed_tasks_grid_all(rs.lengths, ols, lo, window, thre)
        if min_traced:
            assert int(((o.window_ed(want_t)[:, 0] != NOALN) & _semi_domain(want_t)).sum()) >= min_traced
        (n, nt, nc, nu), t, r, off, cg = _blocking(e, lo, hi, window, thre)
        assert n == want_t.shape[0] and (n > 200 or name == "edge")
        assert (t == want_t).all(), np.flatnonzero((t != want_t).any(axis=1))[:10]
        ne = e.window_ed_grid(window, thre)
        _, er = e.fetch_ed_grid(ne)
        assert ne == n and (r[:, [0, 2]] == er).all()                 # every pair's (err, pe) is the distance-only result
        aligned, dom = er[:, 0] != NOALN, _semi_domain(t)
        traced = r[:, 1] >= 0
        assert (traced == (aligned & dom)).all()                      # exactly the aligned pairs inside the semi-global domain get a cigar
        assert nt == int(traced.sum()) and nu == int((aligned & ~dom).sum()) and nc == cg.shape[0]
        assert nt > 0 or name == "edge"
        assert _check_traced(e, o, t, r, off, cg, thre) == nt
        print(f"[trace grid] {name} window {window} thre {thre}: {n} pairs, {nt} traced, {nu} aligned but untraced, {nc} cigar entries")
    finally:
        e.close()


@pytest.mark.parametrize("name,window,thre", CASES)
def test_grid_pairs_traced_on_the_device(name, window, thre):
    _grid_case(name, window, thre)


@pytest.mark.parametrize("case", [("rr", 375, 15)])      # (the emulated twin takes a smaller case of CASES: tests/test_simt_trace_grid_cpu.py)
def test_grid_pairs_traced_in_many_slices(case):
    """the case of CASES with the most traced pairs (rr at 375 / 15: 75 166 of 148 235), with a column budget of 8 bytes: the traced sweep, its scan and its
    compaction walk slices of 256 pairs, the last one partial, where the default budget makes it one slice"""
    _grid_case(*case, env=MANY_SLICES, min_traced=257)


def _parts(which):
    from hifiasm_amd.api import DELIVER_OL, DELIVER_CL, DELIVER_EXACT, DELIVER_ED, DELIVER_TRACE
    return DELIVER_OL | DELIVER_ED | DELIVER_TRACE if which == "ol" else DELIVER_OL | DELIVER_CL | DELIVER_EXACT | DELIVER_ED | DELIVER_TRACE


def _concat(parts_):
    """per-read (tasks, results, cig_off, cigars) -> one batch's arrays with batch-wide offsets"""
    T = np.concatenate([p[0] for p in parts_]) if parts_ else np.zeros((0, 10), np.uint32)
    R = np.concatenate([p[1] for p in parts_]) if parts_ else np.zeros((0, 6), np.int32)
    offs, base = [np.zeros(1, np.uint64)], 0
    for p in parts_:
        offs.append(p[2][1:] + np.uint64(base)); base += int(p[2][-1])
    CG = np.concatenate([p[3] for p in parts_]) if parts_ else np.zeros(0, np.uint16)
    return T, R, np.concatenate(offs), CG


@pytest.mark.parametrize("name,window,thre,parts", [("hifi", 375, 15, "ol"), ("hifi", 375, 40, "all"), ("nn", 375, 15, "all"), ("rr", 375, 15, "ol"),
                                                    ("hifi", 775, 70, "all"), ("nn", 775, 100, "ol"), ("edge", 100, 3, "all")])
def test_streamed_batches_carry_their_traceback(name, window, thre, parts):
    e, rs = _engine(name)
    try:
        e.deliver_ed_config(window, thre)
        lo0 = 3
        cuts = [lo0, lo0 + (rs.n - lo0) // 3, lo0 + 2 * (rs.n - lo0) // 3, rs.n]      # three batches, the first not at read 0
        got, pending = {}, None

        def consume(slot, lo, hi):
            d = e.deliver_wait(slot)
            assert (d.rid_lo, d.n_reads) == (lo, hi - lo) and d.ed is not None and d.tr is not None
            per = [e.delivered_trace(d, q) for q in range(lo, hi)]
            T, R, OFF, CG = _concat(per)
            assert T.shape[0] == d.ed.n_pairs and int((R[:, 1] >= 0).sum()) == d.tr.n_traced and CG.shape[0] == d.tr.n_cigar
            if parts == "all":
                assert d.exact and d.n_cl > 0       # (the other parts still travel beside it)
            got[lo] = (T, R, OFF, CG)

        for lo, hi in zip(cuts[:-1], cuts[1:]):
            slot = e.overlap_batch_async(lo, hi, parts=_parts(parts))
            if pending:                       # batch k is consumed while batch k + 1's copy is (possibly) still in flight
                consume(*pending)
            pending = (slot, lo, hi)
        consume(*pending)
        n_tr = 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):      # each batch against the blocking path over the same range, bit for bit
            (n, nt, nc, nu), t, r, off, cg = _blocking(e, lo, hi, window, thre)
            T, R, OFF, CG = got[lo]
            assert t.shape == T.shape and (t == T).all() and (r == R).all() and (off == OFF).all() and (cg == CG).all(), lo
            n_tr += nt
        assert n_tr > 0 or name == "edge"
        print(f"[trace deliver] {name} window {window} thre {thre} parts {parts}: {n_tr} traced pairs")
    finally:
        e.close()


def test_trace_part_needs_ed_and_a_config():
    from hifiasm_amd.api import HaoError, DELIVER_OL, DELIVER_CL, DELIVER_ED, DELIVER_TRACE
    e, rs = _engine("hifi")
    try:
        with pytest.raises(HaoError):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE)      # no hao_deliver_ed_config yet
        e.deliver_ed_config(375, 15)
        for p in (DELIVER_OL | DELIVER_TRACE, DELIVER_OL | DELIVER_CL | DELIVER_TRACE, DELIVER_TRACE):
            with pytest.raises(HaoError):
                e.overlap_batch_async(0, rs.n, parts=p)                                         # TRACE without ED
        d = e.deliver_wait(e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE))
        assert d.tr.n_traced > 100
        slot = e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED)
        e.deliver_wait(slot)
        with pytest.raises(HaoError):
            e.deliver_trace(slot)                                                                # a slot whose batch did not ask for TRACE
        with pytest.raises(HaoError):
            e.window_trace_grid(375, 128)                                                         # beyond the widest band
        e.overlap_batch(0, rs.n)
        e.window_trace_grid(375, 15)
        e.window_trace_batch(np.zeros((0, 10), np.uint32), mode=3)                                # a host-fed batch reuses the scratch ...
        with pytest.raises(HaoError):
            e.fetch_trace_grid(10, 10)                                                            # ... so the grid's results are gone
    finally:
        e.close()


def test_batch_without_overlaps():
    from hifiasm_amd.api import DELIVER_OL, DELIVER_ED, DELIVER_TRACE
    e, rs = _engine("hifi")
    try:
        e.overlap_batch(5, 5)
        assert e.window_trace_grid(375, 15) == (0, 0, 0, 0)
        t, r, off, cg = e.fetch_trace_grid(0, 0)
        assert t.shape == (0, 10) and off.tolist() == [0] and cg.shape == (0,)
        e.deliver_ed_config(375, 15)
        d = e.deliver_wait(e.overlap_batch_async(5, 5, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE))
        assert d.n_reads == 0 and d.tr.n_traced == 0 and d.tr.n_cigar == 0
        t, r, off, cg = e.delivered_trace(d, 5)
        assert t.shape == (0, 10) and cg.shape == (0,)
    finally:
        e.close()


def test_attached_contexts_have_their_own_grid():
    from hifiasm_amd.api import DELIVER_OL, DELIVER_ED, DELIVER_TRACE
    e, rs = _engine("hifi")
    o = scenario_oracle("hifi")
    v1, v2 = e.attach(), e.attach()
    try:
        v1.deliver_ed_config(375, 15); v2.deliver_ed_config(775, 40)
        lo, hi = 5, rs.n - 4
        s1 = v1.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE)
        s2 = v2.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE)
        for v, s, (w, th) in ((v1, s1, (375, 15)), (v2, s2, (775, 40))):
            d = v.deliver_wait(s)
            assert (d.ed.window, d.ed.thre) == (w, th)
            T, R, OFF, CG = _concat([v.delivered_trace(d, q) for q in range(lo, hi)])
            assert T.shape[0] == d.ed.n_pairs > 200 and int((R[:, 1] >= 0).sum()) == d.tr.n_traced > 100
            assert (T[:, 8] == th).all()
            assert _check_traced(e, o, T, R, OFF, CG, th) == d.tr.n_traced
    finally:
        v1.close(); v2.close(); e.close()


def test_batches_without_trace_are_unchanged():
    """without TRACE a batch's byte count and counts equal a run made before any config was set; with it, the byte count grows by exactly the per-read
    offsets, 4 bytes per pair and 2 bytes per cigar entry"""
    from hifiasm_amd.api import DELIVER_OL, DELIVER_CL, DELIVER_ED, DELIVER_TRACE
    e, rs = _engine("hifi")
    lo, hi = 2, rs.n - 1
    keys = ["rid_lo", "n_reads", "n_ol", "n_fc", "n_chains", "n_cl", "n_exc", "n_codes", "n_pos", "bytes"]
    try:
        def run(parts):
            d = e.deliver_wait(e.overlap_batch_async(lo, hi, parts=parts))
            return d, {k: int(getattr(d, k)) for k in keys}
        d0, f0 = run(DELIVER_OL | DELIVER_CL)
        e.deliver_ed_config(375, 15)
        d1, f1 = run(DELIVER_OL | DELIVER_CL)
        assert f1 == f0 and d1.tr is None
        d2, f2 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED)
        assert d2.tr is None
        d3, f3 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED | DELIVER_TRACE)
        n_pairs, n_cig = int(d3.ed.n_pairs), int(d3.tr.n_cigar)
        assert n_pairs == int(d2.ed.n_pairs) > 200 and n_cig > 0
        assert f3["bytes"] == f2["bytes"] + (hi - lo + 1) * 8 + 4 * n_pairs + 2 * n_cig
        assert {k: f3[k] for k in keys if k != "bytes"} == {k: f0[k] for k in keys if k != "bytes"}
    finally:
        e.close()
