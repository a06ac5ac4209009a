"""The rescue of unaligned windows, the early exit and the verdict of align_hc_ed_post_extz on the device (include/hao.h: hao_window_rescue_ref,
hao_fetch_rescue), blocking path.  For every read of every read set at its own configuration and at tighter e_rates on the same reads (so that many windows
fail at first placement), none left out:
  * the per-overlap records (verdict, flags, exit window, align_length, rescued windows) and the window records (rescued windows and traced anchors) equal
    tests/rescue_model.py driven by the oracle live, over the device's own primary results (which tests/test_gpu_refgrid.py holds against the oracle);
  * on the sampled reads of five cases they equal tests/golden/rescue.npz, recorded from the reference's own functions;
  * the categories of the rescue a case is known to hold are met (EXPECT: forward and backward windows, a failed backward step, backward runs stopped by cs and by
    ys < 0, a leading gap, an early exit, a verdict 0 without an exit, a verdict 1 that the rescue made); each case prints what it met;
  * the blocking contract: HAO_EINVAL without hao_window_ed_ref on the batch, after another window-alignment call - host-fed, or hao_window_ed_grid whatever
    its pair count - after a new batch; fetch argument errors; HAO_DELIVER_TRACE on a reference-placed context still fails with HAO_EUNSUPP;
  * the residency table of the window-alignment calls, row by row on one engine.
Streamed (HAO_DELIVER_OL | HAO_DELIVER_ED | HAO_DELIVER_RESCUE after hao_deliver_ed_config_ref, batches of 64 and 257 reads): what hao_unpack_rescue hands back equals
the blocking path's results over the same ranges; a batch without the part, before and after one with it, has the byte count and contents it has without
the feature, and the part adds exactly 16 bytes per overlap, the offsets and 16 bytes per record; HAO_DELIVER_RESCUE without HAO_DELIVER_ED or on a
diagonal-placed context fails with HAO_EINVAL; hao_unpack_rescue's argument errors."""
import os

import numpy as np
import pytest

from helpers import scenario_reads, scenario_oracle, scenario_engine, MANY_SLICES
import rescue_model as RM

pytestmark = pytest.mark.gpu
NOALN = 2**31 - 1
# (read set, window, e_rate): the grid's own configurations, then tighter e_rates - ont's 1 % reads at 1 % and 1.5 %, hifi's 0.2 % reads at 0.4 %, small windows
CASES = [("hifi", 775, 0.04), ("ont", 375, 0.07), ("nn", 775, 0.04), ("edge", 775, 0.04),
         ("ont", 375, 0.01), ("ont", 375, 0.015), ("hifi", 775, 0.004), ("hifi", 200, 0.01), ("fz2", 375, 0.012), ("bw001", 500, 0.012), ("fz2", 1500, 0.006)]
# the categories of the rescue a case is known to hold (tests/rescue_model.py names them as it goes; the read sets are seeded, so this is fixed): the tight HiFi
# case walks every branch but a re-placement that is taken and a failed forward step (every window between two aligned ones is a full window, whose rescue
# threshold is 31: it takes the 1500-base windows of the last case to fail one)
EXPECT = {("hifi", 775, 0.004): ("forward", "backward", "backward_failed", "backward_cs", "backward_ys", "leading_gap", "exit", "verdict0_no_exit", "verdict1_by_rescue"),
          ("hifi", 775, 0.04): ("backward", "leading_gap", "verdict1_by_rescue"),
          ("ont", 375, 0.015): ("forward", "backward", "replaced", "exit"),      # (the one re-placement that is taken in these cases: read 110)
          ("fz2", 1500, 0.006): ("forward_failed", "backward", "exit")}           # (more than 31 errors in a full window: the only way a forward step fails)
# cases that tests/golden/rescue.npz (the reference's own functions, make_golden_rescue.py) holds on a sample of their reads
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rescue.npz"))
# hao_window_ed_grid(775, GRID_THRE) forms as many pairs on the hifi set as hao_window_ed_ref(775, 0.04): the count a stale-input check by pair count cannot tell apart
GRID_THRE = 31
GOLD_KEY = {("hifi", 775, 0.04): "hifi", ("ont", 375, 0.07): "ont", ("hifi", 775, 0.004): "hifi004", ("ont", 375, 0.015): "ont015", ("fz2", 1500, 0.006): "fz2w"}


def _engine(name, env=None):
    e, rs = scenario_engine(name, env)
    e.ha_ft_gen(); e.ha_pt_gen()
    return e, rs


def check_read(e, r, want, seen):
    """want: tests/rescue_model.py's overlaps of read r"""
    ov, wins = e.fetch_rescue(r)
    assert ov.shape[0] == len(want) == len(wins)
    n = 0
    for i, w in enumerate(want):
        got = (int(ov["verdict"][i]), int(ov["flags"][i]), int(ov["exit_win"][i]), int(ov["align_length"][i]), int(ov["n_rescued"][i]))
        exp = (w["verdict"], w["flags"], w["exit_win"], w["align_length"], w["n_rescued"])
        assert got == exp, (r, i, got, exp)
        assert wins[i].shape == w["wins"].shape and (wins[i] == w["wins"]).all(), (r, i, wins[i], w["wins"])
        n += w["n_rescued"]
        for c in w["events"]:
            seen[c] = seen.get(c, 0) + 1
    return n, len(want)


def _blocking_case(name, wl, e_rate, env=None, min_states=0):
    """min_states: the overlaps in which the model meets an unaligned window before an aligned one ("gap") - each of them takes a state of the stage's sliced
    rounds - are at least that many, asserted before the stage runs"""
    e, rs = _engine(name, env)
    o = scenario_oracle(name)
    align = RM.oracle_aligner(o)
    seen = {}
    try:
        e.overlap_batch(0, rs.n)
        n, unres = e.window_ed_ref(wl, e_rate)
        assert unres == 0
        T, R = e.fetch_ed_grid(n)
        wants, k = [], 0
        for r in range(rs.n):
            ol, fc, fo, _ = e.h_ec_lchain(r)
            m = RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate).shape[0]
            wants.append(RM.read_rescue(ol, fc, fo, rs.lengths, wl, e_rate, R[k:k + m], align)); k += m
        assert k == n
        assert sum("gap" in w["events"] for want in wants for w in want) >= min_states
        total = e.window_rescue_ref()
        got_total = n_ol = 0
        for r in range(rs.n):
            a, b = check_read(e, r, wants[r], seen)
            got_total += a; n_ol += b
        assert got_total == total
        assert n_ol > 100
        ends = [rs.n - 1] + [r for r in range(rs.n) if e.h_ec_lchain(r)[0].shape[0] == 0][:1]      # the two ends of the records' CSR: the batch's last read, a read without overlaps
        for r in ends:
            ov, wins = e.fetch_rescue(r)
            assert ov.shape[0] == len(wins) == e.h_ec_lchain(r)[0].shape[0], r
        print(f"[rescue] {name} ({wl}, {e_rate}): {n} pairs, {int((R[:, 0] != NOALN).sum())} aligned, {total} windows rescued in {n_ol} overlaps; {dict(sorted(seen.items()))}")
        gk = GOLD_KEY.get((name, wl, e_rate))
        if gk:                                                   # the real reference on the sampled reads
            q = 0
            for r in GOLD[gk + "_reads"]:
                ov, wins = e.fetch_rescue(int(r))
                for i in range(ov.shape[0]):
                    assert [int(ov[f][i]) for f in ("verdict", "flags", "exit_win", "align_length", "n_rescued")] == [int(x) for x in GOLD[gk + "_ovlp"][q]], (r, i)
                    a, b = int(GOLD[gk + "_win_off"][q]), int(GOLD[gk + "_win_off"][q + 1])
                    assert wins[i].shape[0] == b - a and (wins[i] == GOLD[gk + "_wins"][a:b]).all(), (r, i)
                    q += 1
            assert q == GOLD[gk + "_ovlp"].shape[0]
        missing = [c for c in EXPECT.get((name, wl, e_rate), ()) if not seen.get(c)]
        assert not missing, (missing, seen)
    finally:
        e.close()


@pytest.mark.parametrize("name,wl,e_rate", CASES)
def test_rescue_blocking_equals_the_model(name, wl, e_rate):
    _blocking_case(name, wl, e_rate)


@pytest.mark.parametrize("case", [("ont", 375, 0.015)])      # (the emulated twin takes a smaller case of CASES: tests/test_simt_rescue_cpu.py)
def test_rescue_blocking_in_many_slices(case):
    """the case of CASES with the most overlaps that need a rescue (ont at 375 / 1.5 %: 5693 in which the model meets a gap), with a column budget of 8 bytes: the
    rounds run over slices of 256 states, the last one partial, where the default budget makes it one slice"""
    _blocking_case(*case, env=MANY_SLICES, min_states=257)


def test_contract():
    from hifiasm_amd.api import HaoError, DELIVER_OL, DELIVER_ED, DELIVER_TRACE
    e, rs = _engine("hifi")
    try:
        e.overlap_batch(0, rs.n)
        with pytest.raises(HaoError, match=r"\(-2\)"):                          # no hao_window_ed_ref on the batch
            e.window_rescue_ref()
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_rescue(0)
        n, _ = e.window_ed_ref(775, 0.004)
        T, R = e.fetch_ed_grid(n)
        e.window_ed_batch(T[:64])                                              # another window-alignment call: the stage's input is gone
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_rescue_ref()
        e.window_ed_ref(775, 0.004)
        total = e.window_rescue_ref()
        assert total > 0
        ov, wins = e.fetch_rescue(3)
        assert ov.shape[0] == e.h_ec_lchain(3)[0].shape[0] == len(wins)
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_rescue(rs.n)
        assert e.window_rescue_ref() == total                                  # again on the same batch: the same result
        ov2, wins2 = e.fetch_rescue(3)
        assert (ov2 == ov).all() and all((a == b).all() for a, b in zip(wins, wins2))
        e.window_ed_ref(775, 0.04)                                             # a new primary pass: the old rescue results are gone
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_rescue(3)
        e.window_rescue_ref()
        n_ref, _ = e.window_ed_ref(775, 0.04)                                  # a diagonal-placed grid call takes the shared scratch: refused whatever its pair count
        n_grid = e.window_ed_grid(775, GRID_THRE)
        print(f"[rescue] contract: {n_ref} pairs of hao_window_ed_ref, {n_grid} of hao_window_ed_grid(775, {GRID_THRE})")
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_rescue_ref()
        e.window_ed_ref(775, 0.04)
        e.window_rescue_ref()
        e.overlap_batch(1, rs.n)                                               # a new batch
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_rescue(3)
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_rescue_ref()
        e.deliver_ed_config_ref(775, 0.04)                                     # the traced stage in reference placement stays refused
        with pytest.raises(HaoError, match=r"\(-4\)"):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_TRACE)
    finally:
        e.close()


def test_residency_table():
    """what each window-alignment call leaves resident and what it takes away (the residency table), walked row by row on one engine"""
    from hifiasm_amd.api import HaoError
    e, rs = _engine("hifi")

    def refused(f, *a):
        with pytest.raises(HaoError, match=r"\(-2\)"):
            f(*a)
    try:
        e.overlap_batch(0, rs.n)                                               # a new batch: nothing is resident
        for f, a in ((e.window_rescue_ref, ()), (e.window_wlist_ref, ()), (e.fetch_ed_ovlp, (3,)), (e.fetch_rescue, (3,)), (e.fetch_wlist, (3,)), (e.fetch_ed_grid, (1,)), (e.fetch_trace_grid, (1, 1))):
            refused(f, *a)
        n, _ = e.window_ed_ref(775, 0.004)                                     # hao_window_ed_ref: its pairs in the shared scratch, its summaries
        T, R = e.fetch_ed_grid(n)
        s0 = e.fetch_ed_ovlp(3)
        refused(e.fetch_rescue, 3); refused(e.window_wlist_ref)
        tg = e.window_trace_grid(775, 20)                                      # hao_window_trace_grid has buffers of its own: the chain goes on, both stay served
        total = e.window_rescue_ref()
        assert total > 0
        tt = e.fetch_trace_grid(tg[0], tg[2])
        assert tt[0].shape[0] == tg[0] > 0 and int(tt[2][-1]) == tg[2] > 0
        ov, wins = e.fetch_rescue(3)
        out = e.window_wlist_ref()
        wl3 = e.fetch_wlist(3)
        assert (e.fetch_ed_grid(n)[1] == R).all()                              # (the later stages leave the scratch to hao_window_ed_ref's pairs)
        e.window_trace_batch(T[:8], cap=80, mode=0)                            # a host-fed call reuses the scratch: what lies in buffers of its own stays served
        refused(e.fetch_ed_grid, 1); refused(e.fetch_trace_grid, 1, 1); refused(e.fetch_wlist, 3); refused(e.window_wlist_ref)
        assert (e.fetch_ed_ovlp(3) == s0).all()
        ov2, wins2 = e.fetch_rescue(3)
        assert (ov2 == ov).all() and all((a == b).all() for a, b in zip(wins, wins2))
        refused(e.window_rescue_ref)                                           # the rescue stage's input is gone; a stage that starts drops its own results
        refused(e.fetch_rescue, 3)
        assert (e.fetch_ed_ovlp(3) == s0).all()
        e.window_ed_ref(775, 0.004)                                            # the chain again, to its end
        assert e.window_rescue_ref() == total and e.window_wlist_ref() == out
        e.window_trace_grid(775, 20)                                           # (behind the chain: it disturbs nothing)
        assert len(e.fetch_wlist(3)) == len(wl3)
        g = e.window_ed_grid(775, 20)                                          # hao_window_ed_grid takes the scratch: the lists and both stages' input go with it
        assert g > 0 and e.fetch_ed_grid(g)[0].shape[0] == g
        refused(e.fetch_wlist, 3); refused(e.window_wlist_ref)
        assert (e.fetch_ed_ovlp(3) == s0).all() and (e.fetch_rescue(3)[0] == ov).all()
        assert e.fetch_trace_grid(tg[0], tg[2])[0].shape[0] == tg[0]
        refused(e.window_rescue_ref)
        e.overlap_batch(0, 0)                                                  # a batch without reads: every stage runs and has nothing to report
        assert e.window_ed_ref(775, 0.04) == (0, 0) and e.window_rescue_ref() == 0 and e.window_wlist_ref() == (0, 0, 0, 0, 0)
        refused(e.fetch_rescue, 0)                                             # (no read to fetch)
    finally:
        e.close()


@pytest.mark.parametrize("name,bs,cfg", [("hifi", 64, (775, 0.004)), ("hifi", 257, (775, 0.04)), ("ont", 64, (375, 0.015)), ("fz2", 257, (1500, 0.006)), ("edge", 257, (775, 0.04))])
def test_rescue_streamed_equals_blocking(name, bs, cfg):
    from hifiasm_amd.api import DELIVER_OL, DELIVER_ED, DELIVER_RESCUE
    wl, e_rate = cfg
    e, rs = _engine(name)
    try:
        e.deliver_ed_config_ref(wl, e_rate)
        cuts = list(range(0, rs.n, bs)) + [rs.n]
        got, pending, totals = {}, None, []

        def consume(slot, lo, hi):
            d = e.deliver_wait(slot)
            assert (d.rid_lo, d.n_reads) == (lo, hi - lo) and d.ed is not None and d.rs is not None and d.rs.n_ol == d.n_ol
            nw = nr = 0
            for r in range(lo, hi):
                got[r] = e.delivered_rescue(d, r, rs.lengths)
                nw += sum(w.shape[0] for w in got[r][1]); nr += int(got[r][0]["n_rescued"].sum())
            assert nw == d.rs.n_wins and nr == d.rs.n_rescued
            totals.append(nr)

        for lo, hi in zip(cuts[:-1], cuts[1:]):
            slot = e.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE)
            if pending:
                consume(*pending)
            pending = (slot, lo, hi)
        consume(*pending)
        k = 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):                 # the blocking path over the same ranges
            e.overlap_batch(lo, hi)
            e.window_ed_ref(wl, e_rate)
            assert e.window_rescue_ref() == totals[k]; k += 1
            for r in range(lo, hi):
                ov, wins = e.fetch_rescue(r)
                assert (ov == got[r][0]).all() and len(wins) == len(got[r][1]) and all(a.shape == b.shape and (a == b).all() for a, b in zip(wins, got[r][1])), r
        assert sum(totals) > (0 if cfg[1] >= 0.04 and name == "edge" else 5)
    finally:
        e.close()


def test_batches_without_the_part_keep_their_bytes():
    from hifiasm_amd.api import DELIVER_OL, DELIVER_CL, DELIVER_ED, DELIVER_RESCUE
    e, rs = _engine("hifi")
    lo, hi = 2, rs.n - 1
    keys = ["rid_lo", "n_reads", "n_ol", "n_fc", "n_chains", "n_cl", "n_exc", "n_codes", "n_pos", "bytes"]
    try:
        e.deliver_ed_config_ref(775, 0.004)

        def run(parts):
            d = e.deliver_wait(e.overlap_batch_async(lo, hi, parts=parts))
            eds = [e.delivered_ed(d, r, rs.lengths) + (e.delivered_ed_ovlp(d, r),) for r in range(lo, hi)] if parts & DELIVER_ED else None
            return d, {k: int(getattr(d, k)) for k in keys}, [e.delivered_read(d, r) for r in range(lo, hi)], eds
        d0, f0, r0, e0 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED)                                   # before
        assert d0.rs is None
        d1, f1, r1, e1 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED | DELIVER_RESCUE)                  # with the part
        assert d1.rs is not None and d1.rs.n_wins > 100
        assert f1["bytes"] == f0["bytes"] + 16 * f0["n_ol"] + 8 * (f0["n_ol"] + 1) + 16 * int(d1.rs.n_wins)
        d2, f2, r2, e2 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED)                                   # after
        assert f2 == f0 and d2.rs is None
        d3, f3, r3, e3 = run(DELIVER_OL | DELIVER_CL)
        assert d3.rs is None and d3.ed is None and f3["bytes"] < f0["bytes"]
        for rr in (r1, r2, r3):
            for a, b in zip(r0, rr):
                assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
        for ee in (e1, e2):
            for a, b in zip(e0, ee):
                assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
    finally:
        e.close()


def test_streamed_contract():
    from hifiasm_amd.api import HaoError, DELIVER_OL, DELIVER_ED, DELIVER_RESCUE
    e, rs = _engine("hifi")
    try:
        e.deliver_ed_config_ref(775, 0.04)
        with pytest.raises(HaoError, match=r"\(-2\)"):                          # without HAO_DELIVER_ED
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_RESCUE)
        e.deliver_ed_config(375, 15)                                             # a diagonal-placed context
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE)
        slot = e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED)      # a batch that did not ask for the part has no rescue view
        d = e.deliver_wait(slot)
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.deliver_rescue(slot)
        e.deliver_ed_config_ref(775, 0.004)
        d = e.deliver_wait(e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE))
        ov, wins = e.delivered_rescue(d, 3, rs.lengths)
        from hifiasm_amd.api import _arr
        oo = _arr(d.ol_off + 8 * 3, 2, np.uint64)
        assert ov.shape[0] == len(wins) == int(oo[1] - oo[0]) > 0
        import ctypes as C
        from hifiasm_amd import api
        L = np.ascontiguousarray(rs.lengths, dtype=np.uint32); lp = L.ctypes.data_as(C.POINTER(C.c_uint32))
        f = api.lib().hao_unpack_rescue
        assert f(C.byref(d), C.byref(d.ed), None, lp, 3, None, None, None, 0, 0) == 2**64 - 1
        assert f(C.byref(d), C.byref(d.ed), C.byref(d.rs), None, 3, None, None, None, 0, 0) == 2**64 - 1
        assert f(C.byref(d), C.byref(d.ed), C.byref(d.rs), lp, rs.n, None, None, None, 0, 0) == 0
        assert f(C.byref(d), C.byref(d.ed), C.byref(d.rs), lp, 3, None, None, None, 0, 0) == ov.shape[0]
        with pytest.raises(HaoError):
            e.delivered_rescue(e.deliver_wait(e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED)), 3, rs.lengths)
    finally:
        e.close()
