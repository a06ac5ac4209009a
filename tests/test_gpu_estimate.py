"""cal_estimate_err over the window lists the blocking chain leaves on the device (include/hao.h: hao_window_estimate_err, hao_window_ladder_adv with
estimate_err = -1 on a stretch longer than wl, hao_fetch_ladder_adv_estimates) against tests/golden/estimate_err.npz - the reference's own function on the "ont"
scenario's lists at wl 375 / e_rate 0.07 (tests/golden/make_golden_estimate.py).  On one engine and on a context attached to it, over a batch of the first ten
reads (it holds every overlap the fixture names):
  (a) after hao_window_ed_ref -> hao_window_rescue_ref -> hao_window_wlist_ref the stage gives the fixture's value on every real case;
  (b) the ladder with estimate_err = -1 on the fixture's `ladder` stretches (record-to-record gaps, wl + 1, four records, the whole overlap of four overlaps, two per
      strand) gives the records, offsets, cigars and open requests per round of the same requests carrying the fixture's value - the path ladder_adv.npz pins - and
      reports those values as the estimates it ran with;
  (c) the lists serve a second and a third ladder call; a new batch has none, hao_window_ed_grid takes them, and after hao_window_ed_ref has run again there are
      none until the chain has completed again;
  (d) the refusals, each beside a neighbour that passes;
  (e) the stage leaves hao_fetch_wlist, hao_fetch_rescue and a previous ladder call's hao_fetch_ladder_adv serving what they served before it."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_gpu_ladder import _engine

pytestmark = pytest.mark.gpu
BATCH = 10
MAXL, MAXE, FORCE_L = 10000, 2047, 512      # MAX_SIN_L / MAX_SIN_E / FORCE_SIN_L, as in ladder_adv.npz


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "estimate_err.npz"))
    return {k: z[k] for k in z.files}


def _cfg(g):
    return int(g["cfg"][0]), float(g["cfg"][1])


def _chain(e, g):
    wl, e_rate = _cfg(g)
    _, unres = e.window_ed_ref(wl, e_rate)
    assert unres == 0
    e.window_rescue_ref()
    return e.window_wlist_ref()


def _slots(e, g, lists=False):
    """index of each fixture overlap in the batch's ol->list, every read of the batch counted through; the overlap (and, lists = True, its window records as
    hao_fetch_wlist hands them out) is held against the fixture's copy"""
    base, at = {}, 0
    for r in range(BATCH):
        base[r] = at; at += e.h_ec_lchain(r)[0].shape[0]
    out = []
    for s, (r, i) in enumerate(zip(g["ov_read"], g["ov_idx"])):
        assert (e.h_ec_lchain(int(r))[0][int(i)] == g["ovlp"][s]).all(), (r, i)
        if lists:
            W = e.fetch_wlist(int(r))[int(i)][0]
            want = g["wins"][int(g["win_off"][s]):int(g["win_off"][s + 1])]
            assert W.shape == want.shape and (W == want).all(), (r, i)
        out.append(base[int(r)] + int(i))
    return np.array(out, dtype=np.int64), at


def _rows(g, slots, sel, est):
    """requests (ol, mode 0, qs, qe, ts, te, estimate_err) of the fixture's real cases sel; cases without a target interval get (0, 1), which the stage does not read"""
    q = g["real_q"][sel].astype(np.int64)
    rows = np.zeros((q.shape[0], 7), dtype=np.int64)
    rows[:, 0] = slots[q[:, 0]]; rows[:, 2] = q[:, 1]; rows[:, 3] = q[:, 2]
    rows[:, 4] = np.where(q[:, 3] >= 0, q[:, 3], 0); rows[:, 5] = np.where(q[:, 4] >= 0, q[:, 4], 1); rows[:, 6] = est
    return rows


def _ladder_sel(g):
    sel = np.flatnonzero(g["real_cat"] == list(g["cats"]).index("ladder"))
    q = g["real_q"][sel]; wl = _cfg(g)[0]
    ql = q[:, 2] - q[:, 1]
    assert (ql > wl).all() and (ql == wl + 1).any() and (ql > 3 * wl).any() and np.unique(q[:, 0]).size == 4
    assert sorted(int(g["ovlp"][s][7]) for s in np.unique(q[:, 0])) == [0, 0, 1, 1]
    assert (g["real_val"][sel] >= 0).all()
    return sel


def _contexts(e):
    yield e
    v = e.attach()
    try:
        yield v
    finally:
        v.close()


def _adv(e, g, rows, wl=None):
    w, e_rate = _cfg(g)
    return e.window_ladder_adv(rows, e_rate, w if wl is None else wl, MAXL, MAXE, FORCE_L)


def test_stage_and_ladder_equal_the_reference(gold):
    """(a) and (b)"""
    e0, rs = _engine()
    wl, e_rate = _cfg(gold)
    try:
        for e in _contexts(e0):
            e.overlap_batch(0, BATCH)
            out = _chain(e, gold)
            assert out[0] > 1000
            slots, n_ol = _slots(e, gold, lists=True)
            every = np.arange(gold["real_q"].shape[0])
            est = e.window_estimate_err(_rows(gold, slots, every, -1), e_rate, wl)
            bad = np.flatnonzero(est != gold["real_val"])
            assert bad.size == 0, (bad[:10], est[bad[:10]], gold["real_val"][bad[:10]], gold["real_q"][bad[:10]])
            assert (est < 0).any() and e.window_estimate_err(np.zeros((0, 7), dtype=np.int64), e_rate, wl).shape == (0,)
            sel = _ladder_sel(gold)
            want = gold["real_val"][sel]
            r1, o1, c1 = _adv(e, gold, _rows(gold, slots, sel, -1))
            rounds1, est1 = e.ladder_adv_rounds(), e.ladder_adv_estimates()
            r2, o2, c2 = _adv(e, gold, _rows(gold, slots, sel, want))
            rounds2, est2 = e.ladder_adv_rounds(), e.ladder_adv_estimates()
            assert (r1 == r2).all() and (o1 == o2).all() and (c1 == c2).all() and rounds1 == rounds2 and sum(rounds1) > 0
            assert (est1 == want).all() and (est2 == want).all()
            assert int(r1["done"].sum()) >= sel.size // 2 and int(o1[-1]) > 0      # (the stretches follow the records' own diagonals: most align)
            # the other entries of the estimates: ql * e_rate on a short stretch, -1 behind an early return, the request's own
            q = _rows(gold, slots, sel[:3], -1)
            q[0, 3] = q[0, 2] + 100; q[0, 5] = q[0, 4] + 100; q[1, 3] = q[1, 2]; q[2, 6] = 77
            _adv(e, gold, q)
            assert e.ladder_adv_estimates().tolist() == [int(100 * e_rate), -1, 77]
    finally:
        e0.close()


def test_lists_stay_for_the_ladder_and_go_with_what_they_came_from(gold):
    """(c)"""
    from hifiasm_amd.api import HaoError
    e0, rs = _engine()
    wl, e_rate = _cfg(gold)
    try:
        for e in _contexts(e0):
            e.overlap_batch(0, BATCH)
            _chain(e, gold)
            slots, _ = _slots(e, gold)
            sel = _ladder_sel(gold)[:6]
            rows = _rows(gold, slots, sel, -1)

            def refused():
                with pytest.raises(HaoError, match=r"\(-2\)"):
                    _adv(e, gold, rows)
                with pytest.raises(HaoError, match=r"\(-2\)"):
                    e.window_estimate_err(rows, e_rate, wl)
            first = _adv(e, gold, rows)
            with pytest.raises(HaoError, match=r"\(-2\)"):      # (the host-fed call took the shared scratch: hao_fetch_wlist refuses, as before)
                e.fetch_wlist(0)
            for _ in range(2):                                     # a second and a third call
                again = _adv(e, gold, rows)
                assert all((a == b).all() for a, b in zip(first, again))
                assert (e.ladder_adv_estimates() == gold["real_val"][sel]).all()
            assert (e.window_estimate_err(rows, e_rate, wl) == gold["real_val"][sel]).all()
            e.window_ed_ref(wl, e_rate)                            # the chain starts again: none until it has completed
            with pytest.raises(HaoError, match=r"\(-2\)"):      # (the stage, which leaves the chain's input alone; the ladder would take the scratch)
                e.window_estimate_err(rows, e_rate, wl)
            e.window_rescue_ref()
            refused()                                              # (the ladder takes the scratch: the chain has to start over)
            _chain(e, gold)
            assert all((a == b).all() for a, b in zip(first, _adv(e, gold, rows)))
            e.window_ed_grid(wl, 15)                               # the grid call
            refused()
            _chain(e, gold)
            assert (e.window_estimate_err(rows, e_rate, wl) == gold["real_val"][sel]).all()
            e.overlap_batch(0, BATCH)                              # a new batch
            refused()
    finally:
        e0.close()


def test_refusals(gold):
    """(d)"""
    from hifiasm_amd.api import HaoError, DELIVER_OL, DELIVER_ED, DELIVER_RESCUE, DELIVER_WLIST
    e, rs = _engine()
    wl, e_rate = _cfg(gold)
    try:
        e.overlap_batch(0, BATCH)
        slots, n_ol = _slots(e, gold)
        sel = _ladder_sel(gold)[:4]
        want = gold["real_val"][sel]
        rows, explicit = _rows(gold, slots, sel, -1), _rows(gold, slots, sel, want)

        def refused(f, *a):
            with pytest.raises(HaoError, match=r"\(-2\)"):
                f(*a)
        # no chain run on the batch; the explicit estimate passes, and so does -1 on a stretch of at most wl
        refused(_adv, e, gold, rows); refused(e.window_estimate_err, rows, e_rate, wl)
        short = rows.copy(); short[:, 3] = short[:, 2] + wl; short[:, 5] = short[:, 4] + wl
        assert _adv(e, gold, explicit)[0].shape[0] == 4 and _adv(e, gold, short)[0].shape[0] == 4
        _chain(e, gold)
        assert (e.window_estimate_err(rows, e_rate, wl) == want).all()
        # another window length than the lists'
        refused(e.window_estimate_err, rows, e_rate, wl + 1); refused(e.window_estimate_err, rows, e_rate, wl - 1); refused(e.window_estimate_err, rows, e_rate, 0)
        refused(_adv, e, gold, rows, wl - 1); refused(_adv, e, gold, rows, wl + 1)      # (wl + 1: the wl + 1 stretch takes ql * e_rate, the longer ones find no lists)
        assert _adv(e, gold, rows, wl)[0].shape[0] == 4
        refused(e.window_estimate_err, rows, 1.5, wl); refused(e.window_estimate_err, rows, -0.1, wl)
        # a computed estimate that is negative: the stage returns it, the ladder refuses the request; the same request with an estimate of its own passes
        neg = np.flatnonzero((gold["real_val"] < 0) & (gold["real_q"][:, 2] - gold["real_q"][:, 1] > wl))[:2]
        assert neg.size == 2
        q = _rows(gold, slots, neg, -1); q[:, 5] = 300
        assert (e.window_estimate_err(q, e_rate, wl) == gold["real_val"][neg]).all()
        refused(_adv, e, gold, q)
        q[:, 6] = 0
        assert _adv(e, gold, q)[0].shape[0] == 2
        # hao_window_estimate_err: ol, qs, qe out of range, each next to the value just inside
        z = gold["ovlp"][gold["real_q"][sel[0], 0]]
        q_tot = int(rs.lengths[int(z[0])])
        for col, v, inside in ((0, n_ol, n_ol - 1), (2, -1, 0), (3, q_tot + 1, q_tot), (2, int(rows[0, 3]) + 1, int(rows[0, 3]))):
            bad = rows.copy(); bad[0, col] = v
            refused(e.window_estimate_err, bad, e_rate, wl)
            good = rows.copy(); good[0, col] = inside
            if col == 0:
                good[0, 2:4] = 0      # (another overlap: the empty stretch, which every query read has)
            assert e.window_estimate_err(good, e_rate, wl).shape == (4,)
        # a streamed batch: its lists live in the output set
        e.deliver_ed_config_ref(wl, e_rate)
        e.deliver_wait(e.overlap_batch_async(0, BATCH, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST))
        refused(e.window_estimate_err, rows, e_rate, wl); refused(_adv, e, gold, rows)
        assert _adv(e, gold, explicit)[0].shape[0] == 4
    finally:
        e.close()


def _fetch_ladder_adv(e):
    n, rounds = C.c_uint64(), (C.c_uint64 * 5)()
    assert e.L.hao_fetch_ladder_adv(e.h, None, 0, C.byref(n), rounds) == 0
    cig = np.zeros(max(1, n.value), dtype=np.uint16)
    assert e.L.hao_fetch_ladder_adv(e.h, cig.ctypes.data_as(C.c_void_p), cig.shape[0], None, None) == 0
    return cig[:n.value], [int(x) for x in rounds]


def test_the_stage_leaves_what_is_resident(gold):
    """(e): a ladder call, then the chain (which leaves the ladder's results alone), then the stage between two rounds of fetches"""
    e0, rs = _engine()
    wl, e_rate = _cfg(gold)
    try:
        for e in _contexts(e0):
            e.overlap_batch(0, BATCH)
            slots, _ = _slots(e, gold)
            sel = _ladder_sel(gold)[:6]
            _adv(e, gold, _rows(gold, slots, sel, gold["real_val"][sel]))
            _chain(e, gold)

            def snapshot():
                wl_, rs_ = [e.fetch_wlist(r) for r in range(BATCH)], [e.fetch_rescue(r) for r in range(BATCH)]
                flat = [x for per in wl_ for w, c in per for x in [w] + list(c)] + [x for ov, wins in rs_ for x in [ov] + list(wins)]
                cig, rounds = _fetch_ladder_adv(e)
                return flat + [cig, np.array(rounds), e.ladder_adv_estimates()]
            a = snapshot()
            est = e.window_estimate_err(_rows(gold, slots, sel, -1), e_rate, wl)
            assert (est == gold["real_val"][sel]).all()
            b = snapshot()
            assert len(a) == len(b) > 50 and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
            assert a[-3].size > 0 and sum(a[-2].tolist()) > 0
    finally:
        e0.close()
