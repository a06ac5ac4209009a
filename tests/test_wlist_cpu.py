"""The window-list model's host side, no GPU: tests/wlist_model.py driven by the oracle over the oracle's own overlaps, primary results and rescue.  The model
asserts on the way that the cleared traced function finds every preset (err, pe) again and that a backward window's or an anchor's trace gives the rescue's
record; here every record is held against its own cigar: the entries consume the window's bases and the target bases y_start .. y_end, and their
non-match steps add up to err.  And tests/golden/wlist.npz (the reference's own functions, tests/golden/make_golden_wlist.py): the model over the oracle gives
the recorded records, cigars and counts on the fixture's sampled reads."""
import numpy as np
import pytest

from helpers import scenario_reads, scenario_oracle
import rescue_model as RM
import wlist_model as WM


@pytest.mark.parametrize("name,wl,e_rate,stride", [("hifi", 775, 0.04, 6), ("hifi", 775, 0.004, 4), ("ont", 375, 0.015, 6), ("fz2", 1500, 0.006, 1)])
def test_records_agree_with_their_cigars(name, wl, e_rate, stride):
    rs, _ = scenario_reads(name)
    o = scenario_oracle(name)
    align, trace = RM.oracle_aligner(o), WM.oracle_tracer(o)
    seen, n = {}, 0
    for r in range(0, rs.n, stride):
        ol, fc, fo, _ = o.lchain(r)
        T = RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate)
        res = o.window_ed(T) if T.shape[0] else np.zeros((0, 2), dtype=np.int32)
        rr, ww = WM.read_wlist(ol, fc, fo, rs.lengths, wl, e_rate, res, align, trace)
        for z, q, (wins, cigs, ev, swept, tried) in zip(ol, rr, ww):
            assert (wins.shape[0] == 0) == (not q["verdict"] or q["align_length"] == 0)
            assert (np.diff(wins[:, 0]) > 0).all()
            for x, c in zip(wins, cigs):
                w, ys, ye, err, thre, src, rep, untr = [int(v) for v in x]
                ql = min((w + 1) * wl - 1, int(z[2])) + 1 - max(w * wl, int(z[1]))
                if untr:
                    assert c == ()
                    continue
                ops = [(e >> 14, e & 0x3fff) for e in c]
                assert sum(k for op, k in ops if op != 2) == ql and sum(k for op, k in ops if op != 3) == ye + 1 - ys and sum(k for op, k in ops if op) == err <= thre, (r, x, c)
                assert all(a[0] != b[0] for a, b in zip(ops, ops[1:]))          # runs, not steps
                n += 1
            for e in ev:
                seen[e] = seen.get(e, 0) + 1
    assert n > 20 and seen.get("primary_traced") and seen.get("backward_traced") and seen.get("anchor_traced"), seen


def test_match_run_splits_like_push_trace():
    assert WM.match_run(775) == (775,) and WM.match_run(0x3fff) == (0x3fff,) and WM.match_run(0x3fff + 5) == (0x3fff, 5) and WM.match_run(2 * 0x3fff) == (0x3fff, 0x3fff)


GOLD_KEYS = {"hifi": "hifi", "ont": "ont", "hifi004": "hifi", "ont015": "ont", "fz2w": "fz2", "nn200": "nn", "hifi375": "hifi"}


@pytest.mark.parametrize("key", sorted(GOLD_KEYS))
def test_model_over_the_oracle_equals_the_reference_fixture(key):
    G = WM.gold()
    name = GOLD_KEYS[key]
    wl, e_rate = int(G[key + "_cfg"][0]), float(G[key + "_cfg"][1])
    rs, _ = scenario_reads(name)
    o = scenario_oracle(name)
    align, trace = RM.oracle_aligner(o), WM.oracle_tracer(o)
    want = WM.gold_lists(G, key)
    q = n = 0
    for r in G[key + "_reads"]:
        ol, fc, fo, _ = o.lchain(int(r))
        T = RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate)
        res = o.window_ed(T) if T.shape[0] else np.zeros((0, 2), dtype=np.int32)
        for wins, cigs, ev, swept, tried in WM.read_wlist(ol, fc, fo, rs.lengths, wl, e_rate, res, align, trace)[1]:
            gw, gc, gs, gt = want[q]
            assert wins.shape == gw.shape and (wins == gw).all() and list(cigs) == gc and (swept, tried) == (gs, gt), (int(r), q)
            q += 1; n += wins.shape[0]
    assert q == len(want) and n > 0
