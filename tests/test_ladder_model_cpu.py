"""tests/ladder_model.py against tests/golden/ladder.npz (the reference's own alignments under the model's control flow, tests/golden/make_golden_ladder.py):
  * the model with the oracle restatement's traced alignments (hao_or_window_trace) as aligner reproduces the fixture's records and cigars.  The restatement holds
    the 64- and 128-bit functions only, so an attempt whose band has three words or more takes the fixture's recorded alignment of the same task, and every one- and
    two-word alignment of the fixture's table is held against the restatement;
  * the threshold arithmetic - the model's and, through hao_ladder_thresholds, the function the kernel calls - agree over ql = 1 .. 10 000 and a grid of
    estimate_err, e_rate and maxe, and match a table of hand-checked values."""
import os

import numpy as np

from helpers import scenario_reads, scenario_oracle, GOLDEN
import ladder_model as LM


def _gold():
    z = np.load(os.path.join(GOLDEN, "ladder.npz"))
    return {k: z[k] for k in z.files}


def test_model_over_the_oracle_equals_the_fixture():
    g = _gold()
    rs, _ = scenario_reads("ont")
    o = scenario_oracle("ont")
    e_rate, maxl, maxe = float(g["cfg"][0]), int(g["cfg"][1]), int(g["cfg"][2])
    tab = {}
    for k in range(g["tab_task"].shape[0]):
        tab[(int(g["tab_mode"][k]), tuple(int(x) for x in g["tab_task"][k]))] = tuple(int(x) for x in g["tab_res"][k]) + (tuple(int(x) for x in g["tab_cig"][int(g["tab_cig_off"][k]):int(g["tab_cig_off"][k + 1])]),)
    oracle = LM.oracle_aligner(o)
    n_or = [0, 0]

    def aligner(mode, task):
        want = tab[(mode, tuple(int(x) for x in task))]
        if LM.nword(task[8]) > 2:
            n_or[1] += 1
            return want
        got = oracle(mode, task)
        assert got == want, (mode, task, got, want)
        n_or[0] += 1
        return got
    ctx, seen = {}, set()
    for k, q in enumerate(g["req"]):
        r, i = int(q[0]), int(q[1])
        if r not in ctx:
            ctx[r] = o.lchain(r)
        ol, fc, fo, _ = ctx[r]
        assert (ol[i] == g["ovlp"][k]).all()
        rec, cig = LM.ladder(ol[i], fc[int(fo[i]):int(fo[i + 1])], rs.lengths, [0] + [int(x) for x in q[2:]], e_rate, maxl, maxe, aligner, seen)
        assert tuple(int(x) for x in g["res"][k]) == tuple(int(x) for x in rec), (k, q, rec, g["res"][k])
        assert tuple(int(x) for x in g["cig"][int(g["cig_off"][k]):int(g["cig_off"][k + 1])]) == cig, k
    assert n_or[0] > 100 and n_or[1] > 20
    assert {"rung1", "rung2", "rung3", "rung4", "no_success", "gate_maxl", "gate_maxe", "rung_skipped", "capped_at_ql", "init_waln_refusal"} <= seen


def test_threshold_arithmetic():
    from hifiasm_amd import api
    # hand-checked against Correct.cpp:14354-14360 and :14599-14631
    assert [LM.scale_ed_thre(x, 2047) for x in (0, 31, 32, 63, 64, 153, 2047, 5000)] == [31, 31, 63, 63, 95, 159, 2047, 2047]
    assert LM.rungs(300, 5, 0.04, 10000, 2047) == [31, -1, 63, 159]
    assert LM.rungs(60, 40, 0.04, 10000, 2047) == [60, -1, 60, -1]      # (thre0 is the threshold computed before, attempted or not: the capped rung comes again)
    assert LM.rungs(300, 5, 0.04, 299, 2047) == [-1] * 4 and LM.rungs(300, 1706, 0.04, 10000, 2047) == [-1] * 4 and LM.rungs(300, 1705, 0.04, 10000, 2047)[0] == 300
    n = 0
    for maxe in (0, 31, 100, 2047):
        for e_rate in (0.0, 0.004, 0.04, 0.07, 0.3, 1.0):
            for est in (0, 1, 31, 32, 90, 1000, 1705, 1706):
                for ql in list(range(1, 10001, 7)) + [10000]:
                    want = LM.rungs(ql, est, e_rate, 10000, maxe)
                    got, cnt = api.ladder_thresholds(ql, est, e_rate, 10000, maxe)
                    assert got == want and cnt == sum(t >= 0 for t in want), (ql, est, e_rate, maxe, got, want)
                    n += 1
    for ql in range(1, 10001):      # every ql once, at the fixture's parameters
        assert api.ladder_thresholds(ql, 10, 0.07, 2000, 2047)[0] == LM.rungs(ql, 10, 0.07, 2000, 2047)
    assert n > 200000
