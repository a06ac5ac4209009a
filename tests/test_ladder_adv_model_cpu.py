"""tests/ladder_adv_model.py against tests/golden/ladder_adv.npz (the reference's own alignments under the model's control flow,
tests/golden/make_golden_ladder_adv.py):
  * the model over the fixture's table of recorded alignments reproduces the fixture's records and cigars, and meets every category the generator asserted; every
    one- and two-word alignment of the table is held against the oracle restatement's traced alignments (hao_or_window_trace);
  * the rung arithmetic - the model's and, through hao_ladder_adv_thresholds, the function the kernel calls - agree over a sweep of (ql, estimate_err) and a grid of
    the call's parameters, estimate_err < 0 included, and match hand-checked values."""
import os

import numpy as np

from helpers import scenario_reads, scenario_oracle, GOLDEN
import ladder_model as LM
import ladder_adv_model as AM


def _gold():
    z = np.load(os.path.join(GOLDEN, "ladder_adv.npz"))
    return {k: z[k] for k in z.files}


def test_model_over_the_table_equals_the_fixture():
    g = _gold()
    rs, _ = scenario_reads("ont")
    o = scenario_oracle("ont")
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
    bases = AM.reads_bases(rs)
    ctx, seen = {}, set()
    for k, q in enumerate(g["req"]):
        r, i = int(q[0]), int(q[1])
        if r not in ctx:
            ctx[r] = o.lchain(r)
        ol, fc, fo, _ = ctx[r]
        assert (ol[i] == g["ovlp"][k]).all()
        c = g["cfg"][int(g["grp"][k])]
        cfg = (float(c[0]), int(c[1]), int(c[2]), int(c[3]), int(c[4]))
        req = [0] + [int(x) for x in q[2:]]
        assert not AM.check_request(ol[i], rs.lengths, req, *cfg)
        rec, cig = AM.ladder(ol[i], fc[int(fo[i]):int(fo[i + 1])], rs.lengths, req, *cfg, aligner, bases, seen)
        assert tuple(int(x) for x in g["res"][k]) == tuple(int(x) for x in rec), (k, q, rec, g["res"][k])
        assert tuple(int(x) for x in g["cig"][int(g["cig_off"][k]):int(g["cig_off"][k + 1])]) == cig, k
    assert n_or[0] > 100 and n_or[1] > 20
    assert {"rung1", "rung2", "rung3", "rung4", "rung5", "exact", "no_success", "early_1", "early_0_forced", "early_0_unset_end", "gate_maxl", "gate_est", "estimated",
            "exact_mismatch", "exact_tl_ne_ql", "exact_rev", "clamped_by_dd", "thre_above_ql", "pthre_abandoned", "rung_skipped", "mode3_explicit_aligned", "mode0", "mode1",
            "mode2", "nword_1", "nword_2", "nword_3_4", "nword_5_8", "nword_9plus", "init_waln_refusal"} <= seen
    assert g["cfg"][0].tolist() == [0.07, 375, 10000, 2047, 512]      # (wl, MAX_SIN_L, MAX_SIN_E, FORCE_SIN_L)


def test_rung_arithmetic():
    from hifiasm_amd import api
    # hand-checked against Correct.cpp:16109-16156: no cap at ql, the gate on estimate_err >> 1, the fifth rung
    assert AM.rungs(300, 5, 0.04, 10000, 2047, 512) == [31, -1, 63, 159, 2047]
    assert AM.rungs(60, 40, 0.04, 10000, 2047, 512) == [63, -1, 63, -1, 2047]      # (thre0 is the threshold computed before, attempted or not: rung 3's 63 exceeds rung 2's 31 and comes again; nothing is capped at ql = 60)
    assert AM.rungs(600, 5, 0.04, 10000, 2047, 512) == [31, -1, 63, 319, -1]
    assert AM.rungs(300, 4095, 0.04, 10000, 2047, 512)[0] == 2047 and AM.rungs(300, 4096, 0.04, 10000, 2047, 512) == [-1] * 5 and AM.rungs(300, 5, 0.04, 299, 2047, 512) == [-1] * 5
    assert AM.estimate(300, -1, 0.07, 375) == 21 and AM.estimate(376, -1, 0.07, 375) is None and AM.estimate(376, 9, 0.07, 375) == 9
    n = 0
    for maxe in (0, 31, 100, 2047):
        for e_rate in (0.0, 0.04, 0.07, 0.3, 1.0):
            for force_l in (0, 512):
                for est in (-1, 0, 1, 31, 32, 90, 1000, 1705, 4095, 4096):
                    for ql in list(range(0, 10001, 13)) + [16, 17, 375, 376, 512, 513, 10000, 10001]:
                        e2 = AM.estimate(ql, est, e_rate, 375)
                        got, gate, cnt = api.ladder_adv_thresholds(ql, est, e_rate, 375, 10000, maxe, force_l)
                        if e2 is None:
                            assert cnt < 0, (ql, est)
                            continue
                        want = AM.rungs(ql, e2, e_rate, 10000, maxe, force_l)
                        assert got == want and cnt == sum(t >= 0 for t in want) and gate == (want[0] >= 0), (ql, est, e_rate, maxe, force_l, got, want)
                        n += 1
    for ql in range(1, 10001):      # every ql once, at the fixture's parameters
        assert api.ladder_adv_thresholds(ql, 10, 0.07, 375, 10000, 2047, 512)[0] == AM.rungs(ql, 10, 0.07, 10000, 2047, 512)
    assert n > 200000
