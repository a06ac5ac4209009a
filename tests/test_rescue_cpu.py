"""The rescue stage's host side, no GPU: tests/rescue_model.py driven by the oracle over the oracle's own overlaps and primary results, and hao_rescue_task
(hao_rescue_pair, the function the device rebuilds its tasks with) held against every forward and backward work item the model asks for."""
import numpy as np
import pytest

from helpers import scenario_reads, scenario_oracle
import rescue_model as RM

NOALN = 2**31 - 1


def _model_over_oracle(name, wl, e_rate, reads):
    rs, _ = scenario_reads(name)
    o = scenario_oracle(name)
    align = RM.oracle_aligner(o)
    out = []
    for r in reads:
        ol, fc, fo, _ = o.lchain(r)
        T = RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate)
        res = o.window_ed(T) if T.shape[0] else np.zeros((0, 2), dtype=np.int32)
        out.append((ol, RM.read_rescue(ol, fc, fo, rs.lengths, wl, e_rate, res, align)))
    return rs, out


@pytest.mark.parametrize("name,wl,e_rate", [("hifi", 775, 0.004), ("hifi", 200, 0.01), ("ont", 375, 0.015)])
def test_rescue_pair_equals_the_models_tasks(name, wl, e_rate):
    from hifiasm_amd import api
    rs, per = _model_over_oracle(name, wl, e_rate, range(0, 40))
    tab = np.zeros(wl + 1, dtype=np.uint8)
    api.lib().hao_ref_thresholds(wl, e_rate, tab.ctypes.data_as(api.C.POINTER(api.C.c_uint8)))
    n = {"fwd": 0, "bwd": 0}
    for ol, results in per:
        for z, w in zip(ol, results):
            for item in w["log"]:
                if item[0] not in n:
                    continue
                kind, task, win, toff = item
                got = api.rescue_task(z, win, wl, toff, tab, rs.lengths[int(z[4])])
                assert got is not None and tuple(int(x) for x in got) == tuple(int(x) for x in task), (kind, win, toff, got, task)
                n[kind] += 1
    assert n["fwd"] > 20 and n["bwd"] > 20, n


def test_rescue_pair_refusals_and_thresholds():
    from hifiasm_amd import api
    wl, e_rate = 375, 0.02
    tab = np.zeros(wl + 1, dtype=np.uint8)
    api.lib().hao_ref_thresholds(wl, e_rate, tab.ctypes.data_as(api.C.POINTER(api.C.c_uint8)))
    z = np.array([0, 100, 1999, 0, 1, 50, 1949, 0, 0, 0, 0, 0], dtype=np.uint32)      # x 100 .. 1999 on read 0, y on read 1
    for ql in (1, 3, 4, 49, 50, 149, 150, 299, 300, 374, 375):
        t = RM.rescue_threshold(ql, wl, e_rate)
        zz = z.copy(); zz[1] = 375; zz[2] = 375 + ql - 1
        got = api.rescue_task(zz, 1, wl, 500, tab, 5000)
        assert got is not None and int(got[8]) == t and int(got[6]) == ql, (ql, t, got)
    l = 2000
    for toff in (-1, l, l + 5):                                                      # init_waln: s < 0, s >= l
        assert api.rescue_task(z, 1, wl, toff, tab, l) is None
    assert api.rescue_task(z, 1, wl, l - 200, tab, l) is None                        # too little target left: l - s + 2 thre + 31 < w_l
    got = api.rescue_task(z, 1, wl, 5, tab, l)                                       # clipped at the target's start: aux_beg
    thre = RM.rescue_threshold(375, wl, e_rate)
    assert got is not None and (int(got[1]), int(got[9]), int(got[2])) == (0, thre - 5, 375 + 2 * thre - (thre - 5))
    assert api.rescue_task(z, 9, wl, 500, tab, l) is None                            # a window the overlap does not cover


GOLD_KEYS = {"hifi": "hifi", "ont": "ont", "hifi004": "hifi", "ont015": "ont", "fz2w": "fz2"}


def _gold():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rescue.npz"))


def _table_aligner(G, key):
    """align(task, traced) over the REFERENCE's recorded results; a task the reference was never asked for is an error"""
    ed = {tuple(int(x) for x in t): (int(r[0]), 0, int(r[1])) for t, r in zip(G[key + "_ed_tasks"], G[key + "_ed_res"])}
    eds = {tuple(int(x) for x in t): tuple(int(x) for x in r) for t, r in zip(G[key + "_eds_tasks"], G[key + "_eds_res"])}
    return lambda task, traced: (eds if traced else ed)[tuple(int(x) for x in task)]


@pytest.mark.parametrize("key", sorted(GOLD_KEYS))
def test_model_and_rescue_pair_equal_the_reference_fixture(key):
    """tests/golden/rescue.npz (the reference's own functions, tests/golden/make_golden_rescue.py) on its sampled reads: (1) the model driven by the ORACLE gives
    the recorded per-overlap and window records - and asks only for alignments the reference was asked for, with the same answers; (2) hao_rescue_task rebuilds
    every forward and backward task of those runs from (overlap, window, toff)"""
    from hifiasm_amd import api
    G = _gold()
    name = GOLD_KEYS[key]
    wl, e_rate = int(G[key + "_cfg"][0]), float(G[key + "_cfg"][1])
    rs, _ = scenario_reads(name)
    o = scenario_oracle(name)
    oracle, recorded = RM.oracle_aligner(o), _table_aligner(G, key)

    def both(task, traced):
        a, b = oracle(task, traced), recorded(task, traced)
        assert (a[0], a[2]) == (b[0], b[2]) and (not traced or a[0] == NOALN or a[1] == b[1]), (task, traced, a, b)
        return a
    tab = np.zeros(wl + 1, dtype=np.uint8)
    api.lib().hao_ref_thresholds(wl, e_rate, tab.ctypes.data_as(api.C.POINTER(api.C.c_uint8)))
    k, n_items = 0, 0
    for r in G[key + "_reads"]:
        r = int(r)
        ol, fc, fo, _ = o.lchain(r)
        T = RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate)
        res = np.array([[recorded(t, False)[0], recorded(t, False)[2]] for t in T], dtype=np.int64).reshape(-1, 2)
        for z, w in zip(ol, RM.read_rescue(ol, fc, fo, rs.lengths, wl, e_rate, res, both)):
            assert [w["verdict"], w["flags"], w["exit_win"], w["align_length"], w["n_rescued"]] == [int(x) for x in G[key + "_ovlp"][k]], (r, k)
            a, b = int(G[key + "_win_off"][k]), int(G[key + "_win_off"][k + 1])
            assert w["wins"].shape[0] == b - a and (w["wins"] == G[key + "_wins"][a:b]).all(), (r, k)
            for item in w["log"]:
                if item[0] in ("fwd", "bwd"):
                    got = api.rescue_task(z, item[2], wl, item[3], tab, rs.lengths[int(z[4])])
                    assert got is not None and tuple(int(x) for x in got) == tuple(int(x) for x in item[1]), item
                    n_items += 1
            k += 1
    assert k == G[key + "_ovlp"].shape[0] and n_items > 0
    rounds, n_gap, n_untr = [int(x) for x in G[key + "_counts"]]
    assert n_untr * 100 <= n_gap
