"""The threshold ladder of hc_aln_exz_adv on the device (include/hao.h: hao_window_ladder_adv; hao_ladder.cuh under its ADV rule set) against
tests/golden/ladder_adv.npz - tests/ladder_adv_model.py's control flow over the REFERENCE's own traced alignments (tests/golden/make_golden_ladder_adv.py): every
request field for field and cigar for cigar, on one engine, through an attached context, and on a two-rank loopback world after the gather (refused before it);
the same requests resolved by the host-driven loop the call replaces - the model's coordinate step, one hao_window_trace_long call per mode and round, survivors
picked on the host - give identical records and the same number of open requests per round; requests both ladders treat alike give one alignment from both calls;
the refusals, each beside a neighbour just inside that passes; a cigar capacity that is too small; the empty call.
The fixture's requests come in groups that differ in the call's parameters (cfg[g]; the second group exists for the gate shut by maxl): one call per group."""
import os

import numpy as np
import pytest

from helpers import scenario_reads, GOLDEN
import ladder_model as LM
import ladder_adv_model as AM
from test_gpu_ladder import _engine, _requests

pytestmark = pytest.mark.gpu
NAME = "ont"


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "ladder_adv.npz"))
    return {k: z[k] for k in z.files}


def _cfg(g, k=0):
    c = g["cfg"][k]
    return float(c[0]), int(c[1]), int(c[2]), int(c[3]), int(c[4])


def _groups(g, pos):
    """[(group, indices into pos / the rows of _requests)]"""
    return [(k, np.flatnonzero(g["grp"][pos] == k)) for k in range(g["cfg"].shape[0])]


def _same(res, off, cig, g, pos):
    want = g["res"][pos]
    for k, f in enumerate(AM.FIELDS):
        bad = np.flatnonzero(res[f].astype(np.int64) != want[:, k])
        assert bad.size == 0, (f, bad[:10], res[bad[:3]], want[bad[:3]], g["req"][pos[bad[:3]]])
    assert (np.diff(off) == want[:, 14]).all()
    for j, k in enumerate(pos):
        w = g["cig"][int(g["cig_off"][k]):int(g["cig_off"][k + 1])]
        assert (cig[int(off[j]):int(off[j + 1])] == w).all(), (j, int(k))


def _run_all(e, g, rows, pos):
    for k, sel in _groups(g, pos):
        res, off, cig = e.window_ladder_adv(rows[sel], *_cfg(g, k))
        _same(res, off, cig, g, pos[sel])


def test_every_request_equals_the_reference(gold):
    """one engine, and a context attached to it; then a capacity that is too small: results and offsets come, the entries do not, and the total says what to ask for;
    the empty call"""
    e, rs = _engine()
    try:
        e.overlap_batch(0, rs.n)
        rows, pos = _requests(e, gold, 0, rs.n)
        assert rows.shape[0] == gold["req"].shape[0]
        _run_all(e, gold, rows, pos)
        sel = _groups(gold, pos)[0][1]
        res, off, cig = e.window_ladder_adv(rows[sel], *_cfg(gold))
        assert set(np.unique(res["rung"])) == {0, 1, 2, 3, 4, 5, 6} and set(np.unique(res["done"])) == {0, 1}
        assert (res["flags"] & 4).any()
        total = int(off[-1])
        r2, o2, c2 = e.window_ladder_adv(rows[sel], *_cfg(gold), cap=total - 1)
        assert c2 is None and int(o2[-1]) == total and (r2 == res).all() and (o2 == off).all()
        r3, o3, c3 = e.window_ladder_adv(rows[sel], *_cfg(gold), cap=total)
        assert (r3 == res).all() and (c3 == cig).all()
        r0, o0, c0 = e.window_ladder_adv(rows[:0], *_cfg(gold))
        assert r0.shape == (0,) and o0.tolist() == [0] and e.ladder_adv_rounds() == [0] * 5
        v = e.attach()
        try:
            v.overlap_batch(0, rs.n)
            _run_all(v, gold, rows, pos)
        finally:
            v.close()
    finally:
        e.close()


def test_host_driven_loop_gives_the_same_records_and_rounds(gold):
    """the loop a caller has to write without the call: per round the model's coordinate step on the host, one hao_window_trace_long call per mode over the open
    requests' tasks, survivors picked on the host.  Its records equal the call's, and the requests it still has open in each round are as many as the device had"""
    e, rs = _engine()
    cfg = _cfg(gold)
    try:
        e.overlap_batch(0, rs.n)
        rows, pos = _requests(e, gold, 0, rs.n)
        sel = _groups(gold, pos)[0][1]
        res, off, cig = e.window_ladder_adv(rows[sel], *cfg)
        dev_rounds = e.ladder_adv_rounds()
        bases = AM.reads_bases(rs)
        ctx = {}
        for q in gold["req"]:
            if int(q[0]) not in ctx:
                ctx[int(q[0])] = e.h_ec_lchain(int(q[0]))
        table, want, rounds = {}, set(), 0

        class Missing(Exception):
            pass

        def aligner(mode, task):
            k = (mode, tuple(int(x) for x in task))
            if k not in table:
                want.add(k); raise Missing()
            return table[k]
        while True:
            want.clear(); done, n_att = {}, {}
            for k in pos[sel]:
                q = gold["req"][k]
                ol, fc, fo, _ = ctx[int(q[0])]
                i = int(q[1]); a = []
                try:
                    done[int(k)] = AM.ladder(ol[i], fc[int(fo[i]) - int(fo[0]):int(fo[i + 1]) - int(fo[0])], rs.lengths, [0] + [int(x) for x in q[2:]], *cfg, aligner, bases, att=a)
                    n_att[int(k)] = a[-1] if a else 0
                except Missing:
                    pass
            if not want:
                break
            rounds += 1
            for mode in range(4):
                ts = sorted(t for m, t in want if m == mode)
                if ts:
                    cap = 2 * max(t[8] for t in ts) + 8
                    r, c = e.window_trace_long(np.array(ts, dtype=np.int64).astype(np.uint32), cap=cap, mode=mode)
                    for t, x, row in zip(ts, r, c):
                        table[(mode, t)] = tuple(int(v) for v in x[:5]) + (tuple(int(v) for v in row[:int(x[5])]),)
        assert 1 <= rounds <= 5
        for j, k in enumerate(pos[sel]):
            rec, cg = done[int(k)]
            assert tuple(int(res[f][j]) for f in AM.FIELDS) == tuple(int(x) for x in rec), (j, res[j], rec)
            assert tuple(int(x) for x in cig[int(off[j]):int(off[j + 1])]) == cg, j
        model_rounds = [sum(1 for n in n_att.values() if n > j) for j in range(5)]
        assert dev_rounds == model_rounds and model_rounds[4] > 0, (dev_rounds, model_rounds)
    finally:
        e.close()


def test_both_ladders_agree_where_their_rules_do(gold):
    """mode 0, ql > 16, ql >= tl, every rung's threshold at most ql, both gates open, no fifth rung: hc_aln_exz and hc_aln_exz_adv make the same attempts, so
    hao_window_ladder and hao_window_ladder_adv give the same alignment once the former's coordinates are made absolute"""
    e, rs = _engine()
    e_rate, wl, maxl, maxe, force_l = _cfg(gold)
    try:
        e.overlap_batch(0, rs.n)
        rows, pos = _requests(e, gold, 0, rs.n)
        keep = []
        for j, q in enumerate(rows):
            _, mode, qs, qe, ts, te, est = (int(x) for x in q)
            ql, tl = qe - qs, te - ts
            if mode != 0 or (ts == -1 and te == -1) or ql <= 16 or tl <= 0 or ql < tl or est < 0 or gold["grp"][pos[j]] != 0:
                continue
            a, b = AM.rungs(ql, est, e_rate, maxl, maxe, force_l), LM.rungs(ql, est, e_rate, maxl, maxe)
            if a[4] == -1 and a[:4] == b and a[0] >= 0 and max(a) <= ql:
                keep.append(j)
        assert len(keep) >= 10
        sub = rows[keep]
        r1, o1, c1 = e.window_ladder(sub, e_rate, maxl, maxe)
        r2, o2, c2 = e.window_ladder_adv(sub, e_rate, wl, maxl, maxe, force_l)
        assert len(set(r1["rung"].tolist())) >= 3      # (the selection exercises more than the first rung)
        for f in ("rung", "thre", "qs", "qe", "ts", "te", "aux_beg", "flags", "err", "n_cigar"):
            assert (r1[f] == r2[f]).all(), f
        hit = r1["rung"] > 0
        assert (r2["done"] == hit).all()
        for f, base in (("a_ps", "ts"), ("a_pe", "ts"), ("a_ts", "qs"), ("a_te", "qs")):
            assert (np.where(hit, r1[f] + r1[base], -1) == r2[f]).all(), f
        assert (o1 == o2).all() and (c1 == c2).all()
    finally:
        e.close()


def test_each_fetch_serves_its_own_call(gold):
    """hao_fetch_ladder after hao_window_ladder_adv is refused (HAO_EINVAL), hao_fetch_ladder_adv serves it - and the reverse after hao_window_ladder"""
    from hifiasm_amd.api import HaoError
    e, rs = _engine()
    e_rate, wl, maxl, maxe, force_l = _cfg(gold)
    try:
        e.overlap_batch(0, rs.n)
        rows, pos = _requests(e, gold, 0, rs.n)
        sel = _groups(gold, pos)[0][1][:40]
        sub = rows[sel]
        e.window_ladder_adv(sub, e_rate, wl, maxl, maxe, force_l)
        assert sum(e.ladder_adv_rounds()) > 0
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.ladder_rounds()
        live = sub[np.array([not LM.check_request(gold["ovlp"][pos[k]], rs.lengths, [int(x) for x in q], e_rate, maxl, maxe) for k, q in zip(sel, sub)], dtype=bool)]      # (those hao_window_ladder takes)
        assert live.shape[0] >= 10
        e.window_ladder(live, e_rate, maxl, maxe)
        assert sum(e.ladder_rounds()) > 0
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.ladder_adv_rounds()
    finally:
        e.close()


def test_two_rank_world_after_the_gather(gold):
    """sharded engines: refused before hao_dist_gather_reads (HAO_EUNSUPP), the fixture's records after it, each rank over the requests of the reads it owns
    (a rank that owns none of them makes the empty call)"""
    from hifiasm_amd.api import HaoError
    from test_gpu_shard_f3 import _world

    def body(rank, e, lo, hi):
        e.overlap_batch(0, hi - lo)
        rows, pos = _requests(e, gold, lo, hi)
        with pytest.raises(HaoError, match=r"\(-4\)"):
            e.window_ladder_adv(rows, *_cfg(gold))
        e.dist_gather_reads()
        _run_all(e, gold, rows, pos)
        return rows.shape[0], int(((gold["ovlp"][pos, 4] < lo) | (gold["ovlp"][pos, 4] >= hi)).sum())
    _, _, n = _world(NAME, 2, body, gather=False)
    assert sum(k for k, _ in n) == gold["req"].shape[0]
    assert sum(x for _, x in n) > 50      # requests whose target read another rank owns: aligned over the gathered store, under global read ids


def test_refusals(gold):
    """HAO_EINVAL: no batch; maxe beyond HAO_ED_LONG_MAX_THRE; negative wl / maxl / force_l; a mode outside 0 - 3; an overlap index outside the batch; coordinates
    outside the reads; estimate_err >= 2^30; estimate_err < 0 on a stretch longer than wl.  One bad request refuses the call; the neighbour just inside passes"""
    from hifiasm_amd.api import HaoError
    e, rs = _engine()
    e_rate, wl, maxl, maxe, force_l = _cfg(gold)
    try:
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_ladder_adv(np.zeros((1, 7), dtype=np.int64), e_rate, wl, maxl, maxe, force_l)
        e.overlap_batch(0, rs.n)
        rows, _ = _requests(e, gold, 0, rs.n)
        n_ol = sum(e.h_ec_lchain(r)[0].shape[0] for r in range(rs.n))
        ok = rows[np.flatnonzero((rows[:, 1] == 0) & (rows[:, 3] - rows[:, 2] > 100) & (rows[:, 3] - rows[:, 2] <= wl) & (rows[:, 5] > rows[:, 4]) & (rows[:, 6] == 0))[:3]].copy()
        assert ok.shape[0] == 3

        def run(q, *cfg):
            return e.window_ladder_adv(q, *(cfg or (e_rate, wl, maxl, maxe, force_l)))[0]

        def refused(q, *cfg):
            with pytest.raises(HaoError, match=r"\(-2\)"):
                run(q, *cfg)
        assert run(ok).shape[0] == 3
        assert run(ok, e_rate, wl, maxl, 2047, force_l).shape[0] == 3 and run(ok, e_rate, 0, 0, 0, 0).shape[0] == 3
        refused(ok, e_rate, wl, maxl, 2048, force_l); refused(ok, e_rate, -1, maxl, maxe, force_l); refused(ok, e_rate, wl, -1, maxe, force_l); refused(ok, e_rate, wl, maxl, maxe, -1)
        refused(ok, 1.5, wl, maxl, maxe, force_l)
        z = ok[1]
        for col, v, inside in ((1, 4, 3), (0, n_ol, n_ol - 1), (2, -1, 0), (3, 1 << 20, None), (4, -1, 0), (5, 1 << 20, None), (6, 1 << 30, (1 << 30) - 1)):
            bad = ok.copy(); bad[1, col] = v
            refused(bad)
            if inside is not None:
                good = ok.copy(); good[1, col] = inside
                if col == 0:
                    good[1, 2:6] = (0, 0, 0, 0)      # (another overlap: the empty stretch, which every overlap has)
                assert run(good).shape[0] == 3
        # estimate_err < 0: ql <= wl passes, ql = wl + 1 is refused (cal_estimate_err is not built); -1 and any other negative value alike
        ql = int(z[3] - z[2])
        for est in (-1, -7):
            good = ok.copy(); good[1, 6] = est
            assert run(good, e_rate, ql, maxl, maxe, force_l).shape[0] == 3
            refused(good, e_rate, ql - 1, maxl, maxe, force_l)
        # behind an early return nothing else of the request is looked at: an unset far end, a stretch that is empty
        early = ok.copy(); early[1, 5] = -1; early[1, 6] = -1; early[2, 3] = early[2, 2]; early[2, 5] = 1 << 20
        r = run(early, e_rate, 0, maxl, maxe, force_l)
        assert r["done"].tolist()[1:] == [0, 0] and r["rung"].tolist()[1:] == [0, 0]
    finally:
        e.close()


def test_length_refusals_on_long_reads():
    """HAO_EINVAL for ql or a length an attempt derives beyond HAO_ED_LONG_MAX_LEN = 16383, each next to a neighbour just inside the bound that passes: on
    test_gpu_ladder's eight error-free 20 kb reads (a stretch aligns at the first rung with err 0, so the passing neighbours cost one narrow sweep each)"""
    from hifiasm_amd import synth
    from hifiasm_amd.api import Engine, HaoError
    g = synth.make_genome(26000, seed=5)
    rs = synth.from_codes([g[o:o + 20000].copy() for o in range(0, 6000, 750)])
    e = Engine(0)
    try:
        e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
        e.overlap_batch(0, rs.n)
        ol = e.h_ec_lchain(0)[0]
        i = int(np.argmax(ol[:, 2].astype(np.int64) - ol[:, 1]))
        xs, xe, ys, rev = int(ol[i, 1]), int(ol[i, 2]), int(ol[i, 5]), int(ol[i, 7])
        assert xe + 1 - xs >= 17000 and rev == 0 and int(ol[i, 0]) == 0
        big = 1 << 40

        def run(mode, ql, tl, maxe, e_rate=0.0):
            q = [i, mode, xs, xs + ql, ys, ys + tl, 0]
            return e.window_ladder_adv(np.array([q], dtype=np.int64), e_rate, 0, big, maxe, 0)[0]

        def refused(*a):
            with pytest.raises(HaoError, match=r"\(-2\)"):
                run(*a)
        # ql itself (mode 0, one rung at thre 31): 16383 passes and aligns, 16384 does not; the target interval of mode 0 alike
        r = run(0, 16383, 16383, 31)
        assert int(r["done"][0]) == 1 and int(r["rung"][0]) == 1 and int(r["err"][0]) == 0 and int(r["thre"][0]) == 31 and int(r["a_ts"][0]) == xs and int(r["a_te"][0]) == xs + 16382
        refused(0, 16384, 16383, 31); refused(0, 16383, 16384, 31)
        # mode 3 with an interval (its length only clamps the thresholds): ql + 2 thre of the widest rung (0.51 ql scaled, capped at maxe = 2047): 12289 + 4094 = 16383
        r = run(3, 12289, 12289, 2047)
        assert int(r["rung"][0]) == 1 and int(r["err"][0]) == 0
        refused(3, 12290, 12290, 2047)
        assert int(run(3, 16383 - 62, 100, 31)["rung"][0]) == 1      # (one rung at thre 31: 16321 + 62)
        refused(3, 16383 - 61, 100, 31)
        # mode 1: the lengths adjust_ext_offset derives from the reads' ends (here 20 000 bases from position 0 of either read)
        def ext(q):
            return e.window_ladder_adv(np.array([q], dtype=np.int64), 0.0, 0, big, 31, 0)[0]
        with pytest.raises(HaoError, match=r"\(-2\)"):
            ext([i, 1, 0, 10, 0, 10, 0])
        with pytest.raises(HaoError, match=r"\(-2\)"):
            ext([i, 1, 20000 - 16383, 20000, 20000 - 16383 - 31, 20000, 0])      # qoff 16383 <= toff: te = ts + 16383 + 31 = t_tot: text 16383, pattern 16414
        assert ext([i, 1, 20000 - 16352, 20000, 20000 - 16383, 20000, 0]).shape[0] == 1      # qoff 16352 <= toff 16383: lengths 16352 / 16383
    finally:
        e.close()
