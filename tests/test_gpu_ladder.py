"""The threshold ladder of hc_aln_exz on the device (include/hao.h: hao_window_ladder; hao_ladder.cuh) against tests/golden/ladder.npz - tests/ladder_model.py's
control flow over the REFERENCE's own traced alignments (tests/golden/make_golden_ladder.py): every request field for field and cigar for cigar, on one engine,
through an attached context, and on a two-rank loopback world after the gather (refused before it); the same requests resolved by the host-driven loop the call
replaces - the model's coordinate step, one hao_window_trace_long call per mode and round, survivors picked on the host - give identical records; the refusals -
the two length bounds on a read set of 20 kb reads made for them, each beside a neighbour just inside that passes; a cigar capacity that is too small."""
import os

import numpy as np
import pytest

from helpers import scenario_reads, GOLDEN
import ladder_model as LM

pytestmark = pytest.mark.gpu
NAME = "ont"


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "ladder.npz"))
    return {k: z[k] for k in z.files}


def _cfg(g):
    return float(g["cfg"][0]), int(g["cfg"][1]), int(g["cfg"][2])


def _engine():
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads(NAME)
    e = Engine(0, **okw)
    e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
    return e, rs


def _requests(e, g, lo, hi):
    """the fixture's requests whose query read lies in [lo, hi), as rows (ol, mode, qs, qe, ts, te, estimate_err) over the batch overlap_batch(0, hi - lo) of an engine
    that owns those reads, and their positions in the fixture; the overlap each names is checked against the fixture's copy"""
    base, at = {}, 0
    for r in range(hi - lo):
        base[lo + r] = at; at += e.h_ec_lchain(r)[0].shape[0]
    rows, pos = [], []
    for k, q in enumerate(g["req"]):
        r, i = int(q[0]), int(q[1])
        if lo <= r < hi:
            assert (e.h_ec_lchain(r - lo)[0][i] == g["ovlp"][k]).all(), (r, i)
            rows.append([base[r] + i] + [int(x) for x in q[2:]]); pos.append(k)
    return np.array(rows, dtype=np.int64).reshape(-1, 7), np.array(pos, dtype=np.int64)


def _same(res, off, cig, g, pos):
    want = g["res"][pos]
    for k, f in enumerate(LM.FIELDS):
        bad = np.flatnonzero(res[f].astype(np.int64) != want[:, k])
        assert bad.size == 0, (f, bad[:10], res[bad[:3]], want[bad[:3]])
    assert (np.diff(off) == want[:, 13]).all()
    for j, k in enumerate(pos):
        w = g["cig"][int(g["cig_off"][k]):int(g["cig_off"][k + 1])]
        assert (cig[int(off[j]):int(off[j + 1])] == w).all(), (j, int(k))


def test_every_request_equals_the_reference(gold):
    """one engine, and a context attached to it; then a capacity that is too small: results and offsets come, the entries do not, and the total says what to ask for"""
    e, rs = _engine()
    try:
        e.overlap_batch(0, rs.n)
        rows, pos = _requests(e, gold, 0, rs.n)
        assert rows.shape[0] == gold["req"].shape[0]
        res, off, cig = e.window_ladder(rows, *_cfg(gold))
        _same(res, off, cig, gold, pos)
        assert set(np.unique(res["rung"])) == {0, 1, 2, 3, 4}
        total = int(off[-1])
        r2, o2, c2 = e.window_ladder(rows, *_cfg(gold), cap=total - 1)
        assert c2 is None and int(o2[-1]) == total and (r2 == res).all() and (o2 == off).all()
        r3, o3, c3 = e.window_ladder(rows, *_cfg(gold), cap=total)
        assert (r3 == res).all() and (c3 == cig).all()
        r0, o0, c0 = e.window_ladder(rows[:0], *_cfg(gold))
        assert r0.shape == (0,) and o0.tolist() == [0]
        v = e.attach()
        try:
            v.overlap_batch(0, rs.n)
            rv, ov, cv = v.window_ladder(rows, *_cfg(gold))
            _same(rv, ov, cv, gold, pos)
        finally:
            v.close()
    finally:
        e.close()


def test_host_driven_loop_gives_the_same_records(gold):
    """the loop a caller had to write before: per round the model's coordinate step on the host, one hao_window_trace_long call per mode over the open requests'
    tasks, survivors picked on the host.  Its records equal the call's - the round logic held against the same kernels without the fixture"""
    e, rs = _engine()
    e_rate, maxl, maxe = _cfg(gold)
    try:
        e.overlap_batch(0, rs.n)
        rows, pos = _requests(e, gold, 0, rs.n)
        res, off, cig = e.window_ladder(rows, e_rate, maxl, maxe)
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
            want.clear(); done = {}
            for k, q in enumerate(gold["req"]):
                ol, fc, fo, _ = ctx[int(q[0])]
                i = int(q[1])
                try:
                    done[k] = LM.ladder(ol[i], fc[int(fo[i]) - int(fo[0]):int(fo[i + 1]) - int(fo[0])], rs.lengths, [0] + [int(x) for x in q[2:]], e_rate, maxl, maxe, aligner)
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
        assert 1 <= rounds <= 4
        for j, k in enumerate(pos):
            rec, cg = done[int(k)]
            assert tuple(int(res[f][j]) for f in LM.FIELDS) == tuple(int(x) for x in rec), (j, res[j], rec)
            assert tuple(int(x) for x in cig[int(off[j]):int(off[j + 1])]) == cg, j
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
            e.window_ladder(rows, *_cfg(gold))
        e.dist_gather_reads()
        res, off, cig = e.window_ladder(rows, *_cfg(gold))
        _same(res, off, cig, gold, pos)
        return rows.shape[0], int(((gold["ovlp"][pos, 4] < lo) | (gold["ovlp"][pos, 4] >= hi)).sum())
    _, _, n = _world(NAME, 2, body, gather=False)
    assert sum(k for k, _ in n) == gold["req"].shape[0]
    assert sum(x for _, x in n) > 50      # requests whose target read another rank owns: aligned over the gathered store, under global read ids


def test_refusals(gold):
    """HAO_EINVAL: no batch; maxe beyond HAO_ED_LONG_MAX_THRE; a mode outside 0 - 3; an overlap index outside the batch; coordinates outside the reads; an
    estimate_err outside [0, 2^30).  One bad request refuses the call.  (The two HAO_ED_LONG_MAX_LEN bounds are out of reach of reads this short: below.)"""
    from hifiasm_amd.api import HaoError
    e, rs = _engine()
    e_rate, maxl, maxe = _cfg(gold)
    try:
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_ladder(np.zeros((1, 7), dtype=np.int64), e_rate, maxl, maxe)
        e.overlap_batch(0, rs.n)
        rows, _ = _requests(e, gold, 0, rs.n)
        n_ol = sum(e.h_ec_lchain(r)[0].shape[0] for r in range(rs.n))
        ok = rows[np.flatnonzero(rows[:, 1] == 0)[:3]].copy()
        assert e.window_ladder(ok, e_rate, maxl, maxe)[0].shape[0] == 3
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_ladder(ok, e_rate, maxl, 2048)
        for col, v in ((1, 4), (0, n_ol), (2, -1), (3, 1 << 20), (5, 1 << 20), (6, -1), (6, 1 << 30)):
            bad = ok.copy(); bad[1, col] = v
            with pytest.raises(HaoError, match=r"\(-2\)"):
                e.window_ladder(bad, e_rate, maxl, maxe)
        # (the two length bounds cannot be reached here: the longest read of the small sets has 7956 bases, so every stretch and every length an attempt derives from it -
        # at most ql + 2 * 2047 - stays below 16384, and a stretch outside its read is refused as a coordinate.  What can be asked: the widest gate lets such a request through)
        assert int(rs.lengths.max()) + 2 * 2047 < 16384
        one = ok[:1].copy(); one[0, 6] = 0
        assert e.window_ladder(one, 1.0, 1 << 40, maxe)[0].shape[0] == 1
    finally:
        e.close()


def test_length_refusals_on_long_reads():
    """HAO_EINVAL for ql or a length an attempt derives beyond HAO_ED_LONG_MAX_LEN = 16383, each next to a neighbour just inside the bound that passes.  The small
    scenarios' reads are too short for that, so: eight error-free 20 kb reads cut from one 26 kb sequence at steps of 750 bases (every pair overlaps by 14 kb and
    more; a stretch aligns at the first rung with err 0, so the passing neighbours cost one narrow sweep each)"""
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
            q = [i, mode, xs, xs + ql] + ([-1, -1] if mode == 3 else [ys, ys + tl]) + [0]
            return e.window_ladder(np.array([q], dtype=np.int64), e_rate, big, maxe)[0]

        def refused(*a):
            with pytest.raises(HaoError, match=r"\(-2\)"):
                run(*a)
        # ql itself (mode 0, one rung at thre 31): 16383 passes and aligns, 16384 does not
        r = run(0, 16383, 16383, 31)
        assert int(r["rung"][0]) == 1 and int(r["err"][0]) == 0 and int(r["thre"][0]) == 31
        refused(0, 16384, 16383, 31); refused(0, 17000, 17000, 31)
        # the target interval of mode 0
        refused(0, 16383, 16384, 31)
        # mode 3: ql + 2 thre of the widest rung (0.51 ql scaled, capped at maxe = 2047): 12289 + 4094 = 16383 passes, 12290 does not; ql = 17000 neither
        r = run(3, 12289, 0, 2047)
        assert int(r["rung"][0]) == 1 and int(r["err"][0]) == 0
        refused(3, 12290, 0, 2047); refused(3, 17000, 0, 2047)
        assert int(run(3, 16383 - 62, 0, 31)["rung"][0]) == 1      # (one rung at thre 31: 16321 + 62)
        refused(3, 16383 - 61, 0, 31)
        # modes 1 / 2: the lengths adjust_ext_offset derives from the reads' ends (here 20 000 bases from position 0 of either read)
        z0 = [i, 1, 0, 10, 0, 10, 0]
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_ladder(np.array([z0], dtype=np.int64), 0.0, big, 31)
        z1 = [i, 1, 20000 - 16383, 20000, 20000 - 16383 - 31, 20000, 0]      # qoff 16383 <= toff: qe = q_tot, te = ts + 16383 + 31 = t_tot: text 16383, pattern 16414 -> refused
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_ladder(np.array([z1], dtype=np.int64), 0.0, big, 31)
        z2 = [i, 1, 20000 - 16352, 20000, 20000 - 16383, 20000, 0]            # qoff 16352 <= toff 16383: te = ts + 16352 + 31 = t_tot: lengths 16352 / 16383 -> inside
        assert e.window_ladder(np.array([z2], dtype=np.int64), 0.0, big, 31)[0].shape[0] == 1
    finally:
        e.close()
