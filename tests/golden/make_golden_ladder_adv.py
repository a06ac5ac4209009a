"""Golden vectors for hc_aln_exz_adv's threshold ladder (hao_window_ladder_adv) from the REAL reference: tests/ladder_adv_model.py's control flow driven by the
reference's own traced alignment functions through oracle/_ref/ref_harness --edg-tasks / --ed1-tasks / --ed2-tasks / --eds-tasks, in make_golden_ladder.py's round
scheme (the model runs over a table of recorded results, the missing tasks go through the harness in one call per round, at most five rounds: one per rung).  The
exact shortcut compares the scenario's own read bases.

Set-up: the "ont" scenario's overlaps, wl = 375, e_rate as in ladder.npz, maxl / maxe / force_l = MAX_SIN_L / MAX_SIN_E / FORCE_SIN_L (Levenshtein_distance.h:756-758)
= 10000 / 2047 / 512.  The scenario's longest read has 7956 bases, so no stretch of it is longer than MAX_SIN_L: the gate shut by maxl cannot be met under that set-up.
Those few requests (and a neighbour that passes) therefore form a second group, run as a call of its own with maxl = 2000, ladder.npz's value; `grp` names each
request's group and cfg[g] = (e_rate, wl, maxl, maxe, force_l).

Requests: make_golden_ladder.py's (the stretches between window records, extensions, crafted intervals; their ts = te = -1 variants are now the forced mode 3 that
returns 0), the same semi-global stretches with an explicit interval, and crafted ones for what hc_aln_exz_adv adds: stretches of 6 - 16 bases on and off the
alignment in every mode (exact shortcut hits, mismatches, intervals clamped at the target's end), target intervals longer than a short query, estimate_err = -1 and
beyond the gate, an extension whose far end is unset, empty stretches.
The pthre test (:15639) fires only after an attempt that got as far as the aligner at a threshold equal to the longer string and still failed, which the reference's
aligners do not do; the fixture reaches it through mode-3 attempts outside the traced semi-global domain (HAO_LADDER_UNTRACED: the attempt counts as failed).
Categories, counted on the model's run over the reference's results and asserted non-empty (NEED).
Run in the build container only:  python tests/golden/make_golden_ladder_adv.py  -> tests/golden/ladder_adv.npz (data arrays only)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from hifiasm_amd import synth  # noqa: E402
from helpers import scenario_reads, scenario_oracle  # noqa: E402
import ladder_adv_model as AM  # noqa: E402
import make_golden_ladder as G0  # noqa: E402

NAME = "ont"
CFG = ((0.07, 375, 10000, 2047, 512), (0.07, 375, 2000, 2047, 512))
NEED = ("rung1", "rung2", "rung3", "rung4", "rung5", "exact", "no_success", "early_1", "early_0_forced", "early_0_unset_end", "gate_maxl", "gate_est", "estimated",
        "exact_mismatch", "exact_tl_ne_ql", "exact_rev", "exact_fwd", "clamped_by_dd", "thre_above_ql", "pthre_abandoned", "rung_skipped", "mode3_explicit_aligned",
        "mode0", "mode1", "mode2", "mode3", "nword_1", "nword_2", "nword_3_4", "nword_5_8", "nword_9plus", "init_waln_refusal")


def requests(rs, o):
    """-> [(group, read, overlap, mode, qs, qe, ts, te, estimate_err)]"""
    out, seen = [], set()

    def add(g, r, i, mode, qs, qe, ts, te, est):
        k = (g, r, i, mode, qs, qe, ts, te, est)
        if k not in seen:
            seen.add(k); out.append(k)
    base = G0.requests(rs, o)
    ov = {}
    n_forced = 0
    for r, i, mode, qs, qe, ts, te, est in base:
        z = ov.setdefault((r, i), o.lchain(r)[0][i])
        t_tot = int(rs.lengths[int(z[4])])
        if ts == -1 and te == -1:
            n_forced += 1
            if n_forced <= 12:
                add(0, r, i, mode, qs, qe, ts, te, est)
            if qe > qs:      # the same stretch in explicit mode 3 (any ts < te inside the target: mode 3 reads their difference only)
                add(0, r, i, 3, qs, qe, 0, min(qe - qs, t_tot), est)
                if qe - qs > 2000:
                    add(1, r, i, 3, qs, qe, 0, min(qe - qs, t_tot), est); add(1, r, i, 3, qs, qs + 2000, 0, 2000, est)
        else:
            add(0, r, i, mode, qs, qe, ts, te, est)
    for n_ov, ((r, i), z) in enumerate(ov.items()):
        q_tot, t_tot = int(rs.lengths[int(z[0])]), int(rs.lengths[int(z[4])])
        xs, xe, ys = int(z[1]), int(z[2]), int(z[5])
        a = lambda *q: add(0, r, i, *q)
        if n_ov >= 4:      # (four overlaps, two on either strand, carry the crafted requests)
            break
        for k, d in enumerate(range(30, 1200, 200)):      # short stretches along the overlap: the diagonal of its start is a guess that drifts, the fake cigar's is not
            qs = xs + d; ql = (6, 9, 12, 16)[k % 4]; t0 = min(max(ys + d, 0), t_tot - 20)
            a(0, qs, qs + ql, t0, t0 + ql, 0); a(3, qs, qs + ql, 0, ql, 0); a(1, qs, qs + ql, t0, t0 + 1, 0); a(2, qs, qs + ql, t0, t0 + ql, 0)
            a(3, qs, qs + ql, 0, ql + 30, -1)
        a(1, xs + 40, xs + 50, t_tot - 5, t_tot, 0); a(0, xs + 40, xs + 52, t_tot - 12, t_tot, 0); a(3, xe - 5, min(q_tot, xe + 9), 0, 14, 0)
        # a target interval longer than a short query: the clamped threshold exceeds ql
        a(0, xs + 60, xs + 80, ys + 60, min(t_tot, ys + 105), 0); a(0, xs + 60, xs + 90, ys + 60, min(t_tot, ys + 160), 0); a(0, xs + 60, xs + 100, ys + 60, min(t_tot, ys + 300), 0)
        a(0, xs + 60, xs + 360, ys + 60, min(t_tot, ys + 360), -1); a(1, xs + 60, xs + 200, ys + 60, min(t_tot, ys + 200), -1); a(3, xs + 60, xs + 435, 0, 375, -1)
        a(0, xs + 60, xs + 360, ys + 60, min(t_tot, ys + 360), 4096); a(0, xs + 60, xs + 360, ys + 60, min(t_tot, ys + 360), 4095)
        a(1, xs + 60, q_tot, ys + 60, -1, 5); a(1, xs + 60, q_tot, ys + 60, ys + 60, 5); a(2, 0, xs + 60, ys + 60, ys + 60, 5); a(0, xs, xs, ys, ys, 0); a(0, xs, xs, ys, ys + 5, 0)
        # unrelated targets: past the first rungs - to the fifth where ql <= force_l, to no success beyond
        far = (ys + t_tot // 2) % max(1, t_tot - 700)
        for ql in (40, 120, 300, 500, 513, 700):
            a(0, xs + 60, xs + 60 + ql, far, far + ql, 0)
        # mode-3 stretches at the target's end, where the band stops covering the pattern, with estimates whose rungs all clamp at the same length
        for est in (0, 200, 500):
            a(3, max(xs, xe - 50), min(q_tot, xe + 350), 0, 10, est); a(3, xe, min(q_tot, xe + 200), 0, 10, est); a(3, xe - 30, min(q_tot, xe + 40), 0, 10, est); a(3, xs, min(q_tot, xs + 120), 0, 10, est)
            a(3, xe - 20, min(q_tot, xe + 20), 0, 10, est); a(3, xs, xs + 40, 0, 10, est)
        if n_ov < 3:
            a(0, xs + 60, xs + 1260, ys + 60, min(t_tot, ys + 1260), 200)      # (a band of seven words)
    # the first base of the target (an overlap that starts there): with a threshold as long as the stretch the whole stretch is absent diagonals, outside the traced domain
    r = base[0][0]; ol = o.lchain(r)[0]
    for i in [i for i, z in enumerate(ol) if int(z[5]) == 0][:2]:
        xs = int(ol[i][1])
        for est in (0, 200, 500):
            add(0, r, i, 3, xs, xs + 40, 0, 10, est); add(0, r, i, 3, xs, xs + 100, 0, 10, est)
    return out


def main():
    rs, okw = scenario_reads(NAME)
    o = scenario_oracle(NAME)
    ont = bool(okw.get("is_ont"))
    d = tempfile.mkdtemp(prefix="hao_ladder_adv_")
    fa = os.path.join(d, "r.fq" if ont else "r.fa")
    synth.write_fasta(fa, rs, fastq=ont)
    bases = AM.reads_bases(rs)

    def harness(by_mode):
        cmd = [os.path.join(ROOT, "oracle", "_ref", "ref_harness"), "-t", "2", "--dump", os.path.join(d, "s"), "--reads-list", "/dev/null", "--no-tables"]
        for mode, tasks in by_mode.items():
            fn = os.path.join(d, f"t{mode}.u32"); np.array(tasks, dtype=np.int64).reshape(-1, 10).astype(np.uint32).tofile(fn)
            cmd += [G0.MODE_FLAG[mode][0], fn]
        r_ = subprocess.run(cmd + (["--ont"] if ont else []) + [fa], capture_output=True, text=True)
        assert r_.returncode == 0, r_.stderr[-2000:]
        res = {}
        for mode, tasks in by_mode.items():
            tag = G0.MODE_FLAG[mode][1]
            r = np.fromfile(os.path.join(d, f"s.{tag}.i32"), dtype=np.int32).reshape(-1, 6)
            cg = np.fromfile(os.path.join(d, f"s.{tag}_cig.u16"), dtype=np.uint16)
            assert r.shape[0] == len(tasks) and cg.size == int(r[:, 5].sum())
            at = 0
            for t, x in zip(tasks, r):
                n = int(x[5]); res[(mode, t)] = tuple(int(v) for v in x[:5]) + (tuple(int(c) for c in cg[at:at + n]),); at += n
        return res

    reqs = requests(rs, o)
    assert 200 <= len(reqs) <= 700, len(reqs)
    ctx = {}
    for _, r, *_ in reqs:
        if r not in ctx:
            ctx[r] = o.lchain(r)
    table, want = {}, set()

    def aligner(mode, task):
        k = (mode, tuple(int(x) for x in task))
        if k not in table:
            want.add(k); raise G0.Missing()
        return table[k]
    rounds = 0
    while True:
        want.clear(); recs, cigs, seen = [], [], set()
        for g, r, i, mode, qs, qe, ts, te, est in reqs:
            ol, fc, fo, _ = ctx[r]
            z = ol[i]; f = fc[int(fo[i]):int(fo[i + 1])]
            q = (0, mode, qs, qe, ts, te, est)
            assert not AM.check_request(z, rs.lengths, q, *CFG[g]), (g, r, i, mode, qs, qe, ts, te, est)
            try:
                ev = set()
                rec, cig = AM.ladder(z, f, rs.lengths, q, *CFG[g], aligner, bases, ev)
                recs.append(rec); cigs.append(cig); seen |= ev
            except G0.Missing:
                pass
        if not want:
            break
        rounds += 1
        by_mode = {}
        for mode, t in sorted(want):
            by_mode.setdefault(mode, []).append(t)
        table.update(harness(by_mode))
    assert rounds <= 5
    R = np.array(recs, dtype=np.int64).reshape(-1, len(AM.FIELDS))
    print(len(reqs), "requests,", rounds, "harness rounds,", len(table), "alignments; done", np.bincount(R[:, 0], minlength=2).tolist(), "rungs", np.bincount(R[:, 1], minlength=7).tolist(),
          "flags", np.bincount(R[:, 8], minlength=8).tolist())
    print(sorted(seen))
    for c in NEED:
        assert c in seen, c
    keys = sorted(table)
    out = {"cfg": np.array(CFG, dtype=np.float64), "grp": np.array([q[0] for q in reqs], dtype=np.uint8), "req": np.array([q[1:] for q in reqs], dtype=np.int32), "res": R.astype(np.int32),
           "cig": np.array([c for cg in cigs for c in cg], dtype=np.uint16), "cig_off": np.concatenate([[0], np.cumsum([len(c) for c in cigs])]).astype(np.int64),
           "ovlp": np.array([ctx[q[1]][0][q[2]] for q in reqs], dtype=np.uint32),
           "tab_mode": np.array([k[0] for k in keys], dtype=np.uint8), "tab_task": np.array([k[1] for k in keys], dtype=np.uint32).reshape(-1, 10),
           "tab_res": np.array([table[k][:5] for k in keys], dtype=np.int32).reshape(-1, 5),
           "tab_cig": np.array([c for k in keys for c in table[k][5]], dtype=np.uint16), "tab_cig_off": np.concatenate([[0], np.cumsum([len(table[k][5]) for k in keys])]).astype(np.int64)}
    fn = os.path.join(HERE, "ladder_adv.npz")
    np.savez_compressed(fn, **out)
    print(os.path.getsize(fn), "bytes")
    assert os.path.getsize(fn) < (1 << 20)


if __name__ == "__main__":
    main()
