"""Golden vectors for the threshold ladder (hao_window_ladder) from the REAL reference: tests/ladder_model.py's control flow (hc_aln_exz's rungs, cal_exz_infi's
coordinate step) driven by the reference's own traced alignment functions through oracle/_ref/ref_harness --edg-tasks / --ed1-tasks / --ed2-tasks / --eds-tasks
(modes 0 - 3; the harness picks the 64-bit, 128-bit or *_infi_* function from the task's threshold, as cal_exz_infi does).  The round scheme is
make_golden_rescue.py's: the model runs over a table of recorded results, a request that asks for a task the table lacks stops there, the missing tasks go
through the harness in one call, repeat until no request stops (at most four rounds: one per rung).

Requests, all over the overlaps of the "ont" read set as h_ec_lchain gives them (a request names its overlap by query read and position in the read's list):
  (a) the verdict-1 overlaps of wlist.npz's configuration ont015 (375-base windows): the stretch from one window record to the next as a global alignment
      (anchored on the records' y_start / y_end), forward extension behind the last record and backward extension before the first, and the same stretches again
      with ts = te = -1 (mode 3);
  (b) crafted requests on the same overlaps: the target interval moved by 40 / 150 bases or to an unrelated place, spans of 60 .. 1500 bases, estimate_err from 0
      to beyond maxe, stretches longer than maxl, extensions next to either end of either read, semi-global stretches that run past the target's end.
Categories, counted on the reference's results alone and asserted non-empty (NEED).
Run in the build container only:  python tests/golden/make_golden_ladder.py  -> tests/golden/ladder.npz (data arrays only)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hifiasm_amd import synth  # noqa: E402
from helpers import scenario_reads, scenario_oracle  # noqa: E402
import ladder_model as LM  # noqa: E402
import wlist_model as WM  # noqa: E402

NAME, KEY, WL = "ont", "ont015", 375
E_RATE, MAXL, MAXE = 0.07, 2000, 2047
NEED = ("rung1", "rung2", "rung3", "rung4", "no_success", "gate_maxl", "gate_maxe", "rung_skipped", "capped_at_ql", "init_waln_refusal", "mode0", "mode1", "mode2", "mode3",
        "nword_1", "nword_2", "nword_3_4", "nword_5_8", "nword_9plus", "ext1_branch0", "ext1_branch1", "ext2_branch0", "ext2_branch1", "clip_at_0", "clip_at_end",
        "mode0_nword_3_4", "mode1_nword_3_4", "mode2_nword_3_4", "mode1_nword_9_16", "mode2_nword_9_16", "mode1_nword_17_32", "mode2_nword_17_32", "mode1_nword_33_64", "mode2_nword_33_64", "mode0_nword_9_16", "mode3_nword_9_16")
MODE_FLAG = {0: ("--edg-tasks", "edg"), 1: ("--ed1-tasks", "ed1"), 2: ("--ed2-tasks", "ed2"), 3: ("--eds-tasks", "eds")}


class Missing(Exception):
    pass


def window_span(z, w):
    xs, xe = int(z[1]), int(z[2])
    return max(w * WL, xs), min(w * WL + WL - 1, xe)


def requests(rs, o):
    G = WM.gold(); lists = WM.gold_lists(G, KEY)
    out, q, n_ov = [], 0, 0
    for r in (int(x) for x in G[KEY + "_reads"]):
        ol = o.lchain(r)[0]
        for i, z in enumerate(ol):
            W = lists[q][0]; q += 1
            if W.shape[0] < 3 or n_ov >= 9:
                continue
            n_ov += 1
            q_tot, t_tot = int(rs.lengths[int(z[0])]), int(rs.lengths[int(z[4])])
            rec = [(window_span(z, int(x[0])), int(x[1]), int(x[2])) for x in W]
            add = lambda mode, qs, qe, ts, te, est: out.append((r, i, mode, qs, qe, ts, te, est))
            # (a) record to record, the two ends, and the same without a target interval
            for k in range(min(len(rec) - 1, 3)):
                (a0, _), ys, _ = rec[k]; (_, b1), _, ye = rec[k + 1]
                add(0, a0, b1 + 1, ys, ye + 1, 10 + 20 * k); add(0, a0, b1 + 1, -1, -1, 10)
            (_, l1), _, lye = rec[-1]; (f0, _), fys, _ = rec[0]
            add(1, l1 + 1, q_tot, lye + 1, t_tot, 5); add(1, l1 + 1, q_tot, -1, -1, 5)
            add(2, 0, f0, 0, fys, 5); add(2, 0, f0, -1, -1, 5)
            # (b) crafted on the same anchors
            (a0, a1), ys, ye = rec[1]
            for d in (40, 150):
                add(0, a0, a1 + 1, min(ys + d, t_tot), min(ye + 1 + d, t_tot), 0)
            far = (ys + t_tot // 2) % max(1, t_tot - (ye + 1 - ys))
            add(0, a0, a1 + 1, far, far + (ye + 1 - ys), 0)
            add(0, a0, a0 + 60, ys, min(ys + 60, t_tot), 40); add(3, a0, a0 + 90, -1, -1, 60); add(0, a0, a0 + 300, far, min(far + 300, t_tot), 0)
            add(0, a0, a1 + 1, ys, ye + 1, 2000); add(3, a0, a1 + 1, 0, 0, 70)
            if len(rec) >= 5:
                (_, e1), _, e_ye = rec[4]
                add(0, a0, e1 + 1, ys, e_ye + 1, 0); add(0, a0, e1 + 1, min(ys + 200, t_tot), min(e_ye + 201, t_tot), 100); add(3, a0, e1 + 1, -1, -1, 130)
            if q_tot > MAXL + 10:
                add(3, 0, MAXL + 5, -1, -1, 0)
            # extensions next to the ends of either read
            add(1, max(0, q_tot - 80), q_tot, max(0, t_tot - 300), t_tot, 0); add(1, max(0, q_tot - 300), q_tot, max(0, t_tot - 80), t_tot, 0)
            add(2, 0, min(80, q_tot), 0, min(300, t_tot), 0); add(2, 0, min(300, q_tot), 0, min(80, t_tot), 0)
            add(1, max(0, q_tot - 80), q_tot, max(0, t_tot - 90), t_tot, 0); add(2, 0, min(80, q_tot), 0, min(90, t_tot), 0)      # (the threshold reaches past the read's end / start: clipped)
            add(1, a0, a0, ys, ys, 0); add(2, a1 + 1, a1 + 1, ye + 1, ye + 1, 0)
            # wide bands in every mode: estimate_err sets the first rung's band - 100: 4 words, 300: 10, 700: 22, 1500: 47 (forward from the second record's start, backward from the last record's end, a global stretch)
            if n_ov <= 3:
                for est in (100, 300, 700, 1500):
                    add(1, a0, min(q_tot, a0 + 1900), ys, t_tot, est); add(2, max(0, l1 + 1 - 1900), l1 + 1, 0, lye + 1, est)
                    if est in (300, 700):
                        add(3, a0, min(q_tot, a0 + 1500), -1, -1, est)
                    if len(rec) >= 6:
                        add(0, a0, rec[5][0][1] + 1, ys, rec[5][2] + 1, est)
            # semi-global stretches that run past the target's end / start inside the overlap's last window
            xe = int(z[2])
            add(3, max(int(z[1]), xe - 50), min(q_tot, xe + 350), -1, -1, 0); add(3, xe, min(q_tot, xe + 200), -1, -1, 0); add(3, int(z[1]), min(q_tot, int(z[1]) + 120), -1, -1, 0)
    return out


def main():
    rs, okw = scenario_reads(NAME)
    o = scenario_oracle(NAME)
    ont = bool(okw.get("is_ont"))
    d = tempfile.mkdtemp(prefix="hao_ladder_")
    fa = os.path.join(d, "r.fq" if ont else "r.fa")
    synth.write_fasta(fa, rs, fastq=ont)

    def harness(by_mode):
        cmd = [os.path.join(ROOT, "oracle", "_ref", "ref_harness"), "-t", "2", "--dump", os.path.join(d, "s"), "--reads-list", "/dev/null", "--no-tables"]
        for mode, tasks in by_mode.items():
            fn = os.path.join(d, f"t{mode}.u32"); np.array(tasks, dtype=np.int64).reshape(-1, 10).astype(np.uint32).tofile(fn)
            cmd += [MODE_FLAG[mode][0], fn]
        r_ = subprocess.run(cmd + (["--ont"] if ont else []) + [fa], capture_output=True, text=True)
        assert r_.returncode == 0, r_.stderr[-2000:]
        res = {}
        for mode, tasks in by_mode.items():
            tag = MODE_FLAG[mode][1]
            r = np.fromfile(os.path.join(d, f"s.{tag}.i32"), dtype=np.int32).reshape(-1, 6)
            cg = np.fromfile(os.path.join(d, f"s.{tag}_cig.u16"), dtype=np.uint16)
            assert r.shape[0] == len(tasks) and cg.size == int(r[:, 5].sum())
            at = 0
            for t, x in zip(tasks, r):
                n = int(x[5]); res[(mode, t)] = tuple(int(v) for v in x[:5]) + (tuple(int(c) for c in cg[at:at + n]),); at += n
        return res

    reqs = requests(rs, o)
    assert 50 <= len(reqs) <= 600, len(reqs)
    ctx = {}
    for r, i, *_ in reqs:
        if r not in ctx:
            ctx[r] = o.lchain(r)
    table, want = {}, set()

    def aligner(mode, task):
        k = (mode, tuple(int(x) for x in task))
        if k not in table:
            want.add(k); raise Missing()
        return table[k]
    rounds = 0
    while True:
        want.clear(); recs, cigs, seen = [], [], set()
        for r, i, mode, qs, qe, ts, te, est in reqs:
            ol, fc, fo, _ = ctx[r]
            z = ol[i]; f = fc[int(fo[i]):int(fo[i + 1])]
            assert not LM.check_request(z, rs.lengths, (0, mode, qs, qe, ts, te, est), E_RATE, MAXL, MAXE), (r, i, mode, qs, qe, ts, te, est)
            try:
                ev = set()
                rec, cig = LM.ladder(z, f, rs.lengths, (0, mode, qs, qe, ts, te, est), E_RATE, MAXL, MAXE, aligner, ev)
                recs.append(rec); cigs.append(cig); seen |= ev
            except Missing:
                pass
        if not want:
            break
        rounds += 1
        by_mode = {}
        for mode, t in sorted(want):
            by_mode.setdefault(mode, []).append(t)
        table.update(harness(by_mode))
    assert rounds <= 4
    if seen & {"clip_q0", "clip_t0"}:
        seen.add("clip_at_0")
    if seen & {"clip_qend", "clip_tend"}:
        seen.add("clip_at_end")
    R = LM.records(recs)
    print(len(reqs), "requests,", rounds, "harness rounds,", len(table), "alignments; rungs", np.bincount(R[:, 0], minlength=5).tolist(), "flags", np.bincount(R[:, 7], minlength=4).tolist())
    print(sorted(seen))
    for c in NEED:
        assert c in seen, c
    keys = sorted(table)
    out = {"cfg": np.array([E_RATE, MAXL, MAXE], dtype=np.float64), "req": np.array(reqs, dtype=np.int32), "res": R.astype(np.int32),
           "cig": np.array([c for cg in cigs for c in cg], dtype=np.uint16), "cig_off": np.concatenate([[0], np.cumsum([len(c) for c in cigs])]).astype(np.int64),
           "ovlp": np.array([ctx[q[0]][0][q[1]] for q in reqs], dtype=np.uint32),
           "tab_mode": np.array([k[0] for k in keys], dtype=np.uint8), "tab_task": np.array([k[1] for k in keys], dtype=np.uint32).reshape(-1, 10),
           "tab_res": np.array([table[k][:5] for k in keys], dtype=np.int32).reshape(-1, 5),
           "tab_cig": np.array([c for k in keys for c in table[k][5]], dtype=np.uint16), "tab_cig_off": np.concatenate([[0], np.cumsum([len(table[k][5]) for k in keys])]).astype(np.int64)}
    fn = os.path.join(HERE, "ladder.npz")
    np.savez_compressed(fn, **out)
    print(os.path.getsize(fn), "bytes")
    assert os.path.getsize(fn) < (1 << 20)


if __name__ == "__main__":
    main()
