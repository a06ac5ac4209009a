"""Golden vectors for the window lists (hao_window_wlist_ref) from the REAL reference: tests/wlist_model.py's control flow (on tests/rescue_model.py's) driven by
the reference's own alignment functions through oracle/_ref/ref_harness --ed-tasks (ed_band_cal_semi_64_w_absent_diag: the primary pass and the forward steps)
and --eds-tasks (ed_band_cal_semi_64_w_absent_diag_trace + gen_trace on a cleared bit_extz_t, with its cigars in PREFIX.eds_cig.u16: every traced window and
every re-placement).  The round scheme is make_golden_rescue.py's: the models run over a table of recorded results, an overlap that asks for a task the table
lacks stops there, the missing tasks go through the harness in one call each, repeat until no overlap stops.  The five configurations of rescue.npz with sparser read samples, and two more (below).

Preset entry against cleared entry: wlist_model.trace_window asserts (err, pe) of the cleared trace against the record's distance-only result on EVERY window
it traces with a preset - here on the reference's results.

Categories, counted on the reference's results alone and asserted non-empty over the fixture (NEED).  The five configurations of rescue.npz hold no re-placement
that is taken inside a passing overlap, no untraced window and no forward window with err == 0.  Every read of hifi, ont, nn, edge, fz2 at (775, 0.04 / 0.004),
(375, 0.07 / 0.015 / 0.012 / 0.01), (200, 0.01), (150, 0.02), (100, 0.01 / 0.004) was scanned with the oracle-driven model (bw001 not reached).  Taken
re-placements: ont (775, 0.04) 1, ont (375, 0.012) 1, ont (200, 0.01) 1, ont (150, 0.02) 13, ont (100, 0.01 / 0.004) 1, nn (200, 0.01) 3, none elsewhere.
Untraced windows: hifi (375, 0.012) 1, hifi (375, 0.01) 2, nn (375, 0.012 / 0.01) 1, none elsewhere.  Forward windows with err == 0: every set at windows of
200 bases and less (19 .. 2771 overlaps), nn and edge (375, 0.01) 1 each, none at 775.  Two configurations are in the fixture for them: nn (200, 0.01) with read
169 (re-placements taken, forward windows with err == 0) and hifi (375, 0.01) with reads 3 and 172 (untraced windows).
Run in the build container only:  python tests/golden/make_golden_wlist.py  -> tests/golden/wlist.npz"""
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
import rescue_model as RM  # noqa: E402
import wlist_model as WM  # noqa: E402

CONFIGS = {"hifi": ("hifi", 775, 0.04, 8), "ont": ("ont", 375, 0.07, 24), "hifi004": ("hifi", 775, 0.004, 6), "ont015": ("ont", 375, 0.015, 12), "fz2w": ("fz2", 1500, 0.006, 2),
           "nn200": ("nn", 200, 0.01, 45), "hifi375": ("hifi", 375, 0.01, 45)}      # (read set, window, e_rate, read stride)
FORCED = {"ont015": (110,), "nn200": (169,), "hifi375": (3, 172)}
NEED = ("primary_err0", "primary_traced", "forward_traced", "backward_traced", "anchor_traced", "recal_not_taken", "verdict1_with_rescued", "verdict0", "indel_both", "replaced", "untraced", "forward_err0")


class Missing(Exception):
    pass


def main():
    out, total = {}, {}
    for key, (name, wl, e_rate, stride) in CONFIGS.items():
        rs, okw = scenario_reads(name)
        o = scenario_oracle(name)
        ont = bool(okw.get("is_ont"))
        d = tempfile.mkdtemp(prefix="hao_wlist_")
        fa = os.path.join(d, "r.fq" if ont else "r.fa")
        synth.write_fasta(fa, rs, fastq=ont)

        def harness(tasks, traced):
            t = np.array(tasks, dtype=np.int64).reshape(-1, 10).astype(np.uint32)
            fn = os.path.join(d, "t.u32"); t.tofile(fn)
            cmd = [os.path.join(ROOT, "oracle", "_ref", "ref_harness"), "-t", "2", "--dump", os.path.join(d, "s"), "--reads-list", "/dev/null", "--no-tables",
                   "--eds-tasks" if traced else "--ed-tasks", fn] + (["--ont"] if ont else []) + [fa]
            r_ = subprocess.run(cmd, capture_output=True, text=True)
            assert r_.returncode == 0, r_.stderr[-2000:]
            if traced:
                r = np.fromfile(os.path.join(d, "s.eds.i32"), dtype=np.int32).reshape(-1, 6)
                cg = np.fromfile(os.path.join(d, "s.eds_cig.u16"), dtype=np.uint16)
                res, at = [], 0
                for x in r:
                    n = int(x[5]); res.append((int(x[0]), int(x[1]), int(x[2]), tuple(int(c) for c in cg[at:at + n]))); at += n
                assert at == cg.shape[0]
                return res
            r = np.fromfile(os.path.join(d, "s.ed.i32"), dtype=np.int32).reshape(-1, 2)
            return [(int(x[0]), 0, int(x[1])) for x in r]

        reads = sorted(set(range(0, rs.n, stride)) | set(FORCED.get(key, ())))
        table, want = {}, set()

        def get(traced, task):
            k = (bool(traced), tuple(int(x) for x in task))
            if k not in table:
                want.add(k); raise Missing()
            return table[k]
        align = lambda task, traced: get(traced, task)[:3]
        trace = lambda task: get(True, task)

        per = {}
        for r in reads:
            ol, fc, fo, _ = o.lchain(r)
            per[r] = (ol, fc, fo, RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate))
        allp = [tuple(int(x) for x in t) for r in reads for t in per[r][3]]
        for t, v in zip(allp, harness(allp, False)):
            table[(False, t)] = v
        rounds, results = 0, {}
        while True:
            want.clear()
            for r in reads:
                ol, fc, fo, T = per[r]
                T2, infos = RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate, with_info=True)
                prim = [dict() for _ in range(len(ol))]
                k = 0
                for i, w, info in infos:
                    if info["unresolved"] or info["refused"]:
                        continue
                    v = table[(False, tuple(int(x) for x in T2[k]))]
                    prim[i][w] = (T2[k], v[0], v[2]); k += 1
                for i in range(len(ol)):
                    if (r, i) in results:
                        continue
                    try:
                        rr = RM.rescue_overlap(ol[i], rs.lengths, wl, e_rate, prim[i], align)
                        results[(r, i)] = WM.wlist_overlap(ol[i], rs.lengths, wl, prim[i], rr, trace)
                    except Missing:
                        pass
            if not want:
                break
            rounds += 1
            for traced in (False, True):
                ks = sorted(k for k in want if k[0] == traced)
                if ks:
                    for k, v in zip(ks, harness([k[1] for k in ks], traced)):
                        table[k] = v
        wins, woff, cig, coff, cnt, seen = [], [0], [], [0], [], {}
        for r in reads:
            for i in range(len(per[r][0])):
                W, cs, ev, sw, nt = results[(r, i)]
                wins.append(W); woff.append(woff[-1] + W.shape[0]); cnt.append([sw, nt])
                for c in cs:
                    cig.extend(c); coff.append(len(cig))
                for c in ev:
                    seen[c] = seen.get(c, 0) + 1
        W = np.concatenate(wins).reshape(-1, 8) if wins else np.zeros((0, 8), dtype=np.int64)
        out[key + "_cfg"] = np.array([wl, e_rate], dtype=np.float64)
        out[key + "_reads"] = np.array(reads, dtype=np.uint32)
        out[key + "_wins"] = W.astype(np.int32)
        out[key + "_win_off"] = np.array(woff, dtype=np.int64)
        out[key + "_cig"] = np.array(cig, dtype=np.uint16)
        out[key + "_cig_off"] = np.array(coff, dtype=np.int64)
        out[key + "_swept_tried"] = np.array(cnt, dtype=np.int32).reshape(-1, 2)
        out[key + "_counts"] = np.array([rounds, int(W[:, 7].sum()) if W.shape[0] else 0], dtype=np.int64)      # rounds, untraced windows
        print(key, (name, wl, e_rate), len(reads), "reads,", len(cnt), "overlaps,", W.shape[0], "records,", len(cig), "entries,", rounds, "rounds,", int(out[key + "_counts"][1]), "untraced;", dict(sorted(seen.items())), flush=True)
        for c, v in seen.items():
            total[c] = total.get(c, 0) + v
    print("all configurations:", dict(sorted(total.items())))
    for c in NEED:
        assert total.get(c, 0) > 0, c
    np.savez_compressed(os.path.join(HERE, "wlist.npz"), **out)


if __name__ == "__main__":
    main()
