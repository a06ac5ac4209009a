"""Golden vectors for cal_estimate_err (Correct.cpp:15369-15401; hao_window_estimate_err, hao_window_ladder_adv with estimate_err < 0 on a stretch longer than
wl) from the REAL reference's own function.  ref_harness cannot call it, so this script writes a throw-away driver of a few lines into a temporary directory -
it includes the reference's Correct.h where it lies, declares the function, fills an overlap_region with the records it reads and prints the return value per
query - links it against the objects build() has left in oracle/_ref/obj/ (the reference's, everything but ref_harness.o) and runs it.  Neither the driver nor
the binary enters the repository: the fixture holds data arrays only.

real: the "ont" scenario at wl = 375, e_rate = ladder_adv.npz's 0.07 - the window lists of tests/wlist_model.py over the oracle (tests/test_wlist_cpu.py holds
that against the reference's lists in wlist.npz) for read 0, whose overlaps the ladder fixture's requests name, and for the scenario's first overlap with verdict 0
(read 9: a batch of the first ten reads holds every case).  Queries per overlap: whole windows; a start and an end inside a window with error > 0; qs == x_end, x_end + 1, qe == x_start,
x_start + 1; stretches longer than wl up to the whole overlap; a stretch beyond the last record with qe > x_pos_e + 1 (the early exit, the unclamped length); a
stretch before x_pos_s (a negative value); an empty list; first / last windows cut by x_pos_s / x_pos_e.  On four overlaps of read 0, two per strand, the
`ladder` queries: record-to-record gaps, wl + 1, four records and the whole overlap, with the target interval a ladder request over them takes.
A stretch across an UNALIGNED window does not exist in real lists: align_hc_ed_post_extz gives an overlap whose rescue leaves a window unaligned verdict 0 and
the list is dropped - scanned with the model over the oracle on ont (375, 0.07 / 0.04 / 0.015), hifi and nn (375, 0.01) and edge (375, 0.07): thousands of
empty lists, no list with a hole.  That category is left to the crafted records.
crafted: hand-made records (the host twin runs them; no read set behind them): one record, holes of several windows, error 0 and 255, e_rate 0.07, 0.001,
0.5, 0 and 1 with lengths at which the products land next to an integer.
Every category is counted and asserted non-empty (NEED).
Run in the build container only:  python tests/golden/make_golden_estimate.py  -> tests/golden/estimate_err.npz (data arrays only)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import scenario_reads, scenario_oracle  # noqa: E402
import rescue_model as RM  # noqa: E402
import wlist_model as WM  # noqa: E402
import estimate_model as EM  # noqa: E402

REF = "/root/reference"
NAME, WL, E_RATE, BATCH = "ont", 375, 0.07, 10
CATS = ("whole_windows", "inside_err_window", "at_x_end", "at_x_end_plus1", "at_x_start", "at_x_start_plus1", "longer_than_wl", "whole_overlap", "beyond_last_unclamped",
        "before_x_pos_s", "negative_value", "empty_list", "first_window_cut", "last_window_cut", "ladder", "crafted_one_record", "crafted_hole", "crafted_err0",
        "crafted_err255", "crafted_next_to_integer", "crafted_across_unaligned")
NEED = CATS
REFOBJS = ("CommandLines Process_Read Assembly Hash_Table POA Correct Levenshtein_distance Overlaps Trio kthread Purge_Dups hist sketch extract sys hic rcut horder ecovlp tovlp "
           "inter kalloc gfa_ut gchain_map anchor ref_htab_dump").split()      # (oracle/Makefile's link line without ref_harness.o)

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "Correct.h"
int64_t cal_estimate_err(overlap_region *z, int64_t wl, int64_t qs, int64_t qe, double e_rate);
int main(void)
{
	long n_ov;
	if (scanf("%ld", &n_ov) != 1) return 2;
	for (long i = 0; i < n_ov; ++i) {
		long xs, xe, nr, nq;
		if (scanf("%ld %ld %ld", &xs, &xe, &nr) != 3) return 2;
		overlap_region z; memset(&z, 0, sizeof(z));
		z.x_pos_s = (uint32_t)xs; z.x_pos_e = (uint32_t)xe;
		z.w_list.n = z.w_list.m = (size_t)nr; z.w_list.a = (window_list*)calloc(nr + 1, sizeof(window_list));
		for (long k = 0; k < nr; ++k) {
			long a, b, e;
			if (scanf("%ld %ld %ld", &a, &b, &e) != 3) return 2;
			z.w_list.a[k].x_start = (int32_t)a; z.w_list.a[k].x_end = (int32_t)b; z.w_list.a[k].y_start = 0; z.w_list.a[k].y_end = 0; z.w_list.a[k].error = (int16_t)e;
		}
		if (scanf("%ld", &nq) != 1) return 2;
		for (long k = 0; k < nq; ++k) {
			long wl, qs, qe; double er;
			if (scanf("%ld %ld %ld %la", &wl, &qs, &qe, &er) != 4) return 2;
			printf("%lld\n", (long long)cal_estimate_err(&z, wl, qs, qe, er));
		}
		free(z.w_list.a);
	}
	return 0;
}
"""


def reference_values(groups):
    """groups = [(xs, xe, [(x_start, x_end, error)], [(wl, qs, qe, e_rate)])] -> the reference's return value per query, flat"""
    d = tempfile.mkdtemp(prefix="hao_estimate_")
    src, exe = os.path.join(d, "drv.cpp"), os.path.join(d, "drv")
    open(src, "w").write(DRIVER)
    objs = [os.path.join(ROOT, "oracle", "_ref", "obj", o + ".o") for o in REFOBJS]
    assert all(os.path.exists(o) for o in objs), "run build() first: oracle/_ref/obj is incomplete"
    subprocess.check_call(["g++", "-O3", "-msse4.2", "-mpopcnt", "-fomit-frame-pointer", "-w", "-I" + REF, src] + objs + ["-o", exe, "-lz", "-lpthread", "-lm"])
    lines = [str(len(groups))]
    for xs, xe, recs, qs in groups:
        lines.append(f"{xs} {xe} {len(recs)}")
        lines += [f"{a} {b} {e}" for a, b, e in recs]
        lines.append(str(len(qs)))
        lines += [f"{wl} {a} {b} {float(er).hex()}" for wl, a, b, er in qs]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [int(x) for x in r.stdout.split()]
    assert len(out) == sum(len(g[3]) for g in groups)
    return out


def real_cases():
    """-> overlaps [(read, index, z, wins int64 [m, 8])], queries [(overlap slot, qs, qe, category, ts, te)] (ts / te: the `ladder` queries' target interval, else -1)"""
    rs, _ = scenario_reads(NAME)
    o = scenario_oracle(NAME)
    align, trace = RM.oracle_aligner(o), WM.oracle_tracer(o)
    lists = {}
    for r in range(rs.n):
        ol, fc, fo, _ = o.lchain(r)
        T = RM.M.read_tasks(ol, fc, fo, rs.lengths, WL, E_RATE)
        res = o.window_ed(T) if T.shape[0] else np.zeros((0, 2), dtype=np.int32)
        for i, (z, w) in enumerate(zip(ol, WM.read_wlist(ol, fc, fo, rs.lengths, WL, E_RATE, res, align, trace)[1])):
            lists[(r, i)] = (z, w[0])
            assert w[0].shape[0] == 0 or (np.diff(w[0][:, 0]) == 1).all(), "a real list with a hole: give it a category"
    empty = [k for k, (z, w) in lists.items() if w.shape[0] == 0]
    assert empty
    pick = [k for k in lists if k[0] == 0] + empty[:1]
    assert empty[0][0] < BATCH      # (the GPU test runs the chain on a batch of the first BATCH reads)
    ovs, qs, lad = [], [], {0: 0, 1: 0}
    for r, i in pick:
        z, W = lists[(r, i)]
        s = len(ovs); ovs.append((r, i, z, W))
        xs, xe, q_tot, t_tot = int(z[1]), int(z[2]), int(rs.lengths[int(z[0])]), int(rs.lengths[int(z[4])])
        add = lambda a, b, cat, ts=-1, te=-1: qs.append((s, max(0, min(a, q_tot)), max(0, min(b, q_tot)), cat, ts, te)) if 0 <= min(a, q_tot) <= min(b, q_tot) else None
        if W.shape[0] == 0:
            add(xs, xe + 1, "empty_list"); add(xs + 10, min(xe + 1, xs + 10 + WL + 1), "empty_list"); add(max(0, xs - 50), xs + 700, "empty_list")
            continue
        rec = [EM.window(z, int(x[0]), WL) + (int(x[3]),) for x in W]
        if xs % WL:
            add(rec[0][0], rec[0][1] + 1, "first_window_cut"); add(rec[0][0] + 3, rec[min(2, len(rec) - 1)][1] + 1, "first_window_cut")
        if (xe + 1) % WL:
            add(rec[-1][0], rec[-1][1] + 1, "last_window_cut"); add(rec[max(0, len(rec) - 3)][0] + 7, rec[-1][1], "last_window_cut")
        add(xs, xe + 1, "whole_overlap"); add(0, q_tot, "whole_overlap")
        add(rec[-1][1] + 1, q_tot, "beyond_last_unclamped"); add(rec[-1][1] + 2, q_tot, "beyond_last_unclamped"); add(rec[-1][1], q_tot, "beyond_last_unclamped")
        for d in (15, 200, 1000):                        # the stretch ends d bases before the overlap starts: (qe - qs) * e_rate after the clamp, negative
            if xs - d > 0:
                add(0, xs - d, "before_x_pos_s")
        if xs >= 2:
            add(0, xs - 1, "before_x_pos_s"); add(max(0, xs - 500), xs, "before_x_pos_s"); add(0, xs + 1, "before_x_pos_s"); add(max(0, xs - 400), xs + 30, "before_x_pos_s")
        for k in range(0, len(rec), max(1, len(rec) // 4)):
            a, b, e = rec[k]
            add(a, b + 1, "whole_windows")
            if k + 2 < len(rec):
                add(a, rec[k + 2][1] + 1, "whole_windows"); add(a, rec[k + 1][1] + 1 + 1, "longer_than_wl"); add(a + 100, rec[k + 2][1] - 50, "longer_than_wl")
            add(b, min(xe + 1, b + WL + 40), "at_x_end"); add(b + 1, min(xe + 1, b + 1 + WL + 40), "at_x_end_plus1")
            add(max(xs, a - WL - 40), a, "at_x_start"); add(max(xs, a - WL - 40), a + 1, "at_x_start_plus1")
        for k, (a, b, e) in enumerate(rec):
            if e > 0 and b - a > 200 and k + 1 < len(rec):
                add(a + 101, rec[k + 1][1] + 1, "inside_err_window"); add(a + 1, b + 1 + 123, "inside_err_window"); add(max(xs, a - WL), b - 17, "inside_err_window")
                add(a + 33, b - 33, "inside_err_window")
        rev = int(z[7])
        if r == 0 and len(rec) >= 6 and lad[rev] < 2 and xe + 1 - xs <= 9000:      # the ladder's stretches: mode 0 over the records' own target interval
            lad[rev] += 1
            ys = lambda k: int(W[k, 1]); ye = lambda k: int(W[k, 2])
            for k in (1, 3):
                add(rec[k][0], rec[k + 1][1] + 1, "ladder", ys(k), ye(k + 1) + 1)
            add(rec[1][0], rec[1][0] + WL + 1, "ladder", ys(1), min(t_tot, ys(1) + WL + 1))
            add(rec[1][0], rec[4][1] + 1, "ladder", ys(1), ye(4) + 1)
            add(xs, xe + 1, "ladder", ys(0), ye(len(rec) - 1) + 1)
    assert lad == {0: 2, 1: 2}, lad
    return ovs, qs


def crafted_cases():
    """-> [(xs, xe, [(grid window, error)], [(qs, qe, e_rate, category)])] at wl = WL"""
    out = []
    xs, xe = 1000, 9000                                   # windows 2 .. 24, the first and the last cut
    full = [(w, (w * 37) % 23) for w in range(2, 25)]
    rates = (0.07, 0.001, 0.5, 0.0, 1.0)

    def near_integer(e_rate):
        """lengths whose product with e_rate lands next to an integer"""
        if e_rate in (0.0, 1.0):
            return [1, 376, 1000]
        ls = []
        for k in range(1, 400):
            for d in (-1, 0, 1):
                l = int(round(k / e_rate)) + d
                if 0 < l < 7000 and abs(l * e_rate - round(l * e_rate)) < 2 * e_rate:
                    ls.append(l)
        return sorted(set(ls))[::max(1, len(set(ls)) // 40)]
    q = []
    for er in rates:
        for l in near_integer(er):
            q.append((1500, 1500 + l, er, "crafted_next_to_integer")); q.append((1000, 1000 + l, er, "crafted_next_to_integer"))
    out.append((xs, xe, full, q))
    # one record; holes of several windows; error 0 and 255
    one = [(10, 9)]
    q = [(a, b, er, "crafted_one_record") for er in rates for a, b in ((1000, 9001), (3750, 4125), (3751, 4124), (3700, 4200), (1000, 3750), (1000, 3751), (4124, 9001), (4125, 9001), (4126, 9001), (3000, 3600), (5000, 6000), (500, 800), (9100, 9500))]
    out.append((xs, xe, one, q))
    holes = [(2, 5), (3, 0), (7, 255), (8, 255), (9, 1), (15, 0), (16, 12), (24, 255)]
    spans = ((1000, 9001), (1125, 1500), (1500, 2625), (1400, 2700), (1500, 5626), (1501, 3376), (2625, 3375), (2626, 5000), (1300, 6001), (3375, 3750), (3374, 3751), (3000, 5625), (3001, 6000),
             (6000, 9001), (8999, 9001), (9000, 9001), (6375, 9000), (4000, 5000), (2400, 2800), (0, 1000), (0, 999), (0, 1300), (9001, 9600), (9002, 9600), (8000, 9600))
    q = []
    for er in rates:
        for a, b in spans:
            cat = "crafted_across_unaligned" if (a < 1500 < b or a < 3750 < b or a < 8000 < b) else "crafted_hole"
            q.append((a, b, er, cat))
        q += [(1500, 1875, er, "crafted_err0"), (1400, 1900, er, "crafted_err0"), (5625, 6000, er, "crafted_err0"), (5700, 6300, er, "crafted_err0"),
              (2625, 3375, er, "crafted_err255"), (2700, 3100, er, "crafted_err255"), (2626, 3374, er, "crafted_err255"), (8900, 9001, er, "crafted_err255"), (9000, 9001, er, "crafted_err255")]
    out.append((xs, xe, holes, q))
    # an overlap inside one window, and one that starts and ends on the grid
    out.append((400, 700, [(1, 3)], [(a, b, er, "crafted_one_record") for er in rates for a, b in ((400, 701), (401, 700), (0, 800), (0, 400), (0, 399), (701, 900), (700, 900), (500, 501))]))
    out.append((750, 1874, [(2, 255), (4, 7)], [(a, b, er, "crafted_hole") for er in rates for a, b in ((750, 1875), (750, 1126), (1124, 1501), (1125, 1500), (1126, 1499), (1000, 1700), (1499, 1875), (1500, 1501))]))
    return out


def main():
    ovs, rq = real_cases()
    groups = []
    for s, (r, i, z, W) in enumerate(ovs):
        recs = [EM.window(z, int(x[0]), WL) + (int(x[3]),) for x in W]
        groups.append((int(z[1]), int(z[2]), recs, [(WL, a, b, E_RATE) for t, a, b, *_ in rq if t == s]))
    order = [k for s in range(len(ovs)) for k, q in enumerate(rq) if q[0] == s]
    vals = reference_values(groups)
    real_val = np.zeros(len(rq), dtype=np.int64)
    real_val[order] = vals
    cr = crafted_cases()
    cgroups = [(xs, xe, [EM.window((0, xs, xe), w, WL) + (e,) for w, e in recs], [(WL, a, b, er) for a, b, er, _ in q]) for xs, xe, recs, q in cr]
    cvals = reference_values(cgroups)
    seen = {}
    for (s, a, b, cat, ts, te), v in zip(rq, real_val):
        seen[cat] = seen.get(cat, 0) + 1
        if v < 0:
            seen["negative_value"] = seen.get("negative_value", 0) + 1
        if b - a > WL:
            seen["longer_than_wl"] = seen.get("longer_than_wl", 0) + 1
    for xs, xe, recs, q in cr:
        for a, b, er, cat in q:
            seen[cat] = seen.get(cat, 0) + 1
    print(len(ovs), "real overlaps,", len(rq), "real queries,", sum(len(g[3]) for g in cr), "crafted queries;", dict(sorted(seen.items())))
    for c in NEED:
        assert seen.get(c, 0) > 0, c
    # the model agrees before anything is written (the CPU test asserts it again on the committed file)
    for (s, a, b, *_), v in zip(rq, real_val):
        assert EM.estimate_err(ovs[s][2], ovs[s][3], WL, a, b, E_RATE) == v, (s, a, b, v)
    woff = np.concatenate([[0], np.cumsum([o[3].shape[0] for o in ovs])]).astype(np.int64)
    c_ovlp, c_wins, c_woff, c_q, c_er, c_cat, k = [], [], [0], [], [], [], 0
    for s, (xs, xe, recs, q) in enumerate(cr):
        c_ovlp.append([0, xs, xe, 0, 1, 0, xe - xs, 0, 1, 0, 0, 0]); c_wins += [[w, 0, 0, e, 0, 3, 0, 0] for w, e in recs]; c_woff.append(len(c_wins))
        for a, b, er, cat in q:
            c_q.append([s, a, b]); c_er.append(er); c_cat.append(CATS.index(cat))
    out = {"cfg": np.array([WL, E_RATE], dtype=np.float64), "cats": np.array(CATS),
           "ov_read": np.array([o[0] for o in ovs], dtype=np.int32), "ov_idx": np.array([o[1] for o in ovs], dtype=np.int32), "ovlp": np.array([o[2] for o in ovs], dtype=np.uint32).reshape(-1, 12),
           "win_off": woff, "wins": (np.concatenate([o[3] for o in ovs]) if ovs else np.zeros((0, 8))).astype(np.int32).reshape(-1, 8),
           "real_q": np.array([[s, a, b, ts, te] for s, a, b, cat, ts, te in rq], dtype=np.int32), "real_cat": np.array([CATS.index(q[3]) for q in rq], dtype=np.uint8), "real_val": real_val,
           "c_ovlp": np.array(c_ovlp, dtype=np.uint32), "c_win_off": np.array(c_woff, dtype=np.int64), "c_wins": np.array(c_wins, dtype=np.int32).reshape(-1, 8),
           "c_q": np.array(c_q, dtype=np.int32), "c_erate": np.array(c_er, dtype=np.float64), "c_cat": np.array(c_cat, dtype=np.uint8), "c_val": np.array(cvals, dtype=np.int64)}
    fn = os.path.join(HERE, "estimate_err.npz")
    np.savez_compressed(fn, **out)
    print(os.path.getsize(fn), "bytes")
    assert os.path.getsize(fn) < (1 << 20)


if __name__ == "__main__":
    main()
