# hao_window_ladder_adv on tools/bench_ladder_adv.py's requests with estimate_err = -1 on every stretch longer than wl, after the blocking chain
# (hao_window_ed_ref -> hao_window_rescue_ref -> hao_window_wlist_ref at the fixture's wl and e_rate) has left the batch's window lists on the device: the set-up kernel
# then runs cal_estimate_err over the lists for those requests (hao_ladder.cuh: hao_ld_estimate_wlist).  Beside it, in the same process and alternating, the same
# requests with the fixture's own estimates (bench_ladder_adv.py's device side) - the two runs do NOT make the same attempts: another estimate is another first rung.
# A request whose list value is negative (refused by the ladder) keeps its own estimate; their number is reported.  Also timed: hao_window_estimate_err alone over
# the requests longer than wl.  Times: the host's clock around blocking calls; --warmup runs, then --reps timed runs; best and median.
# usage: bench_ladder_est.py [--requests N] [--reps N] [--warmup N] [--out FILE]
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from helpers import scenario_reads, GOLDEN  # noqa: E402
from test_gpu_ladder import _requests  # noqa: E402
from hifiasm_amd.api import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--requests", type=int, default=100000); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--out", default=None)
a_ = ap.parse_args()
NAME, GROUP = "ont", 0
g = np.load(os.path.join(GOLDEN, "ladder_adv.npz"))
g = {k: g[k] for k in g.files}
CFG = (float(g["cfg"][GROUP][0]),) + tuple(int(x) for x in g["cfg"][GROUP][1:])      # e_rate, wl, maxl, maxe, force_l
E_RATE, WL = CFG[0], CFG[1]
rs, okw = scenario_reads(NAME)
e = Engine(0, **okw)
e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
e.overlap_batch(0, rs.n)
rows1, pos_all = _requests(e, g, 0, rs.n)
rows1 = rows1[np.flatnonzero(g["grp"][pos_all] == GROUP)]
COPIES = max(1, round(a_.requests / rows1.shape[0]))
t0 = time.time(); e.window_ed_ref(WL, E_RATE); e.window_rescue_ref(); out = e.window_wlist_ref(); t_chain = time.time() - t0
long_ = np.flatnonzero((rows1[:, 3] - rows1[:, 2] > WL) & (rows1[:, 3] >= rows1[:, 2]))
val = e.window_estimate_err(rows1[long_], E_RATE, WL)
neg = int((val < 0).sum())
rows_est = rows1.copy(); rows_est[long_[val >= 0], 6] = -1
rows, rows_est = np.tile(rows1, (COPIES, 1)), np.tile(rows_est, (COPIES, 1))
print(f"{rows1.shape[0]} requests x {COPIES} copies; {long_.size} longer than wl, {neg} of them with a negative list value; chain {t_chain * 1e3:.1f} ms, {out[0]} window records", flush=True)


def run(q):
    t0 = time.time(); r = e.window_ladder_adv(q, *CFG); return time.time() - t0, r


def stage():
    q = np.tile(rows1[long_], (COPIES, 1)); t0 = time.time(); e.window_estimate_err(q, E_RATE, WL); return time.time() - t0


_, (res, off, cig) = run(rows_est)
est = e.ladder_adv_estimates()
n1 = rows1.shape[0]
got = est[long_[val >= 0]]
assert ((got == val[val >= 0]) | (got == -1)).all() and (est[:n1] == est[-n1:]).all()      # (-1: behind an early return the lists are not read)
n_list = int((got != -1).sum())
rounds_est = e.ladder_adv_rounds()
for _ in range(max(0, a_.warmup - 1)):
    run(rows); run(rows_est); stage()
ta, tb, ts = [], [], []
for _ in range(a_.reps):
    ta.append(run(rows)[0]); tb.append(run(rows_est)[0]); ts.append(stage())
    print(f"  own estimates {ta[-1] * 1e3:.1f} ms, from the lists {tb[-1] * 1e3:.1f} ms, the stage alone {ts[-1] * 1e3:.2f} ms", flush=True)
ms = lambda t: {"best": round(min(t) * 1e3, 3), "median": round(float(np.median(t)) * 1e3, 3)}
report = {"scenario": NAME, "fixture_requests": int(n1), "copies": int(COPIES), "requests": int(rows.shape[0]), "e_rate_wl_maxl_maxe_force_l": list(CFG),
          "requests_longer_than_wl_per_copy": int(long_.size), "of_them_negative_list_value_kept_own_estimate": neg, "of_them_estimated_from_the_lists_per_copy": n_list, "window_records": int(out[0]), "blocking_chain_ms_once": round(t_chain * 1e3, 3),
          "hao_window_ladder_adv_own_estimates_ms": ms(ta), "hao_window_ladder_adv_estimates_from_lists_ms": ms(tb), "open_requests_per_round_estimates_from_lists": rounds_est,
          "cigar_entries_estimates_from_lists": int(off[-1]), "hao_window_estimate_err_ms": ms(ts), "hao_window_estimate_err_requests": int(long_.size * COPIES), "reps": a_.reps, "warmup": a_.warmup}
print(json.dumps(report), flush=True)
if a_.out:
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    json.dump(report, open(a_.out, "w"), indent=1)
e.close()
