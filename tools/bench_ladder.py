# The device-resident threshold ladder (hao_window_ladder) against the host-driven loop it replaces - per round one hao_window_trace_long call per mode over the open
# requests' tasks, survivors picked on the host - on the same requests, the same library, the same kernels underneath.
# Requests: the gaps of the verdict-1 overlaps of a batch of query reads of BASELINE configs[1] (bacterial5M_hifi30x; the index holds every read, --reads query
# reads form the batch) after hao_window_ed_ref / hao_window_rescue_ref / hao_window_wlist_ref at 775-base windows and e_rate 0.04: per overlap the global
# stretch from each window record to the next (anchored on the records' y_start / y_end), the forward extension behind the last record, the backward extension
# before the first, and every global stretch once more with ts = te = -1 (mode 3).
# Times: the host's clock around calls that end in a stream synchronise; three warm-up runs of each side, then --reps timed runs ALTERNATING the two sides; best
# and median.  The loop's time counts its hao_window_trace_long calls ONLY: the coordinate step and the picking of survivors run in Python here (tests/ladder_model.py)
# and are reported beside it, not in it - a C caller would do them faster, and nobody would do them in no time.  The records of the two sides are compared first.
# usage: bench_ladder.py [--reads N] [--reps N] [--out FILE] [--dry]      (--dry: build the read set only - runs without a GPU)
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from hifiasm_amd import workloads  # noqa: E402
import ladder_model as LM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=48); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--out", default=None); ap.add_argument("--dry", action="store_true")
ap.add_argument("--workload", default="bacterial5M_hifi30x"); ap.add_argument("--scenario", default=None)      # --scenario NAME: one of the tests' small read sets instead (a rehearsal, not a measurement)
a_ = ap.parse_args()
WL, E_RATE_W = 775, 0.04                  # the window lists' grid
E_RATE, MAXL, MAXE = 0.04, 10000, 2047    # the ladder's call parameters (MAX_SIN_L, MAX_SIN_E)

if a_.scenario:
    from helpers import scenario_reads
    rs, okw = scenario_reads(a_.scenario); a_.workload = "scenario " + a_.scenario; a_.reads = min(a_.reads, rs.n)
else:
    rs, okw = workloads.workload_reads(a_.workload, want_codes=False), {}
print(f"{a_.workload}: {rs.n} reads, {int(rs.lengths.sum())} bases; batch = reads [0, {a_.reads})", flush=True)
if a_.dry:
    raise SystemExit(0)
from hifiasm_amd.api import Engine  # noqa: E402
e = Engine(0, **okw)
e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
e.overlap_batch(0, a_.reads)
e.window_ed_ref(WL, E_RATE_W); e.window_rescue_ref(); e.window_wlist_ref()
L = rs.lengths.astype(np.int64)
rows, ctx, base = [], [], 0
for r in range(a_.reads):
    ol, fc, fo, _ = e.h_ec_lchain(r)
    for i, (W, _cg) in enumerate(e.fetch_wlist(r)):
        if W.shape[0] < 2:
            continue
        z = ol[i]; xs, xe = int(z[1]), int(z[2]); q_tot, t_tot = int(L[int(z[0])]), int(L[int(z[4])])
        span = [(max(int(w) * WL, xs), min(int(w) * WL + WL - 1, xe)) for w in W[:, 0]]
        k0 = len(rows)
        for k in range(W.shape[0] - 1):
            rows.append([base + i, 0, span[k][0], span[k + 1][1] + 1, int(W[k, 1]), int(W[k + 1, 2]) + 1, int(W[k, 3]) + int(W[k + 1, 3])])
            rows.append([base + i, 0, span[k][0], span[k + 1][1] + 1, -1, -1, int(W[k, 3]) + int(W[k + 1, 3])])
        rows.append([base + i, 1, span[-1][1] + 1, q_tot, int(W[-1, 2]) + 1, t_tot, 0])
        rows.append([base + i, 2, 0, span[0][0], 0, int(W[0, 1]), 0])
        ctx += [(z, fc[int(fo[i]) - int(fo[0]):int(fo[i + 1]) - int(fo[0])])] * (len(rows) - k0)
    base += ol.shape[0]
rows = np.array(rows, dtype=np.int64).reshape(-1, 7)
ok = np.array([not LM.check_request(ctx[k][0], L, [int(x) for x in rows[k]], E_RATE, MAXL, MAXE) for k in range(rows.shape[0])], dtype=bool)      # (a record pair whose y_start / y_end do not ascend names no stretch)
rows = rows[ok]; ctx = [c for c, k in zip(ctx, ok) if k]
print(f"{rows.shape[0]} requests over {base} overlaps", flush=True)


def device():
    t0 = time.time(); out = e.window_ladder(rows, E_RATE, MAXL, MAXE); return time.time() - t0, out


def host_loop():
    """-> (seconds inside hao_window_trace_long, seconds of host work, records, cigars)"""
    table, want, t_dev = {}, set(), 0.0

    class Missing(Exception):
        pass

    def aligner(mode, task):
        k = (mode, task)
        if k not in table:
            want.add(k); raise Missing()
        return table[k]
    t_all = time.time(); done = {}
    while True:
        want.clear()
        for k in range(rows.shape[0]):
            if k in done:
                continue
            try:
                done[k] = LM.ladder(ctx[k][0], ctx[k][1], L, [int(x) for x in rows[k]], E_RATE, MAXL, MAXE, aligner)
            except Missing:
                pass
        if not want:
            break
        for mode in range(4):
            ts = sorted(t for m, t in want if m == mode)
            if ts:
                T = np.array(ts, dtype=np.int64).astype(np.uint32); cap = 2 * int(T[:, 8].max()) + 8
                t0 = time.time(); r, c = e.window_trace_long(T, cap=cap, mode=mode); t_dev += time.time() - t0
                for t, x, row in zip(ts, r, c):
                    table[(mode, t)] = tuple(int(v) for v in x[:5]) + (tuple(int(v) for v in row[:int(x[5])]),)
    return t_dev, time.time() - t_all - t_dev, done


_, (res, off, cig) = device()
_, _, done = host_loop()
for k in range(rows.shape[0]):      # the two sides agree before either is timed
    rec, cg = done[k]
    assert tuple(int(res[f][k]) for f in LM.FIELDS) == tuple(int(x) for x in rec), (k, res[k], rec)
    assert tuple(int(x) for x in cig[int(off[k]):int(off[k + 1])]) == cg, k
for _ in range(2):
    device(); host_loop()
td, tl, th = [], [], []
for _ in range(a_.reps):
    td.append(device()[0]); x = host_loop(); tl.append(x[0]); th.append(x[1])
share = np.bincount(res["rung"], minlength=5) / max(1, rows.shape[0])
report = {"workload": a_.workload, "batch_reads": a_.reads, "requests": int(rows.shape[0]), "overlaps": int(base), "cigar_entries": int(off[-1]),
          "open_requests_per_round": e.ladder_rounds(), "share_per_rung_0_to_4": [round(float(x), 5) for x in share],
          "hao_window_ladder_ms": {"best": round(min(td) * 1e3, 3), "median": round(float(np.median(td)) * 1e3, 3)},
          "host_loop_trace_calls_ms": {"best": round(min(tl) * 1e3, 3), "median": round(float(np.median(tl)) * 1e3, 3)},
          "host_loop_python_ms_not_counted": {"best": round(min(th) * 1e3, 1), "median": round(float(np.median(th)) * 1e3, 1)}, "reps": a_.reps, "warmup": 3}
print(json.dumps(report), flush=True)
if a_.out:
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    json.dump(report, open(a_.out, "w"), indent=1)
e.close()
