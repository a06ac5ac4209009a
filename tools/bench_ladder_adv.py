# hao_window_ladder_adv (the device-resident ladder of hc_aln_exz_adv) against the host-driven loop it replaces - per round the coordinate step of cal_exz_infi_adv on
# the host, one hao_window_trace_long call per mode over the open requests' tasks, survivors picked on the host - on the same requests, the same library, the same
# kernels underneath: tools/bench_ladder.py's comparison for the second ladder.
# Requests: those of tests/golden/ladder_adv.npz's first group (the "ont" scenario's overlaps; wl 375, MAX_SIN_L / MAX_SIN_E / FORCE_SIN_L), every one of them
# --requests / their-number times over, copy after copy (default: about 10^5 requests).  The fixture was made to meet every branch of the ladder, not to look like a
# run of reads: rungs 2 - 5, wide bands and requests without an alignment are far more frequent in it than among the gaps of real overlaps.
# The loop sends one task per OPEN REQUEST and round, as a caller without the device-resident ladder has to (equal tasks of different requests are not merged), and
# asks hao_window_trace_long for 2 * (the call's widest threshold) + 8 cigar entries per task - the call takes one capacity for all its tasks.
# Times: the host's clock around calls that end in a stream synchronise; warm-up runs of each side, then --reps timed runs ALTERNATING the two sides; best and median.
# The loop's time counts its hao_window_trace_long calls ONLY.  Its coordinate steps and the picking of survivors run in Python (tests/ladder_adv_model.py) over ONE copy
# of the requests and are reported beside it, not in it and not multiplied - a C caller would do them faster, and nobody would do them in no time.
# Both sides' records are compared with each other and with the fixture before either is timed, and the open requests per round of the device with the loop's.
# usage: bench_ladder_adv.py [--requests N] [--reps N] [--warmup N] [--out FILE] [--dry]      (--dry: requests and the loop's tasks per round from the fixture's table of
#        alignments - runs without a GPU)
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from helpers import scenario_reads, GOLDEN  # noqa: E402
import ladder_adv_model as AM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--requests", type=int, default=100000); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None); ap.add_argument("--dry", action="store_true")
a_ = ap.parse_args()
NAME, GROUP = "ont", 0

g = np.load(os.path.join(GOLDEN, "ladder_adv.npz"))
g = {k: g[k] for k in g.files}
CFG = (float(g["cfg"][GROUP][0]),) + tuple(int(x) for x in g["cfg"][GROUP][1:])      # e_rate, wl, maxl, maxe, force_l
pos = np.flatnonzero(g["grp"] == GROUP)
COPIES = max(1, round(a_.requests / pos.size))
rs, okw = scenario_reads(NAME)
bases = AM.reads_bases(rs)
print(f"scenario {NAME}: {rs.n} reads; {pos.size} requests x {COPIES} copies = {pos.size * COPIES}; e_rate, wl, maxl, maxe, force_l = {CFG}", flush=True)


class Missing(Exception):
    pass


def host_loop(ctx, trace):
    """the loop over ONE copy of the requests; trace(mode, tasks as int rows) -> [(err, ps, pe, ts, te, cigar tuple)] is where the caller's hao_window_trace_long call
    goes (it sends every task COPIES times over).  -> (records and cigars by request, the open requests of each round, seconds outside trace)"""
    table, done, n_att, t_in = {}, {}, {}, 0.0
    t_all = time.time()
    while True:
        want = {}      # request -> (mode, task) it waits for
        for k in pos:
            if int(k) in done:
                continue
            q = g["req"][k]
            ol, fc, fo, _ = ctx[int(q[0])]
            i = int(q[1]); a = []

            def aligner(mode, task):
                key = (mode, tuple(int(x) for x in task))
                if key not in table:
                    want[int(k)] = key; raise Missing()
                return table[key]
            try:
                done[int(k)] = AM.ladder(ol[i], fc[int(fo[i]) - int(fo[0]):int(fo[i + 1]) - int(fo[0])], rs.lengths, [0] + [int(x) for x in q[2:]], *CFG, aligner, bases, att=a)
                n_att[int(k)] = a[-1] if a else 0
            except Missing:
                pass
        if not want:
            break
        for mode in range(4):
            ts = [t for m, t in want.values() if m == mode]      # one task per open request
            if ts:
                t0 = time.time(); out = trace(mode, ts); t_in += time.time() - t0
                for t, x in zip(ts, out):
                    table[(mode, t)] = x
    rounds = [sum(1 for n in n_att.values() if n > j) for j in range(5)]
    return done, rounds, time.time() - t_all - t_in


if a_.dry:      # the fixture's own table in the aligner's place, the fixture's overlaps and the oracle's fake cigars: what the loop would send, round by round
    from helpers import scenario_oracle
    o = scenario_oracle(NAME)
    ctx = {int(r): o.lchain(int(r)) for r in np.unique(g["req"][pos, 0])}
    tab = {(int(m), tuple(int(x) for x in t)): tuple(int(v) for v in r) + (tuple(int(c) for c in g["tab_cig"][int(a):int(b)]),)
           for m, t, r, a, b in zip(g["tab_mode"], g["tab_task"], g["tab_res"], g["tab_cig_off"][:-1], g["tab_cig_off"][1:])}
    sent = []

    def trace(mode, ts):
        sent.append((mode, len(ts), max(t[8] for t in ts))); return [tab[(mode, t)] for t in ts]
    done, rounds, _ = host_loop(ctx, trace)
    for j, k in enumerate(pos):
        assert tuple(int(x) for x in done[int(k)][0]) == tuple(int(x) for x in g["res"][k]), int(k)
    print("open requests per round (one copy):", rounds, "\ncalls (mode, tasks, widest threshold):", sent)
    raise SystemExit(0)

from hifiasm_amd.api import Engine  # noqa: E402
from test_gpu_ladder import _requests  # noqa: E402
e = Engine(0, **okw)
e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
e.overlap_batch(0, rs.n)
rows1, pos_all = _requests(e, g, 0, rs.n)
rows1 = rows1[np.flatnonzero(g["grp"][pos_all] == GROUP)]
assert rows1.shape[0] == pos.size
rows = np.tile(rows1, (COPIES, 1))
ctx = {int(r): e.h_ec_lchain(int(r)) for r in np.unique(g["req"][pos, 0])}
sent = []      # (mode, tasks, cigar capacity) of the loop's calls, of its last run


def device():
    t0 = time.time(); out = e.window_ladder_adv(rows, *CFG); return time.time() - t0, out


def loop():
    """-> (seconds inside hao_window_trace_long, seconds of host work over one copy, records, rounds)"""
    t_dev = [0.0]; del sent[:]

    def trace(mode, ts):
        T = np.tile(np.array(ts, dtype=np.int64).astype(np.uint32), (COPIES, 1)); cap = 2 * int(T[:, 8].max()) + 8
        t0 = time.time(); r, c = e.window_trace_long(T, cap=cap, mode=mode); t_dev[0] += time.time() - t0
        sent.append((mode, int(T.shape[0]), cap))
        n1 = len(ts)
        assert (r[:n1] == r[-n1:]).all()      # (the last copy's results are the first's)
        return [tuple(int(v) for v in x[:5]) + (tuple(int(v) for v in row[:int(x[5])]),) for x, row in zip(r[:n1], c[:n1])]
    done, rounds, t_host = host_loop(ctx, trace)
    return t_dev[0], t_host, done, rounds


_, (res, off, cig) = device()
dev_rounds = e.ladder_adv_rounds()
_, _, done, rounds = loop()
n1 = pos.size
for j, k in enumerate(pos):      # the two sides agree with each other and with the fixture before either is timed; the last copy equals the first
    rec, cg = done[int(k)]
    for jj in (j, (COPIES - 1) * n1 + j):
        assert tuple(int(res[f][jj]) for f in AM.FIELDS) == tuple(int(x) for x in rec) == tuple(int(x) for x in g["res"][k]), (jj, res[jj], rec)
        assert tuple(int(x) for x in cig[int(off[jj]):int(off[jj + 1])]) == cg, jj
assert dev_rounds == [COPIES * x for x in rounds], (dev_rounds, rounds)
print("records agree; open requests per round:", dev_rounds, flush=True)
for _ in range(max(0, a_.warmup - 1)):
    device(); loop()
td, tl, th = [], [], []
for _ in range(a_.reps):
    td.append(device()[0]); x = loop(); tl.append(x[0]); th.append(x[1])
    print(f"  device {td[-1] * 1e3:.1f} ms, loop's calls {tl[-1] * 1e3:.1f} ms", flush=True)
share = np.bincount(res["rung"], minlength=7) / max(1, rows.shape[0])
report = {"scenario": NAME, "fixture_requests": int(n1), "copies": int(COPIES), "requests": int(rows.shape[0]), "cigar_entries": int(off[-1]),
          "e_rate_wl_maxl_maxe_force_l": list(CFG), "open_requests_per_round": dev_rounds, "share_per_rung_0_to_6": [round(float(x), 5) for x in share],
          "hao_window_ladder_adv_ms": {"best": round(min(td) * 1e3, 3), "median": round(float(np.median(td)) * 1e3, 3)},
          "host_loop_trace_calls_ms": {"best": round(min(tl) * 1e3, 3), "median": round(float(np.median(tl)) * 1e3, 3)},
          "host_loop_trace_calls": [{"mode": m, "tasks": n, "cigar_cap": c} for m, n, c in sent],
          "host_loop_python_ms_one_copy_not_counted": {"best": round(min(th) * 1e3, 1), "median": round(float(np.median(th)) * 1e3, 1)}, "reps": a_.reps, "warmup": a_.warmup}
print(json.dumps(report), flush=True)
if a_.out:
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    json.dump(report, open(a_.out, "w"), indent=1)
e.close()
