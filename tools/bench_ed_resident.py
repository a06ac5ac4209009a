"""f3 end to end on the device (hao_window_ed_grid): pairs/s INCLUDING task generation on BASELINE configs[1] (10 000 reads of 15 kb) - every overlap of every read of
one all-reads batch on the reference's window grid (WINDOW = 375), one threshold per call.  Prints one JSON line.  usage: python tools/bench_ed_resident.py [thre] [reps]

--deliver: the same alignment in the streaming pass (HAO_DELIVER_ED): passes of hao_overlap_batch_async batches (both slots in flight) with OL|CL and with OL|CL|ED,
alternately; per batch the ED stage's device time (stage_times "ed_grid" + "ed_align"), its pairs/s and the arena bytes it adds; per pass the wall time of the
delivered step.  usage: python tools/bench_ed_resident.py --deliver [--workload W] [--batch-reads N] [--max-batches K] [--thre T] [--reps R]

--window W: the window of the diagonal grid (default 375).  --ref WINDOW,ERATE (blocking and --deliver): the same stage in REFERENCE placement (hao_window_ed_ref /
hao_deliver_ed_config_ref: fake-cigar shift, per-window thresholds, init_waln), e.g. --ref 775,0.04 beside the diagonal stage at --window 775 and thre 31.
--rescue (blocking, with --ref): then the rescue stage (hao_window_rescue_ref) on the same batch: wall and device time per call, rescued windows, verdicts.
--wlist (with --ref --rescue): then the window lists (hao_window_wlist_ref) on the same batch: wall and device time per call, records, windows swept,
re-placement sweeps, cigar entries, untraced windows and their shares.  --deliver --ref W,E --wlist: the streamed pass also with OL|CL|ED|RESCUE and with
OL|CL|ED|RESCUE|WLIST, alternating: wall time per pass and arena bytes per batch."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from hifiasm_amd import workloads
    from hifiasm_amd.api import Engine
    argv = [x for x in sys.argv[1:]]
    ref, window = None, 375
    rescue = "--rescue" in argv
    if rescue:
        argv.remove("--rescue")
    wlist = "--wlist" in argv
    if wlist:
        argv.remove("--wlist")
    for flag in ("--ref", "--window"):
        if flag in argv:
            i = argv.index(flag); val = argv[i + 1]; del argv[i:i + 2]
            if flag == "--ref":
                ref = (int(val.split(",")[0]), float(val.split(",")[1]))
            else:
                window = int(val)
    thre = int(argv[0]) if len(argv) > 0 else 15
    reps = int(argv[1]) if len(argv) > 1 else 5
    rs = workloads.workload_reads("bacterial5M_hifi30x")
    e = Engine(0); e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
    e.overlap_batch(0, rs.n)
    run = (lambda: e.window_ed_ref(*ref)[0]) if ref else (lambda: e.window_ed_grid(window, thre))
    n = run()      # warm-up (allocations)
    ts = []
    for _ in range(reps):
        t0 = time.time(); n = run(); ts.append(time.time() - t0)
    t, r = e.fetch_ed_grid(min(n, 1_000_000))
    ok = int((r[:, 0] != 2**31 - 1).sum())
    extra = {}
    if rescue and ref:      # the rescue stage over the batch the last primary pass left (it may run again on the same batch)
        n_res = e.window_rescue_ref(); tr = []
        for _ in range(reps):
            t0 = time.time(); n_res = e.window_rescue_ref(); tr.append(time.time() - t0)
        dev_ms = dict(e.stage_times()).get("rescue_ref")      # (before the fetches: they are calls of their own)
        v1 = ol = 0
        for r in range(rs.n):
            ov, _ = e.fetch_rescue(r); v1 += int(ov["verdict"].sum()); ol += ov.shape[0]
        extra = {"rescue_ms_per_call_best": round(min(tr) * 1e3, 3), "rescue_ms_per_call_all": [round(x * 1e3, 3) for x in tr], "rescued_windows": n_res,
                 "rescue_device_ms": dev_ms, "verdict1_overlaps": v1, "overlaps_judged": ol,
                 "rescue_over_ed": round(min(tr) / min(ts), 4)}
        if wlist:      # the window lists over the same batch (the stage may run again on the same rescue results)
            out = e.window_wlist_ref(); tw = []
            for _ in range(reps):
                t0 = time.time(); out = e.window_wlist_ref(); tw.append(time.time() - t0)
            extra.update({"wlist_ms_per_call_best": round(min(tw) * 1e3, 3), "wlist_ms_per_call_all": [round(x * 1e3, 3) for x in tw], "wlist_device_ms": dict(e.stage_times()).get("wlist_ref"),
                          "wlist_records": out[0], "wlist_swept": out[1], "wlist_replacement_sweeps": out[2], "wlist_cigar_entries": out[3], "wlist_untraced": out[4],
                          "wlist_share_err0": round((out[0] - out[1] - out[4]) / max(1, out[0]), 4), "wlist_share_swept": round(out[1] / max(1, out[0]), 4),
                          "wlist_share_replacement_tried": round(out[2] / max(1, out[0]), 4), "wlist_share_untraced": round(out[4] / max(1, out[0]), 4)})
    print(json.dumps({**extra, "workload": "bacterial5M_hifi30x", "reads": int(rs.n), "overlaps": e.batch_totals()["overlaps"], "placement": "reference" if ref else "diagonal",
                      "window": ref[0] if ref else window, "thre": None if ref else thre, "e_rate": ref[1] if ref else None, "pairs": n,
                      "ms_per_call_best": round(min(ts) * 1e3, 3), "ms_per_call_all": [round(x * 1e3, 3) for x in ts], "pairs_per_s": round(n / min(ts)),
                      "within_thre_of_first_million": ok, "what": "task generation on the device from ol->list + distance-only window alignment; nothing crosses the host but two totals"}))
    e.close()


def deliver(a):
    from hifiasm_amd import workloads
    from hifiasm_amd.api import Engine, DELIVER_OL, DELIVER_CL, DELIVER_ED, DELIVER_RESCUE, DELIVER_WLIST
    hi_all = workloads.n_reads_of(a.workload)
    rs = workloads.workload_reads(a.workload)
    e = Engine(0); e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
    ref = (int(a.ref.split(",")[0]), float(a.ref.split(",")[1])) if a.ref else None
    if ref:
        e.deliver_ed_config_ref(*ref)
    else:
        e.deliver_ed_config(a.window, a.thre)
    br = a.batch_reads or (rs.n + 1) // 2
    ranges = [(lo, min(hi_all, lo + br)) for lo in range(0, rs.n, br)][:a.max_batches]

    def one_pass(parts):
        per, pending, t0 = [], None, time.time()

        def take(slot, k):
            d = e.deliver_wait(slot)
            per[k].update(bytes=int(d.bytes), pairs=int(d.ed.n_pairs) if d.ed is not None else 0)
        for k, (lo, hi) in enumerate(ranges):
            slot = e.overlap_batch_async(lo, hi, parts=parts)
            st = {}
            for nm, ms in e.stage_times():
                st[nm] = st.get(nm, 0.0) + ms
            per.append(dict(reads=hi - lo, ed_grid_ms=st.get("ed_grid", 0.0), ed_align_ms=st.get("ed_align", 0.0), kernels_ms=sum(st.values())))
            if pending is not None:
                take(*pending)
            pending = (slot, k)
        take(*pending)
        return (time.time() - t0) * 1e3, per

    one_pass(DELIVER_OL | DELIVER_CL | DELIVER_ED); one_pass(DELIVER_OL | DELIVER_CL)      # warm-up (allocations, arenas)
    walls = {"ol_cl": [], "ol_cl_ed": []}; last = {}
    passes = [("ol_cl", DELIVER_OL | DELIVER_CL), ("ol_cl_ed", DELIVER_OL | DELIVER_CL | DELIVER_ED)]
    if a.wlist and ref:      # the rescue stage and the window lists riding along: ED | RESCUE against ED | RESCUE | WLIST
        passes += [("ol_cl_ed_rescue", DELIVER_OL | DELIVER_CL | DELIVER_ED | DELIVER_RESCUE), ("ol_cl_ed_rescue_wlist", DELIVER_OL | DELIVER_CL | DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST)]
        walls.update({"ol_cl_ed_rescue": [], "ol_cl_ed_rescue_wlist": []})
        one_pass(passes[-1][1])      # warm-up
    for _ in range(a.reps):
        for key, parts in passes:
            w, per = one_pass(parts); walls[key].append(round(w, 2)); last[key] = per
    batches = []
    for b0, b1 in zip(last["ol_cl"], last["ol_cl_ed"]):
        ed_ms = b1["ed_grid_ms"] + b1["ed_align_ms"]
        batches.append(dict(reads=b1["reads"], pairs=b1["pairs"], ed_grid_ms=round(b1["ed_grid_ms"], 3), ed_align_ms=round(b1["ed_align_ms"], 3), ed_ms=round(ed_ms, 3),
                            pairs_per_s_ed_stage=round(b1["pairs"] / max(1e-9, ed_ms * 1e-3)), pairs_per_s_align=round(b1["pairs"] / max(1e-9, b1["ed_align_ms"] * 1e-3)),
                            arena_bytes_ol_cl=b0["bytes"], arena_bytes_ol_cl_ed=b1["bytes"], extra_bytes=b1["bytes"] - b0["bytes"],
                            kernels_ms_ol_cl=round(b0["kernels_ms"], 3), kernels_ms_ol_cl_ed=round(b1["kernels_ms"], 3)))
    print(json.dumps({"workload": a.workload, "reads_indexed": int(rs.n), "placement": "reference" if ref else "diagonal", "window": ref[0] if ref else a.window,
                      "thre": None if ref else a.thre, "e_rate": ref[1] if ref else None, "batches": batches,
                      "delivered_step_ms_all": walls, "arena_bytes_last": {k: [b["bytes"] for b in v] for k, v in last.items()},
                      "delivered_step_ms_ol_cl": walls["ol_cl"], "delivered_step_ms_ol_cl_ed": walls["ol_cl_ed"],
                      "delivered_step_ms_best": {k: min(v) for k, v in walls.items()},
                      "what": "passes over the listed batches with both slots in flight: host wall time per pass with OL|CL and with OL|CL|ED (alternating), the ED stage's device time per batch (stage_times), the bytes it adds to the arena"}))
    e.close()


if __name__ == "__main__":
    if "--deliver" in sys.argv:
        ap = argparse.ArgumentParser()
        ap.add_argument("--deliver", action="store_true")
        ap.add_argument("--workload", default="bacterial5M_hifi30x")
        ap.add_argument("--batch-reads", type=int, default=0, help="reads per batch (0: two batches over the read set)")
        ap.add_argument("--max-batches", type=int, default=1 << 30)
        ap.add_argument("--thre", type=int, default=15)
        ap.add_argument("--reps", type=int, default=3)
        ap.add_argument("--window", type=int, default=375)
        ap.add_argument("--ref", default="", help="WINDOW,ERATE: reference placement")
        ap.add_argument("--wlist", action="store_true", help="with --ref: also passes with ED | RESCUE and with ED | RESCUE | WLIST")
        deliver(ap.parse_args())
    else:
        main()
