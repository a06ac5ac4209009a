"""f3 with traceback in the streaming pass (HAO_DELIVER_TRACE): passes of hao_overlap_batch_async batches (both slots in flight) with OL|CL|ED and with
OL|CL|ED|TRACE, alternately.  Per batch: the traced stage's device time (stage_times "trace_sel": flags + selection, "trace_align": traced sweep, walk and
compaction), traced pairs/s, the column scratch a traced pair needs (three words per band word and text column, + one slot; the host-fed path's form keeps
five) and the bytes the part adds to the arena; per pass the wall time of the delivered step.  Prints one JSON line.
usage: python tools/bench_trace_grid.py [--workload W] [--batch-reads N] [--max-batches K] [--thre T] [--reps R]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(a):
    from hifiasm_amd import workloads
    from hifiasm_amd.api import Engine, DELIVER_OL, DELIVER_CL, DELIVER_ED, DELIVER_TRACE
    hi_all = workloads.n_reads_of(a.workload)
    rs = workloads.workload_reads(a.workload)
    e = Engine(0); e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
    wl = 375
    e.deliver_ed_config(wl, a.thre)
    br = a.batch_reads or (rs.n + 1) // 2
    ranges = [(lo, min(hi_all, lo + br)) for lo in range(0, rs.n, br)][:a.max_batches]
    base, full = DELIVER_OL | DELIVER_CL | DELIVER_ED, DELIVER_OL | DELIVER_CL | DELIVER_ED | DELIVER_TRACE

    def one_pass(parts):
        per, pending, t0 = [], None, time.time()

        def take(slot, k):
            d = e.deliver_wait(slot)
            per[k].update(bytes=int(d.bytes), pairs=int(d.ed.n_pairs), traced=int(d.tr.n_traced) if d.tr is not None else 0,
                          cigar=int(d.tr.n_cigar) if d.tr is not None else 0)
        for k, (lo, hi) in enumerate(ranges):
            slot = e.overlap_batch_async(lo, hi, parts=parts)
            st = {}
            for nm, ms in e.stage_times():
                st[nm] = st.get(nm, 0.0) + ms
            per.append(dict(reads=hi - lo, ed_ms=st.get("ed_grid", 0.0) + st.get("ed_align", 0.0), trace_sel_ms=st.get("trace_sel", 0.0),
                            trace_align_ms=st.get("trace_align", 0.0), kernels_ms=sum(st.values())))
            if pending is not None:
                take(*pending)
            pending = (slot, k)
        take(*pending)
        return (time.time() - t0) * 1e3, per

    one_pass(full); one_pass(base)      # warm-up (allocations, arenas)
    walls = {"ol_cl_ed": [], "ol_cl_ed_trace": []}; last = {}
    for _ in range(a.reps):
        for key, parts in (("ol_cl_ed", base), ("ol_cl_ed_trace", full)):
            w, per = one_pass(parts); walls[key].append(round(w, 2)); last[key] = per
    nword = (2 * a.thre + 1 + 63) // 64
    batches = []
    for b0, b1 in zip(last["ol_cl_ed"], last["ol_cl_ed_trace"]):
        tr_ms = b1["trace_sel_ms"] + b1["trace_align_ms"]
        batches.append(dict(reads=b1["reads"], pairs=b1["pairs"], traced=b1["traced"], cigar_entries=b1["cigar"], ed_ms=round(b1["ed_ms"], 3),
                            trace_sel_ms=round(b1["trace_sel_ms"], 3), trace_align_ms=round(b1["trace_align_ms"], 3), trace_ms=round(tr_ms, 3),
                            traced_pairs_per_s=round(b1["traced"] / max(1e-9, tr_ms * 1e-3)),
                            column_scratch_bytes_per_traced_pair=24 * nword * (wl + 1), column_scratch_bytes_per_traced_pair_five_words=40 * nword * wl,
                            column_scratch_bytes_written=24 * nword * (wl + 1) * b1["traced"],
                            arena_bytes_ol_cl_ed=b0["bytes"], arena_bytes_ol_cl_ed_trace=b1["bytes"], extra_bytes=b1["bytes"] - b0["bytes"],
                            kernels_ms_ol_cl_ed=round(b0["kernels_ms"], 3), kernels_ms_ol_cl_ed_trace=round(b1["kernels_ms"], 3)))
    print(json.dumps({"workload": a.workload, "reads_indexed": int(rs.n), "window": wl, "thre": a.thre, "batches": batches,
                      "delivered_step_ms_ol_cl_ed": walls["ol_cl_ed"], "delivered_step_ms_ol_cl_ed_trace": walls["ol_cl_ed_trace"],
                      "delivered_step_ms_best": {k: min(v) for k, v in walls.items()},
                      "what": "passes over the listed batches with both slots in flight: host wall time per pass with OL|CL|ED and with OL|CL|ED|TRACE (alternating), "
                              "the traced stage's device time per batch (stage_times), its column scratch, the bytes it adds to the arena"}))
    e.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bacterial5M_hifi30x")
    ap.add_argument("--batch-reads", type=int, default=0, help="reads per batch (0: two batches over the read set)")
    ap.add_argument("--max-batches", type=int, default=1 << 30)
    ap.add_argument("--thre", type=int, default=15)
    ap.add_argument("--reps", type=int, default=2)
    main(ap.parse_args())
