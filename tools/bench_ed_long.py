# Throughput of the cooperative window-alignment kernel (hao_align_coop.cuh, hao_window_ed_long) in band-word x columns per second at nword 8 (thre 255) and
# nword 64 (thre 2047), next to the register-resident formulation at its widest (hao_al_kernel<hao_wide<4>, distance-only> at thre 127, hao_window_ed_batch)
# on the SAME strings: text windows of 1000 .. 2000 bases of the ont scenario's overlaps against the target interval on the overlap's diagonal, padded by thre on
# both sides (the pairs align within 127 errors, so no sweep is abandoned early and every configuration walks every column).  A few thousand replicated pairs;
# the time is the host's clock around the blocking call (task upload, host-side order, kernels, result download: the calls end in a stream synchronise) - with
# thousands of columns per pair the kernels are all but all of it; `rocprofv3 --kernel-trace --stats -- python tools/bench_ed_long.py` gives the kernels alone.
# usage: bench_ed_long.py [--pairs N] [--dry]      (--dry: build the tasks only - runs without a GPU)
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from helpers import scenario_reads, scenario_oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4096); ap.add_argument("--dry", action="store_true")
a_ = ap.parse_args()
name = "ont"
rs, okw = scenario_reads(name)
o = scenario_oracle(name)
L = rs.lengths.astype(np.int64)


def tasks(thre, n_distinct=256, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for r in rng.permutation(rs.n):
        for z in o.lchain(int(r))[0]:
            xs, xe, yid, ys, yrev = int(z[1]), int(z[2]), int(z[4]), int(z[5]), int(z[7])
            tn = min(int(rng.integers(1000, 2001)), xe + 1 - xs)
            if tn < 1000:
                continue
            ws = xs + int(rng.integers(0, xe + 2 - xs - tn))
            p0 = ys + (ws - xs) - thre; p1 = min(p0 + tn + 2 * thre, int(L[yid])); ad = 0
            if p0 < 0:
                ad, p0 = -p0, 0
            if ad > 2 * thre or p1 - p0 - tn + ad < 0 or tn <= ad:
                continue
            out.append((yid, p0, p1 - p0, yrev, int(r), ws, tn, 0, thre, ad))
            if len(out) == n_distinct:
                t = np.array(out, dtype=np.uint32)
                return np.concatenate([t] * max(1, a_.pairs // n_distinct))
    raise SystemExit("not enough overlaps")


e = None
if not a_.dry:
    from hifiasm_amd.api import Engine
    e = Engine(0, **okw); e.set_readset(rs)
rate = {}
for label, thre, call in (("hao_al_kernel<hao_wide<4>>, thre 127 (nword 4)", 127, "window_ed_batch"), ("cooperative, thre 255 (nword 8)", 255, "window_ed_long"), ("cooperative, thre 2047 (nword 64)", 2047, "window_ed_long")):
    t = tasks(thre)
    nword = (2 * thre + 64) // 64
    work = float(nword * t[:, 6].astype(np.int64).sum())
    msg = f"{label:48s} {t.shape[0]} pairs, {int(t[:, 6].sum()) / 1e6:.1f} M columns, {work / 1e6:.0f} M word-columns"
    if e is not None:
        res = getattr(e, call)(t)      # (first call: scratch allocation, code objects)
        assert (res[:, 0] <= 127).all(), "a pair did not align: its sweep may have stopped early"
        ts = []
        for _ in range(5):
            t0 = time.time(); getattr(e, call)(t); ts.append(time.time() - t0)
        rate[thre] = work / min(ts)
        msg += f": best of 5 {min(ts) * 1e3:.1f} ms (worst {max(ts) * 1e3:.1f}) = {rate[thre] / 1e9:.2f} G word-columns/s"
    print(msg, flush=True)
if e is not None:
    print(f"ratio to the register-resident kernel: nword 8 {rate[255] / rate[127]:.3f}, nword 64 {rate[2047] / rate[127]:.3f}")
    e.close()
