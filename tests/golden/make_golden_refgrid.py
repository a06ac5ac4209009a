"""Golden vectors for the reference-placed window grid (hao_window_ed_ref, HAO_DELIVER_ED after hao_deliver_ed_config_ref) from the REAL reference: the tasks
tests/refgrid_model.py forms from the oracle's overlaps and fake cigars for a fixed sample of reads - hifi, nn, edge at (775, 0.04), ont at (375, 0.07), and hifi at (375, 0.07) for a pair init_waln refuses - go
through oracle/_ref/ref_harness --ed-tasks (the reference's own ed_band_cal_semi_64_w_absent_diag, Levenshtein_distance.h:3727) and, for the aligned ones
inside the traced domain, --eds-tasks (ed_band_cal_semi_64_w_absent_diag_trace + gen_trace).
Run in the build container only:  python tests/golden/make_golden_refgrid.py  -> tests/golden/refgrid.npz"""
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
import refgrid_model as M  # noqa: E402

# key -> (read set, window, e_rate).  The four cases of the grid's own configurations, and hifi at the ONT configuration: the only case found (every read of hifi,
# nn, edge, ont, rr, low, exact, bw001rr and hifi_15k was scanned at its own configuration: none) in which init_waln REFUSES a pair - read 114, a short last window
# whose shifted target interval ends more than 31 bases early
CONFIGS = {"hifi": ("hifi", 775, 0.04), "nn": ("nn", 775, 0.04), "edge": ("edge", 775, 0.04), "ont": ("ont", 375, 0.07), "hifi375": ("hifi", 375, 0.07)}
TARGET = 7000
NOALN = 2**31 - 1
CATS = ("shifted", "clipped_lower_thre", "aux_beg", "aux_end", "refused")


def categories(infos, wl, e_rate):
    full = M.threshold(wl, e_rate)
    c = dict.fromkeys(CATS, 0)
    for i, w, f in infos:
        if f["unresolved"]:
            continue
        c["refused"] += f["refused"]
        if f["refused"]:
            continue
        c["shifted"] += f["shift"] != 0
        c["clipped_lower_thre"] += f["q_l"] < wl and f["thre"] < full
        c["aux_beg"] += f["aux_beg"] > 0
        c["aux_end"] += f["aux_end"] > 0
    return c


out = {}
total = dict.fromkeys(CATS, 0)
for key, (name, wl, e_rate) in CONFIGS.items():
    rs, okw = scenario_reads(name)
    o = scenario_oracle(name)
    per = []
    for r in range(rs.n):
        ol, fc, fo, _ = o.lchain(r)
        T, infos = M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate, with_info=True)
        assert not any(f["unresolved"] for _, _, f in infos), (key, r)      # (y_start_offset resolves for every apend_be = 1 cigar)
        per.append((T, categories(infos, wl, e_rate)))
    # the sample: reads with a pair init_waln refuses first, then reads with a pair clipped at either end, twelve in all, then every stride-th read up to ~TARGET tasks
    pick = ([r for r in range(rs.n) if per[r][1]["refused"]] + [r for r in range(rs.n) if not per[r][1]["refused"] and (per[r][1]["aux_beg"] or per[r][1]["aux_end"])])[:12]
    have = sum(per[r][0].shape[0] for r in pick)
    stride = 3
    for r in list(range(0, rs.n, stride)) + list(range(1, rs.n, stride)) + list(range(2, rs.n, stride)):
        if have >= TARGET:
            break
        if r not in pick:
            pick.append(r); have += per[r][0].shape[0]
    pick = sorted(pick)
    t = np.concatenate([per[r][0] for r in pick]).reshape(-1, 10)
    cat = {k: sum(per[r][1][k] for r in pick) for k in CATS}
    for k in CATS:
        total[k] += cat[k]
    ti = t.astype(np.int64)
    ai = ti[:, 2] - ti[:, 6] + ti[:, 9]
    d = tempfile.mkdtemp(prefix="hao_refgrid_")
    ont = bool(okw.get("is_ont"))
    fa = os.path.join(d, "r.fq" if ont else "r.fa")
    synth.write_fasta(fa, rs, fastq=ont)
    t.tofile(os.path.join(d, "tasks.u32"))

    def run(extra):
        cmd = [os.path.join(ROOT, "oracle", "_ref", "ref_harness"), "-t", "2", "--dump", os.path.join(d, "s"), "--reads-list", "/dev/null", "--no-tables"] + extra + (["--ont"] if ont else []) + [fa]
        r_ = subprocess.run(cmd, capture_output=True, text=True)
        assert r_.returncode == 0, r_.stderr[-2000:]

    run(["--ed-tasks", os.path.join(d, "tasks.u32")])
    res = np.fromfile(os.path.join(d, "s.ed.i32"), dtype=np.int32).reshape(-1, 2)
    assert res.shape[0] == t.shape[0]
    sidx = np.flatnonzero((res[:, 0] != NOALN) & (ai >= 0) & (ai <= 2 * ti[:, 8]) & (ti[:, 6] > ti[:, 9])).astype(np.uint32)      # aligned and inside the traced domain
    t[sidx].tofile(os.path.join(d, "stasks.u32"))
    run(["--eds-tasks", os.path.join(d, "stasks.u32")])
    sres = np.fromfile(os.path.join(d, "s.eds.i32"), dtype=np.int32).reshape(-1, 6)
    scig = np.fromfile(os.path.join(d, "s.eds_cig.u16"), dtype=np.uint16)
    assert sres.shape[0] == sidx.size and scig.size == int(sres[:, 5].sum())
    out[key + "_cfg"] = np.array([wl, e_rate], dtype=np.float64)
    out[key + "_reads"] = np.array(pick, dtype=np.uint32)
    out[key + "_tasks"] = t; out[key + "_res"] = res
    out[key + "_sidx"] = sidx; out[key + "_sres"] = sres; out[key + "_scig"] = scig
    print(key, (name, wl, e_rate), len(pick), "reads,", t.shape[0], "tasks;", int((res[:, 0] != NOALN).sum()), "aligned;", sidx.size, "traced,", scig.size, "cigar entries;", cat)
print("all scenarios:", total)
for k in CATS:
    assert total[k] > 0, k
np.savez_compressed(os.path.join(HERE, "refgrid.npz"), **out)
