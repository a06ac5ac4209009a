"""Golden vectors for window alignments beyond 127 errors (bands of 5 .. 64 words) from the REAL reference: oracle/_ref/ref_harness runs
ed_band_cal_semi_infi_w_absent_diag, ed_band_cal_global_infi_w_trace, ed_band_cal_extension_infi_{0,1}_w_trace and ed_band_cal_semi_infi_w_absent_diag_trace
(Levenshtein_distance.h:2516-3100) with nword = ceil((2 thre + 1) / 64), as cal_exz_infi does (Correct.cpp:14508-14565), on the tasks of tests/edlong_tasks.py.
Before anything is stored the mix is asserted on the reference's OWN results, per mode: at least 30 % of the tasks align with err >= 128 (beyond what the
register-resident kernels can hold), at least 10 % do not align, and every nword at a segment-size edge (5, 8, 9, 16, 17, 32, 33, 64) has an aligned task with
err >= 128.  Run in the build container only:  python tests/golden/make_golden_ed_long.py  -> tests/golden/ed_long.npz (tasks, results, cigars as u16)."""
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
from helpers import scenario_reads  # noqa: E402
from edlong_tasks import edl_tasks, nword_of, NWORD_EDGES  # noqa: E402

NOALN = 2**31 - 1


def check_mix(tag, t, res):
    err = res[:, 0].astype(np.int64)
    al = err != NOALN
    far = al & (err >= 128)
    print(f"  {tag}: {t.shape[0]} tasks, {int(al.sum())} aligned, {int(far.sum())} with err >= 128, text {int(t[:, 6].min())} .. {int(t[:, 6].max())}")
    assert far.sum() >= 0.30 * t.shape[0], (tag, "too few alignments beyond 127 errors")
    assert (~al).sum() >= 0.10 * t.shape[0], (tag, "too few pairs without an alignment")
    nw = nword_of(t[:, 8])
    for w in NWORD_EDGES:
        assert (far & (nw == w)).any(), (tag, "no aligned task with err >= 128 at nword", w)


out = {}
for name in ("ont", "nn"):
    rs, okw = scenario_reads(name)
    d = tempfile.mkdtemp(prefix="hao_edl_")
    ont = bool(okw.get("is_ont"))
    fa = os.path.join(d, "r.fq" if ont else "r.fa")
    synth.write_fasta(fa, rs, fastq=ont)
    sets = {k: edl_tasks(name, k, big=True) for k in ("", "g", "s", "x")}
    for k, t in sets.items():
        t.tofile(os.path.join(d, f"{k}tasks.u32"))
    cmd = [os.path.join(ROOT, "oracle", "_ref", "ref_harness"), "-t", "2", "--dump", os.path.join(d, "s"), "--reads-list", "/dev/null", "--no-tables",
           "--ed-tasks", os.path.join(d, "tasks.u32"), "--edg-tasks", os.path.join(d, "gtasks.u32"), "--eds-tasks", os.path.join(d, "stasks.u32"),
           "--ed1-tasks", os.path.join(d, "xtasks.u32"), "--ed2-tasks", os.path.join(d, "xtasks.u32")] + (["--ont"] if ont else []) + [fa]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    print(name)
    res = np.fromfile(os.path.join(d, "s.ed.i32"), dtype=np.int32).reshape(-1, 2)
    assert res.shape[0] == sets[""].shape[0]
    check_mix("ed", sets[""], res)
    out[name + "_tasks"] = sets[""]; out[name + "_res"] = res
    for tag, key, tk in (("edg", "g", "g"), ("eds", "s", "s"), ("ed1", "x1", "x"), ("ed2", "x2", "x")):
        tt = sets[tk]
        xr = np.fromfile(os.path.join(d, "s." + tag + ".i32"), dtype=np.int32).reshape(-1, 6)
        xc = np.fromfile(os.path.join(d, "s." + tag + "_cig.u16"), dtype=np.uint16)
        assert xr.shape[0] == tt.shape[0] and xc.size == int(xr[:, 5].sum())
        check_mix(tag, tt, xr)
        assert (xr[-2:, 0] != NOALN).all() and (xr[-2:, 5] > 0).all(), (tag, "the two upper-end pairs must be traced")
        out[name + "_" + tk + "tasks"] = tt
        out[name + "_" + key + "res"] = xr; out[name + "_" + key + "cig"] = xc
        print(f"      cigar entries {xc.size}, max per task {int(xr[:, 5].max())}")
np.savez_compressed(os.path.join(HERE, "ed_long.npz"), **out)
print(os.path.getsize(os.path.join(HERE, "ed_long.npz")), "bytes")
