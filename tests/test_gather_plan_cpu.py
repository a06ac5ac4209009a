"""The gathered read store in the rank memory plan (hifiasm_amd/memplan.py: gathered_reads=True): off by default - the plan every other test holds does not
move - and, switched on, BASELINE.json's configs[3] / configs[4] on 8 GPUs still fit the 288 GB of an MI355X in the all-reads pass and while the gather runs
(the store: a quarter byte per base and 9 bytes per read of ALL reads - 30 GB and 22.5 GB of packed bases); the plan's chunk is the engine's."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gathered_reads_term():
    from hifiasm_amd import memplan
    from hifiasm_amd.workloads import WORKLOADS, n_reads_of
    src = open(os.path.join(ROOT, "hifiasm_amd", "csrc", "hao_ctx.hpp")).read()
    assert "gather_chunk = 64ULL << 20" in src and memplan.GATHER_CHUNK == 64 << 20
    for fixture, target in (("chr1_250M_hifi30x", "human3G_hifi40x"), ("ont50M_30x", "ont_human_30x")):
        g = np.load(os.path.join(ROOT, "tests", "golden", fixture + ".npz"))
        h = g["pt_hist"].astype(np.int64)
        gs, cov = WORKLOADS[fixture][:2]
        density = float((h * np.arange(h.size)).sum()) / float(gs * cov)
        tg, tcov, trl, terr = WORKLOADS[target][:4]
        args = (float(tg) * tcov, n_reads_of(target), 8, density, 0.92 * density * trl * tcov, float(tg))
        base = memplan.rank_plan(*args, err=terr, bloom=terr > 0.005)
        assert base == memplan.rank_plan(*args, err=terr, bloom=terr > 0.005, gathered_reads=False) and "gathered_reads" not in base
        pl = memplan.rank_plan(*args, err=terr, bloom=terr > 0.005, gathered_reads=True)
        store = 0.25 * tg * tcov + 9 * n_reads_of(target)
        assert pl["gathered_reads"] == store and 20e9 < store < 35e9
        assert pl["all_reads_pass"] == base["all_reads_pass"] + store and pl["gather"] > store
        assert all(pl[k] == base[k] for k in ("reads", "ft_gen", "pt_gen", "index", "passes_ft"))
        for phase in ("gather", "all_reads_pass", "peak"):
            assert pl[phase] < 0.9 * memplan.HBM_BYTES, (target, phase, pl[phase] / 1e9)
        print(f"[gathered reads] {target}: store {store / 1e9:.1f} GB, gather {pl['gather'] / 1e9:.1f} GB, all-reads pass {pl['all_reads_pass'] / 1e9:.1f} GB")
    one = memplan.rank_plan(250e6 * 30, 500_000, 1, 0.02873, 11_900, 250e6)
    assert one == memplan.rank_plan(250e6 * 30, 500_000, 1, 0.02873, 11_900, 250e6, gathered_reads=True)      # an unsharded engine gathers nothing
