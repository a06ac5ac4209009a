"""Size and field offsets of hc_aln_exz_adv's result record (include/hao.h: hao_ladder_adv_res_t) as hifiasm_amd/api.py mirrors it, the new constants, and the entry
points' export.  (hao_ladder_adv_thresholds against tests/ladder_adv_model.py: tests/test_ladder_adv_model_cpu.py.)"""
import ctypes as C
import os
import re

import numpy as np

from test_abi_ladder_cpu import _fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_layout():
    from hifiasm_amd import api
    f = _fields("hao_ladder_adv_res_t")
    dt = api.LADDER_ADV_RES
    assert dt.itemsize == 60 == 4 * len(f)
    assert [n for n, _ in f] == list(dt.names)
    for k, (n, ty) in enumerate(f):
        assert dt.fields[n][1] == 4 * k and dt.fields[n][0] == np.dtype({"uint32_t": np.uint32, "int32_t": np.int32}[ty]), n
    # the record is hao_ladder_res_t behind `done`
    assert list(dt.names[1:]) == list(api.LADDER_RES.names)
    src = open(os.path.join(ROOT, "include", "hao.h")).read()
    for name, v in (("HAO_LADDER_REPEAT", api.LADDER_REPEAT), ("HAO_LADDER_RUNG_EXACT", api.LADDER_RUNG_EXACT)):
        assert int(re.search(r"#define " + name + r" (\d+)u", src).group(1)) == v
    assert api.LADDER_REPEAT & (api.LADDER_REFUSED | api.LADDER_UNTRACED) == 0


def test_entry_points_exported():
    from hifiasm_amd import api
    L = C.CDLL(api.lib_path())
    names = {"hao_window_ladder_adv", "hao_fetch_ladder_adv", "hao_ladder_adv_thresholds"}
    assert all(hasattr(L, n) for n in names) and names <= set(api.ABI_SYMBOLS)
    assert hasattr(api.Engine, "window_ladder_adv") and hasattr(api.Engine, "ladder_adv_rounds")
