"""Sizes and field offsets of the threshold ladder's records (include/hao.h: hao_ladder_req_t, hao_ladder_res_t) as hifiasm_amd/api.py mirrors them, and the
entry points' export.  (hao_ladder_thresholds against tests/ladder_model.py: tests/test_ladder_model_cpu.py.)"""
import ctypes as C
import re
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(name):
    src = open(os.path.join(ROOT, "include", "hao.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} " + name + ";", src)
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            out += [(n.strip(), ty) for n in names.split(",")]
    return out


def test_record_layouts():
    from hifiasm_amd import api
    for name, dt, size in (("hao_ladder_req_t", api.LADDER_REQ, 32), ("hao_ladder_res_t", api.LADDER_RES, 56)):
        f = _fields(name)
        assert dt.itemsize == size == 4 * len(f)
        assert [n for n, _ in f] == list(dt.names)
        for k, (n, ty) in enumerate(f):
            assert dt.fields[n][1] == 4 * k and dt.fields[n][0] == np.dtype({"uint32_t": np.uint32, "int32_t": np.int32}[ty]), n
    assert (api.LADDER_REFUSED, api.LADDER_UNTRACED) == (1, 2)


def test_entry_points_exported():
    from hifiasm_amd import api
    L = C.CDLL(api.lib_path())
    assert hasattr(L, "hao_window_ladder") and hasattr(L, "hao_fetch_ladder") and hasattr(L, "hao_ladder_thresholds")
    assert {"hao_window_ladder", "hao_fetch_ladder", "hao_ladder_thresholds"} <= set(api.ABI_SYMBOLS)
