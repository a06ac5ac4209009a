"""The entry points of cal_estimate_err over the resident window lists (include/hao.h: hao_window_estimate_err, hao_fetch_ladder_adv_estimates,
hao_estimate_err_records): exported, declared in hifiasm_amd/api.py, reachable from Engine; the header no longer lists the function as not built, and the
ladder's result record keeps its 60 bytes."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_exported():
    from hifiasm_amd import api
    L = C.CDLL(api.lib_path())
    names = {"hao_window_estimate_err", "hao_fetch_ladder_adv_estimates", "hao_estimate_err_records"}
    assert all(hasattr(L, n) for n in names) and names <= set(api.ABI_SYMBOLS)
    assert hasattr(api.Engine, "window_estimate_err") and hasattr(api.Engine, "ladder_adv_estimates") and hasattr(api, "estimate_err_records")
    assert api.LADDER_ADV_RES.itemsize == 60


def test_header_says_what_is_built():
    src = open(os.path.join(ROOT, "include", "hao.h")).read()
    for name in ("hao_window_estimate_err", "hao_fetch_ladder_adv_estimates", "hao_estimate_err_records"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for m in re.finditer(r"Not built:[^\n]*(?:\n \*[^\n]*)*", src):
        assert "cal_estimate_err" not in m.group(0).split("*/")[0], m.group(0)[:200]
    assert "gen_extend_err_exz" in src and "adjust_specific_ext_offset" in src
