"""The read-back slots (hao_peek_id, hao_ctx.hpp) carry a few words from the device to the host for the batch pass, the index sort and the window stages of one
engine.  No caller's read-back may depend on what another caller left in the mapped words: a batch gives the same totals, seed path and chain census after the
index sort's self-test and a blocking window stage have run on the engine, and the self-test reports on a used engine what it reports on a fresh one."""
import ctypes as C

import pytest

from scenarios import SCENARIOS, build_reads

pytestmark = pytest.mark.gpu

SORT_N = 16      # the smallest n hao_selftest_sortbits accepts


def _engine(rs):
    from hifiasm_amd.api import Engine
    e = Engine(0)
    e.set_readset(rs)
    e.ha_ft_gen(); e.ha_pt_gen()
    return e


def _sortbits(e):
    from hifiasm_amd.api import lib
    L = lib()
    L.hao_selftest_sortbits.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    assert L.hao_selftest_sortbits(e.h, SORT_N, out) == 0
    assert out[0] == 0      # (the 40-bit sort and its fix-up agree with the 64-bit sort)
    return [int(x) for x in out[1:4]]


def _batch(e, n):
    e.overlap_batch(0, n)
    return e.batch_totals(), e.batch_seed_path(), e.batch_chain_path()


def test_no_read_back_depends_on_another_callers_slots():
    rs = build_reads(SCENARIOS["hifi"][0])
    e = _engine(rs)
    try:
        first = _batch(e, rs.n)
        cnt, slow = first[2]
        print(f"[batch slots] totals {first[0]}, seed path {first[1]}, groups per class {cnt}, left to the DP {slow}")
        assert first[0]["overlaps"] > 0 and sum(1 for x in cnt if x) > 1      # groups in more than one size class
        sort_used = _sortbits(e)
        e.window_ed_ref(775, 0.04)
        e.window_rescue_ref()
        assert _batch(e, rs.n) == first
    finally:
        e.close()
    from hifiasm_amd.api import Engine
    fresh = Engine(0)      # (no reads, no batch: nothing has written a slot)
    try:
        sort_fresh = _sortbits(fresh)
    finally:
        fresh.close()
    print(f"[batch slots] sort self-test at n = {SORT_N}: runs, scratch, overflow {sort_used} on the used engine, {sort_fresh} on a fresh one")
    assert sort_used == sort_fresh
