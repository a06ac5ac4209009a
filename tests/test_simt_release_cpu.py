"""Every device buffer an engine reserves is freed by hao_destroy.  TEST INFRASTRUCTURE: runs on tests/simt/_build/libhao_simt.so, whose stand-in for
hipMalloc / hipFree counts the allocations that have not been freed (hao_simt_live_allocations, tests/simt/hip/hip_runtime.h) - and checks the guard zones
round a buffer when it is freed, so a buffer that leaks is also a buffer whose out-of-bounds writes nobody sees.  One engine on the small HiFi set goes
through the stages that own device memory: the tables (the sketch's scratch), a blocking batch with the reference-placed window alignment, its rescue and the
traced grid stage, two streamed batches with every part reference placement delivers (both output sets), and a batch on an attached view."""
import ctypes as C

import pytest

import simt_build
from helpers import scenario_reads


@pytest.fixture(scope="module", autouse=True)
def _simt_library():
    from hifiasm_amd import api
    old_path, old_lib = api.lib_path, api._LIB
    path = simt_build.build_lib()
    api.lib_path = lambda: path; api._LIB = None
    yield
    api.lib_path, api._LIB = old_path, old_lib


def test_destroy_frees_every_device_buffer():
    from hifiasm_amd import api
    from hifiasm_amd.api import Engine, DELIVER_OL, DELIVER_CL, DELIVER_EXACT, DELIVER_ED, DELIVER_RESCUE
    live = api.lib().hao_simt_live_allocations
    live.restype = C.c_long; live.argtypes = []
    rs, okw = scenario_reads("hifi")
    before = live()
    e = Engine(0, **okw)
    e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()                      # (the sketch path reserves its per-unit scratch)
    assert live() > before
    e.overlap_batch(0, rs.n)                                             # blocking: reference placement, rescue, traced grid
    n, _ = e.window_ed_ref(775, 0.04)
    assert n > 0
    e.window_rescue_ref()
    assert e.window_trace_grid(375, 15)[0] > 0
    e.deliver_ed_config_ref(775, 0.04)                                   # streamed: two batches, so both output sets are used
    parts = DELIVER_OL | DELIVER_CL | DELIVER_EXACT | DELIVER_ED | DELIVER_RESCUE
    half = rs.n // 2
    s0 = e.overlap_batch_async(0, half, parts=parts)
    s1 = e.overlap_batch_async(half, rs.n, parts=parts)
    assert {s0, s1} == {0, 1}
    d0 = e.deliver_wait(s0); d1 = e.deliver_wait(s1)
    assert d0.rs is not None and d1.rs is not None and d0.n_ol + d1.n_ol > 100
    v = e.attach()                                                       # a view borrows the owner's reads and index and owns the rest
    v.overlap_batch(0, half)
    held = live()
    v.close()
    assert live() < held
    e.close()
    assert live() == before, f"{live() - before} device allocations outlive hao_destroy"
