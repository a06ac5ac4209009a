"""The selection's three replays of klib's introsort (hao_chain.cuh: hao_intro_sort, hao_wave_intro_sort, hao_block_intro_sort) run alone on the key arrays of
tests/golden/sortperm.npz (hao_dbg_sort_perm), path by path; every permutation has to be the one the reference's own ks_introsort_or_ss / ks_introsort_or_xs gave
(the order of equal keys is observable in ol->list).  tests/test_sortperm_cpu.py checks that the arrays reach what they are for: levels of the quicksort with more
than 64 live sub-ranges, the combsort fallback, a closing insertion sort that moves an element far, ties below 65 keys, keys at the ends of their ranges."""
import numpy as np
import pytest

from helpers import load_sortperm

pytestmark = pytest.mark.gpu

# (path, variant, most keys the path holds): include/hao.h
PATHS = {"seq": (0, 0, 1 << 20), "wave_lds128": (1, 0, 128), "wave_lds1024": (1, 1, 1024), "wave_global": (2, 0, 1 << 20), "block": (3, 0, 4096), "select": (4, 0, 1 << 20)}
# the emulated default run (tests/test_simt_sortperm_cpu.py): arrays that keep every kind of tests/test_sortperm_cpu.py::test_fixture_holds_every_kind
SMALL = lambda nm, n: n <= 129 or nm.split("_")[1] in ("equal", "v3", "asc1", "organ", "family") or nm in ("m0_v8_4096", "m1_v8_4096", "m1_saw_4095", "m0_asc_1025", "m1_desc_1025", "m0_rand_4097", "m1_rand_4097")


def _cases(path, mode, pick=None):
    return [c for c in load_sortperm() if c[1] == mode and len(c[2]) <= PATHS[path][2] and (pick is None or pick(c[0], len(c[2])))]


@pytest.fixture(scope="module")
def eng():
    from hifiasm_amd.api import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", list(PATHS))
def test_sort_matches_reference(eng, path, mode, pick=None):
    if path == "select" and mode == 0:
        return      # (the selection sorts by score only in front of its pruning; hao_dbg_sort_perm refuses the combination: test_refusals)
    cs = _cases(path, mode, pick)
    assert len(cs) >= 20
    got = eng.dbg_sort_perm(mode, PATHS[path][0], [(c[2], c[3]) for c in cs], variant=PATHS[path][1])
    bad = [c[0] for c, g in zip(cs, got) if not np.array_equal(g, c[4])]
    print(f"[sortperm] {path} mode {mode}: {len(cs)} arrays, {sum(len(c[2]) for c in cs)} keys, {len(bad)} differ")
    assert not bad, f"{len(bad)} of {len(cs)} arrays differ from the reference's order: {bad[:8]}"


def test_refusals(eng):
    from hifiasm_amd.api import HaoError
    a = [(np.arange(5, dtype=np.uint64), np.zeros(5, np.int32)), (np.arange(200, dtype=np.uint64), np.zeros(200, np.int32))]
    with pytest.raises(HaoError):
        eng.dbg_sort_perm(1, 0, a, off=[0, 7, 5])            # offsets that do not ascend
    with pytest.raises(HaoError):
        eng.dbg_sort_perm(1, 1, a, variant=0)               # 200 keys in the slice of 128
    with pytest.raises(HaoError):
        eng.dbg_sort_perm(1, 3, [(np.arange(4097, dtype=np.uint64), np.zeros(4097, np.int32))])
    with pytest.raises(HaoError):
        eng.dbg_sort_perm(0, 4, a)                          # the selection without pruning sorts by position only
    with pytest.raises(HaoError):
        eng.dbg_sort_perm(2, 0, a)
    assert [list(p) for p in eng.dbg_sort_perm(1, 0, a[:1])] == [[0, 1, 2, 3, 4]]
