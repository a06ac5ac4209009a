"""The selection's sort, pinned to the reference's own (klib introsort, tie order observable): tests/golden/sortperm.npz holds key arrays and the permutations
ks_introsort_or_ss / ks_introsort_or_xs gave them (tests/golden/make_golden_sortperm.py).  The plain model (tests/sortperm_model.py) and the oracle's sort have to
give the same permutations, and the model says which path of the device sorts each array exercises: the fixture has to hold every kind, or the GPU test
(tests/test_gpu_sortperm.py) would pass without having been anywhere near the code it is for."""
import numpy as np
import pytest

import oracle_py
import sortperm_model
from helpers import SORTPERM_SIZES, load_sortperm, sortperm_cases


@pytest.fixture(scope="module")
def modelled():
    return [(nm, mode, len(xs), perm) + sortperm_model.intro_sort(sortperm_model.sort_keys(mode, xs, sc)) for nm, mode, xs, sc, perm in load_sortperm()]


def test_model_matches_reference(modelled):
    bad = [nm for nm, mode, n, perm, mp, info in modelled if list(perm) != mp]
    assert not bad, bad[:8]


def test_oracle_matches_reference():
    bad = [nm for nm, mode, xs, sc, perm in load_sortperm() if not np.array_equal(oracle_py.sort_perm(mode, xs, sc), perm)]
    assert not bad, bad[:8]


def test_fixture_keys_are_the_generators():
    """(the stored keys are what the GPU test sorts; a generator that drifted would only show when the fixture is rebuilt)"""
    cs, fx = sortperm_cases(), load_sortperm()
    assert [c[0] for c in cs] == [f[0] for f in fx]
    for (nm, mode, xs, sc), (_, fmode, fxs, fsc, _) in zip(cs, fx):
        assert mode == fmode and np.array_equal(xs, fxs) and np.array_equal(sc, fsc), nm


def test_fixture_holds_every_kind(modelled):
    for mode in (0, 1):
        cs = [(nm, n, info) for nm, m, n, perm, mp, info in modelled if m == mode]
        wide = [n for nm, n, info in cs if info["widest"] > 64]      # more live sub-ranges in one level than the segment lists of hao_block_intro_sort once held
        assert len(wide) >= 6 and sum(2049 <= n <= 4096 for n in wide) >= 2, (mode, wide)
        # (at or below 2048 keys a scan of all-equal, 2-, 3-, 4-, 5-, 8- and 16-valued random arrays and of block / interleaved layouts found no level wider than 64)
        assert sum(info["comb"] > 0 for nm, n, info in cs) >= 4, mode
        assert sum(info["far"] for nm, n, info in cs) >= 4, mode
        for size in SORTPERM_SIZES:
            assert sum(n == size for nm, n, info in cs) >= 2, (mode, size)
    small = [(mode, xs, sc) for nm, mode, xs, sc, perm in load_sortperm() if len(xs) <= 64]
    tied = [len(set(sortperm_model.sort_keys(mode, xs, sc))) < len(xs) for mode, xs, sc in small]
    assert sum(tied) >= 4 and len(tied) - sum(tied) >= 4
