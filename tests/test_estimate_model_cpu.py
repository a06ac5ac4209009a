"""cal_estimate_err without a GPU: tests/estimate_model.py (the reference's lines restated) and api.estimate_err_records (hao_estimate_err_records: the device
function hao_ld_estimate_wlist compiled for the host) against tests/golden/estimate_err.npz - the reference's own function on real window lists and on crafted
records (tests/golden/make_golden_estimate.py) - on every case, value for value."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
import estimate_model as EM


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "estimate_err.npz"))
    return {k: z[k] for k in z.files}


def _cases(g):
    """(overlap row, window rows, wl, qs, qe, e_rate, the reference's value, category) of every case, real then crafted"""
    wl, e_rate = int(g["cfg"][0]), float(g["cfg"][1])
    for (s, qs, qe, _, _), v, c in zip(g["real_q"], g["real_val"], g["real_cat"]):
        yield g["ovlp"][s], g["wins"][int(g["win_off"][s]):int(g["win_off"][s + 1])], wl, int(qs), int(qe), e_rate, int(v), str(g["cats"][c])
    for (s, qs, qe), er, v, c in zip(g["c_q"], g["c_erate"], g["c_val"], g["c_cat"]):
        yield g["c_ovlp"][s], g["c_wins"][int(g["c_win_off"][s]):int(g["c_win_off"][s + 1])], wl, int(qs), int(qe), float(er), int(v), str(g["cats"][c])


def test_fixture_holds_every_category(gold):
    seen = {str(gold["cats"][c]) for c in gold["real_cat"]} | {str(gold["cats"][c]) for c in gold["c_cat"]}
    if (gold["real_val"] < 0).any():
        seen.add("negative_value")
    assert seen == {str(c) for c in gold["cats"]}
    assert {0.07, 0.001, 0.5, 0.0, 1.0} <= set(gold["c_erate"].tolist())
    q = gold["real_q"]
    assert (q[:, 2] - q[:, 1] > int(gold["cfg"][0])).sum() > 100


def test_model_equals_the_reference(gold):
    n = 0
    for z, W, wl, qs, qe, er, want, cat in _cases(gold):
        assert EM.estimate_err(z, W, wl, qs, qe, er) == want, (cat, z[1:3], qs, qe, er)
        n += 1
    assert n == gold["real_val"].size + gold["c_val"].size > 1000


def test_host_twin_equals_the_reference(gold):
    from hifiasm_amd import api
    n = 0
    for z, W, wl, qs, qe, er, want, cat in _cases(gold):
        assert api.estimate_err_records(z, W, wl, qs, qe, er) == want, (cat, z[1:3], qs, qe, er)
        n += 1
    assert n > 1000
