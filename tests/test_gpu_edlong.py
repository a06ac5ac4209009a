"""Window alignment beyond 127 errors on the device (hao_window_ed_long / hao_window_trace_long, hao_align_coop.cuh: a segment of 8 .. 64 lanes per pair, one band word
per lane) against the REFERENCE's own ed_band_cal_*_infi_* functions with nword = 5 .. 64 (tests/golden/ed_long.npz, tests/golden/make_golden_ed_long.py: results
and cigars of tests/edlong_tasks.py's pairs, most of which align with 128 errors or more), in mixed calls with the narrower bands, and - every pair forced through
the cooperative kernel (HAO_DBG_FORCE=al_coop) - against the fixtures of the one- to four-word bands (tests/golden/ed.npz, ed_wide.npz).
(The scenarios' longest reads have 7956 and 4991 bases, so the two upper-end pairs per list have texts of ~7000 / ~4000 columns at thre 2047, not 10 000.)"""
import os

import numpy as np
import pytest

from helpers import ed_tasks, ed_global_tasks, ed_semi_trace_tasks, ed_ext_tasks, scenario_reads, scenario_oracle, GOLDEN
from edlong_tasks import edl_tasks, nword_of, NWORD_EDGES, N_BIG

pytestmark = pytest.mark.gpu
NOALN = 2**31 - 1
CAP = 2 * 2047 + 3 + 2      # an alignment within thre has at most 2 thre + 3 entries, + the 0x3fff splits of strings this short: none
TRACED = [(0, "g", "g"), (1, "x", "x1"), (2, "x", "x2"), (3, "s", "s")]      # mode, task list, result key
BIG = [True]      # (the emulated workgroup, tests/test_simt_edlong_cpu.py, leaves the two upper-end pairs out unless HAO_SIMT_FULL is set)


def _fixture(which):
    z = np.load(os.path.join(GOLDEN, which + ".npz"))
    return {k: z[k] for k in z.files}


def _rows(n, big):
    return n if big else n - N_BIG


def _same_cigars(gcig, want, wc, rows):
    off = np.concatenate([[0], np.cumsum(want[:, 5])]).astype(np.int64)
    return [q for q in range(rows) if not (gcig[q, :want[q, 5]] == wc[off[q]:off[q + 1]]).all()]


def _engine(name, env=None):
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads(name)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        e = Engine(0, **okw)      # (the switches are read once, when the engine is created)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    e.set_readset(rs)
    return e


@pytest.mark.parametrize("big", BIG)
@pytest.mark.parametrize("name", ["ont", "nn"])
def test_long_bands_against_the_reference(name, big):
    """(a) distance-only results and all four traced modes, cigars included; the semi-global list once more with a column budget of 1 MB per slice, so that the
    second sweep runs in many slices (the upper-end pairs then get a slice each)"""
    g = _fixture("ed_long")
    e = _engine(name)
    t = edl_tasks(name, "", big=True)
    assert t.shape == g[name + "_tasks"].shape and (t == g[name + "_tasks"]).all(), "the task generator drifted: regenerate the fixture"
    n = _rows(t.shape[0], big)
    want = g[name + "_res"]
    got = e.window_ed_long(t[:n])
    assert (got == want[:n]).all(), (np.flatnonzero((got != want[:n]).any(axis=1))[:10], got[(got != want[:n]).any(axis=1)][:3], want[:n][(got != want[:n]).any(axis=1)][:3])
    far = (want[:n, 0] != NOALN) & (want[:n, 0] >= 128)
    assert far.sum() >= 0.3 * n and set(NWORD_EDGES) <= set(nword_of(t[:n][far, 8]))
    for mode, tk, rk in TRACED:
        t = edl_tasks(name, tk, big=True)
        assert t.shape == g[f"{name}_{tk}tasks"].shape and (t == g[f"{name}_{tk}tasks"]).all(), "the task generator drifted: regenerate the fixture"
        n = _rows(t.shape[0], big)
        want = g[f"{name}_{rk}res"]; wc = g[f"{name}_{rk}cig"]
        got, gcig = e.window_trace_long(t[:n], cap=CAP, mode=mode)
        bad = (got != want[:n]).any(axis=1)
        assert not bad.any(), (mode, np.flatnonzero(bad)[:10], got[bad][:3], want[:n][bad][:3])
        assert not _same_cigars(gcig, want, wc, n), (mode, _same_cigars(gcig, want, wc, n)[:10])
        if mode == 0:      # a capacity below the cigar length: the entries are counted, the result is otherwise the same
            g2, c2 = e.window_trace_long(t[:n], cap=4, mode=mode)
            assert (g2 == want[:n]).all()
    e.close()
    e = _engine(name, {"HAO_DBG_TEST": "al_slice=1000000"})
    t = edl_tasks(name, "s", big=True); n = _rows(t.shape[0], big)
    want = g[name + "_sres"]; wc = g[name + "_scig"]
    got, gcig = e.window_trace_long(t[:n], cap=CAP, mode=3)
    e.close()
    assert (got == want[:n]).all() and not _same_cigars(gcig, want, wc, n)


@pytest.mark.parametrize("name", ["ont"])
def test_mixed_widths_in_one_call(name):
    """(b) one- and two-word tasks (helpers.ed_tasks, against the oracle), the three- / four-word tasks of ed_wide.npz and the long ones, shuffled: element-wise"""
    gl, gw = _fixture("ed_long"), _fixture("ed_wide")
    o = scenario_oracle(name)
    e = _engine(name)
    t1 = ed_tasks(name, n_reads=6, seed=5, wide=False)[:150]; t2 = ed_tasks(name, n_reads=6, seed=5, wide=True)[:150]
    t3 = gw[name + "_tasks"][:200]; t4 = gl[name + "_tasks"][:-N_BIG]
    mix = np.concatenate([t1, t2, t3, t4]); wmix = np.concatenate([o.window_ed(t1), o.window_ed(t2), gw[name + "_res"][:200], gl[name + "_res"][:-N_BIG]])
    assert set(nword_of(mix[:, 8])) >= {1, 2, 3, 4, 5, 64}
    perm = np.random.default_rng(3).permutation(mix.shape[0])
    got = e.window_ed_long(mix[perm])
    assert (got == wmix[perm]).all(), np.flatnonzero((got != wmix[perm]).any(axis=1))[:10]
    # traced, semi-global: the same four sources
    s1 = ed_semi_trace_tasks(name, n_reads=6, seed=5, wide=False)[:100]; s2 = ed_semi_trace_tasks(name, n_reads=6, seed=5, wide=True)[:100]
    w1, c1 = o.window_trace(s1, cap=CAP, mode=3); w2, c2 = o.window_trace(s2, cap=CAP, mode=3)
    s3 = gw[name + "_stasks"][:150]; w3 = gw[name + "_sres"][:150]; s4 = gl[name + "_stasks"][:-N_BIG]; w4 = gl[name + "_sres"][:-N_BIG]
    def rows(want, flat):
        off = np.concatenate([[0], np.cumsum(want[:, 5])]).astype(np.int64); r = np.zeros((want.shape[0], CAP), dtype=np.uint16)
        for q in range(want.shape[0]):
            r[q, :want[q, 5]] = flat[off[q]:off[q + 1]]
        return r
    mix = np.concatenate([s1, s2, s3, s4]); wmix = np.concatenate([w1, w2, w3, w4]); cmix = np.concatenate([c1, c2, rows(w3, gw[name + "_scig"]), rows(w4, gl[name + "_scig"])])
    perm = np.random.default_rng(4).permutation(mix.shape[0])
    got, gcig = e.window_trace_long(mix[perm], cap=CAP, mode=3)
    e.close()
    assert (got == wmix[perm]).all(), np.flatnonzero((got != wmix[perm]).any(axis=1))[:10]
    bad = [q for q in range(got.shape[0]) if not (gcig[q, :got[q, 5]] == cmix[perm][q, :got[q, 5]]).all()]
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", ["hifi", "ont", "nn", "edge"])
def test_forced_cooperative_kernel_on_the_narrow_fixtures(name):
    """(c) HAO_DBG_FORCE=al_coop: the tasks of ed.npz (one and two words) and ed_wide.npz (three and four) through the new calls give those fixtures' results
    and cigars - the cooperative kernel under the ~30 000 reference tasks the project already has (segments of 8 lanes that carry one to four words)"""
    ge, gw = _fixture("ed"), _fixture("ed_wide")
    e = _engine(name, {"HAO_DBG_FORCE": "al_coop"})
    n_tasks = 0
    for g, pre in ((ge, name + "_"), (ge, name + "_w"), (gw, name + "_")):
        if pre + "tasks" not in g:      # (ed_wide.npz has no "edge" lists)
            continue
        t, want = g[pre + "tasks"], g[pre + "res"]
        got = e.window_ed_long(t)
        assert (got == want).all(), (pre, np.flatnonzero((got != want).any(axis=1))[:10])
        n_tasks += t.shape[0]
        for mode, tk, rk in TRACED:
            t, want, wc = g[pre + tk + "tasks"], g[pre + rk + "res"], g[pre + rk + "cig"]
            got, gcig = e.window_trace_long(t, cap=264, mode=mode)
            assert (got == want).all(), (pre, mode, np.flatnonzero((got != want).any(axis=1))[:10])
            assert not _same_cigars(gcig, want, wc, t.shape[0]), (pre, mode)
            n_tasks += t.shape[0]
    e.close()
    assert n_tasks > 5000


def test_refusals():
    """(d) thre 2048, a length of 16384, the semi-global domain rule and the distance-only band rule are refused; an empty call is not"""
    import ctypes as C
    from hifiasm_amd.api import HaoError
    e = _engine("ont")
    t = edl_tasks("ont", "s")[:1]
    assert e.window_ed_long(t).shape == (1, 2)
    for col, v in ((8, 2048), (2, 16384), (6, 16384)):
        bad = t.copy(); bad[0, col] = v
        with pytest.raises(HaoError):
            e.window_ed_long(bad)
        with pytest.raises(HaoError):
            e.window_trace_long(bad, cap=8, mode=0)
    bad = t.copy(); bad[0, 2] = bad[0, 6] - 1; bad[0, 9] = 0      # p_len - t_len + abs_diag < 0: the band does not cover the pattern
    with pytest.raises(HaoError):
        e.window_trace_long(bad, cap=8, mode=3)
    assert e.window_trace_long(bad, cap=8, mode=0)[0].shape == (1, 6)      # (the rule is the semi-global mode's)
    bad = t.copy(); bad[0, 8] = 130; bad[0, 5] = 0; bad[0, 6] = 10; bad[0, 1] = 0; bad[0, 2] = 10 + 64 * 5 + 1; bad[0, 9] = 0      # p_len - t_len + abs_diag = 64 nword + 1
    with pytest.raises(HaoError):
        e.window_ed_long(bad)
    assert e.window_ed_long(np.zeros((0, 10), dtype=np.uint32)).shape == (0, 2)
    assert e.L.hao_window_ed_long(e.h, None, 0, None) == 0 and e.L.hao_window_trace_long(e.h, 3, None, 0, None, None, 0) == 0
    e.close()
