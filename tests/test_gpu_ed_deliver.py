"""f3 in the streaming pass (HAO_DELIVER_ED): every batch of hao_overlap_batch_async also carries the distance-only window alignment of all its grid pairs -
the pairs hao_window_ed_grid(window, thre) forms from the batch's final ol->list, in the same text order, with the same (err, pe).  With both slots in flight over
batches that do not start at read 0: for every read, the tasks hao_unpack_ed rebuilds from the delivered overlaps must equal helpers.ed_tasks_grid_all over
those overlaps, the results the oracle's ed_band_cal_semi_64_w_absent_diag (bands of three words: the upload path's result, itself pinned to the reference's
*_infi_* functions), and one batch must equal the blocking path (hao_window_ed_grid + hao_fetch_ed_grid) over the same range bit for bit.  Then the contract's
edges: ED without OL, without a config, a threshold beyond the widest band, two attached contexts with their own grids, and batches without ED unchanged."""
import numpy as np
import pytest

from helpers import ed_tasks_grid_all, scenario_reads, scenario_oracle

pytestmark = pytest.mark.gpu
NOALN = 2**31 - 1


def _engine(name):
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads(name)
    e = Engine(0, **okw)
    e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
    return e, rs


def _parts(which):
    from hifiasm_amd.api import DELIVER_OL, DELIVER_CL, DELIVER_EXACT, DELIVER_ED
    return DELIVER_OL | DELIVER_ED if which == "ol" else DELIVER_OL | DELIVER_CL | DELIVER_EXACT | DELIVER_ED


@pytest.mark.parametrize("name,window,thre,parts", [("hifi", 375, 15, "ol"), ("hifi", 375, 40, "all"), ("nn", 375, 15, "all"), ("rr", 375, 15, "ol"),
                                                    ("rr", 375, 40, "all"), ("hifi", 775, 70, "all"), ("nn", 775, 70, "ol"), ("edge", 100, 3, "all")])
def test_streamed_batches_carry_their_window_alignment(name, window, thre, parts):
    e, rs = _engine(name)
    o = scenario_oracle(name)
    try:
        e.deliver_ed_config(window, thre)
        lo0 = 3
        cuts = [lo0, lo0 + (rs.n - lo0) // 3, lo0 + 2 * (rs.n - lo0) // 3, rs.n]      # three batches, the first not at read 0
        got = {}       # batch -> (tasks, results) concatenated in read order
        pending = None

        def consume(slot, lo, hi):
            d = e.deliver_wait(slot)
            assert (d.rid_lo, d.n_reads) == (lo, hi - lo) and d.ed is not None
            assert (d.ed.window, d.ed.thre) == (window, thre)
            ts, rs_ = [], []
            for r in range(lo, hi):
                t, res = e.delivered_ed(d, r)
                ol = e.delivered_read(d, r)[0] if parts == "all" else _ol_only(e, d, r)
                want = ed_tasks_grid_all(rs.lengths, [ol], r, window, thre)
                assert t.shape == want.shape and (t == want).all(), r
                ts.append(t); rs_.append(res)
            if parts == "all":
                assert d.exact and d.n_cl > 0       # (the other parts still travel beside it)
            T = np.concatenate(ts) if ts else np.zeros((0, 10), np.uint32)
            assert T.shape[0] == d.ed.n_pairs
            got[lo] = (T, np.concatenate(rs_) if rs_ else np.zeros((0, 2), np.int32))

        for lo, hi in zip(cuts[:-1], cuts[1:]):
            slot = e.overlap_batch_async(lo, hi, parts=_parts(parts))
            if pending:                       # batch k is consumed while batch k + 1's copy is (possibly) still in flight
                consume(*pending)
            pending = (slot, lo, hi)
        consume(*pending)
        T = np.concatenate([got[lo][0] for lo in cuts[:-1]]); R = np.concatenate([got[lo][1] for lo in cuts[:-1]])
        assert T.shape[0] > 200 or name == "edge"
        want_r = o.window_ed(T) if thre <= 63 else e.window_ed_batch(T)
        assert (R == want_r).all(), np.flatnonzero((R != want_r).any(axis=1))[:10]
        # one batch against the blocking path over the same range: hao_window_ed_grid + hao_fetch_ed_grid
        lo, hi = cuts[1], cuts[2]
        e.overlap_batch(lo, hi)
        n = e.window_ed_grid(window, thre)
        bt, br = e.fetch_ed_grid(n)
        assert (bt.shape == got[lo][0].shape) and (bt == got[lo][0]).all() and (br == got[lo][1]).all()
        print(f"[ed deliver] {name} window {window} thre {thre} parts {parts}: {T.shape[0]} pairs, {int((R[:, 0] != NOALN).sum())} within the threshold")
    finally:
        e.close()


def _ol_only(e, d, r):
    import ctypes as C
    from hifiasm_amd.api import _arr
    oo = _arr(d.ol_off + 8 * (r - d.rid_lo), 2, np.uint64); m = int(oo[1] - oo[0])
    ol = np.zeros((m, 12), dtype=np.uint32)
    assert e.L.hao_unpack_overlaps(C.byref(d), r, ol.ctypes.data_as(C.c_void_p), m) == m
    return ol


def test_ed_part_needs_ol_a_config_and_a_valid_threshold():
    from hifiasm_amd.api import HaoError, DELIVER_OL, DELIVER_CL, DELIVER_ED
    e, rs = _engine("hifi")
    try:
        with pytest.raises(HaoError):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED)      # no hao_deliver_ed_config yet
        for w, t in ((375, 128), (0, 15), (65535, 0), (65000, 300)):
            with pytest.raises(HaoError):
                e.deliver_ed_config(w, t)
        with pytest.raises(HaoError):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED)      # (the refused configs set nothing)
        e.deliver_ed_config(375, 15)
        for p in (DELIVER_ED, DELIVER_CL | DELIVER_ED):
            with pytest.raises(HaoError):
                e.overlap_batch_async(0, rs.n, parts=p)                          # ED without OL
        slot = e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED)     # and with OL it runs
        d = e.deliver_wait(slot)
        assert d.ed.n_pairs > 200
        slot = e.overlap_batch_async(0, rs.n, parts=DELIVER_OL)
        e.deliver_wait(slot)
        with pytest.raises(HaoError):
            e.deliver_ed(slot)                                                    # a slot whose batch did not ask for ED
    finally:
        e.close()


def test_attached_contexts_have_their_own_grid():
    from hifiasm_amd.api import DELIVER_OL, DELIVER_ED
    e, rs = _engine("hifi")
    o = scenario_oracle("hifi")
    v1, v2 = e.attach(), e.attach()
    try:
        v1.deliver_ed_config(375, 15); v2.deliver_ed_config(775, 40)
        lo, hi = 5, rs.n - 4
        s1 = v1.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED)
        s2 = v2.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED)
        for v, s, (w, t) in ((v1, s1, (375, 15)), (v2, s2, (775, 40))):
            d = v.deliver_wait(s)
            assert (d.ed.window, d.ed.thre) == (w, t)
            T, R = [], []
            for r in range(lo, hi):
                tt, rr = v.delivered_ed(d, r)
                want = ed_tasks_grid_all(rs.lengths, [_ol_only(v, d, r)], r, w, t)
                assert (tt == want).all(), r
                T.append(tt); R.append(rr)
            T = np.concatenate(T); R = np.concatenate(R)
            assert T.shape[0] > 200 and (R == o.window_ed(T)).all()
        with pytest.raises(Exception):
            e.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED)      # the owner was never configured
    finally:
        v1.close(); v2.close(); e.close()


def test_batches_without_ed_are_unchanged():
    """with ED not requested, a batch's view - byte count, every count, every delivered byte - equals a run made before any config was set; with ED, the byte
    count grows by exactly the offsets and 3 bytes per pair"""
    from hifiasm_amd.api import DELIVER_OL, DELIVER_CL, DELIVER_ED
    e, rs = _engine("hifi")
    lo, hi = 2, rs.n - 1
    keys = ["rid_lo", "n_reads", "n_ol", "n_fc", "n_chains", "n_cl", "n_exc", "n_codes", "n_pos", "bytes"]
    try:
        def run(parts):
            d = e.deliver_wait(e.overlap_batch_async(lo, hi, parts=parts))
            return d, {k: int(getattr(d, k)) for k in keys}, [e.delivered_read(d, r) for r in range(lo, hi)]
        d0, f0, r0 = run(DELIVER_OL | DELIVER_CL)
        assert not bool(d0.exact) and d0.ed is None
        e.deliver_ed_config(375, 15)
        d1, f1, r1 = run(DELIVER_OL | DELIVER_CL)
        assert f1 == f0 and d1.ed is None
        for a, b in zip(r0, r1):
            assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
        d2, f2, r2 = run(DELIVER_OL | DELIVER_CL | DELIVER_ED)
        n_pairs = int(d2.ed.n_pairs)
        assert n_pairs > 200 and f2["bytes"] == f0["bytes"] + (hi - lo + 1) * 8 + 3 * n_pairs
        assert {k: f2[k] for k in keys if k != "bytes"} == {k: f0[k] for k in keys if k != "bytes"}
        for a, b in zip(r0, r2):
            assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
    finally:
        e.close()
