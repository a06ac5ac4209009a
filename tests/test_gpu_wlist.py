"""The window lists of align_hc_ed_post_extz on the device (include/hao.h: hao_window_wlist_ref, hao_fetch_wlist), blocking path.  For every read of the small
read sets, none left out:
  * the records, the cigar offsets and the entries equal tests/wlist_model.py driven by the oracle live, over the device's own primary results (which
    tests/test_gpu_refgrid.py holds against the oracle) and tests/rescue_model.py's rescue (which tests/test_gpu_rescue.py holds the device against);
  * every alignment the model asked the oracle for - each traced window's task and each re-placement - gives the same (err, ps, pe, cigar) through
    hao_window_trace_batch(HAO_ALIGN_SEMI) on the device, so a traced record is what that call gives on the model's task;
  * the categories a case is known to hold are met (EXPECT; each case prints what it met);
  * out[1] equals the model's count of windows in the domain whose record has err > 0 (windows with err == 0 are not swept), out[0] / out[3] / out[4] the
    records, entries and untraced windows of the model;
  * records of backward-rescued windows and anchors carry hao_fetch_rescue's y_start, y_end, err and re-placed bit; the rescue results stay fetchable.
Contract: HAO_EINVAL without hao_window_ed_ref and hao_window_rescue_ref on the batch, after another window-alignment call - host-fed, or hao_window_ed_grid
whatever its pair count (the rescue results stay fetchable) - after a new batch; a second call gives the same result; fetch argument errors; HAO_EUNSUPP from both entry points in a sharded engine.
Streamed (HAO_DELIVER_OL | HAO_DELIVER_ED | HAO_DELIVER_RESCUE | HAO_DELIVER_WLIST after hao_deliver_ed_config_ref, batches of 64 and 257 reads): what
hao_unpack_wlist hands back equals the blocking path's lists over the same ranges; a batch without the part, before and after one with it, has the bytes it has
without the feature, and the part adds exactly the record offsets, 16 bytes per record, the entry offsets and 2 bytes per entry (each padded to 64 bytes in the
arena, which `bytes` does not count); HAO_DELIVER_WLIST without HAO_DELIVER_RESCUE or HAO_DELIVER_ED or on a diagonal-placed context fails with HAO_EINVAL.
On the sampled reads of tests/golden/wlist.npz (the reference's own functions) the blocking lists equal the fixture."""
import numpy as np
import pytest

from helpers import scenario_reads, scenario_oracle, scenario_engine, MANY_SLICES
import rescue_model as RM
import wlist_model as WM

pytestmark = pytest.mark.gpu
NOALN = 2**31 - 1
# the last two: the smallest configurations found (tests/golden/make_golden_wlist.py's scan) that hold a re-placement TAKEN inside a passing overlap and forward
# windows with err == 0 (nn at 200-base windows), and untraced windows (hifi at 375-base windows and 1 %)
CASES = [("hifi", 775, 0.04), ("hifi", 775, 0.004), ("ont", 375, 0.015), ("fz2", 1500, 0.006), ("edge", 775, 0.04), ("nn", 200, 0.01), ("hifi", 375, 0.01)]
# what tests/wlist_model.py meets over the oracle in each case (the read sets are seeded, so this is fixed)
COMMON = ("primary_err0", "primary_traced", "recal_not_taken", "indel_both")
EXPECT = {("hifi", 775, 0.04): COMMON + ("backward_traced", "anchor_traced", "verdict1_with_rescued"),
          ("hifi", 775, 0.004): COMMON + ("forward_traced", "backward_traced", "anchor_traced", "verdict0", "verdict1_with_rescued"),
          ("ont", 375, 0.015): COMMON + ("forward_traced", "backward_traced", "anchor_traced", "verdict0", "verdict1_with_rescued"),
          ("fz2", 1500, 0.006): COMMON + ("forward_traced", "backward_traced", "anchor_traced", "verdict0", "verdict1_with_rescued"),
          ("edge", 775, 0.04): COMMON + ("verdict0",),
          ("nn", 200, 0.01): COMMON + ("replaced", "forward_err0", "forward_traced", "backward_traced", "anchor_traced"),
          ("hifi", 375, 0.01): COMMON + ("untraced", "forward_traced", "backward_traced", "anchor_traced")}


GOLD_KEY = {("hifi", 775, 0.04): "hifi", ("hifi", 775, 0.004): "hifi004", ("ont", 375, 0.015): "ont015", ("fz2", 1500, 0.006): "fz2w", ("nn", 200, 0.01): "nn200", ("hifi", 375, 0.01): "hifi375"}


def _engine(name, env=None):
    e, rs = scenario_engine(name, env)
    e.ha_ft_gen(); e.ha_pt_gen()
    return e, rs


def _blocking_case(name, wl, e_rate, env=None, min_swept=0):
    """min_swept: the windows the model sweeps - the records of the stage's sliced sweep - are at least that many, asserted before the stage runs"""
    e, rs = _engine(name, env)
    o = scenario_oracle(name)
    align, trace0 = RM.oracle_aligner(o), WM.oracle_tracer(o)
    asked = {}

    def trace(task):
        k = tuple(int(x) for x in task)
        if k not in asked:
            asked[k] = trace0(task)
        return asked[k]
    seen = {}
    try:
        e.overlap_batch(0, rs.n)
        n, unres = e.window_ed_ref(wl, e_rate)
        assert unres == 0
        T, R = e.fetch_ed_grid(n)
        wants, k = [], 0
        for r in range(rs.n):
            ol, fc, fo, _ = e.h_ec_lchain(r)
            m = RM.M.read_tasks(ol, fc, fo, rs.lengths, wl, e_rate).shape[0]
            wants.append(WM.read_wlist(ol, fc, fo, rs.lengths, wl, e_rate, R[k:k + m], align, trace))
            k += m
        assert sum(sw for rr, want in wants for ww, wc, ev, sw, nt in want) >= min_swept
        total = e.window_rescue_ref()
        out = e.window_wlist_ref()
        assert e.window_wlist_ref() == out                                       # again on the same batch: the same result
        n_rec = n_swept = n_cig = n_untr = n_ol = n_tried = 0
        for r in range(rs.n):
            rr, want = wants[r]
            got = e.fetch_wlist(r)
            ov, rwins = e.fetch_rescue(r)                                        # (still fetchable)
            assert len(got) == len(want) == ov.shape[0]
            for i, ((gw, gc), (ww, wc, ev, sw, nt)) in enumerate(zip(got, want)):
                assert int(ov["verdict"][i]) == rr[i]["verdict"]
                assert gw.shape == ww.shape and (gw == ww).all(), (r, i, gw, ww)
                assert len(gc) == len(wc) and all(tuple(int(x) for x in a) == tuple(b) for a, b in zip(gc, wc)), (r, i, gc, wc)
                if ww.shape[0]:                                                  # backward windows and anchors: hao_fetch_rescue's values
                    by = {int(x[0]): x for x in rwins[i]}
                    for x in gw:
                        if int(x[5]) in (WM.BWD, WM.ANCHOR) and not int(x[7]):
                            q = by[int(x[0])]
                            assert [int(v) for v in x[:4]] + [int(x[6])] == [int(v) for v in q[:4]] + [int(q[6])] and int(q[5]) == int(x[5]), (r, i, x, q)
                n_rec += ww.shape[0]; n_swept += sw; n_tried += nt; n_cig += sum(len(c) for c in wc); n_untr += int(ww[:, 7].sum()) if ww.shape[0] else 0
                for c in ev:
                    seen[c] = seen.get(c, 0) + 1
            n_ol += len(want)
        assert k == n and n_ol > 100
        print(f"[wlist] {name} ({wl}, {e_rate}): {out[0]} records in {n_ol} overlaps, {out[1]} swept, {out[2]} re-placement sweeps, {out[3]} cigar entries, {out[4]} untraced; {dict(sorted(seen.items()))}")
        assert out == (n_rec, n_swept, n_tried, n_cig, n_untr), (out, n_rec, n_swept, n_tried, n_cig, n_untr)
        assert e.window_rescue_ref() == total                                    # the stage changed nothing the rescue stage reads
        # every alignment the model asked for, through the device's own traced batch call
        tasks = np.array(sorted(asked), dtype=np.int64).reshape(-1, 10).astype(np.uint32)
        assert tasks.shape[0] >= out[1]
        res, cig = e.window_trace_batch(tasks, cap=96, mode=3)
        for t, a, c in zip(sorted(asked), res, cig):
            w = asked[t]
            assert (int(a[0]), int(a[1]), int(a[2])) == w[:3] and tuple(int(x) for x in c[:int(a[5])]) == w[3], (t, a, w)
        gk = GOLD_KEY.get((name, wl, e_rate))
        if gk:                                                                   # the real reference on the sampled reads
            G = WM.gold(); want_g = WM.gold_lists(G, gk); q = 0
            e.overlap_batch(0, rs.n); e.window_ed_ref(wl, e_rate); e.window_rescue_ref(); e.window_wlist_ref()      # (the traced batch call above took the stage's input)
            for r in G[gk + "_reads"]:
                for gw, gc in e.fetch_wlist(int(r)):
                    ww, wc, _, _ = want_g[q]
                    assert gw.shape == ww.shape and (gw == ww).all() and [tuple(int(x) for x in c) for c in gc] == wc, (int(r), q)
                    q += 1
            assert q == len(want_g)
        missing = [c for c in EXPECT[(name, wl, e_rate)] if not seen.get(c)]
        assert not missing, (missing, seen)
    finally:
        e.close()


@pytest.mark.parametrize("name,wl,e_rate", CASES)
def test_wlist_blocking_equals_the_model(name, wl, e_rate):
    _blocking_case(name, wl, e_rate)


@pytest.mark.parametrize("case", [("nn", 200, 0.01)])      # (the emulated twin takes a smaller case of CASES: tests/test_simt_wlist_cpu.py)
def test_wlist_blocking_in_many_slices(case):
    """the case of CASES with the most swept windows (nn at 200 / 1 %: 44 065), with a column budget of 8 bytes: the traced sweep walks slices of 256 records, the
    last one partial, where the default budget makes it one slice"""
    _blocking_case(*case, env=MANY_SLICES, min_swept=257)


def test_contract():
    from hifiasm_amd.api import HaoError
    e, rs = _engine("hifi")
    try:
        e.overlap_batch(0, rs.n)
        with pytest.raises(HaoError, match=r"\(-2\)"):                          # neither stage has run on the batch
            e.window_wlist_ref()
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_wlist(0)
        n, _ = e.window_ed_ref(775, 0.004)
        with pytest.raises(HaoError, match=r"\(-2\)"):                          # no hao_window_rescue_ref
            e.window_wlist_ref()
        T, R = e.fetch_ed_grid(n)
        e.window_rescue_ref()
        e.window_ed_batch(T[:64])                                              # another window-alignment call: the stage's input is gone
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_wlist_ref()
        e.window_ed_ref(775, 0.004)
        e.window_rescue_ref()
        out = e.window_wlist_ref()
        assert out[0] > 1000 and 0 < out[1] < out[0] and out[3] > out[0]
        a = e.fetch_wlist(3)
        assert len(a) == e.h_ec_lchain(3)[0].shape[0]
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_wlist(rs.n)
        assert e.window_wlist_ref() == out
        b = e.fetch_wlist(3)
        assert all((x[0] == y[0]).all() and all((p == q).all() for p, q in zip(x[1], y[1])) for x, y in zip(a, b))
        e.window_rescue_ref()                                                  # a new rescue pass: the lists are gone until the stage runs again
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_wlist(3)
        e.window_wlist_ref()
        GRID_THRE = 31                                                         # (as many pairs as hao_window_ed_ref forms here: tests/test_gpu_rescue.py)
        n_ref, _ = e.window_ed_ref(775, 0.04)                                  # a diagonal-placed grid call takes the shared scratch: refused whatever its pair count
        e.window_rescue_ref(); e.window_wlist_ref()
        ov, wins = e.fetch_rescue(3)
        n_grid = e.window_ed_grid(775, GRID_THRE)
        print(f"[wlist] contract: {n_ref} pairs of hao_window_ed_ref, {n_grid} of hao_window_ed_grid(775, {GRID_THRE})")
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_wlist_ref()
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_wlist(0)
        ov2, wins2 = e.fetch_rescue(3)                                         # (the rescue results lie in buffers of their own)
        assert (ov2 == ov).all() and all((a == b).all() for a, b in zip(wins, wins2))
        e.overlap_batch(1, rs.n)                                               # a new batch
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.fetch_wlist(3)
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.window_wlist_ref()
    finally:
        e.close()


def _same(a, b):
    return len(a) == len(b) and all(x[0].shape == y[0].shape and (x[0] == y[0]).all() and len(x[1]) == len(y[1]) and all(p.shape == q.shape and (p == q).all() for p, q in zip(x[1], y[1])) for x, y in zip(a, b))


@pytest.mark.parametrize("name,bs,cfg", [("hifi", 64, (775, 0.004)), ("hifi", 257, (775, 0.04)), ("ont", 64, (375, 0.015)), ("fz2", 257, (1500, 0.006)), ("edge", 257, (775, 0.04))])
def test_wlist_streamed_equals_blocking(name, bs, cfg):
    from hifiasm_amd.api import DELIVER_OL, DELIVER_ED, DELIVER_RESCUE, DELIVER_WLIST
    wl, e_rate = cfg
    e, rs = _engine(name)
    try:
        e.deliver_ed_config_ref(wl, e_rate)
        cuts = list(range(0, rs.n, bs)) + [rs.n]
        got, pending, totals = {}, None, []

        def consume(slot, lo, hi):
            d = e.deliver_wait(slot)
            assert (d.rid_lo, d.n_reads) == (lo, hi - lo) and d.rs is not None and d.wl is not None and d.wl.n_ol == d.n_ol
            nw = nc = 0
            for r in range(lo, hi):
                got[r] = e.delivered_wlist(d, r, rs.lengths)
                nw += sum(x[0].shape[0] for x in got[r]); nc += sum(len(c) for x in got[r] for c in x[1])
            assert (nw, nc) == (d.wl.n_wins, d.wl.n_cigar)
            totals.append((int(d.wl.n_wins), int(d.wl.n_swept), int(d.wl.n_replace), int(d.wl.n_cigar), int(d.wl.n_untraced)))

        for lo, hi in zip(cuts[:-1], cuts[1:]):
            slot = e.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST)
            if pending:
                consume(*pending)
            pending = (slot, lo, hi)
        consume(*pending)
        for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):                 # the blocking path over the same ranges
            e.overlap_batch(lo, hi)
            e.window_ed_ref(wl, e_rate); e.window_rescue_ref()
            assert e.window_wlist_ref() == totals[k]
            for r in range(lo, hi):
                assert _same(e.fetch_wlist(r), got[r]), r
        assert sum(t[0] for t in totals) > 100
    finally:
        e.close()


def test_batches_without_the_part_keep_their_bytes():
    from hifiasm_amd.api import DELIVER_OL, DELIVER_CL, DELIVER_ED, DELIVER_RESCUE, DELIVER_WLIST
    e, rs = _engine("hifi")
    lo, hi = 2, rs.n - 1
    keys = ["rid_lo", "n_reads", "n_ol", "n_fc", "n_chains", "n_cl", "n_exc", "n_codes", "n_pos", "bytes"]
    try:
        e.deliver_ed_config_ref(775, 0.004)

        def run(parts):
            d = e.deliver_wait(e.overlap_batch_async(lo, hi, parts=parts))
            return d, {k: int(getattr(d, k)) for k in keys}, [e.delivered_read(d, r) for r in range(lo, hi)], [e.delivered_rescue(d, r, rs.lengths) for r in range(lo, hi)]
        base = DELIVER_OL | DELIVER_CL | DELIVER_ED | DELIVER_RESCUE
        d0, f0, r0, s0 = run(base)                                                       # before
        assert d0.wl is None
        d1, f1, r1, s1 = run(base | DELIVER_WLIST)                                       # with the part
        assert d1.wl is not None and d1.wl.n_wins > 1000 and d1.wl.n_cigar > d1.wl.n_wins
        assert f1["bytes"] == f0["bytes"] + 8 * (f0["n_ol"] + 1) + 16 * int(d1.wl.n_wins) + 8 * (int(d1.wl.n_wins) + 1) + 2 * int(d1.wl.n_cigar)
        d2, f2, r2, s2 = run(base)                                                       # after
        assert f2 == f0 and d2.wl is None
        for rr in (r1, r2):
            for a, b in zip(r0, rr):
                assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
        for ss in (s1, s2):
            for a, b in zip(s0, ss):
                assert (a[0] == b[0]).all() and all(x.shape == y.shape and (x == y).all() for x, y in zip(a[1], b[1]))
    finally:
        e.close()


def test_streamed_contract():
    from hifiasm_amd.api import HaoError, DELIVER_OL, DELIVER_ED, DELIVER_RESCUE, DELIVER_WLIST
    e, rs = _engine("hifi")
    try:
        e.deliver_ed_config_ref(775, 0.04)
        with pytest.raises(HaoError, match=r"\(-2\)"):                          # without HAO_DELIVER_RESCUE
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_WLIST)
        with pytest.raises(HaoError, match=r"\(-2\)"):                          # without HAO_DELIVER_ED
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_WLIST)
        e.deliver_ed_config(375, 15)                                             # a diagonal-placed context
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST)
        e.deliver_ed_config_ref(775, 0.004)
        slot = e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE)      # a batch that did not ask for the part has no view
        d = e.deliver_wait(slot)
        with pytest.raises(HaoError, match=r"\(-2\)"):
            e.deliver_wlist(slot)
        with pytest.raises(HaoError):
            e.delivered_wlist(d, 3, rs.lengths)
        d = e.deliver_wait(e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST))
        assert len(e.delivered_wlist(d, 3, rs.lengths)) == e.delivered_rescue(d, 3, rs.lengths)[0].shape[0] > 0
    finally:
        e.close()


def test_sharded_engine_is_refused():
    """a sharded engine holds only its own reads' bases: both entry points return HAO_EUNSUPP (one rank over the in-process transport is a sharded engine)"""
    from hifiasm_amd.api import Engine, HaoError, lib, DELIVER_OL, DELIVER_ED, DELIVER_RESCUE, DELIVER_WLIST
    rs, okw = scenario_reads("hifi")
    grp = lib().hao_loop_create(1)
    e = Engine(0, **okw)
    try:
        e.set_readset(rs); e.set_shard(0, rs.lengths); e.dist_init_loopback(grp, 0)
        e.ha_ft_gen(); e.ha_pt_gen()
        e.overlap_batch(0, rs.n)
        with pytest.raises(HaoError, match=r"\(-4\)"):
            e.window_wlist_ref()
        with pytest.raises(HaoError, match=r"\(-4\)"):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_WLIST)
        with pytest.raises(HaoError, match=r"\(-4\)"):
            e.overlap_batch_async(0, rs.n, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST)
    finally:
        e.close()
        lib().hao_loop_destroy(grp)
