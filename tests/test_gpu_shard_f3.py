"""The stages beyond the seam in SHARDED engines, over the gathered read store (include/hao.h: hao_dist_gather_reads, hao_reads_digest).  Loopback worlds of 2
and 3 ranks on one GPU, one host thread per rank, ragged shares (the world of 3 has a rank that owns a single read), over the small scenarios the window-list
tests run at the same window and error rate.  For every rank and every read it owns, bit for bit what ONE unsharded engine over the whole read set returns
(computed once per case and shared):
  * hao_fetch_exact; the tasks and results of hao_fetch_ed_grid after hao_window_ed_ref; hao_fetch_ed_ovlp, hao_fetch_rescue, hao_fetch_wlist (records,
    offsets, cigars); the streamed parts ED | RESCUE | WLIST | EXACT in batches of 64 reads;
  * the host-fed calls on tasks of tests/golden/ed.npz whose pattern AND text read belong to other ranks, against the fixture (hao_window_ed_batch and the
    four traced modes);
  * hao_reads_digest: every rank's value equals the unsharded engine's and a numpy computation of the definition;
  * the multi-chunk path (HAO_DBG_TEST=gather_chunk=4096): the same results and digests;
  * contracts: the refusal before the gather and again after hao_set_reads, a second gather is a no-op, an attached view runs a streamed batch, HAO_OK and no
    allocation on an unsharded engine (the emulated device library counts live allocations: the CPU twin checks the counter)."""
import functools
import os
import threading

import numpy as np
import pytest

from helpers import scenario_reads

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [("hifi", 775, 0.04), ("hifi", 775, 0.004), ("ont", 375, 0.015), ("nn", 200, 0.01)]
BS = 64      # reads per streamed batch


def _cuts(n, world):
    """ragged shares; the world of 3 has a rank that owns a single read"""
    return [0, n * 3 // 7, n] if world == 2 else [0, n * 2 // 5, n * 2 // 5 + 1, n]


def _shard(rs, lo, hi):
    from hifiasm_amd.synth import ReadSet
    return ReadSet(lo, rs.lengths[lo:hi].copy(), rs.packed[int(rs.pk_off[lo]):int(rs.pk_off[hi])].copy(), (rs.pk_off[lo:hi + 1] - rs.pk_off[lo]).copy(),
                   rs.codes[int(rs.code_off[lo]):int(rs.code_off[hi])].copy(), (rs.code_off[lo:hi + 1] - rs.code_off[lo]).copy())


# ---- hao_reads_digest on the host (the definition in include/hao.h) ----
_K1, _K2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93)


def _term(stream, i, w):
    """hao_dg_term on uint64 arrays (mod 2^64)"""
    z = np.asarray(w, dtype=np.uint64) + _K1 * (np.asarray(i, dtype=np.uint64) + np.uint64(1)) + np.full(1, stream, dtype=np.uint64) * _K2
    z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xbf58476d1ce4e5b9)
    z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def _host_digest(rs):
    mask = rs.n_mask()
    b = np.zeros(rs.n, dtype=np.uint64); s = np.zeros(rs.n, dtype=np.uint64)
    for r in range(rs.n):
        L = int(rs.lengths[r]); nb = L // 4 + 1
        raw = np.zeros((nb + 7) // 8 * 8, dtype=np.uint8); raw[:nb] = rs.packed[int(rs.pk_off[r]):int(rs.pk_off[r]) + nb]
        w = raw.view("<u8")
        b[r:r + 1] = _term(5, np.zeros(1), np.array([L])) + _term(5, np.arange(1, w.size + 1), w).sum(dtype=np.uint64, keepdims=True)
        sites = np.flatnonzero(mask[int(rs.code_off[r]):int(rs.code_off[r + 1])]) if mask is not None else np.zeros(0, dtype=np.int64)
        s[r:r + 1] = _term(6, np.zeros(1), np.array([sites.size])) + _term(6, np.arange(1, sites.size + 1), sites).sum(dtype=np.uint64, keepdims=True)
    rid = np.arange(rs.n)
    return int(_term(7, rid, b).sum(dtype=np.uint64)), int(_term(8, rid, s).sum(dtype=np.uint64))


# ---- what one engine returns for reads [0, n) of its own numbering (g0 = the global id of its read 0) ----
def _blocking(e, n, g0, wl, e_rate):
    """per GLOBAL read id: exact flags, the read's grid tasks and results, summaries, rescue results, window lists"""
    e.overlap_batch(0, n)
    exact = [e.fetch_exact(r) for r in range(n)]
    nt, unres = e.window_ed_ref(wl, e_rate)
    T, R = e.fetch_ed_grid(nt)
    sums = [e.fetch_ed_ovlp(r) for r in range(n)]
    resc = e.window_rescue_ref()
    rs_ = [e.fetch_rescue(r) for r in range(n)]
    tot = e.window_wlist_ref()
    wl_ = [e.fetch_wlist(r) for r in range(n)]
    out = {}
    for r in range(n):
        m = T[:, 4] == g0 + r                                                   # (t_rid: the query read, a global id)
        out[g0 + r] = dict(exact=exact[r], T=T[m], R=R[m], sums=sums[r], rs=rs_[r], wl=wl_[r])
    assert sum(v["T"].shape[0] for v in out.values()) == nt                     # every task belongs to a read of the batch
    return out, (nt, unres, resc) + tot


def _streamed(e, n, g0, wl, e_rate, lengths, first=0, last=None):
    """per GLOBAL read id, out of DELIVER_OL | ED | RESCUE | WLIST | EXACT batches of BS reads: exact flags, pairs, summaries, rescue results, window lists"""
    from hifiasm_amd.api import DELIVER_OL, DELIVER_ED, DELIVER_RESCUE, DELIVER_WLIST, DELIVER_EXACT, _arr
    e.deliver_ed_config_ref(wl, e_rate)
    last = n if last is None else last
    cuts = list(range(first, last, BS)) + [last]
    out, pending = {}, None

    def consume(slot, lo, hi):
        d = e.deliver_wait(slot)
        assert (int(d.rid_lo), int(d.n_reads)) == (lo, hi - lo) and d.ed is not None and d.rs is not None and d.wl is not None
        g = e.delivery_global(d) if g0 else d                                   # (the unpack helpers name reads as the lengths array does: globally)
        off = _arr(d.ol_off, hi - lo + 1, np.uint64); ex = _arr(d.exact, int(d.n_ol), np.uint8)
        for r in range(lo, hi):
            t, res = e.delivered_ed(g, g0 + r, lengths)
            out[g0 + r] = dict(exact=ex[int(off[r - lo]):int(off[r - lo + 1])], T=t, R=res, sums=e.delivered_ed_ovlp(g, g0 + r),
                               rs=e.delivered_rescue(g, g0 + r, lengths), wl=e.delivered_wlist(g, g0 + r, lengths))

    for lo, hi in zip(cuts[:-1], cuts[1:]):
        slot = e.overlap_batch_async(lo, hi, parts=DELIVER_OL | DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST | DELIVER_EXACT)
        if pending:
            consume(*pending)
        pending = (slot, lo, hi)
    consume(*pending)
    return out


def _same_wl(a, b):
    return len(a) == len(b) and all(x[0].shape == y[0].shape and (x[0] == y[0]).all() and len(x[1]) == len(y[1]) and all(p.shape == q.shape and (p == q).all() for p, q in zip(x[1], y[1])) for x, y in zip(a, b))


def _same_rs(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and len(a[1]) == len(b[1]) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a[1], b[1]))


def _diff(got, want):
    """the first field of a read's results that differs, or None (a streamed pair's results are the delivery's bytes widened: the same values)"""
    if not (got["exact"].shape == want["exact"].shape and (got["exact"] == want["exact"]).all()):
        return "exact"
    if not (got["T"].shape == want["T"].shape and (got["T"] == want["T"]).all() and (got["R"] == want["R"]).all()):
        return "grid tasks / results"
    if not (got["sums"].shape == want["sums"].shape and (got["sums"] == want["sums"]).all()):
        return "summaries"
    if not _same_rs(got["rs"], want["rs"]):
        return "rescue"
    if not _same_wl(got["wl"], want["wl"]):
        return "wlist"
    return None


@functools.lru_cache(maxsize=None)
def _reference(name, wl, e_rate):
    """the unsharded engine over the whole read set: blocking and streamed results per read, the totals, the digest; computed once per case"""
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads(name)
    e = Engine(0, **okw)
    try:
        e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
        blk, tot = _blocking(e, rs.n, 0, wl, e_rate)
        stm = _streamed(e, rs.n, 0, wl, e_rate, rs.lengths)
        return dict(blk=blk, tot=tot, stm=stm, digest=e.reads_digest())
    finally:
        e.close()


def _world(name, world, body, gather=True):
    """`world` sharded engines over scenario `name` in one loopback group, one thread per rank: tables, (gather,) body(rank, engine, lo, hi) -> result per rank"""
    from hifiasm_amd.api import Engine, lib
    rs, okw = scenario_reads(name)
    cuts = _cuts(rs.n, world)
    grp = lib().hao_loop_create(world)
    errors, out = [], [None] * world

    def run(rank):
        e = None
        try:
            lo, hi = cuts[rank], cuts[rank + 1]
            e = Engine(0, **okw)
            e.set_readset(_shard(rs, lo, hi)); e.set_shard(lo, rs.lengths); e.dist_init_loopback(grp, rank)
            e.ha_ft_gen(); e.ha_pt_gen()
            if gather:
                e.dist_gather_reads()
            out[rank] = body(rank, e, lo, hi)
        except Exception as ex:  # noqa: BLE001
            errors.append(f"rank {rank}: {ex!r}")
        finally:
            if e is not None:
                e.close()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    assert not any(t.is_alive() for t in th), "a rank is stuck in a collective"
    lib().hao_loop_destroy(grp)
    assert not errors, errors[:5]
    return rs, cuts, out


def _parity(name, wl, e_rate, world):
    ref = _reference(name, wl, e_rate)
    rs0, _ = scenario_reads(name)

    def body(rank, e, lo, hi):
        dg = e.reads_digest()
        blk, tot = _blocking(e, hi - lo, lo, wl, e_rate)
        stm = _streamed(e, hi - lo, lo, wl, e_rate, rs0.lengths)
        return dg, blk, tot, stm

    rs, cuts, out = _world(name, world, body)
    tot = np.zeros(8, dtype=np.int64)
    for rank, (dg, blk, t, stm) in enumerate(out):
        assert dg == ref["digest"], f"rank {rank}: the gathered store's digest differs from the unsharded engine's"
        assert sorted(blk) == sorted(stm) == list(range(cuts[rank], cuts[rank + 1]))
        for r in blk:
            d = _diff(blk[r], ref["blk"][r])
            assert d is None, f"rank {rank}, read {r}: blocking {d} differs from the unsharded engine's"
            d = _diff(stm[r], ref["stm"][r])
            assert d is None, f"rank {rank}, read {r}: streamed {d} differs from the unsharded engine's"
        tot += np.array(t, dtype=np.int64)
    assert tuple(int(x) for x in tot) == ref["tot"]                              # pairs, unresolved, rescued windows and the five window-list counts add up
    assert ref["tot"][0] > 1000 and ref["tot"][3] > 100
    return ref


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,wl,e_rate", CASES)
def test_sharded_stages_equal_the_unsharded_engine(name, wl, e_rate, world):
    _parity(name, wl, e_rate, world)


def test_multi_chunk_gather(monkeypatch):
    """4 KB a rank and exchange: the packed bytes, the offsets and the N sites of the nn set cross in several chunks each; results and digests do not change"""
    monkeypatch.setenv("HAO_DBG_TEST", "gather_chunk=4096")
    rs, _ = scenario_reads("nn")
    assert int(rs.pk_off[_cuts(rs.n, 3)[1]]) > 3 * 4096                         # (rank 0's bytes alone take more than three exchanges)
    _parity("nn", 200, 0.01, 3)


@pytest.mark.parametrize("name", ["hifi", "nn"])
def test_reads_digest_equals_the_definition(name):
    """the device's digest of an unsharded engine's store = the definition computed with numpy; hao_dist_gather_reads there: HAO_OK and nothing allocated"""
    from hifiasm_amd.api import Engine, lib
    rs, okw = scenario_reads(name)
    try:
        live = lib().hao_simt_live_allocations                                   # (the emulated device library's counter of live allocations: CPU twin only)
        import ctypes as C
        live.restype = C.c_long; live.argtypes = []
    except AttributeError:
        live = None
    e = Engine(0, **okw)
    try:
        e.set_readset(rs)
        before = live() if live else 0
        e.dist_gather_reads(); e.dist_gather_reads()
        assert (live() if live else 0) == before
        got = e.reads_digest()
        assert e.reads_digest() == got                                           # (the scratch word is zeroed per call)
        assert got == _host_digest(rs), (got, _host_digest(rs))
        if name == "nn":
            assert rs.n_mask() is not None and rs.n_mask().sum() > 0             # the N-site half covers sites
    finally:
        e.close()


@pytest.mark.parametrize("world", [2, 3])
def test_host_fed_tasks_between_other_ranks_reads(world):
    """hao_window_ed_batch and the four traced modes in a sharded engine: a few hundred fixture tasks per rank whose pattern and text reads both belong to OTHER
    ranks, against the fixture's results (the reference's own functions, tests/test_oracle_ed.py)"""
    g = np.load(os.path.join(GOLDEN, "ed.npz"))
    name = "nn"

    def pick(tasks, lo, hi):
        other = ((tasks[:, 0] < lo) | (tasks[:, 0] >= hi)) & ((tasks[:, 4] < lo) | (tasks[:, 4] >= hi))
        return np.flatnonzero(other)[:300]

    def body(rank, e, lo, hi):
        bad = []
        ix = pick(g[f"{name}_tasks"], lo, hi)
        if not (ix.size >= 100 and (e.window_ed_batch(g[f"{name}_tasks"][ix]) == g[f"{name}_res"][ix]).all()):
            bad.append(("ed", ix.size))
        for mode, key in ((0, "g"), (3, "s"), (1, "x1"), (2, "x2")):
            tk = f"{name}_{'x' if key.startswith('x') else key}tasks"
            want, wcig = g[f"{name}_{key}res"], g[f"{name}_{key}cig"]
            off = np.concatenate(([0], np.cumsum(want[:, 5])))
            ix = pick(g[tk], lo, hi)
            res, cig = e.window_trace_batch(g[tk][ix], cap=136, mode=mode)
            if not (ix.size >= 100 and (res == want[ix]).all() and all((cig[k, :want[q, 5]] == wcig[off[q]:off[q + 1]]).all() for k, q in enumerate(ix))):
                bad.append((mode, ix.size))
        return bad

    _, _, out = _world(name, world, body)
    assert all(b == [] for b in out), out


def test_contracts():
    """the refusal before the gather and again after hao_set_reads; a second gather is a no-op; an attached view runs a streamed batch over the borrowed store"""
    from hifiasm_amd.api import HaoError
    name, wl, e_rate = "hifi", 775, 0.004
    ref = _reference(name, wl, e_rate)
    rs0, _ = scenario_reads(name)
    g = np.load(os.path.join(GOLDEN, "ed.npz"))

    def refused(f):
        try:
            f()
        except HaoError as ex:
            return "(-4)" in str(ex) and "single-device mode only" in str(ex)
        return False

    def body(rank, e, lo, hi):
        seen = []
        e.overlap_batch(0, hi - lo)
        seen.append(refused(lambda: e.window_ed_ref(wl, e_rate)))                # before the gather: today's refusal
        seen.append(refused(lambda: e.fetch_exact(0)))
        seen.append(refused(e.reads_digest))
        e.dist_gather_reads()
        dg = e.reads_digest()
        e.dist_gather_reads()                                                    # valid: a no-op (no collective: a rank may call it alone)
        if rank == 0:
            e.dist_gather_reads()
        seen.append(e.reads_digest() == dg == ref["digest"])
        v = e.attach()                                                           # a view borrows the store
        try:
            last = min(hi - lo, BS)
            stm = _streamed(v, hi - lo, lo, wl, e_rate, rs0.lengths, 0, last)
            seen.append(all(_diff(stm[r], ref["stm"][r]) is None for r in range(lo, lo + last)))
            seen.append(v.reads_digest() == dg)
        finally:
            v.close()
        e.set_readset(_shard(rs0, lo, hi)); e.set_shard(lo, rs0.lengths)         # new reads: the store is gone, the refusal is back
        seen.append(refused(lambda: e.window_ed_batch(g["hifi_tasks"][:8])))
        seen.append(refused(e.reads_digest))
        e.dist_gather_reads()                                                    # (a collective again)
        seen.append(e.reads_digest() == dg)
        seen.append(bool((e.window_ed_batch(g["hifi_tasks"][:64]) == g["hifi_res"][:64]).all()))
        return seen

    _, _, out = _world(name, 2, body, gather=False)
    assert all(all(s) for s in out), out


def _ngpu():
    import torch
    return torch.cuda.device_count()


def test_rccl_gather_between_processes():
    """the gather over RCCL, one process per GPU (tests/gather_worker.py); needs 2 GPUs - tests/test_dist_gather_cpu.py runs the same worker over the
    emulated transport"""
    import subprocess
    import sys
    if _ngpu() < 2:
        pytest.skip(f"{_ngpu()} GPU(s) visible, 2 needed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29517",
           os.path.join(root, "tests", "gather_worker.py"), "hifi"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("0 differ") == 2, r.stdout[-1500:]
