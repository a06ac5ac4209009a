"""The chain stage routes every (query, target) group of seed hits by its size (hao_size_class: up to 8 / 64 / 128 / 256 / 512 / 2048 hits and beyond) to a quick-check
kernel and, where that does not settle the group, to the DP kernel of the class: fourteen paths.  Scenario "cedge" (scenarios.chain_edge_reads) holds crafted groups
on both sides of every capacity edge, accepted and rejected ones; here the engine's census (hao_batch_chain_path) must show that every one of the fourteen paths ran,
its class counts must equal a host model of the classifier, and every read must give the oracle's seed hits, overlaps, fake cigars and chained hits - in one batch,
under the debug switches that force the chain stage's fallbacks, and with the query read alone in its batch or at its end."""
import os

import numpy as np
import pytest

import oracle_py
from scenarios import CEDGE_QID, CEDGE_TABLE, cedge_class, chain_edge_reads
from test_gpu_altpaths import SWITCHES, _env_of

pytestmark = pytest.mark.gpu

CHAIN_SWITCHES = [s for s in SWITCHES if s in ("HAO_DBG_FORCE=seq_chain", "HAO_DBG_FORCE=dp_nospec", "HAO_DBG_FORCE=dp_seqtail", "HAO_DBG_FORCE=dp_serial")]
_REF = {}


def _reference():
    """the read set, and once for all tests: the oracle's seed hits and results of every read, and the host model's groups per class of every read"""
    if not _REF:
        rs = chain_edge_reads()
        o = oracle_py.Oracle(rs.codes, rs.code_off)
        hom_ft = o.ft_gen(); o.pt_gen()
        kh = [o.seed_hits(r) for r in range(rs.n)]
        res = [o.lchain(r) for r in range(rs.n)]
        cls = np.zeros((rs.n, 7), dtype=np.int64); own = np.zeros((rs.n, 7), dtype=np.int64)
        for r in range(rs.n):      # a group = the seed hits of one target id, both strands
            for t, n in zip(*np.unique(kh[r][:, 0] & 0x7fffffff, return_counts=True)):
                cls[r, cedge_class(int(n))] += 1
                own[r, cedge_class(int(n))] += int(t) == r      # (a read's hits to itself are a group as well: counted, then skipped by every chain kernel)
        _REF.update(rs=rs, o=o, hom_ft=hom_ft, kh=kh, res=res, cls=cls, own=own)
    return _REF


def _engine(ref):
    from hifiasm_amd.api import Engine
    e = Engine(0)
    e.set_readset(ref["rs"])
    assert e.ha_ft_gen() == ref["hom_ft"]
    st = ref["o"].stats()
    assert e.ha_pt_gen() == (st["hom_cov"], st["het_cov"])
    return e


def _compare(e, ref, lo, hi):
    """every array of every read of the batch, no tolerance; then the census against the host model"""
    for r in range(lo, hi):
        a, b = e.fetch_seed_hits(r), ref["kh"][r]
        assert a.shape == b.shape and (a == b).all(), f"seed hits of read {r}"
        ol, fc, fo, cl = e.h_ec_lchain(r)
        ool, ofc, ofo, ocl = ref["res"][r]
        assert ol.shape == ool.shape and (ol == ool).all(), f"overlaps of read {r}"
        assert fc.shape == ofc.shape and (fc == ofc).all() and (fo == ofo).all(), f"fake cigars of read {r}"
        assert cl.shape == ocl.shape and (cl == ocl).all(), f"chained hits of read {r}"
    assert e.batch_totals()["overlaps"] == sum(ref["res"][r][0].shape[0] for r in range(lo, hi))
    cnt, slow = e.batch_chain_path()
    print(f"[chain census] reads {lo} .. {hi}: groups per class {cnt}, left to the DP {slow}")
    assert cnt == [int(x) for x in ref["cls"][lo:hi].sum(axis=0)]
    assert all(0 <= s <= c for s, c in zip(slow, cnt))
    return cnt, slow


def test_every_class_on_both_paths():
    ref = _reference()
    e = _engine(ref)
    try:
        e.overlap_batch(0, ref["rs"].n)
        cnt, slow = _compare(e, ref, 0, ref["rs"].n)
    finally:
        e.close()
    own = ref["own"].sum(axis=0)
    for x in range(7):
        assert slow[x] >= 1, f"class {x}: no group left to its DP kernel"
        assert cnt[x] - slow[x] - int(own[x]) >= 1, f"class {x}: no group settled by the quick check"


@pytest.mark.parametrize("switch", CHAIN_SWITCHES)
def test_fallbacks_at_the_edges(switch):
    ref = _reference()
    env = _env_of(switch)
    os.environ.update(env)
    try:
        e = _engine(ref)
        try:
            e.overlap_batch(0, ref["rs"].n)
            _compare(e, ref, 0, ref["rs"].n)
        finally:
            e.close()
    finally:
        for k in env:
            del os.environ[k]


def test_query_alone_and_last_of_two():
    """the class lists of a batch of one read, and of a batch that ends with it, lay out the same results"""
    ref = _reference()
    e = _engine(ref)
    try:
        for lo, hi in ((CEDGE_QID, CEDGE_QID + 1), (CEDGE_QID - 1, CEDGE_QID + 1)):
            e.overlap_batch(lo, hi)
            cnt, slow = _compare(e, ref, lo, hi)
            assert sum(cnt) >= len(CEDGE_TABLE)
            own = ref["own"][lo:hi].sum(axis=0)
            for x in range(7):      # the crafted targets alone put every class on both paths
                assert slow[x] >= 1 and cnt[x] - slow[x] - int(own[x]) >= 1, (x, cnt, slow)
    finally:
        e.close()
