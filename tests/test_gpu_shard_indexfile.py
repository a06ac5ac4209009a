"""Index files from and into SHARDED engines (include/hao.h: hao_index_save as a collective, hao_index_load_dist).  Loopback worlds of 2 and 3 ranks on one
GPU, one host thread per rank, the ragged cuts of tests/test_gpu_shard_f3.py (the world of 3 has a rank that owns a single read), over the small scenarios:
hifi (plain), nn (N sites on both sides of a cut), edge (ragged and degenerate reads), ont.
  * save: the world builds its tables, gathers and saves; the three files are byte for byte what ONE unsharded engine over all reads writes (computed once per
    scenario and shared), with default names and with explicit names on rank 0 and NULL elsewhere; every rank reads the files the moment its own call
    returns (a peer's return waits for rank 0's write); before the gather every rank is refused (HAO_EUNSUPP) and no file appears;
  * load: the world loads the unsharded engine's files with the ragged cuts and with NULL cuts; on every rank the tables and thresholds equal the golden
    dump, every owned read's overlaps, fake cigars and chained hits and every 7th read's sketch equal the oracle's, and after hao_dist_gather_reads the
    digest of the store equals the unsharded engine's; the same for a file the unmodified reference wrote (hifi, nn; where oracle/_ref/ref_harness exists);
  * round trip: load sharded, gather, save sharded - the bytes of the input;
  * failures: a prefix that exists on all ranks but one, a file cut inside the last rank's packed reads, cuts that do not end at the read count - an error on
    EVERY rank, nobody left in a collective, no index afterwards, and a good load on the same engines succeeds after each;
  * an unsharded engine: hao_index_load_dist with NULL and with the cuts [0, n] is hao_index_load."""
import ctypes as C
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

from helpers import scenario_reads, scenario_oracle, load_golden
from test_gpu_shard_f3 import _cuts, _shard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
NAMES = ["hifi", "nn", "edge", "ont"]
SUFFIXES = (".pt_flt", ".pt_flt.bin", ".pt_flt.paf.bin")
STATS = ("hom_cov", "het_cov", "max_n_chain", "high_occ", "low_occ")


def _blob(prefix):
    return {s: open(prefix + s, "rb").read() for s in SUFFIXES}


def _read_names(n):
    """names of unequal lengths, none of them the default"""
    return [f"m{i % 7}/{i * i}/ccs" for i in range(n)]


@functools.lru_cache(maxsize=None)
def _single(name):
    """the unsharded engine over the whole read set: its files with default and with explicit names, its digest; computed once per scenario"""
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads(name)
    d = tempfile.mkdtemp(prefix="hao_sidx_")
    e = Engine(0, **okw)
    try:
        e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
        e.index_save(os.path.join(d, "one"))
        e.index_save(os.path.join(d, "one_named"), names=_read_names(rs.n))
        return dict(dir=d, prefix=os.path.join(d, "one"), blob=_blob(os.path.join(d, "one")), named=_blob(os.path.join(d, "one_named")), digest=e.reads_digest())
    finally:
        e.close()


def _world(name, world, body):
    """`world` engines of scenario `name`'s options in one loopback group, one thread per rank: body(rank, engine) -> result per rank"""
    from hifiasm_amd.api import Engine, lib
    _, okw = scenario_reads(name)
    grp = lib().hao_loop_create(world)
    errors, out = [], [None] * world

    def run(rank):
        e = None
        try:
            e = Engine(0, **okw)
            e.dist_init_loopback(grp, rank)
            out[rank] = body(rank, e)
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
    return out


def _build(e, rs, lo, hi):
    e.set_readset(_shard(rs, lo, hi)); e.set_shard(lo, rs.lengths)
    e.ha_ft_gen(); e.ha_pt_gen()


def _code(f):
    """the error code a call fails with, or 0"""
    from hifiasm_amd.api import HaoError
    try:
        f()
    except HaoError as ex:
        return int(str(ex).split("failed (")[1].split(")")[0]), str(ex)
    return 0, ""


# ---- save ----
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_sharded_save_writes_the_unsharded_engines_bytes(name, world):
    one = _single(name)
    rs, _ = scenario_reads(name)
    cuts = _cuts(rs.n, world)
    d = tempfile.mkdtemp(prefix="hao_sidx_")

    def body(rank, e):
        _build(e, rs, cuts[rank], cuts[rank + 1])
        early = _code(lambda: e.index_save(os.path.join(d, "early")))
        e.dist_gather_reads()
        e.index_save(os.path.join(d, "w"))
        plain = _blob(os.path.join(d, "w"))                                      # (read when THIS rank's call returned)
        e.index_save(os.path.join(d, "w_named"), names=_read_names(rs.n) if rank == 0 else None)
        return early, plain, _blob(os.path.join(d, "w_named"))

    for rank, (early, plain, named) in enumerate(_world(name, world, body)):
        assert early[0] == -4 and "hao_dist_gather_reads" in early[1], (rank, early)      # HAO_EUNSUPP, and the message says what is missing
        for s in SUFFIXES:
            assert plain[s] == one["blob"][s], f"rank {rank}: {s} differs from the unsharded engine's"
            assert named[s] == one["named"][s], f"rank {rank}: {s} with names differs from the unsharded engine's"
    assert not [f for f in os.listdir(d) if f.startswith("early")]              # the refused call created nothing
    assert one["named"][".pt_flt.bin"] != one["blob"][".pt_flt.bin"]


# ---- load ----
def _loaded_state(e, n_local):
    """what a rank reports after a load: layout, tables, thresholds, every local read's lists, every local read's sketch, the digest after a gather"""
    ft, pt, st = e.ft_table(), e.pt_table(), e.stats()
    e.overlap_batch(0, n_local)
    lists = [e.h_ec_lchain(r) for r in range(n_local)]
    e.sketch_batch(0, n_local)
    sk = [e.fetch_sketch(r) for r in range(n_local)]
    e.dist_gather_reads()
    return dict(layout=(e.rid_base, e.n_reads, e.lengths.copy()), ft=ft, pt=pt, st=st, lists=lists, sk=sk, digest=e.reads_digest())


def _check_loaded(name, rank, lo, hi, got, rounds, digest):
    rs, _ = scenario_reads(name)
    g, o = load_golden(name), scenario_oracle(name)
    assert got["rounds"] == rounds
    assert got["layout"][:2] == (lo, hi - lo) and (got["layout"][2] == rs.lengths[lo:hi]).all(), f"rank {rank}: layout"
    keys, vals = got["ft"]
    assert keys.shape == g["ft_keys"].shape and (keys == g["ft_keys"]).all() and (vals == g["ft_vals"]).all(), f"rank {rank}: filter table"
    pk, po, pp = got["pt"]
    assert pk.shape == g["pt_keys"].shape and (pk == g["pt_keys"]).all() and (po == g["pt_off"]).all() and (pp == g["pt_pos"]).all(), f"rank {rank}: position index"
    for key in STATS:
        assert got["st"][key] == g["meta"][key], (rank, key)
    for r in range(lo, hi):
        ol, fc, fo, cl = got["lists"][r - lo]
        ool, ofc, ofo, ocl = o.lchain(r)
        assert ol.shape == ool.shape and (ol == ool).all() and (fc == ofc).all() and cl.shape == ocl.shape and (cl == ocl).all(), f"rank {rank}: read {r}"
        if r % 7 == 0:
            assert (got["sk"][r - lo] == o.sketch(r)).all(), f"rank {rank}: sketch of read {r}"
    assert got["digest"] == digest, f"rank {rank}: the gathered store's digest after the load"


def _load_world(name, world, prefix, cuts, digest, rounds=3):
    """digest: hao_reads_digest of an UNSHARDED engine over the same file"""
    from hifiasm_amd import shard
    rs, _ = scenario_reads(name)
    own = cuts if cuts is not None else [shard.shard_range(rs.n, r, world)[0] for r in range(world)] + [rs.n]

    def body(rank, e):
        got = dict(rounds=e.index_load(prefix, cuts))
        got.update(_loaded_state(e, own[rank + 1] - own[rank]))
        return got

    for rank, got in enumerate(_world(name, world, body)):
        _check_loaded(name, rank, own[rank], own[rank + 1], got, rounds, digest)


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "equal"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_sharded_load_equals_the_build(name, world, ragged):
    rs, _ = scenario_reads(name)
    _load_world(name, world, _single(name)["prefix"], _cuts(rs.n, world) if ragged else None, _single(name)["digest"])


@functools.lru_cache(maxsize=None)
def _reference_file(name):
    """the index the UNMODIFIED reference writes for the scenario (ref_harness --save-index), and the digest of an unsharded engine that loaded it (the
    packed bytes the reads do not define - the base under an N site, the bits behind the last base - are the reference's own there: the digest of the store
    is compared between the two kinds of engine over the SAME file); once"""
    from hifiasm_amd import synth
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads(name)
    d = tempfile.mkdtemp(prefix="hao_sidx_")
    fa = os.path.join(d, "r.fa")
    synth.write_fasta(fa, rs)
    r = subprocess.run([HARNESS, "-t", "2", "--save-index", os.path.join(d, "ref"), fa], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    e = Engine(0, **okw)
    try:
        assert e.index_load(os.path.join(d, "ref")) == 3
        return os.path.join(d, "ref"), e.reads_digest()
    finally:
        e.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["hifi", "nn"])
def test_sharded_load_of_a_reference_written_index(name, world):
    if not os.path.exists(HARNESS):
        pytest.skip("oracle/_ref/ref_harness not built (needs the reference's sources at build time)")
    rs, _ = scenario_reads(name)
    prefix, digest = _reference_file(name)
    _load_world(name, world, prefix, _cuts(rs.n, world), digest)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_round_trip(name, world):
    one = _single(name)
    rs, _ = scenario_reads(name)
    cuts = _cuts(rs.n, world)
    d = tempfile.mkdtemp(prefix="hao_sidx_")

    def body(rank, e):
        e.index_load(one["prefix"], cuts)
        e.dist_gather_reads()
        e.index_save(os.path.join(d, "again"))
        return _blob(os.path.join(d, "again"))

    for rank, blob in enumerate(_world(name, world, body)):
        for s in SUFFIXES:
            assert blob[s] == one["blob"][s], f"rank {rank}: {s}"


# ---- failures ----
@pytest.mark.parametrize("world", [2, 3])
def test_failures_are_every_ranks(world):
    name = "hifi"
    one = _single(name)
    rs, _ = scenario_reads(name)
    o = scenario_oracle(name)
    cuts = _cuts(rs.n, world)
    d = tempfile.mkdtemp(prefix="hao_sidx_")
    # the read store's file: header (44 bytes), per read its N-site count (+ sites), the lengths, then the packed reads - cut in the middle of the last rank's
    n_sites = int(rs.n_mask().sum()) if rs.n_mask() is not None else 0
    pk_start = 44 + 8 * rs.n + 8 * n_sites + 8 * rs.n
    pk_len = (rs.lengths.astype(np.int64) // 4 + 1)
    cut = pk_start + int(pk_len[:cuts[-2]].sum()) + int(pk_len[cuts[-2]:].sum()) // 2
    assert pk_start + int(pk_len.sum()) < len(one["blob"][".pt_flt.bin"])
    for s in SUFFIXES:
        open(os.path.join(d, "cut") + s, "wb").write(one["blob"][s][:cut] if s == ".pt_flt.bin" else one["blob"][s])
    short = cuts[:-1] + [rs.n - 1]

    def body(rank, e):
        seen, lists = [], []

        def good():
            e.index_load(one["prefix"], cuts)
            e.overlap_batch(0, min(4, cuts[rank + 1] - cuts[rank]))
            lists.append(e.h_ec_lchain(0))

        for prefix, c in ((os.path.join(d, "missing") if rank == world - 1 else one["prefix"], cuts), (os.path.join(d, "cut"), cuts), (one["prefix"], short)):
            seen.append(_code(lambda: e.index_load(prefix, c))[0])
            seen.append(_code(lambda: e.overlap_batch(0, 1))[0])                 # no index after a failed load
            good()
        return seen, lists

    for rank, (seen, lists) in enumerate(_world(name, world, body)):
        assert seen[0] != 0 and seen[2] != 0 and seen[4] == -2, (rank, seen)     # (cuts that do not end at the read count: HAO_EINVAL)
        assert seen[1] != 0 and seen[3] != 0 and seen[5] != 0, (rank, seen)
        ool, ofc, _, ocl = o.lchain(cuts[rank])
        for ol, fc, _, cl in lists:
            assert len(lists) == 3 and ol.shape == ool.shape and (ol == ool).all() and (fc == ofc).all() and (cl == ocl).all(), rank


# ---- an unsharded engine ----
def test_unsharded_engine_takes_both_calls():
    from hifiasm_amd.api import Engine, lib
    name = "nn"
    one = _single(name)
    rs, okw = scenario_reads(name)
    o = scenario_oracle(name)

    def state(e):
        e.overlap_batch(0, rs.n)
        return e.ft_table(), e.pt_table(), e.stats(), [e.h_ec_lchain(r) for r in range(0, rs.n, 5)], e.reads_digest()

    def same(a, b):
        flat = lambda s: [x for t in (s[0], s[1]) for x in t] + [x for l in s[3] for x in l]
        return a[2] == b[2] and a[4] == b[4] and all(x.shape == y.shape and (x == y).all() for x, y in zip(flat(a), flat(b)))

    e = Engine(0, **okw)
    try:
        assert e.index_load(one["prefix"]) == 3
        assert (e.n_reads, e.rid_base) == (rs.n, 0) and (e.lengths == rs.lengths).all()
        want = state(e)
        ool = o.lchain(5)[0]
        assert want[3][1][0].shape == ool.shape and (want[3][1][0] == ool).all() and want[4] == one["digest"]
        r = C.c_int32(0)
        assert lib().hao_index_load_dist(e.h, one["prefix"].encode(), None, C.byref(r)) == 0 and r.value == 3      # NULL cuts
        assert same(state(e), want)
        assert e.index_load(one["prefix"], [0, rs.n]) == 3                       # a world of one
        assert same(state(e), want)
        assert _code(lambda: e.index_load(one["prefix"], [0, rs.n - 1]))[0] == -2
        assert _code(lambda: e.overlap_batch(0, 1))[0] != 0
        assert e.index_load(one["prefix"], [0, rs.n]) == 3
        assert same(state(e), want)
    finally:
        e.close()
