"""Scenario "cedge" (scenarios.chain_edge_reads) holds what its table says: for the query read Q the oracle's groups of seed hits - the hits of one target id, both
strands - have exactly the committed sizes, every capacity edge of the chain stage's size classes is there in plain form, and every rearranged target at its size.
CPU only; tests/test_gpu_chain_classes.py runs the set through the engine."""
import numpy as np

from helpers import scenario_reads, scenario_oracle
from scenarios import CEDGE_QID, CEDGE_TABLE, CEDGE_Q, cedge_class

PLAIN = (1, 8, 9, 63, 64, 65, 127, 128, 129, 192, 256, 257, 512, 513, 2047, 2048, 2049, 2112)
STRUCT = (9, 64, 65, 128, 129, 256, 257, 512, 513, 2048, 2049)
BIG = (3000, 4000)      # "one around 3500"


def _sizes():
    o = scenario_oracle("cedge")
    kh = o.seed_hits(CEDGE_QID)
    tid = (kh[:, 0] & 0x7fffffff).astype(np.int64)
    return np.bincount(tid, minlength=o.n_reads), np.bincount(tid[(kh[:, 0] >> 31) == 0], minlength=o.n_reads)


def test_group_sizes_equal_the_table():
    rs, _ = scenario_reads("cedge")
    assert rs.n == CEDGE_QID + 1 + len(CEDGE_TABLE) and int(rs.lengths[CEDGE_QID]) == CEDGE_Q[1] - CEDGE_Q[0]
    n, nf = _sizes()
    got = [(int(n[CEDGE_QID + 1 + i]), int(nf[CEDGE_QID + 1 + i])) for i in range(len(CEDGE_TABLE))]
    want = [(row[5], row[6]) for row in CEDGE_TABLE]
    assert got == want, "the set drifted: re-tune the table (tests/golden/make_cedge_table.py): " + str([(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])


def test_every_edge_in_plain_form():
    have = {row[5] for row in CEDGE_TABLE if row[0] == "plain"}
    assert set(PLAIN) <= have, sorted(set(PLAIN) - have)
    big = [h for h in have if BIG[0] <= h <= BIG[1]]
    assert len(big) == 1
    assert {cedge_class(h) for h in have} == set(range(7))
    for row in CEDGE_TABLE:      # a plain target is a substring of Q: all of its hits on the forward strand
        if row[0] == "plain":
            assert row[6] == row[5] and row[1] + row[2] <= CEDGE_Q[1] - CEDGE_Q[0]


def test_every_rearranged_target_at_its_size():
    big = [row[5] for row in CEDGE_TABLE if row[0] == "plain" and BIG[0] <= row[5] <= BIG[1]]
    for shape in ("swap", "del", "inv"):
        have = {row[5] for row in CEDGE_TABLE if row[0] == shape}
        assert set(STRUCT) | set(big) <= have, (shape, sorted((set(STRUCT) | set(big)) - have))
        assert {cedge_class(h) for h in have} == set(range(7)), shape      # (8 hits: a rejected group for the smallest class too)
    for row in CEDGE_TABLE:
        shape, start, length, cut, gap, hits, fwd = row
        assert 0 < cut < length - gap or shape == "plain"
        if shape == "inv":
            assert 0 < fwd < hits      # two strand blocks
        else:
            assert fwd == hits
        if shape == "del":             # beyond the chaining band (2 % of the overlap), or the quick check would accept the group
            assert gap > 0.02 * (length - gap) + 16
    bnd = {(row[5], row[6]) for row in CEDGE_TABLE if row[0] == "inv"}      # the strand boundary on the last lane of the first 64-hit tile, on the first of the second, and one further
    assert {(h, f) for h in (128, 129) for f in (63, 64, 65)} <= bnd
