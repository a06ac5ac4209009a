"""Tune the table of crafted targets of scenario "cedge" (tests/scenarios.py: CEDGE_TABLE) so that every (Q, target) group of seed hits has EXACTLY the
wanted number of hits - the capacity edges of the chain stage's size classes.  Needs only the oracle (oracle/liboracle.so):
    python tests/golden/make_cedge_table.py            # prints the table as Python literals; paste it into tests/scenarios.py
A target is a substring of the query read Q, possibly rearranged (scenarios.cedge_target); the search trims or extends the substring's end (a base more or
less changes the group by 0 or 1 hits) and, for the inversions with a wanted strand-block boundary, moves the cut.  All targets are tuned together, since
every read of the set enters the k-mer counts that decide which minimizers are indexed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenarios  # noqa: E402
import oracle_py  # noqa: E402

BIG = 3500                     # "around 3500": a group well inside the last class (more than 2048 hits: DP arrays in global scratch)
PLAIN = (1, 8, 9, 63, 64, 65, 127, 128, 129, 192, 256, 257, 512, 513, 2047, 2048, 2049, 2112, BIG)
STRUCT = (8, 9, 64, 65, 128, 129, 256, 257, 512, 513, 2048, 2049, BIG)      # (8: the one-lane pass of the smallest class needs a rejected group too)
BND = ((128, 63), (128, 64), (128, 65), (129, 63), (129, 64), (129, 65))    # inversions: (hits, hits in front of the strand boundary)
PER_HIT = 34.6
QLEN = scenarios.CEDGE_Q[1] - scenarios.CEDGE_Q[0]


def gap_of(hits):
    """bases a `del` target leaves out: beyond the chaining band (2 % of the overlap), or the quick check accepts the group"""
    return 1000 if hits <= 600 else 4000


def wanted():
    w = [("plain", h, None) for h in PLAIN]
    for h in STRUCT:
        w += [("swap", h, None), ("del", h, None), ("inv", h, None)]
    w += [("inv", h, f) for h, f in BND]
    return w


def place(w):
    """starts in Q, longest first, each where the crafted coverage so far is lowest"""
    est = [int(h * PER_HIT) + 80 + (gap_of(h) if s == "del" else 0) for s, h, f in w]
    cov = np.zeros(QLEN, dtype=np.int32)
    start = [0] * len(w)
    for i in sorted(range(len(w)), key=lambda i: -est[i]):
        L = min(est[i] + 2500, QLEN)      # (room to grow)
        cs = np.concatenate([[0], np.cumsum(cov, dtype=np.int64)])
        cand = np.arange(0, QLEN - L + 1, 250)
        cost = cs[cand + L] - cs[cand]
        start[i] = int(cand[int(np.argmin(cost))])
        cov[start[i]:start[i] + est[i]] += 1
    print(f"# crafted coverage of Q: mean {cov.mean():.1f}, max {cov.max()}", file=sys.stderr)
    return start, est


def main():
    w = wanted()
    start, length = place(w)
    cut = [L // 2 for L in length]
    for i, (s, h, f) in enumerate(w):
        if s == "del":
            cut[i] = (length[i] - gap_of(h)) // 2
        if f is not None:
            cut[i] = int(f * PER_HIT) + 40
    step = [16] * len(w); last = [0] * len(w); cstep = [16] * len(w); clast = [0] * len(w); stuck = [0] * len(w)
    for it in range(400):
        table = [(w[i][0], start[i], length[i], cut[i], gap_of(w[i][1]) if w[i][0] == "del" else 0, w[i][1], w[i][2]) for i in range(len(w))]
        rs = scenarios.chain_edge_reads(table)
        o = oracle_py.Oracle(rs.codes, rs.code_off)
        o.ft_gen(); o.pt_gen()
        kh = o.seed_hits(scenarios.CEDGE_QID)
        tid = (kh[:, 0] & 0x7fffffff).astype(np.int64)
        n = np.bincount(tid, minlength=rs.n)
        nf = np.bincount(tid[(kh[:, 0] >> 31) == 0], minlength=rs.n)
        bad = 0
        for i, (s, h, f) in enumerate(w):
            t = scenarios.CEDGE_QID + 1 + i
            if f is not None and int(nf[t]) != f:        # the boundary first: the cut moves it, and with it the total
                e = f - int(nf[t]); bad += 1
                sg = 1 if e > 0 else -1
                if clast[i] and sg != clast[i]:
                    stuck[i] += cstep[i] == 1
                    cstep[i] = max(1, cstep[i] // 2)
                clast[i] = sg
                d = sg * (int(abs(e) * PER_HIT * 0.9) if abs(e) > 1 else cstep[i])
                cut[i] += d; length[i] += d
                continue
            e = h - int(n[t])
            if e == 0:
                continue
            bad += 1
            sg = 1 if e > 0 else -1
            if last[i] and sg != last[i]:
                stuck[i] += step[i] == 1
                step[i] = max(1, step[i] // 2)
            if stuck[i] >= 2:      # this end steps over the wanted count (two minimizers come or go with one base): try another substring
                start[i] = max(0, start[i] - 13); stuck[i] = 0; step[i] = cstep[i] = 8
                print(f"#   target {i} {w[i]} moved to start {start[i]}", file=sys.stderr)
            last[i] = sg
            length[i] += sg * (int(abs(e) * PER_HIT * 0.9) if abs(e) > 1 else step[i])
            length[i] = min(length[i], QLEN - start[i])
            if f is None and s in ("swap", "inv"):
                cut[i] = length[i] // 2
            elif s == "del":
                cut[i] = (length[i] - gap_of(h)) // 2
        st = o.stats()
        print(f"# iteration {it}: {bad} targets off; hom_cov {st['hom_cov']} high_occ {st['high_occ']} reads {rs.n} bases {rs.total_bases}", file=sys.stderr)
        if bad == 0:
            break
    else:
        raise SystemExit("no convergence")
    print("CEDGE_TABLE = [")
    for i, r in enumerate(table):
        t = scenarios.CEDGE_QID + 1 + i
        print(f"    ({r[0]!r}, {r[1]}, {r[2]}, {r[3]}, {r[4]}, {int(n[t])}, {int(nf[t])}),")
    print("]")


if __name__ == "__main__":
    main()
