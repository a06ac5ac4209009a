"""Tasks for the window alignment beyond 127 errors (hao_window_ed_long / hao_window_trace_long; the reference's ed_band_cal_*_infi_* functions with nword = 5 .. 64):
deterministic, few and small.  Every segment size of the cooperative kernel occurs at both of its edges - nword 5, 8 | 9, 16 | 17, 32 | 33, 64 - and the wide band
has to DECIDE: a text window of an overlap is paired with a target interval displaced along the overlap's diagonal by d in 0 .. thre + thre / 4, so the optimum
leaves the 255 diagonals of the register-resident kernels, or fails by a little.
  semi-global (distance-only and traced): the pattern is about as long as the text and starts d bases before the text's partner, so it ends d bases early: err ~ d
  global: both ends are off by d / 2: err ~ d                       extension: the common start (end) is off by d: err ~ d
plus unrelated pairs, and two pairs at the upper end (thre 2047, the text most of the set's longest read, displaced against itself) that are traced through the
sliced second sweep.  tests/golden/make_golden_ed_long.py runs the reference on them and asserts the mix (share of err >= 128, share without an alignment, an
aligned err >= 128 for every nword above) on the reference's own results.  Same records as helpers.ed_tasks: uint32 [n, 10]."""
import numpy as np

from helpers import scenario_reads, scenario_oracle

THRE = (130, 159, 255, 256, 511, 512, 1023, 1024, 2047, 200, 700, 1500)      # the first nine: nword 5, 5, 8, 9, 16, 17, 32, 33, 64
NWORD_EDGES = (5, 8, 9, 16, 17, 32, 33, 64)
N_PAIRS = 132        # overlap pairs per list (eleven per threshold)
N_UNRELATED = 24
N_BIG = 2            # the last rows of a list made with big=True
SEEDS = {"": 11, "g": 12, "s": 13, "x": 14}      # distance-only, global, semi-global traced, extension (forward and backward)


def nword_of(thre):
    return (2 * np.asarray(thre, dtype=np.int64) + 64) // 64


def _displacement(rng, thre):
    """0 .. thre + thre / 4; narrow bands lean towards their upper end (only there can they reach 128 errors)"""
    lo = 0.8 if thre < 300 else 0.0 if rng.integers(0, 3) == 0 else 0.3
    return int(rng.uniform(lo, 1.25) * thre)


def _pair(key, rng, thre, tn, dp, tl):
    """pattern interval (p0, pn, abs_diag) on the target strand for a text of tn bases whose first base's partner is target position dp; None = does not fit"""
    d = _displacement(rng, thre)
    ad = 0
    if key in ("", "s"):
        p0 = dp - d
        pn = tn + int(rng.integers(0, thre // 8 + 1))
        if p0 < 0:
            ad, p0 = -p0, 0
            pn -= ad
        pn = min(pn, tl - p0)
        ai = pn - tn + ad
        if ad > 2 * thre or pn <= 0 or ai < 0 or ai > 2 * thre or tn <= ad:      # (the traced call's domain; the distance-only list keeps to it too)
            return None
    elif key == "g":
        p0 = dp - d // 2
        pn = tn + int(rng.integers(-3, 4))
        if p0 < 0 or p0 + pn > tl or pn <= 0:
            return None
    else:
        p0 = dp + (d if rng.integers(0, 2) else -d)
        pn = tn + int(rng.choice([-60, -9, 0, 0, 0, 3, 80]))
        if p0 < 0 or p0 + pn > tl or pn <= 0:
            return None
    return p0, pn, ad


def edl_tasks(name, key, big=False):
    """key: "" distance-only, "g" global, "s" semi-global traced, "x" extension; big: + the two upper-end pairs (last rows)"""
    rs, okw = scenario_reads(name)
    o = scenario_oracle(name)
    rng = np.random.default_rng(SEEDS[key])
    L = rs.lengths.astype(np.int64)
    out = []
    order = rng.permutation(rs.n)
    q = 0
    while len(out) < N_PAIRS:
        r = int(order[q % rs.n]); q += 1
        assert q < 50 * rs.n, "no overlaps to draw from"
        ol = o.lchain(r)[0]
        if ol.shape[0] == 0:
            continue
        z = ol[int(rng.integers(0, ol.shape[0]))]
        xs, xe, yid, ys, yrev = int(z[1]), int(z[2]), int(z[4]), int(z[5]), int(z[7])
        thre = THRE[len(out) % len(THRE)]
        tn = min(int(rng.integers(300, 2001)), xe + 1 - xs)
        if tn < 250:
            continue
        ws = xs + int(rng.integers(0, xe + 2 - xs - tn))
        pr = _pair(key, rng, thre, tn, ys + (ws - xs), int(L[yid]))
        if pr is None:
            continue
        out.append((yid, pr[0], pr[1], yrev, r, ws, tn, 0, thre, pr[2]))
    for _ in range(N_UNRELATED):      # unrelated strings, either strand
        a, b = (int(x) for x in rng.integers(0, rs.n, 2))
        thre = int(rng.choice(THRE))
        tn = int(rng.integers(300, min(1500, int(L[b])) + 1))
        pn = tn + (int(rng.integers(0, thre + 1)) if key in ("", "s") else int(rng.integers(-3, 4)))
        pn = max(1, min(pn, int(L[a])))
        if key in ("", "s") and pn < tn:
            continue
        out.append((a, int(rng.integers(0, L[a] - pn + 1)), pn, int(rng.integers(0, 2)), b, int(rng.integers(0, L[b] - tn + 1)), tn, int(rng.integers(0, 2)), thre, 0))
    if big:
        a = int(np.argmax(L))
        for d in (600, 900):      # the longest read against itself, d bases on: err = d (global: 2 d) exactly
            tn = int(L[a]) - d
            if key == "g":
                out.append((a, 0, tn - d, 0, a, d, tn - d, 0, 2047, 0))
            else:
                out.append((a, 0, tn, 0, a, d, tn, 0, 2047, 0))
    return np.array(out, dtype=np.uint32)
