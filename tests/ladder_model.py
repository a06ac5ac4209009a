"""The threshold ladder of hc_aln_exz (Correct.cpp:14576-14636), restated in plain Python from the reference's own lines - independent of hao_ladder.cuh, which the
tests hold against it:

  scale_ed_thre           Correct.cpp:14354-14360 (uint32 arithmetic, bitw = 6)
  the rungs               :14599-14631: scale_ed_thre(estimate_err), ql * e_rate, twice that, ql * 0.51 - each through scale_ed_thre(., maxe), capped at ql, skipped
                          unless larger than the threshold before (thre0 is the threshold COMPUTED before, attempted or not)
  cal_exz_infi            :14508-14574: update_semi_coord (:14364-14380: y_start_offset + init_waln, tests/refgrid_model.py) in mode 3, adjust_ext_offset
                          (:14400-14422) in modes 1 / 2, the test qe > qs && te > ts, the traced alignment, is_align
  ts == te == -1          forces mode 3 (:14582)

The aligner is pluggable: aligner(mode, task) -> (err, ps, pe, ts, te, cigar tuple), task = the ten fields of hao_ed_task_t (pattern = target stretch, text =
query stretch).  A record is LADDER_RES's fields in order; the conventions where the reference has no value are include/hao.h's (rung 0, the two flags)."""
import numpy as np

import refgrid_model as M

NOALN = 2**31 - 1
REFUSED, UNTRACED = 1, 2
MAX_THRE, MAX_LEN = 2047, 16383
FIELDS = ("rung", "thre", "qs", "qe", "ts", "te", "aux_beg", "flags", "err", "a_ps", "a_pe", "a_ts", "a_te", "n_cigar")


def scale_ed_thre(err, max_err):
    err &= 0xFFFFFFFF; max_err &= 0xFFFFFFFF
    bd = ((err << 1) + 1) & 0xFFFFFFFF
    w = (bd >> 6) << 6
    if w < bd:
        w += 64
    err = ((w - 1) >> 1) & 0xFFFFFFFF
    return min(err, max_err)


def rungs(ql, estimate_err, e_rate, maxl, maxe):
    """-> [thre of rung 1 .. 4], -1 where the rung is skipped or the gate is shut"""
    out = [-1, -1, -1, -1]
    if not (ql <= maxl and estimate_err * 1.2 <= maxe):
        return out
    thre = min(scale_ed_thre(estimate_err, maxe), ql)
    out[0] = thre
    for k, f in ((1, lambda t: int(ql * e_rate)), (2, lambda t: t << 1), (3, lambda t: int(ql * 0.51))):
        thre0 = thre
        thre = min(scale_ed_thre(f(thre), maxe), ql)
        if thre > thre0:
            out[k] = thre
    return out


def nword(thre):
    return (2 * thre + 1 + 63) >> 6


def adjust_ext_offset(qs, qe, ts, te, ql, tl, thre, mode):
    if mode == 1:
        qoff, toff = ql - qs, tl - ts
        if qoff <= toff:
            qe = ql; te = ts + qoff + thre; branch = 0
        else:
            te = tl; qe = qs + toff + thre; branch = 1
    else:
        qoff, toff = qe, te
        if qoff <= toff:
            qs = 0; ts = te - qoff - thre; branch = 0
        else:
            ts = 0; qs = qe - toff - thre; branch = 1
    clip = set()
    if qs < 0:
        qs = 0; clip.add("q0")
    if ts < 0:
        ts = 0; clip.add("t0")
    if qe > ql:
        qe = ql; clip.add("qend")
    if te > tl:
        te = tl; clip.add("tend")
    return qs, qe, ts, te, branch, clip


def semi_domain(p_len, t_len, abs_diag, thre):
    ai = p_len - t_len + abs_diag
    return 0 <= ai <= 2 * thre and t_len > abs_diag and abs_diag <= 2 * thre


def attempt(z, fc, lengths, req, mode, thre, ev=None):
    """cal_exz_infi's coordinate step -> (task or None, flags, (qs, qe, ts, te, aux_beg))"""
    xid, xs, yid, ys, yrev = int(z[0]), int(z[1]), int(z[4]), int(z[5]), int(z[7])
    q_tot, t_tot = int(lengths[xid]), int(lengths[yid])
    _, _, qs, qe, ts, te, _ = req
    aux, fl = 0, 0
    if mode == 3:
        sh = M.y_start_offset(qs, fc)
        if sh is M.UNRESOLVED or sh > 32767 or sh <= -32768:
            return None, UNTRACED, (qs, qe, -1, -1, -1)
        r = M.init_waln(thre, (qs - xs) + ys + sh, t_tot, (qe - qs) + (thre << 1))
        if r is None:
            if ev is not None:
                ev.add("init_waln_refusal")
            return None, REFUSED, (qs, qe, -1, -1, -1)
        aux, _, ts, rl = r
        te = ts + rl
    elif mode in (1, 2):
        qs, qe, ts, te, branch, clip = adjust_ext_offset(qs, qe, ts, te, q_tot, t_tot, thre, mode)
        if ev is not None:
            ev.add(f"ext{mode}_branch{branch}")
            for c in clip:
                ev.add("clip_" + c)
    co = (qs, qe, ts, te, aux)
    if not (qe > qs and te > ts and ts != -1 and te != -1):
        return None, REFUSED, co
    if mode == 3 and not semi_domain(te - ts, qe - qs, aux, thre):
        return None, UNTRACED, co
    assert 0 <= qs and qe <= q_tot and 0 <= ts and te <= t_tot
    return (yid, ts, te - ts, yrev, xid, qs, qe - qs, 0, thre, aux), 0, co


def check_request(z, lengths, req, e_rate, maxl, maxe):
    """the refusals of hao_window_ladder for one request (True: HAO_EINVAL)"""
    _, mode, qs, qe, ts, te, est = req
    if mode not in (0, 1, 2, 3) or not 0 <= est < 2**30:
        return True
    if ts == -1 and te == -1:
        mode = 3
    q_tot, t_tot = int(lengths[int(z[0])]), int(lengths[int(z[4])])
    if not 0 <= qs <= qe <= q_tot or (mode != 3 and not 0 <= ts <= te <= t_tot):
        return True
    ql = qe - qs
    th = [t for t in rungs(ql, est, e_rate, maxl, maxe) if t >= 0]
    if th and ql > MAX_LEN:
        return True
    for t in th:
        if mode == 3:
            if ql + 2 * t > MAX_LEN:
                return True
        else:
            a = adjust_ext_offset(qs, qe, ts, te, q_tot, t_tot, t, mode) if mode else (qs, qe, ts, te)
            if a[1] - a[0] > MAX_LEN or a[3] - a[2] > MAX_LEN:
                return True
    return False


def ladder(z, fc, lengths, req, e_rate, maxl, maxe, aligner, ev=None):
    """one request (ol, mode, qs, qe, ts, te, estimate_err) over overlap z (12 uint32) and its fake cigar -> (record in FIELDS' order, cigar tuple).  ev: a set that
    collects what the request met (the fixture's categories)"""
    _, mode, qs, qe, ts, te, est = (int(x) for x in req)
    forced = ts == -1 and te == -1
    if forced:
        mode = 3
    ql = qe - qs
    th = rungs(ql, est, e_rate, maxl, maxe)
    rec0 = [0, 0, qs, qe, -1 if mode == 3 else ts, -1 if mode == 3 else te, 0]
    flags = 0
    if ev is not None:
        ev.add(f"mode{mode}")
        if all(t < 0 for t in th):
            ev.add("gate_maxl" if ql > maxl else "gate_maxe")
        elif any(t < 0 for t in th):
            ev.add("rung_skipped")
    for k, thre in enumerate(th):
        if thre < 0:
            continue
        if ev is not None and thre == ql:
            ev.add("capped_at_ql")
        task, fl, co = attempt(z, fc, lengths, (0, mode, qs, qe, ts, te, est), mode, thre, ev)
        flags |= fl
        if task is None:
            continue
        if ev is not None:
            w = nword(thre)
            ev.add("nword_1" if w == 1 else "nword_2" if w == 2 else "nword_3_4" if w <= 4 else "nword_5_8" if w <= 8 else "nword_9plus")
            ev.add(f"mode{mode}_nword_" + ("1" if w == 1 else "2" if w == 2 else "3_4" if w <= 4 else "5_8" if w <= 8 else "9_16" if w <= 16 else "17_32" if w <= 32 else "33_64"))
        err, ps, pe, a_ts, a_te, cig = aligner(mode, task)
        if err <= thre:      # is_align
            if ev is not None:
                ev.add(f"rung{k + 1}")
            return tuple([k + 1, thre] + list(co) + [flags, err, ps, pe, a_ts, a_te, len(cig)]), tuple(cig)
    if ev is not None and any(t >= 0 for t in th):
        ev.add("no_success")
    return tuple(rec0 + [flags, NOALN, -1, -1, -1, -1, 0]), ()


def oracle_aligner(o):
    """the oracle restatement's traced alignments (hao_or_window_trace) as an aligner"""
    def f(mode, task):
        r, c = o.window_trace(np.array([task], dtype=np.int64).astype(np.uint32), cap=2 * task[8] + 8, mode=mode)
        n = int(r[0, 5])
        return int(r[0, 0]), int(r[0, 1]), int(r[0, 2]), int(r[0, 3]), int(r[0, 4]), tuple(int(x) for x in c[0, :n])
    return f


def records(recs):
    """list of record tuples -> structured array with LADDER_RES's fields (int64)"""
    a = np.array(recs, dtype=np.int64).reshape(-1, len(FIELDS))
    return a
