"""The threshold ladder of hc_aln_exz_adv (Correct.cpp:16082-16165), restated in plain Python from the reference's own lines - independent of hao_ladder.cuh, which
the tests hold against it.  It reuses tests/ladder_model.py's coordinate functions (scale_ed_thre, adjust_ext_offset, y_start_offset, init_waln, the semi-global
domain) and differs from that model's ladder where the reference does:

  entry                   :16087-16091: ts == te == -1 forces mode 3; ql == 0 && te - ts == 0 returns 1; ql <= 0 || te - ts <= 0 returns 0 - on the request's own ts / te
  estimate_err < 0        :16092-16095: ql * e_rate (truncated) when ql <= wl; the other branch (cal_estimate_err) is not built: check_request refuses it
  exact shortcut          :16100-16107 / cal_exact_exz :15725-15767, ql <= 16: the mode's target interval, clamped to [0, t_tot]; tl == ql and equal bases (memcmp over
                          the strings of recover_UC_Read_sub_region, Process_Read.cpp:524-615, which writes 'N' at the N sites of either strand: N equals N only)
  gate                    :16109: ql <= maxl and (estimate_err >> 1) <= maxe
  rungs                   :16110-16156: no cap at ql; thre > thre0 for rungs 2 - 4 (thre0: the RAW threshold computed before); a fifth rung thre = maxe when ql <= force_l
  cal_exz_infi_adv        :15617-15672: dd = max(ql, tl) of the request, the coordinate step with min(thre, dd), the test, dd of the new lengths, thre = min(thre, dd),
                          abandoned if thre <= pthre, else pthre = thre and the traced alignment in that band; absolute coordinates on success (:15665-15666)

The aligner is ladder_model's: aligner(mode, task) -> (err, ps, pe, ts, te, cigar tuple).  bases(rid, pos, n, rev) -> the codes (0 - 3, 4 = N) of n bases from `pos`
of strand `rev` of read `rid`.  A record is LADDER_ADV_RES's fields in order."""
import ladder_model as LM
import refgrid_model as M

NOALN = LM.NOALN
REFUSED, UNTRACED, REPEAT = 1, 2, 4
RUNG_EXACT = 6
FIELDS = ("done",) + LM.FIELDS


def estimate(ql, est, e_rate, wl):
    """-> the estimate the ladder runs with, or None where the reference would call cal_estimate_err"""
    if est >= 0:
        return est
    return int(ql * e_rate) if ql <= wl else None


def rungs(ql, est, e_rate, maxl, maxe, force_l):
    """-> [raw thre of rung 1 .. 5], -1 where the rung is skipped or the gate is shut (est: already estimated)"""
    out = [-1] * 5
    if not (ql <= maxl and (est >> 1) <= maxe):
        return out
    thre = LM.scale_ed_thre(est, maxe)
    out[0] = thre
    for k, f in ((1, lambda t: int(ql * e_rate)), (2, lambda t: t << 1), (3, lambda t: int(ql * 0.51))):
        thre0 = thre
        thre = LM.scale_ed_thre(f(thre), maxe)
        if thre > thre0:
            out[k] = thre
    if ql <= force_l:
        out[4] = maxe
    return out


def reads_bases(rs):
    """bases() over a read set's codes"""
    def f(rid, pos, n, rev):
        lo = int(rs.code_off[rid]); L = int(rs.lengths[rid])
        if not rev:
            return [int(c) for c in rs.codes[lo + pos:lo + pos + n]]
        return [int(c) if c > 3 else 3 - int(c) for c in rs.codes[lo + L - pos - n:lo + L - pos][::-1]]
    return f


def exact(z, fc, lengths, req, mode, bases, ev=None):
    """cal_exact_exz -> (hit, flags, (qs, qe, ts, te))"""
    xid, xs, yid, ys, yrev = int(z[0]), int(z[1]), int(z[4]), int(z[5]), int(z[7])
    t_tot = int(lengths[yid])
    _, _, qs, qe, ts, te, _ = req
    ql = qe - qs
    if mode == 3:
        sh = M.y_start_offset(qs, fc)
        if sh is M.UNRESOLVED or sh > 32767 or sh <= -32768:
            return False, UNTRACED, None
        ts = (qs - xs) + ys + sh; te = ts + ql
    elif mode == 1:
        te = ts + ql
    elif mode == 2:
        ts = te - ql
    ts = min(max(ts, 0), t_tot); te = min(te, t_tot)
    if te - ts != ql:
        if ev is not None:
            ev.add("exact_tl_ne_ql")
        return False, 0, None
    if bases(xid, qs, ql, 0) != bases(yid, ts, ql, yrev):
        if ev is not None:
            ev.add("exact_mismatch")
        return False, 0, None
    if ev is not None:
        ev.add("exact"); ev.add("exact_rev" if yrev else "exact_fwd")
    return True, 0, (qs, qe, ts, te)


def attempt(z, fc, lengths, req, mode, raw, pthre, ev=None):
    """cal_exz_infi_adv up to the aligner -> (task or None, flags, (qs, qe, ts, te, aux_beg), clamped thre, new pthre)"""
    xid, xs, yid, ys, yrev = int(z[0]), int(z[1]), int(z[4]), int(z[5]), int(z[7])
    q_tot, t_tot = int(lengths[xid]), int(lengths[yid])
    _, _, qs, qe, ts, te, _ = req
    dd = max(qe - qs, te - ts)
    thre = min(raw, dd)
    if ev is not None and raw > dd:
        ev.add("clamped_by_dd")
    aux = 0
    if mode == 3:
        sh = M.y_start_offset(qs, fc)
        if sh is M.UNRESOLVED or sh > 32767 or sh <= -32768:
            return None, UNTRACED, (qs, qe, -1, -1, -1), thre, pthre
        r = M.init_waln(thre, (qs - xs) + ys + sh, t_tot, (qe - qs) + (thre << 1))
        if r is None:
            if ev is not None:
                ev.add("init_waln_refusal")
            return None, REFUSED, (qs, qe, -1, -1, -1), thre, pthre
        aux, _, ts, rl = r
        te = ts + rl
    elif mode in (1, 2):
        qs, qe, ts, te, _, _ = LM.adjust_ext_offset(qs, qe, ts, te, q_tot, t_tot, thre, mode)
    co = (qs, qe, ts, te, aux)
    if not (qe > qs and te > ts and ts != -1 and te != -1):
        return None, REFUSED, co, thre, pthre
    thre = min(raw, max(qe - qs, te - ts))
    if thre <= pthre:
        if ev is not None:
            ev.add("pthre_abandoned")
        return None, REPEAT, co, thre, pthre
    pthre = thre
    if mode == 3 and not LM.semi_domain(te - ts, qe - qs, aux, thre):
        return None, UNTRACED, co, thre, pthre
    assert 0 <= qs and qe <= q_tot and 0 <= ts and te <= t_tot
    if ev is not None and thre > qe - qs and te - ts > qe - qs:
        ev.add("thre_above_ql")
    return (yid, ts, te - ts, yrev, xid, qs, qe - qs, 0, thre, aux), 0, co, thre, pthre


def check_request(z, lengths, req, e_rate, wl, maxl, maxe, force_l):
    """the refusals of hao_window_ladder_adv for one request (True: HAO_EINVAL)"""
    _, mode, qs, qe, ts, te, est = req
    if mode not in (0, 1, 2, 3) or est >= 2**30:
        return True
    if ts == -1 and te == -1:
        mode = 3
    q_tot, t_tot = int(lengths[int(z[0])]), int(lengths[int(z[4])])
    if not 0 <= qs <= qe <= q_tot:
        return True
    ql, tl = qe - qs, te - ts
    if ql <= 0 or tl <= 0:
        return False      # (an early return)
    if ts < 0 or te > t_tot:
        return True
    est = estimate(ql, est, e_rate, wl)
    if est is None:
        return True
    th = [t for t in rungs(ql, est, e_rate, maxl, maxe, force_l) if t >= 0]
    if th and ql > LM.MAX_LEN:
        return True
    for t in th:
        t = min(t, max(ql, tl))
        if mode == 3:
            if ql + 2 * t > LM.MAX_LEN:
                return True
        else:
            a = LM.adjust_ext_offset(qs, qe, ts, te, q_tot, t_tot, t, mode) if mode else (qs, qe, ts, te)
            if a[1] - a[0] > LM.MAX_LEN or a[3] - a[2] > LM.MAX_LEN:
                return True
    return False


def ladder(z, fc, lengths, req, e_rate, wl, maxl, maxe, force_l, aligner, bases, ev=None, att=None):
    """one request (ol, mode, qs, qe, ts, te, estimate_err) over overlap z (12 uint32) and its fake cigar -> (record in FIELDS' order, cigar tuple).  ev: a set that
    collects what the request met (the fixture's categories); att: a list that receives the attempts the request made - the rounds it was open in"""
    _, mode, qs, qe, ts, te, est = (int(x) for x in req)
    forced = ts == -1 and te == -1
    if forced:
        mode = 3
    ql, tl = qe - qs, te - ts
    none = lambda done, flags: (tuple([done, 0, 0, qs, qe, ts, te, 0, flags, NOALN, -1, -1, -1, -1, 0]), ())
    if ql == 0 and tl == 0:
        if ev is not None:
            ev.add("early_1")
        return none(1, 0)
    if ql <= 0 or tl <= 0:
        if ev is not None:
            ev.add("early_0_forced" if forced else "early_0_unset_end" if mode in (1, 2) else "early_0")
        return none(0, 0)
    if ev is not None:
        ev.add(f"mode{mode}")
        if est < 0:
            ev.add("estimated")
    est = estimate(ql, est, e_rate, wl)
    assert est is not None
    flags = 0
    if att is not None:
        att.append(0)
    r = (0, mode, qs, qe, ts, te, est)
    if ql <= 16:
        hit, fl, co = exact(z, fc, lengths, r, mode, bases, ev)
        flags |= fl
        if hit:
            return tuple([1, RUNG_EXACT, 0, co[0], co[1], co[2], co[3], 0, flags, 0, co[2], co[3] - 1, co[0], co[1] - 1, 1]), (ql,)
    th = rungs(ql, est, e_rate, maxl, maxe, force_l)
    if ev is not None:
        if all(t < 0 for t in th):
            ev.add("gate_maxl" if ql > maxl else "gate_est")
        elif any(t < 0 for t in th[1:4]):
            ev.add("rung_skipped")
    pthre, n_att = -1, 0
    for k, raw in enumerate(th):
        if raw < 0:
            continue
        n_att += 1
        if att is not None:
            att[-1:] = [n_att]
        task, fl, co, thre, pthre = attempt(z, fc, lengths, r, mode, raw, pthre, ev)
        flags |= fl
        if task is None:
            continue
        if ev is not None:
            w = LM.nword(thre)
            ev.add("nword_1" if w == 1 else "nword_2" if w == 2 else "nword_3_4" if w <= 4 else "nword_5_8" if w <= 8 else "nword_9plus")
        err, ps, pe, a_ts, a_te, cig = aligner(mode, task)
        if err <= thre:      # is_align
            if ev is not None:
                ev.add(f"rung{k + 1}")
                if mode == 3 and not forced:
                    ev.add("mode3_explicit_aligned")
            return tuple([1, k + 1, thre] + list(co) + [flags, err, ps + co[2], pe + co[2], a_ts + co[0], a_te + co[0], len(cig)]), tuple(cig)
    if ev is not None and any(t >= 0 for t in th):
        ev.add("no_success")
    return none(0, flags)
