"""The second half of align_hc_ed_post_extz (Correct.cpp:12951-13012), restated in plain Python from the reference's own lines - independent of hao_rescue_pair
and of the device's state machine (hifiasm_amd/csrc/hao_rescue.cuh), which the rescue tests are held against:

  the rescue at an aligned window   push_hc_wlst_exz (Correct.cpp:12776-12836)
  one rescue alignment              aln_wlst_adv_exz (:4057-4131): double_error_threshold(get_init_err_thres(ql, e_rate, w_l, 31), ql) (:917, :1042), init_waln,
                                    the refusal t_pri_l + thres < ql, distance-only forwards (ps forced to 0), traced backwards
  the anchor's trace                gen_backtrace_adv_exz (:12563-12639): the traced function entered with the primary (err, pe) preset - its err == 0 shortcut
                                    gives ps = pe - (ql - 1); otherwise its search (Levenshtein_distance.h:3832-3849) is skipped and the walk starts from the preset
                                    pe, which is what the same search gave the distance-only function on the same task, so a cleared entry yields the same
                                    (err, ps, pe): the model calls the cleared function and asserts (err, pe) against the primary result
  the re-placement                  recal_boundary_exz (:2429-2468)
  the exit test and the verdict     pass_qovlp (:12773) after every aligned window and at the end

The alignments themselves come from a callback, align(task, traced) -> (err, ps, pe) (err NOALN: none; ps ignored when not traced), so the same control flow
runs over the oracle or over recorded results.  A traced alignment outside the domain in which the reference's traced function stays inside its band word
(0 <= p_len - t_len + abs_diag <= 2 thre, t_len > abs_diag) is not made: the backward run ends there and the overlap is flagged UNTRACED."""
import numpy as np

import refgrid_model as M

NOALN = 2**31 - 1
FWD, BWD, ANCHOR = 0, 1, 2
UNTRACED = 1
NO_EXIT = 0xFFFFFFFF


def rescue_threshold(ql, wl, e_rate):
    t = M.THRESHOLD_MAX_SIZE if ql >= wl else M.threshold(ql, e_rate)      # get_init_err_thres(ql, e_rate, w_l, THRESHOLD_MAX_SIZE)
    if t == 0 and ql >= 4:                                                   # double_error_threshold
        t = 1
    t *= 2
    if ql >= 300 and t < M.THRESHOLD_MAX_SIZE:
        t = M.THRESHOLD_MAX_SIZE
    return min(t, M.THRESHOLD_MAX_SIZE)


def pass_qovlp(o, a, r=0.9):
    return a > 0 and o * r <= a


def traced_domain(task):
    p_len, t_len, thre, ab = int(task[2]), int(task[6]), int(task[8]), int(task[9])
    ai = p_len - t_len + ab
    return 0 <= ai <= 2 * thre and t_len > ab and ab <= 2 * thre


class _Untraced(Exception):
    pass


def _recal(task, l, ps, pe, err, align, log):
    """recal_boundary_exz after a traced alignment (err, ps, pe) of task -> (task, err, ps, pe) re-placed, or None"""
    yid, r_s, r_l, yrev, xid, q_s, ql, _, thres, _ = [int(x) for x in task]
    if ps == 0:
        ts = r_s
    elif pe + 1 == r_l:
        ts = r_s + pe - ql + 1
    else:
        return None
    r = M.init_waln(thres, ts, l, ql + 2 * thres)
    if r is None:
        return None
    aux_beg, _, n_s, n_l = r
    if n_s == r_s and n_l == r_l:
        return None
    t2 = (yid, n_s, n_l, yrev, xid, q_s, ql, 0, thres, aux_beg)
    if not traced_domain(t2):
        raise _Untraced()
    log.append(("recal", t2))
    e2, ps2, pe2 = align(t2, True)
    if e2 != NOALN and e2 < err:
        return t2, e2, ps2, pe2
    return None


def _aln_wlst(z, l, wl, e_rate, w, q_s, q_e, t_s, is_cigar, align, log, flags):
    """aln_wlst_adv_exz -> None or the window record [win, y_start, y_end, err, thre, dir, re-placed]"""
    ql = q_e + 1 - q_s
    thres = rescue_threshold(ql, wl, e_rate)
    r = M.init_waln(thres, t_s, l, ql + 2 * thres)
    if r is None:
        return None
    aux_beg, _, r_s, r_l = r
    if r_l + thres < ql:
        return None
    task = (int(z[4]), r_s, r_l, int(z[7]), int(z[0]), q_s, ql, 0, thres, aux_beg)
    if is_cigar and not traced_domain(task):
        flags[0] |= UNTRACED
        return None
    log.append(("bwd" if is_cigar else "fwd", task, w, t_s))
    err, ps, pe = align(task, bool(is_cigar))
    if not is_cigar:
        ps = 0
    if err == NOALN:
        return None
    replaced = 0
    if is_cigar and (pe + 1 == r_l or ps == 0) and err > 0:
        try:
            rr = _recal(task, l, ps, pe, err, align, log)
        except _Untraced:
            flags[0] |= UNTRACED; rr = None
        if rr is not None:
            task, err, ps, pe = rr; r_s = task[1]; replaced = 1
    return [w, r_s + ps, r_s + pe, err, thres, BWD if is_cigar else FWD, replaced]


def rescue_overlap(z, lengths, wl, e_rate, prim, align):
    """z: hao_ovlp_t as 12 uint32; prim: {grid window: (task, err, pe)} of the windows the primary pass admitted.  -> dict(verdict, flags, exit_win, align_length,
    n_rescued, events, wins (int64 [m, 7] in window order: win, y_start, y_end, err, thre, direction, re-placed), log (every alignment asked for, in order))"""
    xs, xe, l = int(z[1]), int(z[2]), int(lengths[int(z[4])])
    wins = M.windows(xs, xe, wl)
    ovl = xe + 1 - xs
    w_list, recs, log, flags, ev = [], [], [], [0], set()      # w_list entries: [slot, y_start, y_end]; ev: what happened (the fixture's and the tests' categories)
    align_length, exit_win = 0, NO_EXIT
    for idx, (w, q_s, q_e) in enumerate(wins):
        p = prim.get(w)
        if p is None or int(p[1]) == NOALN:
            continue
        task, err, pe = p[0], int(p[1]), int(p[2])
        r_s, r_l, ql = int(task[1]), int(task[2]), q_e + 1 - q_s
        y_start, y_end = r_s, r_s + pe
        cs = 0
        if w_list:                                   # forward, from the end of the previous window
            j, toff = w_list[-1][0] + 1, w_list[-1][2] + 1
            if j < idx:
                ev.add("gap")
            while j < idx and toff < l:
                wj, ws, we = wins[j]
                r = _aln_wlst(z, l, wl, e_rate, wj, ws, we, toff, 0, align, log, flags)
                if r is None:
                    ev.add("forward_failed"); break
                recs.append(r); w_list.append([j, r[1], r[2]]); align_length += we + 1 - ws; ev.add("forward")
                toff = r[2] + 1; j += 1
            cs = w_list[-1][0] + 1
        a_n = len(w_list)
        if idx > cs:                                 # backward, from the start of this window
            replaced, untr = 0, 0
            ev.add("gap")
            if not w_list:
                ev.add("leading_gap")
            if err == 0:                             # (the traced function's shortcut)
                y_start = r_s + pe - (ql - 1)
            elif not traced_domain(task):
                untr = 1; flags[0] |= UNTRACED
            else:
                log.append(("anchor", tuple(int(x) for x in task)))
                e2, ps, pe2 = align(task, True)
                assert (e2, pe2) == (err, pe), ("cleared entry differs from the preset one", task, (e2, pe2), (err, pe))
                y_start = r_s + ps
                if (pe + 1 == r_l or ps == 0) and err > 0:
                    try:
                        rr = _recal(task, l, ps, pe, err, align, log)
                    except _Untraced:
                        flags[0] |= UNTRACED; rr = None
                    if rr is not None:
                        t2, err, ps, pe = rr; replaced = 1; ev.add("replaced")
                        y_start, y_end = int(t2[1]) + ps, int(t2[1]) + pe
            if not untr:
                toff, j = y_start - 1, idx - 1
                while j >= cs:
                    wj, ws, we = wins[j]
                    ys = toff + 1 - (we + 1 - ws)
                    if ys < 0:
                        ev.add("backward_ys"); break
                    r = _aln_wlst(z, l, wl, e_rate, wj, ws, we, ys, 1, align, log, flags)
                    if r is None:
                        ev.add("backward_failed"); break
                    recs.append(r); w_list.append([j, r[1], r[2]]); align_length += we + 1 - ws; ev.add("backward")
                    if r[6]:
                        ev.add("replaced")
                    toff = r[1] - 1; j -= 1
                else:
                    ev.add("backward_cs")
            recs.append([w, y_start, y_end, err, int(task[8]), ANCHOR, replaced])
        align_length += ql
        aln = ovl - ((q_e + 1 - xs) - align_length)
        if not pass_qovlp(ovl, aln):
            exit_win = w; ev.add("exit")
            break
        w_list[a_n:] = w_list[a_n:][::-1]
        w_list.append([idx, y_start, y_end])
    verdict = 1 if exit_win == NO_EXIT and pass_qovlp(ovl, align_length) else 0
    if exit_win == NO_EXIT and not verdict:
        ev.add("verdict0_no_exit")
    if verdict and not pass_qovlp(ovl, sum(q_e + 1 - q_s for w, q_s, q_e in wins if w in prim and int(prim[w][1]) != NOALN)):
        ev.add("verdict1_by_rescue")
    if flags[0] & UNTRACED:
        ev.add("untraced")
    recs.sort(key=lambda r: r[0])
    W = np.array(recs, dtype=np.int64).reshape(-1, 7)
    return dict(verdict=verdict, flags=flags[0], exit_win=exit_win, align_length=align_length, n_rescued=int((W[:, 5] < ANCHOR).sum()), wins=W, log=log, events=ev)


def read_rescue(ol, fc, fc_off, lengths, wl, e_rate, res, align):
    """every overlap of one read: res = the primary results (int32 [m, 2]) in refgrid_model.read_tasks' order -> list of rescue_overlap's dicts"""
    T, infos = M.read_tasks(ol, fc, fc_off, lengths, wl, e_rate, with_info=True)
    prim = [dict() for _ in range(len(ol))]
    k = 0
    for i, w, info in infos:
        if info["unresolved"] or info["refused"]:
            continue
        prim[i][w] = (T[k], int(res[k, 0]), int(res[k, 1])); k += 1
    assert k == T.shape[0]
    return [rescue_overlap(ol[i], lengths, wl, e_rate, prim[i], align) for i in range(len(ol))]


def oracle_aligner(o):
    """align(task, traced) over the oracle: hao_or_window_ed, and hao_or_window_trace mode 3 (ed_band_cal_semi_64_w_absent_diag_trace on a cleared bit_extz_t)"""
    def align(task, traced):
        t = np.array([task], dtype=np.int64).astype(np.uint32)
        if traced:
            out, _ = o.window_trace(t, cap=80, mode=3)
            return int(out[0, 0]), int(out[0, 1]), int(out[0, 2])
        r = o.window_ed(t)
        return int(r[0, 0]), 0, int(r[0, 1])
    return align
