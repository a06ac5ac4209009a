"""The product of align_hc_ed_post_extz (Correct.cpp:12951-13012), z->w_list, as the reference holds it once every window has been through
gen_backtrace_adv_exz - restated in plain Python from the reference's own lines, on top of tests/rescue_model.py's control flow, and independent of the device's
builders (hifiasm_amd/csrc/hao_wlist.cuh), which the window-list tests are held against:

  the trace of one window        gen_backtrace_adv_exz (Correct.cpp:12563-12639): the record's x_start / x_end, y_start, extra_begin / extra_end and threshold give
                                 init_waln's task again (aux_end >= 0: t_pri_l = aln_l - aux_beg - aux_end = r_l); the traced function is entered with (err, pe)
                                 preset
  its shortcut                   err == 0 (Levenshtein_distance.h:3783-3787): no sweep, ps = pe - (ql - 1), one match run of ql
  the re-placement               recal_boundary_exz (:2429-2468) when (pe + 1 == tl or ps == 0) and err > 0; taken iff it aligns with a strictly smaller err, and
                                 then its cigar replaces the first (z->w_list.c.n = p->cidx; push_wcigar)
  the cigar's encoding           push_trace (Levenshtein_distance.h:522-531): op << 14 | len, a run split at 0x3fff

Which task a window was aligned on is read from rescue_model's own log (its init_waln, its thresholds): a first-placement window and an anchor on the primary
task, a forward window on the task from its predecessor's y_end + 1, a backward window on the task that ends before its successor's y_start.  The reference
traces lazily (clen == 0) what the rescue has not traced; the trace is a pure function of the record, so tracing everything here gives the same list.
Backward windows and anchors were traced by the rescue: their trace here is that same call again and must give rescue_model's record (asserted).

The alignments come from a callback trace(task) -> (err, ps, pe, cigar) (the cleared traced function; err NOALN: none).  Nothing is guessed outside the domain
in which the reference's traced function stays inside its band word: such a window keeps its distance-only values, has no cigar and is flagged untraced; a
re-placement outside the domain is not made."""
import numpy as np

import rescue_model as RM

M = RM.M
NOALN = RM.NOALN
FWD, BWD, ANCHOR, PRIMARY = 0, 1, 2, 3


def match_run(ql):
    """push_trace(op 0, ql)"""
    out = []
    while ql >= 0x3fff:
        out.append(0x3fff); ql -= 0x3fff
    if ql:
        out.append(ql)
    return tuple(out)


def trace_window(task, l, trace, preset=None, log=None):
    """gen_backtrace_adv_exz on the record of `task` -> [y_start, y_end, err, re-placed, untraced, cigar, recal tried]; preset = the record's (err, pe), None for a
    window the rescue traced from a cleared entry"""
    yid, r_s, r_l, yrev, xid, q_s, ql, _, thres, _ = [int(x) for x in task]
    if preset is not None and preset[0] == 0:
        pe = preset[1]
        return [r_s + pe - (ql - 1), r_s + pe, 0, 0, 0, match_run(ql), 0]
    if not RM.traced_domain(task):
        assert preset is not None
        return [r_s, r_s + preset[1], preset[0], 0, 1, (), 0]
    err, ps, pe, cig = trace(task)
    if log is not None:
        log.append(tuple(int(x) for x in task))
    if preset is not None:
        assert (err, pe) == tuple(preset), ("cleared entry differs from the preset one", task, (err, pe), preset)
    assert err != NOALN
    replaced = tried = 0
    if (pe + 1 == r_l or ps == 0) and err > 0:
        ts = r_s if ps == 0 else r_s + pe - ql + 1
        r = M.init_waln(thres, ts, l, ql + 2 * thres)
        if r is not None:
            aux_beg, _, n_s, n_l = r
            t2 = (yid, n_s, n_l, yrev, xid, q_s, ql, 0, thres, aux_beg)
            if not (n_s == r_s and n_l == r_l) and RM.traced_domain(t2):
                tried = 1
                e2, ps2, pe2, cig2 = trace(t2)
                if log is not None:
                    log.append(t2)
                if e2 != NOALN and e2 < err:
                    err, ps, pe, cig, r_s, replaced = e2, ps2, pe2, cig2, n_s, 1
    return [r_s + ps, r_s + pe, err, replaced, 0, tuple(int(x) for x in cig), tried]


def wlist_overlap(z, lengths, wl, prim, res, trace, log=None):
    """res = rescue_model.rescue_overlap's result for the overlap, prim = its primary windows -> (wins int64 [m, 8]: win, y_start, y_end, err, thre, source,
    re-placed, untraced; cigars: a tuple per record; events; windows that need a sweep; re-placements tried)"""
    ev = set()
    if not res["verdict"]:
        ev.add("verdict0")
        return np.zeros((0, 8), dtype=np.int64), [], ev, 0, 0
    l = int(lengths[int(z[4])])
    rec = {int(r[0]): r for r in res["wins"]}
    tasks = {}
    for item in res["log"]:                                     # the task every rescued window was aligned on (the last request for the window is the one that stood)
        if item[0] in ("fwd", "bwd"):
            tasks[int(item[2])] = item[1]
    wins, cigs, swept, tried = [], [], 0, 0
    for w in sorted(set(rec) | {w for w, p in prim.items() if int(p[1]) != NOALN}):
        r = rec.get(w)
        if w in prim and int(prim[w][1]) != NOALN:
            task, err, pe = prim[w][0], int(prim[w][1]), int(prim[w][2])
            src = ANCHOR if r is not None else PRIMARY
            t = trace_window(task, l, trace, (err, pe), log)
            thre = int(task[8]); e0 = err
        else:
            src = int(r[5]); task = tasks[w]; thre = int(task[8]); e0 = int(r[3])
            if src == FWD:
                assert int(r[1]) == int(task[1])
                t = trace_window(task, l, trace, (int(r[3]), int(r[2]) - int(r[1])), log)
            else:
                t = trace_window(task, l, trace, None, log)
        if r is not None and src != FWD and not t[4]:           # traced by the rescue already: the same call again
            assert (t[0], t[1], t[2], t[3]) == (int(r[1]), int(r[2]), int(r[3]), int(r[6])), (w, t, r)
        wins.append([w, t[0], t[1], t[2], thre, src, t[3], t[4]]); cigs.append(t[5])
        tried += t[6]
        swept += e0 > 0 and not t[4]                            # a sweep is needed unless the record's err is 0 (the shortcut; a backward window that the rescue traced to err 0 is one match run) or the task is outside the domain
        ev.add(("primary", "forward", "backward", "anchor")[(src + 1) % 4] + ("_err0" if t[2] == 0 and not t[3] and src in (PRIMARY, FWD) else "_untraced" if t[4] else "_traced"))
        if t[3]:
            ev.add("replaced")
        elif t[6]:
            ev.add("recal_not_taken")
        ops = {c >> 14 for c in t[5]}
        if 2 in ops and 3 in ops:
            ev.add("indel_both")
        if t[4]:
            ev.add("untraced")
    if any(x[5] in (FWD, BWD) for x in wins):
        ev.add("verdict1_with_rescued")
    return np.array(wins, dtype=np.int64).reshape(-1, 8), cigs, ev, swept, tried


def read_wlist(ol, fc, fc_off, lengths, wl, e_rate, res, align, trace, log=None):
    """every overlap of one read: res = the primary results (int32 [m, 2]) in refgrid_model.read_tasks' order -> (rescue_model's dicts, [(wins, cigars, events, swept, tried)])"""
    T, infos = M.read_tasks(ol, fc, fc_off, lengths, wl, e_rate, with_info=True)
    prim = [dict() for _ in range(len(ol))]
    k = 0
    for i, w, info in infos:
        if info["unresolved"] or info["refused"]:
            continue
        prim[i][w] = (T[k], int(res[k, 0]), int(res[k, 1])); k += 1
    assert k == T.shape[0]
    rr = [RM.rescue_overlap(ol[i], lengths, wl, e_rate, prim[i], align) for i in range(len(ol))]
    return rr, [wlist_overlap(ol[i], lengths, wl, prim[i], rr[i], trace, log) for i in range(len(ol))]


def oracle_tracer(o):
    """trace(task) over the oracle: hao_or_window_trace mode 3 (ed_band_cal_semi_64_w_absent_diag_trace on a cleared bit_extz_t + gen_trace)"""
    def trace(task):
        t = np.array([task], dtype=np.int64).astype(np.uint32)
        out, cig = o.window_trace(t, cap=96, mode=3)
        n = int(out[0, 5])
        assert n <= 96
        return int(out[0, 0]), int(out[0, 1]), int(out[0, 2]), tuple(int(x) for x in cig[0, :n])
    return trace


def gold():
    """tests/golden/wlist.npz: the lists recorded from the reference's own functions (tests/golden/make_golden_wlist.py)"""
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wlist.npz"))


def gold_lists(G, key):
    """the fixture's lists of one configuration, one (wins int64 [m, 8], [cigar tuples], swept, tried) per overlap of its sampled reads, in order"""
    W, wo, cg, co, st = G[key + "_wins"].astype(np.int64), G[key + "_win_off"], G[key + "_cig"], G[key + "_cig_off"], G[key + "_swept_tried"]
    return [(W[int(wo[q]):int(wo[q + 1])], [tuple(int(x) for x in cg[int(co[j]):int(co[j + 1])]) for j in range(int(wo[q]), int(wo[q + 1]))], int(st[q, 0]), int(st[q, 1])) for q in range(len(wo) - 1)]
