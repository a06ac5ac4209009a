"""Reference placement of the window / candidate pairs, restated in plain Python from the reference's own lines - independent of hao_ref_pair
(hifiasm_amd/csrc/hao_grid_pair.cuh), which every task comparison of the reference-placed grid is held against:

  the window grid        get_num_wins / get_win_se_by_normalize_xs (Correct.cpp:782-787): windows at multiples of `window`, clipped to [x_pos_s, x_pos_e]
  the target start       (q_s - x_pos_s) + y_pos_s + y_start_offset(q_s, &z->f_cigar)   (Correct.cpp:12966-12967, Hash_Table.h:165-189)
  the threshold          thre = q_l * e_rate (truncated); Adjust_Threshold (Correct.h:46); at most THRESHOLD_MAX_SIZE = 31   (Correct.cpp:12963-12964)
  admission, clipping    init_waln (Correct.cpp:764-779)

Tasks come out in the device's order: (query read, grid window, position in ol->list)."""
import numpy as np

THRESHOLD_MAX_SIZE = 31
UNRESOLVED = None


def threshold(q_l, e_rate):
    t = int(q_l * e_rate)            # (int64_t)(q_l * e_rate): a double product, truncated
    if t == 0 and q_l >= 4:          # Adjust_Threshold
        t = 1
    return min(t, THRESHOLD_MAX_SIZE)


def fake_gap_pos(e):
    return int(e) >> 32


def fake_gap_shift(e):
    v = int(e) & 0xFFFFFFFF
    return -(v >> 1) if v & 1 else v >> 1


def y_start_offset(x_start, fc):
    """Hash_Table.h:165-189; UNRESOLVED where the reference prints ERROR and exits"""
    n = len(fc)
    if n == 0:
        return UNRESOLVED
    if x_start == fake_gap_pos(fc[n - 1]):
        return fake_gap_shift(fc[n - 1])
    i = 0
    while i < n:
        if x_start < fake_gap_pos(fc[i]):
            break
        i += 1
    if i == 0 or i == n:
        return UNRESOLVED
    return fake_gap_shift(fc[i - 1])   # note here return i - 1


def init_waln(err, s, l, w_l):
    """Correct.cpp:764-779 -> None or (aux_beg, aux_end, r_s, r_l)"""
    if s < 0 or s >= l or (l - s + 2 * err + THRESHOLD_MAX_SIZE) < w_l:
        return None
    r_s = s - err
    r_l = l - r_s
    if r_l > w_l:
        r_l = w_l
    aux_end = w_l - r_l
    aux_beg = 0
    if r_s < 0:
        aux_beg = -r_s; r_s = 0; r_l -= aux_beg
    return aux_beg, aux_end, r_s, r_l


def windows(xs, xe, wl):
    """(grid window index, q_s, q_e) of an overlap's windows: align_hc_ed_post_extz's loop"""
    nl = (xe + 1) - (xs // wl) * wl
    nw = nl // wl + (1 if nl % wl else 0)
    q_s = xs
    q_e = (xs // wl) * wl + wl - 1
    if q_e >= xe:
        q_e = xe
    out = []
    for k in range(nw):
        out.append((xs // wl + k, q_s, q_e))
        q_s = q_e + 1; q_e = q_s + wl - 1
        if q_e >= xe:
            q_e = xe
    return out


def overlap_pairs(z, fc, lengths, wl, e_rate):
    """every window of overlap z (12 uint32: hao_ovlp_t) with fake cigar fc -> list of (grid window, task or None, info); info = dict(shift, thre, aux_beg, aux_end,
    refused, unresolved)"""
    xid, xs, xe, yid, ys, yrev = int(z[0]), int(z[1]), int(z[2]), int(z[4]), int(z[5]), int(z[7])
    l = int(lengths[yid])
    out = []
    for w, q_s, q_e in windows(xs, xe, wl):
        q_l = 1 + q_e - q_s
        thre = threshold(q_l, e_rate)
        sh = y_start_offset(q_s, fc)
        info = dict(shift=sh, thre=thre, aux_beg=0, aux_end=0, refused=False, unresolved=sh is UNRESOLVED, q_l=q_l)
        if sh is UNRESOLVED:
            out.append((w, None, info)); continue
        t_s = (q_s - xs) + ys + sh
        aln_l = q_l + (thre << 1)
        r = init_waln(thre, t_s, l, aln_l)
        if r is None:
            info["refused"] = True
            out.append((w, None, info)); continue
        aux_beg, aux_end, r_s, r_l = r
        info["aux_beg"], info["aux_end"] = aux_beg, aux_end
        out.append((w, (yid, r_s, r_l, yrev, xid, q_s, q_l, 0, thre, aux_beg), info))
    return out


def read_tasks(ol, fc, fc_off, lengths, wl, e_rate, with_info=False):
    """the tasks of one read (ol uint32 [n,12], fc uint64, fc_off [n+1] relative offsets) in the device's order: grid window, then position in ol->list.
    -> uint32 [m,10] (and, with_info, the list of (overlap index, grid window, info) of EVERY covered window, admitted or not)"""
    per = []
    for i, z in enumerate(ol):
        per.append(overlap_pairs(z, fc[int(fc_off[i]):int(fc_off[i + 1])], lengths, wl, e_rate))
    rows, infos, keyed = [], [], []
    for i, lst in enumerate(per):
        for w, t, info in lst:
            keyed.append((w, i, t, info))
    keyed.sort(key=lambda x: (x[0], x[1]))
    for w, i, t, info in keyed:
        infos.append((i, w, info))
        if t is not None:
            rows.append(t)
    T = np.array(rows, dtype=np.int64).reshape(-1, 10).astype(np.uint32)
    return (T, infos) if with_info else T


def summaries(ol, fc, fc_off, lengths, wl, e_rate, res):
    """per-overlap (windows covered, windows aligned, aligned bases, error sum) from the read's results res (int32 [m,2], in read_tasks' order)"""
    T, infos = read_tasks(ol, fc, fc_off, lengths, wl, e_rate, with_info=True)
    out = np.zeros((len(ol), 4), dtype=np.uint32)
    k = 0
    for i, w, info in infos:
        out[i, 0] += 1
        if info["unresolved"] or info["refused"]:
            continue
        if int(res[k, 0]) != 2**31 - 1:
            out[i, 1] += 1; out[i, 2] += info["q_l"]; out[i, 3] += int(res[k, 0])
        k += 1
    assert k == T.shape[0]
    return out
