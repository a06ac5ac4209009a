"""cal_estimate_err (Correct.cpp:15369-15401) restated in plain Python from the reference's own lines - the executable description the device function
(hifiasm_amd/csrc/hao_ladder.cuh: hao_ld_estimate_wlist) and its host twin are held against, beside tests/golden/estimate_err.npz, the reference's own values.

The list is z->w_list as align_hc_ed_post_extz leaves it: one record per aligned window, ascending; x_start / x_end of a record are its grid window clipped to
the overlap (Correct.h:1306-1314), error its distance.  The loops are the reference's, the guess of get_win_id_by_s included; a Python float is the reference's
double, int() its truncating cast, and `tot +=` of a double into an int64 truncates at every step, as C's compound assignment does."""


def window(z, w, wl):
    """x_start, x_end of grid window w of overlap z (a row of h_ec_lchain's overlap array)"""
    xs, xe = int(z[1]), int(z[2])
    return max(w * wl, xs), min(w * wl + wl - 1, xe)


def records(z, wins, wl):
    """[(x_start, x_end, error)] of window records given as rows (grid window, y_start, y_end, err, ...)"""
    return [window(z, int(x[0]), wl) + (int(x[3]),) for x in wins]


def estimate_err(z, wins, wl, qs, qe, e_rate):
    a = records(z, wins, wl)
    wn = len(a)
    est = int((qe - qs) * e_rate)
    if not wn:
        return est
    xs, xe = int(z[1]), int(z[2])
    if qs < xs:
        qs = xs
    if qe > xe + 1:
        qe = xe + 1
    ws = qs // wl * wl
    n_s = xs // wl * wl
    wid = (ws - n_s) // wl                       # get_win_id_by_s
    if wid >= wn:
        wid = wn - 1
    k = wid
    while k < wn and qs > a[k][1]:
        k += 1
    if k == wn:
        return est
    while k >= 0 and qs < a[k][0]:
        k -= 1
    if k < 0:
        k = 0
    tot = cov_l = 0
    while k < wn and a[k][0] < qe:
        ws, we = a[k][0], a[k][1] + 1
        os_, oe = max(qs, ws), min(qe, we)
        ovlp = oe - os_ if oe > os_ else 0
        if ovlp:
            cov_l += ovlp
            if ovlp == we - ws:
                tot += a[k][2]
            else:
                tot = int(tot + float(a[k][2]) * float(ovlp) / float(we - ws))
        k += 1
    tot = int(tot + ((qe - qs) - cov_l) * e_rate)
    return tot
