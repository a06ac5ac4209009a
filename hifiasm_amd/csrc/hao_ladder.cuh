// The threshold ladder of hc_aln_exz (Correct.cpp:14576-14636) on the device: the caller of the long alignments (hao_align.cuh, hao_align_coop.cuh), which this file
// calls and does not restate.  A request is a stretch of an overlap's query read (and, outside mode 3, of its target); the reference tries it at up to four
// growing thresholds and keeps the first alignment that ends within its threshold.  The four thresholds depend on the request alone, so:
//   1. hao_ld_thre_kernel: a thread per request - the range checks, the gate (ql <= maxl, estimate_err * 1.2 <= maxe), the rungs that are not skipped
//      (hao_ld_rungs: scale_ed_thre, the FP64 products truncated to int64, the cap at ql, thre > thre0), the result preset to "none", and the first open list;
//   2. per round j (at most four), hao_ld_task_kernel: a thread per open request - cal_exz_infi's coordinate step with rung j's threshold (hao_ld_coords: mode 3
//      update_semi_coord = hao_ref_shift + hao_rs_init_waln, modes 1 / 2 adjust_ext_offset), the test qe > qs && te > ts, the task record, a sort key (mode, kernel
//      class, text) and the counters the host needs to launch the sweeps: tasks per (mode, class), band words, longest text, widest column block;
//   3. the traced sweeps of hao_window_trace_long, per mode and class, over the sorted slots (hao_f3.hip: hao_al_ladder);
//   4. hao_ld_commit_kernel: a thread per open request - an alignment within its threshold becomes the request's result (its cigar stays in the round's rows until
//      the end), any other request with a rung left goes into the next round's list;
//   5. a scan of the entry counts and hao_ld_fill_kernel: the rows into one CSR array.
// Requests, results and lists stay on the device; the host reads counters.
//
// The same machinery serves hc_aln_exz_adv (Correct.cpp:16082-16165; hao_window_ladder_adv), the sibling the read-overlap path runs: every kernel and the host runner
// (hao_f3.hip: hao_ld_run) take the rule set as a template parameter ADV, and hao_ld_rule<ADV> names what it changes - the result record and the attempts per request.
// Under ADV: the entry's early returns, estimate_err < 0 (ql * e_rate, or cal_estimate_err over the batch's resident window lists: hao_ld_estimate_wlist), the gate on estimate_err >> 1, five raw rungs without the cap at ql (hao_ld_rungs_adv), cal_exz_infi_adv's
// clamps by dd = max(ql, tl) before and after the coordinate step and its pthre test (per-request state across rounds: pth[]), absolute result coordinates, and between
// set-up and the rounds hao_ld_exact_kernel, cal_exact_exz (:15725-15767) over the requests with ql <= 16 - those it settles never enter a round.
#pragma once
#include "hao_align.cuh"
#include "hao_align_coop.cuh"
#include "hao_grid_pair.cuh"
#include "hao_rescue.cuh"          // (hao_rs_init_waln)
#include "hao_trace_grid.cuh"      // (hao_tg_semi_domain)

// scale_ed_thre (Correct.cpp:14354-14360): the largest threshold whose band has as many 64-bit words as err's, capped; the arithmetic in the reference's types
HAO_AL_FN int64_t hao_ld_scale(uint32_t err, uint32_t max_err)
{
	const uint64_t bd = (uint32_t)((err << 1) + 1); uint64_t w = (bd >> 6) << 6;
	if (w < bd) w += 64;
	err = (uint32_t)((w - 1) >> 1); if (err > max_err) err = max_err;
	return err;
}
// the rungs of a request (hc_aln_exz :14599-14631): thre[k] = rung k + 1's threshold, -1 where the rung is skipped or the gate is shut; returns the attempts
HAO_AL_FN int hao_ld_rungs(int64_t ql, int64_t estimate_err, double e_rate, int64_t maxl, int64_t maxe, int32_t thre[4])
{
	thre[0] = thre[1] = thre[2] = thre[3] = -1;
	if (!(ql <= maxl && ((double)estimate_err * 1.2) <= (double)maxe)) return 0;
	int64_t t = hao_ld_scale((uint32_t)estimate_err, (uint32_t)maxe), t0; if (t > ql) t = ql;
	int n = 1; thre[0] = (int32_t)t;
	t0 = t; t = (int64_t)((double)ql * e_rate);
	t = hao_ld_scale((uint32_t)t, (uint32_t)maxe); if (t > ql) t = ql;
	if (t > t0) { thre[1] = (int32_t)t; ++n; }
	t0 = t; t <<= 1;
	t = hao_ld_scale((uint32_t)t, (uint32_t)maxe); if (t > ql) t = ql;
	if (t > t0) { thre[2] = (int32_t)t; ++n; }
	t0 = t; t = (int64_t)((double)ql * 0.51);
	t = hao_ld_scale((uint32_t)t, (uint32_t)maxe); if (t > ql) t = ql;
	if (t > t0) { thre[3] = (int32_t)t; ++n; }
	return n;
}
// the rungs of hc_aln_exz_adv (:16109-16156): no cap at ql, the gate on estimate_err >> 1, thre > thre0 for rungs 2 - 4 only, a fifth rung at maxe when ql <= force_l
HAO_AL_FN int hao_ld_rungs_adv(int64_t ql, int64_t estimate_err, double e_rate, int64_t maxl, int64_t maxe, int64_t force_l, int32_t thre[5])
{
	thre[0] = thre[1] = thre[2] = thre[3] = thre[4] = -1;
	if (!(ql <= maxl && (estimate_err >> 1) <= maxe)) return 0;
	int64_t t = hao_ld_scale((uint32_t)estimate_err, (uint32_t)maxe), t0;
	int n = 1; thre[0] = (int32_t)t;
	t0 = t; t = (int64_t)((double)ql * e_rate); t = hao_ld_scale((uint32_t)t, (uint32_t)maxe);
	if (t > t0) { thre[1] = (int32_t)t; ++n; }
	t0 = t; t <<= 1; t = hao_ld_scale((uint32_t)t, (uint32_t)maxe);
	if (t > t0) { thre[2] = (int32_t)t; ++n; }
	t0 = t; t = (int64_t)((double)ql * 0.51); t = hao_ld_scale((uint32_t)t, (uint32_t)maxe);
	if (t > t0) { thre[3] = (int32_t)t; ++n; }
	if (ql <= force_l) { thre[4] = (int32_t)maxe; ++n; }
	return n;
}
// estimate_err < 0 (:16092-16095): ql * e_rate when ql <= wl; false = the other branch (cal_estimate_err over z->w_list: hao_ld_estimate_wlist, which needs the overlap's records)
HAO_AL_FN bool hao_ld_estimate(int64_t ql, double e_rate, int64_t wl, int64_t *estimate_err)
{
	if (*estimate_err >= 0) return true;
	if (ql > wl) return false;
	*estimate_err = (int64_t)((double)ql * e_rate);
	return true;
}
// cal_estimate_err (Correct.cpp:15369-15401) over the n records of overlap z as hao_window_wlist_ref leaves them (hao_wlist.cuh): aligned windows only, ascending, x_start /
// x_end + 1 of a record = hao_ref_window of its grid window, error = info & 0xff (untraced records count like any other).  est, from the unclamped request, when the list is
// empty or ends before the clamped qs (the exit at :15377 - the reference walks forward from get_win_id_by_s's guess, which on an ascending list ends at the first record
// with x_end >= qs or beyond the last; the walk back at :15379 only adds records that do not reach qs).  Then, in record order: a record covered whole adds its error, a
// partly covered one error * ovlp / length in double INTO the int64 sum (truncated at every step, as the reference's `tot +=` does), the uncovered rest * e_rate at the end.
// FP64 in the reference's operation order; the build contracts nothing (-ffp-contract=off)
HAO_AL_FN int64_t hao_ld_estimate_wlist(const hao_ovlp_t &z, const hao_rs_win *w, uint64_t n, int64_t wl, int64_t qs, int64_t qe, double e_rate)
{
	const int64_t est = (int64_t)((double)(qe - qs) * e_rate);
	if (!n) return est;
	if (qs < (int64_t)z.x_pos_s) qs = (int64_t)z.x_pos_s;
	if (qe > (int64_t)z.x_pos_e + 1) qe = (int64_t)z.x_pos_e + 1;
	uint64_t lo = 0, hi = n;      // first record with x_end >= qs
	while (lo < hi) {
		const uint64_t m = (lo + hi) >> 1; int64_t ws, wn; hao_ref_window(z, w[m].win, (uint32_t)wl, &ws, &wn);
		if (ws + wn - 1 < qs) lo = m + 1; else hi = m;
	}
	if (lo == n) return est;
	int64_t tot = 0, cov_l = 0;
	for (uint64_t k = lo; k < n; ++k) {
		int64_t ws, wn; hao_ref_window(z, w[k].win, (uint32_t)wl, &ws, &wn);
		if (!(ws < qe)) break;
		const int64_t we = ws + wn, os = qs > ws ? qs : ws, oe = qe < we ? qe : we, ovlp = oe > os ? oe - os : 0;
		if (!ovlp) continue;
		cov_l += ovlp;
		const int64_t error = (int64_t)(w[k].info & 0xffu);
		if (ovlp == we - ws) tot += error;
		else tot = (int64_t)((double)tot + ((double)error) * ((double)ovlp) / ((double)(we - ws)));
	}
	tot = (int64_t)((double)tot + (double)((qe - qs) - cov_l) * e_rate);
	return tot;
}
// adjust_ext_offset (Correct.cpp:14400-14422)
HAO_AL_FN void hao_ld_adjust_ext(int64_t *qs, int64_t *qe, int64_t *ts, int64_t *te, int64_t ql, int64_t tl, int64_t thre, int mode)
{
	if (mode == 1) {
		const int64_t qoff = ql - *qs, toff = tl - *ts;
		if (qoff <= toff) { *qe = ql; *te = *ts + qoff + thre; } else { *te = tl; *qe = *qs + toff + thre; }
	} else if (mode == 2) {
		const int64_t qoff = *qe, toff = *te;
		if (qoff <= toff) { *qs = 0; *ts = *te - qoff - thre; } else { *ts = 0; *qs = *qe - toff - thre; }
	}
	if (*qs < 0) *qs = 0;
	if (*ts < 0) *ts = 0;
	if (*qe > ql) *qe = ql;
	if (*te > tl) *te = tl;
}

struct hao_ld_args {
	const hao_ladder_req_t *req; uint64_t n_req;
	const hao_ovlp_t *ol; uint64_t n_ol; const uint64_t *fc, *fc_off; const uint32_t *len; uint64_t n_reads;
	double e_rate; int64_t maxl, maxe; int coop_all;      // coop_all: HAO_DBG_FORCE=al_coop
	int64_t wl, force_l;                                  // hc_aln_exz_adv's two further parameters (ADV only)
	const uint64_t *wl_off; const hao_rs_win *wl_wins; int64_t wl_len;      // ADV only: the batch's window lists (hao_window_wlist_ref's record offsets per overlap and records) and the window length they were built on; null / 0 when none are resident
};
// what a rule set changes in the records: ADV = false hc_aln_exz, true hc_aln_exz_adv
template<bool ADV> struct hao_ld_rule { typedef hao_ladder_res_t res_t; enum { N_ATT = 4 }; };
template<> struct hao_ld_rule<true> { typedef hao_ladder_adv_res_t res_t; enum { N_ATT = 5 }; };
#define HAO_LD_ROUNDS 5      // the most rounds of either rule set; row set HAO_LD_ROUNDS of hao_ld_rows holds the exact shortcut's one-entry cigars
// (hao_ld_coord, the coordinates an attempt hands the aligner, lives in hao_grid_pair.cuh: the context holds a buffer of them; its flags: HAO_LADDER_* | HAO_LD_TASK)
#define HAO_LD_TASK 0x80000000u      // the slot holds a task of this round
// the counters (64 words): the fixed ones, then what a round's task kernel counts (HAO_LD_RND .. + HAO_LD_RND_N: one read-back)
enum { HAO_LD_BAD = 0, HAO_LD_OPEN = 1, HAO_LD_NEXT = 2, HAO_LD_OVER = 3, HAO_LD_RND = 4, HAO_LD_THRE = 4, HAO_LD_CNT = 8, HAO_LD_WORDS = 28, HAO_LD_TN = 32, HAO_LD_PW = 36, HAO_LD_RND_N = 48, HAO_LD_XCNT = 52 };      // (HAO_LD_XCNT: the requests of the exact shortcut's list)

// cal_exz_infi's coordinate step and test for request q at threshold thre (:14517-14523): true = T is the task; C = the coordinates either way.
// pthre != null, cal_exz_infi_adv (:15636-15640): thre is the rung's threshold already clamped by the request's dd, raw the rung's own; past the test the threshold becomes
// min(raw, max of the new lengths), and the attempt is abandoned unless it exceeds *pthre, which it then replaces
__device__ __forceinline__ bool hao_ld_coords(const hao_ld_args &A, const hao_ladder_req_t &q, int mode, int64_t thre, int64_t raw, int32_t *pthre, hao_ed_task_t *T, hao_ld_coord *C)
{
	const hao_ovlp_t z = A.ol[q.ol];
	const int64_t q_tot = A.len[z.x_id], t_tot = A.len[z.y_id];
	int64_t qs = q.qs, qe = q.qe, ts = q.ts, te = q.te, aux = 0; uint32_t fl = 0;
	if (mode == 3) {
		const int32_t sh = hao_ref_shift(A.fc + A.fc_off[q.ol], z.fc_len, qs);
		int64_t rs, rl;
		if (sh == HAO_REF_NOSHIFT) { fl |= HAO_LADDER_UNTRACED; ts = te = aux = -1; }
		else if (!hao_rs_init_waln(thre, (qs - (int64_t)z.x_pos_s) + (int64_t)z.y_pos_s + sh, t_tot, (qe - qs) + 2 * thre, &rs, &rl, &aux)) { fl |= HAO_LADDER_REFUSED; ts = te = aux = -1; }
		else { ts = rs; te = rs + rl; }
	} else if (mode == 1 || mode == 2) hao_ld_adjust_ext(&qs, &qe, &ts, &te, q_tot, t_tot, thre, mode);
	C->qs = (int32_t)qs; C->qe = (int32_t)qe; C->ts = (int32_t)ts; C->te = (int32_t)te; C->aux = (int32_t)aux;
	bool ok = !fl;
	if (ok && !(qe > qs && te > ts && ts != -1 && te != -1)) { fl |= HAO_LADDER_REFUSED; ok = false; }
	if (ok && pthre) {
		const int64_t dd = (qe - qs) > (te - ts) ? (qe - qs) : (te - ts);
		thre = raw > dd ? dd : raw;
		if (thre <= (int64_t)*pthre) { fl |= HAO_LADDER_REPEAT; ok = false; } else *pthre = (int32_t)thre;
	}
	if (ok) {
		T->p_rid = z.y_id; T->p_pos = (uint32_t)ts; T->p_len = (uint32_t)(te - ts); T->p_rev = z.y_pos_strand;
		T->t_rid = z.x_id; T->t_pos = (uint32_t)qs; T->t_len = (uint32_t)(qe - qs); T->t_rev = 0; T->thre = (uint32_t)thre; T->abs_diag = (uint32_t)aux;
		if (mode == 3 && !hao_tg_semi_domain(*T)) { fl |= HAO_LADDER_UNTRACED; ok = false; }
		// (what the range checks of hao_ld_thre_kernel and the clipping above guarantee, asked once more before a kernel indexes the reads with it)
		if (qs < 0 || ts < 0 || qe > q_tot || te > t_tot || te - ts > HAO_ED_LONG_MAX_LEN || qe - qs > HAO_ED_LONG_MAX_LEN || thre > HAO_ED_LONG_MAX_THRE) { fl |= HAO_LADDER_REFUSED; ok = false; }
	}
	C->flags = fl | (ok ? HAO_LD_TASK : 0u);
	return ok;
}

// hao_window_estimate_err: a thread per request (its ol, qs, qe only) - cal_estimate_err over the overlap's resident records, the value as it is; a request outside the batch
// or its query read is counted in *bad and reads nothing
__global__ __launch_bounds__(256) void hao_ld_estimate_kernel(const hao_ladder_req_t *req, uint64_t n, const hao_ovlp_t *ol, uint64_t n_ol, const uint32_t *len, uint64_t n_reads,
		const uint64_t *woff, const hao_rs_win *wins, int64_t wl, double e_rate, int64_t *est, unsigned long long *bad)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const hao_ladder_req_t q = req[i];
	est[i] = -1;
	if (q.ol >= n_ol) { atomicAdd(bad, 1ULL); return; }
	const hao_ovlp_t z = ol[q.ol];
	if (z.x_id >= n_reads || q.qs < 0 || q.qe < q.qs || (int64_t)q.qe > (int64_t)len[z.x_id]) { atomicAdd(bad, 1ULL); return; }
	est[i] = hao_ld_estimate_wlist(z, wins + woff[q.ol], woff[q.ol + 1] - woff[q.ol], wl, q.qs, q.qe, e_rate);
}

// per request: checks, rungs, the preset result, the first open list.  att[N_ATT i + k] = the threshold of attempt k, rung id in the top byte (attempts are the rungs that
// are not skipped).  ADV: the early returns, estimate_err < 0, raw rungs, pth[i] = -1; a request with ql <= 16 goes to xlist, not to the open list (hao_ld_exact_kernel)
template<bool ADV> __global__ __launch_bounds__(256) void hao_ld_thre_kernel(hao_ld_args A, int32_t *att, typename hao_ld_rule<ADV>::res_t *res, uint64_t *ncig, uint32_t *open, uint32_t *xlist, int32_t *pth, int64_t *est_out, unsigned long long *ctr)
{
	constexpr int NA = hao_ld_rule<ADV>::N_ATT;
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n_req) return;
	const hao_ladder_req_t q = A.req[i];
	typename hao_ld_rule<ADV>::res_t r; r.rung = 0; r.thre = 0; r.qs = q.qs; r.qe = q.qe; r.ts = q.ts; r.te = q.te; r.aux_beg = 0; r.flags = 0; r.err = HAO_AL_NONE; r.a_ps = r.a_pe = r.a_ts = r.a_te = -1; r.n_cigar = 0;
	if constexpr (ADV) { r.done = 0; pth[i] = -1; est_out[i] = -1; }
	ncig[i] = 0; for (int k = 0; k < NA; ++k) att[NA * i + k] = -1;
	bool bad = q.ol >= A.n_ol || q.mode > 3u || (!ADV && q.estimate_err < 0) || q.estimate_err >= (1 << 30), exact = false;
	int mode = (int)q.mode, n = 0;
	if (!bad) {
		if (q.ts == -1 && q.te == -1) mode = 3;
		const hao_ovlp_t z = A.ol[q.ol];
		if (z.x_id >= A.n_reads || z.y_id >= A.n_reads) bad = true;
		else {
			const int64_t q_tot = A.len[z.x_id], t_tot = A.len[z.y_id], ql = (int64_t)q.qe - q.qs, tl = (int64_t)q.te - q.ts;
			int64_t est = q.estimate_err; bool live = true;      // live: past the entry's early returns
			if (q.qs < 0 || q.qe < q.qs || q.qe > q_tot) bad = true;
			if constexpr (ADV) {      // :16088-16095 - the early returns look at the request's own ts / te, the forced (-1, -1) included
				if (ql == 0 && tl == 0) { r.done = 1; live = false; }
				else if (ql <= 0 || tl <= 0) live = false;
				if (live && (q.ts < 0 || q.te > t_tot)) bad = true;
				if (live && !bad && !hao_ld_estimate(ql, A.e_rate, A.wl, &est)) {      // ql > wl: cal_estimate_err over the overlap's resident records; a negative value (a stretch that ends before the overlap starts) is a refused request
					if (A.wl_off && A.wl_len == A.wl) est = hao_ld_estimate_wlist(z, A.wl_wins + A.wl_off[q.ol], A.wl_off[q.ol + 1] - A.wl_off[q.ol], A.wl, q.qs, q.qe, A.e_rate);
					if (est < 0) bad = true;
				}
				if (live && !bad) { exact = ql <= 16; est_out[i] = est; }
			} else {
				if (mode != 3 && (q.ts < 0 || q.te < q.ts || q.te > t_tot)) bad = true;
				if (mode == 3) { r.ts = r.te = -1; }
			}
			int32_t th[NA];
			if (!bad && live) {
				if constexpr (ADV) n = hao_ld_rungs_adv(ql, est, A.e_rate, A.maxl, A.maxe, A.force_l, th);
				else n = hao_ld_rungs(ql, est, A.e_rate, A.maxl, A.maxe, th);
			}
			if (n) {      // the lengths every attempt derives (mode 3: init_waln leaves at most ql + 2 thre; ADV: thre clamped by dd = max(ql, tl), :15624-15632)
				if (ql > HAO_ED_LONG_MAX_LEN) bad = true;
				int k2 = 0;
				for (int k = 0; k < NA && !bad; ++k) if (th[k] >= 0) {
					int64_t qs = q.qs, qe = q.qe, ts = q.ts, te = q.te, t = th[k];
					if (ADV && t > (ql > tl ? ql : tl)) t = ql > tl ? ql : tl;
					if (mode == 3) { ts = 0; te = ql + 2 * t; }
					else hao_ld_adjust_ext(&qs, &qe, &ts, &te, q_tot, t_tot, t, mode);
					if (te - ts > HAO_ED_LONG_MAX_LEN || qe - qs > HAO_ED_LONG_MAX_LEN) bad = true;
					att[NA * i + k2++] = th[k] | (k + 1) << 24;
				}
			}
		}
	}
	res[i] = r;
	if (bad) { atomicAdd(ctr + HAO_LD_BAD, 1ULL); return; }
	if (exact) xlist[atomicAdd(ctr + HAO_LD_XCNT, 1ULL)] = (uint32_t)i;
	else if (n) open[atomicAdd(ctr + HAO_LD_OPEN, 1ULL)] = (uint32_t)i;
}

// cal_exact_exz (:15725-15767) over the slots of the shortcut's list (bound >= their count, which lies in ctr[HAO_LD_XCNT]): the target interval of the mode, clamped, must
// have ql (<= 16) bases equal to the query's - N equals N only, as in the strings recover_UC_Read_sub_region hands memcmp.  A request it settles gets its result and the
// one-entry cigar in xrow[slot]; any other with an attempt joins the first open list
__global__ __launch_bounds__(256) void hao_ld_exact_kernel(hao_ld_args A, hao_ed_reads R, const uint32_t *xlist, uint64_t bound, const int32_t *att, hao_ladder_adv_res_t *res,
		uint64_t *ncig, uint64_t *rowref, uint16_t *xrow, uint32_t *open, unsigned long long *ctr)
{
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= bound || s >= ctr[HAO_LD_XCNT]) return;
	const uint32_t i = xlist[s];
	const hao_ladder_req_t q = A.req[i];
	const hao_ovlp_t z = A.ol[q.ol];
	const int64_t t_tot = A.len[z.y_id], qs = q.qs, qe = q.qe, ql = qe - qs;      // (1 <= ql <= 16, [qs, qe) inside the query read: hao_ld_thre_kernel)
	int64_t ts = q.ts, te = q.te; uint32_t fl = 0; bool ok = true;
	if (q.mode == 3u) {      // (the forced mode 3 never gets here)
		const int32_t sh = hao_ref_shift(A.fc + A.fc_off[q.ol], z.fc_len, qs);
		if (sh == HAO_REF_NOSHIFT) { fl = HAO_LADDER_UNTRACED; ok = false; }
		else { ts = (qs - (int64_t)z.x_pos_s) + (int64_t)z.y_pos_s + sh; te = ts + ql; }
	} else if (q.mode == 1u) te = ts + ql;
	else if (q.mode == 2u) ts = te - ql;
	if (ts < 0) ts = 0;
	if (ts > t_tot) ts = t_tot;
	if (te > t_tot) te = t_tot;
	if (te - ts != ql) ok = false;      // (else 0 <= ts < te <= t_tot)
	if (ok) {
		hao_al_pstream P, Q;
		hao_al_pstream_init(P, hao_al_walk_of(R, z.y_id, (uint32_t)ts, (uint32_t)ql, z.y_pos_strand, false));
		hao_al_pstream_init(Q, hao_al_walk_of(R, z.x_id, (uint32_t)qs, (uint32_t)ql, 0u, false));
		for (int64_t k = 0; k < ql; ++k) if (hao_al_pstream_next(P) != hao_al_pstream_next(Q)) ok = false;
	}
	if (ok) {
		hao_ladder_adv_res_t r; r.done = 1; r.rung = HAO_LADDER_RUNG_EXACT; r.thre = 0; r.qs = (int32_t)qs; r.qe = (int32_t)qe; r.ts = (int32_t)ts; r.te = (int32_t)te; r.aux_beg = 0; r.flags = 0;
		r.err = 0; r.a_ps = (int32_t)ts; r.a_pe = (int32_t)te - 1; r.a_ts = (int32_t)qs; r.a_te = (int32_t)qe - 1; r.n_cigar = 1;
		res[i] = r; ncig[i] = 1; xrow[s] = (uint16_t)ql; rowref[i] = (uint64_t)HAO_LD_ROUNDS << 32 | s;      // (push_trace(0, ql): op 0 in the top bits)
		return;
	}
	res[i].flags = fl;
	if (att[hao_ld_rule<true>::N_ATT * (uint64_t)i] >= 0) open[atomicAdd(ctr + HAO_LD_OPEN, 1ULL)] = i;
}

// round j over the slots of the open list (bound >= their count, which lies in ctr[HAO_LD_OPEN]): coordinates, task, sort key, the round's counters
// (ADV: the rung's threshold clamped by the request's dd for the coordinate step, clamped again on the new lengths and tested against pth[i] inside hao_ld_coords; the
// band class follows the task's - clamped - threshold)
template<bool ADV> __global__ __launch_bounds__(256) void hao_ld_task_kernel(hao_ld_args A, int j, const int32_t *att, const uint32_t *open, uint64_t bound, hao_ed_task_t *task, hao_ld_coord *coord,
		uint64_t *key, uint32_t *idx, int32_t *pth, unsigned long long *ctr)
{
	constexpr int NA = hao_ld_rule<ADV>::N_ATT;
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= bound) return;
	idx[s] = (uint32_t)s; key[s] = ~0ULL;
	if (s >= ctr[HAO_LD_OPEN]) return;
	const uint32_t i = open[s];
	const hao_ladder_req_t q = A.req[i];
	const int mode = (q.ts == -1 && q.te == -1) ? 3 : (int)q.mode;
	const int64_t raw = att[NA * (uint64_t)i + j] & 0xffffff;
	int64_t thre = raw;
	if constexpr (ADV) { const int64_t ql = (int64_t)q.qe - q.qs, tl = (int64_t)q.te - q.ts, dd = ql > tl ? ql : tl; if (thre > dd) thre = dd; }
	hao_ed_task_t T; hao_ld_coord C;
	T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	const bool ok = hao_ld_coords(A, q, mode, thre, raw, ADV ? pth + i : nullptr, &T, &C);
	task[s] = T; coord[s] = C;
	if (!ok) return;
	const uint32_t nw = hao_al_nword(T.thre);
	const int cls = (nw <= 4 && !A.coop_all) ? 0 : hao_alc_lg(nw) - 2;
	key[s] = (uint64_t)mode << 61 | (uint64_t)cls << 58 | (uint64_t)(cls ? 0u : nw - 1) << 56 | ((hao_al_sort_key(T) & ((1ULL << 62) - 1)) >> 6);
	atomicAdd(ctr + HAO_LD_CNT + mode * 5 + cls, 1ULL);
	atomicMax(ctr + HAO_LD_THRE, (unsigned long long)T.thre);
	if (cls == 0) { atomicOr(ctr + HAO_LD_WORDS + mode, 1ULL << (nw - 1)); atomicMax(ctr + HAO_LD_TN + mode, (unsigned long long)T.t_len); }
	else atomicMax(ctr + HAO_LD_PW + mode * 4 + (cls - 1), (unsigned long long)hao_alc_path_words(T.thre, T.t_len));
}

// column offsets of a cooperative class's selected pairs: slices of `per` pairs, `pw` words each
__global__ void hao_ld_poff_kernel(uint64_t *poff, uint64_t n, uint64_t per, uint64_t pw)
{
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s < n) poff[s] = (s % per) * pw;
}

// round j's end: the attempts that aligned become results, the other requests with an attempt left form the next list
// (ADV: the threshold is the task's, the clamped one; the bit_extz_t coordinates become absolute, :15665-15666)
template<bool ADV> __global__ __launch_bounds__(256) void hao_ld_commit_kernel(int j, const int32_t *att, const uint32_t *open, uint64_t bound, const hao_ed_task_t *task, const hao_ld_coord *coord,
		const hao_trace_result_t *tr, uint32_t cap, typename hao_ld_rule<ADV>::res_t *res, uint64_t *ncig, uint64_t *rowref, uint32_t *next, unsigned long long *ctr)
{
	constexpr int NA = hao_ld_rule<ADV>::N_ATT;
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= bound || s >= ctr[HAO_LD_OPEN]) return;
	const uint32_t i = open[s];
	const hao_ld_coord C = coord[s];
	const int32_t a = att[NA * (uint64_t)i + j], thre = ADV ? (int32_t)task[s].thre : (a & 0xffffff);
	const uint32_t fl = res[i].flags | (C.flags & ~HAO_LD_TASK);
	if (C.flags & HAO_LD_TASK) {
		const hao_trace_result_t x = tr[s];
		if (x.err <= thre) {      // is_align (Levenshtein_distance.h:787)
			typename hao_ld_rule<ADV>::res_t r; r.rung = (uint32_t)(a >> 24); r.thre = thre; r.qs = C.qs; r.qe = C.qe; r.ts = C.ts; r.te = C.te; r.aux_beg = C.aux; r.flags = fl;
			r.err = x.err; r.a_ps = x.ps; r.a_pe = x.pe; r.a_ts = x.ts; r.a_te = x.te; r.n_cigar = x.n_cigar;
			if constexpr (ADV) { r.done = 1; r.a_ps += C.ts; r.a_pe += C.ts; r.a_ts += C.qs; r.a_te += C.qs; }
			res[i] = r; ncig[i] = (uint64_t)x.n_cigar; rowref[i] = (uint64_t)j << 32 | s;
			if ((uint32_t)x.n_cigar > cap) atomicAdd(ctr + HAO_LD_OVER, 1ULL);
			return;
		}
	}
	res[i].flags = fl;
	if (j < NA - 1 && att[NA * (uint64_t)i + j + 1] >= 0) next[atomicAdd(ctr + HAO_LD_NEXT, 1ULL)] = i;
}

// the rows of the requests that aligned into the CSR array (rows[j] / cap[j]: round j's)
struct hao_ld_rows { const uint16_t *rows[HAO_LD_ROUNDS + 1]; uint32_t cap[HAO_LD_ROUNDS + 1]; };
__global__ __launch_bounds__(256) void hao_ld_fill_kernel(hao_ld_rows W, const uint64_t *ncig, const uint64_t *rowref, const uint64_t *off, uint64_t n, uint16_t *cig, uint64_t total)
{
	const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; const int lane = threadIdx.x & 63;
	if (i >= n) return;
	const uint64_t m = ncig[i], o = off[i];
	if (m == 0 || o + m > total) return;
	const uint64_t rr = rowref[i]; const int j = (int)(rr >> 32) & 7;
	if (j > HAO_LD_ROUNDS || m > W.cap[j]) return;
	const uint16_t *src = W.rows[j] + (rr & 0xffffffffULL) * W.cap[j];
	for (uint64_t k = lane; k < m; k += 64) cig[o + k] = src[k];
}
