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
};
// (hao_ld_coord, the coordinates an attempt hands the aligner, lives in hao_grid_pair.cuh: the context holds a buffer of them; its flags: HAO_LADDER_* | HAO_LD_TASK)
#define HAO_LD_TASK 0x80000000u      // the slot holds a task of this round
// the counters (64 words): the fixed ones, then what a round's task kernel counts (HAO_LD_RND .. + HAO_LD_RND_N: one read-back)
enum { HAO_LD_BAD = 0, HAO_LD_OPEN = 1, HAO_LD_NEXT = 2, HAO_LD_OVER = 3, HAO_LD_RND = 4, HAO_LD_THRE = 4, HAO_LD_CNT = 8, HAO_LD_WORDS = 28, HAO_LD_TN = 32, HAO_LD_PW = 36, HAO_LD_RND_N = 48 };

// cal_exz_infi's coordinate step and test for request q at threshold thre (:14517-14523): true = T is the task; C = the coordinates either way
__device__ __forceinline__ bool hao_ld_coords(const hao_ld_args &A, const hao_ladder_req_t &q, int mode, int64_t thre, hao_ed_task_t *T, hao_ld_coord *C)
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

// per request: checks, rungs, the preset result, the first open list.  att[4 i + k] = the threshold of attempt k, rung id in the top byte (attempts are the rungs that are not skipped)
__global__ __launch_bounds__(256) void hao_ld_thre_kernel(hao_ld_args A, int32_t *att, hao_ladder_res_t *res, uint64_t *ncig, uint32_t *open, unsigned long long *ctr)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n_req) return;
	const hao_ladder_req_t q = A.req[i];
	hao_ladder_res_t r; r.rung = 0; r.thre = 0; r.qs = q.qs; r.qe = q.qe; r.ts = q.ts; r.te = q.te; r.aux_beg = 0; r.flags = 0; r.err = HAO_AL_NONE; r.a_ps = r.a_pe = r.a_ts = r.a_te = -1; r.n_cigar = 0;
	ncig[i] = 0; att[4 * i] = att[4 * i + 1] = att[4 * i + 2] = att[4 * i + 3] = -1;
	bool bad = q.ol >= A.n_ol || q.mode > 3u || q.estimate_err < 0 || q.estimate_err >= (1 << 30);
	int mode = (int)q.mode, n = 0;
	if (!bad) {
		if (q.ts == -1 && q.te == -1) mode = 3;
		const hao_ovlp_t z = A.ol[q.ol];
		if (z.x_id >= A.n_reads || z.y_id >= A.n_reads) bad = true;
		else {
			const int64_t q_tot = A.len[z.x_id], t_tot = A.len[z.y_id], ql = (int64_t)q.qe - q.qs;
			if (q.qs < 0 || q.qe < q.qs || q.qe > q_tot) bad = true;
			if (mode != 3 && (q.ts < 0 || q.te < q.ts || q.te > t_tot)) bad = true;
			if (mode == 3) { r.ts = r.te = -1; }
			int32_t th[4];
			if (!bad) n = hao_ld_rungs(ql, q.estimate_err, A.e_rate, A.maxl, A.maxe, th);
			if (n) {      // the lengths every attempt derives (mode 3: init_waln leaves at most ql + 2 thre)
				if (ql > HAO_ED_LONG_MAX_LEN) bad = true;
				int k2 = 0;
				for (int k = 0; k < 4 && !bad; ++k) if (th[k] >= 0) {
					int64_t qs = q.qs, qe = q.qe, ts = q.ts, te = q.te;
					if (mode == 3) { ts = 0; te = ql + 2 * (int64_t)th[k]; }
					else hao_ld_adjust_ext(&qs, &qe, &ts, &te, q_tot, t_tot, th[k], mode);
					if (te - ts > HAO_ED_LONG_MAX_LEN || qe - qs > HAO_ED_LONG_MAX_LEN) bad = true;
					att[4 * i + k2++] = th[k] | (k + 1) << 24;
				}
			}
		}
	}
	res[i] = r;
	if (bad) { atomicAdd(ctr + HAO_LD_BAD, 1ULL); return; }
	if (n) open[atomicAdd(ctr + HAO_LD_OPEN, 1ULL)] = (uint32_t)i;
}

// round j over the slots of the open list (bound >= their count, which lies in ctr[HAO_LD_OPEN]): coordinates, task, sort key, the round's counters
__global__ __launch_bounds__(256) void hao_ld_task_kernel(hao_ld_args A, int j, const int32_t *att, const uint32_t *open, uint64_t bound, hao_ed_task_t *task, hao_ld_coord *coord,
		uint64_t *key, uint32_t *idx, unsigned long long *ctr)
{
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= bound) return;
	idx[s] = (uint32_t)s; key[s] = ~0ULL;
	if (s >= ctr[HAO_LD_OPEN]) return;
	const uint32_t i = open[s];
	const hao_ladder_req_t q = A.req[i];
	const int mode = (q.ts == -1 && q.te == -1) ? 3 : (int)q.mode;
	const int64_t thre = att[4 * (uint64_t)i + j] & 0xffffff;
	hao_ed_task_t T; hao_ld_coord C;
	T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	const bool ok = hao_ld_coords(A, q, mode, thre, &T, &C);
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
__global__ __launch_bounds__(256) void hao_ld_commit_kernel(int j, const int32_t *att, const uint32_t *open, uint64_t bound, const hao_ed_task_t *task, const hao_ld_coord *coord,
		const hao_trace_result_t *tr, uint32_t cap, hao_ladder_res_t *res, uint64_t *ncig, uint64_t *rowref, uint32_t *next, unsigned long long *ctr)
{
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= bound || s >= ctr[HAO_LD_OPEN]) return;
	const uint32_t i = open[s];
	const hao_ld_coord C = coord[s];
	const int32_t a = att[4 * (uint64_t)i + j], thre = a & 0xffffff;
	const uint32_t fl = res[i].flags | (C.flags & ~HAO_LD_TASK);
	if (C.flags & HAO_LD_TASK) {
		const hao_trace_result_t x = tr[s];
		if (x.err <= thre) {      // is_align (Levenshtein_distance.h:787)
			hao_ladder_res_t r; r.rung = (uint32_t)(a >> 24); r.thre = thre; r.qs = C.qs; r.qe = C.qe; r.ts = C.ts; r.te = C.te; r.aux_beg = C.aux; r.flags = fl;
			r.err = x.err; r.a_ps = x.ps; r.a_pe = x.pe; r.a_ts = x.ts; r.a_te = x.te; r.n_cigar = x.n_cigar;
			res[i] = r; ncig[i] = (uint64_t)x.n_cigar; rowref[i] = (uint64_t)j << 32 | s;
			if ((uint32_t)x.n_cigar > cap) atomicAdd(ctr + HAO_LD_OVER, 1ULL);
			return;
		}
	}
	res[i].flags = fl;
	if (j < 3 && att[4 * (uint64_t)i + j + 1] >= 0) next[atomicAdd(ctr + HAO_LD_NEXT, 1ULL)] = i;
}

// the rows of the requests that aligned into the CSR array (rows[j] / cap[j]: round j's)
struct hao_ld_rows { const uint16_t *rows[4]; uint32_t cap[4]; };
__global__ __launch_bounds__(256) void hao_ld_fill_kernel(hao_ld_rows W, const uint64_t *ncig, const uint64_t *rowref, const uint64_t *off, uint64_t n, uint16_t *cig, uint64_t total)
{
	const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; const int lane = threadIdx.x & 63;
	if (i >= n) return;
	const uint64_t m = ncig[i], o = off[i];
	if (m == 0 || o + m > total) return;
	const uint64_t rr = rowref[i]; const int j = (int)(rr >> 32) & 3;
	if (m > W.cap[j]) return;
	const uint16_t *src = W.rows[j] + (rr & 0xffffffffULL) * W.cap[j];
	for (uint64_t k = lane; k < m; k += 64) cig[o + k] = src[k];
}
