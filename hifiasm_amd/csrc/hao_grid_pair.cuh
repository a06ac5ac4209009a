// One window / candidate pair of the reference's fixed window grid (hao_grid.cuh describes the grid), shared by every side that forms pairs: the device's
// generators (hao_grid.cuh: hao_window_ed_grid and the delivery path's pair list), the delivery path's alignment kernel (hao_ed_deliver.cuh), which rebuilds
// each task in its lane, and the host decoder of a delivered batch (hao_unpack_ed), which rebuilds the tasks that did not travel.  A header of its own so that
// both translation units of libhao.so can include it (hao_grid.cuh's kernels live in hao_capi.hip's).
#pragma once
#include "hao_common.cuh"

// the pair of overlap z and grid window w (helpers.ed_tasks_grid); false: the overlap does not cover the window, or the pair is empty / not expressible
__host__ __device__ __forceinline__ bool hao_grid_pair(const hao_ovlp_t &z, uint32_t w, uint32_t wl, uint32_t thre, uint32_t nword, const uint32_t *len, hao_ed_task_t *t)
{
	const int64_t xs = z.x_pos_s, xe = z.x_pos_e, g0 = (int64_t)w * wl;
	if (xs / wl > (int64_t)w || xe / wl < (int64_t)w) return false;
	const int64_t ws = g0 > xs ? g0 : xs, we = g0 + wl - 1 < xe ? g0 + wl - 1 : xe, tn = we + 1 - ws, tl = len[z.y_id];
	int64_t p0 = (int64_t)z.y_pos_s + (ws - xs) - (int64_t)thre, p1 = p0 + tn + 2 * (int64_t)thre, ad = 0;
	if (p0 < 0) { ad = -p0 < 2 * (int64_t)thre ? -p0 : 2 * (int64_t)thre; p0 = 0; }
	if (p1 > tl) p1 = tl;
	if (p1 <= p0 || tn <= 0) return false;
	// bands of more than one word: the final scan reads bit i of VP / VN for i < p_len - t_len + abs_diag, which must lie inside the band's words (hao_window_ed_batch refuses such a task)
	if (nword > 1 && (p1 - p0) - tn + ad > 64 * (int64_t)nword) return false;
	t->p_rid = z.y_id; t->p_pos = (uint32_t)p0; t->p_len = (uint32_t)(p1 - p0); t->p_rev = z.y_pos_strand;
	t->t_rid = z.x_id; t->t_pos = (uint32_t)ws; t->t_len = (uint32_t)tn; t->t_rev = 0; t->thre = thre; t->abs_diag = (uint32_t)ad;
	return true;
}

// a pair of the delivery path's list (HAO_DELIVER_ED): the overlap (index in the batch's final ol->list) and the grid window of its query read - 8 bytes
// instead of the 40 of its hao_ed_task_t, which the alignment kernel rebuilds with hao_grid_pair
struct hao_ed_pair { uint32_t ol, w; };

// ---- reference placement (align_hc_ed_post_extz, Correct.cpp:12951-13006; the same loop in align_ul_ed_post_extz :12900 and verify_window :382-559) ----
// The same grid windows, placed as the reference's correction pass places them: the target start on the diagonal of the nearest chained seed before the
// window (y_start_offset over the overlap's fake cigar, Hash_Table.h:165-189), one threshold per window from its length, admission and clipping by init_waln
// (Correct.cpp:764-779).  Shared like hao_grid_pair by the device's generators, the delivery path's alignment kernel and the host decoder.
#define HAO_REF_NOSHIFT (-32768)      // a window whose start resolves to no cigar entry (or whose shift does not fit 16 bits): no pair, counted as unresolved

// the thresholds of windows of 0 .. wl bases: (int64_t)(q_l * e_rate), Adjust_Threshold (Correct.h:46), capped at THRESHOLD_MAX_SIZE = 31 (Hash_Table.h:24).
// Host only and in double, as the reference computes it; the kernels read the table.
static inline void hao_ref_thre_table(uint32_t wl, double e_rate, uint8_t *tab)
{
	for (uint32_t q = 0; q <= wl; ++q) {
		int64_t t = (int64_t)((int64_t)q * e_rate);
		if (t == 0 && q >= 4) t = 1;
		tab[q] = (uint8_t)(t > 31 ? 31 : t);
	}
}

// get_fake_gap_shift (Hash_Table.cpp:69-87) of a resident 8-byte entry (site << 32 | |shift| << 1 | sign)
__host__ __device__ __forceinline__ int32_t hao_fc_shift(uint64_t e) { const uint32_t v = (uint32_t)e; return (v & 1u) ? -(int32_t)(v >> 1) : (int32_t)(v >> 1); }

// y_start_offset(q_s, cigar) (Hash_Table.h:165-189) over n entries whose sites ascend: a site equal to the last entry's takes the last shift, otherwise the
// last entry with site <= q_s (the reference returns entry i - 1 of the first i with q_s < site[i]); HAO_REF_NOSHIFT where the reference would exit
__host__ __device__ __forceinline__ int32_t hao_ref_shift(const uint64_t *fc, uint32_t n, int64_t q_s)
{
	if (n == 0) return HAO_REF_NOSHIFT;
	int32_t sh;
	if (q_s == (int64_t)(fc[n - 1] >> 32)) sh = hao_fc_shift(fc[n - 1]);
	else {
		uint32_t lo = 0, hi = n;      // first i with q_s < site[i]
		while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (q_s < (int64_t)(fc[m] >> 32)) hi = m; else lo = m + 1; }
		if (lo == 0 || lo == n) return HAO_REF_NOSHIFT;
		sh = hao_fc_shift(fc[lo - 1]);
	}
	return sh > 32767 || sh <= HAO_REF_NOSHIFT ? HAO_REF_NOSHIFT : sh;
}

// the pair of overlap z and grid window w in reference placement: shift = hao_ref_shift at the window's start, tab = hao_ref_thre_table, tl = the target's
// length.  false: the overlap does not cover the window or init_waln refuses it.  p_pos / p_len = init_waln's r_s / r_l, abs_diag = its aux_beg (aux_end is
// w_l - r_l - aux_beg: the pattern simply ends early)
__host__ __device__ __forceinline__ bool hao_ref_pair(const hao_ovlp_t &z, uint32_t w, uint32_t wl, int32_t shift, const uint8_t *tab, uint32_t tl, hao_ed_task_t *t)
{
	const int64_t xs = z.x_pos_s, xe = z.x_pos_e, g0 = (int64_t)w * wl;
	if (xs / wl > (int64_t)w || xe / wl < (int64_t)w || shift == HAO_REF_NOSHIFT) return false;
	const int64_t qs = g0 > xs ? g0 : xs, qe = g0 + wl - 1 < xe ? g0 + wl - 1 : xe, ql = qe + 1 - qs, l = tl;
	if (ql <= 0) return false;
	const int64_t thre = tab[ql], wln = ql + 2 * thre, s = (qs - xs) + (int64_t)z.y_pos_s + shift;
	if (s < 0 || s >= l || l - s + 2 * thre + 31 < wln) return false;
	int64_t rs = s - thre, rl = l - rs, ab = 0;
	if (rl > wln) rl = wln;
	if (rs < 0) { ab = -rs; rs = 0; rl -= ab; }
	t->p_rid = z.y_id; t->p_pos = (uint32_t)rs; t->p_len = (uint32_t)rl; t->p_rev = z.y_pos_strand;
	t->t_rid = z.x_id; t->t_pos = (uint32_t)qs; t->t_len = (uint32_t)ql; t->t_rev = 0; t->thre = (uint32_t)thre; t->abs_diag = (uint32_t)ab;
	return true;
}

// ---- rescue of unaligned windows (push_hc_wlst_exz, Correct.cpp:12776-12836, through aln_wlst_adv_exz :4057-4131; hao_rescue.cuh) ----
// the threshold of a rescue alignment of a window of ql bases: double_error_threshold(get_init_err_thres(ql, e_rate, w_l, 31), ql) (:917, :1042) over the
// table of hao_ref_thre_table (whose entries are get_init_err_thres' for ql < w_l)
__host__ __device__ __forceinline__ uint32_t hao_rescue_thre(uint32_t ql, uint32_t wl, const uint8_t *tab)
{
	uint32_t t = ql >= wl ? 31u : tab[ql];
	if (t == 0 && ql >= 4) t = 1;
	t *= 2;
	if (ql >= 300 && t < 31) t = 31;
	return t > 31 ? 31 : t;
}
// grid window w of overlap z clipped to the overlap: its first base and its length (0: not covered)
__host__ __device__ __forceinline__ void hao_ref_window(const hao_ovlp_t &z, uint32_t w, uint32_t wl, int64_t *qs, int64_t *ql)
{
	const int64_t xs = z.x_pos_s, xe = z.x_pos_e, g0 = (int64_t)w * wl;
	*qs = g0 > xs ? g0 : xs; const int64_t qe = g0 + wl - 1 < xe ? g0 + wl - 1 : xe; *ql = qe + 1 - *qs;
	if (*ql < 0) *ql = 0;
}
// the task of a rescue alignment: grid window w of overlap z against the target from toff on (aln_wlst_adv_exz's t_s: the end of the window before + 1 in a
// forward run, the start of the window after - the window's length in a backward run), init_waln with the rescue threshold.  false: init_waln refuses it, or
// the pattern is too short (t_pri_l + thres < ql).  p_pos = the r_s the window record's y_start / y_end are counted from.  Shared by the rescue kernel, the
// host decoder and the tests.
__host__ __device__ __forceinline__ bool hao_rescue_pair(const hao_ovlp_t &z, uint32_t w, uint32_t wl, int64_t toff, const uint8_t *tab, uint32_t tl, hao_ed_task_t *t)
{
	int64_t qs, ql; hao_ref_window(z, w, wl, &qs, &ql);
	if (ql <= 0) return false;
	const int64_t thre = hao_rescue_thre((uint32_t)ql, wl, tab), wln = ql + 2 * thre, s = toff, l = tl;
	if (s < 0 || s >= l || l - s + 2 * thre + 31 < wln) return false;
	int64_t rs = s - thre, rl = l - rs, ab = 0;
	if (rl > wln) rl = wln;
	if (rs < 0) { ab = -rs; rs = 0; rl -= ab; }
	if (rl + thre < ql) return false;
	t->p_rid = z.y_id; t->p_pos = (uint32_t)rs; t->p_len = (uint32_t)rl; t->p_rev = z.y_pos_strand;
	t->t_rid = z.x_id; t->t_pos = (uint32_t)qs; t->t_len = (uint32_t)ql; t->t_rev = 0; t->thre = (uint32_t)thre; t->abs_diag = (uint32_t)ab;
	return true;
}
// per-overlap result of the rescue stage and a window record (hao.h: hao_rescue_ovlp_t, hao_rescue_win_t)
struct hao_rs_ovlp { uint16_t verdict, flags; uint32_t exit_win, align_length, n_rescued; };
struct hao_rs_win { int32_t y_start, y_end; uint32_t win, info; };
// the rescue stage's state of one overlap (hao_rescue.cuh runs it; here because the context holds a buffer of them).  k: the aligned window (slot) being pushed;
// j: the window the pending alignment is for; last: slot of w_list's last entry (-1: empty); cs: first slot the backward run may reach; toff: target offset of
// the pending alignment; a_*: window k's record (y_start is its r_s until it is traced)
struct hao_rs_state { uint32_t ol; int32_t phase, k, j, last, cs; uint32_t aflags; int32_t a_ys, a_ye, a_err; int64_t toff; uint64_t base; };
// device-only bits of a record's info word, stripped before a record leaves the library: the slot holds a record; on an anchor's record, a traced step of its
// backward run fell outside the traced domain (becomes HAO_RESCUE_UNTRACED in the overlap's flags)
#define HAO_RS_VALID 0x80000000u
#define HAO_RS_UNTRACED_BIT (1u << 19)
// a record's plan in the window-list stage (hao_wlist.cuh; here because the context holds a buffer of them): overlap, slot | source << 28 | needs-a-sweep bit, target offset of a rescue task
struct hao_wl_plan { uint32_t ol, ks; int64_t toff; };
// the threshold ladder (hao_ladder.cuh; here because the context holds a buffer of them): the coordinates an attempt hands the aligner, per slot of a round's open list
struct hao_ld_coord { int32_t qs, qe, ts, te, aux; uint32_t flags; };

// what the reference-placed generators read beside the overlaps: the covered windows of overlap i are slots win_off[i] .. win_off[i + 1] of shift[] (slot
// k = grid window x_pos_s / window + k), tab = the threshold table; all null in diagonal placement
struct hao_ref_args { const uint64_t *win_off; const int16_t *shift; const uint8_t *tab; };
// (placement of a grid stage: HAO_PLACE_DIAG / HAO_PLACE_REF, hao.h)
// per-overlap summary of a reference-placed stage (hao.h: hao_ed_ovlp_t)
struct hao_ed_ovlp_sum { uint32_t n_win, n_aligned, aligned_bases, err_sum; };
