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
