// f3 with traceback on the device grid (hao_window_trace_grid, HAO_DELIVER_TRACE): the semi-global traced alignment
// (ed_band_cal_semi_64_w_absent_diag_trace + gen_trace, Levenshtein_distance.h:3778-3848, 903-985; called after the distance-only call at Correct.cpp:3897-3911)
// of the grid pairs whose distance-only result aligned and whose band covers the pattern.  The input is the pair list (overlap, window) and the error bytes
// the distance-only stage already wrote (hao_ed_deliver.cuh); no task record is stored: every kernel rebuilds its pair's task in the lane with hao_grid_pair.
//   1. hao_tg_flag_kernel: which pairs get a cigar, and an upper bound of their cigar entries (the compact array's size before any walk has run);
//   2. rocprim::select of the flagged pair indices (text order kept: a wave still takes 64 neighbours that mostly share one text);
//   3. hao_trace_grid_kernel: the sweep with three words per band word and column (hao_al_keep3: D0, VP, VN - HP / HN are derived in the walk), the
//      walk into a row of 2 thre + 3 entries, per-pair ps and entry count;
//   4. per slice of the column scratch: a scan of the counts and hao_tg_compact_kernel, which copies the rows into the compact (CSR) cigar array.
#pragma once
#include "hao_align.cuh"
#include "hao_grid_pair.cuh"

// the semi-global traced domain of a task (hao_window_trace_batch accepts no other for HAO_ALIGN_SEMI): 0 <= p_len - t_len + abs_diag <= 2 thre, t_len > abs_diag
HAO_AL_FN bool hao_tg_semi_domain(const hao_ed_task_t &t)
{
	const int64_t ai = (int64_t)t.p_len - (int64_t)t.t_len + (int64_t)t.abs_diag;
	return ai >= 0 && ai <= 2 * (int64_t)t.thre && t.t_len > t.abs_diag && t.abs_diag <= 2 * t.thre;
}
// cigar entries of a semi-global walk that ends with error err: each step that is not a match lowers the error by one, so there are at most err of them and
// 2 err + 1 runs; push_trace splits a run at 0x3fff, which adds at most (steps) / 0x3fff entries, and steps <= p_len + t_len
HAO_AL_FN uint64_t hao_tg_bound(const hao_ed_task_t &t, uint32_t err) { return 2 * (uint64_t)err + 1 + ((uint64_t)t.p_len + t.t_len) / 0x3fff; }

// want[i] = pair i gets a cigar; *bound += the cigar-entry bound of those that do; *untraced += the aligned pairs that do not
__global__ __launch_bounds__(256) void hao_tg_flag_kernel(const uint32_t *len, const hao_ovlp_t *ol, const hao_ed_pair *pairs, uint64_t n, uint32_t wl, uint32_t thre,
		const uint8_t *err, uint8_t *want, unsigned long long *ctr)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long b = 0, u = 0;
	if (i < n) {
		uint8_t w = 0;
		if (err[i] != 0xff) {
			const hao_ed_pair q = pairs[i]; hao_ed_task_t t;
			if (hao_grid_pair(ol[q.ol], q.w, wl, thre, hao_al_nword(thre), len, &t) && hao_tg_semi_domain(t)) { w = 1; b = hao_tg_bound(t, err[i]); }
			else u = 1;
		}
		want[i] = w;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) { b += __shfl_xor(b, d); u += __shfl_xor(u, d); }
	if ((threadIdx.x & 63) == 0) { if (b) atomicAdd(ctr, b); if (u) atomicAdd(ctr + 1, u); }
}
struct hao_tg_flagged { const uint8_t *f; __host__ __device__ bool operator()(const uint32_t &i) const { return f[i] != 0; } };

// One lane per selected pair of the slice sel[0 .. m): the traced sweep over the three-word columns in path[] (slot = lane's place in the slice, `stride` slots
// per row), the walk into rows[slot * cap ..], and the pair's ps / entry count at its place in the grid (ps16 / ncig16, indexed by pair) and in cnt[slot].
template<typename WT>
__global__ __launch_bounds__(256) void hao_trace_grid_kernel(hao_ed_reads R, const hao_ovlp_t *ol, const hao_ed_pair *pairs, const uint32_t *sel, uint64_t m, uint32_t wl, uint32_t thre,
		uint64_t *path, uint64_t stride, uint16_t *rows, uint32_t cap, uint64_t *cnt, uint16_t *ps16, uint16_t *ncig16)
{
	__shared__ uint8_t s_text[4][HAO_AL_CH];
	const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t slot = ((uint64_t)blockIdx.x * 4 + wv) * 64 + lane;
	hao_ed_task_t T; T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	bool mine = false; uint32_t pi = 0;
	if (slot < m) { pi = sel[slot]; const hao_ed_pair q = pairs[pi]; mine = hao_grid_pair(ol[q.ol], q.w, wl, thre, hao_al_nword(thre), R.len, &T); }      // (always true: the flag kernel kept these)
	uint64_t *col = path + slot;
	hao_al_state<WT> S;
	hao_al_tile_sweep<WT, HAO_AL_SEMI, true, 3>(R, T, mine, S, s_text[wv], lane, col, stride);
	if (slot < m) {
		hao_trace_result_t res; res.ps = -1; res.n_cigar = 0;
		const bool tr = mine && hao_al_finish<WT, HAO_AL_SEMI, true, 3>(S, T, res, col, stride, rows + slot * cap, cap);
		// n_cigar <= 2 thre + 3 = cap (include/hao.h), ps < p_len <= window + 2 thre < 65535 (hao_window_trace_grid / hao_deliver_ed_config)
		const uint32_t nc = tr ? (uint32_t)res.n_cigar : 0u;
		cnt[slot] = nc; ps16[pi] = tr ? (uint16_t)res.ps : (uint16_t)0xffff; ncig16[pi] = (uint16_t)nc;
	}
}

// the slice's rows into the compact array: loc = exclusive scan of the slice's counts (loc[m] = their sum), off = the traced pairs' offsets into cig (off[0] of
// the slice was written by the slice before it, or is 0); entries past cig_cap are not written (the bound of hao_tg_flag_kernel rules that out)
__global__ void hao_tg_compact_kernel(const uint16_t *rows, uint32_t cap, const uint64_t *loc, uint64_t m, uint64_t *off, uint16_t *cig, uint64_t cig_cap)
{
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= m) return;
	const uint64_t base = off[0], a = base + loc[k], nk = loc[k + 1] - loc[k];
	off[k + 1] = base + loc[k + 1];
	for (uint64_t j = 0; j < nk && j < cap && a + j < cig_cap; ++j) cig[a + j] = rows[k * cap + j];
}

// out[r] = the offset in cig of the first entry of pair at[r] or later (at = NULL: pair r), r = 0 .. n: the traced pairs sel[] ascend, so it is off[] at
// the first of them at or after that pair
__global__ void hao_tg_off_kernel(const uint64_t *at, uint64_t n, const uint32_t *sel, uint64_t n_sel, const uint64_t *off, uint64_t *out)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r > n) return;
	const uint64_t p = at ? at[r] : r;
	uint64_t lo = 0, hi = n_sel;
	while (lo < hi) { const uint64_t md = (lo + hi) >> 1; if ((uint64_t)sel[md] < p) lo = md + 1; else hi = md; }
	out[r] = off[lo];
}

// the blocking path's fetch: every grid pair's task rebuilt from the pair list, and its result widened (err INT32_MAX / pe -1 without an alignment; ps -1
// without a cigar; ts = 0, te = t_len - 1)
__global__ void hao_tg_expand_kernel(const uint32_t *len, const hao_ovlp_t *ol, const hao_ed_pair *pairs, uint64_t n, uint32_t wl, uint32_t thre,
		const uint8_t *err, const uint16_t *pe, const uint16_t *ps16, const uint16_t *ncig16, hao_ed_task_t *tasks, hao_trace_result_t *res)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const hao_ed_pair q = pairs[i]; hao_ed_task_t t;
	if (!hao_grid_pair(ol[q.ol], q.w, wl, thre, hao_al_nword(thre), len, &t)) { t.p_rid = t.p_pos = t.p_len = t.p_rev = t.t_rid = t.t_pos = t.t_len = t.t_rev = t.thre = t.abs_diag = 0; }
	hao_trace_result_t r;
	r.err = err[i] == 0xff ? HAO_AL_NONE : (int32_t)err[i]; r.pe = pe[i] == 0xffff ? -1 : (int32_t)pe[i];
	r.ps = ps16[i] == 0xffff ? -1 : (int32_t)ps16[i]; r.ts = 0; r.te = (int32_t)t.t_len - 1; r.n_cigar = (int32_t)ncig16[i];
	tasks[i] = t; res[i] = r;
}
