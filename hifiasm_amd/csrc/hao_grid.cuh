// f3 on the device end to end: the window / candidate pairs of a batch, generated ON THE DEVICE from the batch's final ol->list on the reference's fixed window grid
// (windows of WINDOW = 375 query bases starting at multiples of WINDOW: Hash_Table.h:9, Correct.cpp:5645, 5993; a pair per overlap and grid window it covers, the
// window clipped to the overlap at its two ends, the pattern = the target interval on the overlap's diagonal padded by thre on both sides and clipped at the read ends,
// abs_diag = the bases clipped at the start: Correct.cpp:3897's call of ed_band_cal_semi_64_w_absent_diag without the fake-cigar shift - the same pairs as
// tests/helpers.py ed_tasks_grid).  Tasks come out in TEXT order - (query read, grid window, position in ol->list) - which is the order the window-alignment kernels
// want (hao_align.cuh: a wave takes 64 neighbours, which share their text), so nothing is uploaded, sorted or downloaded: two counting kernels, two scans, one fill.
#pragma once
#include "hao_common.cuh"
#include "hao_grid_pair.cuh"      // (hao_grid_pair: one pair of the grid)

__global__ void ed_grid_nwin_kernel(const uint32_t *len, uint64_t rid_lo, uint64_t n, uint32_t wl, uint64_t *nwin)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r > n) return;
	nwin[r] = r < n ? (len[rid_lo + r] + wl - 1) / wl : 0;
}

// one wave per read of the batch, a lane per grid window (64 at a time); OUT = ED_GRID_COUNT: pairs per window -> cnt[wbase[r] + w]; ED_GRID_TASKS: the pairs themselves at
// off[wbase[r] + w] ..; ED_GRID_PAIRS: the same places as (overlap, window) (the delivery path, HAO_DELIVER_ED: its alignment kernel rebuilds the tasks in the lane)
enum { ED_GRID_COUNT = 0, ED_GRID_TASKS = 1, ED_GRID_PAIRS = 2 };
template<int OUT>
__global__ __launch_bounds__(256) void ed_grid_kernel(const hao_ovlp_t *ol, const uint64_t *fin_off, const uint32_t *len, uint64_t rid_lo, uint64_t n, uint32_t wl, uint32_t thre, uint32_t nword,
		const uint64_t *wbase, uint64_t *cnt_or_off, hao_ed_task_t *tasks, hao_ed_pair *pairs)
{
	constexpr bool FILL = OUT != ED_GRID_COUNT;
	const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (r >= n) return;
	const int lane = hao_lane();
	const uint64_t o0 = fin_off[r], o1 = fin_off[r + 1], wb = wbase[r]; const uint32_t nw = (uint32_t)(wbase[r + 1] - wb);
	for (uint32_t w = lane; w < nw; w += 64) {
		uint64_t k = 0; const uint64_t at = FILL ? cnt_or_off[wb + w] : 0;
		for (uint64_t i = o0; i < o1; ++i) {
			hao_ed_task_t t;
			if (!hao_grid_pair(ol[i], w, wl, thre, nword, len, &t)) continue;
			if (OUT == ED_GRID_TASKS) tasks[at + k] = t;
			if (OUT == ED_GRID_PAIRS) { hao_ed_pair q; q.ol = (uint32_t)i; q.w = w; pairs[at + k] = q; }
			++k;
		}
		if (!FILL) cnt_or_off[wb + w] = k;
	}
}

// the delivery path's per-read pair offsets: pairs of read r start at woff[wbase[r]] (r = 0 .. n; woff = exclusive scan of the per-window counts)
__global__ void ed_read_off_kernel(const uint64_t *wbase, const uint64_t *woff, uint64_t n, uint64_t *ed_off)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r <= n) ed_off[r] = woff[wbase[r]];
}
