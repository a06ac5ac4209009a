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
// PLACE = HAO_PLACE_REF: the pairs of reference placement (hao_ref_pair; A = the shifts of ed_ref_shift_kernel and the threshold table; thre / nword unused);
// there ED_GRID_TASKS writes the (overlap, window) list too (hao_window_ed_ref needs both)
template<int OUT, int PLACE = HAO_PLACE_DIAG>
__global__ __launch_bounds__(256) void ed_grid_kernel(const hao_ovlp_t *ol, const uint64_t *fin_off, const uint32_t *len, uint64_t rid_lo, uint64_t n, uint32_t wl, uint32_t thre, uint32_t nword,
		const uint64_t *wbase, uint64_t *cnt_or_off, hao_ed_task_t *tasks, hao_ed_pair *pairs, hao_ref_args A = hao_ref_args{nullptr, nullptr, nullptr})
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
			if (PLACE == HAO_PLACE_DIAG) { if (!hao_grid_pair(ol[i], w, wl, thre, nword, len, &t)) continue; }
			else {
				const hao_ovlp_t z = ol[i]; const uint32_t w0 = z.x_pos_s / wl;
				if (w0 > w || z.x_pos_e / wl < w || z.x_pos_e < z.x_pos_s) continue;      // (before the shift is read: slot w - w0 exists only for a covered window)
				if (!hao_ref_pair(z, w, wl, A.shift[A.win_off[i] + (w - w0)], A.tab, len[z.y_id], &t)) continue;
			}
			if (OUT == ED_GRID_TASKS) tasks[at + k] = t;
			if (OUT == ED_GRID_PAIRS || (OUT == ED_GRID_TASKS && PLACE == HAO_PLACE_REF)) { hao_ed_pair q; q.ol = (uint32_t)i; q.w = w; pairs[at + k] = q; }      // (the blocking reference-placed call keeps both: one fill pass)
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

// ---- reference placement: the shift of every (overlap, covered window), in a pass of its own ----
// covered windows per overlap (get_num_wins, Correct.cpp:782-787): x_pos_e / wl - x_pos_s / wl + 1; entry n_ol = 0 for the scan
__global__ void ed_ref_nwin_kernel(const hao_ovlp_t *ol, uint64_t n_ol, uint32_t wl, uint64_t *cnt)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n_ol) return;
	cnt[i] = i < n_ol && ol[i].x_pos_e >= ol[i].x_pos_s ? (uint64_t)(ol[i].x_pos_e / wl - ol[i].x_pos_s / wl + 1) : 0;      // (an inverted record covers nothing, as hao_grid_pair has it)
}

// 16 lanes per overlap, a lane per covered window (16 at a time): y_start_offset of the window's start over the overlap's resident fake cigar
// (8-byte entries, fc_off[i] .. + fc_len) -> shift[win_off[i] + k].  Why this shape: an overlap covers x span / window + 1 windows - at most ~20 for 15 kb
// HiFi reads at 775, ~130 for 50 kb ONT reads at 375 - and its cigar has tens of entries, so a whole wave per overlap would idle three quarters of its
// lanes on HiFi while a lane per overlap would walk cigar and windows serially with 2-byte stores 2 * n_win bytes apart.  With 16 lanes the stores of a
// group are contiguous (32 bytes per step), the entries are read by all 16 lanes from the same few cache lines, and the search is log2(fc_len) dependent
// loads instead of a serial merge.  Unresolved windows (the reference would exit there) get HAO_REF_NOSHIFT and are counted.
__global__ __launch_bounds__(256) void ed_ref_shift_kernel(const hao_ovlp_t *ol, uint64_t n_ol, const uint64_t *fc, const uint64_t *fc_off, uint32_t wl, const uint64_t *win_off,
		int16_t *shift, unsigned long long *unresolved)
{
	const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; const uint32_t sub = threadIdx.x & 15;
	if (i >= n_ol) return;
	const hao_ovlp_t z = ol[i];
	const uint64_t s0 = win_off[i]; const uint32_t nw = (uint32_t)(win_off[i + 1] - s0), w0 = z.x_pos_s / wl;
	const uint64_t *e = fc + fc_off[i];
	uint32_t bad = 0;
	for (uint32_t k = sub; k < nw; k += 16) {
		const int64_t g0 = (int64_t)(w0 + k) * wl, qs = g0 > (int64_t)z.x_pos_s ? g0 : (int64_t)z.x_pos_s;
		const int32_t sh = hao_ref_shift(e, z.fc_len, qs);
		shift[s0 + k] = (int16_t)sh;
		bad += sh == HAO_REF_NOSHIFT;
	}
	if (bad) atomicAdd(unresolved, (unsigned long long)bad);
}

// (err, pair) of an aligned pair -> the error byte of its CSR slot (0xff: no pair or no alignment; the slots are preset to 0xff); blocking path
__global__ void ed_ref_scatter_kernel(const hao_ovlp_t *ol, const hao_ed_pair *pairs, const hao_ed_result_t *res, uint64_t n, uint32_t wl, const uint64_t *win_off, uint8_t *werr)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const hao_ed_pair q = pairs[p]; const int32_t e = res[p].err;
	if (e != 0x7fffffff) werr[win_off[q.ol] + (q.w - ol[q.ol].x_pos_s / wl)] = (uint8_t)e;      // (err <= thre <= 31)
}

// per-overlap summary over the overlap's CSR slots: windows covered, windows aligned, the sum of their lengths (the align_length align_hc_ed_post_extz
// accumulates before its rescue step) and of their errors.  A thread per overlap: integer sums over at most a few hundred bytes
__global__ void ed_ref_summary_kernel(const hao_ovlp_t *ol, uint64_t n_ol, uint32_t wl, const uint64_t *win_off, const uint8_t *werr, hao_ed_ovlp_sum *out)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_ol) return;
	const hao_ovlp_t z = ol[i];
	const uint64_t s0 = win_off[i]; const uint32_t nw = (uint32_t)(win_off[i + 1] - s0), w0 = z.x_pos_s / wl;
	hao_ed_ovlp_sum s; s.n_win = nw; s.n_aligned = s.aligned_bases = s.err_sum = 0;
	for (uint32_t k = 0; k < nw; ++k) {
		const uint8_t e = werr[s0 + k];
		if (e == 0xff) continue;
		const int64_t g0 = (int64_t)(w0 + k) * wl, qs = g0 > (int64_t)z.x_pos_s ? g0 : (int64_t)z.x_pos_s, qe = g0 + wl - 1 < (int64_t)z.x_pos_e ? g0 + wl - 1 : (int64_t)z.x_pos_e;
		++s.n_aligned; s.aligned_bases += (uint32_t)(qe + 1 - qs); s.err_sum += e;
	}
	out[i] = s;
}
