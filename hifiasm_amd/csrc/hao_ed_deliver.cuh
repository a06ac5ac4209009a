// f3 in the streaming pass (HAO_DELIVER_ED, hao_overlap_batch_async): the distance-only window alignment of every grid pair of a batch, written straight into
// the compact records that travel with the batch - one error byte (0xff: no alignment within thre) and a 16-bit pattern end (0xffff: -1) per pair.
// The pair list is (overlap, window) in text order (ed_grid_kernel<ED_GRID_PAIRS>, hao_grid.cuh); each lane rebuilds its task from the batch's ol->list with
// hao_grid_pair - the same function the blocking path's generator and the host decoder (hao_unpack_ed) use - so no 40-byte task record is written to or read
// back from HBM.  The sweep is hao_al_kernel's (hao_al_tile_sweep: 64 neighbours per wave, their texts staged in LDS), so the results are those of
// hao_window_ed_grid bit for bit.  One launch per batch; WT = the band word of the configured threshold (one to four 64-bit words).
#pragma once
#include "hao_align.cuh"
#include "hao_grid_pair.cuh"

// PLACE = HAO_PLACE_REF (hao_deliver_ed_config_ref): the lane rebuilds its task with hao_ref_pair from the shifts and the threshold table (A), and an
// aligned pair also leaves its error byte in its overlap's CSR slot (werr, preset to 0xff) for the per-overlap summary (ed_ref_summary_kernel, hao_grid.cuh)
template<typename WT, int PLACE = HAO_PLACE_DIAG>
__global__ __launch_bounds__(256) void hao_ed_deliver_kernel(hao_ed_reads R, const hao_ovlp_t *ol, const hao_ed_pair *pairs, uint64_t n, uint32_t wl, uint32_t thre,
		uint8_t *err, uint16_t *pe, hao_ref_args A = hao_ref_args{nullptr, nullptr, nullptr}, uint8_t *werr = nullptr)
{
	__shared__ uint8_t s_text[4][HAO_AL_CH];
	const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t slot = ((uint64_t)blockIdx.x * 4 + wv) * 64 + lane;
	hao_ed_task_t T; T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	bool mine = false; uint64_t ws = 0;
	if (slot < n) {      // (always true: the generator kept exactly these pairs)
		const hao_ed_pair q = pairs[slot];
		if (PLACE == HAO_PLACE_DIAG) mine = hao_grid_pair(ol[q.ol], q.w, wl, thre, hao_al_nword(thre), R.len, &T);
		else { const hao_ovlp_t z = ol[q.ol]; ws = A.win_off[q.ol] + (q.w - z.x_pos_s / wl); mine = hao_ref_pair(z, q.w, wl, A.shift[ws], A.tab, R.len[z.y_id], &T); }
	}
	hao_al_state<WT> S;
	hao_al_tile_sweep<WT, HAO_AL_ED, false>(R, T, mine, S, s_text[wv], lane, (uint64_t*)nullptr, 0);
	if (slot < n) {
		hao_trace_result_t res;
		hao_al_finish<WT, HAO_AL_ED, false>(S, T, res, (const uint64_t*)nullptr, 0, (uint16_t*)nullptr, 0);
		// err <= thre <= 127 when there is an alignment; pe < p_len <= window + 2 thre < 65535 (hao_deliver_ed_config)
		err[slot] = res.err == HAO_AL_NONE ? (uint8_t)0xff : (uint8_t)res.err;
		pe[slot] = res.pe < 0 ? (uint16_t)0xffff : (uint16_t)res.pe;
		if (PLACE == HAO_PLACE_REF && mine && res.err != HAO_AL_NONE) werr[ws] = (uint8_t)res.err;
	}
}
