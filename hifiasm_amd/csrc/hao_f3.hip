// libhao.so, second translation unit: f3, the window-alignment batches (hao_align.cuh) - 36 instantiations of hao_al_kernel (five modes, with and without
// traceback, bands of one to four words), the nine of the cooperative kernel for wider bands (hao_align_coop.cuh), the four of the delivery path's kernel (hao_ed_deliver.cuh) and the four of the traced grid stage's
// (hao_trace_grid.cuh) that the rest of the library reaches through hao_al_ed_resident / hao_al_ed_deliver / hao_al_trace_grid only, the rescue stage
// (hao_rescue.cuh, hao_al_rescue), the window lists (hao_wlist.cuh, hao_al_wlist) and the threshold ladder (hao_ladder.cuh, hao_al_ladder); compiled beside
// hao_capi.hip (hifiasm_amd/build.py).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "hao_ctx.hpp"
#include "hao_comm.hpp"
#include "hao_align.cuh"
#include "hao_align_coop.cuh"
#include "hao_ed_deliver.cuh"
#include "hao_trace_grid.cuh"
#include "hao_rescue.cuh"
#include "hao_wlist.cuh"
#include "hao_ladder.cuh"

// ---- the choices every stage makes, each written once ----
// f(hao_type<WT>{}) with the band vector of nword 64-bit words (one to four: the callers hold wider bands off)
template<typename T> struct hao_type { using type = T; };
template<typename F> static void hao_by_nword(uint32_t nword, F &&f)
{
	if (nword == 1) f(hao_type<uint64_t>{}); else if (nword == 2) f(hao_type<hao_u128>{}); else if (nword == 3) f(hao_type<hao_wide<3> >{}); else f(hao_type<hao_wide<4> >{});
}
// f(M), decltype(M)::value = hao_align.cuh's MODE of a traced mode of include/hao.h (HAO_ALIGN_*, which the entry points have checked)
template<typename F> static int hao_by_mode(int mode, F &&f)
{
	if (mode == HAO_ALIGN_EXT_FWD) return f(std::integral_constant<int, HAO_AL_EXT_FWD>{});
	if (mode == HAO_ALIGN_EXT_BWD) return f(std::integral_constant<int, HAO_AL_EXT_BWD>{});
	if (mode == HAO_ALIGN_SEMI) return f(std::integral_constant<int, HAO_AL_SEMI>{});
	return f(std::integral_constant<int, HAO_AL_GLOBAL>{});
}
// one sweep of hao_al_kernel over order[0 .. n): a launch per band word count set in `words` (bit nword - 1; a launch skips the tasks of the other widths, hao_al_mine)
template<int MODE, bool TRACE> static int hao_al_sweep(hao_ctx *c, const hao_ed_reads &R, const hao_ed_task_t *tasks, const uint32_t *order, uint64_t n, uint32_t words,
		uint64_t *path, uint64_t stride, hao_ed_result_t *out_ed, hao_trace_result_t *out_tr, uint8_t *want, uint16_t *dc, uint32_t cap)
{
	const dim3 g_((unsigned)((n + 255) / 256)), b_(256);
	for (uint32_t nw = 1; nw <= 4; ++nw) if (words >> (nw - 1) & 1u) {
		hao_by_nword(nw, [&](auto w) { hipLaunchKernelGGL((hao_al_kernel<typename decltype(w)::type, MODE, TRACE>), g_, b_, 0, c->stream, R, tasks, order, n, path, stride, out_ed, out_tr, want, dc, cap); });
		HAO_CHECK_LAUNCH();
	}
	return HAO_OK;
}
// al_order = the slots of al_k1 / al_i1 (key and index per task) by key: text order
static int hao_al_sort_by_text(hao_ctx *c, uint64_t n) { return hao_sort_pairs(c, c->al_k1.p, c->al_k2.p, c->al_i1.p, c->al_order.p, n, 64); }

// ---- f3 (hao_align.cuh): host side of the window-alignment batches ----
// tasks -> device, and their order by text window (hao_align.cuh: a wave takes 64 neighbours of that order, which mostly share one text)
static int hao_al_upload_sorted(hao_ctx *c, const hao_ed_task_t *tasks, uint64_t n)
{
	HIP_TRY(c->al_task.reserve(n)); HIP_TRY(c->al_k1.reserve(n)); HIP_TRY(c->al_k2.reserve(n)); HIP_TRY(c->al_i1.reserve(n)); HIP_TRY(c->al_order.reserve(n));
	HIP_TRY(hipMemcpyAsync(c->al_task.p, tasks, n * sizeof(hao_ed_task_t), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(hao_al_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->al_task.p, n, c->al_k1.p, c->al_i1.p); HAO_CHECK_LAUNCH();
	return hao_al_sort_by_text(c, n);
}
// the reads of a launch: the context's view (hao_ctx.hpp: hao_reads_view; the entry points refuse before they get here when there is none)
static hao_ed_reads hao_al_reads_of(hao_ctx *c)
{
	hao_read_view V; (void)hao_reads_view(c, &V);
	hao_ed_reads R; R.packed = V.packed; R.pk_off = V.pk_off; R.len = V.len; R.nsite_off = V.nsite_off; R.nsite = V.nsite;
	return R;
}

template<int MODE> static int hao_al_trace_run(hao_ctx *c, const hao_ed_reads &R, const hao_ed_task_t *dt, const uint32_t *order, uint64_t n, uint32_t words /* bit (nword - 1): some task's band has nword words */, uint64_t tn_max,
		hao_trace_result_t *dr, uint8_t *want, uint16_t *dc, uint32_t cap)
{
	// first sweep: no column storage, every task; decides which tasks end within their threshold (want[])
	if (int rc = hao_al_sweep<MODE, false>(c, R, dt, order, n, words, nullptr, 0, nullptr, dr, want, nullptr, 0u)) return rc;
	// the tasks of the second sweep, still in text order
	DevBuf<uint32_t> &sel = c->al_sel; DevBuf<uint64_t> &path = c->al_path; uint64_t n_sel = 0;
	HIP_TRY(sel.reserve(n + 1)); HIP_TRY(c->d_cursor.reserve(2));
	if (int rc = hao_select(c, order, hao_al_flagged{want}, sel.p, (uint64_t*)c->d_cursor.p, n)) return rc;
	HIP_TRY(hipMemcpyAsync(&n_sel, c->d_cursor.p, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (n_sel) {
		// second sweep: 40 bytes per band word, text column and selected pair, in slices whose columns fit the budget; then the traceback
		const uint64_t cw = 5 * (uint64_t)((words & 8u) ? 4 : (words & 4u) ? 3 : (words & 2u) ? 2 : 1);
		const uint64_t slice = hao_col_slice(c, n_sel, 8 * cw * tn_max);
		HIP_TRY(path.reserve(cw * tn_max * slice + 1));
		for (uint64_t lo = 0; lo < n_sel; lo += slice) {
			if (int rc = hao_al_sweep<MODE, true>(c, R, dt, sel.p + lo, std::min<uint64_t>(slice, n_sel - lo), words, path.p, slice, nullptr, dr, nullptr, dc, cap)) return rc; }
	}
	return HAO_OK;
}

// the distance-only window alignment over n tasks that already lie in c->al_task in text order (hao_window_ed_grid, hao_batch.hpp): results in c->al_res
int hao_al_ed_resident(hao_ctx *c, uint64_t n, uint32_t nword)
{
	HIP_TRY(c->al_order.reserve(n + 1)); HIP_TRY(c->al_res.reserve(n + 1));
	hipLaunchKernelGGL(hao_al_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->al_order.p, n); HAO_CHECK_LAUNCH();
	const hao_ed_reads R = hao_al_reads_of(c);
	return hao_al_sweep<HAO_AL_ED, false>(c, R, c->al_task.p, c->al_order.p, n, 1u << (nword - 1), nullptr, 0, c->al_res.p, nullptr, nullptr, nullptr, 0u);
}

// the delivery path's alignment (HAO_DELIVER_ED, hao_batch.hpp): n pairs (overlap, window) of the batch's ol->list in text order -> err[n] / pe[n] of the output set
// (place = HAO_PLACE_REF: the pairs of reference placement - thresholds <= 31, the one-word band - with the shifts and the threshold table in A and the CSR slots' error bytes in werr)
int hao_al_ed_deliver(hao_ctx *c, const hao_ovlp_t *ol, const hao_ed_pair *pairs, uint64_t n, uint32_t wl, uint32_t thre, uint8_t *err, uint16_t *pe, int place, hao_ref_args A, uint8_t *werr)
{
	const hao_ed_reads R = hao_al_reads_of(c);
	const dim3 g_((unsigned)((n + 255) / 256)), b_(256);
	const uint32_t nword = hao_al_nword(thre);
	if (place == HAO_PLACE_REF) hipLaunchKernelGGL((hao_ed_deliver_kernel<uint64_t, HAO_PLACE_REF>), g_, b_, 0, c->stream, R, ol, pairs, n, wl, thre, err, pe, A, werr);
	else hao_by_nword(nword, [&](auto w) { hipLaunchKernelGGL((hao_ed_deliver_kernel<typename decltype(w)::type>), g_, b_, 0, c->stream, R, ol, pairs, n, wl, thre, err, pe, hao_ref_args{nullptr, nullptr, nullptr}, (uint8_t*)nullptr); });
	HAO_CHECK_LAUNCH();
	return HAO_OK;
}

// the traced grid stage (hao_trace_grid.cuh; hao_window_trace_grid and HAO_DELIVER_TRACE, hao_batch.hpp): n pairs (overlap, window) of the batch's ol->list in
// text order and their distance-only error bytes -> ps16[n] / ncig16[n] (0xffff / 0 for the pairs without a cigar), the cigars of the traced pairs in pair
// order in cig, and c->tg.sel / c->tg.off (the traced pairs and their offsets into cig: hao_tg_off_kernel's input).  Two peeks at totals on the way.
int hao_al_trace_grid(hao_ctx *c, const hao_ovlp_t *ol, const hao_ed_pair *pairs, uint64_t n, uint32_t wl, uint32_t thre, const uint8_t *err,
		uint16_t *ps16, uint16_t *ncig16, DevBuf<uint16_t> &cig, uint64_t *n_traced, uint64_t *n_cigar, uint64_t *n_untraced)
{
	hao_ctx::TraceGrid &G = c->tg;
	*n_traced = 0; *n_cigar = 0; *n_untraced = 0;
	if (n == 0) { HIP_TRY(cig.reserve(1)); HIP_TRY(G.off.reserve(2)); HIP_TRY(hipMemsetAsync(G.off.p, 0, 8, c->stream)); c->timer.mark("trace_sel"); c->timer.mark("trace_align"); return HAO_OK; }
	const hao_ed_reads R = hao_al_reads_of(c);
	const uint32_t nword = hao_al_nword(thre), cap = 2 * thre + 3;
	HIP_TRY(G.want.reserve(n + 1)); HIP_TRY(G.sel.reserve(n + 1)); HIP_TRY(G.ctr.reserve(2)); HIP_TRY(c->d_cursor.reserve(2));
	HIP_TRY(hipMemsetAsync(ps16, 0xff, n * 2, c->stream)); HIP_TRY(hipMemsetAsync(ncig16, 0, n * 2, c->stream)); HIP_TRY(hipMemsetAsync(G.ctr.p, 0, 16, c->stream));
	hipLaunchKernelGGL(hao_tg_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, R.len, ol, pairs, n, wl, thre, err, G.want.p, G.ctr.p); HAO_CHECK_LAUNCH();
	const auto idx = rocprim::make_counting_iterator<uint32_t>(0);
	if (int rc = hao_select(c, idx, G.want.p, G.sel.p, (uint64_t*)c->d_cursor.p, n)) return rc;
	if (int rc = hao_peek(c, c->d_cursor.p, 1, PK_TG_TRACED)) return rc;
	if (int rc = hao_peek(c, G.ctr.p, 2, PK_TG_CTR)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t T = c->peeked(PK_TG_TRACED), bound = c->peeked(PK_TG_CTR);
	*n_untraced = c->peeked(PK_TG_CTR, 1);
	c->timer.mark("trace_sel");
	HIP_TRY(cig.reserve(bound + 1)); HIP_TRY(G.off.reserve(T + 2)); HIP_TRY(hipMemsetAsync(G.off.p, 0, 8, c->stream));      // (off[0] = 0: no traced pair, every offset is 0)
	if (T) {
		// column scratch: 24 bytes per band word, text column (t_len <= wl, + slot 0) and selected pair, in slices whose columns fit the budget (hao_col_slice); rows of 2 thre + 3 entries per slice
		const uint64_t cw = 3 * (uint64_t)nword, ncol = (uint64_t)wl + 1;
		const uint64_t slice = hao_col_slice(c, T, 8 * cw * ncol);
		HIP_TRY(G.path.reserve(cw * ncol * slice + 1)); HIP_TRY(G.rows.reserve(slice * cap + 1)); HIP_TRY(G.cnt.reserve(slice + 2)); HIP_TRY(G.loc.reserve(slice + 2));
		const dim3 b_(256);
		for (uint64_t lo = 0; lo < T; lo += slice) {
			const uint64_t m = std::min<uint64_t>(slice, T - lo);
			const dim3 g2((unsigned)((m + 255) / 256));
			HIP_TRY(hipMemsetAsync(G.cnt.p + m, 0, 8, c->stream));
			hao_by_nword(nword, [&](auto w) { hipLaunchKernelGGL((hao_trace_grid_kernel<typename decltype(w)::type>), g2, b_, 0, c->stream, R, ol, pairs, G.sel.p + lo, m, wl, thre, G.path.p, slice, G.rows.p, cap, G.cnt.p, ps16, ncig16); });
			HAO_CHECK_LAUNCH();
			if (int rc = hao_excl_scan_u64(c, G.cnt.p, G.loc.p, m + 1)) return rc;
			hipLaunchKernelGGL(hao_tg_compact_kernel, g2, b_, 0, c->stream, G.rows.p, cap, G.loc.p, m, G.off.p + lo, cig.p, (uint64_t)cig.cap); HAO_CHECK_LAUNCH();
		}
		if (int rc = hao_peek(c, G.off.p + T, 1, PK_TG_NCIG)) return rc;
		HIP_TRY(hipStreamSynchronize(c->stream));
		*n_cigar = c->peeked(PK_TG_NCIG);
		if (*n_cigar > bound) { hao_set_err(c, "traced grid stage: more cigar entries than their bound"); return HAO_EUNSUPP; }      // (hao_tg_bound rules it out)
	}
	c->timer.mark("trace_align");
	*n_traced = T;
	return HAO_OK;
}

// out[r] = offset into the traced grid stage's cigars of pair at[r] (at = NULL: of pair r), r = 0 .. n (hao_tg_off_kernel over c->tg.sel / c->tg.off)
int hao_al_trace_grid_off(hao_ctx *c, const uint64_t *at, uint64_t n, uint64_t n_traced, uint64_t *out)
{
	hipLaunchKernelGGL(hao_tg_off_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, at, n, c->tg.sel.p, n_traced, c->tg.off.p, out); HAO_CHECK_LAUNCH();
	return HAO_OK;
}

// hao_fetch_trace_grid's expansion: the first n pairs of hao_window_trace_grid's list as tasks and widened results (device buffers of n entries each)
int hao_al_trace_grid_expand(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n, hao_ed_task_t *tasks, hao_trace_result_t *res)
{
	if (n == 0) return HAO_OK;
	hipLaunchKernelGGL(hao_tg_expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, hao_al_reads_of(c).len, ol, c->tg_pairs.p, n, c->tg_wl, c->tg_thre,
		c->tg_err.p, c->tg_pe.p, c->tg_ps.p, c->tg_ncig16.p, tasks, res); HAO_CHECK_LAUNCH();
	return HAO_OK;
}

// the rescue stage (hao_rescue.cuh; hao_rescue_run, hao_batch.hpp): over the overlaps of a batch whose reference-placed ED stage has just run (io; at least one
// overlap) - its CSR, shifts and error bytes per slot in c->rf.  Leaves the per-overlap results in io.rs_ovlp, the records compacted by overlap in io.rs_off /
// io.rs_wins (in window order, the device-only bits stripped), the record regions in c->rs.rec (c->rs.rbase[i]: overlap i's) for the window lists, and the counts
// in c->rs_*.  Host round trips: one for the two sizes, one count per round, one for the number of records, one for the total.
int hao_al_rescue(hao_ctx *c, const hao_ref_io &io)
{
	hao_ctx::Rescue &G = c->rs; const hao_ovlp_t *ol = io.ol; const uint64_t n_ol = io.n_ol, n_pairs = io.n_pairs, n_slots = io.n_slots; const uint32_t wl = io.wl;
	hao_ref_args RA; RA.win_off = c->rf.woff.p; RA.shift = c->rf.shift.p; RA.tab = io.tab;
	HIP_TRY(G.rbase.reserve(n_ol + 1)); HIP_TRY(G.wpe.reserve(n_slots + 1)); HIP_TRY(G.ctr.reserve(8));
	HIP_TRY(hipMemsetAsync(G.ctr.p, 0, 64, c->stream));
	const dim3 b_(256), go((unsigned)((n_ol + 255) / 256));
	if (n_pairs && io.res) { hipLaunchKernelGGL(hao_rs_scatter_pe_kernel, dim3((unsigned)((n_pairs + 255) / 256)), b_, 0, c->stream, ol, io.pairs, io.res, n_pairs, wl, RA.win_off, G.wpe.p); HAO_CHECK_LAUNCH(); }
	else if (n_pairs) { hipLaunchKernelGGL(hao_rs_scatter_pe16_kernel, dim3((unsigned)((n_pairs + 255) / 256)), b_, 0, c->stream, ol, io.pairs, io.err8, io.pe16, n_pairs, wl, RA.win_off, G.wpe.p); HAO_CHECK_LAUNCH(); }
	hao_rs_args A; A.ol = ol; A.n_ol = n_ol; A.wl = wl; A.win_off = RA.win_off; A.shift = RA.shift; A.tab = RA.tab; A.werr = c->rf.werr.p; A.wpe = G.wpe.p; A.len = hao_al_reads_of(c).len;
	hipLaunchKernelGGL((hao_rs_gap_kernel<false>), go, b_, 0, c->stream, A, G.ctr.p, (uint64_t*)nullptr, (hao_rs_state*)nullptr, (hao_rs_win*)nullptr); HAO_CHECK_LAUNCH();
	if (int rc = hao_peek(c, G.ctr.p, 2, PK_RS_SIZES)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t na = c->peeked(PK_RS_SIZES), ns = c->peeked(PK_RS_SIZES, 1);
	HIP_TRY(G.st.reserve(na + 1)); HIP_TRY(G.rec.reserve(ns + 1));
	hipLaunchKernelGGL((hao_rs_gap_kernel<true>), go, b_, 0, c->stream, A, G.ctr.p, G.rbase.p, G.st.p, G.rec.p); HAO_CHECK_LAUNCH();
	uint64_t rounds = 0;
	if (na) {
		// column scratch: 24 bytes per text column (t_len <= wl, + slot 0) and lane, in slices of the states whose columns fit the budget (hao_col_slice); a slice runs its rounds to the end
		const hao_ed_reads R = hao_al_reads_of(c);
		const uint64_t ncol = (uint64_t)wl + 1;
		const uint64_t slice = hao_col_slice(c, na, 24 * ncol);
		HIP_TRY(G.path.reserve(3 * ncol * slice + 1));
		for (uint64_t lo = 0; lo < na; lo += slice) {
			const uint64_t m = std::min<uint64_t>(slice, na - lo);
			for (;;) {
				HIP_TRY(hipMemsetAsync(G.ctr.p + 4, 0, 8, c->stream));
				hipLaunchKernelGGL(hao_rs_round_kernel, dim3((unsigned)((m + 255) / 256)), b_, 0, c->stream, R, A, G.st.p + lo, m, G.rec.p, G.path.p, slice, G.ctr.p + 4); HAO_CHECK_LAUNCH();
				if (int rc = hao_peek(c, G.ctr.p + 4, 1, PK_RS_WAITING)) return rc;
				HIP_TRY(hipStreamSynchronize(c->stream));
				++rounds;
				if (c->peeked(PK_RS_WAITING) == 0) break;
				if (rounds > 4 * n_slots + 16) { G.path.release(); hao_set_err(c, "rescue stage: more rounds than alignment steps exist"); return HAO_EUNSUPP; }      // (every round completes a step of every waiting lane)
			}
		}
	}
	hipLaunchKernelGGL(hao_rs_verdict_kernel, go, b_, 0, c->stream, A, G.rbase.p, G.rec.p, io.rs_ovlp->p, G.ctr.p + 5); HAO_CHECK_LAUNCH();
	HIP_TRY(c->al_k1.reserve(n_ol + 2));      // (al_k1: the upload path's key buffer, free here)
	hipLaunchKernelGGL(hao_rs_count_kernel, dim3((unsigned)((n_ol + 256) / 256)), b_, 0, c->stream, n_ol, RA.win_off, G.rbase.p, G.rec.p, c->al_k1.p); HAO_CHECK_LAUNCH();
	if (int rc = hao_excl_scan_u64(c, c->al_k1.p, io.rs_off->p, n_ol + 1)) return rc;
	if (int rc = hao_peek(c, io.rs_off->p + n_ol, 1, PK_RS_NWINS)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t n_wins = c->peeked(PK_RS_NWINS);
	HIP_TRY(io.rs_wins->reserve(n_wins + 1));
	if (n_wins) { hipLaunchKernelGGL(hao_rs_compact_kernel, go, b_, 0, c->stream, n_ol, RA.win_off, G.rbase.p, G.rec.p, io.rs_off->p, io.rs_wins->p); HAO_CHECK_LAUNCH(); }
	if (int rc = hao_peek(c, G.ctr.p + 5, 1, PK_RS_TOTAL)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->rs_total = c->peeked(PK_RS_TOTAL); c->rs_rounds = rounds; c->rs_active = na; c->rs_slots = ns; c->rs_nw = n_wins;
	hao_release_above(G.path, HAO_SCRATCH_KEEP);
	return HAO_OK;
}

// the window lists (hao_wlist.cuh; hao_wlist_run, hao_batch.hpp): over the overlaps of a batch whose rescue stage has just run (io; at least one overlap and one
// covered window) - the CSR, shifts and error bytes in c->rf; pe per slot, the rescue records and their region starts in c->rs; the per-overlap results in
// io.rs_ovlp; io.n_slots bounds the records, so that nothing the plan writes is sized by a count read.  Results into io.wl_woff (records per overlap, scanned),
// io.wl_wins, io.wl_cigoff and io.wl_cig; c->wl_out: records, windows swept, re-placement sweeps, cigar entries, untraced windows.  Host round trips: one for the
// sizes of the sort, the rows and the cigar array, one for the totals at the end (which the streamed path needs to size its arena part).
int hao_al_wlist(hao_ctx *c, const hao_ref_io &io)
{
	const hao_ovlp_t *ol = io.ol; const uint64_t n_ol = io.n_ol, n_slots = io.n_slots; const uint32_t wl = io.wl; uint64_t *out = c->wl_out;
	DevBuf<uint64_t> &o_woff = *io.wl_woff, &o_cigoff = *io.wl_cigoff; DevBuf<hao_rs_win> &o_wins = *io.wl_wins; DevBuf<uint16_t> &o_cig = *io.wl_cig;
	hao_ctx::Wlist &G = c->wl;
	if (n_slots >= (1ULL << 28)) { hao_set_err(c, "window lists: more than 2^28 covered windows in one batch"); return HAO_EUNSUPP; }
	HIP_TRY(G.cnt.reserve(n_ol + 2)); HIP_TRY(o_woff.reserve(n_ol + 2)); HIP_TRY(G.plan.reserve(n_slots + 1)); HIP_TRY(o_wins.reserve(n_slots + 1)); HIP_TRY(G.ncig.reserve(n_slots + 2));
	HIP_TRY(o_cigoff.reserve(n_slots + 2)); HIP_TRY(G.key.reserve(n_slots + 1)); HIP_TRY(G.key2.reserve(n_slots + 1)); HIP_TRY(G.idx.reserve(n_slots + 1)); HIP_TRY(G.sel.reserve(n_slots + 1));
	HIP_TRY(G.rowof.reserve(n_slots + 1)); HIP_TRY(G.ctr.reserve(8));
	HIP_TRY(hipMemsetAsync(G.ctr.p, 0, 64, c->stream));
	hao_wl_args W; W.A.ol = ol; W.A.n_ol = n_ol; W.A.wl = wl; W.A.win_off = c->rf.woff.p; W.A.shift = c->rf.shift.p; W.A.tab = io.tab; W.A.werr = c->rf.werr.p; W.A.wpe = c->rs.wpe.p; W.A.len = hao_al_reads_of(c).len;
	W.rbase = c->rs.rbase.p; W.rec = c->rs.rec.p; W.ov = io.rs_ovlp->p;
	// sort key of a record that needs a sweep: query read << wbits | grid window (a read has fewer than 2^32 / wl windows)
	uint32_t wbits = 32; while (wbits > 1 && (wl >> (32 - wbits + 1))) --wbits;
	hao_read_view V; (void)hao_reads_view(c, &V);
	uint32_t rbits = 1; while (rbits < 32 && (V.n >> rbits)) ++rbits;      // (x_id names a read of the view)
	const dim3 b_(256), go((unsigned)((n_ol + 255) / 256));
	hipLaunchKernelGGL(hao_wl_count_kernel, dim3((unsigned)((n_ol + 256) / 256)), b_, 0, c->stream, W, G.cnt.p); HAO_CHECK_LAUNCH();
	if (int rc = hao_excl_scan_u64(c, G.cnt.p, o_woff.p, n_ol + 1)) return rc;
	hipLaunchKernelGGL(hao_wl_plan_kernel, go, b_, 0, c->stream, W, o_woff.p, G.plan.p, o_wins.p, G.ncig.p, G.key.p, G.idx.p, wbits, G.ctr.p); HAO_CHECK_LAUNCH();
	if (int rc = hao_peek(c, o_woff.p + n_ol, 1, PK_WL_N)) return rc;
	if (int rc = hao_peek(c, G.ctr.p, 3, PK_WL_PLAN)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t N = c->peeked(PK_WL_N), M = c->peeked(PK_WL_PLAN), bound = c->peeked(PK_WL_PLAN, 1);
	if (N > n_slots || M > N) { hao_set_err(c, "window lists: more records than covered windows"); return HAO_EUNSUPP; }
	const uint32_t cap = 2 * 31 + 3 + (2 * wl + 62) / 0x3fff;      // (hao_tg_bound for thre <= 31 and a window of wl bases)
	if (M) {
		// text order: the records that need a sweep to the front, by (query read, grid window); stable, so overlaps of one window keep their order
		if (int rc = hao_sort_pairs(c, G.key.p, G.key2.p, G.idx.p, G.sel.p, N, wbits + rbits)) return rc;
		// column scratch: 24 bytes per text column (t_len <= wl, + slot 0) and lane, in slices whose columns fit the budget (hao_col_slice); two rows of `cap` entries per swept record
		const hao_ed_reads R = hao_al_reads_of(c);
		const uint64_t ncol = (uint64_t)wl + 1;
		const uint64_t slice = hao_col_slice(c, M, 24 * ncol);
		HIP_TRY(G.path.reserve(3 * ncol * slice + 1)); HIP_TRY(G.rows.reserve(M * 2 * (uint64_t)cap + 1));
		for (uint64_t lo = 0; lo < M; lo += slice) {
			const uint64_t m = std::min<uint64_t>(slice, M - lo);
			hipLaunchKernelGGL(hao_wl_trace_kernel, dim3((unsigned)((m + 255) / 256)), b_, 0, c->stream, R, W, G.plan.p, G.sel.p + lo, m, lo, G.path.p, slice, G.rows.p, cap, o_wins.p, G.ncig.p, G.rowof.p, G.ctr.p); HAO_CHECK_LAUNCH();
		}
	}
	HIP_TRY(hipMemsetAsync(G.ncig.p + N, 0, 8, c->stream));
	if (int rc = hao_excl_scan_u64(c, G.ncig.p, o_cigoff.p, N + 1)) return rc;
	HIP_TRY(o_cig.reserve(bound + 1));
	if (N) { hipLaunchKernelGGL(hao_wl_fill_kernel, dim3((unsigned)((N + 255) / 256)), b_, 0, c->stream, W, G.plan.p, o_wins.p, N, o_cigoff.p, G.rowof.p, G.rows.p, cap, o_cig.p, bound); HAO_CHECK_LAUNCH(); }
	if (int rc = hao_peek(c, o_cigoff.p + N, 1, PK_WL_NCIG)) return rc;
	if (int rc = hao_peek(c, G.ctr.p, 6, PK_WL_CTR)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	hao_release_above(G.path, HAO_SCRATCH_KEEP); hao_release_above(G.rows, HAO_SCRATCH_KEEP);
	if (c->peeked(PK_WL_NCIG) > bound) { hao_set_err(c, "window lists: more cigar entries than their bound"); return HAO_EUNSUPP; }      // (hao_tg_bound rules it out)
	if (c->peeked(PK_WL_CTR, 4) || c->peeked(PK_WL_CTR, 5)) {      // (a broken invariant is an error, not an untraced window)
		hao_set_err(c, "window lists: " + std::to_string(c->peeked(PK_WL_CTR, 5)) + " records whose task could not be rebuilt from the rescue records, " + std::to_string(c->peeked(PK_WL_CTR, 4)) + " whose traced sweep lost the distance-only alignment or overran its row");
		return HAO_EUNSUPP;
	}
	out[0] = N; out[1] = M; out[2] = c->peeked(PK_WL_CTR, 3); out[3] = c->peeked(PK_WL_NCIG); out[4] = c->peeked(PK_WL_CTR, 2);
	return HAO_OK;
}

// ---- the host-fed calls: prologue, check, run, copy out ----
// prologue (`who`: the entry point, for its messages; args_ok: its argument check): the view or today's refusal; what the grid calls left in the shared task /
// result scratch is gone (hao_window_trace_grid's results follow the same rule).  The caller returns at once when this fails or the call is empty.
static int hao_al_host_fed(hao_ctx *c, const char *who, bool args_ok, uint64_t n_tasks, hao_read_view *V)
{
	if (!args_ok) return HAO_EINVAL;
	if (int rc = hao_view_refresh(c)) return rc;
	if (!hao_reads_view(c, V)) { hao_set_err(c, std::string(who) + " needs the bases of both reads: single-device mode only"); return HAO_EUNSUPP; }
	c->win.on_host_fed();
	if (n_tasks >= (1ULL << 32)) { hao_set_err(c, std::string(who) + ": more than 2^32 tasks in one call"); return HAO_EUNSUPP; }
	return HAO_OK;
}
// the range checks (the reference indexes its strings unchecked; a device kernel must not): every task inside its reads, thre <= max_thre, both lengths <= max_len,
// and the rules of the call's kind -
//   HAO_AL_RULE_ED, the distance-only calls: abs_diag <= 2 thre, and p_len - t_len + abs_diag inside the band's words - the final scan would read VP / VN bits beyond
//     them (the reference then indexes the neighbouring vectors of its bit_extz_t)
//   HAO_AL_RULE_SEMI, the traced calls in semi-global mode: the band covers the pattern (0 <= p_len - t_len + abs_diag <= 2 thre, t_len > abs_diag, abs_diag <= 2 thre)
// *words (may be null): bit (nword - 1) = some band of at most four words needs nword 64-bit words (the reference's cal_exz_infi picks nword =
// ceil((2 thre + 1) / 64), Correct.cpp:14508-14565); *tn_max (may be null): the longest text, 1 at the least
// (always inlined, and the refusal out of line: a distance-only call of 400 000 tasks lasts 2 ms, and this loop with the limits and rules as run-time values costs 0.3 ms of it)
enum { HAO_AL_RULE_ED = 1, HAO_AL_RULE_SEMI = 2 };
__attribute__((noinline)) static int hao_al_refuse(hao_ctx *c, const char *who, uint64_t i, const char *why) { hao_set_err(c, std::string(who) + ": task " + std::to_string(i) + why); return HAO_EINVAL; }
__attribute__((always_inline)) static inline int hao_al_check_tasks(hao_ctx *c, const char *who, const hao_read_view &V, const hao_ed_task_t *tasks, uint64_t n, uint32_t max_thre, uint32_t max_len, int rules, uint32_t *words, uint64_t *tn_max)
{
	uint32_t w = 0; uint64_t tn = 1;
	for (uint64_t i = 0; i < n; ++i) {
		const hao_ed_task_t &t = tasks[i];
		if (t.p_rid >= V.n || t.t_rid >= V.n || (uint64_t)t.p_pos + t.p_len > V.h_len[t.p_rid] || (uint64_t)t.t_pos + t.t_len > V.h_len[t.t_rid] ||
			t.thre > max_thre || t.p_len > max_len || t.t_len > max_len || ((rules & HAO_AL_RULE_ED) && t.abs_diag > 2 * t.thre)) return hao_al_refuse(c, who, i, " out of range");
		const uint32_t nw = hao_al_nword(t.thre); const int64_t ai = (int64_t)t.p_len - (int64_t)t.t_len + (int64_t)t.abs_diag;
		if ((rules & HAO_AL_RULE_ED) && nw > 1 && ai > 64 * (int64_t)nw) return hao_al_refuse(c, who, i, ": p_len - t_len + abs_diag beyond the band's words");
		if ((rules & HAO_AL_RULE_SEMI) && (ai < 0 || ai > 2 * (int64_t)t.thre || t.t_len <= t.abs_diag || t.abs_diag > 2 * t.thre)) return hao_al_refuse(c, who, i, ": the band does not cover the pattern");
		if (nw <= 4) w |= 1u << (nw - 1);
		tn = std::max<uint64_t>(tn, t.t_len);
	}
	if (words) *words = w;
	if (tn_max) *tn_max = tn;
	return HAO_OK;
}
// the traced calls' result buffers: begin reserves them and zeroes the flags and the cigar rows (tasks without an alignment get no cigar: their rows read as zeros,
// not as an earlier call's entries); end copies results and cigars out and keeps no more than HAO_SCRATCH_KEEP of column scratch or of cigar rows
static int hao_al_traced_begin(hao_ctx *c, uint64_t n, uint32_t cigar_cap)
{
	HIP_TRY(c->al_tres.reserve(n)); HIP_TRY(c->al_want.reserve(n)); HIP_TRY(c->al_cig.reserve(n * (uint64_t)cigar_cap + 1));
	HIP_TRY(hipMemsetAsync(c->al_want.p, 0, n, c->stream));
	if (cigar_cap) HIP_TRY(hipMemsetAsync(c->al_cig.p, 0, n * (uint64_t)cigar_cap * 2, c->stream));
	return HAO_OK;
}
static int hao_al_traced_end(hao_ctx *c, uint64_t n, uint32_t cigar_cap, hao_trace_result_t *out, uint16_t *cigars)
{
	HIP_TRY(hipMemcpyAsync(out, c->al_tres.p, n * sizeof(hao_trace_result_t), hipMemcpyDeviceToHost, c->stream));
	if (cigar_cap) HIP_TRY(hipMemcpyAsync(cigars, c->al_cig.p, n * (uint64_t)cigar_cap * 2, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	hao_release_above(c->al_path, HAO_SCRATCH_KEEP); hao_release_above(c->al_cig, HAO_SCRATCH_KEEP);
	return HAO_OK;
}

extern "C" {

int hao_window_ed_batch(hao_ctx *c, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_ed_result_t *out)
{
	hao_read_view V; uint32_t words = 0;
	if (int rc = hao_al_host_fed(c, "hao_window_ed_batch", c && (tasks || !n_tasks) && (out || !n_tasks), n_tasks, &V); rc || !n_tasks) return rc;
	if (int rc = hao_al_check_tasks(c, "hao_window_ed_batch", V, tasks, n_tasks, HAO_ED_MAX_THRE, UINT32_MAX, HAO_AL_RULE_ED, &words, nullptr)) return rc;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_al_upload_sorted(c, tasks, n_tasks)) return rc;
	HIP_TRY(c->al_res.reserve(n_tasks));
	if (int rc = hao_al_sweep<HAO_AL_ED, false>(c, hao_al_reads_of(c), c->al_task.p, c->al_order.p, n_tasks, words, nullptr, 0, c->al_res.p, nullptr, nullptr, nullptr, 0u)) return rc;
	HIP_TRY(hipMemcpyAsync(out, c->al_res.p, n_tasks * sizeof(hao_ed_result_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HAO_OK;
}

int hao_window_trace_batch(hao_ctx *c, int mode, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_trace_result_t *out, uint16_t *cigars, uint32_t cigar_cap)
{
	hao_read_view V; uint32_t words = 0; uint64_t tn_max = 1;
	if (int rc = hao_al_host_fed(c, "hao_window_trace_batch", c && mode >= HAO_ALIGN_GLOBAL && mode <= HAO_ALIGN_SEMI && (tasks || !n_tasks) && (out || !n_tasks) && (cigars || !n_tasks || !cigar_cap), n_tasks, &V); rc || !n_tasks) return rc;
	// (no rule on abs_diag outside semi-global mode: the three other modes take any diagonal, as in hao_window_trace_long)
	if (int rc = hao_al_check_tasks(c, "hao_window_trace_batch", V, tasks, n_tasks, HAO_ED_MAX_THRE, UINT32_MAX, mode == HAO_ALIGN_SEMI ? HAO_AL_RULE_SEMI : 0, &words, &tn_max)) return rc;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_al_upload_sorted(c, tasks, n_tasks)) return rc;
	if (int rc = hao_al_traced_begin(c, n_tasks, cigar_cap)) return rc;
	const hao_ed_reads R = hao_al_reads_of(c);
	if (int rc = hao_by_mode(mode, [&](auto M) { return hao_al_trace_run<decltype(M)::value>(c, R, c->al_task.p, c->al_order.p, n_tasks, words, tn_max, c->al_tres.p, c->al_want.p, c->al_cig.p, cigar_cap); })) return rc;
	return hao_al_traced_end(c, n_tasks, cigar_cap, out, cigars);
}

}

// ---- the long calls (hao_align_coop.cuh): bands of up to 64 words ----
// Classes of a call's pairs: 0 = bands of at most four words, served by hao_al_kernel; 1 .. 4 = the cooperative kernel's segments of 8, 16, 32 and 64 lanes
// (HAO_DBG_FORCE=al_coop: no class 0).  The order is made on the host - class, then text, stable - so that a wave's segments are full and neighbours share a text.
struct hao_alc_plan { uint64_t lo[6]; uint32_t words; uint64_t tn_max0; };      // class k = order[lo[k] .. lo[k + 1]); words / tn_max0: class 0's band words and longest text
static int hao_alc_upload(hao_ctx *c, const hao_ed_task_t *tasks, uint64_t n, hao_alc_plan &P, std::vector<uint32_t> &ord)
{
	std::vector<uint64_t> key(n); std::vector<uint8_t> cls(n);
	P.words = 0; P.tn_max0 = 1;
	for (uint64_t i = 0; i < n; ++i) {
		const uint32_t nw = hao_al_nword(tasks[i].thre);
		if (nw <= 4 && !c->sw.al_coop) { cls[i] = 0; key[i] = hao_al_sort_key(tasks[i]); P.words |= 1u << (nw - 1); P.tn_max0 = std::max<uint64_t>(P.tn_max0, tasks[i].t_len); }
		else { cls[i] = (uint8_t)(hao_alc_lg(nw) - 2); key[i] = hao_al_sort_key(tasks[i]) & ((1ULL << 62) - 1); }
	}
	ord.resize(n); for (uint64_t i = 0; i < n; ++i) ord[i] = (uint32_t)i;
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return cls[a] != cls[b] ? cls[a] < cls[b] : key[a] < key[b]; });
	for (int k = 0; k <= 5; ++k) P.lo[k] = (uint64_t)(std::lower_bound(ord.begin(), ord.end(), k, [&](uint32_t a, int v) { return (int)cls[a] < v; }) - ord.begin());
	HIP_TRY(c->al_task.reserve(n)); HIP_TRY(c->al_order.reserve(n));
	HIP_TRY(hipMemcpyAsync(c->al_task.p, tasks, n * sizeof(hao_ed_task_t), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->al_order.p, ord.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	return HAO_OK;
}
// one launch of the cooperative kernel: m pairs of class k (order / poff: their entries)
template<int MODE, bool TRACE> static int hao_alc_launch(hao_ctx *c, const hao_ed_reads &R, int k, const uint32_t *order, uint64_t m, uint64_t *path, const uint64_t *poff,
		hao_ed_result_t *out_ed, hao_trace_result_t *out_tr, uint8_t *want, uint16_t *dc, uint32_t cap)
{
	const int lg = k + 2; const uint64_t per_block = 4 * (uint64_t)(64 >> lg);
	hipLaunchKernelGGL((hao_alc_kernel<MODE, TRACE>), dim3((unsigned)((m + per_block - 1) / per_block)), dim3(256), 0, c->stream, R, (const hao_ed_task_t*)c->al_task.p, order, m, lg, path, poff, out_ed, out_tr, want, dc, cap);
	HAO_CHECK_LAUNCH();
	return HAO_OK;
}
// the first sweep of the cooperative kernel over classes 1 - 4 (lo[k] .. lo[k + 1]: class k's stretch of `order`): keeps nothing, marks in want[] the pairs that end
// within their threshold; after(k, m) follows the launch of class k's m pairs
template<int MODE, typename F> static int hao_alc_first(hao_ctx *c, const hao_ed_reads &R, const uint32_t *order, const uint64_t lo[6], hao_trace_result_t *dr, uint8_t *want, F after)
{
	for (int k = 1; k <= 4; ++k) if (lo[k + 1] > lo[k]) {
		const uint64_t m = lo[k + 1] - lo[k];
		if (int rc = hao_alc_launch<MODE, false>(c, R, k, order + lo[k], m, nullptr, nullptr, nullptr, dr, want, nullptr, 0u)) return rc;
		if (int rc = after(k, m)) return rc;
	}
	return HAO_OK;
}
// the traced modes over the plan's classes: class 0 through hao_al_trace_run, the others in two sweeps of the cooperative kernel - the first keeps nothing and marks
// the pairs that end within their threshold, the second keeps three words per band word and column for those, in slices whose columns fit c->sw.al_slice bytes
template<int MODE> static int hao_alc_trace_run(hao_ctx *c, const hao_ed_reads &R, const hao_ed_task_t *tasks, const hao_alc_plan &P, const std::vector<uint32_t> &ord, uint64_t n,
		hao_trace_result_t *dr, uint8_t *want, uint16_t *dc, uint32_t cap)
{
	const uint32_t *order = c->al_order.p;
	if (P.lo[1]) { if (int rc = hao_al_trace_run<MODE>(c, R, c->al_task.p, order, P.lo[1], P.words, P.tn_max0, dr, want, dc, cap)) return rc; }
	if (P.lo[5] == P.lo[1]) return HAO_OK;
	if (int rc = hao_alc_first<MODE>(c, R, order, P.lo, dr, want, [](int, uint64_t) { return (int)HAO_OK; })) return rc;
	// (selection on the host and exact per-pair blocks; the ladder's hao_ld_first / hao_ld_second select on the device and pack class-uniform blocks - merging them is a change of its own)
	std::vector<uint8_t> hw(n);
	HIP_TRY(hipMemcpyAsync(hw.data(), want, n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	// the selected pairs, still by class and text; a slice = consecutive pairs of one class whose columns fit the budget (at least one pair), offsets from the slice's start
	struct Slice { int k; uint64_t lo, m; };
	std::vector<uint32_t> sel; std::vector<uint64_t> off; std::vector<Slice> slices;
	const uint64_t budget = c->sw.al_slice / 8; uint64_t most = 0;
	for (int k = 1; k <= 4; ++k) {
		uint64_t used = 0; Slice sl{k, sel.size(), 0};
		for (uint64_t q = P.lo[k]; q < P.lo[k + 1]; ++q) if (hw[ord[q]]) {
			const uint64_t w = hao_alc_path_words(tasks[ord[q]].thre, tasks[ord[q]].t_len);
			if (sl.m && used + w > budget) { slices.push_back(sl); sl = Slice{k, sel.size(), 0}; used = 0; }
			sel.push_back(ord[q]); off.push_back(used); used += w; ++sl.m; most = std::max(most, used);
		}
		if (sl.m) slices.push_back(sl);
	}
	if (sel.empty()) return HAO_OK;
	HIP_TRY(c->al_sel.reserve(sel.size())); HIP_TRY(c->al_k1.reserve(off.size())); HIP_TRY(c->al_path.reserve(most + 1));
	HIP_TRY(hipMemcpyAsync(c->al_sel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->al_k1.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
	for (const Slice &sl : slices) { if (int rc = hao_alc_launch<MODE, true>(c, R, sl.k, c->al_sel.p + sl.lo, sl.m, c->al_path.p, c->al_k1.p + sl.lo, nullptr, dr, nullptr, dc, cap)) return rc; }
	HIP_TRY(hipStreamSynchronize(c->stream));      // (sel / off leave scope)
	return HAO_OK;
}

extern "C" {

int hao_window_ed_long(hao_ctx *c, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_ed_result_t *out)
{
	hao_read_view V;
	if (int rc = hao_al_host_fed(c, "hao_window_ed_long", c && (tasks || !n_tasks) && (out || !n_tasks), n_tasks, &V); rc || !n_tasks) return rc;
	// (hao_window_ed_batch's rules; only the limits differ)
	if (int rc = hao_al_check_tasks(c, "hao_window_ed_long", V, tasks, n_tasks, HAO_ED_LONG_MAX_THRE, HAO_ED_LONG_MAX_LEN, HAO_AL_RULE_ED, nullptr, nullptr)) return rc;
	HIP_TRY(hipSetDevice(c->device));
	hao_alc_plan P; std::vector<uint32_t> ord;
	if (int rc = hao_alc_upload(c, tasks, n_tasks, P, ord)) return rc;
	HIP_TRY(c->al_res.reserve(n_tasks));
	hao_ed_task_t *dt = c->al_task.p; uint32_t *order = c->al_order.p; hao_ed_result_t *dr = c->al_res.p;
	const hao_ed_reads R = hao_al_reads_of(c);
	if (P.lo[1]) { if (int rc = hao_al_sweep<HAO_AL_ED, false>(c, R, dt, order, P.lo[1], P.words, nullptr, 0, dr, nullptr, nullptr, nullptr, 0u)) return rc; }
	for (int k = 1; k <= 4; ++k) if (P.lo[k + 1] > P.lo[k]) {
		if (int rc = hao_alc_launch<HAO_AL_ED, false>(c, R, k, order + P.lo[k], P.lo[k + 1] - P.lo[k], nullptr, nullptr, dr, nullptr, nullptr, nullptr, 0u)) return rc; }
	HIP_TRY(hipMemcpyAsync(out, dr, n_tasks * sizeof(hao_ed_result_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HAO_OK;
}

int hao_window_trace_long(hao_ctx *c, int mode, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_trace_result_t *out, uint16_t *cigars, uint32_t cigar_cap)
{
	hao_read_view V;
	if (int rc = hao_al_host_fed(c, "hao_window_trace_long", c && mode >= HAO_ALIGN_GLOBAL && mode <= HAO_ALIGN_SEMI && (tasks || !n_tasks) && (out || !n_tasks) && (cigars || !n_tasks || !cigar_cap), n_tasks, &V); rc || !n_tasks) return rc;
	// (hao_window_trace_batch's rules; only the limits differ)
	if (int rc = hao_al_check_tasks(c, "hao_window_trace_long", V, tasks, n_tasks, HAO_ED_LONG_MAX_THRE, HAO_ED_LONG_MAX_LEN, mode == HAO_ALIGN_SEMI ? HAO_AL_RULE_SEMI : 0, nullptr, nullptr)) return rc;
	HIP_TRY(hipSetDevice(c->device));
	hao_alc_plan P; std::vector<uint32_t> ord;
	if (int rc = hao_alc_upload(c, tasks, n_tasks, P, ord)) return rc;
	if (int rc = hao_al_traced_begin(c, n_tasks, cigar_cap)) return rc;
	const hao_ed_reads R = hao_al_reads_of(c);
	if (int rc = hao_by_mode(mode, [&](auto M) { return hao_alc_trace_run<decltype(M)::value>(c, R, tasks, P, ord, n_tasks, c->al_tres.p, c->al_want.p, c->al_cig.p, cigar_cap); })) return rc;
	return hao_al_traced_end(c, n_tasks, cigar_cap, out, cigars);
}

}

// ---- the threshold ladder (hao_ladder.cuh; hao_window_ladder, hao_capi_rest.hpp) ----
// one round's sweeps of one mode over the sorted slots: lo[k] .. lo[k + 1] = class k's stretch of `order` (class 0: hao_al_trace_run, which selects and traces on
// its own; classes 1 - 4: the first sweep of the cooperative kernel and the selection of the pairs that aligned, into sel / selcnt)
template<int MODE> static int hao_ld_first(hao_ctx *c, const hao_ed_reads &R, int mode, const uint64_t lo[6], uint32_t words, uint64_t tn_max0, hao_trace_result_t *dr, uint8_t *want, uint16_t *dc, uint32_t cap)
{
	hao_ctx::Ladder &G = c->ld; const uint32_t *order = c->al_order.p;
	if (lo[1] > lo[0]) { if (int rc = hao_al_trace_run<MODE>(c, R, c->al_task.p, order + lo[0], lo[1] - lo[0], words, tn_max0, dr, want, dc, cap)) return rc; }
	// (selection on the device and class-uniform blocks; hao_alc_trace_run selects on the host and packs exact per-pair blocks - merging them is a change of its own)
	return hao_alc_first<MODE>(c, R, order, lo, dr, want, [&](int k, uint64_t m) { return hao_select(c, order + lo[k], hao_al_flagged{want}, G.sel.p + lo[k], G.selcnt.p + mode * 4 + (k - 1), m); });
}
// the second sweep of class k's n_sel selected pairs (sel: their slots), every pair with a column block of pw words, in slices that fit the column budget
template<int MODE> static int hao_ld_second(hao_ctx *c, const hao_ed_reads &R, int k, const uint32_t *sel, uint64_t n_sel, uint64_t pw, hao_trace_result_t *dr, uint16_t *dc, uint32_t cap)
{
	hao_ctx::Ladder &G = c->ld;
	const uint64_t per = std::max<uint64_t>(1, std::min<uint64_t>(n_sel, (c->sw.al_slice / 8) / pw));
	HIP_TRY(G.poff.reserve(n_sel + 1)); HIP_TRY(c->al_path.reserve(per * pw + 1));
	hipLaunchKernelGGL(hao_ld_poff_kernel, dim3((unsigned)((n_sel + 255) / 256)), dim3(256), 0, c->stream, G.poff.p, n_sel, per, pw); HAO_CHECK_LAUNCH();
	for (uint64_t at = 0; at < n_sel; at += per) {
		if (int rc = hao_alc_launch<MODE, true>(c, R, k, sel + at, std::min<uint64_t>(per, n_sel - at), c->al_path.p, G.poff.p + at, nullptr, dr, nullptr, dc, cap)) return rc; }
	return HAO_OK;
}

// n requests (already in c->ld.req) over the overlaps ol[n_ol] and their fake cigars: results in c->ld.res (ADV: c->ld.res_adv), CSR offsets in c->ld.off (n + 1), entries
// in c->ld.cig; *n_cigar = the entries.  Host round trips: one for the checks, per round one for its counters, one per mode with narrow bands (hao_al_trace_run's selection) and
// one for the cooperative classes' selections, one for the total at the end.  ADV (hao_ladder.cuh: the rule set of hc_aln_exz_adv, with wl and force_l): up to five rounds,
// and the exact shortcut's kernel between the set-up and the first read-back, so that it costs no round trip of its own.
template<bool ADV> static int hao_ld_run(hao_ctx *c, const char *who, typename hao_ld_rule<ADV>::res_t *res, const hao_ovlp_t *ol, uint64_t n_ol, const uint64_t *fc, const uint64_t *fc_off, uint64_t n,
		double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l, uint64_t *n_cigar, uint64_t *rounds_out)
{      // (ADV with c->win.wlist_records_resident(): the batch's window lists serve estimate_err < 0 on a stretch longer than wl, when wl is the window length they were built on)
	constexpr int NA = hao_ld_rule<ADV>::N_ATT;      // attempts per request = the most rounds
	const std::string w_ = who;
	hao_ctx::Ladder &G = c->ld; *n_cigar = 0;
	hao_read_view V; (void)hao_reads_view(c, &V);
	const hao_ed_reads R = hao_al_reads_of(c);
	HIP_TRY(G.att.reserve(NA * n)); HIP_TRY(G.ncig.reserve(n + 1)); HIP_TRY(G.rowref.reserve(n)); HIP_TRY(G.off.reserve(n + 2)); HIP_TRY(G.open[0].reserve(n)); HIP_TRY(G.open[1].reserve(n));
	HIP_TRY(G.sel.reserve(n)); HIP_TRY(G.selcnt.reserve(16)); HIP_TRY(G.coord.reserve(n)); HIP_TRY(G.ctr.reserve(64)); HIP_TRY(G.cig.reserve(1));
	HIP_TRY(c->al_task.reserve(n)); HIP_TRY(c->al_k1.reserve(n)); HIP_TRY(c->al_k2.reserve(n)); HIP_TRY(c->al_i1.reserve(n)); HIP_TRY(c->al_order.reserve(n)); HIP_TRY(c->al_tres.reserve(n)); HIP_TRY(c->al_want.reserve(n));
	HIP_TRY(hipMemsetAsync(G.ctr.p, 0, 64 * 8, c->stream));
	hao_ld_args A; A.req = G.req.p; A.n_req = n; A.ol = ol; A.n_ol = n_ol; A.fc = fc; A.fc_off = fc_off; A.len = V.len; A.n_reads = V.n; A.e_rate = e_rate; A.maxl = maxl; A.maxe = maxe; A.coop_all = c->sw.al_coop ? 1 : 0; A.wl = wl; A.force_l = force_l;
	const bool lists = ADV && c->win.wlist_records_resident() && c->rf_tab_wl && (int64_t)c->rf_tab_wl == wl;
	A.wl_off = lists ? c->wl.woff.p : nullptr; A.wl_wins = lists ? c->wl.wins.p : nullptr; A.wl_len = lists ? (int64_t)c->rf_tab_wl : 0;
	const dim3 b_(256), gn((unsigned)((n + 255) / 256));
	if (ADV) { HIP_TRY(G.xlist.reserve(n)); HIP_TRY(G.xrow.reserve(n)); HIP_TRY(G.pth.reserve(n)); HIP_TRY(G.est.reserve(n)); }
	hipLaunchKernelGGL(hao_ld_thre_kernel<ADV>, gn, b_, 0, c->stream, A, G.att.p, res, G.ncig.p, G.open[0].p, G.xlist.p, G.pth.p, G.est.p, G.ctr.p); HAO_CHECK_LAUNCH();
	if constexpr (ADV) { hipLaunchKernelGGL(hao_ld_exact_kernel, gn, b_, 0, c->stream, A, R, (const uint32_t*)G.xlist.p, n, (const int32_t*)G.att.p, res, G.ncig.p, G.rowref.p, G.xrow.p, G.open[0].p, G.ctr.p); HAO_CHECK_LAUNCH(); }
	if (int rc = hao_peek(c, G.ctr.p, 2, PK_LD_SETUP)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (c->peeked(PK_LD_SETUP)) { hao_set_err(c, w_ + ": " + std::to_string(c->peeked(PK_LD_SETUP)) + " requests out of range (overlap index, mode, estimate_err - negative on a stretch longer than wl without window lists of that window length on the batch, or a negative value from them -, coordinates, or a length beyond HAO_ED_LONG_MAX_LEN)"); return HAO_EINVAL; }
	uint64_t m = c->peeked(PK_LD_SETUP, 1);
	if (m > n) { hao_set_err(c, w_ + ": more open requests than requests"); return HAO_EUNSUPP; }
	hao_ld_rows W; for (int j = 0; j <= HAO_LD_ROUNDS; ++j) { W.rows[j] = nullptr; W.cap[j] = 0; }
	for (int j = 0; j < NA; ++j) rounds_out[j] = 0;
	if (ADV) { W.rows[HAO_LD_ROUNDS] = G.xrow.p; W.cap[HAO_LD_ROUNDS] = 1; }
	for (int j = 0; j < NA && m; ++j) {
		rounds_out[j] = m;
		const uint32_t *open = G.open[j & 1].p; uint32_t *next = G.open[(j + 1) & 1].p;
		const dim3 gm((unsigned)((m + 255) / 256));
		HIP_TRY(hipMemsetAsync(G.ctr.p + HAO_LD_RND, 0, HAO_LD_RND_N * 8, c->stream)); HIP_TRY(hipMemsetAsync(G.selcnt.p, 0, 16 * 8, c->stream)); HIP_TRY(hipMemsetAsync(c->al_want.p, 0, m, c->stream));
		hipLaunchKernelGGL(hao_ld_task_kernel<ADV>, gm, b_, 0, c->stream, A, j, (const int32_t*)G.att.p, open, m, c->al_task.p, G.coord.p, c->al_k1.p, c->al_i1.p, G.pth.p, G.ctr.p); HAO_CHECK_LAUNCH();
		if (int rc = hao_al_sort_by_text(c, m)) return rc;
		if (int rc = hao_peek(c, G.ctr.p + HAO_LD_RND, HAO_LD_RND_N, PK_LD_ROUND)) return rc;
		HIP_TRY(hipStreamSynchronize(c->stream));
		auto rnd = [&](int k) { return (uint64_t)c->peeked(PK_LD_ROUND, k - HAO_LD_RND); };
		// a row of the round holds the longest cigar an alignment within the round's widest threshold can have (hao.h: 2 thre + 3 for strings this short)
		const uint32_t cap = 2 * (uint32_t)rnd(HAO_LD_THRE) + 3;
		uint64_t lo[4][6], at = 0, n_task = 0;
		for (int md = 0; md < 4; ++md) { for (int k = 0; k < 5; ++k) { lo[md][k] = at; at += rnd(HAO_LD_CNT + md * 5 + k); } lo[md][5] = at; }
		n_task = at;
		if (n_task > m) { hao_set_err(c, w_ + ": more tasks than open requests"); return HAO_EUNSUPP; }
		DevBuf<uint16_t> &rows = G.rows[j];
		HIP_TRY(rows.reserve(m * (uint64_t)cap + 1)); W.rows[j] = rows.p; W.cap[j] = cap;
		hao_trace_result_t *dr = c->al_tres.p; uint8_t *want = c->al_want.p;
		for (int md = 0; md < 4; ++md) if (lo[md][5] > lo[md][0]) {
			const uint32_t words = (uint32_t)rnd(HAO_LD_WORDS + md); const uint64_t tn0 = std::max<uint64_t>(1, rnd(HAO_LD_TN + md));
			if (int rc = hao_by_mode(md, [&](auto M) { return hao_ld_first<decltype(M)::value>(c, R, md, lo[md], words, tn0, dr, want, rows.p, cap); })) return rc;
		}
		bool coop = false; for (int md = 0; md < 4; ++md) coop = coop || lo[md][5] > lo[md][1];
		if (coop) {
			if (int rc = hao_peek(c, G.selcnt.p, 16, PK_LD_SEL)) return rc;
			HIP_TRY(hipStreamSynchronize(c->stream));
			for (int md = 0; md < 4; ++md) for (int k = 1; k <= 4; ++k) {
				const uint64_t n_sel = c->peeked(PK_LD_SEL, md * 4 + (k - 1)), pw = rnd(HAO_LD_PW + md * 4 + (k - 1));
				if (!n_sel) continue;
				if (n_sel > lo[md][k + 1] - lo[md][k] || !pw) { hao_set_err(c, w_ + ": more selected pairs than tasks"); return HAO_EUNSUPP; }
				const uint32_t *sel = G.sel.p + lo[md][k];
				if (int rc = hao_by_mode(md, [&](auto M) { return hao_ld_second<decltype(M)::value>(c, R, k, sel, n_sel, pw, dr, rows.p, cap); })) return rc;
			}
		}
		hipLaunchKernelGGL(hao_ld_commit_kernel<ADV>, gm, b_, 0, c->stream, j, (const int32_t*)G.att.p, open, m, (const hao_ed_task_t*)c->al_task.p, (const hao_ld_coord*)G.coord.p, (const hao_trace_result_t*)dr, cap, res, G.ncig.p, G.rowref.p, next, G.ctr.p); HAO_CHECK_LAUNCH();
		// the next round's list becomes the open one; its count crosses with the checks of the next round - here, to size that round's launches
		HIP_TRY(hipMemcpyAsync(G.ctr.p + HAO_LD_OPEN, G.ctr.p + HAO_LD_NEXT, 8, hipMemcpyDeviceToDevice, c->stream)); HIP_TRY(hipMemsetAsync(G.ctr.p + HAO_LD_NEXT, 0, 8, c->stream));
		if (int rc = hao_peek(c, G.ctr.p, 2, PK_LD_SETUP)) return rc;
		HIP_TRY(hipStreamSynchronize(c->stream));
		m = c->peeked(PK_LD_SETUP, 1);
		if (m > n) { hao_set_err(c, w_ + ": more open requests than requests"); return HAO_EUNSUPP; }
	}
	HIP_TRY(hipMemsetAsync(G.ncig.p + n, 0, 8, c->stream));
	if (int rc = hao_excl_scan_u64(c, G.ncig.p, G.off.p, n + 1)) return rc;
	HIP_TRY(hipMemcpyAsync(G.ctr.p + HAO_LD_NEXT, G.off.p + n, 8, hipMemcpyDeviceToDevice, c->stream));
	if (int rc = hao_peek(c, G.ctr.p + HAO_LD_NEXT, 2, PK_LD_END)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t total = c->peeked(PK_LD_END);
	if (c->peeked(PK_LD_END, 1)) { hao_set_err(c, w_ + ": " + std::to_string(c->peeked(PK_LD_END, 1)) + " cigars longer than their row"); return HAO_EUNSUPP; }      // (2 thre + 3 entries bound an alignment within thre)
	HIP_TRY(G.cig.reserve(total + 1));
	if (total) { hipLaunchKernelGGL(hao_ld_fill_kernel, dim3((unsigned)((n * 64 + 255) / 256)), b_, 0, c->stream, W, G.ncig.p, G.rowref.p, G.off.p, n, G.cig.p, total); HAO_CHECK_LAUNCH(); }
	*n_cigar = total;
	return HAO_OK;
}

int hao_al_ladder(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n_ol, const uint64_t *fc, const uint64_t *fc_off, uint64_t n, double e_rate, int64_t maxl, int64_t maxe, uint64_t *n_cigar, uint64_t rounds_out[4])
{
	HIP_TRY(c->ld.res.reserve(n));
	return hao_ld_run<false>(c, "hao_window_ladder", c->ld.res.p, ol, n_ol, fc, fc_off, n, e_rate, 0, maxl, maxe, 0, n_cigar, rounds_out);
}
int hao_al_ladder_adv(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n_ol, const uint64_t *fc, const uint64_t *fc_off, uint64_t n, double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l, uint64_t *n_cigar, uint64_t rounds_out[5])
{
	HIP_TRY(c->ld.res_adv.reserve(n));
	return hao_ld_run<true>(c, "hao_window_ladder_adv", c->ld.res_adv.p, ol, n_ol, fc, fc_off, n, e_rate, wl, maxl, maxe, force_l, n_cigar, rounds_out);
}

// hao_window_estimate_err (hao_capi_rest.hpp): n requests (already in c->ld.e_req) over the overlaps ol[n_ol] and the batch's resident window lists -> c->ld.e_est; *n_bad = the
// requests outside the batch or their query read.  One kernel, a thread per request; nothing of the shared scratch
int hao_al_estimate(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n_ol, uint64_t n, double e_rate, int64_t wl, uint64_t *n_bad)
{
	hao_ctx::Ladder &G = c->ld;
	hao_read_view V; (void)hao_reads_view(c, &V);
	HIP_TRY(G.e_est.reserve(n)); HIP_TRY(G.e_ctr.reserve(1));
	HIP_TRY(hipMemsetAsync(G.e_ctr.p, 0, 8, c->stream));
	hipLaunchKernelGGL(hao_ld_estimate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const hao_ladder_req_t*)G.e_req.p, n, ol, n_ol, V.len, V.n,
		(const uint64_t*)c->wl.woff.p, (const hao_rs_win*)c->wl.wins.p, wl, e_rate, G.e_est.p, G.e_ctr.p); HAO_CHECK_LAUNCH();
	unsigned long long bad = 0;
	HIP_TRY(hipMemcpyAsync(&bad, G.e_ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	*n_bad = bad;
	return HAO_OK;
}

extern "C" int64_t hao_estimate_err_records(const hao_ovlp_t *z, const hao_wlist_win_t *wins, uint64_t n, int64_t wl, int64_t qs, int64_t qe, double e_rate)
{
	static_assert(sizeof(hao_wlist_win_t) == sizeof(hao_rs_win), "hao_wlist_win_t is hao_rs_win");
	return hao_ld_estimate_wlist(*z, (const hao_rs_win*)wins, n, wl, qs, qe, e_rate);
}

extern "C" int hao_ladder_adv_thresholds(int64_t ql, int64_t estimate_err, double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l, int32_t thre[5], int32_t *gate)
{
	if (!thre || !hao_ld_estimate(ql, e_rate, wl, &estimate_err)) return HAO_EINVAL;
	const int n = hao_ld_rungs_adv(ql, estimate_err, e_rate, maxl, maxe, force_l, thre);
	if (gate) *gate = n > 0;      // (an open gate always makes the first attempt)
	return n;
}

extern "C" int hao_ladder_thresholds(int64_t ql, int64_t estimate_err, double e_rate, int64_t maxl, int64_t maxe, int32_t thre[4])
{
	if (!thre) return HAO_EINVAL;
	return hao_ld_rungs(ql, estimate_err, e_rate, maxl, maxe, thre);
}
