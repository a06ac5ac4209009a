// Host orchestration of one query batch: h_ec_lchain for reads [lo, hi) (part of libhao.so).
#pragma once
#include "hao_tables.hpp"
#include "hao_query.cuh"
#include "hao_query3.cuh"
#include "hao_query5.cuh"
#include "hao_grid.cuh"
#include "hao_chain.cuh"

struct hao_ctx::Batch {
	uint64_t n_generic = 0, n_generic_hits = 0, seed_path = 0, seed_left[3] = {0, 0, 0}; DevBuf<unsigned long long> stats, dbgbuf;      // stats: the counter block (hao_stat, hao_query.cuh)
	unsigned long long *stat(hao_stat s, int k = 0) { return &stats.p[(int)s + k]; }      // word k of a named counter
	uint64_t cls_n[HAO_NCLS] = {0, 0, 0, 0, 0, 0, 0}, slow_n[HAO_NCLS] = {0, 0, 0, 0, 0, 0, 0};      // the chain stage's census (hao_batch_chain_path): groups per size class, and those the quick check left to the class's DP kernel
	uint64_t lo = 0, n = 0, mz0 = 0, n_mz = 0, n_anchor = 0, n_groups = 0, n_chains = 0, n_cl = 0, n_fc_raw = 0, n_ol = 0, n_fc = 0, n_fcw = 0;
	bool valid = false, host_valid = false;
	DevBuf<uint64_t> s_start, s_pk, a_off, seg, g_cnt, g_off, g_start, ch_base, cl_base, fc_base, fcs, fc_raw, ol_fc_off, cc_off, cc, fc_final, fcf_off;
	DevBuf<uint64_t> nch64;
	DevBuf<uint64_t> g_tmp, cls_cc, cls_co; DevBuf<hao_gent> glist; DevBuf<uint8_t> g_cls; DevBuf<uint32_t> slow, ovf_list; hipStream_t side[HAO_NCLS]; hipEvent_t ev_qc[HAO_NCLS], ev_dp[HAO_NCLS]; bool side_ready = false; hipEvent_t ev_pk0 = nullptr, ev_pk1 = nullptr; DevBuf<unsigned char> pk_tmp;
	DevBuf<uint32_t> q_pos, q_cnt, s_n, g_read, wgt, nch, nout, perm, n_final, fclen;
	DevBuf<hao_hit_t> hits, ohits, cl;
	DevBuf<int32_t> f, ii, p, key_sc, tm; DevBuf<int64_t> t; DevBuf<uint64_t> key_xs; DevBuf<uint32_t> key_al, key_tmp;
	DevBuf<hao_chain_rec> rec; DevBuf<hao_ovlp_t> ol; DevBuf<hao_cdesc> cd; bool cl_valid = false;
	DevBuf<uint16_t> hq, ohq; DevBuf<uint8_t> hcode;      // delivery path: query minimizer index / wire code of every seed hit (seed kernel, chain_group_kernel)
	DevBuf<uint32_t> pk_cnt, pk_ecnt, pk_erank; uint64_t n_codes = 0;      // one code byte per chained hit (device only) before it is split into bits + code bytes
	// Results of a batch that leave the device.  Two sets, one per delivery slot: while the copy stream drains the set of batch i, batch i + 1
	// computes into the other one (hao_overlap_batch_async).  The blocking API keeps using the current set.
	struct OutSet {
		DevBuf<hao_ovlp_t> ol_out; DevBuf<hao_ovlp_wire_t> ol_wire; DevBuf<uint64_t> fin_off, fc_out, fc_out_off, ch_off, cl_off, qm_off, fcw_off; DevBuf<uint32_t> fcw;      // (fcw*: the fake cigars as they travel, hao_deliver.cuh)
		//      // ol->list in final order, per-read offsets, fake cigars
		DevBuf<hao_chain_hdr_t> hdr; DevBuf<uint64_t> bits; DevBuf<uint32_t> rank, rank4; DevBuf<uint8_t> codes; DevBuf<hao_exc_t> exc; DevBuf<hao_qmz_t> qmz; DevBuf<uint16_t> qmz_pos, qmz_cnt; bool qmz16 = false;   // cl->list in the wire format (hao_deliver.cuh)
		DevBuf<uint8_t> exact;                                                                        // exact-overlap flags of ol_out
		DevBuf<uint64_t> ed_off; DevBuf<uint8_t> ed_err; DevBuf<uint16_t> ed_pe;                      // HAO_DELIVER_ED: pairs per read, error byte and pattern end per pair (hao_ed_deliver.cuh)
		DevBuf<hao_ed_ovlp_sum> ed_sum;                                                               // HAO_DELIVER_ED in reference placement: the per-overlap summaries (ed_ref_summary_kernel)
		DevBuf<uint64_t> wl_woff, wl_cigoff; DevBuf<hao_rs_win> wl_wins; DevBuf<uint16_t> wl_cig;      // HAO_DELIVER_WLIST: record offsets per overlap, the records, entry offsets per record, the entries (hao_wlist.cuh)
		DevBuf<hao_rs_ovlp> rs_ovlp; DevBuf<uint64_t> rs_off; DevBuf<hao_rs_win> rs_wins;                // HAO_DELIVER_RESCUE: per-overlap results, record offsets per overlap, the records (hao_rescue.cuh)
		DevBuf<uint64_t> tr_off; DevBuf<uint16_t> tr_ps, tr_ncig, tr_cig;                            // HAO_DELIVER_TRACE: cigar entries per read, ps and entry count per pair, the entries (hao_trace_grid.cuh)
	};
	// One delivery slot: the output set its batch computes into, the pinned host arena the copy stream drains that set into, and what the caller sees of it
	// (members: hao_deliver_host.hpp)
	struct Slot {
		OutSet out;
		unsigned char *arena = nullptr; size_t arena_cap = 0; bool arena_reg = false, arena_bad = false; int arena_retry = 0;      // arena_reg: mmap + mbind + hipHostRegister (hao_arena_alloc_bound); arena_bad / arena_retry: hao_deliver_wait saw a slow copy - allocated again for the next batch, once
		hipEvent_t ev_ready = nullptr, ev_done = nullptr, ev_cstart = nullptr;      // compute stream: the batch's results are complete; copy stream: the copy has landed / starts
		bool pending = false;      // a copy is queued that nobody has waited for
		uint32_t parts = 0;        // the HAO_DELIVER_* bits the slot's last streamed batch asked for
		hao_delivery_t dl = {}; hao_ed_delivery_t ed = {}; hao_trace_delivery_t tr = {}; hao_rescue_delivery_t rs = {}; hao_wlist_delivery_t wl = {};      // the views (ed.window 0: the batch did not ask for HAO_DELIVER_ED)
		void begin(uint32_t parts_, uint64_t lo, uint64_t n, const hao_ctx *c);
		void arena_free();
	} slot[2];
	int cur = 0;
	OutSet &O() { return slot[cur].out; }
	hipStream_t copy_stream = nullptr; int arena_node = -1; bool dl_ready = false;      // delivery state shared by the slots (hao_deliver_init); arena_node: the NUMA node a probe found best (a box of round 6 reported the GPU on node 0 and copied at 30 GB/s into node 0, 56 into node 1)
	uint32_t wgt_hi = 0xffffffffu, wgt_lo = 0xffffffffu, wgt_max = 0xffffffffu;      // (wgt_max: the largest k_mer_hit::cnt the pass's weight table can give)
	double t_evsync = 0, t_enq = 0, t_alloc = 0, t_s1 = 0, t_s2 = 0, t_s3 = 0, t_run = 0, t_pre = 0; uint64_t t_n = 0, t_nrun = 0;      // host-side time spent in the delivery plumbing (HAO_DBG_PRINT=dl)
	uint64_t ed_unres = 0;      // HAO_DELIVER_ED in reference placement: windows of the batch whose start resolved to no cigar entry
	DevBuf<uint64_t> ed_nwin, ed_wbase, ed_wcnt, ed_woff; DevBuf<hao_ed_pair> ed_pairs; uint64_t ed_n = 0;      // HAO_DELIVER_ED scratch (compute stream only: not per output set); ed_n = pairs of the batch
	uint64_t tr_n = 0, tr_ncig = 0;      // HAO_DELIVER_TRACE: traced pairs and cigar entries of the batch
	uint64_t dl_seq = 0, n_exc = 0; uint32_t dl_parts = 0; bool exact_valid = false; std::vector<uint8_t> h_exact;
	// host copies for fetch
	std::vector<uint64_t> h_seg, h_fin_off, h_cl_off, h_fc_out_off; std::vector<hao_hit_t> h_hits, h_cl; std::vector<hao_ovlp_t> h_ol; std::vector<uint64_t> h_fc;
	std::vector<uint64_t> fetch_fc_off, h_cco;
	// the non-memory part: events and streams, the copy stream synchronised before the arenas go; the buffers free themselves after it
	~Batch() {
		if (ev_pk0) { (void)hipEventDestroy(ev_pk0); (void)hipEventDestroy(ev_pk1); }
		if (side_ready) { for (int x = 0; x < HAO_NCLS; ++x) { (void)hipStreamDestroy(side[x]); (void)hipEventDestroy(ev_qc[x]); (void)hipEventDestroy(ev_dp[x]); } }
		if (dl_ready) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); for (Slot &s : slot) { (void)hipEventDestroy(s.ev_ready); (void)hipEventDestroy(s.ev_done); (void)hipEventDestroy(s.ev_cstart); s.arena_free(); } }
	}
};

// coverage windows per read of the selection's pruning scan (anchor.cpp:1966-2055: ocv_w-sized windows over the query): len / ocv_w + 2
__global__ void hao_cc_count_kernel(const uint32_t *len, uint64_t rid0, uint64_t n, uint64_t ocv_w, uint64_t *out)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r > n) return;
	out[r] = r < n ? len[rid0 + r] / ocv_w + 2 : 0;
}

__global__ void hao_fclen_kernel(const hao_chain_rec *rec, const uint32_t *nch, uint64_t n_groups, uint64_t *out)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;     // chain slot g*3+c
	if (i > n_groups * HAO_MCOPY_MAX) return;
	if (i == n_groups * HAO_MCOPY_MAX) { out[i] = 0; return; }
	uint64_t g = i / HAO_MCOPY_MAX; uint32_t c = (uint32_t)(i % HAO_MCOPY_MAX);
	out[i] = c < nch[g] ? rec[i].fc_len : 0;
}

#include <chrono>
static inline double hao_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#include "hao_deliver_host.hpp"

static int hao_scan_u32(hao_ctx *c, const uint32_t *in, uint64_t *out, uint64_t n_plus1)
{
	auto it = rocprim::make_transform_iterator(in, U32ToU64());
	return hao_excl_scan_u64(c, it, out, n_plus1);
}

// exact-overlap flags of the batch's final ol->list (device resident, current output set)
static int hao_exact_run(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch;
	if (B.exact_valid) return HAO_OK;
	HAO_STAGE_VIEW(c, V, "hao_exact_check needs the bases of the target reads");
	HIP_TRY(B.O().exact.reserve(B.n_ol + 1));
	if (B.n_ol) {
		hao_exact_args a;
		a.ol = B.O().ol_out.p; a.n_ol = B.n_ol; a.rid_base = V.id_base; a.packed = V.packed; a.pk_off = V.pk_off; a.len = V.len;
		a.nsite_off = V.nsite_off; a.nsite = V.nsite; a.flags = B.O().exact.p;
		hipLaunchKernelGGL(hao_exact_check_kernel, dim3((unsigned)((B.n_ol + 3) / 4)), dim3(256), 0, c->stream, a);
		HAO_CHECK_LAUNCH();
	}
	B.exact_valid = true;
	return HAO_OK;
}

// ---- reference placement (hao_grid_pair.cuh: hao_ref_pair; hao_grid.cuh: the kernels) ----
// the front of a reference-placed stage over the current batch's final ol->list: covered windows per overlap and their scan (the CSR of the shifts), one peek
// at their total, the shifts (ed_ref_shift_kernel), the CSR slots' error bytes preset to "none".  tab = the threshold table on the device.
static int hao_ed_ref_front(hao_ctx *c, uint32_t wl, const uint8_t *tab, hao_ref_args *A, uint64_t *n_slots)
{
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::OutSet &O = B.O(); hao_ctx::RefGrid &G = c->rf; const uint64_t m = B.n_ol;
	HIP_TRY(G.cnt.reserve(m + 2)); HIP_TRY(G.woff.reserve(m + 2)); HIP_TRY(G.ctr.reserve(2));
	HIP_TRY(hipMemsetAsync(G.ctr.p, 0, 8, c->stream));
	hipLaunchKernelGGL(ed_ref_nwin_kernel, dim3((unsigned)((m + 256) / 256)), dim3(256), 0, c->stream, O.ol_out.p, m, wl, G.cnt.p); HAO_CHECK_LAUNCH();
	if (int rc = hao_excl_scan_u64(c, G.cnt.p, G.woff.p, m + 1)) return rc;
	if (int rc = hao_peek(c, G.woff.p + m, 1, PK_REF_SLOTS)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t Wc = c->peeked(PK_REF_SLOTS);
	HIP_TRY(G.shift.reserve(Wc + 1)); HIP_TRY(G.werr.reserve(Wc + 1));
	if (Wc) HIP_TRY(hipMemsetAsync(G.werr.p, 0xff, Wc, c->stream));
	hipLaunchKernelGGL(ed_ref_shift_kernel, dim3((unsigned)((m * 16 + 255) / 256)), dim3(256), 0, c->stream, O.ol_out.p, m, O.fc_out.p, O.fc_out_off.p, wl, G.woff.p, G.shift.p, G.ctr.p); HAO_CHECK_LAUNCH();
	A->win_off = G.woff.p; A->shift = G.shift.p; A->tab = tab; *n_slots = Wc;
	return HAO_OK;
}
static bool hao_ed_ref_args_ok(uint32_t wl, double e_rate) { return wl != 0 && (uint64_t)wl + 62 < 65535 && e_rate > 0 && e_rate < 1; }
static int hao_ed_ref_upload(hao_ctx *c, uint32_t wl, double e_rate, DevBuf<uint8_t> &tab)
{
	std::vector<uint8_t> h((size_t)wl + 1); hao_ref_thre_table(wl, e_rate, h.data());
	HIP_TRY(tab.reserve((size_t)wl + 1));
	HIP_TRY(hipMemcpy(tab.p, h.data(), (size_t)wl + 1, hipMemcpyHostToDevice));
	return HAO_OK;
}

// ---- the grid's pair list, built in one place for the four stages below ----
// the one launch site of ed_grid_kernel: the instance of run-time `out` (ED_GRID_*) and `place` (HAO_PLACE_*) over the current batch's final ol->list
static void hao_ed_grid_launch(hao_ctx *c, int out, uint32_t place, uint32_t wl, uint32_t thre, uint32_t nword, const uint64_t *wbase, uint64_t *cnt_or_off, hao_ed_task_t *tasks, hao_ed_pair *pairs, hao_ref_args A)
{
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::OutSet &O = B.O();
	hao_read_view V; (void)hao_reads_view(c, &V);      // (the callers hold a view: they refused otherwise)
	auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)((B.n + 3) / 4)), dim3(256), 0, c->stream, O.ol_out.p, O.fin_off.p, V.len, V.local0 + B.lo, B.n, wl, thre, nword, wbase, cnt_or_off, tasks, pairs, A); };
	switch (out * 2 + (place == HAO_PLACE_REF)) {
	case ED_GRID_COUNT * 2: go(ed_grid_kernel<ED_GRID_COUNT, HAO_PLACE_DIAG>); break;
	case ED_GRID_COUNT * 2 + 1: go(ed_grid_kernel<ED_GRID_COUNT, HAO_PLACE_REF>); break;
	case ED_GRID_TASKS * 2: go(ed_grid_kernel<ED_GRID_TASKS, HAO_PLACE_DIAG>); break;
	case ED_GRID_TASKS * 2 + 1: go(ed_grid_kernel<ED_GRID_TASKS, HAO_PLACE_REF>); break;
	case ED_GRID_PAIRS * 2: go(ed_grid_kernel<ED_GRID_PAIRS, HAO_PLACE_DIAG>); break;
	default: go(ed_grid_kernel<ED_GRID_PAIRS, HAO_PLACE_REF>); break;
	}
}
// what hao_ed_grid_pairs hands back: pairs, grid windows, and in reference placement the covered windows (CSR slots), the unresolved ones and the kernels'
// arguments (CSR, shifts, table); wbase / woff = the scans of windows per read and pairs per window (ed_read_off_kernel's input)
struct hao_grid_list { uint64_t T = 0, W = 0, Wc = 0, UR = 0; hao_ref_args A{nullptr, nullptr, nullptr}; const uint64_t *wbase = nullptr, *woff = nullptr; };
// The pair list of the current batch's final ol->list on the window grid, in text order: windows per read (their total from the host's copy of the lengths: no
// device round trip) and their scan, in reference placement the shifts (hao_ed_ref_front; tab = the threshold table on the device), pairs per window
// (ed_grid_kernel) and their scan, the totals, then the fill pass into `tasks` (with, in reference placement, the (overlap, window) list in `pairs` from the same
// pass) or, without `tasks`, into `pairs`; both are sized here.  Scratch: B.ed_* (compute stream only).  The totals come through mapped host memory
// (hao_peek: PK_GRID_PAIRS, PK_REF_UNRES), not a copy - a device-to-host copy would queue behind the previous batch's delivery on the DMA engine - and cost one
// synchronisation (reference placement: one more, for the covered windows, in hao_ed_ref_front).  who: the caller's name in the error string.  No timer marks.
// Fill mode: `tasks` alone - ED_GRID_TASKS; `pairs` alone - ED_GRID_PAIRS; both - ED_GRID_TASKS, which writes the pair list too in REFERENCE placement only (in
// diagonal placement that kernel instance leaves `pairs` unfilled: pass one of the two there).
static int hao_ed_grid_pairs(hao_ctx *c, const char *who, uint32_t place, uint32_t wl, uint32_t thre, uint32_t nword, const uint8_t *tab, DevBuf<hao_ed_task_t> *tasks, DevBuf<hao_ed_pair> *pairs, hao_grid_list *L)
{
	hao_ctx::Batch &B = *c->batch; const uint64_t n = B.n; const bool ref = place == HAO_PLACE_REF && B.n_ol;      // (no overlap: no shifts, no counter - and no pair)
	*L = hao_grid_list();
	hao_read_view V; if (!hao_reads_view(c, &V)) { hao_set_err(c, std::string(who) + " needs the bases of both reads: single-device mode only"); return HAO_EUNSUPP; }
	for (uint64_t r = 0; r < n; ++r) L->W += (c->h_len[B.lo + r] + wl - 1) / wl;
	const uint64_t W = L->W;
	HIP_TRY(B.ed_nwin.reserve(n + 2)); HIP_TRY(B.ed_wbase.reserve(n + 2)); HIP_TRY(B.ed_wcnt.reserve(W + 2)); HIP_TRY(B.ed_woff.reserve(W + 2));
	hipLaunchKernelGGL(ed_grid_nwin_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, V.len, V.local0 + B.lo, n, wl, B.ed_nwin.p); HAO_CHECK_LAUNCH();
	if (int rc = hao_excl_scan_u64(c, B.ed_nwin.p, B.ed_wbase.p, n + 1)) return rc;
	HIP_TRY(hipMemsetAsync(B.ed_wcnt.p + W, 0, 8, c->stream));
	if (ref) { if (int rc = hao_ed_ref_front(c, wl, tab, &L->A, &L->Wc)) return rc; }
	hao_ed_grid_launch(c, ED_GRID_COUNT, place, wl, thre, nword, B.ed_wbase.p, B.ed_wcnt.p, nullptr, nullptr, L->A); HAO_CHECK_LAUNCH();
	if (int rc = hao_excl_scan_u64(c, B.ed_wcnt.p, B.ed_woff.p, W + 1)) return rc;
	if (int rc = hao_peek(c, B.ed_woff.p + W, 1, PK_GRID_PAIRS)) return rc;
	if (ref) { if (int rc = hao_peek(c, c->rf.ctr.p, 1, PK_REF_UNRES)) return rc; }
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t T = c->peeked(PK_GRID_PAIRS);
	if (T >= (1ULL << 32)) { hao_set_err(c, std::string(who) + ": more than 2^32 pairs in one batch"); return HAO_EUNSUPP; }
	if (tasks) HIP_TRY(tasks->reserve(T + 1));
	if (pairs) HIP_TRY(pairs->reserve(T + 1));
	if (T) { hao_ed_grid_launch(c, tasks ? ED_GRID_TASKS : ED_GRID_PAIRS, place, wl, thre, nword, B.ed_wbase.p, B.ed_woff.p, tasks ? tasks->p : nullptr, pairs ? pairs->p : nullptr, L->A); HAO_CHECK_LAUNCH(); }
	L->T = T; L->UR = ref ? c->peeked(PK_REF_UNRES) : 0; L->wbase = B.ed_wbase.p; L->woff = B.ed_woff.p;
	return HAO_OK;
}

// f3 on the device end to end (hao_grid.cuh): window / candidate pairs of the current batch's final ol->list on the grid, in text order, into c->al_task; then the distance-only
// window alignment over them where they lie (hao_al_ed_resident, hao_f3.hip): results in c->al_res.  No host round trip but the total.
int hao_al_ed_resident(hao_ctx *c, uint64_t n_tasks, uint32_t nword);      // (hao_f3.hip)
static int hao_ed_grid_run(hao_ctx *c, uint32_t wl, uint32_t thre, uint64_t *n_tasks)
{
	hao_ctx::Batch &B = *c->batch; *n_tasks = 0; c->win.on_grid(0);      // (the scratch is this call's from here on, whatever becomes of it)
	{ HAO_STAGE_VIEW(c, V, "hao_window_ed_grid needs the bases of both reads"); (void)V; }
	if (wl == 0 || thre > HAO_ED_MAX_THRE) { hao_set_err(c, "hao_window_ed_grid: window length 0 or threshold beyond the widest band"); return HAO_EINVAL; }
	const uint32_t nword = (2 * thre + 1 + 63) / 64;
	if (B.n == 0 || B.n_ol == 0) return HAO_OK;
	hao_grid_list L;
	if (int rc = hao_ed_grid_pairs(c, "hao_window_ed_grid", HAO_PLACE_DIAG, wl, thre, nword, nullptr, &c->al_task, nullptr, &L)) return rc;
	*n_tasks = L.T; c->win.on_grid(L.T);
	return L.T ? hao_al_ed_resident(c, L.T, nword) : HAO_OK;
}

// hao_window_ed_ref: hao_ed_grid_run in reference placement - tasks into c->al_task, results into c->al_res (hao_fetch_ed_grid serves them), plus the pair list,
// the per-overlap summaries (c->rf_sum) and the count of unresolved windows
static int hao_ed_ref_run(hao_ctx *c, uint32_t wl, double e_rate, uint64_t *n_tasks, uint64_t *unresolved)
{
	hao_ctx::Batch &B = *c->batch; *n_tasks = 0; if (unresolved) *unresolved = 0; c->win.on_ref_begin(WinResident::ED); c->rf_unres = 0; c->rs_wc = 0;
	{ HAO_STAGE_VIEW(c, V, "hao_window_ed_ref needs the bases of both reads"); (void)V; }
	if (!hao_ed_ref_args_ok(wl, e_rate)) { hao_set_err(c, "hao_window_ed_ref: window length 0, window + 62 beyond 16 bits, or e_rate outside (0, 1)"); return HAO_EINVAL; }
	if (B.n == 0 || B.n_ol == 0) { c->win.on_ref_done(WinResident::ED); return HAO_OK; }
	if (B.n_ol >= (1ULL << 32)) { hao_set_err(c, "hao_window_ed_ref: more than 2^32 overlaps in one batch"); return HAO_EUNSUPP; }
	if (c->rf_tab_wl != wl || c->rf_tab_erate != e_rate) { c->rf_tab_wl = 0; if (int rc = hao_ed_ref_upload(c, wl, e_rate, c->rf_tab)) return rc; c->rf_tab_wl = wl; c->rf_tab_erate = e_rate; }
	hao_ctx::Batch::OutSet &O = B.O();
	hao_grid_list L;      // (tasks and pair list in one fill pass; threshold and band width come from the table)
	if (int rc = hao_ed_grid_pairs(c, "hao_window_ed_ref", HAO_PLACE_REF, wl, 0, 1, c->rf_tab.p, &c->al_task, &c->rf.pairs, &L)) return rc;
	HIP_TRY(c->rf_sum.reserve(B.n_ol + 1));
	const uint64_t T = L.T;
	*n_tasks = T; c->rf_unres = L.UR; c->rs_wc = L.Wc; if (unresolved) *unresolved = L.UR;
	if (T) {
		if (int rc = hao_al_ed_resident(c, T, 1)) return rc;
		hipLaunchKernelGGL(ed_ref_scatter_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, c->stream, O.ol_out.p, c->rf.pairs.p, c->al_res.p, T, wl, L.A.win_off, c->rf.werr.p); HAO_CHECK_LAUNCH();
	}
	hipLaunchKernelGGL(ed_ref_summary_kernel, dim3((unsigned)((B.n_ol + 255) / 256)), dim3(256), 0, c->stream, O.ol_out.p, B.n_ol, wl, L.A.win_off, c->rf.werr.p, c->rf_sum.p); HAO_CHECK_LAUNCH();
	c->win.on_ref_done(WinResident::ED, T);
	return HAO_OK;
}

// ---- the rescue stage (hao_rescue.cuh) and the window lists (hao_wlist.cuh): one runner each under the blocking calls and the streamed parts ----
int hao_al_rescue(hao_ctx *c, const hao_ref_io &io);      // (hao_f3.hip)
int hao_al_wlist(hao_ctx *c, const hao_ref_io &io);
int hao_al_ladder(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n_ol, const uint64_t *fc, const uint64_t *fc_off, uint64_t n, double e_rate, int64_t maxl, int64_t maxe, uint64_t *n_cigar, uint64_t rounds_out[4]);      // (the threshold ladder, hao_ladder.cuh)
int hao_al_ladder_adv(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n_ol, const uint64_t *fc, const uint64_t *fc_off, uint64_t n, double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l, uint64_t *n_cigar, uint64_t rounds_out[5]);      // (the same under hc_aln_exz_adv's rules)
int hao_al_estimate(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n_ol, uint64_t n, double e_rate, int64_t wl, uint64_t *n_bad);      // (cal_estimate_err over the resident window lists, hao_ladder.cuh)
// the batch as the blocking chain has it: hao_ed_ref_run's table, pair list and results per pair (c->al_res); results into the context's own buffers
static hao_ref_io hao_ref_io_ctx(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch; hao_ref_io io;
	io.ol = B.O().ol_out.p; io.n_ol = B.n_ol; io.wl = c->rf_tab_wl; io.tab = c->rf_tab.p; io.pairs = c->rf.pairs.p; io.n_pairs = c->win.scratch_pairs(); io.n_slots = c->rs_wc;
	io.res = c->al_res.p; io.err8 = nullptr; io.pe16 = nullptr;
	io.rs_ovlp = &c->rs.ovlp; io.rs_off = &c->rs.off; io.rs_wins = &c->rs.wins; io.wl_woff = &c->wl.woff; io.wl_wins = &c->wl.wins; io.wl_cigoff = &c->wl.cig_off; io.wl_cig = &c->wl.cig;
	return io;
}
// the batch as the streamed parts have it: hao_ed_deliver_run's table, pair list and compact records; results into the current output set (its copy runs under the next batch's compute, which reuses the scratch in c->rs / c->wl)
static hao_ref_io hao_ref_io_out(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::OutSet &O = B.O(); hao_ref_io io;
	io.ol = O.ol_out.p; io.n_ol = B.n_ol; io.wl = c->ded_window; io.tab = c->ded_tab.p; io.pairs = B.ed_pairs.p; io.n_pairs = B.ed_n; io.n_slots = c->rs_wc;
	io.res = nullptr; io.err8 = O.ed_err.p; io.pe16 = O.ed_pe.p;
	io.rs_ovlp = &O.rs_ovlp; io.rs_off = &O.rs_off; io.rs_wins = &O.rs_wins; io.wl_woff = &O.wl_woff; io.wl_wins = &O.wl_wins; io.wl_cigoff = &O.wl_cigoff; io.wl_cig = &O.wl_cig;
	return io;
}
// the rescue stage over io: per-overlap results, the records compacted on the device into a CSR by overlap (a batch without overlaps: one offset, 0), the counts in c->rs_*
static int hao_rescue_run(hao_ctx *c, const hao_ref_io &io)
{
	c->rs_slots = c->rs_rounds = c->rs_active = c->rs_total = c->rs_nw = 0;
	HIP_TRY(io.rs_ovlp->reserve(io.n_ol + 1)); HIP_TRY(io.rs_off->reserve(io.n_ol + 2)); HIP_TRY(io.rs_wins->reserve(1));
	if (io.n_ol == 0) { HIP_TRY(hipMemsetAsync(io.rs_off->p, 0, 8, c->stream)); return HAO_OK; }
	return hao_al_rescue(c, io);
}
// the window lists over io and the rescue stage's results in it (which they do not change); the five counts in c->wl_out.  Two count reads: the stage's sizes, and its totals
static int hao_wlist_run(hao_ctx *c, const hao_ref_io &io)
{
	for (int k = 0; k < 5; ++k) c->wl_out[k] = 0;
	HIP_TRY(io.wl_woff->reserve(io.n_ol + 2)); HIP_TRY(io.wl_wins->reserve(1)); HIP_TRY(io.wl_cigoff->reserve(2)); HIP_TRY(io.wl_cig->reserve(1));
	if (io.n_ol == 0 || io.n_slots == 0) { HIP_TRY(hipMemsetAsync(io.wl_woff->p, 0, (io.n_ol + 1) * 8, c->stream)); HIP_TRY(hipMemsetAsync(io.wl_cigoff->p, 0, 8, c->stream)); return HAO_OK; }
	return hao_al_wlist(c, io);
}

// hao_window_rescue_ref: over what hao_ed_ref_run left - the CSR, shifts and error bytes in c->rf, the pair list, and the results per pair in the shared scratch
static int hao_rescue_ref_run(hao_ctx *c, uint64_t *n_rescued)
{
	*n_rescued = 0; c->win.on_ref_begin(WinResident::RESCUE);
	if (!c->win.ref_input_resident()) { hao_set_err(c, "hao_window_rescue_ref: hao_window_ed_ref has not run on this batch (or another window-alignment call has run since)"); return HAO_EINVAL; }
	{ HAO_STAGE_VIEW(c, V, "hao_window_rescue_ref needs the bases of both reads"); (void)V; }      // (the gathered store has gone since hao_window_ed_ref)
	if (int rc = hao_rescue_run(c, hao_ref_io_ctx(c))) return rc;
	*n_rescued = c->rs_total; c->win.on_ref_done(WinResident::RESCUE);
	return HAO_OK;
}

// hao_window_wlist_ref: over what hao_ed_ref_run and hao_rescue_ref_run left
static int hao_wlist_ref_run(hao_ctx *c, uint64_t out[5])
{
	for (int k = 0; k < 5; ++k) out[k] = 0; c->win.on_ref_begin(WinResident::WLIST);
	{ HAO_STAGE_VIEW(c, V, "hao_window_wlist_ref needs the bases of both reads"); (void)V; }
	if (!c->win.wlist_input_resident()) { hao_set_err(c, "hao_window_wlist_ref: hao_window_ed_ref and hao_window_rescue_ref have not both run on this batch (or another window-alignment call has run since)"); return HAO_EINVAL; }
	if (int rc = hao_wlist_run(c, hao_ref_io_ctx(c))) return rc;
	for (int k = 0; k < 5; ++k) out[k] = c->wl_out[k];
	c->win.on_ref_done(WinResident::WLIST);
	return HAO_OK;
}

// HAO_DELIVER_ED (hao_overlap_batch_async): the grid pairs of the current batch's final ol->list (hao_deliver_ed_config's window and threshold) aligned on the
// compute stream into the output set's compact records (hao_ed_deliver.cuh), so that they travel with the batch.  Scratch and results are the batch's own: the
// blocking path's task / result buffers (c->al_*) are not touched.  Windows per read (from the host's copy of the lengths: no device round trip), pairs per
// window (ed_grid_kernel), a scan, the per-read offsets, one peek at the total, the pair list (8 bytes a pair), one alignment launch.
int hao_al_ed_deliver(hao_ctx *c, const hao_ovlp_t *ol, const hao_ed_pair *pairs, uint64_t n, uint32_t wl, uint32_t thre, uint8_t *err, uint16_t *pe,
		int place = HAO_PLACE_DIAG, hao_ref_args A = hao_ref_args{nullptr, nullptr, nullptr}, uint8_t *werr = nullptr);      // (hao_f3.hip)
static int hao_ed_deliver_run(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::OutSet &O = B.O(); const uint64_t n = B.n;
	const uint32_t wl = c->ded_window, thre = c->ded_thre, nword = (2 * thre + 1 + 63) / 64;
	B.ed_n = 0; B.ed_unres = 0;
	// reference placement (hao_deliver_ed_config_ref): the same pair list with hao_ref_pair, the alignment kernel's reference instance, and the per-overlap
	// summaries into the output set.  A batch in diagonal placement runs none of it.
	const bool ref = c->ded_place == HAO_PLACE_REF;
	c->timer.mark("q_totals");      // (labels what ran since q_final - the totals' read-back and, with HAO_DELIVER_EXACT, the exact check - so that ed_grid / ed_align time the ED stage alone)
	if (B.n_ol >= (1ULL << 32)) { hao_set_err(c, "HAO_DELIVER_ED: more than 2^32 overlaps in one batch"); return HAO_EUNSUPP; }
	HIP_TRY(O.ed_off.reserve(n + 2)); if (ref) HIP_TRY(O.ed_sum.reserve(B.n_ol + 1));
	hao_grid_list L;
	if (int rc = hao_ed_grid_pairs(c, "HAO_DELIVER_ED", c->ded_place, wl, thre, nword, c->ded_tab.p, nullptr, &B.ed_pairs, &L)) return rc;
	const uint64_t T = L.T; B.ed_unres = L.UR; c->rs_wc = L.Wc;
	HIP_TRY(O.ed_err.reserve(T + 64)); HIP_TRY(O.ed_pe.reserve(T + 64));
	hipLaunchKernelGGL(ed_read_off_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, L.wbase, L.woff, n, O.ed_off.p); HAO_CHECK_LAUNCH();
	c->timer.mark("ed_grid");
	if (T) { if (int rc = hao_al_ed_deliver(c, O.ol_out.p, B.ed_pairs.p, T, wl, thre, O.ed_err.p, O.ed_pe.p, c->ded_place, L.A, ref ? c->rf.werr.p : nullptr)) return rc; }
	if (ref && B.n_ol) { hipLaunchKernelGGL(ed_ref_summary_kernel, dim3((unsigned)((B.n_ol + 255) / 256)), dim3(256), 0, c->stream, O.ol_out.p, B.n_ol, wl, L.A.win_off, c->rf.werr.p, O.ed_sum.p); HAO_CHECK_LAUNCH(); }
	c->timer.mark("ed_align");
	B.ed_n = T;
	return HAO_OK;
}

// f3 with traceback on the grid (hao_trace_grid.cuh, hao_f3.hip)
int hao_al_trace_grid(hao_ctx *c, const hao_ovlp_t *ol, const hao_ed_pair *pairs, uint64_t n, uint32_t wl, uint32_t thre, const uint8_t *err,
		uint16_t *ps16, uint16_t *ncig16, DevBuf<uint16_t> &cig, uint64_t *n_traced, uint64_t *n_cigar, uint64_t *n_untraced);
int hao_al_trace_grid_off(hao_ctx *c, const uint64_t *at, uint64_t n, uint64_t n_traced, uint64_t *out);
int hao_al_trace_grid_expand(hao_ctx *c, const hao_ovlp_t *ol, uint64_t n, hao_ed_task_t *tasks, hao_trace_result_t *res);

// HAO_DELIVER_TRACE: the traced grid stage over the pairs and error bytes HAO_DELIVER_ED has just written (same grid, nothing swept twice), into the output
// set's records: ps and entry count per pair, the compact cigars, and the entries' offsets per read (pairs of read r start at ed_off[r])
static int hao_trace_deliver_run(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::OutSet &O = B.O(); const uint64_t n = B.n, T = B.ed_n;
	B.tr_n = 0; B.tr_ncig = 0;
	HIP_TRY(O.tr_ps.reserve(T + 64)); HIP_TRY(O.tr_ncig.reserve(T + 64)); HIP_TRY(O.tr_off.reserve(n + 2));
	uint64_t nt = 0, nc = 0, nu = 0;
	if (int rc = hao_al_trace_grid(c, O.ol_out.p, B.ed_pairs.p, T, c->ded_window, c->ded_thre, O.ed_err.p, O.tr_ps.p, O.tr_ncig.p, O.tr_cig, &nt, &nc, &nu)) return rc;
	if (int rc = hao_al_trace_grid_off(c, O.ed_off.p, n, nt, O.tr_off.p)) return rc;
	B.tr_n = nt; B.tr_ncig = nc;
	return HAO_OK;
}

// hao_window_trace_grid: the grid pairs of the current batch (hao_window_ed_grid's), their distance-only alignment (the delivery path's kernel, into the
// context's own buffers) and the traced stage; everything stays resident for hao_fetch_trace_grid.  out: pairs, traced pairs, cigar entries, aligned but untraced pairs.
static int hao_trace_grid_run(hao_ctx *c, uint32_t wl, uint32_t thre, uint64_t out[4])
{
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::OutSet &O = B.O(); const uint64_t n = B.n;
	c->win.on_trace_grid(false); out[0] = out[1] = out[2] = out[3] = 0;
	{ HAO_STAGE_VIEW(c, V, "hao_window_trace_grid needs the bases of both reads"); (void)V; }
	if (wl == 0 || thre > HAO_ED_MAX_THRE || (uint64_t)wl + 2 * (uint64_t)thre >= 0xffff) { hao_set_err(c, "hao_window_trace_grid: window length 0, threshold beyond the widest band, or window + 2 thre beyond 16 bits"); return HAO_EINVAL; }
	const uint32_t nword = (2 * thre + 1 + 63) / 64;
	c->tg_wl = wl; c->tg_thre = thre; c->tg_n = c->tg_nsel = c->tg_ncig = c->tg_nuntr = 0;
	if (n == 0 || B.n_ol == 0) { c->win.on_trace_grid(true); return HAO_OK; }
	if (B.n_ol >= (1ULL << 32)) { hao_set_err(c, "hao_window_trace_grid: more than 2^32 overlaps in one batch"); return HAO_EUNSUPP; }
	hao_grid_list L;      // (the pair list as the delivery path forms it, into the context's own list)
	if (int rc = hao_ed_grid_pairs(c, "hao_window_trace_grid", HAO_PLACE_DIAG, wl, thre, nword, nullptr, nullptr, &c->tg_pairs, &L)) return rc;
	const uint64_t T = L.T;
	HIP_TRY(c->tg_err.reserve(T + 64)); HIP_TRY(c->tg_pe.reserve(T + 64)); HIP_TRY(c->tg_ps.reserve(T + 64)); HIP_TRY(c->tg_ncig16.reserve(T + 64));
	c->timer.mark("ed_grid");
	if (T) { if (int rc = hao_al_ed_deliver(c, O.ol_out.p, c->tg_pairs.p, T, wl, thre, c->tg_err.p, c->tg_pe.p)) return rc; }
	c->timer.mark("ed_align");
	uint64_t nt = 0, nc = 0, nu = 0;
	if (int rc = hao_al_trace_grid(c, O.ol_out.p, c->tg_pairs.p, T, wl, thre, c->tg_err.p, c->tg_ps.p, c->tg_ncig16.p, c->tg_cig, &nt, &nc, &nu)) return rc;
	c->tg_n = T; c->tg_nsel = nt; c->tg_ncig = nc; c->tg_nuntr = nu; c->win.on_trace_grid(true);
	out[0] = T; out[1] = nt; out[2] = nc; out[3] = nu;
	return HAO_OK;
}

// The one body of the blocking window stages over the resident batch (include/hao.h: hao_window_ed_ref, hao_window_rescue_ref, hao_window_wlist_ref, hao_window_trace_grid): view, device, timer, the stage, its end awaited, the stage times collected
template <class Run> static int hao_window_stage(hao_ctx *c, const char *mark, Run run)
{
	if (!c->batch || !c->batch->valid) return HAO_EINVAL;
	if (int rc = hao_view_refresh(c)) return rc;
	HIP_TRY(hipSetDevice(c->device));
	c->timer.begin(c->stream);
	if (int rc = run()) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (mark) c->timer.mark(mark);
	c->timer.collect(c->stage_ms);
	return HAO_OK;
}

// ---- the batch pass: h_ec_lchain for reads [lo, hi), one function per stage (hao_overlap_run calls them in order) ----
// What a run hands from stage to stage.  The buffers, the side streams and the batch's totals are members of Batch.
struct hao_run {
	hao_ctx *c; hao_ctx::Batch &B; const hao_pass_t &ps; uint32_t parts; double t0;      // parts: the HAO_DELIVER_* bits (0: blocking API); t0: the run's start on the host's clock (HAO_DBG_PRINT=dl)
	uint64_t lo = 0, hi = 0, n = 0, glo = 0, nm = 0;      // query reads [lo, hi); glo: global read id of the first (== lo when unsharded; minimizer arrays are indexed locally); nm: their minimizers
	uint64_t A = 0, G = 0;                                // seed hits, target groups
	// no host round trip between the chain stage and the totals: the buffers downstream are sized by bounds known from G and A (<= 3 chains per group, chained hits <= seed
	// hits, fake-cigar entries <= hits + 6 per group); the exact totals are read back once, after the last kernel
	uint64_t NCmax = 0, FCmax = 0, NW = 0;                // NW: 64-position words of the wire format's bit stream (positions = seed hits)
	hao_cls_layout L; unsigned long long cls_cnt[HAO_NCLS];      // the work lists: first entry of each size class, groups per class
	hao_chain_par par; hao_pack_args pa; bool pack_on_side = false;      // pa: the wire pack's arguments (the exception re-pack runs it again); pack_on_side: it runs on a side stream under the selection
};

// a new batch: the previous one's flags dropped and, with parts, the delivery slot it computes into claimed
static int hao_q_begin(hao_run &R, uint64_t lo, uint64_t hi, int *slot_out)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint32_t parts = R.parts;
	c->win.on_new_batch();      // (the window-alignment results of the previous batch's overlaps are stale)
	B.valid = false; B.host_valid = false; B.cl_valid = false; B.exact_valid = false; B.h_exact.clear(); B.lo = lo; B.n = hi - lo; B.dl_parts = parts; B.n_exc = 0;
	R.lo = lo; R.hi = hi; R.n = B.n; R.glo = c->rid_base + lo;
	if (parts) {
		if (int rc = hao_deliver_init(c, B)) return rc;
		B.cur = (int)(B.dl_seq++ & 1);
		if (slot_out) *slot_out = B.cur;
	}
	// the output set about to be written may still be feeding a copy (its previous async batch): wait for that copy, never for the other slot's
	hao_ctx::Batch::Slot &S = B.slot[B.cur];
	if (B.dl_ready && S.pending) { const double t0_ = hao_now(); HIP_TRY(hipEventSynchronize(S.ev_done)); S.pending = false; B.t_evsync += hao_now() - t0_; }
	if (parts) S.begin(parts, lo, R.n, c);
	return HAO_OK;
}

// Q1 seed lookup: every minimizer's lookup result was computed when the index was built (hao_index_finish_kernel; in sharded mode by the owner of its hash,
// hao_tables.hpp); unpacked here, scanned into the hits' offsets, their total read back (the batch's first synchronise)
static int hao_q_lookup(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const hao_pass_t &ps = R.ps; const uint64_t lo = R.lo, n = R.n;
	// minimizer range of the batch (host knows the per-read offsets? keep a host copy once)
	if (c->h_ix_mz_off.size() != c->n_reads + 1) {
		c->h_ix_mz_off.resize(c->n_reads + 1);
		HIP_TRY(hipMemcpy(c->h_ix_mz_off.data(), c->d_ix_mz_off.p, (c->n_reads + 1) * 8, hipMemcpyDeviceToHost));
	}
	B.mz0 = c->h_ix_mz_off[lo]; B.n_mz = c->h_ix_mz_off[R.hi] - B.mz0;
	const uint64_t nm = R.nm = B.n_mz;
	// (no host-to-device copies inside a batch: with the delivery path's bulk copy of the previous batch in flight they would queue behind it on the DMA engines)
	if (B.wgt_hi != ps.high_occ || B.wgt_lo != ps.low_occ || !B.wgt.p) {      // seed weights depend on the pass's occurrence thresholds only: uploaded when those change
		std::vector<uint32_t> wt; hao_seed_weight_table(ps.high_occ, ps.low_occ, wt);
		HIP_TRY(B.wgt.reserve(4096)); HIP_TRY(hipMemcpy(B.wgt.p, wt.data(), 4096 * 4, hipMemcpyHostToDevice));
		B.wgt_hi = ps.high_occ; B.wgt_lo = ps.low_occ; B.wgt_max = *std::max_element(wt.begin(), wt.end());
	}
	HIP_TRY(B.q_pos.reserve(nm + 1)); HIP_TRY(B.q_cnt.reserve(nm + 1));
	HIP_TRY(B.s_start.reserve(nm + 1)); HIP_TRY(B.s_pk.reserve(nm + 1)); HIP_TRY(B.s_n.reserve(nm + 1)); HIP_TRY(B.a_off.reserve(nm + 2)); HIP_TRY(B.seg.reserve(n + 2));
	HIP_TRY(c->d_err.reserve(2)); HIP_TRY(hipMemsetAsync(c->d_err.p, 0, 8, c->stream));
	if (!c->lk_valid) { hao_set_err(c, "index without per-minimizer lookup results"); return HAO_EINVAL; }
	hipLaunchKernelGGL(seed_unpack_kernel, dim3((unsigned)((nm + 256) / 256)), dim3(256), 0, c->stream, c->d_ix_lk.p, c->d_ix_mz_info.p, B.mz0, nm, B.wgt.p, B.s_start.p, B.s_n.p, B.q_pos.p, B.q_cnt.p, B.s_pk.p);
	HAO_CHECK_LAUNCH();
	if (int rc = hao_scan_u32(c, B.s_n.p, B.a_off.p, nm + 1)) return rc;
	hipLaunchKernelGGL(seed_segments_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, c->d_ix_mz_off.p, lo, n, B.mz0, B.a_off.p, B.seg.p);
	HAO_CHECK_LAUNCH();
	if (int rc = hao_peek(c, B.a_off.p + nm, 1, PK_ANCHORS)) return rc;
	const double ts0_ = hao_now();
	HIP_TRY(hipStreamSynchronize(c->stream));
	B.t_s1 += hao_now() - ts0_; B.t_pre += ts0_ - R.t0;
	R.A = B.n_anchor = c->peeked(PK_ANCHORS);
	c->timer.mark("q_lookup");
	if (R.A >= (1ULL << 32)) { hao_set_err(c, "batch produces >= 2^32 anchors: use a smaller read range"); return HAO_EUNSUPP; }
	return HAO_OK;
}

// the seed stage's table tiers: kernels of one signature (seed_bin_kernel, seed_bin3_kernel) and the dynamic LDS each asks for
typedef void (*hao_seed_tier_fn)(hao_seed_args, const uint32_t*, const unsigned long long*, uint32_t*, unsigned long long*);
typedef void (*hao_seed_lds_fn)(hao_seed_args, const uint64_t*, const uint32_t*, const uint64_t*, uint32_t, uint32_t, uint32_t*, unsigned long long*, unsigned long long*);
struct hao_seed_tiers { hao_seed_tier_fn k[3]; size_t lds[3]; };
// The ladder: the 512-slot tier over the reads of list in0 / cursor in0_cnt (null: over every read of the batch), the 1024-slot tier over the reads the first
// leaves, the 2048-slot tier over the reads the second leaves (it gives none up)
static int hao_seed_ladder(hao_ctx *c, const hao_seed_args &sa, const hao_seed_tiers &T, const uint32_t *in0, const unsigned long long *in0_cnt)
{
	hao_ctx::Batch &B = *c->batch; const unsigned n = (unsigned)sa.n_sel;
	uint32_t *const ovf1 = B.ovf_list.p, *const ovf2 = B.ovf_list.p + (sa.n_sel + 1); unsigned long long *const cnt1 = B.stat(HAO_ST_OVF1), *const cnt2 = B.stat(HAO_ST_OVF2);
	for (int t = 0; t < 3; ++t) HIP_TRY(hipFuncSetAttribute((const void*)T.k[t], hipFuncAttributeMaxDynamicSharedMemorySize, (int)T.lds[t]));      // beyond the default dynamic LDS limit: opt in (the CU has 160 KB)
	hipLaunchKernelGGL(T.k[0], dim3(n), dim3(256), T.lds[0], c->stream, sa, in0, in0_cnt, ovf1, cnt1); HAO_CHECK_LAUNCH();
	hipLaunchKernelGGL(T.k[1], dim3(n), dim3(256), T.lds[1], c->stream, sa, (const uint32_t*)ovf1, (const unsigned long long*)cnt1, ovf2, cnt2); HAO_CHECK_LAUNCH();
	hipLaunchKernelGGL(T.k[2], dim3(n), dim3(256), T.lds[2], c->stream, sa, (const uint32_t*)ovf2, (const unsigned long long*)cnt2, (uint32_t*)nullptr, (unsigned long long*)nullptr); HAO_CHECK_LAUNCH();
	return HAO_OK;
}

// Q2-Q5 in one kernel: index records -> bins -> sorted k_mer_hits + group lists (no anchor keys in memory).  Which kernels carry a batch: B.seed_path
static int hao_seed_launch(hao_run &R, const hao_seed_args &sa_, uint64_t max_q, uint64_t sum_q)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint64_t n = R.n, A = R.A;
	const size_t lds_tile = std::max<size_t>((size_t)512 * (sizeof(hao_stage_t) + 4), 12 * 512);      // staged tile (>= the 12 bytes per slot of the bin sort it shares memory with)
	const size_t lds_q = 12 * (size_t)sa_.qcap + 16;
	const size_t lds1 = (size_t)22 * 512 + lds_tile + lds_q, lds2_ql = hao_seed3_lds<10>::FIXED + lds_q, lds3_ql = hao_seed3_lds<11>::FIXED + lds_q;      // (the tiers without staged tiles: hao_query3.cuh)
	B.seed_path = 0;
	if (max_q <= HAO_QTAB_CAP && !c->sw.seed_noql && c->sw.seed_lds && (double)A * 100.0 <= (double)c->sw.seed_lds_ratio * (double)sum_q * (double)std::max(1, c->hom_cov) && c->n_total < HAO_L5_MASK && c->ix_n_pos + c->sw.ix_pad < (1ULL << 40)) {
		B.seed_path = 2;
		// the list-major kernel (hao_query5.cuh): one persistent workgroup per CU, a read's position lists read once with adjacent lanes on adjacent records into LDS,
		// merged by target there.  The reads it leaves (more than 1536 minimizers, more records than the LDS holds, more than seed_merge_maxn hits) go through the
		// table kernels below it (512-slot launch over the overflow list, then the launches without staged tiles).  Batches of reads across repeat families - hundreds of
		// targets per read, a merge step each - keep the table kernels (341 against 226 ms per pass of the repeat-rich 250 Mb set, profiles/r06/seed_ab.txt).  What tells
		// them apart whatever the coverage: seed hits per (query minimizer x coverage peak) - 1.0 on repeat-free reads at 30 x and at 40 x (every minimizer meets the reads
		// that cover it), 0.5 on ONT reads (1 % error), 1.4 on the repeat-rich set; the list-major kernel takes batches up to seed_lds_ratio = 1.2.
		const hao_seed_tiers T = {{seed_bin_kernel<9, 1, 512, true>, seed_bin3_kernel<10, 1, 4>, seed_bin3_kernel<11, 2, 4>}, {lds1, lds2_ql, lds3_ql}};
		const bool b16 = c->max_len_all < 65536, wide = max_q > 2 * HAO_L5_THREADS, dbg = c->sw.seedphase && b16 && !wide;      // offsets of the staged records in 16 bits; reads with more than 1024 minimizers: three per thread; the phase timers exist in one instance
		hao_seed_lds_fn k0;
		if (dbg) k0 = seed_lds_kernel<true, 2, 14, true>;
		else if (b16) k0 = wide ? seed_lds_kernel<true, 3, 8, false> : seed_lds_kernel<true, 2, 16, false>;
		else k0 = wide ? seed_lds_kernel<false, 3, 8, false> : seed_lds_kernel<false, 2, 16, false>;
		const size_t lds0 = b16 ? hao_l5_lds<true, 2>::TOTAL : hao_l5_lds<false, 2>::TOTAL;
		uint32_t *const ovf0 = B.ovf_list.p + 2 * (n + 1);
		HIP_TRY(hipFuncSetAttribute((const void*)k0, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds0));
		hipLaunchKernelGGL(k0, dim3((unsigned)std::min<uint64_t>(n, (uint64_t)c->n_cu)), dim3(HAO_L5_THREADS), lds0, c->stream, sa_, (const uint64_t*)c->d_ix_sinfo.p, (const uint32_t*)c->d_len_all.p, (const uint64_t*)B.s_pk.p,
			(uint32_t)c->sw.seed_merge_maxn, 176u /* wave 0's share in 1/1024: profiles/r06/seed_ab.txt */, ovf0, B.stat(HAO_ST_OVF0), B.stat(HAO_ST_L5_CURSOR));
		HAO_CHECK_LAUNCH();
		return hao_seed_ladder(c, sa_, T, ovf0, B.stat(HAO_ST_OVF0));
	}
	if (max_q <= HAO_QTAB_CAP && !c->sw.seed_noql) {      // every read's minimizer table fits the LDS; reads whose bins overflow the 512-slot table: the launches without staged tiles (hao_query3.cuh)
		const hao_seed_tiers T = {{seed_bin_kernel<9, 0, 512, true>, seed_bin3_kernel<10, 1, 4>, seed_bin3_kernel<11, 2, 4>}, {lds1, lds2_ql, lds3_ql}};
		return hao_seed_ladder(c, sa_, T, nullptr, nullptr);
	}
	const hao_seed_tiers T = {{seed_bin_kernel<9, 0, 512, false>, seed_bin_kernel<10, 1, 512, false>, seed_bin_kernel<11, 2, 512, false>},
		{lds1, (size_t)22 * 1024 + std::max<size_t>(lds_tile, 12 * 1024) + lds_q, (size_t)22 * 2048 + std::max<size_t>(lds_tile, 12 * 2048) + lds_q}};      // (third tier: 2048 slots = up to 1760 bins per id-range round)
	return hao_seed_ladder(c, sa_, T, nullptr, nullptr);
}

// HAO_DBG_PRINT=seed: the phase timers the seed kernels left in B.dbgbuf
static int hao_seed_dbg_print(hao_ctx *c)
{
	unsigned long long d_[64]; HIP_TRY(hipMemcpy(d_, c->batch->dbgbuf.p, 512, hipMemcpyDeviceToHost));
	if (d_[9]) { fprintf(stderr, "[seed lds] merge us per read, waves 0 - 7:"); for (int w_ = 0; w_ < 8; ++w_) fprintf(stderr, " %.2f", d_[16 + w_] / 100.0 / d_[9]); fprintf(stderr, "\n"); }
	if (d_[9]) fprintf(stderr, "[seed lds] reads %llu  avg us per read (wave 0): stage %.2f  barrier %.2f  prepare %.2f  barrier %.2f  issue loads %.2f  splitters %.2f  merge %.2f  barrier + groups %.2f  barrier %.2f\n", d_[9],
		d_[0] / 100.0 / d_[9], d_[1] / 100.0 / d_[9], d_[2] / 100.0 / d_[9], d_[3] / 100.0 / d_[9], d_[4] / 100.0 / d_[9], d_[5] / 100.0 / d_[9], d_[6] / 100.0 / d_[9], d_[7] / 100.0 / d_[9], d_[8] / 100.0 / d_[9]);
	else if (d_[3]) fprintf(stderr, "[seed] blocks %llu  avg us: count pass %.1f  sort+scan %.1f  scatter pass %.1f\n", d_[3], d_[0] / 100.0 / d_[3], d_[1] / 100.0 / d_[3], d_[2] / 100.0 / d_[3]);
	return HAO_OK;
}

// seed bins: the counter block zeroed, the seed kernels' arguments, the kernels (hao_seed_launch)
static int hao_q_sort_bins(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint64_t lo = R.lo, hi = R.hi, n = R.n, A = R.A;
	HIP_TRY(B.hits.reserve(A + 1));
	uint64_t max_q = 1;
	for (uint64_t r = lo; r < hi; ++r) max_q = std::max<uint64_t>(max_q, c->h_ix_mz_off[r + 1] - c->h_ix_mz_off[r]);
	const uint64_t sum_q = c->h_ix_mz_off[hi] - c->h_ix_mz_off[lo];      // minimizers of the batch's reads
	int tb = 1; while ((1ULL << tb) < c->n_total) ++tb;
	HIP_TRY(B.g_cnt.reserve(n + 2)); HIP_TRY(B.g_off.reserve(n + 2)); HIP_TRY(B.g_tmp.reserve(A + 1));
	HIP_TRY(B.stats.reserve(HAO_ST_COUNT)); HIP_TRY(hipMemsetAsync(B.stats.p, 0, HAO_ST_COUNT * 8, c->stream));
	hao_seed_args sa_;
	sa_.mz_off = c->d_ix_mz_off.p; sa_.mz_info = c->d_ix_mz_info.p; sa_.rid_lo = lo; sa_.mz0 = B.mz0; sa_.s_start = B.s_start.p; sa_.s_n = B.s_n.p; sa_.a_off = B.a_off.p; sa_.seg = B.seg.p;
	sa_.sinfo = c->d_ix_sinfo.p; sa_.len = c->d_len_all.p; sa_.q_pos = B.q_pos.p; sa_.q_cnt = B.q_cnt.p; sa_.hits = B.hits.p; sa_.g_tmp = B.g_tmp.p; sa_.g_cnt = B.g_cnt.p; sa_.n_sel = n; sa_.tb = tb;
	sa_.qcap = (uint32_t)std::min<uint64_t>((max_q + 63) & ~63ULL, HAO_QTAB_CAP);
	sa_.dbg = nullptr; sa_.hq = nullptr;
	if (R.parts & HAO_DELIVER_CL) {      // the wire format's code array (one byte per seed hit, 0x08 = nothing to say) and, for the quick check's codes, every hit's minimizer index
		HIP_TRY(B.hcode.reserve(A + 64));
		// (the quick-check kernels write every position of every group they see; only the debug paths that bypass them need the array pre-filled)
		if (c->sw.seq_chain || c->sw.dp_seqtail || c->sw.dp_nospec) { const uint64_t n16 = (A + 31) / 16; hipLaunchKernelGGL(hao_fill16_kernel, dim3((unsigned)std::min<uint64_t>((n16 + 255) / 256, 1u << 14)), dim3(256), 0, c->stream, (hao_fill_v4*)B.hcode.p, n16, 0x08080808u); HAO_CHECK_LAUNCH(); }
		HIP_TRY(B.hq.reserve(A + 64)); sa_.hq = B.hq.p;
	}
	if (c->sw.seedphase) { HIP_TRY(B.dbgbuf.reserve(64)); HIP_TRY(hipMemsetAsync(B.dbgbuf.p, 0, 512, c->stream)); sa_.dbg = B.dbgbuf.p; }
	HIP_TRY(B.ovf_list.reserve(3 * (n + 1)));      // the reads each of the three seed launches leaves to the next
	if (int rc = hao_seed_launch(R, sa_, max_q, sum_q)) return rc;
	if (c->sw.seedphase) { if (int rc = hao_seed_dbg_print(c)) return rc; }
	c->timer.mark("q_sort_bins");
	return HAO_OK;
}

// groups: the target groups of every read classified by size, the classes' work lists laid out (their bases read back: the second synchronise) and filled
static int hao_q_groups(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint64_t n = R.n;
	HIP_TRY(B.cls_cc.reserve(HAO_NCLS * (n + 1) + 1)); HIP_TRY(B.cls_co.reserve(HAO_NCLS * (n + 1) + 1));
	hipLaunchKernelGGL(groups_classify_kernel, dim3((unsigned)((n + 4) / 4)), dim3(256), 0, c->stream, B.g_tmp.p, B.seg.p, B.g_cnt.p, n, B.cls_cc.p);
	HAO_CHECK_LAUNCH();
	if (int rc = hao_excl_scan_u64(c, B.cls_cc.p, B.cls_co.p, HAO_NCLS * (n + 1))) return rc;
	hipLaunchKernelGGL(groups_layout_kernel, dim3(1), dim3(64), 0, c->stream, B.cls_co.p, n, B.stat(HAO_ST_CLS_BASE));
	HAO_CHECK_LAUNCH();
	if (int rc = hao_peek(c, B.stat(HAO_ST_CLS_BASE), HAO_NCLS + 1, PK_CLS_BASE)) return rc;
	const double ts1_ = hao_now();
	HIP_TRY(hipStreamSynchronize(c->stream));
	B.t_s2 += hao_now() - ts1_;
	for (int x = 0; x <= HAO_NCLS; ++x) R.L.base[x] = c->peeked(PK_CLS_BASE, x);
	for (int x = 0; x < HAO_NCLS; ++x) R.cls_cnt[x] = R.L.base[x + 1] - R.L.base[x];
	const uint64_t G = R.G = B.n_groups = R.L.base[HAO_NCLS];
	HIP_TRY(B.g_start.reserve(G + 1)); HIP_TRY(B.g_read.reserve(G + 1)); HIP_TRY(B.g_cls.reserve(G + 1)); HIP_TRY(B.glist.reserve(G + 1)); HIP_TRY(B.slow.reserve(G + 1));
	hipLaunchKernelGGL(groups_compact_kernel, dim3((unsigned)((n + 4) / 4)), dim3(256), 0, c->stream, B.g_tmp.p, B.seg.p, B.cls_co.p, n, R.glo, c->d_len_all.p, B.g_off.p, B.g_start.p, B.g_read.p, B.g_cls.p, B.glist.p);
	HAO_CHECK_LAUNCH();
	c->timer.mark("q_groups");
	return HAO_OK;
}

// the side streams of the chain stage (one per size class) and their events, made once; same priority class as the engine's stream (see hao_create)
static int hao_side_streams(hao_ctx *c, hao_ctx::Batch &B)
{
	if (B.side_ready) return HAO_OK;
	int plo_ = 0, phi_ = 0; (void)hipDeviceGetStreamPriorityRange(&plo_, &phi_);
	for (int x = 0; x < HAO_NCLS; ++x) { HIP_TRY(hipStreamCreateWithPriority(&B.side[x], hipStreamNonBlocking, plo_)); HIP_TRY(hipEventCreateWithFlags(&B.ev_qc[x], hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&B.ev_dp[x], hipEventDisableTiming)); }
	B.side_ready = true;
	return HAO_OK;
}

// HAO_DBG_PRINT=qc: the phase timers the quick check left in B.dbgbuf
static int hao_qc_dbg_print(hao_ctx *c)
{
	unsigned long long d_[5]; HIP_TRY(hipMemcpy(d_, c->batch->dbgbuf.p, 40, hipMemcpyDeviceToHost));
	if (d_[3]) fprintf(stderr, "[qc] fast groups %llu (avg %.0f hits)  avg us: entry + tile 0 %.2f  scan loop %.2f  cigar + record %.2f\n", d_[3], (double)d_[4] / d_[3], d_[0] / 100.0 / d_[3], d_[1] / 100.0 / d_[3], d_[2] / 100.0 / d_[3]);
	return HAO_OK;
}

// Q6 chain: quick check per size class, biggest first; the groups it does not settle go to the DP kernel of their class on a side
// stream, so the long sequential DPs of big groups run under the quick checks of the smaller classes
static int hao_q_chain(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint64_t A = R.A, G = R.G; const hao_cls_layout &L = R.L; const unsigned long long *cls_cnt = R.cls_cnt;
	HIP_TRY(B.ohits.reserve(A + 1));
	HIP_TRY(B.fcs.reserve(A + 6 * G + 1)); HIP_TRY(B.rec.reserve(G * HAO_MCOPY_MAX + 1)); HIP_TRY(B.nch.reserve(G + 2)); HIP_TRY(B.nout.reserve(G + 2));
	R.par = hao_chain_params(c->opt.k, R.ps);
	if (G) {
		hao_chain_args ca;
		ca.hits = B.hits.p; ca.g_start = B.g_start.p; ca.g_read = B.g_read.p; ca.g_off = B.g_off.p; ca.seg = B.seg.p; ca.n_groups = G; ca.rid_lo = R.glo; ca.len = c->d_len_all.p; ca.par = R.par;
		ca.dbg_qc = nullptr; ca.hq = nullptr; ca.hcode = nullptr; ca.ohq = nullptr; ca.exc_every = (uint32_t)c->sw.exc_every;
		if (R.parts & HAO_DELIVER_CL) { HIP_TRY(B.ohq.reserve(A + 64)); ca.hq = B.hq.p; ca.hcode = B.hcode.p; ca.ohq = B.ohq.p; }
		if (c->sw.qcphase) { HIP_TRY(B.dbgbuf.reserve(8)); HIP_TRY(hipMemsetAsync(B.dbgbuf.p, 0, 64, c->stream)); ca.dbg_qc = B.dbgbuf.p; }
		ca.stats = B.stats.p; ca.dbg_stats = c->sw.dp_stats ? 1 : 0;
		ca.dbg_seq = c->sw.seq_chain ? 1 : (c->sw.dp_seqtail ? 3 : (c->sw.dp_nospec ? 4 : 0));
		// per-hit DP scratch in global memory is only touched by groups beyond the LDS variants (and the sequential debug path)
		const bool need_scratch = cls_cnt[HAO_NCLS - 1] > 0 || ca.dbg_seq == 1;
		if (need_scratch) { HIP_TRY(B.f.reserve(A + 1)); HIP_TRY(B.ii.reserve(A + 1)); HIP_TRY(B.p.reserve(A + 1)); HIP_TRY(B.t.reserve(A + 1)); HIP_TRY(B.tm.reserve(A + 1)); }
		ca.tm = B.tm.p; ca.f = B.f.p; ca.ii = B.ii.p; ca.p = B.p.p; ca.t = B.t.p; ca.ohits = B.ohits.p; ca.fcs = B.fcs.p; ca.rec = B.rec.p; ca.nch = B.nch.p; ca.nout = B.nout.p;
		if (int rc = hao_side_streams(c, B)) return rc;
		const bool serial = c->sw.dp_serial;      // DP kernels on the main stream (no overlap), for A/B timing
		const int spec_min = 2;      // tiles of <= 64 hits gain nothing from speculation
		const int dbg_seq0 = ca.dbg_seq;
		for (int x = HAO_NCLS - 1; x >= 1; --x) {
			const uint64_t nl = cls_cnt[x]; if (!nl) continue;
			ca.dbg_seq = (dbg_seq0 == 0 && x < spec_min) ? 4 : dbg_seq0;
			const hao_gent *lst = B.glist.p + L.base[x]; uint32_t *slow = B.slow.p + L.base[x];
			hipLaunchKernelGGL(chain_group_kernel, dim3((unsigned)nl), dim3(64), 0, c->stream, ca, lst, nl, slow, x);
			HAO_CHECK_LAUNCH();
			hipStream_t ds = serial ? c->stream : B.side[x];
			if (!serial) { HIP_TRY(hipEventRecord(B.ev_qc[x], c->stream)); HIP_TRY(hipStreamWaitEvent(ds, B.ev_qc[x], 0)); }
			if (x <= 2) hipLaunchKernelGGL(chain_dp128_kernel, dim3((unsigned)std::min<uint64_t>(nl, 256 * 16)), dim3(64), 0, ds, ca, lst, slow, B.stat(HAO_ST_SLOW, x));
			else if (x <= 4) hipLaunchKernelGGL((chain_dp_kernel<512, true>), dim3((unsigned)std::min<uint64_t>(nl, 256 * 8)), dim3(64), 0, ds, ca, lst, slow, B.stat(HAO_ST_SLOW, x));
			else hipLaunchKernelGGL((chain_dp_kernel<HAO_DP_CAP, false>), dim3((unsigned)std::min<uint64_t>(nl, 256 * 3)), dim3(64), 0, ds, ca, lst, slow, B.stat(HAO_ST_SLOW, x));
			HAO_CHECK_LAUNCH();
			if (!serial) HIP_TRY(hipEventRecord(B.ev_dp[x], ds));
		}
		ca.dbg_seq = dbg_seq0;
		if (cls_cnt[0]) {      // groups of <= HAO_TINY_MAX hits: eight per wave through the data-parallel quick check, the rejected ones by one lane each (HAO_DBG_FORCE=seq_chain: all of them)
			const hao_gent *lst0 = B.glist.p + L.base[0]; uint32_t *slow0 = B.slow.p + L.base[0];
			const unsigned nb_lane = (unsigned)std::min<uint64_t>((cls_cnt[0] + 63) / 64, 256 * 64);
			if (ca.dbg_seq == 1) hipLaunchKernelGGL(chain_tiny_kernel, dim3(nb_lane), dim3(64), 0, c->stream, ca, lst0, (uint64_t)cls_cnt[0], (const uint32_t*)nullptr, (const unsigned long long*)nullptr);
			else {
				hipLaunchKernelGGL(chain_pack8_kernel, dim3((unsigned)((cls_cnt[0] + 31) / 32)), dim3(256), 0, c->stream, ca, lst0, (uint64_t)cls_cnt[0], slow0);
				HAO_CHECK_LAUNCH();
				hipLaunchKernelGGL(chain_tiny_kernel, dim3(nb_lane), dim3(64), 0, c->stream, ca, lst0, (uint64_t)cls_cnt[0], (const uint32_t*)slow0, (const unsigned long long*)B.stat(HAO_ST_SLOW));
			}
			HAO_CHECK_LAUNCH();
		}
		if (ca.dbg_qc) { if (int rc = hao_qc_dbg_print(c)) return rc; }
		c->timer.mark("q_chain");
		if (!serial) for (int x = 1; x < HAO_NCLS; ++x) if (cls_cnt[x]) HIP_TRY(hipStreamWaitEvent(c->stream, B.ev_dp[x], 0));
	}
	HIP_TRY(hipMemsetAsync(B.nch.p + G, 0, 4, c->stream)); HIP_TRY(hipMemsetAsync(B.nout.p + G, 0, 4, c->stream));
	c->timer.mark("q_chain_dp");
	return HAO_OK;
}

// cl->list -> wire format (hao_deliver.cuh), on stream st: chain headers; codes of the chains the DP compacted; then ONE pass over the code array the quick check
// filled - bits, rank directory, code bytes of the flagged positions, verbatim list.  (The number of chains is only known on the device here: launches
// cover the bound, the kernels stop at ch_base[G].)  Its scans have a scratch buffer of their own: c->d_tmp belongs to the scans of the selection.
static int hao_wire_pack(hao_run &R, hipStream_t st)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; hao_ctx::Batch::OutSet &O = B.O(); const hao_pack_args &pa = R.pa; const uint64_t A = R.A, G = R.G, NW = R.NW;
	if (!G) return HAO_OK;
	hipLaunchKernelGGL(hao_pack_hdr_kernel, dim3((unsigned)((R.NCmax + 255) / 256)), dim3(256), 0, st, pa, B.ch_base.p + G); HAO_CHECK_LAUNCH();
	hipLaunchKernelGGL(hao_pack_bits_kernel, dim3((unsigned)((NW * 8 + 256 * HAO_PACK_U - 1) / (256 * HAO_PACK_U))), dim3(256), 0, st, pa, A, NW, O.bits.p, B.pk_cnt.p, B.pk_ecnt.p); HAO_CHECK_LAUNCH();      // (the verbatim list: by count + scan, in position order)
	size_t tb = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, tb, B.pk_cnt.p, O.rank.p, 0u, NW + 1, rocprim::plus<uint32_t>(), st)); HIP_TRY(B.pk_tmp.reserve(tb + 256));
	HIP_TRY(rocprim::exclusive_scan(B.pk_tmp.p, tb, B.pk_cnt.p, O.rank.p, 0u, NW + 1, rocprim::plus<uint32_t>(), st));
	HIP_TRY(rocprim::exclusive_scan(B.pk_tmp.p, tb, B.pk_ecnt.p, B.pk_erank.p, 0u, NW + 1, rocprim::plus<uint32_t>(), st));
	hipLaunchKernelGGL(hao_pack_codes_kernel, dim3((unsigned)((NW * 8 + 255) / 256)), dim3(256), 0, st, pa, B.hcode.p, A, O.bits.p, O.rank.p, NW, O.codes.p, B.stat(HAO_ST_CODES), B.pk_erank.p); HAO_CHECK_LAUNCH();
	{ const uint64_t n4 = NW / 4 + 1; hipLaunchKernelGGL(hao_rank4_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, O.rank.p, n4, O.rank4.p); HAO_CHECK_LAUNCH(); }
	return HAO_OK;
}

// HAO_DELIVER_CL: the wire's buffers and arguments, the pack (hao_wire_pack), per-read ranges and the minimizer tables.
// The pack kernels need the chain descriptors (chain_assemble_kernel) and nothing the selection and chain_final_kernel write: they run on a side stream UNDER those
// (one-wave-per-read kernels that leave most of the device idle) and join the engine's stream in front of the batch's totals.  On the engine's stream they were
// 9.4 ms of a configs[2] pass that nothing else ran under.
static int hao_wire_stage(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; hao_ctx::Batch::OutSet &O = B.O(); hao_pack_args &pa = R.pa; const uint64_t lo = R.lo, n = R.n, nm = R.nm, A = R.A, NW = R.NW;
	HIP_TRY(O.hdr.reserve(R.NCmax + 1)); HIP_TRY(O.exc.reserve(c->sw.exc_cap >= 0 ? (uint64_t)c->sw.exc_cap + 1 : std::max<uint64_t>(1 << 14, A / 256)));
	HIP_TRY(O.bits.reserve(NW + 2)); HIP_TRY(O.rank.reserve(NW + 6)); HIP_TRY(O.rank4.reserve(NW / 4 + 2)); HIP_TRY(B.pk_cnt.reserve(NW + 2)); HIP_TRY(O.codes.reserve(A + 16));
	HIP_TRY(B.pk_ecnt.reserve(NW + 2)); HIP_TRY(B.pk_erank.reserve(NW + 2));
	HIP_TRY(O.ch_off.reserve(n + 2)); HIP_TRY(O.cl_off.reserve(n + 2)); HIP_TRY(O.qm_off.reserve(n + 2));
	O.qmz16 = c->max_len_all < 65536 && B.wgt_max < 256 && !c->sw.qmz_raw;
	if (O.qmz16) { HIP_TRY(O.qmz_pos.reserve(nm + 1)); HIP_TRY(O.qmz_cnt.reserve(nm + 1)); } else HIP_TRY(O.qmz.reserve(nm + 1));
	pa.cd = B.cd.p; pa.hits = B.hits.p; pa.ohits = B.ohits.p; pa.mz_off = c->d_ix_mz_off.p; pa.seg = B.seg.p; pa.n_sel = n; pa.rid_lo = lo; pa.mz0 = B.mz0; pa.q_pos = B.q_pos.p;
	pa.hq = B.hq.p; pa.ohq = B.ohq.p;
	pa.hdr = O.hdr.p; pa.bytes = B.hcode.p; pa.exc = O.exc.p; pa.exc_cnt = B.stat(HAO_ST_EXC); pa.exc_every = (uint32_t)c->sw.exc_every;
	pa.exc_cap = c->sw.exc_cap >= 0 ? std::min<uint64_t>(O.exc.cap, (uint64_t)c->sw.exc_cap) : O.exc.cap;
	hipStream_t st = c->stream;
	if (B.side_ready && !c->sw.dp_serial) {      // (the side streams exist once a batch had groups; HAO_DBG_FORCE=dp_serial keeps everything on the engine's stream)
		if (!B.ev_pk0) { HIP_TRY(hipEventCreateWithFlags(&B.ev_pk0, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&B.ev_pk1, hipEventDisableTiming)); }
		st = B.side[0]; R.pack_on_side = true;
		HIP_TRY(hipEventRecord(B.ev_pk0, c->stream)); HIP_TRY(hipStreamWaitEvent(st, B.ev_pk0, 0));
	}
	HIP_TRY(hipMemsetAsync(B.pk_cnt.p + NW, 0, 4, st));      // (the scans run over NW + 1 counts: their last output is the total)
	HIP_TRY(hipMemsetAsync(B.pk_ecnt.p + NW, 0, 4, st));
	if (int rc = hao_wire_pack(R, st)) return rc;
	hipLaunchKernelGGL(hao_read_ranges_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, B.g_off.p, B.ch_base.p, B.cl_base.p, c->d_ix_mz_off.p, lo, B.mz0, n, O.ch_off.p, O.cl_off.p, O.qm_off.p);
	HAO_CHECK_LAUNCH();
	if (nm && O.qmz16) { hipLaunchKernelGGL(hao_qtab16_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, st, B.q_pos.p, B.q_cnt.p, nm, O.qmz_pos.p, O.qmz_cnt.p, c->d_err.p); HAO_CHECK_LAUNCH(); }
	else if (nm) { hipLaunchKernelGGL(hao_qtab_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, st, B.q_pos.p, B.q_cnt.p, nm, O.qmz.p); HAO_CHECK_LAUNCH(); }
	if (R.pack_on_side) HIP_TRY(hipEventRecord(B.ev_pk1, st));
	return HAO_OK;
}

// Q7 assembly: chains, chained hits and fake-cigar entries per group scanned into bases, the chains' records and descriptors (chain_assemble_kernel); with
// HAO_DELIVER_CL the wire pack behind it
static int hao_q_assemble(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint64_t A = R.A, G = R.G;
	HIP_TRY(B.ch_base.reserve(G + 2)); HIP_TRY(B.cl_base.reserve(G + 2)); HIP_TRY(B.fc_base.reserve(G * HAO_MCOPY_MAX + 2)); HIP_TRY(B.nch64.reserve(G * HAO_MCOPY_MAX + 2));
	if (int rc = hao_scan_u32(c, B.nch.p, B.ch_base.p, G + 1)) return rc;
	if (int rc = hao_scan_u32(c, B.nout.p, B.cl_base.p, G + 1)) return rc;
	hipLaunchKernelGGL(hao_fclen_kernel, dim3((unsigned)((G * HAO_MCOPY_MAX + 256) / 256)), dim3(256), 0, c->stream, B.rec.p, B.nch.p, G, B.nch64.p);
	HAO_CHECK_LAUNCH();
	if (int rc = hao_excl_scan_u64(c, B.nch64.p, B.fc_base.p, G * HAO_MCOPY_MAX + 1)) return rc;
	const uint64_t NCmax = R.NCmax = G * HAO_MCOPY_MAX, FCmax = R.FCmax = A + 6 * G;
	R.NW = (A + 63) / 64;
	HIP_TRY(B.ol.reserve(NCmax + 1)); HIP_TRY(B.ol_fc_off.reserve(NCmax + 1)); HIP_TRY(B.cd.reserve(NCmax + 1)); HIP_TRY(B.fc_raw.reserve(FCmax + 1)); HIP_TRY(B.perm.reserve(NCmax + 1));
	if (G) {
		hao_asm_args aa;
		aa.g_start = B.g_start.p; aa.g_read = B.g_read.p; aa.g_cls = B.g_cls.p; aa.g_off = B.g_off.p; aa.n_groups = G; aa.rid_lo = R.glo; aa.ohits = B.ohits.p; aa.hits = B.hits.p; aa.fcs = B.fcs.p; aa.rec = B.rec.p; aa.nch = B.nch.p;
		aa.ch_base = B.ch_base.p; aa.cl_base = B.cl_base.p; aa.fc_base = B.fc_base.p; aa.ol = B.ol.p; aa.ol_fc_off = B.ol_fc_off.p; aa.cd = B.cd.p; aa.fc = B.fc_raw.p;
		hipLaunchKernelGGL(chain_assemble_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, aa); HAO_CHECK_LAUNCH();
	}
	memset(&R.pa, 0, sizeof(R.pa));
	if (R.parts & HAO_DELIVER_CL) { if (int rc = hao_wire_stage(R)) return rc; }
	c->timer.mark("q_assemble");
	return HAO_OK;
}

// HAO_DBG_PRINT=sel: the phase timers the selection left in B.dbgbuf
static int hao_sel_dbg_print(hao_ctx *c)
{
	unsigned long long d_[5]; HIP_TRY(hipMemcpy(d_, c->batch->dbgbuf.p, 40, hipMemcpyDeviceToHost));
	if (d_[4]) fprintf(stderr, "[select] reads %llu  avg us: score sort %.1f  prune %.1f  position sort %.1f  weak filter %.1f\n", d_[4], d_[0] / 100.0 / d_[4], d_[1] / 100.0 / d_[4], d_[2] / 100.0 / d_[4], d_[3] / 100.0 / d_[4]);
	return HAO_OK;
}

// Q8 selection: per read, the chains that survive (hao_select_launch, hao_chain.cuh) and their order; the overlaps and fake-cigar entries per read scanned
static int hao_q_select(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const hao_chain_par &par = R.par; const uint64_t n = R.n, glo = R.glo, NC = R.NCmax;
	{
		uint64_t o = 0;      // coverage windows of the pruning scan: len / ocv_w + 2 per read; offsets by a device scan, the total (a size) from the host's copy of the lengths
		for (uint64_t r = 0; r < n; ++r) o += c->h_len_all[glo + r] / par.ocv_w + 2;
		HIP_TRY(B.cc_off.reserve(n + 2)); HIP_TRY(B.cc.reserve(o + 1)); HIP_TRY(B.n_final.reserve(n + 2)); HIP_TRY(B.fc_final.reserve(n + 2));
		HIP_TRY(B.O().fin_off.reserve(n + 2)); HIP_TRY(B.fcf_off.reserve(n + 2)); HIP_TRY(B.nch64.reserve(n + 2));
		hipLaunchKernelGGL(hao_cc_count_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, c->d_len_all.p, glo, n, (uint64_t)par.ocv_w, B.nch64.p);
		HAO_CHECK_LAUNCH();
		if (int rc = hao_excl_scan_u64(c, B.nch64.p, B.cc_off.p, n + 1)) return rc;
	}
	HIP_TRY(B.key_xs.reserve(NC + 1)); HIP_TRY(B.key_sc.reserve(NC + 1)); HIP_TRY(B.key_al.reserve(NC + 1));
	hao_sel_args sa;
	HIP_TRY(B.key_tmp.reserve(5 * NC + 8));
	sa.key_xs = B.key_xs.p; sa.key_sc = B.key_sc.p; sa.key_al = B.key_al.p; sa.key_tmp = B.key_tmp.p;
	sa.ol = B.ol.p; sa.g_off = B.g_off.p; sa.ch_base = B.ch_base.p; sa.cl_base = B.cl_base.p; sa.cd = B.cd.p; sa.hits = B.hits.p; sa.ohits = B.ohits.p; sa.n_sel = n; sa.rid_lo = glo; sa.len = c->d_len_all.p; sa.cc_off = B.cc_off.p; sa.cc = B.cc.p;
	sa.perm = B.perm.p; sa.n_final = B.n_final.p; sa.fc_final = B.fc_final.p; sa.max_n_chain = par.max_n_chain; sa.ocv_w = par.ocv_w; sa.chain_cutoff = par.chain_cutoff;
	sa.dbg = nullptr; sa.dbg_seq_prune = c->sw.seq_prune ? 1 : 0;
	if (c->sw.selphase) { HIP_TRY(B.dbgbuf.reserve(8)); HIP_TRY(hipMemsetAsync(B.dbgbuf.p, 0, 64, c->stream)); sa.dbg = B.dbgbuf.p; }
	sa.err = c->d_err.p + 1;      // (word 0: hao_qtab16_kernel's, possibly on the side stream)
	HIP_TRY(hao_select_launch(sa, n, c->stream));      // one launch per tier of chain counts (hao_chain.cuh)
	if (int rc = hao_scan_u32(c, B.n_final.p, B.O().fin_off.p, n + 1)) return rc;
	if (int rc = hao_excl_scan_u64(c, B.fc_final.p, B.fcf_off.p, n + 1)) return rc;
	if (sa.dbg) { if (int rc = hao_sel_dbg_print(c)) return rc; }
	c->timer.mark("q_select");
	return HAO_OK;
}

// final: ol->list and the fake cigars in their final order (chain_final_kernel); with HAO_DELIVER_OL as they travel; the wire pack joins the engine's stream
static int hao_q_final(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; hao_ctx::Batch::OutSet &O = B.O(); const uint64_t n = R.n, NCmax = R.NCmax, FCmax = R.FCmax;
	HIP_TRY(O.ol_out.reserve(NCmax + 1)); HIP_TRY(O.fc_out.reserve(FCmax + 1)); HIP_TRY(O.fc_out_off.reserve(NCmax + 2));
	const bool fcw_ = (R.parts & HAO_DELIVER_OL) != 0;
	if (fcw_) { HIP_TRY(O.fcw_off.reserve(NCmax + 2)); HIP_TRY(O.fcw.reserve(3 * (FCmax + 1))); HIP_TRY(O.ol_wire.reserve(NCmax + 1)); }      // main region: entries - overlaps words; raw overlaps behind it: two words per entry
	hipLaunchKernelGGL(chain_final_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, B.ol.p, B.ol_fc_off.p, B.fc_raw.p, B.perm.p, B.g_off.p, B.ch_base.p,
					   O.fin_off.p, B.fcf_off.p, n, O.ol_out.p, O.fc_out.p, O.fc_out_off.p, fcw_ ? O.fcw.p : (uint32_t*)nullptr, fcw_ ? O.fcw_off.p : (uint64_t*)nullptr, B.stat(HAO_ST_FCW), (uint32_t)c->sw.fc_raw_every);
	HAO_CHECK_LAUNCH();
	if (fcw_) { hipLaunchKernelGGL(hao_ol_wire_kernel, dim3((unsigned)std::min<uint64_t>((NCmax + 255) / 256, 4096)), dim3(256), 0, c->stream, O.ol_out.p, O.fin_off.p + n, O.ol_wire.p); HAO_CHECK_LAUNCH(); }
	if (R.pack_on_side) HIP_TRY(hipStreamWaitEvent(c->stream, B.ev_pk1, 0));      // the pack kernels have run under the selection
	c->timer.mark("q_final");
	return HAO_OK;
}

// HAO_DBG_PRINT=dp: what the quick checks left to the DP kernels
static void hao_dp_dbg_print(const hao_run &R, const unsigned long long *slow_st)
{
	fprintf(stderr, "[dp] slow groups by class:"); for (int x = 0; x < HAO_NCLS; ++x) fprintf(stderr, " %llu/%llu", slow_st[HAO_ST_SLOW + x], R.cls_cnt[x]);
	fprintf(stderr, "  hits %llu  dp range %llu  spec-committed %llu  spec-failures %llu\n", slow_st[HAO_ST_SLOW_HITS], slow_st[HAO_ST_SPEC_RANGE], slow_st[HAO_ST_SPEC_OK], slow_st[HAO_ST_SPEC_FAIL]);
}

// more verbatim hits than the wire's list holds: grow it and pack again (the sources are untouched); a synchronise of its own
static int hao_exc_repack(hao_run &R, unsigned long long *n_exc)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; hao_pack_args &pa = R.pa; const uint64_t NW = R.NW;
	HIP_TRY(B.O().exc.reserve(*n_exc + 1024)); pa.exc = B.O().exc.p; pa.exc_cap = B.O().exc.cap;
	HIP_TRY(hipMemsetAsync(B.stat(HAO_ST_EXC), 0, 8, c->stream));
	HIP_TRY(hipMemsetAsync(B.pk_cnt.p + NW, 0, 4, c->stream)); HIP_TRY(hipMemsetAsync(B.pk_ecnt.p + NW, 0, 4, c->stream));
	if (int rc = hao_wire_pack(R, c->stream)) return rc;
	if (int rc = hao_peek(c, B.stat(HAO_ST_EXC), 1, PK_N_EXC)) return rc;
	if (int rc = hao_peek(c, B.stat(HAO_ST_CODES), 1, PK_N_CODES)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	B.n_codes = c->peeked(PK_N_CODES);
	*n_exc = c->peeked(PK_N_EXC);
	return HAO_OK;
}

// the totals of the batch: one wave each gathers them into mapped host memory (the third synchronise); the kernels' error words; the census
static int hao_q_totals(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint32_t parts = R.parts; const uint64_t n = R.n, G = R.G;
	constexpr int N_SLOW = HAO_ST_CLS_BASE - HAO_ST_SLOW;      // the slow statistics: per class, their hits, the speculation's three
	static_assert(HAO_PEEK[PK_SLOW].n == N_SLOW && HAO_PEEK[PK_CLS_BASE].n == HAO_NCLS + 1 && HAO_PEEK[PK_SEED_OVF].n == HAO_ST_L5_CURSOR - HAO_ST_OVF1, "read-back slots sized for the counter block");
	if (int rc = hao_peek(c, B.ch_base.p + G, 1, PK_N_CHAINS)) return rc;
	if (int rc = hao_peek(c, B.cl_base.p + G, 1, PK_N_CL)) return rc;
	if (int rc = hao_peek(c, B.fc_base.p + G * HAO_MCOPY_MAX, 1, PK_N_FC_RAW)) return rc;
	if (int rc = hao_peek(c, B.O().fin_off.p + n, 1, PK_N_OL)) return rc;
	if (int rc = hao_peek(c, B.fcf_off.p + n, 1, PK_N_FC)) return rc;
	if (int rc = hao_peek(c, B.stat(HAO_ST_SLOW), N_SLOW, PK_SLOW)) return rc;
	if (int rc = hao_peek(c, B.stat(HAO_ST_EXC), 1, PK_N_EXC)) return rc;
	if (int rc = hao_peek(c, B.stat(HAO_ST_CODES), 1, PK_N_CODES)) return rc;
	if (int rc = hao_peek(c, B.stat(HAO_ST_FCW), 1, PK_N_FCW)) return rc;
	if (int rc = hao_peek(c, B.stat(HAO_ST_OVF1), HAO_PEEK[PK_SEED_OVF].n, PK_SEED_OVF)) return rc;
	if (int rc = hao_peek(c, c->d_err.p, 1, PK_ERR)) return rc;
	const double ts2_ = hao_now();
	HIP_TRY(hipStreamSynchronize(c->stream));
	B.t_s3 += hao_now() - ts2_; B.t_run += hao_now() - R.t0; ++B.t_nrun;
	if (c->sw.dltime && (B.t_nrun & 15) == 0) fprintf(stderr, "[batch] %llu runs (parts %u): total %.1f ms  before sync1 %.1f  sync1 %.1f  sync2 %.1f  sync3 %.1f\n", (unsigned long long)B.t_nrun, parts, B.t_run * 1e3, B.t_pre * 1e3, B.t_s1 * 1e3, B.t_s2 * 1e3, B.t_s3 * 1e3);
	B.n_chains = c->peeked(PK_N_CHAINS); B.n_cl = c->peeked(PK_N_CL); B.n_fc_raw = c->peeked(PK_N_FC_RAW); B.n_ol = c->peeked(PK_N_OL); B.n_fc = c->peeked(PK_N_FC);
	unsigned long long slow_st[N_SLOW], n_exc = 0;
	for (int x = 0; x < N_SLOW; ++x) slow_st[x] = c->peeked(PK_SLOW, x);
	B.seed_left[0] = c->peeked(PK_SEED_OVF, HAO_ST_OVF0 - HAO_ST_OVF1); B.seed_left[1] = c->peeked(PK_SEED_OVF, 0); B.seed_left[2] = c->peeked(PK_SEED_OVF, HAO_ST_OVF2 - HAO_ST_OVF1);      // reads left by the first seed launch / by the 512-slot / by the 1024-slot table
	if (parts & HAO_DELIVER_CL) { n_exc = c->peeked(PK_N_EXC); B.n_codes = G ? c->peeked(PK_N_CODES) : 0; }
	const unsigned long long err = c->peeked(PK_ERR);
	if ((parts & HAO_DELIVER_CL) && (uint32_t)err) { hao_set_err(c, "a minimizer position or seed weight that does not fit the packed minimizer table"); return HAO_EUNSUPP; }      // (hao_qtab16_kernel; the host's bounds rule it out)
	if (err >> 32) { hao_set_err(c, "selection sort: more sub-ranges alive in one level than its list holds"); return HAO_EUNSUPP; }      // (hao_block_intro_sort's bound, hao_chain.cuh)
	if ((parts & HAO_DELIVER_OL) && (c->peeked(PK_N_FCW) >> 63)) { hao_set_err(c, "an overlap without fake-cigar entries: the packed cigar layout holds at least one per overlap"); return HAO_EUNSUPP; }
	B.n_fcw = (parts & HAO_DELIVER_OL) ? (B.n_fc - B.n_ol) + c->peeked(PK_N_FCW) : 0;      // main region + the raw overlaps' words
	if ((parts & HAO_DELIVER_CL) && n_exc > R.pa.exc_cap) { if (int rc = hao_exc_repack(R, &n_exc)) return rc; }
	B.n_exc = n_exc;
	B.n_generic = 0; for (int x = 0; x < HAO_NCLS; ++x) B.n_generic += slow_st[HAO_ST_SLOW + x];
	B.n_generic_hits = slow_st[HAO_ST_SLOW_HITS];
	for (int x = 0; x < HAO_NCLS; ++x) { B.cls_n[x] = R.cls_cnt[x]; B.slow_n[x] = slow_st[HAO_ST_SLOW + x]; }
	if (c->sw.dp_stats) hao_dp_dbg_print(R, slow_st);
	B.valid = true;
	return HAO_OK;
}

// the delivery stages the caller asked for, over the final ol->list, then the copy of everything queued into the slot's arena
static int hao_q_deliver(hao_run &R)
{
	hao_ctx *c = R.c; hao_ctx::Batch &B = R.B; const uint32_t parts = R.parts;
	if (parts & HAO_DELIVER_EXACT) { if (int rc = hao_exact_run(c)) return rc; }
	if (parts & HAO_DELIVER_ED) { if (int rc = hao_ed_deliver_run(c)) return rc; }
	if (parts & HAO_DELIVER_TRACE) { if (int rc = hao_trace_deliver_run(c)) return rc; }
	// HAO_DELIVER_RESCUE / HAO_DELIVER_WLIST: the blocking calls' runners over what HAO_DELIVER_ED has just left, into the output set; their counts (c->rs_nw, c->rs_total, c->wl_out) size the arena parts
	if (parts & HAO_DELIVER_RESCUE) { if (int rc = hao_rescue_run(c, hao_ref_io_out(c))) return rc; c->timer.mark("rescue"); }
	if (parts & HAO_DELIVER_WLIST) { if (int rc = hao_wlist_run(c, hao_ref_io_out(c))) return rc; c->timer.mark("wlist"); }
	if (!parts) return HAO_OK;
	const double t0_ = hao_now(); const int rc_ = hao_deliver_enqueue(c); B.t_enq += hao_now() - t0_; ++B.t_n;
	if (c->sw.dltime && (B.t_n & 15) == 0) fprintf(stderr, "[deliver] %llu batches: slot wait %.1f ms, enqueue %.1f ms (arena alloc %.1f ms)\n", (unsigned long long)B.t_n, B.t_evsync * 1e3, B.t_enq * 1e3, B.t_alloc * 1e3);
	return rc_;
}

// parts = 0: results stay in HBM (blocking API).  parts != 0 (hao_overlap_batch_async): the batch computes into output set `dl_seq & 1`, packs cl->list
// into the wire format and queues the copy of everything asked for into that slot's pinned arena on the copy stream.
static int hao_overlap_run(hao_ctx *c, uint64_t lo, uint64_t hi, const hao_pass_t &ps, uint32_t parts = 0, int *slot_out = nullptr)
{
	if (ps.apend_be != 1 || ps.is_accurate != 1 || ps.gen_off != 1 || ps.mcopy_num > HAO_MCOPY_MAX || ps.ocv_w == 0) { hao_set_err(c, "unsupported h_ec_lchain arguments"); return HAO_EUNSUPP; }
	if (int rc = hao_view_refresh(c)) return rc;
	if (!c->has_pt) { hao_set_err(c, "hao_pt_gen must run before hao_overlap_batch"); return HAO_EINVAL; }
	if (!c->batch) c->batch = new hao_ctx::Batch();
	hao_ctx::Batch &B = *c->batch;
	hao_run R{c, B, ps, parts, hao_now()};
	if (int rc = hao_q_begin(R, lo, hi, slot_out)) return rc;
	if (R.n == 0) { B.n_anchor = B.n_groups = B.n_chains = B.n_cl = B.n_ol = B.n_fc = B.n_fcw = B.n_mz = 0; B.valid = true; return HAO_OK; }      // (an empty delivery: nothing to copy, the view stays zeroed)
	if (int rc = hao_q_lookup(R)) return rc;         // seed_unpack_kernel -> seed hits per minimizer                        [sync 1: their total]
	if (int rc = hao_q_sort_bins(R)) return rc;      // seed_lds_kernel / seed_bin*_kernel -> k_mer_hits + target groups
	if (int rc = hao_q_groups(R)) return rc;         // groups_*_kernel -> work lists per size class                         [sync 2: their layout]
	if (int rc = hao_q_chain(R)) return rc;          // chain_group / pack8 / tiny kernels, chain_dp*_kernel on side streams
	if (int rc = hao_q_assemble(R)) return rc;       // chain_assemble_kernel (+ the wire pack on a side stream)
	if (int rc = hao_q_select(R)) return rc;         // chain_select*_kernel
	if (int rc = hao_q_final(R)) return rc;          // chain_final_kernel -> ol->list, fake cigars
	if (int rc = hao_q_totals(R)) return rc;         //                                                                      [sync 3: the totals]
	return hao_q_deliver(R);                         // exact check, window stages, the copy queued
}

// cl->list of the batch as tagged k_mer_hits in HBM: built on demand from the chain descriptors (the blocking fetch API and the digests read it;
// the streaming delivery path packs straight from the descriptors and never needs it)
static int hao_batch_materialize_cl(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch;
	if (B.cl_valid) return HAO_OK;
	HIP_TRY(B.cl.reserve(B.n_cl + 1));
	if (B.n_chains) {
		hipLaunchKernelGGL(chain_materialize_kernel, dim3((unsigned)((B.n_chains + 3) / 4)), dim3(256), 0, c->stream, B.cd.p, B.n_chains, B.hits.p, B.ohits.p, B.cl.p);
		HAO_CHECK_LAUNCH();
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
	B.cl_valid = true;
	return HAO_OK;
}

// host copies for the fetch API (one bulk download per batch)
static int hao_batch_download(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch;
	if (B.host_valid) return HAO_OK;
	if (int rc = hao_batch_materialize_cl(c)) return rc;
	const uint64_t n = B.n;
	B.h_seg.assign(n + 1, 0); B.h_fin_off.assign(n + 1, 0); B.h_cl_off.assign(n + 1, 0);
	B.h_hits.resize(B.n_anchor); B.h_cl.resize(B.n_cl); B.h_ol.resize(B.n_ol); B.h_fc.resize(B.n_fc); B.h_fc_out_off.assign(B.n_ol + 1, 0);
	if (n) {
		HIP_TRY(hipMemcpy(B.h_seg.data(), B.seg.p, (n + 1) * 8, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(B.h_fin_off.data(), B.O().fin_off.p, (n + 1) * 8, hipMemcpyDeviceToHost));
		std::vector<uint64_t> goff(n + 1), clb(B.n_groups + 1);
		HIP_TRY(hipMemcpy(goff.data(), B.g_off.p, (n + 1) * 8, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(clb.data(), B.cl_base.p, (B.n_groups + 1) * 8, hipMemcpyDeviceToHost));
		for (uint64_t r = 0; r <= n; ++r) B.h_cl_off[r] = clb[goff[r]];
	}
	if (B.n_anchor) HIP_TRY(hipMemcpy(B.h_hits.data(), B.hits.p, B.n_anchor * sizeof(hao_hit_t), hipMemcpyDeviceToHost));
	if (B.n_cl) HIP_TRY(hipMemcpy(B.h_cl.data(), B.cl.p, B.n_cl * sizeof(hao_hit_t), hipMemcpyDeviceToHost));
	if (B.n_ol) {
		HIP_TRY(hipMemcpy(B.h_ol.data(), B.O().ol_out.p, B.n_ol * sizeof(hao_ovlp_t), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(B.h_fc_out_off.data(), B.O().fc_out_off.p, B.n_ol * 8, hipMemcpyDeviceToHost));
	}
	B.h_fc_out_off[B.n_ol] = B.n_fc;
	if (B.n_fc) HIP_TRY(hipMemcpy(B.h_fc.data(), B.O().fc_out.p, B.n_fc * 8, hipMemcpyDeviceToHost));
	B.host_valid = true;
	return HAO_OK;
}
