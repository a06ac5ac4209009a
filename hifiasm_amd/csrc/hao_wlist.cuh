// The product of align_hc_ed_post_extz (Correct.cpp:12951-13012) in reference placement: z->w_list, the window records of an overlap with their alignments, as
// the reference holds them once every window has been through gen_backtrace_adv_exz (:12563-12639; recal_boundary_exz :2429-2468).  It runs after the rescue
// stage (hao_rescue.cuh) over what that stage left: the CSR slots' error byte and pattern end, the rescue records and the verdicts.  Overlaps with verdict 0 get
// no record (the reference drops them, :25637).
//
// The trace of a window is a pure function of the record align_hc_ed_post_extz left, so every window is traced here, eagerly, from that record:
//   a first-placement window (with or without an anchor record)   hao_ref_pair, the primary (err, pe)
//   a forward-rescued window                                      hao_rescue_pair from its predecessor's y_end + 1 (the predecessor's record as the rescue left it)
//   a backward-rescued window                                     hao_rescue_pair from its successor's final y_start - its own length
// Backward windows and anchors were traced by the rescue stage already, which keeps no walk; they are traced again here from the same task, which gives the same
// (y_start, y_end, err, re-placed) - the stage reads nothing the rescue stage would have to keep for it, and hao_rs_round_kernel stays as it is.
//   1. hao_wl_count_kernel + a scan: records per overlap (one per aligned slot of an overlap with verdict 1);
//   2. hao_wl_plan_kernel: a thread per overlap writes per record its source, its task parameters, the record itself where no sweep is needed (err == 0: the
//      traced function's shortcut, Levenshtein_distance.h:3783-3787; a task outside hao_tg_semi_domain: distance-only values, flagged untraced) and a sort key;
//   3. a stable sort of the records that need a sweep by (query read, grid window): text order, so that a wave's 64 lanes mostly share one text in LDS;
//   4. hao_wl_trace_kernel: a lane per such record - the task rebuilt in the lane, the traced sweep (three-word columns) and walk, recal_boundary_exz's
//      re-placement as a second sweep of the same launch under a wave-uniform ballot, the record, the cigar row;
//   5. a scan of the entry counts and hao_wl_fill_kernel: the rows (and the single match run of the err == 0 records) into the CSR cigar array.
#pragma once
#include "hao_rescue.cuh"

#define HAO_WL_PRIMARY 3u                 // source of a first-placement window the rescue did not trace (hao.h: HAO_WLIST_PRIMARY)
#define HAO_WL_UNTRACED (1u << 19)        // (hao.h: HAO_WLIST_UNTRACED)
#define HAO_WL_NEED 0x80000000u           // plan: the record needs a sweep
// (hao_wl_plan lives in hao_grid_pair.cuh)
struct hao_wl_args { hao_rs_args A; const uint64_t *rbase; const hao_rs_win *rec; const hao_rs_ovlp *ov; };

// cnt[i] = records of overlap i, i = 0 .. n_ol (cnt[n_ol] = 0 for the scan)
__global__ void hao_wl_count_kernel(hao_wl_args W, uint64_t *cnt)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > W.A.n_ol) return;
	uint64_t n = 0;
	if (i < W.A.n_ol && W.ov[i].verdict) {
		const uint64_t s0 = W.A.win_off[i], nw = W.A.win_off[i + 1] - s0;
		const hao_rs_win *rw = W.rbase[i] == UINT64_MAX ? nullptr : W.rec + W.rbase[i];
		for (uint64_t k = 0; k < nw; ++k) n += W.A.werr[s0 + k] != 0xff || (rw && (rw[k].info & HAO_RS_VALID));
	}
	cnt[i] = n;
}

// entries of one match run of ql bases in push_trace's encoding (split at 0x3fff)
HAO_AL_FN uint64_t hao_wl_run_entries(int64_t ql) { return (uint64_t)(ql / 0x3fff) + (ql % 0x3fff ? 1 : 0); }

// the task of record (slot k, source src) of overlap z (hao_wlist.cuh's table); toff: hao_rescue_pair's target offset of a rescued window
__device__ __forceinline__ bool hao_wl_task(const hao_rs_args &A, const hao_ovlp_t &z, uint64_t s0, uint32_t k, uint32_t src, int64_t toff, hao_ed_task_t *T)
{
	const uint32_t w0 = z.x_pos_s / A.wl, tl = A.len[z.y_id];
	return (src == HAO_WL_PRIMARY || src == 2u) ? hao_ref_pair(z, w0 + k, A.wl, A.shift[s0 + k], A.tab, tl, T) : hao_rescue_pair(z, w0 + k, A.wl, toff, A.tab, tl, T);
}

// a thread per overlap; woff = the scan of hao_wl_count_kernel's counts.  ctr[0] += records that need a sweep, ctr[1] += bound of the cigar entries, ctr[2] += untraced records,
// ctr[5] += records whose task could not be rebuilt (none by construction; the host fails the call if there is one)
__global__ __launch_bounds__(256) void hao_wl_plan_kernel(hao_wl_args W, const uint64_t *woff, hao_wl_plan *plan, hao_rs_win *wins, uint64_t *ncig, uint64_t *key, uint32_t *idx, uint32_t wbits, unsigned long long *ctr)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const hao_rs_args &A = W.A;
	unsigned long long ns = 0, nb = 0, nu = 0, nx = 0;
	if (i < A.n_ol && W.ov[i].verdict) {
		const hao_ovlp_t z = A.ol[i];
		const uint64_t s0 = A.win_off[i]; const uint32_t nw = (uint32_t)(A.win_off[i + 1] - s0), w0 = z.x_pos_s / A.wl, tl = A.len[z.y_id];
		const hao_rs_win *rw = W.rbase[i] == UINT64_MAX ? nullptr : W.rec + W.rbase[i];
		uint64_t g = woff[i];
		for (uint32_t k = 0; k < nw; ++k) {
			const bool pr = A.werr[s0 + k] != 0xff, rv = rw && (rw[k].info & HAO_RS_VALID);
			if (!pr && !rv) continue;
			int64_t qs, ql; hao_ref_window(z, w0 + k, A.wl, &qs, &ql);
			hao_ed_task_t T; T.p_pos = T.p_len = T.t_len = T.thre = T.abs_diag = 0;
			uint32_t src, err, flags = 0; int64_t toff = 0; int32_t ye; bool ok = false;
			if (pr) {
				src = rv ? 2u : HAO_WL_PRIMARY; err = A.werr[s0 + k];
				ok = hao_ref_pair(z, w0 + k, A.wl, A.shift[s0 + k], A.tab, tl, &T);
				ye = (int32_t)T.p_pos + (int32_t)A.wpe[s0 + k];
			} else {
				const hao_rs_win r = rw[k];
				src = HAO_RESCUE_DIR(r.info); err = r.info & 0xffu; ye = r.y_end; flags = r.info & HAO_RESCUE_REPLACED;
				if (src == 0u && k > 0) {      // forward: from the end of the window before - a rescue record (a forward window, or the anchor as the rescue left it) or a primary result
					int32_t pye;
					if (rw[k - 1].info & HAO_RS_VALID) pye = rw[k - 1].y_end;
					else { hao_ed_task_t P; P.p_pos = 0; hao_ref_pair(z, w0 + k - 1, A.wl, A.shift[s0 + k - 1], A.tab, tl, &P); pye = (int32_t)P.p_pos + (int32_t)A.wpe[s0 + k - 1]; }
					toff = (int64_t)pye + 1; ok = true;
				} else if (src == 1u && k + 1 < nw && (rw[k + 1].info & HAO_RS_VALID)) { toff = (int64_t)rw[k + 1].y_start - ql; ok = true; }      // backward: ends where the window after starts
				ok = ok && hao_rescue_pair(z, w0 + k, A.wl, toff, A.tab, tl, &T);
				if (!ok) { T.p_pos = (uint32_t)r.y_start; T.thre = (r.info >> 8) & 0xffu; }
			}
			hao_rs_win o; o.win = w0 + k; o.y_end = ye; o.y_start = (int32_t)T.p_pos;
			uint64_t nc = 0; uint32_t need = 0;
			if (err == 0) { o.y_start = ye - (int32_t)(ql - 1); nc = hao_wl_run_entries(ql); nb += nc; }
			else if (!ok) { flags = HAO_WL_UNTRACED; ++nx; }      // (the record's task cannot be rebuilt: a broken invariant, the call fails)
			else if (!hao_tg_semi_domain(T)) { flags = HAO_WL_UNTRACED; ++nu; }
			else { need = HAO_WL_NEED; flags = 0; ++ns; nb += hao_tg_bound(T, err); }
			o.info = err | T.thre << 8 | src << 16 | flags;
			wins[g] = o; ncig[g] = nc;
			hao_wl_plan P; P.ol = (uint32_t)i; P.ks = k | src << 28 | need; P.toff = toff; plan[g] = P;
			// (wbits: bits of a grid window index; the sort looks at the key's low wbits + read bits only, in which UINT64_MAX is still the largest)
			key[g] = need ? ((uint64_t)z.x_id << wbits | (uint64_t)(w0 + k)) : UINT64_MAX; idx[g] = (uint32_t)g;
			++g;
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) { ns += __shfl_xor(ns, d); nb += __shfl_xor(nb, d); nu += __shfl_xor(nu, d); nx += __shfl_xor(nx, d); }
	if ((threadIdx.x & 63) == 0) { if (ns) atomicAdd(ctr, ns); if (nb) atomicAdd(ctr + 1, nb); if (nu) atomicAdd(ctr + 2, nu); if (nx) atomicAdd(ctr + 5, nx); }
}

// One lane per record of the slice sel[0 .. m) (record indices in text order): path = the column scratch (three words per text column, `stride` lanes per
// row); rows = two rows of cap entries per lane (the walk, and the re-placement's walk, which replaces the first only if it is taken); rowof[g] = the lane's
// place row0 + slot.  ctr[3] += re-placement sweeps, ctr[4] += records whose traced sweep found no alignment or whose walk has more entries than a row (none by
// construction: the cleared traced function finds the distance-only result again, hao_tg_bound bounds the walk; the host fails the call if there is one)
__global__ __launch_bounds__(256) void hao_wl_trace_kernel(hao_ed_reads R, hao_wl_args W, const hao_wl_plan *plan, const uint32_t *sel, uint64_t m, uint64_t row0, uint64_t *path, uint64_t stride,
		uint16_t *rows, uint32_t cap, hao_rs_win *wins, uint64_t *ncig, uint32_t *rowof, unsigned long long *ctr)
{
	__shared__ uint8_t s_text[4][HAO_AL_CH];
	const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t slot = ((uint64_t)blockIdx.x * 4 + wv) * 64 + lane;
	const hao_rs_args &A = W.A;
	hao_ed_task_t T; T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	bool mine = false; uint32_t g = 0; int64_t tl = 0;
	if (slot < m) {
		g = sel[slot]; const hao_wl_plan P = plan[g]; const hao_ovlp_t z = A.ol[P.ol];
		mine = hao_wl_task(A, z, A.win_off[P.ol], P.ks & 0x0fffffffu, (P.ks >> 28) & 3u, P.toff, &T);      // (always true: the plan kernel built the same task)
		tl = A.len[z.y_id];
	}
	// (a lane without a task must not look like its neighbour's text: the sweep starts a text segment where a lane's text differs from its left neighbour's)
	if (!mine) T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	uint64_t *col = path + slot;
	uint16_t *row = rows + (row0 + (slot < m ? slot : 0)) * 2 * (uint64_t)cap;
	hao_al_state<uint64_t> S;
	hao_al_tile_sweep<uint64_t, HAO_AL_SEMI, true, 3>(R, T, mine, S, s_text[wv], lane, col, stride);
	hao_trace_result_t res; res.err = HAO_AL_NONE; res.ps = -1; res.pe = -1; res.n_cigar = 0;
	bool need2 = false; hao_ed_task_t T2 = T;
	if (mine) {
		hao_al_finish<uint64_t, HAO_AL_SEMI, true, 3>(S, T, res, col, stride, row, cap);
		// recal_boundary_exz's condition and its new placement
		if (res.err != HAO_AL_NONE && res.err > 0 && (res.pe + 1 == (int32_t)T.p_len || res.ps == 0)) {
			const int64_t ql = T.t_len, ts = res.ps == 0 ? (int64_t)T.p_pos : (int64_t)T.p_pos + res.pe - ql + 1;
			int64_t rs, rl, ab;
			if (hao_rs_init_waln(T.thre, ts, tl, ql + 2 * (int64_t)T.thre, &rs, &rl, &ab) && !(rs == (int64_t)T.p_pos && rl == (int64_t)T.p_len)) {
				T2.p_pos = (uint32_t)rs; T2.p_len = (uint32_t)rl; T2.abs_diag = (uint32_t)ab;
				need2 = hao_tg_semi_domain(T2);      // (outside the domain: the first trace stands)
			}
		}
	}
	uint32_t replaced = 0;
	if (!need2) T2.p_rid = T2.p_pos = T2.p_len = T2.p_rev = T2.t_rid = T2.t_pos = T2.t_len = T2.t_rev = T2.thre = T2.abs_diag = 0;
	const unsigned long long retry = __ballot(need2);
	if (retry) {      // (wave-uniform)
		hao_al_state<uint64_t> S2;
		hao_al_tile_sweep<uint64_t, HAO_AL_SEMI, true, 3>(R, T2, need2, S2, s_text[wv], lane, col, stride);
		if (need2) {
			hao_trace_result_t r2; r2.err = HAO_AL_NONE; r2.ps = -1; r2.pe = -1; r2.n_cigar = 0;
			hao_al_finish<uint64_t, HAO_AL_SEMI, true, 3>(S2, T2, r2, col, stride, row + cap, cap);
			if (r2.err != HAO_AL_NONE && r2.err < res.err) {
				res = r2; T = T2; replaced = 1;
				for (int32_t j = 0; j < r2.n_cigar && (uint32_t)j < cap; ++j) row[j] = row[cap + j];
			}
		}
	}
	bool lost = false;
	if (mine) {
		hao_rs_win o = wins[g];
		if (res.err != HAO_AL_NONE) {
			o.y_start = (int32_t)T.p_pos + res.ps; o.y_end = (int32_t)T.p_pos + res.pe;
			o.info = (o.info & 0x00ffff00u) | (uint32_t)res.err | (replaced ? HAO_RESCUE_REPLACED : 0u);
			if ((uint32_t)res.n_cigar > cap) lost = true;      // (more entries than hao_tg_bound allows: counted, the host fails the call)
			ncig[g] = (uint32_t)res.n_cigar <= cap ? (uint64_t)res.n_cigar : 0;
		} else { o.info |= HAO_WL_UNTRACED; ncig[g] = 0; lost = true; }
		wins[g] = o; rowof[g] = (uint32_t)(row0 + slot);
	}
	const unsigned long long nl = __ballot(lost);
	if (lane == 0) { if (retry) atomicAdd(ctr + 3, (unsigned long long)__popcll(retry)); if (nl) atomicAdd(ctr + 4, (unsigned long long)__popcll(nl)); }
}

// a thread per record: its entries into the CSR array (off = the scan of ncig) - the lane's row, or the match run of an err == 0 record
__global__ void hao_wl_fill_kernel(hao_wl_args W, const hao_wl_plan *plan, const hao_rs_win *wins, uint64_t n, const uint64_t *off, const uint32_t *rowof, const uint16_t *rows, uint32_t cap, uint16_t *cig, uint64_t cig_cap)
{
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= n) return;
	const uint64_t a = off[g], nk = off[g + 1] - a;
	if (nk == 0) return;
	const hao_wl_plan P = plan[g];
	if (P.ks & HAO_WL_NEED) {
		const uint16_t *row = rows + (uint64_t)rowof[g] * 2 * cap;
		for (uint64_t j = 0; j < nk && j < cap && a + j < cig_cap; ++j) cig[a + j] = row[j];
	} else {
		int64_t qs, ql; hao_ref_window(W.A.ol[P.ol], wins[g].win, W.A.wl, &qs, &ql);
		for (uint64_t j = 0; j < nk && a + j < cig_cap; ++j) { const int64_t rem = ql - (int64_t)j * 0x3fff; cig[a + j] = (uint16_t)(rem >= 0x3fff ? 0x3fff : rem); }
	}
}
