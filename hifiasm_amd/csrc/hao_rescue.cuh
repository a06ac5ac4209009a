// The second half of align_hc_ed_post_extz (Correct.cpp:12951-13012) on the device: the rescue of the windows that did not align at first placement
// (push_hc_wlst_exz :12776-12836, aln_wlst_adv_exz :4057-4131, gen_backtrace_adv_exz :12563-12639, recal_boundary_exz :2429-2468), the exit test after every
// aligned window and the return value.  It runs after the reference-placed distance-only stage over that stage's CSR slots: the error byte and the pattern end
// of every (overlap, covered window).
//
// Why a lane per OVERLAP and not per gap: a run of open windows between two aligned ones is rescued forwards from its left anchor and backwards from its right
// one, and the right anchor is traced for that - which may RE-PLACE it (recal_boundary_exz), and the re-placed y_end is where the forward run of the NEXT gap
// starts.  So an overlap's gaps form one chain; the chains of different overlaps are independent.  Fewer than 1 % of the overlaps have an open window before an
// aligned one, so:
//   1. hao_rs_gap_kernel: a thread per overlap finds those overlaps (one pass to count them and their slots, one to hand out a state and a record region each);
//   2. hao_rs_round_kernel: a lane per such overlap.  Its state names the ONE alignment the chain waits for - a forward window, the anchor's trace, a backward
//      window; the lane rebuilds that task (hao_rescue_pair / hao_ref_pair), the wave sweeps its 64 tasks together (hao_al_tile_sweep, three-word columns), the
//      lane walks back where the step is traced, runs the recal_boundary_exz retry as a second sweep of the same launch where its condition holds, applies
//      the result and steps its state to the next alignment.  Rounds repeat until a launch reports no lane left; the host reads that one count per round.
//   3. hao_rs_verdict_kernel: a thread per overlap, every overlap: the running align_length over its slots and rescued records, the exit window, the verdict;
//      records beyond the exit are dropped (the reference never computed them).
// Cigars are not kept: only ps, pe and err of a traced step are used (hao_wlist.cuh traces every window of a passing overlap again and keeps the walks).
#pragma once
#include "hao_align.cuh"
#include "hao_grid_pair.cuh"
#include "hao_trace_grid.cuh"      // (hao_tg_semi_domain)

struct hao_rs_args { const hao_ovlp_t *ol; uint64_t n_ol; uint32_t wl; const uint64_t *win_off; const int16_t *shift; const uint8_t *tab; const uint8_t *werr; const uint16_t *wpe; const uint32_t *len; };
// control phases (resolved inside a lane without an alignment) and the three phases that wait for one
enum { HAO_RS_SEEK = 0, HAO_RS_FWD_CHECK, HAO_RS_BWD_START, HAO_RS_BWD_CHECK, HAO_RS_PUSH, HAO_RS_FWD, HAO_RS_ANCHOR, HAO_RS_BWD, HAO_RS_DONE };
enum { HAO_RS_A_TRACED = 1, HAO_RS_A_REPLACED = 2, HAO_RS_A_UNTRACED = 4 };
// (hao_rs_state, the lane's state, lives in hao_grid_pair.cuh: the context holds a buffer of them)

// the pattern end of every pair into its overlap's CSR slot (the blocking path keeps pe per pair)
__global__ void hao_rs_scatter_pe_kernel(const hao_ovlp_t *ol, const hao_ed_pair *pairs, const hao_ed_result_t *res, uint64_t n, uint32_t wl, const uint64_t *win_off, uint16_t *wpe)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const hao_ed_pair q = pairs[p];
	if (res[p].err != 0x7fffffff) wpe[win_off[q.ol] + (q.w - ol[q.ol].x_pos_s / wl)] = (uint16_t)res[p].pe;
}

// the same from the delivery path's compact records (an error byte and a 16-bit pattern end per pair)
__global__ void hao_rs_scatter_pe16_kernel(const hao_ovlp_t *ol, const hao_ed_pair *pairs, const uint8_t *err, const uint16_t *pe, uint64_t n, uint32_t wl, const uint64_t *win_off, uint16_t *wpe)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const hao_ed_pair q = pairs[p];
	if (err[p] != 0xff) wpe[win_off[q.ol] + (q.w - ol[q.ol].x_pos_s / wl)] = pe[p];
}

// ASSIGN = false: ctr[0] += overlaps with an open window before an aligned one, ctr[1] += their covered windows.  ASSIGN = true: each of them takes a state
// (ctr[2]) and a record region of one slot per covered window (ctr[3]); rbase[i] = the region's start, UINT64_MAX for the others
template<bool ASSIGN>
__global__ __launch_bounds__(256) void hao_rs_gap_kernel(hao_rs_args A, unsigned long long *ctr, uint64_t *rbase, hao_rs_state *st, hao_rs_win *rec)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool act = false; uint32_t nw = 0;
	if (i < A.n_ol) {
		const uint64_t s0 = A.win_off[i]; nw = (uint32_t)(A.win_off[i + 1] - s0);
		bool open = false;
		for (uint32_t k = 0; k < nw; ++k) { if (A.werr[s0 + k] == 0xff) open = true; else if (open) { act = true; break; } }
	}
	if (!ASSIGN) {
		unsigned long long na = act ? 1 : 0, ns = act ? nw : 0;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) { na += __shfl_xor(na, d); ns += __shfl_xor(ns, d); }
		if ((threadIdx.x & 63) == 0 && na) { atomicAdd(ctr, na); atomicAdd(ctr + 1, ns); }
	} else if (i < A.n_ol) {
		if (!act) { rbase[i] = UINT64_MAX; return; }
		const unsigned long long a = atomicAdd(ctr + 2, 1ULL), b = atomicAdd(ctr + 3, (unsigned long long)nw);
		rbase[i] = b;
		hao_rs_state S; S.ol = (uint32_t)i; S.phase = HAO_RS_SEEK; S.k = -1; S.j = 0; S.last = -1; S.cs = 0; S.aflags = 0; S.a_ys = S.a_ye = S.a_err = 0; S.toff = 0; S.base = b;
		st[a] = S;
		hao_rs_win z; z.y_start = z.y_end = 0; z.win = 0; z.info = 0;
		for (uint32_t k = 0; k < nw; ++k) rec[b + k] = z;
	}
}

// init_waln (Correct.cpp:764-779)
HAO_AL_FN bool hao_rs_init_waln(int64_t thre, int64_t s, int64_t l, int64_t wln, int64_t *rs, int64_t *rl, int64_t *ab)
{
	if (s < 0 || s >= l || l - s + 2 * thre + 31 < wln) return false;
	*rs = s - thre; *rl = l - *rs; *ab = 0;
	if (*rl > wln) *rl = wln;
	if (*rs < 0) { *ab = -*rs; *rs = 0; *rl -= *ab; }
	return true;
}

// steps the state through its control phases until it waits for an alignment (true; *T = its task) or the overlap is finished (false)
__device__ __forceinline__ bool hao_rs_advance(const hao_rs_args &A, const hao_ovlp_t &z, hao_rs_state &S, hao_rs_win *rec, hao_ed_task_t *T)
{
	const uint64_t s0 = A.win_off[S.ol]; const int32_t nw = (int32_t)(A.win_off[S.ol + 1] - s0); const uint32_t w0 = z.x_pos_s / A.wl, tl = A.len[z.y_id];
	for (;;) {
		if (S.phase == HAO_RS_DONE) return false;
		if (S.phase == HAO_RS_SEEK) {
			int32_t k = S.k + 1;
			while (k < nw && A.werr[s0 + k] == 0xff) ++k;
			if (k >= nw) { S.phase = HAO_RS_DONE; return false; }
			const int32_t prev_ye = S.a_ye;
			S.k = k; S.aflags = 0;
			hao_ref_pair(z, w0 + k, A.wl, A.shift[s0 + k], A.tab, tl, T);      // (true: the pair aligned)
			S.a_ys = (int32_t)T->p_pos; S.a_ye = (int32_t)T->p_pos + (int32_t)A.wpe[s0 + k]; S.a_err = A.werr[s0 + k];
			if (S.last >= 0) { S.j = S.last + 1; S.toff = (int64_t)prev_ye + 1; S.phase = HAO_RS_FWD_CHECK; }
			else { S.cs = 0; S.phase = HAO_RS_BWD_START; }
		} else if (S.phase == HAO_RS_FWD_CHECK) {
			if (S.j < S.k && S.toff < (int64_t)tl && hao_rescue_pair(z, w0 + S.j, A.wl, S.toff, A.tab, tl, T)) { S.phase = HAO_RS_FWD; return true; }
			S.cs = S.last + 1; S.phase = HAO_RS_BWD_START;
		} else if (S.phase == HAO_RS_BWD_START) {
			if (S.k > S.cs) {
				hao_ref_pair(z, w0 + S.k, A.wl, A.shift[s0 + S.k], A.tab, tl, T);
				if (S.a_err == 0) {      // the traced function's shortcut: ps = pe - (te - ts), no sweep
					S.a_ys = S.a_ye - ((int32_t)T->t_len - 1); S.aflags |= HAO_RS_A_TRACED;
					S.toff = (int64_t)S.a_ys - 1; S.j = S.k - 1; S.phase = HAO_RS_BWD_CHECK;
				} else if (!hao_tg_semi_domain(*T)) { S.aflags |= HAO_RS_A_UNTRACED; S.phase = HAO_RS_PUSH; }
				else { S.phase = HAO_RS_ANCHOR; return true; }
			} else S.phase = HAO_RS_PUSH;
		} else if (S.phase == HAO_RS_BWD_CHECK) {
			bool go = false;
			if (S.j >= S.cs) {
				int64_t qs, ql; hao_ref_window(z, w0 + S.j, A.wl, &qs, &ql);
				const int64_t ys = S.toff + 1 - ql;
				if (ys >= 0 && hao_rescue_pair(z, w0 + S.j, A.wl, ys, A.tab, tl, T)) { if (hao_tg_semi_domain(*T)) go = true; else S.aflags |= HAO_RS_A_UNTRACED; }
			}
			if (go) { S.phase = HAO_RS_BWD; return true; }
			S.phase = HAO_RS_PUSH;
		} else if (S.phase == HAO_RS_PUSH) {
			if (S.aflags) {
				hao_rs_win r; r.y_start = S.a_ys; r.y_end = S.a_ye; r.win = w0 + (uint32_t)S.k;
				r.info = (uint32_t)S.a_err | (2u << 16) |((S.aflags & HAO_RS_A_REPLACED) ? (1u << 18) : 0u) | ((S.aflags & HAO_RS_A_UNTRACED) ? HAO_RS_UNTRACED_BIT : 0u) | HAO_RS_VALID;
				int64_t qs, ql; hao_ref_window(z, r.win, A.wl, &qs, &ql); r.info |= (uint32_t)A.tab[ql] << 8;
				rec[S.k] = r;
			}
			S.last = S.k; S.phase = HAO_RS_SEEK;
		} else return true;      // (FWD / ANCHOR / BWD: the task is rebuilt by the caller)
	}
}
// the task a waiting state stands for
__device__ __forceinline__ void hao_rs_task(const hao_rs_args &A, const hao_ovlp_t &z, const hao_rs_state &S, hao_ed_task_t *T)
{
	const uint64_t s0 = A.win_off[S.ol]; const uint32_t w0 = z.x_pos_s / A.wl, tl = A.len[z.y_id];
	if (S.phase == HAO_RS_FWD) hao_rescue_pair(z, w0 + S.j, A.wl, S.toff, A.tab, tl, T);
	else if (S.phase == HAO_RS_ANCHOR) hao_ref_pair(z, w0 + S.k, A.wl, A.shift[s0 + S.k], A.tab, tl, T);
	else { int64_t qs, ql; hao_ref_window(z, w0 + S.j, A.wl, &qs, &ql); hao_rescue_pair(z, w0 + S.j, A.wl, S.toff + 1 - ql, A.tab, tl, T); }
}

// One round: lane = state lo + slot of the launch; path = the column scratch (three words per text column, `stride` lanes per row); *left += the lanes whose
// overlap still waits for an alignment after this round
__global__ __launch_bounds__(256) void hao_rs_round_kernel(hao_ed_reads R, hao_rs_args A, hao_rs_state *st, uint64_t m, hao_rs_win *rec, uint64_t *path, uint64_t stride, unsigned long long *left)
{
	__shared__ uint8_t s_text[4][HAO_AL_CH];
	const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint64_t slot = ((uint64_t)blockIdx.x * 4 + wv) * 64 + lane;
	hao_ed_task_t T; T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	hao_rs_state S; S.phase = HAO_RS_DONE; S.ol = 0; S.base = 0;
	hao_ovlp_t z; bool mine = false;
	if (slot < m) {
		S = st[slot];
		if (S.phase != HAO_RS_DONE) { z = A.ol[S.ol]; mine = hao_rs_advance(A, z, S, rec + S.base, &T); if (mine) hao_rs_task(A, z, S, &T); }
	}
	// (a lane without a task must not look like its neighbour's text: the sweep starts a text segment where a lane's text differs from its left neighbour's)
	if (!mine) T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0;
	uint64_t *col = path + slot;
	hao_al_state<uint64_t> W;
	// One sweep for all three kinds of step.  A forward (distance-only) lane is swept in HAO_AL_SEMI form and finished as HAO_AL_ED: hao_al_init and hao_al_column
	// are the same code for the two modes but for SEMI's refusal of p_len <= 0, and a task of hao_rescue_pair has p_len >= 1 (init_waln leaves min(l, ql + thre)
	// bases at least); the columns such a lane keeps are not read.  If the two modes ever part in init or column code, forward lanes need a sweep of their own.
	hao_al_tile_sweep<uint64_t, HAO_AL_SEMI, true, 3>(R, T, mine, W, s_text[wv], lane, col, stride);
	hao_trace_result_t res; res.err = HAO_AL_NONE; res.ps = -1; res.pe = -1; res.n_cigar = 0;
	bool need2 = false; hao_ed_task_t T2 = T;
	const int64_t tl = mine ? (int64_t)A.len[z.y_id] : 0;
	if (mine) {
		if (S.phase == HAO_RS_FWD) { hao_al_finish<uint64_t, HAO_AL_ED, false, 3>(W, T, res, col, stride, nullptr, 0u); res.ps = 0; }
		else {
			hao_al_finish<uint64_t, HAO_AL_SEMI, true, 3>(W, T, res, col, stride, nullptr, 0u);
			// recal_boundary_exz's condition and its new placement
			if (res.err != HAO_AL_NONE && res.err > 0 && (res.pe + 1 == (int32_t)T.p_len || res.ps == 0)) {
				const int64_t ql = T.t_len, ts = res.ps == 0 ? (int64_t)T.p_pos : (int64_t)T.p_pos + res.pe - ql + 1;
				int64_t rs, rl, ab;
				if (hao_rs_init_waln(T.thre, ts, tl, ql + 2 * (int64_t)T.thre, &rs, &rl, &ab) && !(rs == (int64_t)T.p_pos && rl == (int64_t)T.p_len)) {
					T2.p_pos = (uint32_t)rs; T2.p_len = (uint32_t)rl; T2.abs_diag = (uint32_t)ab;
					if (hao_tg_semi_domain(T2)) need2 = true; else S.aflags |= HAO_RS_A_UNTRACED;
				}
			}
		}
	}
	uint32_t replaced = 0;
	if (!need2) T2.p_rid = T2.p_pos = T2.p_len = T2.p_rev = T2.t_rid = T2.t_pos = T2.t_len = T2.t_rev = T2.thre = T2.abs_diag = 0;
	if (__ballot(need2)) {      // (wave-uniform: the retry is rare)
		hao_al_state<uint64_t> W2;
		hao_al_tile_sweep<uint64_t, HAO_AL_SEMI, true, 3>(R, T2, need2, W2, s_text[wv], lane, col, stride);
		if (need2) {
			hao_trace_result_t r2; r2.err = HAO_AL_NONE; r2.ps = -1; r2.pe = -1; r2.n_cigar = 0;
			hao_al_finish<uint64_t, HAO_AL_SEMI, true, 3>(W2, T2, r2, col, stride, nullptr, 0u);
			if (r2.err != HAO_AL_NONE && r2.err < res.err) { res = r2; T = T2; replaced = 1; }
		}
	}
	if (mine) {
		const bool ok = res.err != HAO_AL_NONE; const uint32_t w0 = z.x_pos_s / A.wl; const int32_t rs = (int32_t)T.p_pos;
		if (S.phase == HAO_RS_FWD) {
			if (ok) {
				hao_rs_win r; r.y_start = rs; r.y_end = rs + res.pe; r.win = w0 + (uint32_t)S.j; r.info = (uint32_t)res.err | T.thre << 8 | HAO_RS_VALID;
				rec[S.base + S.j] = r;
				S.last = S.j; S.toff = (int64_t)r.y_end + 1; ++S.j; S.phase = HAO_RS_FWD_CHECK;
			} else { S.cs = S.last + 1; S.phase = HAO_RS_BWD_START; }
		} else if (S.phase == HAO_RS_ANCHOR) {
			if (ok) { S.a_ys = rs + res.ps; S.a_ye = rs + res.pe; S.a_err = res.err; S.aflags |= HAO_RS_A_TRACED | (replaced ? HAO_RS_A_REPLACED : 0); }
			S.toff = (int64_t)S.a_ys - 1; S.j = S.k - 1; S.phase = HAO_RS_BWD_CHECK;
		} else {
			if (ok) {
				hao_rs_win r; r.y_start = rs + res.ps; r.y_end = rs + res.pe; r.win = w0 + (uint32_t)S.j; r.info = (uint32_t)res.err | T.thre << 8 | (1u << 16) | (replaced << 18) | HAO_RS_VALID;
				rec[S.base + S.j] = r;
				S.toff = (int64_t)r.y_start - 1; --S.j; S.phase = HAO_RS_BWD_CHECK;
			} else S.phase = HAO_RS_PUSH;
		}
		hao_ed_task_t Tn;
		mine = hao_rs_advance(A, z, S, rec + S.base, &Tn);
		st[slot] = S;
	}
	const unsigned long long waiting = __ballot(mine);
	if (lane == 0 && waiting) atomicAdd(left, (unsigned long long)__popcll(waiting));
}

// a thread per overlap: align_hc_ed_post_extz's running align_length over the overlap's slots with the rescued windows of the gap before each aligned
// window, the exit test after each, the final verdict; records beyond the exit window are dropped.  *total += rescued windows kept
__global__ __launch_bounds__(256) void hao_rs_verdict_kernel(hao_rs_args A, const uint64_t *rbase, hao_rs_win *rec, hao_rs_ovlp *out, unsigned long long *total)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n_ol) return;
	const hao_ovlp_t z = A.ol[i];
	const uint64_t s0 = A.win_off[i], rb = rbase[i]; const uint32_t nw = (uint32_t)(A.win_off[i + 1] - s0), w0 = z.x_pos_s / A.wl;
	const int64_t ovl = (int64_t)z.x_pos_e + 1 - (int64_t)z.x_pos_s;
	hao_rs_win *rw = rb == UINT64_MAX ? nullptr : rec + rb;
	hao_rs_ovlp o; o.verdict = 0; o.flags = 0; o.exit_win = 0xffffffffu; o.n_rescued = 0;
	int64_t al = 0; uint32_t g = 0, k = 0; bool exited = false;
	for (; k < nw; ++k) {
		if (A.werr[s0 + k] == 0xff) continue;
		if (rw) {
			for (; g < k; ++g) if ((rw[g].info & HAO_RS_VALID) && ((rw[g].info >> 16) & 3u) < 2u) { int64_t qs, ql; hao_ref_window(z, w0 + g, A.wl, &qs, &ql); al += ql; ++o.n_rescued; }
			if (rw[k].info & HAO_RS_UNTRACED_BIT) o.flags |= 1u;
		}
		g = k + 1;
		int64_t qs, ql; hao_ref_window(z, w0 + k, A.wl, &qs, &ql);
		al += ql;
		const int64_t aln = ovl - ((qs + ql - (int64_t)z.x_pos_s) - al);
		if (!(aln > 0 && (double)ovl * 0.9 <= (double)aln)) { o.exit_win = w0 + k; exited = true; break; }
	}
	if (exited && rw) for (uint32_t q = k + 1; q < nw; ++q) rw[q].info = 0;
	o.align_length = (uint32_t)al;
	o.verdict = (!exited && al > 0 && (double)ovl * 0.9 <= (double)al) ? 1 : 0;
	out[i] = o;
	if (o.n_rescued) atomicAdd(total, (unsigned long long)o.n_rescued);
}

// The delivery path's compact form of the records (HAO_DELIVER_RESCUE): cnt[i] = records overlap i keeps (after the verdict kernel; cnt[n_ol] = 0 for the scan),
// then, with off = their exclusive scan, the records themselves in window order with the device-only bits stripped - what hao_fetch_rescue builds on the host
__global__ void hao_rs_count_kernel(uint64_t n_ol, const uint64_t *win_off, const uint64_t *rbase, const hao_rs_win *rec, uint64_t *cnt)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n_ol) return;
	uint64_t k = 0;
	if (i < n_ol && rbase[i] != UINT64_MAX) { const hao_rs_win *rw = rec + rbase[i]; for (uint64_t w = 0, nw = win_off[i + 1] - win_off[i]; w < nw; ++w) k += (rw[w].info & HAO_RS_VALID) != 0; }
	cnt[i] = k;
}
__global__ void hao_rs_compact_kernel(uint64_t n_ol, const uint64_t *win_off, const uint64_t *rbase, const hao_rs_win *rec, const uint64_t *off, hao_rs_win *out)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_ol || rbase[i] == UINT64_MAX) return;
	const hao_rs_win *rw = rec + rbase[i]; uint64_t at = off[i];
	for (uint64_t w = 0, nw = win_off[i + 1] - win_off[i]; w < nw && at < off[i + 1]; ++w)
		if (rw[w].info & HAO_RS_VALID) { hao_rs_win r = rw[w]; r.info &= ~(HAO_RS_VALID | HAO_RS_UNTRACED_BIT); out[at++] = r; }
}
