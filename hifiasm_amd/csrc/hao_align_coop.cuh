// Window alignment beyond 127 errors: the reference's ed_band_cal_*_infi_* functions (Levenshtein_distance.h:2134-3100) as cal_exz_infi calls them
// (Correct.cpp:14508-14565) from hc_aln_exz / hc_aln_exz_adv, with nword = ceil((2 thre + 1) / 64) up to 64 (thre <= MAX_SIN_E = 2047, patterns to MAX_SIN_L = 10000).
//
// hao_align.cuh keeps a pair's band in ONE lane's registers (nine vectors of up to four words); at 64 words that would be 9 x 64 words per lane.  Here a pair is owned
// by a SEGMENT of S = 8 / 16 / 32 / 64 lanes of a wave (the smallest of them >= nword; a wave carries 64 / S pairs) and lane j of the segment holds WORD j of eq[0..3],
// VP, VN, HP, HN and D0 - a hao_al_state<uint64_t> whose scalars every lane of the segment keeps in step.  Lanes j >= nword hold zeros.  The band is exactly the
// reference's nword words (hao_align.cuh: the word count is part of the semantics): what enters at the top of word nword - 1 is zero, not word nword's bit.
//
// Per text column (hao_al_column's recurrence, word by word):
//   * VP + (X & VP) is added word-wise; two ballots say which words overflowed (generate) and which came out all ones (propagate) - never both - and ONE integer addition
//     on the segment's bits of the two masks resolves every carry: carry into word k = bit k of ((g | p) + g) ^ p, because that addition's own carry chain is
//     c[k + 1] = g[k] | (p[k] & c[k]).  The masks are cut to the segment first, so no carry crosses into the neighbour pair.
//   * D0 >> 1 and the four eq >>= 1 need bit 0 of the next lane's word: the five bits travel packed in one DPP move (wave_shl:1); the top word takes zero.
//   * the next pattern character is or-ed in by the lane that owns bit 2 thre (always word nword - 1), which alone advances the segment's pattern stream.
//   * the running error reads bit 0 of word 0 (a third ballot); the extension modes' row error reads one bit of HP / HN from its owner lane (one ds_bpermute), its
//     first value is a masked popcount summed over the segment (log2 S shuffles, once per pair).
// Every cross-lane operation stands in wave-uniform control flow: all lanes walk the columns of the wave's longest text and a segment that has finished or died simply
// does not commit (`run`).
// The text is staged as in hao_al_tile_sweep: the wave's HAO_AL_CH bytes of LDS cut into one strip per segment, filled by the segment's own lanes.  After the last
// column the segment spills VP / VN into the same LDS bytes and its first lane runs hao_al_finish itself - scans, tie rules and the traceback (hao_al_walk_back) -
// over a run-time-width view of those words (hao_al_dynw): at most 4095 sequential steps once per pair against thousands of columns, and no second statement of a rule.
// Traced sweeps keep hao_al_keep3's three-word columns as [pair][column][vector][word]: a segment's stores are contiguous, 24 nword bytes per column.
//
// Budget (gfx950): the state is 9 words = 18 VGPRs, the pattern stream ~20, the task 10, scalars and temporaries ~40: under 128 VGPRs, i.e. 4 waves per SIMD = the
// 16 waves per CU a 256-thread block layout gives with 4 blocks; LDS 1 KiB per wave (4 KiB per block: no limit).  The column is a dependent chain
// ballot -> scalar add -> vector add, so the kernel is latency-bound and lives on those co-resident waves, not on issue rate.
#pragma once
#include "hao_align.cuh"

// an n-word band vector in memory seen through a right shift - all hao_al_finish asks of a band type: copy, >>, >>=, & with 1, and the low bits as an integer
struct hao_al_dynw {
	const uint64_t *w; int32_t n, sh; uint64_t lit;      // w: the words (nullptr: the literal lit)
	__device__ __forceinline__ hao_al_dynw() : w(nullptr), n(0), sh(0), lit(0) {}
	__device__ __forceinline__ hao_al_dynw(int v) : w(nullptr), n(0), sh(0), lit((uint64_t)(int64_t)v) {}
	__device__ __forceinline__ hao_al_dynw(const uint64_t *w_, int32_t n_) : w(w_), n(n_), sh(0), lit(0) {}
	__device__ __forceinline__ uint64_t low() const { if (!w) return lit; const int32_t k = sh >> 6; return k < n ? w[k] >> (sh & 63) : 0; }      // (bit 0 is all that is read)
	__device__ __forceinline__ hao_al_dynw operator&(const hao_al_dynw &o) const { return hao_al_dynw((int)(low() & o.low() & 1)); }
	__device__ __forceinline__ hao_al_dynw operator>>(int s) const { hao_al_dynw r = *this; r.sh += s; return r; }
	__device__ __forceinline__ hao_al_dynw &operator>>=(int s) { sh += s; return *this; }
	__device__ __forceinline__ explicit operator int32_t() const { return (int32_t)low(); }
};
template<> struct hao_al_words<hao_al_dynw> { static __device__ __forceinline__ int of(int32_t thre) { return (int)hao_al_nword((uint32_t)thre); } };

// lanes of the segment that owns a band of nword words, as a power of two's exponent (3 .. 6)
__host__ __device__ __forceinline__ int hao_alc_lg(uint32_t nword) { return nword <= 8 ? 3 : nword <= 16 ? 4 : nword <= 32 ? 5 : 6; }
// word j of the integer whose low l bits are set
__device__ __forceinline__ uint64_t hao_alc_low_word(int32_t l, int j) { const int32_t r = l - 64 * j; return r >= 64 ? ~0ULL : r <= 0 ? 0ULL : (1ULL << r) - 1; }
// 64-bit words of column scratch of a traced pair: slot 0 and one slot per text column, rounded to a cache line so that no two pairs share one
__host__ __device__ __forceinline__ uint64_t hao_alc_path_words(uint32_t thre, uint32_t t_len) { return (3 * (uint64_t)hao_al_nword(thre) * ((uint64_t)t_len + 1) + 15) & ~15ULL; }

// One launch serves the pairs of one segment size (lg = log2 S): order[] = their task indices by text, 64 >> lg of them per wave.  TRACE launches run over the selected
// pairs of a slice and keep their columns at path + poff[slot].
template<int MODE, bool TRACE>
__global__ __launch_bounds__(256) void hao_alc_kernel(hao_ed_reads R, const hao_ed_task_t *task, const uint32_t *order, uint64_t n_order, int lg, uint64_t *path, const uint64_t *poff,
		hao_ed_result_t *out_ed, hao_trace_result_t *out_tr, uint8_t *want_trace, uint16_t *cig, uint32_t cap)
{
	__shared__ uint64_t s_buf[4][HAO_AL_CH / 8];      // per wave: the staged text, then the spilled VP / VN (64 + 64 words)
	constexpr bool ext = MODE == HAO_AL_EXT_FWD || MODE == HAO_AL_EXT_BWD;
	const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int SL = 1 << lg, seg = lane >> lg, j = lane & (SL - 1), base = seg << lg, nseg = 64 >> lg;
	const uint64_t segmask = SL == 64 ? ~0ULL : (1ULL << SL) - 1;
	const uint64_t slot = ((uint64_t)blockIdx.x * 4 + wv) * nseg + seg;
	const bool have = slot < n_order;
	const uint32_t ti = have ? order[slot] : 0;
	hao_ed_task_t T; if (have) T = task[ti]; else { T.p_rid = T.p_pos = T.p_len = T.p_rev = T.t_rid = T.t_pos = T.t_len = T.t_rev = T.thre = T.abs_diag = 0; }
	const int nw = have ? (int)hao_al_nword(T.thre) : 0;
	const bool act = j < nw;
	const uint64_t actm = act ? ~0ULL : 0ULL;
	uint64_t *col = TRACE && have ? path + poff[slot] + j : nullptr;      // (word j of a vector; hao_al_keep3 with stride nw: [column][vector][word])
	uint8_t *codes = (uint8_t*)s_buf[wv];

	// ---- set-up: hao_al_init, the vectors word by word ----
	hao_al_state<uint64_t> S;
	int32_t first = 0, bd = 0;
	S.alive = 0; S.dead = 0; S.tn = 0; S.pn = 0; S.thre = 0;
	S.eq[0] = 0; S.eq[1] = 0; S.eq[2] = 0; S.eq[3] = 0; S.VP = 0; S.VN = 0; S.HP = 0; S.HN = 0; S.D0 = 0; S.top = 0;
	if (have && hao_al_init_head<uint64_t, MODE>(S, T, first, bd)) {
		const int32_t thre = S.thre;
		const hao_al_walk pw = hao_al_walk_of(R, T.p_rid, T.p_pos, T.p_len, T.p_rev, MODE == HAO_AL_EXT_BWD);
		if (MODE == HAO_AL_SEMI || MODE == HAO_AL_ED) S.VN = (nw == 2 && S.adiag == 64) ? 0ULL : hao_alc_low_word(S.adiag, j);      // (two words, abs_diag 64: hao_al_lsub's VN = 0)
		else { S.VN = hao_alc_low_word(thre, j); S.VP = hao_alc_low_word((thre << 1) + 1, j) ^ S.VN; }
		S.VN &= actm; S.VP &= actm;
		// the pattern characters that enter before the first column: character q sits at band bit first + q, so this lane's are q in [64 j - first, 64 j + 64 - first)
		int32_t q0 = 64 * j - first, q1 = q0 + 64; if (q0 < 0) q0 = 0; if (q1 > bd) q1 = bd;
		if (act && q0 < q1) {
			hao_al_walk w2 = pw; w2.f0 += (int64_t)w2.dir * q0;
			hao_al_pstream_init(S.ps, w2);
			uint64_t mm = 1ULL << ((first + q0) & 63);
			for (int32_t q = q0; q < q1; ++q) { hao_al_eq_or(S, hao_al_pstream_next(S.ps), mm); mm <<= 1; }
		}
		if (j == nw - 1) {      // the owner of bit 2 thre streams the rest of the pattern
			hao_al_walk w2 = pw; w2.f0 += (int64_t)w2.dir * bd;
			hao_al_pstream_init(S.ps, w2);
			S.top = 1ULL << ((thre << 1) & 63);
		}
		S.alive = 1;
		if (TRACE && act) hao_al_keep3(S.D0, S.VP, S.VN, col, (uint64_t)nw, 0);      // (slot 0: the vectors the first column starts from)
	}

	// ---- the sweep ----
	const int32_t chs = (int32_t)(HAO_AL_CH >> (6 - lg));
	uint8_t *strip = codes + seg * chs;
	const hao_al_walk tw = hao_al_walk_of(R, T.t_rid, T.t_pos, T.t_len, T.t_rev, MODE == HAO_AL_EXT_BWD);
	int32_t tn_mx = S.alive ? S.tn : 0;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) { const int32_t o_ = __shfl_xor(tn_mx, d); tn_mx = o_ > tn_mx ? o_ : tn_mx; }
	tn_mx = __builtin_amdgcn_readfirstlane(tn_mx);
	for (int32_t k0 = 0; k0 < tn_mx; k0 += chs) {
		if (!__any(S.alive && !S.dead && S.tn > k0)) break;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");      // (the previous range has been read)
		const int32_t n = S.alive && !S.dead && S.tn > k0 ? (S.tn - k0 < chs ? S.tn - k0 : chs) : 0;      // (S.tn <= t_len)
		hao_al_stage_bases(tw, k0, n, strip, j, SL);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		if (R.nsite_off) {      // N sites (after the bases are in place)
			hao_al_stage_nsites(tw, k0, n, strip, j, SL);
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		}
		const int32_t k1 = k0 + chs < tn_mx ? k0 + chs : tn_mx;
		for (int32_t i = k0; i < k1; ++i) {
			const bool run = S.alive && !S.dead && i < S.tn, last = i == S.tn - 1;
			const uint32_t tc = run ? strip[i - k0] : 4u;
			// Myers' column on word j
			const uint64_t X = hao_al_eq_of(S, tc) | S.VN, A = X & S.VP;
			uint64_t sum = S.VP + A;
			const unsigned long long G = __ballot(sum < A), P = __ballot(sum == ~0ULL);
			const uint64_t gs = (G >> base) & segmask, ps = (P >> base) & segmask;
			sum += ((((gs | ps) + gs) ^ ps) >> j) & 1ULL & actm;
			const uint64_t D0 = (sum ^ S.VP) | X, HN = S.VP & D0, HP = (S.VN | ~(S.VP | D0)) & actm;
			uint32_t nb = hao_wave_shl1((uint32_t)(D0 & 1) | (uint32_t)(S.eq[0] & 1) << 1 | (uint32_t)(S.eq[1] & 1) << 2 | (uint32_t)(S.eq[2] & 1) << 3 | (uint32_t)(S.eq[3] & 1) << 4, 0u);
			if (j >= nw - 1) nb = 0;      // (the top word takes a zero; the segment's last lane would otherwise read the neighbour pair)
			const uint64_t Xs = D0 >> 1 | (uint64_t)(nb & 1) << 63;
			const uint64_t VN = Xs & HP, VP = (HN | ~(Xs | HP)) & actm;
			const int32_t d0 = (int32_t)((__ballot((int)(D0 & 1)) >> base) & 1ULL);
			const int32_t err = S.err + (d0 ^ 1);
			const bool go = run && err <= S.cut;
			int32_t hb = 0, first_sum = 0;
			const int32_t kk = i + S.thre - (S.pn - 1);      // >= 0: the band has reached the pattern's last row
			if (ext) {
				const int32_t k2 = (S.thre << 1) - kk;      // the row's band bit in this column
				hb = (int32_t)((HP >> (k2 & 63)) & 1ULL) | (int32_t)((HN >> (k2 & 63)) & 1ULL) << 1;
				hb = __shfl(hb, base + ((k2 >> 6) & (SL - 1)));
				if (__any(go && !last && kk >= 0 && S.tmp_e == HAO_AL_NONE)) {      // the row's error from the running one: VP / VN bits [0, pn - 1 - (i - thre)) of the new column
					first_sum = __popcll(VP & hao_alc_low_word(k2, j)) - __popcll(VN & hao_alc_low_word(k2, j));
					for (int d = 1; d < SL; d <<= 1) first_sum += __shfl_xor(first_sum, d);
				}
			}
			if (run) {
				S.D0 = D0; S.HN = HN; S.HP = HP; S.VN = VN; S.VP = VP; S.err = err;
				if (!go) S.dead = 1;
				else {
					if (ext && !last && kk >= 0) {
						const int32_t k2 = (S.thre << 1) - kk;
						if (S.tmp_e == HAO_AL_NONE) S.tmp_e = S.err + first_sum;
						else if (k2 >= 0) S.tmp_e += (hb & 1) - (hb >> 1 & 1);
						if (S.tmp_e <= S.thre && S.tmp_e < S.best) { S.best = S.tmp_e; S.a_p = S.pn - 1; S.a_t = i; }
					}
					if (!last) {
						S.eq[0] = S.eq[0] >> 1 | (uint64_t)(nb >> 1 & 1) << 63; S.eq[1] = S.eq[1] >> 1 | (uint64_t)(nb >> 2 & 1) << 63;
						S.eq[2] = S.eq[2] >> 1 | (uint64_t)(nb >> 3 & 1) << 63; S.eq[3] = S.eq[3] >> 1 | (uint64_t)(nb >> 4 & 1) << 63;
					}
					if (TRACE && act) hao_al_keep3(S.D0, S.VP, S.VN, col, (uint64_t)nw, i + 1);
					if (!last) {
						++S.i_bd;
						if (S.i_bd < S.pn && j == nw - 1) hao_al_eq_or(S, hao_al_pstream_next(S.ps), S.top);
					}
				}
			}
		}
	}

	// ---- finish: VP / VN to LDS, then hao_al_finish on the segment's first lane ----
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");      // (the last strip has been read)
	s_buf[wv][lane] = S.VP; s_buf[wv][64 + lane] = S.VN;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // (and the kept columns, which the first lane reads, are visible to it)
	if (have && j == 0) {
		hao_al_state<hao_al_dynw> F;
		F.pn = S.pn; F.tn = S.tn; F.thre = S.thre; F.adiag = S.adiag; F.cut = S.cut; F.err = S.err; F.i_bd = S.i_bd; F.best = S.best; F.a_p = S.a_p; F.a_t = S.a_t; F.tmp_e = S.tmp_e;
		F.alive = S.alive; F.dead = S.dead;
		F.VP = hao_al_dynw(&s_buf[wv][base], nw); F.VN = hao_al_dynw(&s_buf[wv][64 + base], nw);
		hao_trace_result_t res;
		const bool tr = hao_al_finish<hao_al_dynw, MODE, TRACE, 3>(F, T, res, col, 1, TRACE ? cig + (uint64_t)ti * cap : nullptr, cap);
		if (MODE == HAO_AL_ED) { hao_ed_result_t r2; r2.err = res.err; r2.pe = res.pe; out_ed[ti] = r2; }
		else { out_tr[ti] = res; if (!TRACE) want_trace[ti] = tr ? 1 : 0; }
	}
}
