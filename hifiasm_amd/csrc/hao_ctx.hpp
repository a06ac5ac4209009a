// Engine context: device buffers, stream, stage timers (host side of libhao.so).
#pragma once
#include <time.h>
#include <rocprim/rocprim.hpp>
#include <map>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "hao_common.cuh"
#include "hao_grid_pair.cuh"      // (hao_ed_pair)

struct hao_ctx;
static void hao_set_err(hao_ctx *c, const std::string &m);

// grow-only device buffer that owns its memory: freed when it goes out of scope (or with its context), movable, not copyable
template<typename T> struct DevBuf {
	T *p = nullptr; size_t cap = 0; bool borrowed = false;      // borrowed: a read-only view of another engine's buffer (hao_attach) - never freed or grown here
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete; DevBuf &operator=(const DevBuf&) = delete;
	DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), borrowed(o.borrowed) { o.p = nullptr; o.cap = 0; o.borrowed = false; }
	DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; borrowed = o.borrowed; o.p = nullptr; o.cap = 0; o.borrowed = false; } return *this; }
	~DevBuf() { release(); }
	hipError_t reserve(size_t n) {
		if (n <= cap) return hipSuccess;
		if (borrowed) return hipErrorInvalidValue;
		if (p) (void)hipFree(p);
		p = nullptr; cap = 0;
		size_t want = n + n / 8 + 64;
		hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
		if (e == hipSuccess) cap = want;
		return e;
	}
	// allocate exactly n elements if smaller (twin of a ping-pong pair: avoids a late first allocation inside a timed pass)
	hipError_t reserve_exact(size_t n) {
		if (n <= cap) return hipSuccess;
		if (borrowed) return hipErrorInvalidValue;
		if (p) (void)hipFree(p);
		p = nullptr; cap = 0;
		hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
		if (e == hipSuccess) cap = n;
		return e;
	}
	void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; cap = 0; borrowed = false; }
	void borrow(const DevBuf<T> &o) { release(); p = o.p; cap = o.cap; borrowed = o.p != nullptr; }
};

inline bool hao_dbg_sync = false;      // HAO_DBG_PRINT=sync (hao_switches::load): wait after every stage and say its name - localises a device fault
struct StageTimer {
	std::vector<std::string> names; std::vector<hipEvent_t> ev; std::vector<double> host_t; hipStream_t st = nullptr;
	static double now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
	void begin(hipStream_t s) { st = s; names.clear(); host_t.clear(); mark("__begin"); }
	void mark(const char *name) {
		size_t i = names.size();
		if (i >= ev.size()) { hipEvent_t e; (void)hipEventCreate(&e); ev.push_back(e); }
		names.push_back(name); host_t.push_back(now()); (void)hipEventRecord(ev[i], st);
		if (hao_dbg_sync) { const hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[stage] %s: %s\n", name, hipGetErrorString(e)); fflush(stderr); }
	}
	// after stream sync: ms between consecutive marks, labelled by the later mark
	void collect(std::vector<std::pair<std::string, float> > &out) {
		out.clear();
		for (size_t i = 1; i < names.size(); ++i) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]); out.push_back(std::make_pair(names[i], ms)); }
		// the HOST's wall clock between the same marks for ha_ft_gen's stages ("host_ft_..."): its wall time is allocation, scratch and per-read host loops, not kernels
		for (size_t i = 1; i < names.size(); ++i) if (names[i].compare(0, 3, "ft_") == 0) out.push_back(std::make_pair("host_" + names[i], (float)((host_t[i] - host_t[i - 1]) * 1e3)));
	}
	~StageTimer() { for (auto e : ev) (void)hipEventDestroy(e); }
};

// run-time switches: read from the environment ONCE, in hao_create.  Eight variables:
//   HAO_SEED_LDS, HAO_SEED_LDS_RATIO, HAO_SEED_MERGE_MAXN   which reads / batches the list-major seed kernel takes (below)
//   HAO_FT_PASSES                                           ha_ft_gen's hash-range passes (0: what the free device memory asks for)
//   HAO_ARENA_NUMA                                          placement of the pinned delivery arenas
//   HAO_DBG_PRINT=seed,qc,dp,sel,dl,bloom,sync              timers / counters on stderr (sync: wait after every stage and say its name - localises a device fault)
//   HAO_DBG_FORCE=seq_chain,dp_seqtail,dp_nospec,dp_serial,seq_prune,noql,al_coop      send every read / group down one of the engine's FALLBACK paths (tests: each has to give the default path's bytes)
//   HAO_DBG_TEST=ix_pad=N,sort40_min=N,sk_gcap=N,exc_cap=N,fc_raw_every=N,exc_every=N,qmz_raw=1,arena_probe=1,ft_chunk_slots=N,gather_chunk=N,al_slice=N      capacities and thresholds shrunk so that small inputs reach the overflow / big-index code
struct hao_switches {
	bool seedphase = false, qcphase = false, dp_stats = false, selphase = false, dltime = false, bloom = false;                 // HAO_DBG_PRINT
	bool seq_chain = false, dp_seqtail = false, dp_nospec = false, dp_serial = false, seq_prune = false, seed_noql = false, al_coop = false;     // HAO_DBG_FORCE
	long long sk_gcap = -1, exc_cap = -1, ft_chunk_slots = 0; unsigned long long gather_chunk = 64ULL << 20, al_slice = 4ULL << 30, ix_pad = 0, sort40_min = 1ULL << 23; int fc_raw_every = 0, exc_every = 0; bool qmz_raw = false, arena_probe = false;      // HAO_DBG_TEST
	int arena_numa = 3, seed_merge_maxn = 24000, seed_lds_ratio = 120, ft_passes = 0, seed_lds = 1;
	static bool in_list(const char *v, const char *name) {      // name is an element of the comma-separated list v
		const size_t n = strlen(name);
		for (const char *p = v; p && *p; ) { const char *e = strchr(p, ','); const size_t l = e ? (size_t)(e - p) : strlen(p); if (l == n && strncmp(p, name, n) == 0) return true; p = e ? e + 1 : nullptr; }
		return false;
	}
	static bool in_kv(const char *v, const char *name, unsigned long long &out) {      // "name=123" is an element of v
		const size_t n = strlen(name);
		for (const char *p = v; p && *p; ) { const char *e = strchr(p, ','); if (strncmp(p, name, n) == 0 && p[n] == '=') { out = strtoull(p + n + 1, nullptr, 10); return true; } p = e ? e + 1 : nullptr; }
		return false;
	}
	void load() {
		if (const char *v = getenv("HAO_DBG_PRINT")) {
			seedphase = in_list(v, "seed"); qcphase = in_list(v, "qc"); dp_stats = in_list(v, "dp"); selphase = in_list(v, "sel"); dltime = in_list(v, "dl"); bloom = in_list(v, "bloom"); hao_dbg_sync = in_list(v, "sync");
		}
		if (const char *v = getenv("HAO_DBG_FORCE")) {
			seq_chain = in_list(v, "seq_chain");      // every group through the complete sequential chaining routine (one lane per group)
			dp_seqtail = in_list(v, "dp_seqtail");    // groups the quick check rejects: the DP's tail walked sequentially
			dp_nospec = in_list(v, "dp_nospec");      // the DP without speculation
			dp_serial = in_list(v, "dp_serial");      // DP and pack kernels on the engine's stream (no side streams)
			seq_prune = in_list(v, "seq_prune");      // the selection's pruning by one lane
			seed_noql = in_list(v, "noql");           // the seed kernels' generic per-minimizer tables (the path of batches with a read of more than HAO_QTAB_CAP minimizers)
			al_coop = in_list(v, "al_coop");          // hao_window_ed_long / hao_window_trace_long: every pair through the cooperative kernel (hao_align_coop.cuh), bands of one to four words included
		}
		if (const char *v = getenv("HAO_DBG_TEST")) {
			unsigned long long x;
			if (in_kv(v, "ix_pad", x)) ix_pad = x;                        // unused position records in front of the index (list starts beyond 2^32 on a small read set)
			if (in_kv(v, "sort40_min", x)) sort40_min = x;                // the big-index path (40-bit sort + fix-up, gather, windowed scatter) from this many minimizers on (default 2^23: rocprim's bit-range sort, tests/test_gpu_rocprim.py)
			if (in_kv(v, "sk_gcap", x)) sk_gcap = (long long)x;           // capacity of the sketch's minimizer pool (the grow-and-rerun path)
			if (in_kv(v, "exc_cap", x)) exc_cap = (long long)x;           // capacity of the wire format's verbatim-hit list (the grow-and-repack path)
			if (in_kv(v, "fc_raw_every", x)) fc_raw_every = (int)x;       // every n-th overlap's fake cigar travels raw (the fallback of the packed wire form)
			if (in_kv(v, "exc_every", x)) exc_every = (int)x;             // every n-th hit of a chain travels verbatim (the exception list)
			if (in_kv(v, "qmz_raw", x)) qmz_raw = x != 0;                   // the delivered minimizer tables in their 8-byte form whatever the read lengths (the form of batches with a read of 65 536 bases or more)
			if (in_kv(v, "arena_probe", x)) arena_probe = x != 0;           // the delivery arenas' placement probe (hao_arena_ensure) whatever their size and rate
			if (in_kv(v, "ft_chunk_slots", x)) ft_chunk_slots = (long long)x;      // k-mer slots hashed per chunk of reads in ha_ft_gen's pass mode
			if (in_kv(v, "al_slice", x)) al_slice = std::max<unsigned long long>(x, 8);      // bytes of column scratch per slice of every traced sweep (default 4 GB): hao_col_slice's stages - hao_window_trace_batch's second sweep, the traced grid, the rescue rounds, the window lists - cut whole blocks of 256 pairs, so 8 gives them slices of 256; hao_window_trace_long's and the ladder's second sweeps pack per-pair blocks (a few hundred KB walk several slices on a handful of pairs)
			if (in_kv(v, "gather_chunk", x)) gather_chunk = std::max<unsigned long long>(x, 64);      // bytes a rank contributes per exchange of hao_dist_gather_reads (default 64 MB: a few KB walk the multi-chunk path on a small read set)
		}
		if (const char *e = getenv("HAO_SEED_LDS")) seed_lds = atoi(e) ? 1 : 0;      // 0 = the table kernels (hao_query.cuh, hao_query3.cuh) for every read instead of the list-major kernel (hao_query5.cuh): the tests run them on every scenario - they carry repeat-rich batches and the reads the list-major kernel leaves
		if (const char *e = getenv("HAO_SEED_LDS_RATIO")) seed_lds_ratio = std::max(0, atoi(e));      // (per cent) batches with more seed hits per (query minimizer x coverage peak) than this take the table kernels: reads across repeat families (hao_batch.hpp); tests force either side
		if (const char *e = getenv("HAO_SEED_MERGE_MAXN")) seed_merge_maxn = std::max(0, atoi(e));      // reads with more seed hits than this are left to the table kernels by the list-major kernel (repeat families: hundreds of targets per read)
		if (const char *e = getenv("HAO_FT_PASSES")) ft_passes = std::max(0, atoi(e));
		if (const char *e = getenv("HAO_ARENA_NUMA")) arena_numa = atoi(e);      // 0: plain hipHostMalloc, 1: thread policy "prefer the GPU's node", 3 (default): "bind to it", then 1 if that fails - and, when the pages still are elsewhere, mmap + mbind + hipHostRegister; 2: 3 + hipHostMallocNumaUser; 4: always mmap + mbind + hipHostRegister (tests)
	}
};

// A few words the host needs from the device in the middle of a batch (sizes for the next allocation): written by a one-wave kernel into pinned,
// device-mapped host memory instead of a hipMemcpy.  A D2H memcpy - however small - queues on the device-to-host DMA engine, behind the bulk copy of the
// previous batch's results that the delivery path has in flight there: the "asynchronous" delivery would serialise with the compute it should hide under.
static __global__ void hao_peek_kernel(const unsigned long long *src, int n, unsigned long long *dst)
{ if ((int)threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x]; }
// The read-back slots: which words of the 512 (hao_ctx::peek_h / peek_d) each value lands in.  A slot belongs to one reader - hao_peek writes it, hao_ctx::peeked
// reads it after the reader's own synchronise - so a value may stay in its slot across calls without another caller writing over it.
enum hao_peek_id : int {
	PK_ANCHORS, PK_CLS_BASE,                                                  // hao_batch.hpp: the batch's seed hits; the class layout (HAO_NCLS + 1 words)
	PK_N_CHAINS, PK_N_CL, PK_N_FC_RAW, PK_N_OL, PK_N_FC,                      //   the batch's totals: chains, chained hits, raw and final fake-cigar entries, overlaps
	PK_N_EXC, PK_N_CODES, PK_N_FCW, PK_SEED_OVF, PK_ERR, PK_SLOW,             //   verbatim hits, code bytes, raw cigar words, the three seed overflow cursors, c->d_err, the slow statistics (HAO_ST_SLOW .. HAO_ST_CLS_BASE)
	PK_GRID_PAIRS, PK_REF_SLOTS, PK_REF_UNRES,                                //   the window grid: pairs, covered windows, unresolved windows
	PK_SORT40,                                                                // hao_tables.hpp: hao_index_sort's runs listed, scratch used, scratch overflow
	PK_TG_TRACED, PK_TG_CTR, PK_TG_NCIG,                                      // hao_f3.hip, traced grid: selected pairs; (entry bound, untraced pairs); cigar entries
	PK_RS_SIZES, PK_RS_WAITING, PK_RS_TOTAL, PK_RS_NWINS,                     //   rescue: (states, record slots); lanes still waiting after a round; rescued windows; records
	PK_WL_N, PK_WL_PLAN, PK_WL_NCIG, PK_WL_CTR,                               //   window lists: records; (swept records, entry bound, -); cigar entries; the stage's six counters
	PK_LD_SETUP, PK_LD_ROUND, PK_LD_SEL, PK_LD_END,                           //   threshold ladder: (refused requests, open requests); a round's counters (hao_ladder.cuh: HAO_LD_RND ..); selected pairs per (mode, cooperative class); (cigar entries, rows that overran)
	PK_COUNT
};
struct hao_peek_rng { int at, n; };
static constexpr hao_peek_rng HAO_PEEK[PK_COUNT] = {
	/* PK_ANCHORS */ {0, 1}, /* PK_CLS_BASE */ {1, 8},
	/* PK_N_CHAINS */ {9, 1}, /* PK_N_CL */ {10, 1}, /* PK_N_FC_RAW */ {11, 1}, /* PK_N_OL */ {12, 1}, /* PK_N_FC */ {13, 1},
	/* PK_N_EXC */ {14, 1}, /* PK_N_CODES */ {15, 1}, /* PK_N_FCW */ {19, 1}, /* PK_SEED_OVF */ {20, 3}, /* PK_ERR */ {23, 1}, /* PK_SLOW */ {64, 11},
	/* PK_GRID_PAIRS */ {32, 1}, /* PK_REF_SLOTS */ {37, 1}, /* PK_REF_UNRES */ {38, 1},
	/* PK_SORT40 */ {16, 3},
	/* PK_TG_TRACED */ {33, 1}, /* PK_TG_CTR */ {34, 2}, /* PK_TG_NCIG */ {36, 1},
	/* PK_RS_SIZES */ {40, 2}, /* PK_RS_WAITING */ {42, 1}, /* PK_RS_TOTAL */ {43, 1}, /* PK_RS_NWINS */ {44, 1},
	/* PK_WL_N */ {48, 1}, /* PK_WL_PLAN */ {49, 3}, /* PK_WL_NCIG */ {52, 1}, /* PK_WL_CTR */ {53, 6},
	/* PK_LD_SETUP */ {80, 2}, /* PK_LD_ROUND */ {82, 48}, /* PK_LD_SEL */ {130, 16}, /* PK_LD_END */ {146, 2},
};
constexpr int HAO_PEEK_WORDS = 512;
constexpr bool hao_peek_table_ok()
{
	for (int i = 0; i < PK_COUNT; ++i) {
		if (HAO_PEEK[i].at < 0 || HAO_PEEK[i].n < 1 || HAO_PEEK[i].at + HAO_PEEK[i].n > HAO_PEEK_WORDS) return false;
		for (int j = 0; j < i; ++j) if (HAO_PEEK[i].at < HAO_PEEK[j].at + HAO_PEEK[j].n && HAO_PEEK[j].at < HAO_PEEK[i].at + HAO_PEEK[i].n) return false;
	}
	return true;
}
static_assert(hao_peek_table_ok(), "read-back slots: a range beyond the mapped words, or two ranges that overlap");

// What the window-alignment calls have left resident on the current batch.  Every write is a transition, every read a predicate: nothing outside assigns a member.
//   owner, n   whose pairs lie in the shared scratch al_task / al_res: nobody's (a new batch or a host-fed call), hao_window_ed_grid's n, or hao_window_ed_ref's n
//   chain      how far hao_window_ed_ref -> hao_window_rescue_ref -> hao_window_wlist_ref has got; a stage that starts (again) drops itself and the later ones until
//              it completes.  Summaries and rescue results lie in buffers of their own; the rescue stage READS the scratch, and the lists ask for its owner too
//   host       bit s: stage s's fetch call holds host copies of the current results (cleared where the device side is)
//   trace      hao_window_trace_grid's results are resident (buffers of their own)
//   lists      the batch's window records are on the device (wl.woff / wl.wins, buffers of their own that no host-fed call writes: DESIGN.md 4): set when the chain
//              completes, dropped with the batch, by a chain stage that starts (again) and by the grid call - NOT by a host-fed call, so the threshold ladder and
//              hao_window_estimate_err find them call after call (hao_fetch_wlist keeps asking for the scratch's owner as well, as before)
struct WinResident {
	enum Stage { NONE, ED, RESCUE, WLIST };
	void on_new_batch() { *this = WinResident(); }
	void on_host_fed() { owner = NOBODY; n = 0; trace = false; }
	void on_grid(uint64_t pairs) { owner = GRID; n = pairs; lists = false; }
	void on_ref_begin(Stage s) { if (chain >= s) chain = (Stage)(s - 1); host &= (1u << s) - 1; if (s == ED) { owner = NOBODY; n = 0; } lists = false; }
	void on_ref_done(Stage s, uint64_t pairs = 0) { chain = s; if (s == ED) { owner = REF; n = pairs; } if (s == WLIST) lists = true; }
	void on_host_copy(Stage s) { host |= 1u << s; }
	void on_trace_grid(bool done) { trace = done; }
	uint64_t scratch_pairs() const { return owner == NOBODY ? 0 : n; }      // what hao_fetch_ed_grid serves (either grid call's)
	bool ed_resident() const { return chain >= ED; } bool rescue_resident() const { return chain >= RESCUE; } bool trace_resident() const { return trace; }
	bool ref_input_resident() const { return chain >= ED && owner == REF; }      // + hao_window_ed_ref's results per pair in al_res: the rescue stage's input
	bool wlist_input_resident() const { return chain >= RESCUE && owner == REF; }
	bool wlist_resident() const { return chain >= WLIST && owner == REF; }
	bool wlist_records_resident() const { return lists; }      // the records alone: what cal_estimate_err reads (hao_ladder.cuh: hao_ld_estimate_wlist)
	bool host_current(Stage s) const { return (host >> s) & 1u; }
private:
	enum Owner { NOBODY, GRID, REF } owner = NOBODY; uint64_t n = 0; Stage chain = NONE; uint32_t host = 0; bool trace = false, lists = false;
};

// A reference-placed batch whose ED stage has run, as hao_al_rescue and hao_al_wlist (hao_f3.hip) take it: filled from the context's own buffers by the blocking calls, from the
// output set's by the streamed parts (hao_batch.hpp); the CSR of covered windows, the shifts and the error byte per slot are the ED stage's scratch in c->rf on both paths.
struct hao_ref_io {
	const hao_ovlp_t *ol; uint64_t n_ol;                                        // the batch's final ol->list
	uint32_t wl; const uint8_t *tab;                                            // window length, threshold table (on the device)
	const hao_ed_pair *pairs; uint64_t n_pairs, n_slots;                        // the pair list, its length, the covered windows (CSR slots)
	const hao_ed_result_t *res; const uint8_t *err8; const uint16_t *pe16;      // the primary results per pair: res, or (res == NULL) the compact records err8 / pe16
	DevBuf<hao_rs_ovlp> *rs_ovlp; DevBuf<uint64_t> *rs_off; DevBuf<hao_rs_win> *rs_wins;                          // rescue: per-overlap results, record offsets per overlap, the records
	DevBuf<uint64_t> *wl_woff; DevBuf<hao_rs_win> *wl_wins; DevBuf<uint64_t> *wl_cigoff; DevBuf<uint16_t> *wl_cig;      // window lists: record offsets per overlap, the records, entry offsets per record, the entries
};

struct hao_ctx {
	int device = 0; hao_opt_t opt; std::string err; hipStream_t stream = nullptr; hao_switches sw;
	// hao_attach: a second batch context over this engine's reads and index (own stream, scratch, results); index_gen counts the owner's rebuilds
	hao_ctx *owner = nullptr; uint64_t index_gen = 0, attached_gen = 0;
	unsigned long long *peek_h = nullptr, *peek_d = nullptr;      // HAO_PEEK_WORDS words of mapped pinned memory, laid out by HAO_PEEK
	unsigned long long peeked(hao_peek_id slot, int k = 0) const { return peek_h[HAO_PEEK[slot].at + k]; }      // word k of a slot, once the stream that ran hao_peek is synchronised
	// ---- read store (HBM) ----
	uint64_t n_reads = 0, n_bases = 0, n_pk_bytes = 0; bool has_n = false; uint32_t max_len = 0;
	DevBuf<uint8_t> d_packed; DevBuf<uint64_t> d_pk_off; DevBuf<uint32_t> d_len; DevBuf<uint64_t> d_nsite_off; DevBuf<uint32_t> d_nsite;
	std::vector<uint32_t> h_len; std::vector<uint64_t> h_nsite_off;
	// sharded mode: this engine holds reads [rid_base, rid_base + n_reads) of n_total; lengths of ALL reads are replicated
	uint64_t rid_base = 0, n_total = 0; uint32_t max_len_all = 0; int n_cu = 256; DevBuf<uint32_t> d_len_all; std::vector<uint32_t> h_len_all; struct hao_comm *comm = nullptr;
	// the gathered store (hao_dist_gather_reads, hao_gather.hpp): the bases and N sites of ALL n_total reads in global read-id order, on every rank of a sharded
	// engine (with d_len_all it is what hao_reads_view hands the stages beyond the seam); gs_valid: it belongs to the current reads and shard layout
	bool gs_valid = false, gs_has_n = false; uint64_t gs_pk_bytes = 0, gs_nsites = 0;
	DevBuf<uint8_t> g_packed; DevBuf<uint64_t> g_pk_off, g_nsite_off; DevBuf<uint32_t> g_nsite;
	// ---- filter table ----
	bool has_ft = false; int ft_peak_hom = -1, ft_peak_het = -1, ft_cutoff = 0, ft_passes_used = 1; int64_t ft_hist[HAO_N_COUNTS];
	std::vector<uint64_t> h_ft_keys; std::vector<int32_t> h_ft_vals;
	DevBuf<uint64_t> d_ft_keys; DevBuf<int32_t> d_ft_vals; DevBuf<uint32_t> d_ft_bucket;
	DevBuf<uint32_t> d_ft_hbit; DevBuf<unsigned long long> d_ft_hslot; int ft_hbits = 0;      // the filter table's hash view for the device lookups (hao_sketch.cuh: hao_ft_dev)
	int max_n_chain = 100, hom_cov = -1, het_cov = -1;
	// ---- sketch workspace / results ----
	uint64_t sk_lo = 0, sk_n = 0, sk_total = 0; bool sk_is_index = false;
	DevBuf<uint64_t> d_tile_off; DevBuf<uint32_t> d_tile_ord, d_n_runs, d_tot_l; DevBuf<uint64_t> d_chunk_off, d_chunk_cnt64;
	DevBuf<uint8_t> d_scalar_flag; DevBuf<uint32_t> d_scalar_list, d_unit_rid;
	DevBuf<uint64_t> d_pool_x, d_pool_info; DevBuf<uint32_t> d_pool_ord; DevBuf<unsigned long long> d_cursor; DevBuf<int> d_err;
	DevBuf<uint64_t> d_chunk_base, d_chunk_dst; DevBuf<uint32_t> d_chunk_cnt;
	DevBuf<uint64_t> d_g_x, d_g_info; DevBuf<uint32_t> d_g_ord; DevBuf<uint64_t> d_g_off; DevBuf<uint32_t> d_new_n; DevBuf<uint64_t> d_new_n64;
	DevBuf<uint64_t> d_mz_x, d_mz_info, d_mz_off;          // final per-read minimizers of the last sketch_batch
	DevBuf<unsigned char> d_tmp; DevBuf<unsigned char> d_ring; DevBuf<uint32_t> d_ringord, d_cnt_ws;
	std::vector<uint64_t> h_mz_off; std::vector<hao_mz_t> h_mz_fetch;
	// ---- index (pt) ----
	bool has_pt = false; int64_t pt_hist[HAO_N_COUNTS];
	uint64_t ix_n_mz = 0, ix_n_sorted = 0, ix_n_keys = 0, ix_n_pos = 0, ix_pad = 0; int ix_bucket_bits = 16;   // ix_n_mz: local read-ordered records; ix_n_sorted: records in the (replicated) index
	DevBuf<uint64_t> d_ix_mz_x, d_ix_mz_info, d_ix_mz_off;  // all reads' minimizers in read order (query side reuses them)
	DevBuf<uint64_t> d_ix_sx, d_ix_sinfo;                    // sorted by hash (stable)
	DevBuf<uint64_t> d_ix_lk; bool lk_valid = false; DevBuf<uint32_t> w_runid;   // per minimizer (read order): list start | count << 48 of its key (single-device build)
	DevBuf<uint64_t> d_ix_keys, d_ix_start; DevBuf<uint32_t> d_ix_cnt; DevBuf<uint32_t> d_ix_bucket;
	DevBuf<uint64_t> w_ukeys, w_flag, w_kpos, w_ustart; DevBuf<uint32_t> w_ucnt; DevBuf<unsigned long long> w_hist; DevBuf<uint32_t> w_ok, w_ok2, w_oi, w_oi2;   // persistent scratch of the index build
	DevBuf<uint32_t> w_s40_list, w_s40_o; DevBuf<uint64_t> w_s40_x, w_lkv2; DevBuf<unsigned long long> w_s40_cnt; uint64_t s40_runs = 0;      // fix-up of the 40-bit index sort (hao_index.cuh)
	std::vector<uint64_t> h_ix_keys, h_ix_off, h_ix_pos, h_ix_mz_off; bool h_ix_valid = false;
	// ---- query batch ----
	// f3 (hao_align.cuh): scratch of the window-alignment batches, kept between calls (a hipMalloc / hipFree pair per buffer and call cost more than the kernels)
	WinResident win;      // who owns al_task / al_res, and which results of the window-alignment calls are resident
	DevBuf<hao_ed_task_t> al_task; DevBuf<uint64_t> al_k1, al_k2, al_path; DevBuf<uint32_t> al_i1, al_order, al_sel; DevBuf<hao_ed_result_t> al_res; DevBuf<hao_trace_result_t> al_tres;
	DevBuf<uint8_t> al_want; DevBuf<uint16_t> al_cig;
	uint32_t ded_window = 0, ded_thre = 0;      // hao_deliver_ed_config: the grid of HAO_DELIVER_ED (window 0: not configured); per context, a view has its own
	// reference placement (hao_grid_pair.cuh: hao_ref_pair).  ded_place / ded_erate / ded_tab: hao_deliver_ed_config_ref (the table is uploaded at configuration
	// time: no host-to-device copy inside a batch).  rf: the stage's scratch, compute stream only (the blocking call and HAO_DELIVER_ED share it) - covered windows
	// per overlap and their scan, the shifts, the error byte per CSR slot, the pair list, the unresolved counter; rf_tab / rf_sum / rf_*: what hao_window_ed_ref
	// leaves for hao_fetch_ed_ovlp (resident while win.ed_resident()); rs_wc: the covered windows (CSR slots) of the batch the ED stage - blocking or streamed - last ran on
	uint32_t ded_place = 0; double ded_erate = 0; DevBuf<uint8_t> ded_tab;
	struct RefGrid {
		DevBuf<uint64_t> cnt, woff; DevBuf<int16_t> shift; DevBuf<uint8_t> werr; DevBuf<hao_ed_pair> pairs; DevBuf<unsigned long long> ctr;
	} rf;
	DevBuf<uint8_t> rf_tab; uint32_t rf_tab_wl = 0; double rf_tab_erate = 0; DevBuf<hao_ed_ovlp_sum> rf_sum; std::vector<hao_ed_ovlp_sum> rf_hsum; uint64_t rf_unres = 0, rs_wc = 0;
	// the rescue stage (hao_rescue.cuh; hao_window_rescue_ref and HAO_DELIVER_RESCUE): pe per CSR slot, record region start per overlap, the states of the overlaps
	// with an open window, their record regions, the column scratch, six counters - scratch of both paths; ovlp / off / wins: the blocking path's results (per-overlap
	// results and the records compacted on the device into a CSR by overlap, resident while win.rescue_resident()); h_*: hao_fetch_rescue's plain copies of the three
	struct Rescue {
		DevBuf<uint16_t> wpe; DevBuf<uint64_t> rbase, path, off; DevBuf<hao_rs_state> st; DevBuf<hao_rs_win> rec, wins; DevBuf<hao_rs_ovlp> ovlp; DevBuf<unsigned long long> ctr;
		std::vector<hao_rs_ovlp> h_ovlp; std::vector<uint64_t> h_win_off; std::vector<hao_rs_win> h_wins;
	} rs;
	uint64_t rs_slots = 0, rs_rounds = 0, rs_active = 0, rs_total = 0, rs_nw = 0;      // the last rescue stage's record slots, rounds, overlaps with an open window, rescued windows, records kept
	// the window lists (hao_wlist.cuh; hao_window_wlist_ref): records per overlap and their scan, the plan, the records, entry counts and their scan (the CSR
	// offsets), sort keys and record indices (sel: the records that need a sweep, in text order), the column scratch, two rows per swept record, the compact
	// cigars, five counters; woff / wins / cig_off / cig: the blocking path's results (resident while win.wlist_resident()); h_*: hao_fetch_wlist's host copies and
	// the read it last served; wl_out: the last stage's five counts
	struct Wlist {
		DevBuf<uint64_t> cnt, woff, ncig, cig_off, key, key2, path; DevBuf<hao_wl_plan> plan; DevBuf<hao_rs_win> wins; DevBuf<uint32_t> idx, sel, rowof; DevBuf<uint16_t> rows, cig; DevBuf<unsigned long long> ctr;
		std::vector<uint64_t> h_woff, h_cig_off, r_woff, r_cig_off; std::vector<hao_rs_win> h_wins; std::vector<uint16_t> h_cig;
	} wl;
	uint64_t wl_out[5] = { 0, 0, 0, 0, 0 };
	// the threshold ladder (hao_ladder.cuh; hao_window_ladder): requests, results, the attempts' thresholds, entry counts / row references / CSR offsets per request,
	// the open lists of this round and the next, per slot of a round the coordinates, the selected pairs of the cooperative classes and their column offsets, the
	// cigar rows of each round (kept until the CSR array is filled), the CSR array, 64 counters
	struct Ladder {
		DevBuf<hao_ladder_req_t> req; DevBuf<hao_ladder_res_t> res; DevBuf<int32_t> att; DevBuf<uint64_t> ncig, rowref, off, poff, selcnt; DevBuf<uint32_t> open[2], sel; DevBuf<hao_ld_coord> coord;
		DevBuf<uint16_t> rows[5], cig; DevBuf<unsigned long long> ctr;
		// hao_window_ladder_adv only: its results, the exact shortcut's list and one-entry cigars, the threshold of each request's last attempt (pthre)
		DevBuf<hao_ladder_adv_res_t> res_adv; DevBuf<uint32_t> xlist; DevBuf<uint16_t> xrow; DevBuf<int32_t> pth;
		DevBuf<int64_t> est;      // the estimate each request of the last hao_window_ladder_adv call ran with (hao_fetch_ladder_adv_estimates)
		// hao_window_estimate_err's own requests, values and counter: the stage touches nothing the ladder calls left resident
		DevBuf<hao_ladder_req_t> e_req; DevBuf<int64_t> e_est; DevBuf<unsigned long long> e_ctr;
	} ld;
	uint64_t ld_n = 0;      // the requests of the last ladder call
	bool ld_valid = false, ld_adv = false; uint64_t ld_ncig = 0, ld_rounds[5] = { 0, 0, 0, 0, 0 };      // hao_fetch_ladder[_adv]: the last call's entries are resident in ld.cig (ld_adv: it was hao_window_ladder_adv); their number; the open requests of each round
	// f3 with traceback on the grid (hao_trace_grid.cuh): the stage's scratch, compute stream only (hao_window_trace_grid and HAO_DELIVER_TRACE share it) -
	// flags and selected pairs, entry counts and their scans, the compact array's offsets, the column scratch, the rows of one slice, two counters
	struct TraceGrid {
		DevBuf<uint8_t> want; DevBuf<uint32_t> sel; DevBuf<uint64_t> cnt, loc, off, path; DevBuf<uint16_t> rows; DevBuf<unsigned long long> ctr;
	} tg;
	// hao_window_trace_grid's results, kept for hao_fetch_trace_grid (resident while win.trace_resident(): until a new batch or a host-fed window-alignment call):
	// the pair list, the distance-only err / pe, ps and entry count per pair, the compact cigars; pairs, traced pairs, entries, aligned but untraced pairs
	uint32_t tg_wl = 0, tg_thre = 0; uint64_t tg_n = 0, tg_nsel = 0, tg_ncig = 0, tg_nuntr = 0;
	DevBuf<hao_ed_pair> tg_pairs; DevBuf<uint8_t> tg_err; DevBuf<uint16_t> tg_pe, tg_ps, tg_ncig16, tg_cig;
	struct Batch;
	Batch *batch = nullptr;
	StageTimer timer; std::vector<std::pair<std::string, float> > stage_ms;
};

static void hao_set_err(hao_ctx *c, const std::string &m) { if (c) c->err = m; }

#define HAO_CHECK_LAUNCH() HIP_TRY(hipGetLastError())

// `words` device words at src into a read-back slot, on the engine's stream (one wave; no copy engine: see hao_peek_kernel)
static int hao_peek(hao_ctx *c, const void *src, int words, hao_peek_id slot)
{
	if (words > HAO_PEEK[slot].n) { hao_set_err(c, "hao_peek: more words than the slot holds"); return HAO_EINVAL; }
	hipLaunchKernelGGL(hao_peek_kernel, dim3(1), dim3(64), 0, c->stream, (const unsigned long long*)src, words, c->peek_d + HAO_PEEK[slot].at); HAO_CHECK_LAUNCH();
	return HAO_OK;
}

// sharded mode (the engine holds a slice of the read store)?  A view (hao_attach) has no communicator of its own: its owner's decides.
static bool hao_comm_is_active(const struct hao_comm *cm);
static inline bool hao_is_sharded(const hao_ctx *c) { const hao_ctx *o = c->owner ? c->owner : c; return o->comm && hao_comm_is_active(o->comm); }

// The reads as the stages beyond the seam see them (hao_exact_check, the window alignments, hao_reads_digest): ONE store whose entries are named by the ids the
// tasks, ol->list and the batch's queries carry.  An unsharded engine: its local store (id_base = rid_base, the id of entry 0, which only the exact check
// subtracts; local0 = 0).  A sharded engine with a gathered store: that store and the replicated lengths, entries = global ids (id_base = 0; local0 = rid_base,
// the entry of the engine's local read 0).  A sharded engine without one has no view: the stages refuse.  h_len: the host's copy of len.
struct hao_read_view {
	const uint8_t *packed; const uint64_t *pk_off; const uint32_t *len; const uint64_t *nsite_off; const uint32_t *nsite;      // nsite_off == nullptr: no read has N
	const uint32_t *h_len; uint64_t n, id_base, local0;
};
static inline bool hao_reads_view(const hao_ctx *c, hao_read_view *V)
{
	if (!hao_is_sharded(c)) {
		V->packed = c->d_packed.p; V->pk_off = c->d_pk_off.p; V->len = c->d_len.p; V->nsite_off = c->has_n ? c->d_nsite_off.p : nullptr; V->nsite = c->has_n ? c->d_nsite.p : nullptr;
		V->h_len = c->h_len.data(); V->n = c->n_reads; V->id_base = c->rid_base; V->local0 = 0;
		return true;
	}
	if (!c->gs_valid) return false;
	V->packed = c->g_packed.p; V->pk_off = c->g_pk_off.p; V->len = c->d_len_all.p; V->nsite_off = c->gs_has_n ? c->g_nsite_off.p : nullptr; V->nsite = c->gs_has_n ? c->g_nsite.p : nullptr;
	V->h_len = c->h_len_all.data(); V->n = c->n_total; V->id_base = 0; V->local0 = c->rid_base;
	return true;
}
// a stage's first step: its view, or today's refusal (`what`: the entry point and what it needs, as the message has always said)
#define HAO_STAGE_VIEW(c, V, what) hao_read_view V; do { if (!hao_reads_view((c), &V)) { hao_set_err((c), what ": single-device mode only"); return HAO_EUNSUPP; } } while (0)

// scratch for rocprim calls
static inline hipError_t hao_tmp(hao_ctx *c, size_t bytes) { return c->d_tmp.reserve(bytes + 256); }

// a rocprim call: run(nullptr, bytes) asks for the scratch size, run(scratch, bytes) does the work
template<typename F>
static int hao_rocprim(hao_ctx *c, F run)
{
	size_t tb = 0;
	HIP_TRY(run((void*)nullptr, tb));
	HIP_TRY(hao_tmp(c, tb));
	HIP_TRY(run((void*)c->d_tmp.p, tb));
	return HAO_OK;
}
template<typename In, typename Out>
static int hao_excl_scan_u64(hao_ctx *c, In in, Out out, size_t n)
{
	return hao_rocprim(c, [&](void *tmp, size_t &tb) { return rocprim::exclusive_scan(tmp, tb, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), c->stream); });
}
// (k_in, v_in) -> (k_out, v_out), stable, by the low `bits` bits of the key
template<typename K, typename V>
static int hao_sort_pairs(hao_ctx *c, K *k_in, K *k_out, V *v_in, V *v_out, size_t n, unsigned bits)
{
	return hao_rocprim(c, [&](void *tmp, size_t &tb) { return rocprim::radix_sort_pairs(tmp, tb, k_in, k_out, v_in, v_out, n, 0, bits, c->stream); });
}
// out = the entries of `in` that a flag array (a pointer: flag[i] of entry i) or a predicate on the entry's value keeps, in order; *count = how many
template<typename In, typename F, typename Out>
static int hao_select(hao_ctx *c, In in, F flags_or_pred, Out out, uint64_t *count, size_t n)
{
	return hao_rocprim(c, [&](void *tmp, size_t &tb) {
		if constexpr (std::is_pointer<F>::value) return rocprim::select(tmp, tb, in, flags_or_pred, out, count, n, c->stream);
		else return rocprim::select(tmp, tb, in, out, count, n, flags_or_pred, c->stream);
	});
}

// column scratch of the window-alignment stages: pairs per slice of a sweep over n pairs that keeps bytes_per_pair each - whole blocks of 256, within the budget
// (c->sw.al_slice, 4 GB unless a test shrinks it), one block at the least
static inline uint64_t hao_col_slice(const hao_ctx *c, uint64_t n, uint64_t bytes_per_pair)
{
	return std::max<uint64_t>(256, std::min<uint64_t>((n + 255) & ~255ULL, (c->sw.al_slice / bytes_per_pair) & ~255ULL));
}
// scratch of more than `bytes` is not kept between calls
#define HAO_SCRATCH_KEEP (1ULL << 30)
template<typename T> static inline void hao_release_above(DevBuf<T> &b, uint64_t bytes) { if ((uint64_t)b.cap * sizeof(T) > bytes) b.release(); }

// An attached batch context (hao_attach) reads the owner's read store and index through borrowed pointers; they are taken again whenever the owner has
// rebuilt something since (the owner must not be rebuilding while a view runs a batch: same rule as for the owner's own batches).
static int hao_view_refresh(hao_ctx *c)
{
	hao_ctx *o = c->owner;
	if (!o || c->attached_gen == o->index_gen) return HAO_OK;
	c->opt = o->opt;
	c->n_reads = o->n_reads; c->n_bases = o->n_bases; c->n_pk_bytes = o->n_pk_bytes; c->has_n = o->has_n; c->max_len = o->max_len;
	c->rid_base = o->rid_base; c->n_total = o->n_total; c->max_len_all = o->max_len_all; c->n_cu = o->n_cu; c->max_n_chain = o->max_n_chain; c->hom_cov = o->hom_cov; c->het_cov = o->het_cov;
	c->has_pt = o->has_pt; c->ix_n_mz = o->ix_n_mz; c->ix_n_sorted = o->ix_n_sorted; c->ix_n_keys = o->ix_n_keys; c->ix_n_pos = o->ix_n_pos; c->ix_pad = o->ix_pad; c->ix_bucket_bits = o->ix_bucket_bits; c->lk_valid = o->lk_valid;
	c->h_len = o->h_len; c->h_nsite_off = o->h_nsite_off; c->h_len_all = o->h_len_all; c->h_ix_mz_off = o->h_ix_mz_off;      // (empty: copied from the device on first use)
	c->d_packed.borrow(o->d_packed); c->d_pk_off.borrow(o->d_pk_off); c->d_len.borrow(o->d_len); c->d_len_all.borrow(o->d_len_all); c->d_nsite_off.borrow(o->d_nsite_off); c->d_nsite.borrow(o->d_nsite);
	c->gs_valid = o->gs_valid; c->gs_has_n = o->gs_has_n; c->gs_pk_bytes = o->gs_pk_bytes; c->gs_nsites = o->gs_nsites;
	c->g_packed.borrow(o->g_packed); c->g_pk_off.borrow(o->g_pk_off); c->g_nsite_off.borrow(o->g_nsite_off); c->g_nsite.borrow(o->g_nsite);
	c->d_ix_mz_x.borrow(o->d_ix_mz_x); c->d_ix_mz_info.borrow(o->d_ix_mz_info); c->d_ix_mz_off.borrow(o->d_ix_mz_off); c->d_ix_sinfo.borrow(o->d_ix_sinfo); c->d_ix_lk.borrow(o->d_ix_lk);
	c->d_ix_keys.borrow(o->d_ix_keys); c->d_ix_start.borrow(o->d_ix_start); c->d_ix_cnt.borrow(o->d_ix_cnt); c->d_ix_bucket.borrow(o->d_ix_bucket);
	c->attached_gen = o->index_gen;
	return HAO_OK;
}
