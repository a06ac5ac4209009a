/* hao.h - C ABI of the MI355X-native all-vs-all overlap engine ("hao" = hifiasm-amd
 * overlap).  Plain pointers and sizes only; every entry point names the reference
 * interface (chhylp123/hifiasm 0.25.0-r726, file:line) it stands in for.
 *
 * The reference has no plugin/FFI layer: its seam is three externally linked C++
 * functions reached from per-read worker threads,
 *     ha_ft_gen   (htab.h:79,  htab.cpp:1136)   k-mer count -> high-count filter table
 *     ha_pt_gen   (htab.h:86,  htab.cpp:1232)   minimizer count + position index
 *     h_ec_lchain (anchor.cpp:2302, declared ad hoc at ecovlp.cpp:110)
 *                                               per-read seeds -> chains -> overlap list
 * plus the accessors ha_ft_cnt (htab.h:80), ha_pt_get / ha_pt_cnt (htab.h:88-90) and the
 * finer per-read seam mz1_ha_sketch (htab.h:122).  A GPU wants batches, so this ABI is
 * "precompute, then serve": hao_overlap_batch() runs the whole path for a range of
 * query reads on the device and hao_fetch_*() serve the per-read results that a
 * drop-in h_ec_lchain shim copies into the caller's overlap_region_alloc /
 * Candidates_list (INTEGRATION.md shows that shim).
 *
 * All functions return 0 on success, a negative HAO_E* code otherwise (the reference
 * itself exits on error; a shim maps non-zero to exit(1)).  There is NO CPU fallback:
 * without a HIP device hao_create fails.
 */
#ifndef HAO_H
#define HAO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAO_OK          0
#define HAO_ENODEV     -1   /* no HIP device / HIP runtime error */
#define HAO_EINVAL     -2   /* bad argument or call order */
#define HAO_ENOMEM     -3
#define HAO_EUNSUPP    -4   /* input outside what the device path implements (fails loudly, never falls back) */

typedef struct hao_ctx hao_ctx;

/* Mirrors the fields of hifiasm_opt_t (CommandLines.h:35-173) the hot path reads. */
typedef struct {
	int32_t k;             /* k_mer_length   (CommandLines.cpp:259) default 51 */
	int32_t w;             /* mz_win         (CommandLines.cpp:263) default 51 */
	int32_t hpc;           /* !(flag & HA_F_NO_HPC), default 1 */
	int32_t sample_dist;   /* mz_sample_dist (CommandLines.cpp:268) default 500 */
	int32_t rewin;         /* mz_rewin       (CommandLines.cpp:266) default 1000 */
	int32_t min_hist_cnt;  /* min_hist_kmer_cnt, default 5 */
	int32_t max_kmer_cnt;  /* (CommandLines.cpp:270) default 2000 */
	int32_t max_n_chain;   /* (CommandLines.cpp:276) default 100; raised like ha_opt_update_cov */
	double  high_factor;   /* (CommandLines.cpp:271) default 5.0 */
	int32_t is_ont;        /* --ont: bw_thres 0.05 instead of 0.02 (ecovlp.cpp:3274) */
	int32_t bf_shift;      /* -f (CommandLines.cpp:269, reference default 37): log2 of the Bloom filter bits in front of the k-mer count table of
	                        * ha_ft_gen (htab.cpp:99-116,140-160,196-206); 0 = exact counting. hao_opt_default sets 0; a shim passes asm_opt.bf_shift */
	int64_t hg_size;       /* --hg-size (CommandLines.cpp:331,959; default -1): when > 0 the peak finder is given the prior
	                        * homozygous coverage total_bases / hg_size (htab.cpp:1156,1254; adj_m_peak_hom, hist.cpp:46-72) */
} hao_opt_t;

/* ha_mz1_t (htab.h:13-18): info = rid:28 | pos:27 | rev:1 | span:8 (LSB first).
 * ha_idxpos_t (htab.h:20-22) has the same bit layout without x. */
typedef struct { uint64_t x, info; } hao_mz_t;
/* k_mer_hit (Hash_Table.h:116-120): w0 = readID:31 | strand:1 */
typedef struct { uint32_t w0, offset, self_offset, cnt; } hao_hit_t;
/* the scalar fields of overlap_region (Hash_Table.h:78-106) that h_ec_lchain defines */
typedef struct {
	uint32_t x_id, x_pos_s, x_pos_e, x_pos_strand;
	uint32_t y_id, y_pos_s, y_pos_e, y_pos_strand;
	int32_t  shared_seed;
	uint32_t align_length;            /* zero on return (anchor.cpp:2098) */
	uint32_t non_homopolymer_errors;  /* index of the chain's first hit in the read's hit list */
	uint32_t fc_len;                  /* Fake_Cigar.length */
} hao_ovlp_t;

void hao_opt_default(hao_opt_t *o);                       /* init_opt, CommandLines.cpp:243-380 */
int  hao_create(int device, const hao_opt_t *opt, hao_ctx **out);
void hao_destroy(hao_ctx *c);
const char *hao_last_error(const hao_ctx *c);

/* Read store hand-over.  Layout = the reference's All_reads (Process_Read.h:115-146):
 * packed = concatenation of read_sperate[i] (len/4+1 bytes per read, 4 bases/byte, first base
 * in bits 7..6; ha_compress_base, Process_Read.cpp:792-850), pk_off[n+1] byte offsets,
 * len[n] = read_length[], nsite_off[n+1]/nsite[] = flattened N_site lists (may be NULL).
 * Host pointers; copied to HBM once. */
int hao_set_reads(hao_ctx *c, const uint8_t *packed, const uint64_t *pk_off, const uint32_t *len, uint64_t n_reads,
				  const uint64_t *nsite_off, const uint32_t *nsite);

/* ---- sharded mode: one process per GPU, reads partitioned by query read ----
 * The reference shards its tables over threads (4096 sub-tables, htab.cpp:147-151,594-606); across GPUs the engine
 * shards READS: rank r holds reads [rid_base, rid_base+n_local) of n_total.  After hao_set_reads (local reads) call
 * hao_set_shard with the lengths of ALL reads (read_length[], replicated: 4 B/read), and hao_dist_init with an id
 * produced once by hao_dist_unique_id and broadcast by the launcher (ncclGetUniqueId / ncclCommInitRank).
 * hao_ft_gen then counts k-mers by hash range (all-to-all-v of 8-byte hashes, 32 KB histogram all-reduce,
 * all-gather-v of the small filter table); hao_pt_gen all-gathers the 16-byte minimizer records so every rank holds
 * the whole index; hao_overlap_batch needs no communication.  Read ids in all results are GLOBAL; the batch range of
 * hao_overlap_batch / hao_fetch_* stays LOCAL (0 .. n_local). */
int hao_set_shard(hao_ctx *c, uint64_t rid_base, uint64_t n_total, const uint32_t *all_len);
int hao_dist_unique_id(uint8_t id[128]);
int hao_dist_init(hao_ctx *c, const uint8_t id[128], int rank, int world);
/* loopback exchange backend: `world` engines in ONE process (one host thread each) on one GPU; test-only substitute for RCCL */
void *hao_loop_create(int world);
void hao_loop_destroy(void *grp);
int hao_dist_init_loopback(hao_ctx *c, void *grp, int rank);
/* The stages beyond the seam - hao_exact_check / HAO_DELIVER_EXACT, hao_window_ed_batch, hao_window_trace_batch, hao_window_ed_grid, hao_window_trace_grid,
 * hao_window_ed_ref, hao_window_rescue_ref, hao_window_wlist_ref and HAO_DELIVER_ED / TRACE / RESCUE / WLIST - read the bases of BOTH reads of an overlap, and a
 * sharded engine holds the bases of its own slice only: they return HAO_EUNSUPP there ("single-device mode only"), as their comments below say - until
 * hao_dist_gather_reads has run.  A collective over the engine's transport (every rank calls it; after hao_set_reads, hao_set_shard and the dist init, in any
 * order relative to hao_ft_gen / hao_pt_gen): it replicates the read store as hao_pt_gen replicates the index - every rank's packed bytes, pack offsets, N-site
 * offsets and N sites all-gathered in chunks of bounded size into one GATHERED STORE in global read-id order (packed bytes of all n_total reads + 8 bytes per read,
 * + 8 bytes per read and 4 per site when a read has N), pack and N-site offsets turned from local to global on the device.  From then on every stage named above
 * runs in the sharded engine, blocking and streamed, over that store: tasks, x_id and y_id name reads by GLOBAL id there (hao_window_ed_batch /
 * hao_window_trace_batch take tasks between any two of the n_total reads), batch ranges and the hao_fetch_* read argument stay LOCAL, and the results are bit for
 * bit the unsharded engine's.  The hao_unpack_* helpers index one `len` array by a delivery's rid_lo-based read ids and by y_id: for a sharded engine's
 * delivery pass a copy of the view with rid_lo += rid_base, the lengths of all reads and global read ids.
 *   Calling it again while the store is valid is a no-op (no communication); hao_set_reads and hao_set_shard discard the store (the refusals are back until the
 *   next gather); an attached context (hao_attach) borrows it.  The ranks fail together (a rank whose allocation failed takes part in the status exchange and
 *   all return an error).  Shards that are not contiguous slices in rank order: HAO_EINVAL on every rank.  On an unsharded engine: HAO_OK, nothing is allocated -
 *   the local store is the whole store.  hao_index_save on a sharded engine needs this store (below).
 *   HAO_DBG_TEST=gather_chunk=N: bytes a rank sends per exchange (default 64 MB; a few KB walk the multi-chunk path on a small read set). */
int hao_dist_gather_reads(hao_ctx *c);
/* Digest of the reads as the stages above see them - the local store of an unsharded engine, the gathered store of a sharded one (HAO_EUNSUPP without it) -
 * computed on the device (one wave per read).  With term() as for hao_batch_digest below, for read r (its id in that store) of L bases and m N sites:
 *   bases(r) = term(5, 0, L) + sum of term(5, j + 1, w_j) over the little-endian 64-bit words w_j of the read's L / 4 + 1 packed bytes, zero-padded to a word
 *   sites(r) = term(6, 0, m) + sum of term(6, k + 1, site_k) over the read's N sites
 *   out[0] = sum over r of term(7, r, bases(r)),  out[1] = sum over r of term(8, r, sites(r))      (mod 2^64)
 * Pack offsets are not part of it: any layout of the same reads gives the same value, so every rank of a sharded engine must report what an unsharded engine
 * over the same reads reports. */
int hao_reads_digest(hao_ctx *c, uint64_t out[2]);

/* ha_ft_gen (htab.cpp:1136-1169), exact (-f0) or through the reference's blocked Bloom filter (opt.bf_shift > 12, bit-exact incl. its false
 * positives: see hao_tables.hpp), + ha_opt_update_cov (CommandLines.cpp:411-418). */
int hao_ft_gen(hao_ctx *c, int32_t *hom_cov);
/* ha_pt_gen (htab.cpp:1232-1287) + the asm_opt.hom_cov/het_cov update of Assembly.cpp:1007-1008.
 * The index and the per-read minimizers stay resident in HBM. */
int hao_pt_gen(hao_ctx *c, int32_t *hom_cov, int32_t *het_cov);

/* host-side views (what non-default CPU consumers of ha_flt_tab / ha_idx need) */
int32_t hao_ft_cnt(hao_ctx *c, uint64_t y);                                   /* ha_ft_cnt htab.cpp:1064 */
int hao_pt_get(hao_ctx *c, uint64_t hash, const uint64_t **pos, int32_t *n);  /* ha_pt_get htab.cpp:518  */
int hao_ft_table(hao_ctx *c, uint64_t *n, const uint64_t **keys, const int32_t **vals);
int hao_pt_table(hao_ctx *c, uint64_t *n_keys, const uint64_t **keys, const uint64_t **off, const uint64_t **pos, uint64_t *n_pos);
int hao_hist(hao_ctx *c, int which /*0 = all k-mers (ft), 1 = minimizers (pt)*/, int64_t cnt[4096]);
/* out[0..7] = ft peak_hom, ft peak_het, ft cutoff, max_n_chain, hom_cov, het_cov, high_occ, low_occ */
int hao_stats(hao_ctx *c, int64_t out[8]);
/* hash-range passes the last hao_ft_gen counted in (1: every k-mer occurrence of the local reads at once, 2 x 8 bytes per base; more when that does not fit the
   free device memory, or as HAO_FT_PASSES says: htab.cpp:707-882 never holds all occurrences either); < 0: error */
int hao_ft_passes(hao_ctx *c);

/* mz1_ha_sketch (sketch.cpp:454-579) for reads [rid_lo, rid_hi): results stay on the device;
 * use_ft = 0 passes hf = NULL; sample_dist <= w disables the high-count thinning (sketch.cpp:575).
 * hao_fetch_sketch copies one read's list (rid field = read id, as at index time htab.cpp:691). */
int hao_sketch_batch(hao_ctx *c, uint64_t rid_lo, uint64_t rid_hi, int use_ft, int sample_dist);
int hao_fetch_sketch(hao_ctx *c, uint64_t rid, const hao_mz_t **mz, uint64_t *n);

/* The per-pass arguments of h_ec_lchain (anchor.cpp:2302). hao_pass_default fills them as
 * worker_hap_ec does (ecovlp.cpp:3237-3238,3274): bw_thres 0.02 (0.05 --ont), max_n_chain and
 * high/low_occ from the current coverage peaks, mcopy 3 / 0.7 / 32, chain_cutoff 2, ocv_w 3072.
 * The final-round caller (ecovlp.cpp:3957) differs only in bw_thres = 0.001. */
typedef struct {
	double   bw_thres;
	int32_t  max_n_chain;
	uint32_t high_occ, low_occ;
	int32_t  apend_be, is_accurate, gen_off;   /* must be 1, 1, 1 (every hot-path call site) */
	int32_t  mcopy_num;                        /* <= 3 */
	double   mcopy_rate;
	uint32_t chain_cutoff, mcopy_khit_cut;
	uint64_t ocv_w;
} hao_pass_t;
int hao_pass_default(hao_ctx *c, hao_pass_t *p);

/* h_ec_lchain (anchor.cpp:2302-2315) for query reads [rid_lo, rid_hi); hao_overlap_batch uses
 * hao_pass_default. Results stay in HBM and are served per read by hao_fetch_*. */
int hao_overlap_batch(hao_ctx *c, uint64_t rid_lo, uint64_t rid_hi);
int hao_overlap_batch_ex(hao_ctx *c, uint64_t rid_lo, uint64_t rid_hi, const hao_pass_t *pass);
/* seed hits before chaining (cl->list after minimizers_qgen0, anchor.cpp:987-1081) */
int hao_fetch_seed_hits(hao_ctx *c, uint64_t rid, const hao_hit_t **hits, uint64_t *n);
/* ol->list[0..n_ol), their fake cigars (fc_off[n_ol+1] into fc) and cl->list[0..n_cl) */
int hao_fetch_overlaps(hao_ctx *c, uint64_t rid, const hao_ovlp_t **ol, uint64_t *n_ol, const uint64_t **fc, const uint64_t **fc_off,
					   const hao_hit_t **cl, uint64_t *n_cl);
/* totals of the last batch: out[0] = overlaps (sum ol->length), out[1] = chained hits, out[2] = seed hits,
 * out[3] = chain groups, out[4] = minimizers of the query reads */
int hao_batch_totals(hao_ctx *c, uint64_t out[8]);
/* which kernels carried the seed stage (minimizers_qgen0, anchor.cpp:987-1081) of the last batch - a measurement aid, the results do not depend on it:
 * out[0] = first launch: 2 the list-major kernel (hao_query5.cuh), 1 unused (round 5's one-wave merge kernel), 0 the table kernels for every read;
 * out[1] = reads that launch left to the table kernels, out[2] / out[3] = reads whose bins overflowed the 512- / the 1024-slot table */
int hao_batch_seed_path(hao_ctx *c, uint64_t out[4]);
/* which kernels carried the chain stage (h_ec_lchain's chaining of one (query, target) group of seed hits) of the last batch - the results do not depend on it.
 * Groups are routed by their number of hits: class 0 = 1 .. 8, 1 = 9 .. 64, 2 = 65 .. 128, 3 = 129 .. 256, 4 = 257 .. 512, 5 = 513 .. 2048, 6 = more.
 * out[0 .. 6] = groups of each class, out[7 .. 13] = of those, the groups the data-parallel quick check did not settle and handed to the DP kernel of their
 * class (class 0: to the one-lane-per-group pass), out[14] = seed hits of the handed-over groups, out[15] = 0 */
int hao_batch_chain_path(hao_ctx *c, uint64_t out[16]);

/* A second (third ...) batch context over the same reads and index: own stream, scratch and result buffers, nothing else.  Batches on different
 * contexts are independent, so one host thread per context keeps two batches in flight on the device: the seed stage of one (memory-bound) runs under
 * the chain stage of the other (instruction-bound) - the all-reads pass of configs[2] takes 128 instead of 149 ms with two contexts.  Every batch,
 * fetch, delivery and digest call works on a view; calls that change reads or index (hao_set_reads, hao_ft_gen, hao_pt_gen, ...) belong to the owner
 * and return HAO_EINVAL on a view.  A view follows the owner's rebuilds by itself (it takes the owner's buffers again at its next batch); as with the
 * owner's own batches, no batch may run while the owner rebuilds, and views are destroyed (hao_destroy) before their owner. */
int hao_attach(hao_ctx *owner, hao_ctx **view);

/* ---- streaming result delivery: results of batch i cross PCIe while batch i + 1 computes ----
 * h_ec_lchain hands ol->list and cl->list back to a per-read caller (anchor.cpp:2302; consumed by gen_hc_r_alin_ea, ecovlp.cpp:3288).  A batch's
 * results are ~190 KB per 15 kb read, almost all of it cl->list (16 bytes per chained hit), more than PCIe can carry at the rate the device produces
 * them.  The delivery path therefore (a) ships cl->list in a wire format of ~0.3 bytes per hit: a chained hit is (query minimizer, target offset);
 * self_offset and cnt belong to the query minimizer (anchor.cpp:1065-1076) and travel once per read in its minimizer table; a hit whose
 * chain simply moves on to the read's next minimizer on the same diagonal (> 90 % of them) is a 0 in the batch's bit stream, any other hit a 1
 * plus one code byte - minimizers skipped since the previous hit of the chain (high nibble) and diagonal shift + 8 (low nibble), 0xff = look the
 * hit up in the (sorted) exception list.  Bits, codes and exceptions are addressed by POSITION = index among the batch's sorted seed hits (a chain is
 * a contiguous run of positions, its header says where it starts; the code at a chain's first position is not the chain's and is skipped; positions
 * in no chain cost their bit); the consumer thread decodes straight into its Candidates_list (hao_unpack_hits); (b) copies into one of two pinned host
 * arenas on copy streams, under the next batch's kernels.  hao_overlap_batch_async returns when the batch's kernels are done and its copy is
 * queued; hao_deliver_wait blocks until the copy has landed and describes the arena.  A slot's arena (and the device buffers behind it) is reused by
 * the second-next async batch: at most two batches are in flight, and the caller must be done with batch i before it starts batch i + 2.  The views
 * are read-only and may be read by any number of threads; hao_unpack_hits is a pure function of the view. */
#define HAO_DELIVER_OL 1u      /* ol->list + fake cigars */
#define HAO_DELIVER_CL 2u      /* cl->list (wire format) */
#define HAO_DELIVER_EXACT 4u   /* one byte per overlap: the exact-overlap check of the final round (hao_exact_check) */
/* one overlap of ol->list on the wire, 32 bytes: hao_ovlp_t without what the receiver knows (x_id = the read, x_pos_strand = 0, align_length = 0; y = y_id | y_pos_strand << 31) - hao_unpack_overlaps */
typedef struct { uint32_t y, x_pos_s, x_pos_e, y_pos_s, y_pos_e; int32_t shared_seed; uint32_t non_homopolymer_errors, fc_len; } hao_ovlp_wire_t;
typedef struct { uint32_t n_hits, w0, q0, offset; uint64_t pos; } hao_chain_hdr_t;   /* one chain of cl->list: hit count, the readID word its hits share, first hit: minimizer index in the read, target offset, position; hit i of the chain has position pos + i */
typedef struct { uint32_t self_offset, cnt; } hao_qmz_t;                  /* one query minimizer: k_mer_hit::self_offset and ::cnt of every hit it seeds */
typedef struct { uint64_t index; uint32_t q, pad; hao_hit_t hit; } hao_exc_t;   /* verbatim hit: its position, its minimizer index, the hit (its readID word is the seed stage's: the decoder writes the chain's) */
typedef struct {
	uint64_t rid_lo, n_reads, n_ol, n_fc, n_chains, n_cl, n_exc, n_codes, n_pos, bytes;   /* n_pos = positions of the batch (its seed hits); bytes = what crossed PCIe for this batch */
	const uint64_t *ol_off;          /* [n_reads + 1]: ol->list of read r = ol[ol_off[r] .. ol_off[r + 1]) */
	const hao_ovlp_wire_t *ol;       /* [n_ol]: read them with hao_unpack_overlaps */
	const uint64_t *fc_off;          /* [n_ol + 1]: the fake cigar of overlap j starts at 32-bit word fc_off[j] & ~HAO_FC_RAW of fc[]; read it with hao_unpack_cigar */
	const uint32_t *fc;              /* [n_fc] words: 4 bytes per cigar entry after an overlap's first (site step | zigzag(shift step) << 20); raw overlaps (bit 63 of their offset): 2 words per entry */
	const uint64_t *ch_off, *cl_off, *qm_off; /* [n_reads + 1]: chains / hits / minimizers of read r = chains[ch_off[r] ..), hits cl_off[r] .. of the batch, qmz[qm_off[r] ..) */
	const hao_chain_hdr_t *chains;
	const uint64_t *cl_bits;         /* bit p (word p / 64, bit p % 64) = position p has a code byte */
	const uint32_t *cl_rank;         /* [n_pos / 256 + 1]: code bytes before position 256 i */
	const uint8_t *cl_codes;         /* [n_codes] code bytes, in position order */
	const hao_qmz_t *qmz;            /* minimizer tables of the batch's reads; NULL when they travel packed (qmz_pos / qmz_cnt below) */
	const hao_exc_t *cl_exc;         /* [n_exc] sorted by position */
	const uint8_t *exact;            /* [n_ol] with HAO_DELIVER_EXACT, else NULL */
	double copy_ms;                  /* from "batch computed" to "copy landed" (includes waiting behind the previous batch's copy); filled by hao_deliver_wait */
	const uint16_t *qmz_pos;         /* packed minimizer tables (4 instead of 8 bytes per minimizer): self_offset and cnt of minimizer qm_off[r] + q in two 16-bit arrays.  The engine packs when */
	const uint16_t *qmz_cnt;         /* every read is shorter than 65 536 bases and the pass's seed weights (anchor.cpp:160-173; cnt = weight << 8 | span) are below 256; else both are NULL and qmz is set */
} hao_delivery_t;
#define HAO_FC_RAW (1ULL << 63)
/* The fake cigar (Fake_Cigar, Hash_Table.h:54-59; gen_fake_cigar, Hash_Table.cpp:88-109) of overlap j of a delivered batch as its ol[j].fc_len 8-byte entries
 * (site << 32 | shift code), rebuilt from the packed words: a pure function of the view.  Returns the entry count (nothing is written when it exceeds cap). */
uint32_t hao_unpack_cigar(const hao_delivery_t *d, uint64_t j, uint64_t *out, uint32_t cap);
/* ol->list of read rid (a read of the delivered batch) as hao_ovlp_t records in out[cap]: overlaps ol_off[r] .. ol_off[r + 1) of the batch; returns their number (nothing is
 * written if cap is too small).  A pure function of the view. */
uint64_t hao_unpack_overlaps(const hao_delivery_t *d, uint64_t rid, hao_ovlp_t *out, uint64_t cap);
int hao_overlap_batch_async(hao_ctx *c, uint64_t rid_lo, uint64_t rid_hi, const hao_pass_t *pass /* NULL: hao_pass_default */, uint32_t parts, int *slot);
/* The delivery slot (0 / 1) the NEXT hao_overlap_batch_async of this context will write: the caller must have stopped reading that arena before it
 * starts the batch (the engine alternates the two slots; asking it keeps that policy out of the caller). */
int hao_next_slot(hao_ctx *c, int *slot);
int hao_deliver_wait(hao_ctx *c, int slot, hao_delivery_t *out);
/* cl->list of read rid (a read of the delivered batch) decoded into out[cap]; returns the number of hits (nothing is written if cap is too small) */
uint64_t hao_unpack_hits(const hao_delivery_t *d, uint64_t rid, hao_hit_t *out, uint64_t cap);

/* Exact-overlap check right after chaining: exact_ec_check (ecovlp.cpp:2803-2808) as the final round applies it to every
 * candidate h_ec_lchain returns (h_ec_lchain_fast_new, ecovlp.cpp:5103-5131; also gen_hc_r_alin_ea's pre-pass :2847-2856): flag = 1 iff the query
 * interval [x_pos_s, x_pos_e] and the target interval [y_pos_s, y_pos_e] on strand y_pos_strand (recover_UC_Read_sub_region,
 * Process_Read.cpp:524-614) have equal length and equal characters, N sites included.  Runs on the packed reads resident in HBM, one wave per
 * overlap, for the final ol->list of the last batch; single-device mode only (a sharded engine holds only its own reads' bases: HAO_EUNSUPP).
 * hao_fetch_exact serves one read's flags (aligned with hao_fetch_overlaps' ol). */
int hao_exact_check(hao_ctx *c);
int hao_fetch_exact(hao_ctx *c, uint64_t rid, const uint8_t **flags, uint64_t *n);

/* Windowed bit-vector edit distance: ed_band_cal_semi_64_w_absent_diag (Levenshtein_distance.h:3727-3776) for a batch of independent
 * (pattern, text) pairs taken from the reads resident in HBM - the call Correct.cpp:3897,4092,4156 makes per 775-base query window and candidate:
 * pattern = the padded target region [p_pos, p_pos + p_len) of read p_rid on strand p_rev, text = the query window [t_pos, t_pos + t_len) of read
 * t_rid on strand t_rev, thre = error threshold, abs_diag = leading diagonals missing because the pattern was clipped at the start of its read.
 * Band width: 2 thre + 1 diagonals in one 64-bit word (thre <= 31), in two (thre 32 .. 63: the reference's ed_band_cal_*_128_* functions, generated
 * from the same text by HA_ED_INIT(128), :1287-2129, and chosen by band width, cal_exz_global Correct.cpp:15482-15494), or in nword = 3 / 4 words
 * (thre 64 .. 95 / 96 .. 127: the reference's ed_band_cal_*_infi_* functions, :2134-3100, which cal_exz_infi calls with nword = ceil((2 thre + 1) / 64),
 * Correct.cpp:14508-14565); thre > HAO_ED_MAX_THRE: HAO_EINVAL here - wider bands, up to nword = 64 (thre <= HAO_ED_LONG_MAX_THRE), are hao_window_ed_long's and
 * hao_window_trace_long's, where a segment of 8 .. 64 lanes owns a pair and each lane holds one word of the band.  With a band of two or more words p_len - t_len + abs_diag <= 64 nword is required
 * (beyond it the reference's final scan indexes past its band words).  out[i].err = edit distance or INT32_MAX (no alignment within thre, the reference's clear_align state), out[i].pe = end of the
 * alignment on the pattern or -1; ps = -1, ts = 0, te = t_len - 1 are constants of the call.  One lane per pair; single-device mode (the bases of
 * both reads must be local).  This is the data-parallel core of the window alignment; window placement and retries stay with the caller. */
#define HAO_ED_MAX_THRE 127     /* widest band: 255 diagonals in four 64-bit words */
typedef struct { uint32_t p_rid, p_pos, p_len, p_rev, t_rid, t_pos, t_len, t_rev, thre, abs_diag; } hao_ed_task_t;
typedef struct { int32_t err, pe; } hao_ed_result_t;
int hao_window_ed_batch(hao_ctx *c, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_ed_result_t *out);

/* f3 without a host in the loop (round 5): the window / candidate pairs of the LAST batch (hao_overlap_batch[_ex]; results resident) are generated on the device from the
 * batch's final ol->list on the reference's fixed window grid - windows of `window` query bases (WINDOW = 375, Hash_Table.h:9; Correct.cpp:5645, 5993) starting at
 * multiples of `window`, one pair per overlap and grid window it covers, the window clipped to the overlap at its ends, the pattern = the target interval on the
 * overlap's diagonal padded by thre on both sides and clipped at the read ends with abs_diag = the bases clipped at its start (the operands Correct.cpp:3897 hands to
 * ed_band_cal_semi_64_w_absent_diag, without the fake-cigar shift: DIAGONAL placement; hao_window_ed_ref below places them as the reference does) - in text order (query read, grid window, position in ol->list), and the distance-only window
 * alignment (hao_window_ed_batch's kernels) runs over them where they lie.  Tasks and results stay in device memory; *n_tasks = their number.
 * hao_fetch_ed_grid copies the first `cap` of them out (either pointer may be NULL).  One threshold per call (thre <= HAO_ED_MAX_THRE); single-device mode. */
int hao_window_ed_grid(hao_ctx *c, uint32_t window, uint32_t thre, uint64_t *n_tasks);
int hao_fetch_ed_grid(hao_ctx *c, hao_ed_task_t *tasks, hao_ed_result_t *res, uint64_t cap);

/* f3 in the streaming pass: the window alignment delivered WITH each batch.  HAO_DELIVER_ED in the parts of hao_overlap_batch_async (with HAO_DELIVER_OL; after
 * hao_deliver_ed_config on this context, else HAO_EINVAL; sharded mode: HAO_EUNSUPP) aligns, on the device and right after chaining, every grid pair of the batch -
 * the pairs hao_window_ed_grid(window, thre) forms from the batch's final ol->list, in the same text order (query read, grid window, position in ol->list), with
 * the same (err, pe) - and the results cross PCIe in the batch's arena: 3 bytes per pair (an error byte, 0xff = no alignment within thre, and a 16-bit pattern
 * end, 0xffff = -1) plus the pairs' offsets per read.  Tasks do not travel: hao_unpack_ed rebuilds them from the delivered overlaps.  The blocking path's
 * task / result scratch (hao_window_ed_grid / hao_fetch_ed_grid) is not touched; batches without HAO_DELIVER_ED keep their arena layout and byte count.
 * The pairs above are DIAGONAL placement (target start on the overlap's first diagonal, one threshold per call); hao_deliver_ed_config_ref switches the context
 * to REFERENCE placement (below: the fake-cigar shift, per-window thresholds, init_waln).  Not covered: the sharded path.  The semi-global traced mode rides
 * along as HAO_DELIVER_TRACE (below; diagonal placement only); the other traced modes stay host-fed.
 *   hao_deliver_ed_config: the grid of this context's HAO_DELIVER_ED batches (an attached view has its own).  window == 0, thre > HAO_ED_MAX_THRE or
 *                          window + 2 thre >= 65535 (pe travels in 16 bits): HAO_EINVAL.  Bands of two or more words leave out the pairs hao_window_ed_grid leaves out.
 *   hao_deliver_ed:        the ED view of a slot whose batch asked for HAO_DELIVER_ED, valid after hao_deliver_wait on that slot; its pointers live in the slot's
 *                          pinned arena, with the same lifetime as the hao_delivery_t's.  HAO_EINVAL for a slot without ED results or not yet waited for.
 *   hao_unpack_ed:         read rid's pairs as hao_ed_task_t records rebuilt from the delivered overlaps (d: the same slot's hao_delivery_t; len: the lengths of
 *                          ALL reads, as given to hao_set_reads) and their results widened to hao_ed_result_t (err INT32_MAX / pe -1 without an alignment).
 *                          Returns the pair count; nothing is written when it exceeds cap (or tasks / res is NULL); 0 for a read outside the batch;
 *                          UINT64_MAX when the rebuilt pairs do not match the delivered count (len is not the batch's).  A pure function of the two views. */
/* REFERENCE PLACEMENT of the grid pairs: the window / candidate pairs as the reference's correction pass forms them (align_hc_ed_post_extz,
 * Correct.cpp:12951-13006, per overlap from gen_hc_r_alin :25637; the same loop in align_ul_ed_post_extz :12900 and verify_window :382-559).  The grid windows
 * and the text order of the pairs are those of hao_window_ed_grid; what differs is
 *   - the target start: (q_s - x_pos_s) + y_pos_s + y_start_offset(q_s, fake cigar) (Hash_Table.h:165-189) - the diagonal of the nearest chained seed before
 *     the window, read from the overlap's own fake cigar.  A window whose start resolves to no cigar entry (the reference would exit) forms no pair and is
 *     counted as unresolved, as is one whose shift does not fit 16 bits (0 for every cigar h_ec_lchain produces with apend_be = 1);
 *   - the threshold: one per window from its length q_l, (int64_t)(q_l * e_rate), 0 -> 1 when q_l >= 4 (Adjust_Threshold, Correct.h:46), at most 31
 *     (THRESHOLD_MAX_SIZE, Hash_Table.h:24): computed on the host in double as a table of window + 1 bytes (hao_ref_thresholds) that the kernels read;
 *   - admission and clipping: init_waln (Correct.cpp:764-779).  p_pos / p_len = its r_s / r_l, abs_diag = its aux_beg.
 * window = WINDOW_HC 775 (HiFi) / WINDOW_OHC 375 (ONT), e_rate = asm_opt.max_ov_diff_ec 0.04 / 0.07 in the reference.  window == 0, window + 62 >= 65535 or
 * e_rate outside (0, 1): HAO_EINVAL; sharded mode: HAO_EUNSUPP.
 *   hao_window_ed_ref:         blocking, over the last batch; tasks and results lie where hao_window_ed_grid leaves them, so hao_fetch_ed_grid serves them;
 *                              *unresolved (may be NULL) = the batch's unresolved windows.
 *   hao_fetch_ed_ovlp:         the per-overlap summaries of the last hao_window_ed_ref for read rid, aligned with hao_fetch_overlaps' ol: windows covered, windows
 *                              aligned (err != INT32_MAX), the sum of their lengths - the align_length the reference's loop accumulates before its rescue step (hao_rescue_ovlp_t has the final one),
 *                              what its OVERLAP_THRESHOLD_HIFI_FILTER test (simi_pass) starts from - and the sum of their errors.
 *   hao_deliver_ed_config_ref: this context's following HAO_DELIVER_ED batches are reference-placed (hao_deliver_ed_config switches back).  The 3 bytes per pair
 *                              and the per-read offsets travel as before, the summaries (16 bytes per overlap) after them; hao_deliver_ed's view names placement
 *                              and e_rate, and hao_unpack_ed rebuilds a read's tasks from the delivered overlaps AND their delivered fake cigars.
 * The traced stage in reference placement is hao_window_wlist_ref / HAO_DELIVER_WLIST (below; it traces the windows of the overlaps that pass the rescue stage's
 * verdict).  The diagonal traced grid has no reference-placed form: HAO_DELIVER_TRACE on a reference-placed context returns HAO_EUNSUPP, hao_window_trace_grid has no
 * reference-placed form, and hao_unpack_trace returns 0 for a reference-placed view (never diagonal cigars under a reference-placed configuration).  The reference's rescue of unaligned windows from their aligned neighbours, its early exit and its
 * return value: hao_window_rescue_ref below (blocking path). */
#define HAO_PLACE_DIAG 0u
#define HAO_PLACE_REF 1u
typedef struct { uint32_t n_win, n_aligned, aligned_bases, err_sum; } hao_ed_ovlp_t;
#define HAO_DELIVER_ED 8u      /* window-alignment results of the batch's grid pairs (hao_deliver_ed_config, hao_deliver_ed, hao_unpack_ed) */
typedef struct {
	uint64_t n_pairs;           /* pairs of the batch */
	uint32_t window, thre;      /* the grid the batch was aligned on (hao_deliver_ed_config at the time of the batch) */
	const uint64_t *ed_off;     /* [n_reads + 1]: pairs of read r = [ed_off[r], ed_off[r + 1]) */
	const uint8_t *err;         /* [n_pairs]: edit distance, 0xff = no alignment within thre */
	const uint16_t *pe;         /* [n_pairs]: end of the alignment on the pattern, 0xffff = -1 */
	/* (the fields below were added with reference placement: hao_deliver_ed now writes 72 bytes, so callers built against the 40-byte struct must be rebuilt) */
	uint32_t placement, pad;    /* HAO_PLACE_DIAG / HAO_PLACE_REF: how the batch's pairs were placed; in reference placement thre = the full window's threshold */
	double e_rate;              /* reference placement: the e_rate of hao_deliver_ed_config_ref at the time of the batch (0 in diagonal placement) */
	uint64_t unresolved;        /* reference placement: covered windows of the batch whose start resolved to no fake-cigar entry, or whose shift does not fit the
	                             * 16 bits the device keeps per window (|shift| > 32767): they form no pair.  0 for every cigar h_ec_lchain produces */
	const hao_ed_ovlp_t *ovlp;  /* reference placement: [n_ol] per-overlap summaries, aligned with the hao_delivery_t's ol; NULL in diagonal placement */
} hao_ed_delivery_t;
int hao_deliver_ed_config(hao_ctx *c, uint32_t window, uint32_t thre);
int hao_deliver_ed(hao_ctx *c, int slot, hao_ed_delivery_t *out);
uint64_t hao_unpack_ed(const hao_ed_delivery_t *e, const hao_delivery_t *d, const uint32_t *len, uint64_t rid, hao_ed_task_t *tasks, hao_ed_result_t *res, uint64_t cap);
int hao_window_ed_ref(hao_ctx *c, uint32_t window, double e_rate, uint64_t *n_tasks, uint64_t *unresolved);
int hao_fetch_ed_ovlp(hao_ctx *c, uint64_t rid, const hao_ed_ovlp_t **summary, uint64_t *n);
int hao_deliver_ed_config_ref(hao_ctx *c, uint32_t window, double e_rate);
void hao_ref_thresholds(uint32_t window, double e_rate, uint8_t *out /* [window + 1] */);     /* host code, no context */

/* The second half of align_hc_ed_post_extz (Correct.cpp:12951-13012): the rescue of the windows that did not align at first placement from their aligned
 * neighbours (push_hc_wlst_exz :12776-12836 through aln_wlst_adv_exz :4057-4131), the early exit after every aligned window and the function's return value
 * pass_qovlp(x_pos_e + 1 - x_pos_s, align_length, 0.9).  Per overlap, at every window k that aligned at first placement, in ascending order:
 *   forward:   from the window after the previous aligned window, with the target start = that window's y_end + 1, windows are aligned distance-only with the
 *              doubled threshold (31 for windows of 300 bases or more) until one fails, the gap is closed or the target is used up;
 *   backward:  if windows are still open before k, window k is traced (ed_band_cal_semi_64_w_absent_diag_trace; recal_boundary_exz may re-place it) to learn
 *              its y_start, and the windows before it are aligned leftwards with traceback, each ending at the start of the one after it (again with a
 *              recal_boundary_exz retry), until one fails, the gap is closed or the target start would be negative;
 *   exit test: align_length += the rescued windows + window k; pass_qovlp(ovl, ovl - ((q_e + 1 - x_pos_s) - align_length), 0.9) must hold, else the function
 *              returns 0 at this window (exit_win) and no later window is looked at.
 * hao_window_rescue_ref runs this on the device over the batch hao_window_ed_ref has just aligned (its pair list, error bytes and pe; HAO_EINVAL without it or
 * after another window-alignment call): one lane per overlap that has an open window before an aligned one, one alignment step per lane and round, one count
 * read per round; then a thread per overlap for the verdict.  *n_rescued = rescued windows of the batch (forward + backward, up to each overlap's exit).
 * hao_fetch_rescue: read rid's overlaps, aligned with hao_fetch_overlaps: ovlp[n], and the window records of overlap i at wins[win_off[i] .. win_off[i + 1])
 * in ascending window order (pointers valid until the next call on the context).  Records exist for rescued windows and for the aligned windows that were
 * traced (HAO_RESCUE_ANCHOR: y_start known, y_end / err possibly re-placed); none beyond exit_win.
 * HAO_RESCUE_UNTRACED in an overlap's flags: a traced alignment of a backward run (the anchor, a window, or a re-placement) fell outside the domain in which
 * the reference's traced function stays inside its band word (HAO_ALIGN_SEMI's domain below); that run ends there and nothing is guessed.
 * HAO_DELIVER_RESCUE in the parts of hao_overlap_batch_async runs the same stage on the slots, pairs and records of the batch's reference-placed ED stage and
 * delivers, after every other part: a hao_rescue_ovlp_t per overlap (aligned with the hao_delivery_t's ol), n_ol + 1 offsets, and the window records in
 * overlap and window order.  Valid only with HAO_DELIVER_ED on a context configured by hao_deliver_ed_config_ref (else HAO_EINVAL); HAO_EUNSUPP in a sharded
 * engine.  A batch without the part keeps its arena layout and byte count.
 *   hao_deliver_rescue: the view of a slot whose batch asked for the part, valid after hao_deliver_wait on that slot (HAO_EINVAL otherwise).
 *   hao_unpack_rescue:  read rid's overlaps out of the three views - ovlp[n], win_off[0 .. n] counted from the read's first record, and the records.  Returns n;
 *                       nothing is written when n exceeds cap_ovlp, the read's records exceed cap_wins, or ovlp / win_off / wins is NULL; 0 for a read outside
 *                       the batch; UINT64_MAX for a NULL view, a view that is not reference-placed, or views that do not belong together (overlap counts,
 *                       offsets that do not ascend or run past n_wins, a record whose window its overlap does not cover - the overlap's window range is
 *                       rebuilt from the delivered overlap - or that lies beyond read rid's grid as len, the lengths of all reads, has it).  Pure host code, any
 *                       thread.
 * The cigars of every window of an overlap that passed: hao_window_wlist_ref below.  Not built: gen_extend_err_exz and everything after it in gen_hc_r_alin. */
typedef struct { uint16_t verdict, flags; uint32_t exit_win, align_length, n_rescued; } hao_rescue_ovlp_t;      /* exit_win 0xffffffff: no early exit */
typedef struct { int32_t y_start, y_end; uint32_t win, info; } hao_rescue_win_t;      /* win: grid window; info: err | thre << 8 | direction << 16 | flags */
#define HAO_RESCUE_FWD 0u
#define HAO_RESCUE_BWD 1u
#define HAO_RESCUE_ANCHOR 2u
#define HAO_RESCUE_DIR(info) (((info) >> 16) & 3u)
#define HAO_RESCUE_REPLACED (1u << 18)      /* info: recal_boundary_exz's re-placement was taken */
#define HAO_RESCUE_UNTRACED 1u              /* hao_rescue_ovlp_t.flags */
#define HAO_DELIVER_RESCUE 32u      /* the rescue stage's results of the batch (with HAO_DELIVER_ED in reference placement; hao_deliver_rescue, hao_unpack_rescue) */
typedef struct {
	uint64_t n_ol, n_wins, n_rescued;      /* overlaps, window records and rescued windows (forward + backward) of the batch */
	const hao_rescue_ovlp_t *ovlp;         /* [n_ol] */
	const uint64_t *win_off;               /* [n_ol + 1]: records of overlap i = wins[win_off[i] .. win_off[i + 1]) */
	const hao_rescue_win_t *wins;          /* [n_wins] */
} hao_rescue_delivery_t;
int hao_window_rescue_ref(hao_ctx *c, uint64_t *n_rescued);
int hao_fetch_rescue(hao_ctx *c, uint64_t rid, const hao_rescue_ovlp_t **ovlp, uint64_t *n, const uint64_t **win_off, const hao_rescue_win_t **wins);
int hao_deliver_rescue(hao_ctx *c, int slot, hao_rescue_delivery_t *out);
uint64_t hao_unpack_rescue(const hao_delivery_t *d, const hao_ed_delivery_t *e, const hao_rescue_delivery_t *r, const uint32_t *len, uint64_t rid,
                           hao_rescue_ovlp_t *ovlp, uint64_t *win_off, hao_rescue_win_t *wins, uint64_t cap_ovlp, uint64_t cap_wins);
/* The product of align_hc_ed_post_extz: z->w_list, the window records of every overlap with their alignments, as the reference holds them once every window
 * has been through gen_backtrace_adv_exz (Correct.cpp:12563-12639) - what gen_extend_err_exz and gen_hc_fast_cigar0 read next.  Per overlap whose rescue
 * verdict is 1 (the others get an empty list: the reference drops them, :25637), one record per window that is aligned after the rescue, in ascending window
 * order.  The trace is a pure function of the record align_hc_ed_post_extz left, so every window is traced eagerly, on the task it aligned on:
 *   HAO_WLIST_PRIMARY / HAO_RESCUE_ANCHOR  the first-placement task (hao_window_ed_ref's), with the primary (err, pe);
 *   HAO_RESCUE_FWD                         the rescue task from the predecessor's y_end + 1 as the rescue left it;
 *   HAO_RESCUE_BWD                         the rescue task that ends at the successor's final y_start - 1.
 *   err == 0:  the traced function's shortcut (Levenshtein_distance.h:3783-3787): no sweep, y_start = y_end - (q_l - 1), one match run of q_l bases;
 *   err > 0:   ed_band_cal_semi_64_w_absent_diag_trace + gen_trace, then recal_boundary_exz (:2429-2468) where the alignment touches an end of the pattern: the
 *              re-placed task is swept too and taken iff it aligns with a strictly smaller err (HAO_RESCUE_REPLACED; its cigar replaces the first);
 *   a task outside HAO_ALIGN_SEMI's domain: nothing is guessed - the record keeps its distance-only err and y_end, y_start = the task's start, no cigar,
 *              HAO_WLIST_UNTRACED; a re-placement outside the domain is not made and the first trace stands.
 * Backward-rescued windows and anchors come out with the y_start, y_end, err and re-placed bit hao_fetch_rescue reports (they are traced again here from the
 * same tasks; the rescue stage and its records are unchanged).  Cigars are in push_trace's encoding and in the orientation of
 * hao_window_trace_batch(HAO_ALIGN_SEMI) for the same task, at most 2 * 31 + 3 entries plus the 0x3fff splits.
 *   hao_window_wlist_ref: blocking, over the batch hao_window_ed_ref and hao_window_rescue_ref have just processed (HAO_EINVAL without both, after another
 *                         window-alignment call or a new batch; HAO_EUNSUPP in a sharded engine).  out = window records, windows swept (err > 0, in the domain),
 *                         re-placement sweeps made, cigar entries, untraced windows.  The rescue results stay fetchable; a second call gives the same result.
 *   hao_fetch_wlist:      read rid's overlaps, aligned with hao_fetch_overlaps / hao_fetch_rescue: *n_ol of them, the records of overlap i at
 *                         wins[win_off[i] .. win_off[i + 1]) (counted from the read's first record), the cigar of record j at cigars[cig_off[j] .. cig_off[j + 1])
 *                         (counted from the read's first entry).  Pointers valid until the next call on the context.
 * HAO_DELIVER_WLIST in the parts of hao_overlap_batch_async runs the same stage inside the batch, after the rescue stage, and delivers after every other part:
 * n_ol + 1 record offsets, the records, n_wins + 1 entry offsets and the entries (each padded to 64 bytes in the arena).  Valid only together with
 * HAO_DELIVER_ED | HAO_DELIVER_RESCUE on a context configured by hao_deliver_ed_config_ref (else HAO_EINVAL); HAO_EUNSUPP in a sharded engine.  A batch without
 * the part keeps its arena layout and byte count.
 *   hao_deliver_wlist:    the view of a slot whose batch asked for the part, valid after hao_deliver_wait on that slot (HAO_EINVAL otherwise).
 *   hao_unpack_wlist:     read rid's lists out of the four views - win_off[0 .. n] counted from the read's first record, the records, cig_off[0 .. records]
 *                         counted from the read's first entry, the entries.  Returns the read's overlap count n; nothing is written when n exceeds cap_ovlp,
 *                         the records cap_wins, the entries cap_cigars, or an output pointer is NULL; 0 for a read outside the batch; UINT64_MAX for a NULL
 *                         view, a view that is not reference-placed, or views that do not belong together (overlap counts that differ, offsets that do not
 *                         ascend or run past their totals, a record whose window its overlap does not cover or that lies beyond read rid's grid as len has
 *                         it, a record in an overlap whose delivered verdict is 0, entry counts that do not add up).  Pure host code, any thread.
 * Not built: gen_extend_err_exz and everything after it in gen_hc_r_alin - its extension functions (Reserve_Banded_BPM_Extension[_REV]) are not reachable
 * through the reference harness, so nothing could hold them. */
typedef struct { int32_t y_start, y_end; uint32_t win, info; } hao_wlist_win_t;      /* info: err | thre << 8 | source << 16 | flags */
#define HAO_WLIST_PRIMARY 3u               /* source: a first-placement window the rescue did not trace (beside HAO_RESCUE_FWD / BWD / ANCHOR) */
#define HAO_WLIST_UNTRACED (1u << 19)      /* info: the task lies outside the traced domain: distance-only values, no cigar */
#define HAO_DELIVER_WLIST 64u      /* the window lists of the batch (with HAO_DELIVER_ED | HAO_DELIVER_RESCUE in reference placement; hao_deliver_wlist, hao_unpack_wlist) */
typedef struct {
	uint64_t n_ol, n_wins, n_cigar;              /* overlaps, window records and cigar entries of the batch */
	uint64_t n_swept, n_replace, n_untraced;     /* windows swept, re-placement sweeps made, untraced windows (hao_window_wlist_ref's out[1], out[2], out[4]) */
	const uint64_t *win_off;                     /* [n_ol + 1]: records of overlap i = wins[win_off[i] .. win_off[i + 1]) */
	const hao_wlist_win_t *wins;                 /* [n_wins] */
	const uint64_t *cig_off;                     /* [n_wins + 1]: entries of record j = cigars[cig_off[j] .. cig_off[j + 1]) */
	const uint16_t *cigars;                      /* [n_cigar] */
} hao_wlist_delivery_t;
int hao_window_wlist_ref(hao_ctx *c, uint64_t out[5]);
int hao_deliver_wlist(hao_ctx *c, int slot, hao_wlist_delivery_t *out);
uint64_t hao_unpack_wlist(const hao_delivery_t *d, const hao_ed_delivery_t *e, const hao_rescue_delivery_t *r, const hao_wlist_delivery_t *w, const uint32_t *len, uint64_t rid,
                          uint64_t *win_off, hao_wlist_win_t *wins, uint64_t *cig_off, uint16_t *cigars, uint64_t cap_ovlp, uint64_t cap_wins, uint64_t cap_cigars);
int hao_fetch_wlist(hao_ctx *c, uint64_t rid, uint64_t *n_ol, const uint64_t **win_off, const hao_wlist_win_t **wins, const uint64_t **cig_off, const uint16_t **cigars);
/* test support (host code, no context): the task of a rescue alignment as the kernel rebuilds it (window `win` of overlap z against the target from toff on;
 * tab = hao_ref_thresholds; 0: refused), so that the tests can hold the builder against work items recorded from the reference */
int hao_rescue_task(const hao_ovlp_t *z, uint32_t win, uint32_t window, int64_t toff, const uint8_t *tab, uint32_t target_len, hao_ed_task_t *out);

/* Second variant: global alignment inside the band WITH traceback - ed_band_cal_global_64_w_trace (Levenshtein_distance.h:3370-3442) on a
 * cleared bit_extz_t followed by gen_trace(ez, thre, 1) (:903-985), the call cal_exz_global / Correct.cpp:14537 make once a window's end points are fixed.
 * Same task records (abs_diag is ignored); both strings are consumed entirely, so |p_len - t_len| <= thre or there is no alignment.  Per task: err
 * (INT32_MAX = none within thre; then pe = te = -1 and no cigar), ps = ts = 0, pe = p_len - 1, te = t_len - 1, and the cigar in push_trace's encoding
 * (uint16: op << 14 | len; op 0 match, 1 mismatch, 2 more pattern, 3 more text) at cigars + i * cigar_cap; n_cigar entries exist, those past cigar_cap
 * are not written (an alignment within thre has at most 2 thre + 3 entries for strings shorter than 16 383: 257 for the widest band).  Band widths as for
 * hao_window_ed_batch (thre <= HAO_ED_MAX_THRE). */
typedef struct { int32_t err, ps, pe, ts, te, n_cigar; } hao_trace_result_t;
#define HAO_ALIGN_GLOBAL 0      /* ed_band_cal_global_64_w_trace */
#define HAO_ALIGN_EXT_FWD 1     /* ed_band_cal_extension_64_0_w_trace (:3512-3618): both strings start together, the alignment ends where the pattern or the text runs out (the
                                 * longer one is first cut to the other's length + thre): pe / te come out of the sweep.  Without an alignment: err INT32_MAX, pe = te = -1 */
#define HAO_ALIGN_EXT_BWD 2     /* ed_band_cal_extension_64_1_w_trace (:3620-3735): both strings END together; ps / ts come out (INT32_MAX without an alignment), pe = p_len - 1,
                                 * te = t_len - 1.  In both extension modes an alignment whose sweep was later abandoned (running error > 3 thre) keeps err and coordinates
                                 * but has no cigar (n_cigar = 0), as in the reference */
#define HAO_ALIGN_SEMI 3        /* ed_band_cal_semi_64_w_absent_diag_trace (Levenshtein_distance.h:3778-3848): the traced twin of hao_window_ed_batch - the text is consumed, the
                                 * pattern starts and ends inside the band: ps comes out of the walk, ts = 0, te = t_len - 1 (also without an alignment), abs_diag is used.
                                 * The band must cover the pattern: 0 <= p_len - t_len + abs_diag <= 2 thre and t_len > abs_diag (else HAO_EINVAL: the reference's
                                 * traceback would index its column words out of range).  (Numbering: the modes of Correct.cpp:14536-14545.) */
int hao_window_trace_batch(hao_ctx *c, int mode, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_trace_result_t *out, uint16_t *cigars, uint32_t cigar_cap);

/* Window alignment beyond 127 errors: the alignments of the stretches between anchored windows - cal_exz_infi (Correct.cpp:14508-14565) as hc_aln_exz (:14576-14636)
 * and hc_aln_exz_adv (:16082) call it, with patterns of up to MAX_SIN_L = 10000 bases and thresholds scaled up to MAX_SIN_E = 2047 (Levenshtein_distance.h:751-758),
 * i.e. the ed_band_cal_*_infi_* functions (:2134-3100) with nword = ceil((2 thre + 1) / 64) up to 64.  hao_window_ed_long is hao_window_ed_batch and
 * hao_window_trace_long is hao_window_trace_batch - same task and result records, modes and cigar encoding, same domain rules (p_len - t_len + abs_diag <= 64 nword
 * for the distance-only call, the band covering the pattern for HAO_ALIGN_SEMI), bit for bit the same results - for thre <= HAO_ED_LONG_MAX_THRE and
 * p_len, t_len <= HAO_ED_LONG_MAX_LEN (else HAO_EINVAL).  A call may mix all widths: pairs whose band fits four words run on hao_window_ed_batch's kernels, the others
 * on the cooperative kernel (hao_align_coop.cuh).  The traced call runs two sweeps; the second keeps 24 nword bytes per text column of the pairs that aligned (about
 * 21 MB for 64 words and 14 000 columns), in slices of at most ~4 GB.  Attached contexts and sharded engines (after hao_dist_gather_reads) as for the batch calls. */
#define HAO_ED_LONG_MAX_THRE 2047     /* the reference's MAX_SIN_E: 4095 diagonals in 64 words */
#define HAO_ED_LONG_MAX_LEN 16383     /* covers MAX_SIN_L + 2 MAX_SIN_E */
int hao_window_ed_long(hao_ctx *c, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_ed_result_t *out);
int hao_window_trace_long(hao_ctx *c, int mode, const hao_ed_task_t *tasks, uint64_t n_tasks, hao_trace_result_t *out, uint16_t *cigars, uint32_t cigar_cap);

/* The threshold ladder of hc_aln_exz (Correct.cpp:14576-14636) on the device: the caller of the long alignments.  A request names a stretch [qs, qe) of the
 * query read of overlap `ol` (index into the resident ol->list of the current batch, all reads of the batch counted through) and, for modes 0 - 2, a stretch
 * [ts, te) of its target; ts == te == -1 forces mode 3, as :14582 does.  Per request the stage makes up to four attempts (rungs) at growing thresholds -
 * scale_ed_thre(estimate_err), ql * e_rate, twice the second, ql * 0.51, each through scale_ed_thre(., maxe) and capped at ql = qe - qs, a rung skipped unless its
 * threshold exceeds the one before - and every attempt is one cal_exz_infi (:14508-14574): the coordinate step of the mode (3: update_semi_coord over the
 * overlap's resident fake cigar and init_waln; 1 / 2: adjust_ext_offset with the rung's threshold; 0: none), the test qe > qs && te > ts, and the traced
 * alignment of hao_window_trace_long in the band that threshold asks for.  The first rung whose alignment ends within its threshold is the result.  A request with
 * ql > maxl or estimate_err * 1.2 > maxe gets rung 0 without an attempt.  q_tot is the length of the overlap's query read, t_tot of its target.
 *   Result: rung (0: none), its threshold, the coordinates and aux_beg the aligner was given (rung 0: the request's own, ts = te = -1 in mode 3,
 *   thre = aux_beg = 0), the bit_extz_t fields of hao_trace_result_t (rung 0: err INT32_MAX, the others -1, no cigar), and flags over ALL attempts made:
 *     HAO_LADDER_REFUSED   an attempt's coordinate step left nothing to align (init_waln refused, or an empty interval): that attempt failed, as in the reference;
 *     HAO_LADDER_UNTRACED  a mode-3 attempt whose start resolves to no fake-cigar entry (the reference exits there) or whose band does not cover the pattern
 *                          (HAO_ALIGN_SEMI's domain: the reference's traceback would index its columns out of range): nothing is guessed, the attempt failed.
 *   Cigars in CSR form, push_trace's encoding: request i's entries at cigars[cig_off[i] .. cig_off[i + 1]).  out, cig_off (n + 1 entries) and *n_cigar (the
 *   entries of all requests) are always written; the entries only when *n_cigar <= cigar_cap - call again with that capacity otherwise.
 * On the device: one kernel computes every request's rungs; then at most four rounds of a coordinate-and-task kernel over the open requests, the traced sweeps by
 * band width (hao_al_kernel up to four words, hao_alc_kernel beyond) and a commit kernel that writes the results of the requests that aligned and compacts the
 * rest into the next round's list.  Only counters cross to the host between rounds.
 * Blocking; over the current batch (HAO_EINVAL without one).  Like every host-fed window-alignment call it takes the shared task scratch: fetch what
 * hao_window_ed_ref / hao_window_wlist_ref left before calling it.  Attached contexts and sharded engines (after hao_dist_gather_reads; HAO_EUNSUPP before) as for
 * the batch calls.  HAO_EINVAL: maxe > HAO_ED_LONG_MAX_THRE or negative, maxl negative, e_rate outside [0, 1], and any request with `ol` outside the batch, a mode outside 0 - 3,
 * estimate_err outside [0, 2^30), coordinates outside 0 <= qs <= qe <= q_tot or (modes 0 - 2; mode 3 does not read ts / te) 0 <= ts <= te <= t_tot, or - for a request that passes the maxl / maxe gate - ql or a
 * text length an attempt derives beyond HAO_ED_LONG_MAX_LEN.
 * Not built: adjust_specific_ext_offset (:14424; the caller passes the interval and the mode it wants), a streamed part.  (hc_aln_exz_adv: hao_window_ladder_adv, below.) */
typedef struct { uint32_t ol, mode; int32_t qs, qe, ts, te, estimate_err; uint32_t reserved; } hao_ladder_req_t;      /* 32 bytes */
typedef struct { uint32_t rung; int32_t thre, qs, qe, ts, te, aux_beg; uint32_t flags; int32_t err, a_ps, a_pe, a_ts, a_te, n_cigar; } hao_ladder_res_t;      /* 56 bytes */
#define HAO_LADDER_REFUSED 1u
#define HAO_LADDER_UNTRACED 2u
int hao_window_ladder(hao_ctx *c, const hao_ladder_req_t *req, uint64_t n_req, double e_rate, int64_t maxl, int64_t maxe,
                      hao_ladder_res_t *out, uint64_t *cig_off, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar);
/* The cigar entries of the last hao_window_ladder call on this context, which stay resident until its next call (HAO_EINVAL before the first and after one that
 * failed): *n_cigar = their number, the entries into cigars when they fit cigar_cap - so a caller that does not know the capacity runs the stage once, not
 * twice - and rounds[j] = the requests that were open in round j (n_cigar, cigars and rounds may be NULL). */
int hao_fetch_ladder(hao_ctx *c, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar, uint64_t rounds[4]);
/* TEST SUPPORT, not part of the stable interface (it may change or go with the kernel it mirrors): host code, no context - the rungs of one request as the
 * kernel computes them, thre[4] (-1 where the rung is skipped or the gate is shut); returns the number of attempts */
int hao_ladder_thresholds(int64_t ql, int64_t estimate_err, double e_rate, int64_t maxl, int64_t maxe, int32_t thre[4]);

/* The threshold ladder of hc_aln_exz_adv (Correct.cpp:16082-16165) on the device: hc_aln_exz's sibling, which the read-overlap path runs (chain_aln and sub_base_aln under
 * gen_hc_fast_cigar, with MAX_SIN_L / MAX_SIN_E / FORCE_SIN_L for maxl / maxe / force_l).  Same request record, same rounds and sweeps as hao_window_ladder; the rules that differ:
 *   entry      ts == te == -1 forces mode 3; ql == 0 && te - ts == 0 returns 1 with nothing aligned; ql <= 0 || te - ts <= 0 returns 0 - both on the request's own ts / te, so a
 *              forced mode 3 and an extension whose far end is unset (te <= ts) never reach the aligner, an explicit mode 3 with ts < te does;
 *   estimate   estimate_err < 0 stands for (int64)(ql * e_rate) when ql <= wl, and for cal_estimate_err(z, wl, qs, qe, e_rate) (:15369-15401) over the overlap's window list
 *              when ql > wl: the records hao_window_wlist_ref left on the device for this batch, when wl is the window length they were built on (see below);
 *   shortcut   ql <= 16: cal_exact_exz (:15725-15767) - the target interval of the mode (3: hao_ref_shift over the resident fake cigar; 1: te = ts + ql; 2: ts = te - ql), clamped
 *              into [0, t_tot]; success when it has ql bases equal to the query's (strand y_pos_strand; an N equals an N only, as in the strings the reference compares): err 0, one
 *              entry (0, ql).  It comes before the gate and does not depend on it;
 *   gate       ql <= maxl && (estimate_err >> 1) <= maxe;
 *   rungs      the four recipes of hc_aln_exz WITHOUT the cap at ql, rungs 2 - 4 skipped unless larger than the threshold computed before, and a fifth, thre = maxe, when
 *              ql <= force_l;
 *   attempt    cal_exz_infi_adv (:15617-15672): the coordinate step runs with min(thre, dd), dd = max(ql, te - ts) of the request; after the test the threshold becomes
 *              min(thre, max of the NEW lengths); the attempt is abandoned (HAO_LADDER_REPEAT) unless that exceeds the threshold of the request's last attempt that got this
 *              far; else the traced alignment runs in the band of that threshold;
 *   result     absolute coordinates: a_ps, a_pe += ts and a_ts, a_te += qs of the attempt.
 * Result: done = the function's return value; rung 0 none, 1 - 5 the attempt that aligned, HAO_LADDER_RUNG_EXACT the shortcut; thre = the clamped threshold the aligner was given
 * (0 for rung 0 and the shortcut); qs .. aux_beg = what the aligner (or the shortcut's comparison) was given, the request's own for rung 0 (ts = te = -1 in forced mode 3); flags
 * over all attempts; err .. n_cigar as in hao_window_ladder (rung 0: INT32_MAX, -1, no cigar), a_* absolute.  A HAO_LADDER_UNTRACED attempt counts as failed where the
 * reference would have aligned (or exited), and one whose band does not cover the pattern has still set the last threshold tried: a request that carries that flag can therefore
 * show HAO_LADDER_REPEAT and end on a later rung or on rung 0 where the reference would not - its result is the project's, not the reference's.  Cigars, capacity, residency, blocking, the shared task scratch,
 * attached contexts and sharded engines: as for hao_window_ladder.  On the device: the set-up kernel, an exact-match kernel over the requests with ql <= 16 (those it settles
 * never enter the rounds), then at most five rounds of hao_window_ladder's machinery under this rule set.
 * HAO_EINVAL: maxe > HAO_ED_LONG_MAX_THRE or negative, maxl, wl or force_l negative, e_rate outside [0, 1], and any request with `ol` outside the batch, a mode outside 0 - 3,
 * estimate_err >= 2^30, qs / qe outside 0 <= qs <= qe <= q_tot, or - past the two early returns - ts / te outside 0 <= ts < te <= t_tot (every mode: mode 3 reads te - ts),
 * estimate_err < 0 with ql > wl when no window lists of that window length are on the device for the batch or when the lists give a negative value (a stretch that ends before
 * the overlap starts: the reference would carry the negative number through scale_ed_thre's uint32 cast; nothing is guessed), or - past the gate - ql or a length an attempt can
 * derive beyond HAO_ED_LONG_MAX_LEN.
 * The window lists: the blocking chain hao_window_ed_ref -> hao_window_rescue_ref -> hao_window_wlist_ref leaves the batch's records on the device, and they stay there for this
 * call and hao_window_estimate_err - across any number of ladder calls and other host-fed window-alignment calls, which take the shared task scratch (and with it what
 * hao_fetch_wlist serves) but not the records - until a new batch, a chain stage that runs again (then until the chain has completed again) or hao_window_ed_grid.  The lists
 * of a batch delivered with HAO_DELIVER_WLIST live in its output set, not here: such a batch has none (HAO_EINVAL as above), nor has a sharded engine that could not run the
 * chain.  The estimate is the reference's function on align_hc_ed_post_extz's list; the reference calls it after gen_extend_err_exz has been over the list, which is not built.
 * Not built: adjust_specific_ext_offset, a streamed part, gen_extend_err_exz. */
typedef struct { int32_t done; uint32_t rung; int32_t thre, qs, qe, ts, te, aux_beg; uint32_t flags; int32_t err, a_ps, a_pe, a_ts, a_te, n_cigar; } hao_ladder_adv_res_t;      /* 60 bytes */
#define HAO_LADDER_REPEAT 4u          /* an attempt was abandoned because its clamped threshold did not exceed the last one tried (the pthre test) */
#define HAO_LADDER_RUNG_EXACT 6u
int hao_window_ladder_adv(hao_ctx *c, const hao_ladder_req_t *req, uint64_t n_req, double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l,
                          hao_ladder_adv_res_t *out, uint64_t *cig_off, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar);
/* hao_fetch_ladder for the last hao_window_ladder_adv call (each fetch serves its own call only: HAO_EINVAL after the other one); rounds[j]: the open requests of round j of five */
int hao_fetch_ladder_adv(hao_ctx *c, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar, uint64_t rounds[5]);
/* TEST SUPPORT, like hao_ladder_thresholds: the five raw rungs of hc_aln_exz_adv for one request (-1: skipped, or the gate is shut); estimate_err < 0 is replaced as above
 * (with ql > wl: HAO_EINVAL, a negative return).  *gate (may be NULL) = the gate is open; returns the number of attempts */
int hao_ladder_adv_thresholds(int64_t ql, int64_t estimate_err, double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l, int32_t thre[5], int32_t *gate);
/* The estimates the last hao_window_ladder_adv call on this context ran with, one per request: the request's own where it was >= 0, (int64)(ql * e_rate) or the window lists'
 * value where it was < 0, -1 behind an early return.  Resident like the call's cigars; writes min(cap, requests) entries into est (may be NULL) and returns the call's number of
 * requests, or (uint64_t)HAO_EINVAL under hao_fetch_ladder_adv's conditions (no such call, one that failed, or hao_window_ladder since). */
uint64_t hao_fetch_ladder_adv_estimates(hao_ctx *c, int64_t *est, uint64_t cap);
/* cal_estimate_err (Correct.cpp:15369-15401) as a stage of its own over the window lists the blocking chain left on the device for the current batch (above): est[i] = the
 * function's value for request i's ol, qs, qe (nothing else of the request is read), as it is - a negative one included.  Blocking; one kernel, a thread per request.  It
 * takes no shared scratch and changes nothing another window-alignment call left resident: every fetch call serves afterwards what it served before.
 * HAO_EINVAL: no batch, no lists on the device for it, wl other than the window length they were built on, e_rate outside [0, 1], a request with `ol` outside the batch or
 * qs / qe outside 0 <= qs <= qe <= q_tot.  n_req == 0: HAO_OK. */
int hao_window_estimate_err(hao_ctx *c, const hao_ladder_req_t *req, uint64_t n_req, double e_rate, int64_t wl, int64_t *est);
/* TEST SUPPORT, not part of the stable interface, like hao_ladder_adv_thresholds: host code, no context - the function the two calls above run on the device, over the n records
 * of one overlap z as hao_fetch_wlist hands them out (ascending windows) */
int64_t hao_estimate_err_records(const hao_ovlp_t *z, const hao_wlist_win_t *wins, uint64_t n, int64_t wl, int64_t qs, int64_t qe, double e_rate);

/* f3 with traceback on the device grid: the semi-global traced alignment (HAO_ALIGN_SEMI: ed_band_cal_semi_64_w_absent_diag_trace + gen_trace, the call
 * Correct.cpp:3897-3911 makes right after the distance-only one) of the grid pairs hao_window_ed_grid(window, thre) forms, in the same text order.  A pair is
 * TRACED iff its distance-only result aligned (err <= thre) and its band covers the pattern (0 <= p_len - t_len + abs_diag <= 2 thre, t_len > abs_diag: the
 * domain hao_window_trace_batch accepts for HAO_ALIGN_SEMI).  A traced pair's (err, pe) is the distance-only result and (ps, ts = 0, te = t_len - 1, cigar)
 * is what hao_window_trace_batch(HAO_ALIGN_SEMI) gives for the same task; an aligned pair outside the domain (clipped at a read end) keeps its distance-only
 * (err, pe) with ps = -1 and no cigar (ALIGNED BUT UNTRACED); a pair without an alignment reads err = INT32_MAX, pe = ps = -1.  ts = 0 and te = t_len - 1 for
 * every pair.  A cigar has at most 2 thre + 3 entries (push_trace's encoding, op << 14 | len).  Not covered: reference placement (diagonal pairs only), the other
 * traced modes (host-fed: hao_window_trace_batch), the sharded path (HAO_EUNSUPP).  On the device, the traced sweep keeps three words per band word and text
 * column (D0, VP, VN; the walk derives HP / HN) in slices of ~4 GB, and the cigars are compacted into one array.
 *   hao_window_trace_grid: over the last batch (hao_overlap_batch[_ex]; results resident).  out[0] = grid pairs, out[1] = traced pairs, out[2] = cigar entries,
 *                          out[3] = aligned but untraced pairs.  thre > HAO_ED_MAX_THRE, window == 0 or window + 2 thre >= 65535: HAO_EINVAL.  Its results stay
 *                          resident until the next batch or hao_window_ed_batch / hao_window_trace_batch call.
 *   hao_fetch_trace_grid:  the first min(cap_pairs, out[0]) pairs: tasks (rebuilt from the pair list), results, cig_off[0 .. m] (offsets into cigars; untraced
 *                          pairs have empty ranges) and the cigar entries of those pairs, the first cap_cigars of them.  Any pointer may be NULL.
 * HAO_DELIVER_TRACE in the parts of hao_overlap_batch_async (only with HAO_DELIVER_ED, else HAO_EINVAL) runs the same stage on the pairs and error bytes of
 * the ED stage (hao_deliver_ed_config's window and threshold) and delivers, after the ED records: per read a uint64 offset of its first cigar entry, per pair a
 * uint16 ps (0xffff: none) and a uint16 entry count, and the entries in pair order.  Batches without the part keep their arena layout and byte count.
 *   hao_deliver_trace:     the view of a slot whose batch asked for HAO_DELIVER_TRACE, valid after hao_deliver_wait on that slot (HAO_EINVAL otherwise); its
 *                          pointers live in the slot's pinned arena.
 *   hao_unpack_trace:      read rid's pairs as hao_unpack_ed rebuilds them, their results (hao_fetch_trace_grid's values), per-pair offsets cig_off[0 .. n]
 *                          into the read's cigar entries and those entries.  Returns the pair count; nothing is written when it exceeds cap_pairs, the read's
 *                          entries exceed cap_cigars, or tasks / res / cig_off / cigars is NULL; 0 for a read outside the batch; UINT64_MAX when the rebuilt
 *                          pairs or the entry counts do not match the delivered ones (len is not the batch's).  A pure function of the three views. */
int hao_window_trace_grid(hao_ctx *c, uint32_t window, uint32_t thre, uint64_t out[4]);
int hao_fetch_trace_grid(hao_ctx *c, hao_ed_task_t *tasks, hao_trace_result_t *res, uint64_t *cig_off, uint16_t *cigars, uint64_t cap_pairs, uint64_t cap_cigars);
#define HAO_DELIVER_TRACE 16u      /* traceback of the batch's aligned grid pairs (with HAO_DELIVER_ED; hao_deliver_trace, hao_unpack_trace) */
typedef struct {
	uint64_t n_traced, n_cigar;  /* traced pairs and cigar entries of the batch */
	const uint64_t *cg_off;      /* [n_reads + 1]: cigar entries of read r = [cg_off[r], cg_off[r + 1]) */
	const uint16_t *ps;          /* [n_pairs] (the ED view's pairs): start of the alignment on the pattern, 0xffff = no cigar */
	const uint16_t *n_cig;       /* [n_pairs]: cigar entries of the pair */
	const uint16_t *cigar;       /* [n_cigar]: the entries, pair after pair */
} hao_trace_delivery_t;
int hao_deliver_trace(hao_ctx *c, int slot, hao_trace_delivery_t *out);
uint64_t hao_unpack_trace(const hao_trace_delivery_t *t, const hao_ed_delivery_t *e, const hao_delivery_t *d, const uint32_t *len, uint64_t rid,
                          hao_ed_task_t *tasks, hao_trace_result_t *res, uint64_t *cig_off, uint16_t *cigars, uint64_t cap_pairs, uint64_t cap_cigars);

/* On-disk formats: the filter table, the position index and the read store in the reference's own resume format, so a GPU-built
 * index can be handed to a stock hifiasm (load_pt_index, htab.cpp:1432-1550, called from Assembly.cpp:2078):
 *   <prefix>.pt_flt  (write_pt_index, htab.cpp:1367-1430),  <prefix>.pt_flt.bin  (write_All_reads, Process_Read.cpp:69-125 - the layout of *.ec.bin),
 *   <prefix>.pt_flt.paf.bin  (empty overlap lists).
 * names[i] = read names or NULL ("r<i>"); number_of_round must equal the loader's -r (default 3: it exits otherwise, htab.cpp:1501-1505).
 * Needs hao_ft_gen + hao_pt_gen (or a loaded index).
 *   On a sharded engine the call is a COLLECTIVE: every rank calls it, rank 0 writes the three files - from its replicated filter table and position index,
 *   the gathered read store and the replicated lengths - and they are byte for byte what one unsharded engine over all reads writes (global read ids in the
 *   position lists, N sites, names, peaks, max_n_chain).  `names` is read on rank 0 only and is indexed by GLOBAL read id; the other ranks may pass NULL.
 *   The ranks exchange a status before a file is created and after rank 0 has closed the last one, and every rank returns the same code (the ranks fail
 *   together): a peer's HAO_OK says the files are complete.  Without a valid gathered store (hao_dist_gather_reads): HAO_EUNSUPP on every rank, no file. */
int hao_index_save(hao_ctx *c, const char *prefix, int32_t number_of_round, const char *const *names);
/* The reader of the same files = load_pt_index (htab.cpp:1432-1550) for the engine: an index written by a stock hifiasm (write_pt_index) or by
 * hao_index_save becomes the engine's read store (replaces hao_set_reads), filter table and position index (replace hao_ft_gen / hao_pt_gen), with the
 * file's hom_cov / het_cov / max_n_chain; *number_of_round = the value stored in the file.  The read-ordered minimizers of the query side are
 * sketched here with the loaded filter table (the reference re-sketches every query read).  The file's k must equal the engine's; w, HPC and the
 * other options are the caller's to match, as with the reference.  Histograms are not in the file: hao_hist returns zeros afterwards.
 * A load that fails leaves the engine without an index.
 *   hao_index_load_dist loads into a SHARDED engine (after hao_dist_init / hao_dist_init_loopback; a collective, every rank calls it and reads the files
 *   itself: a shared file system).  first_rid[world + 1], the same on every rank: rank r is to own the reads [first_rid[r], first_rid[r + 1]); it must ascend
 *   from 0 to the file's read count (HAO_EINVAL otherwise); NULL: near-equal read counts, rank r owns [n r / world, n (r + 1) / world).  A rank reads the table
 *   file, the read store's header, every read's N-site count and length, and - by seeking - the N sites and packed bases of its own slice only.  Afterwards the
 *   engine is what hao_set_reads (the slice), hao_set_shard (the slice's first read, the file's lengths), hao_ft_gen and hao_pt_gen on the same cut leave:
 *   filter table, position index, peaks and max_n_chain replicated, the query side built for the local reads without communication; a gathered store from
 *   before the load is discarded, and hao_dist_gather_reads and every stage behind it run as after a build.  The ranks exchange a status after parsing and
 *   after installing: a file that one rank cannot read or that is damaged, or an invalid first_rid, is the same error on every rank, and nobody waits.
 *   On an unsharded engine the call is hao_index_load (first_rid: NULL or { 0, read count }); hao_index_load on a sharded engine is this call with NULL. */
int hao_index_load(hao_ctx *c, const char *prefix, int32_t *number_of_round);
int hao_index_load_dist(hao_ctx *c, const char *prefix, const uint64_t *first_rid /* world + 1 entries, rank order; NULL: equal read counts */, int32_t *number_of_round);
/* The engine's current read layout (after hao_set_reads / hao_set_shard or a load): local reads, global id of the first, reads of all ranks, and the engine's
 * own copy of all lengths (valid until the reads change); any pointer may be NULL. */
int hao_shard_layout(hao_ctx *c, uint64_t *n_reads, uint64_t *rid_base, uint64_t *n_total, const uint32_t **all_len);

/* <prefix>.ovlp.source.bin / .ovlp.reverse.bin (write_ma_hit_ts / load_ma_hit_ts, Overlaps.cpp:23328-23469): the per-read lists of ma_hit_t the reference builds from the
 * overlap regions AFTER alignment and correction (not a product of this path: the engine serves h_ec_lchain, the reference's own code fills and writes these lists - the
 * drop-in run's files are byte-identical, tests/test_gpu_dropin.py).  Reader and writer of the format, for tools on either side of the path: a record is the field-by-field
 * image write_ma produces (42 bytes: qns u64, qe tn ts te u32, el no_l_indel u8, ml rev bl del as u32 each - the bit fields widened), a read contributes
 * (is_fully_corrected u8, is_abnormal u8, length u32, its records), the file starts with the read count as int64.  Host code, no device, no context.
 *   hao_ovlp_bin_read: *flags = 2 bytes per read, *off = n_reads + 1 record offsets, *hits = the records; all three malloc'ed (free() them); HAO_EINVAL on a damaged file
 *   hao_ovlp_bin_write: the inverse; the output of a read is byte-identical to what was read */
typedef struct { uint64_t qns; uint32_t qe, tn, ts, te; uint32_t ml, rev, bl, del; uint8_t el, no_l_indel, pad[6]; } hao_ma_hit_t;      /* 48 bytes in memory */
int hao_ovlp_bin_read(const char *path, uint64_t *n_reads, uint8_t **flags, uint64_t **off, hao_ma_hit_t **hits);
int hao_ovlp_bin_write(const char *path, uint64_t n_reads, const uint8_t *flags, const uint64_t *off, const hao_ma_hit_t *hits);

/* Per-read digests of the last batch's results, computed on the device (one workgroup per read) and copied to out[n] / out_kh[n]
 * (n = reads of the batch; out_kh may be NULL):
 *   out[r]    = sum of term(1, i, w) over the 64-bit words of ol->list (6 per overlap_region: the 12 u32 fields of hao_ovlp_t)
 *             + sum of term(2, i, w) over the read's fake cigars in ol order + sum of term(3, i, w) over cl->list (2 words per k_mer_hit)
 *   out_kh[r] = sum of term(4, i, w) over the seed hits before chaining (hao_fetch_seed_hits)
 *   term(s, i, w) = mix64(w + 0x9E3779B97F4A7C15 * (i + 1) + s * 0xD6E8FEB86659FD93)  mod 2^64,  mix64 = splitmix64's finaliser.
 * An end-to-end integrity check for consumers on the far side of the PCIe boundary, and the way the full-size parity tests compare
 * EVERY read of a 500 000-read pass with the reference (oracle/ref_harness.cpp --digest computes the same value from the reference's
 * own overlap_region / Candidates_list after h_ec_lchain, anchor.cpp:2302). */
int hao_batch_digest(hao_ctx *c, uint64_t *out, uint64_t *out_kh);
/* The same out[r] for every read of a DELIVERED batch (needs HAO_DELIVER_OL | HAO_DELIVER_CL), computed on the host from what landed in the pinned arena:
 * ol->list, the fake cigars, and cl->list decoded out of the wire format by hao_unpack_hits.  A pure function of the view (any thread, while the slot is
 * not being rewritten); the reads are spread over n_threads host threads.  What crossed PCIe can thus be compared, read by read, with the device's own
 * digest or with the reference's (tests/test_gpu_fullgold.py does it for all 500 000 reads of configs[2]; bench.py for the batches it delivers). */
int hao_delivery_digest(const hao_delivery_t *d, uint64_t *out, int n_threads);

/* Device self-test of the record grouping used by the sharded index build (pins a rocPRIM bit-range sort behaviour, see hao_capi_rest.hpp):
 * out[0] = order violations of the begin_bit = 48 sort, out[1] = of the path the engine uses (must be 0). */
int hao_selftest_rocprim(uint64_t n, uint64_t out[2]);
/* Self-test of the code paths that handle more than 2^32 items (grid-stride launches, run-length encoding through reduce_by_key): n u32 keys i / 8;
 * out = { runs, sum of run lengths, runs of a length other than 8 } - n / 8, n, 0 for n a multiple of 8 (tests/test_gpu_rocprim.py). */
int hao_selftest_big(uint64_t n, uint64_t out[3]);

/* Self-test of the index sort on 40 of the 64 hash bits + fix-up of the runs that hold several keys (hao_index.cuh; what hao_pt_gen runs on more than 2^23
 * minimizers): n synthetic keys with many such runs, sorted that way and by the stable 64-bit sort; out = { positions where the two results differ (must
 * be 0), runs the fix-up rewrote (must be > 0 for the test to mean anything), scratch elements used, scratch overflow flag }. */
int hao_selftest_sortbits(hao_ctx *c, uint64_t n, uint64_t out[4]);

/* HAO_DBG_*: debug entry - the selection's sorts alone, on given keys (hao_sortdbg.hpp; tests/test_gpu_sortperm.py).  The order of ol->list depends on the tie order
 * of klib's introsort (ksort.h:110-160), which the device replays three ways; this entry runs one of them on n_arr key arrays given as a CSR (off[0] = 0, off[n_arr]
 * keys in xs / sc) and returns, for array a, perm[off[a] + i] = index within the array of the key at slot i.  mode 0 sorts by sc descending (oreg_ss_lt, anchor.cpp:35),
 * mode 1 by xs = x_pos_s << 32 | x_pos_e ascending (oreg_xs_lt, anchor.cpp:32).  The paths call the device functions the selection calls:
 *   HAO_SORTDBG_SEQ          hao_intro_sort on one lane, keys in global memory;
 *   HAO_SORTDBG_WAVE_LDS     hao_wave_intro_sort, keys in the LDS of chain_select_kernel<1, 128> (variant 0, arrays of at most 128 keys) or <1, 1024> (variant 1, 1024);
 *   HAO_SORTDBG_WAVE_GLOBAL  hao_wave_intro_sort, keys and work arrays in global scratch as the selection lays them out for reads beyond every LDS tier;
 *   HAO_SORTDBG_BLOCK        hao_block_intro_sort on four waves in the LDS of chain_select4_kernel, the tier chosen by the array's length as the selection chooses it
 *                            (arrays below the first four-wave tier run in its slice); at most 4096 keys;
 *   HAO_SORTDBG_SELECT       mode 1 only: the selection's own launches over one synthetic read per array, without pruning and without the weak-chain filter.
 * variant is 0 except where named.  Offsets that do not ascend, an array longer than the path holds, mode 0 with HAO_SORTDBG_SELECT: HAO_EINVAL; a sort whose
 * level list would overflow: HAO_EUNSUPP (as in a batch). */
#define HAO_SORTDBG_SEQ 0
#define HAO_SORTDBG_WAVE_LDS 1
#define HAO_SORTDBG_WAVE_GLOBAL 2
#define HAO_SORTDBG_BLOCK 3
#define HAO_SORTDBG_SELECT 4
int hao_dbg_sort_perm(hao_ctx *c, int mode, int path, int variant, uint64_t n_arr, const uint64_t *off, const uint64_t *xs, const int32_t *sc, uint32_t *perm);

/* per-stage device time of the last call in milliseconds (HIP events on the engine's stream);
 * names[i] points to static strings. Returns the number of stages. */
int hao_stage_times(hao_ctx *c, const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif
