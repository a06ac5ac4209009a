// remaining C ABI entry points
#pragma once

#include <atomic>
#include <new>
#include <stdexcept>
#include <thread>
extern "C" {

int hao_ft_gen(hao_ctx *c, int32_t *hom_cov)
{
	if (!c) return HAO_EINVAL;
	HAO_NOT_ON_VIEW(c, "hao_ft_gen"); ++c->index_gen;
	HIP_TRY(hipSetDevice(c->device));
	c->timer.begin(c->stream);
	int rc = hao_ft_run(c);
	if (rc != HAO_OK) return rc;
	c->timer.mark("ft_release");      // (hao_ft_run's buffers are gone: host_ft_release = what freeing them took)
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->timer.collect(c->stage_ms);
	if (hom_cov) *hom_cov = c->ft_peak_hom;
	return HAO_OK;
}

int32_t hao_ft_cnt(hao_ctx *c, uint64_t y)
{
	if (!c || !c->has_ft) return 0;
	int64_t i = hao_bsearch(c->h_ft_keys.data(), c->h_ft_keys.size(), y);
	return i < 0 ? 0 : c->h_ft_vals[i];
}

int hao_ft_table(hao_ctx *c, uint64_t *n, const uint64_t **keys, const int32_t **vals)
{
	if (!c || !c->has_ft) return HAO_EINVAL;
	*n = c->h_ft_keys.size(); *keys = c->h_ft_keys.data(); *vals = c->h_ft_vals.data();
	return HAO_OK;
}

int hao_hist(hao_ctx *c, int which, int64_t cnt[4096])
{
	if (!c) return HAO_EINVAL;
	memcpy(cnt, which == 0 ? c->ft_hist : c->pt_hist, sizeof(int64_t) * HAO_N_COUNTS);
	return HAO_OK;
}

int hao_stats(hao_ctx *c, int64_t out[8])
{
	if (!c) return HAO_EINVAL;
	uint32_t h, l; hao_occ_thresholds(c->hom_cov, &h, &l);
	out[0] = c->ft_peak_hom; out[1] = c->ft_peak_het; out[2] = c->ft_cutoff; out[3] = c->max_n_chain;
	out[4] = c->hom_cov; out[5] = c->het_cov; out[6] = h; out[7] = l;
	return HAO_OK;
}

int hao_ft_passes(hao_ctx *c) { return c ? c->ft_passes_used : HAO_EINVAL; }

int hao_pt_gen(hao_ctx *c, int32_t *hom_cov, int32_t *het_cov)
{
	if (!c) return HAO_EINVAL;
	HAO_NOT_ON_VIEW(c, "hao_pt_gen"); ++c->index_gen;
	HIP_TRY(hipSetDevice(c->device));
	c->timer.begin(c->stream);
	int rc = hao_pt_run(c);
	if (rc != HAO_OK) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->timer.collect(c->stage_ms);
	if (hom_cov) *hom_cov = c->hom_cov;
	if (het_cov) *het_cov = c->het_cov;
	return HAO_OK;
}

int hao_pt_get(hao_ctx *c, uint64_t hash, const uint64_t **pos, int32_t *n)
{
	if (!c || !c->has_pt) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_pt_download(c)) return rc;
	int64_t i = hao_bsearch(c->h_ix_keys.data(), c->h_ix_keys.size(), hash);
	if (i < 0) { *pos = nullptr; *n = 0; return HAO_OK; }
	*pos = c->h_ix_pos.data() + c->h_ix_off[i]; *n = (int32_t)(c->h_ix_off[i + 1] - c->h_ix_off[i]);
	return HAO_OK;
}

int hao_pass_default(hao_ctx *c, hao_pass_t *p)
{
	if (!c || !p) return HAO_EINVAL;
	if (int rc = hao_view_refresh(c)) return rc;
	memset(p, 0, sizeof(*p));
	p->bw_thres = c->opt.is_ont ? 0.05 : 0.02; p->max_n_chain = c->max_n_chain;
	hao_occ_thresholds(c->hom_cov, &p->high_occ, &p->low_occ);
	p->apend_be = 1; p->is_accurate = 1; p->gen_off = 1; p->mcopy_num = 3; p->mcopy_rate = 0.7; p->chain_cutoff = 2; p->mcopy_khit_cut = 32; p->ocv_w = 3072;
	return HAO_OK;
}

int hao_overlap_batch(hao_ctx *c, uint64_t rid_lo, uint64_t rid_hi)
{
	hao_pass_t ps;
	if (int rc = hao_pass_default(c, &ps)) return rc;
	return hao_overlap_batch_ex(c, rid_lo, rid_hi, &ps);
}

int hao_overlap_batch_ex(hao_ctx *c, uint64_t rid_lo, uint64_t rid_hi, const hao_pass_t *pass)
{
	if (c) { if (int rc = hao_view_refresh(c)) return rc; }
	if (!c || !pass || rid_lo > rid_hi || rid_hi > c->n_reads) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	c->timer.begin(c->stream);
	int rc = hao_overlap_run(c, rid_lo, rid_hi, *pass);
	if (rc != HAO_OK) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	c->timer.collect(c->stage_ms);
	return HAO_OK;
}

int hao_overlap_batch_async(hao_ctx *c, uint64_t rid_lo, uint64_t rid_hi, const hao_pass_t *pass, uint32_t parts, int *slot)
{
	if (c) { if (int rc = hao_view_refresh(c)) return rc; }
	if (!c || rid_lo > rid_hi || rid_hi > c->n_reads || !(parts & (HAO_DELIVER_OL | HAO_DELIVER_CL | HAO_DELIVER_EXACT))) return HAO_EINVAL;
	if (parts & HAO_DELIVER_ED) {
		{ HAO_STAGE_VIEW(c, V, "HAO_DELIVER_ED needs the bases of both reads"); (void)V; }
		if (!(parts & HAO_DELIVER_OL)) { hao_set_err(c, "HAO_DELIVER_ED needs HAO_DELIVER_OL: the decoder rebuilds the pairs from the delivered overlaps"); return HAO_EINVAL; }
		if (!c->ded_window) { hao_set_err(c, "HAO_DELIVER_ED before hao_deliver_ed_config"); return HAO_EINVAL; }
	}
	if ((parts & HAO_DELIVER_TRACE) && (parts & HAO_DELIVER_ED) && c->ded_place == HAO_PLACE_REF) { hao_set_err(c, "HAO_DELIVER_TRACE: the traced grid stage is not built in reference placement (hao_deliver_ed_config_ref)"); return HAO_EUNSUPP; }
	if (parts & HAO_DELIVER_RESCUE) {
		{ HAO_STAGE_VIEW(c, V, "HAO_DELIVER_RESCUE needs the bases of both reads"); (void)V; }
		if (!(parts & HAO_DELIVER_ED)) { hao_set_err(c, "HAO_DELIVER_RESCUE needs HAO_DELIVER_ED: it rescues the windows the ED stage left open"); return HAO_EINVAL; }
		if (c->ded_place != HAO_PLACE_REF) { hao_set_err(c, "HAO_DELIVER_RESCUE needs reference placement (hao_deliver_ed_config_ref)"); return HAO_EINVAL; }
	}
	if (parts & HAO_DELIVER_WLIST) {
		{ HAO_STAGE_VIEW(c, V, "HAO_DELIVER_WLIST needs the bases of both reads"); (void)V; }
		if (!(parts & HAO_DELIVER_ED) || !(parts & HAO_DELIVER_RESCUE)) { hao_set_err(c, "HAO_DELIVER_WLIST needs HAO_DELIVER_ED | HAO_DELIVER_RESCUE: it traces the windows those stages aligned"); return HAO_EINVAL; }
		if (c->ded_place != HAO_PLACE_REF) { hao_set_err(c, "HAO_DELIVER_WLIST needs reference placement (hao_deliver_ed_config_ref)"); return HAO_EINVAL; }
	}
	if ((parts & HAO_DELIVER_TRACE) && !(parts & HAO_DELIVER_ED)) { hao_set_err(c, "HAO_DELIVER_TRACE needs HAO_DELIVER_ED: it traces the pairs the ED stage aligned"); return HAO_EINVAL; }
	hao_pass_t ps;
	if (!pass) { if (int rc = hao_pass_default(c, &ps)) return rc; pass = &ps; }
	HIP_TRY(hipSetDevice(c->device));
	c->timer.begin(c->stream);
	int rc = hao_overlap_run(c, rid_lo, rid_hi, *pass, parts, slot);
	if (rc != HAO_OK) return rc;
	if (parts & HAO_DELIVER_ED) HIP_TRY(hipStreamSynchronize(c->stream));      // (the ED stage's kernels run after the read-back of the totals: they too are done when the call returns)
	c->timer.collect(c->stage_ms);      // (the batch's kernels are complete: hao_overlap_run ends with the read-back of its totals; only the copy is still running)
	return HAO_OK;
}

int hao_deliver_wait(hao_ctx *c, int slot, hao_delivery_t *out)
{
	if (!c || !out || slot < 0 || slot > 1 || !c->batch || !c->batch->dl_ready) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	hao_ctx::Batch::Slot &S = c->batch->slot[slot];
	if (S.pending) { HIP_TRY(hipEventSynchronize(S.ev_done)); S.pending = false; float ms = 0; if (hipEventElapsedTime(&ms, S.ev_ready, S.ev_done) == hipSuccess) S.dl.copy_ms = ms;
		// the rate of the copy itself: a big batch that crossed at less than 40 GB/s (a good arena gives 50 - 56 beside the next batch's kernels) gets its arena allocated again
		// before the slot's next batch, with a timed copy into every NUMA node (batches of 256 MB and more: smaller ones pay per-copy overheads that say nothing about the arena) (once per slot; round 6 saw arenas that passed the probe at allocation and then copied at 30 GB/s for the whole run)
		float cms = 0; const double mb_ = (double)S.dl.bytes / 1e6;
		if (hipEventElapsedTime(&cms, S.ev_cstart, S.ev_done) == hipSuccess && cms > 0 && S.arena_retry < 1 && ((mb_ >= 256.0 && mb_ / cms < 40.0) || (c->sw.arena_probe && mb_ > 0))) {
			S.arena_bad = true; ++S.arena_retry;
			fprintf(stderr, "[hao] delivery arena %d: a batch of %.0f MB was copied at %.1f GB/s; the arena is allocated again for the slot's next batch, every NUMA node tried\n", slot, mb_, mb_ / cms);
		}
	}
	if (S.dl.n_ol && S.dl.fc_off) ((uint64_t*)S.dl.fc_off)[S.dl.n_ol] = S.dl.n_fc;      // end of the last cigar: a host-side word next to the region the copy wrote, set once the copy has landed
	*out = S.dl;
	return HAO_OK;
}

// pure function of a delivered view (any thread): the wire bytes of read rid back into k_mer_hits (hao_deliver.cuh describes the format)
uint64_t hao_unpack_hits(const hao_delivery_t *d, uint64_t rid, hao_hit_t *out, uint64_t cap)
{
	if (!d || rid < d->rid_lo || rid >= d->rid_lo + d->n_reads || !d->cl_off) return 0;
	const uint64_t r = rid - d->rid_lo, h0 = d->cl_off[r], nh = d->cl_off[r + 1] - h0;
	if (nh > cap || !out) return nh;
	const hao_qmz_t *qt = d->qmz ? d->qmz + d->qm_off[r] : nullptr;
	const uint16_t *qp16 = d->qmz ? nullptr : d->qmz_pos + d->qm_off[r]; const uint16_t *qc8 = d->qmz ? nullptr : d->qmz_cnt + d->qm_off[r];      // (the packed tables)
	auto q_self = [&](uint32_t q_) -> uint32_t { return qt ? qt[q_].self_offset : (uint32_t)qp16[q_]; };
	auto q_cnt = [&](uint32_t q_) -> uint32_t { return qt ? qt[q_].cnt : (uint32_t)qc8[q_]; };
	uint64_t k = 0;
	for (uint64_t ci = d->ch_off[r]; ci < d->ch_off[r + 1]; ++ci) {
		const hao_chain_hdr_t &H = d->chains[ci];
		uint32_t q = H.q0, off = H.offset;
		const uint64_t g = H.pos;      // position of the chain's first hit; the code bytes of its later hits start at rank(g + 1) (the byte at g itself, if any, is not the chain's)
		uint64_t cp = 0;
		if (H.n_hits > 1) {      // the directory has an entry per 256 positions: + the bits of the words between it and the position
			const uint64_t wp = (g + 1) >> 6;
			cp = d->cl_rank[wp >> 2];
			for (uint64_t w = wp & ~3ULL; w < wp; ++w) cp += (uint64_t)__builtin_popcountll(d->cl_bits[w]);
			cp += (uint64_t)__builtin_popcountll(d->cl_bits[wp] & ((1ULL << ((g + 1) & 63)) - 1));
		}
		for (uint32_t i = 0; i < H.n_hits; ++i) {
			hao_hit_t &o = out[k + i];
			if (i) {
				const uint64_t gi = g + i; uint8_t w = 0x08;      // no code byte: the read's next minimizer, same diagonal
				if (d->cl_bits[gi >> 6] >> (gi & 63) & 1) w = d->cl_codes[cp++];
				if (w == 0xff) {      // verbatim: binary search of the position in the sorted exception list
					uint64_t lo = 0, hi = d->n_exc;
					while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (d->cl_exc[m].index < gi) lo = m + 1; else hi = m; }
					o = d->cl_exc[lo].hit; o.w0 = H.w0; q = d->cl_exc[lo].q; off = o.offset;
					continue;
				}
				const uint32_t qn = q + (w >> 4) + 1; off = (uint32_t)((int64_t)off + (int64_t)(q_self(qn) - q_self(q)) + (int64_t)(w & 15) - 8); q = qn;
			}
			o.w0 = H.w0; o.offset = off; o.self_offset = q_self(q); o.cnt = q_cnt(q);
		}
		k += H.n_hits;
	}
	return k;
}

// ol->list of a delivered read back into hao_ovlp_t records (the wire drops x_id, x_pos_strand and align_length: the read, 0 and 0 - hao_ol_wire_kernel)
uint64_t hao_unpack_overlaps(const hao_delivery_t *d, uint64_t rid, hao_ovlp_t *out, uint64_t cap)
{
	if (!d || rid < d->rid_lo || rid >= d->rid_lo + d->n_reads || !d->ol_off || !d->ol) return 0;
	const uint64_t r = rid - d->rid_lo, o0 = d->ol_off[r], n = d->ol_off[r + 1] - o0;
	if (n > cap || !out) return n;
	for (uint64_t i = 0; i < n; ++i) {
		const hao_ovlp_wire_t &w = d->ol[o0 + i]; hao_ovlp_t &o = out[i];
		o.x_id = (uint32_t)rid; o.x_pos_s = w.x_pos_s; o.x_pos_e = w.x_pos_e; o.x_pos_strand = 0;
		o.y_id = w.y & 0x7fffffffu; o.y_pos_s = w.y_pos_s; o.y_pos_e = w.y_pos_e; o.y_pos_strand = w.y >> 31;
		o.shared_seed = w.shared_seed; o.align_length = 0; o.non_homopolymer_errors = w.non_homopolymer_errors; o.fc_len = w.fc_len;
	}
	return n;
}

// the fake cigar of delivered overlap j back into 8-byte entries (hao_deliver.cuh: "fake cigars on the wire")
uint32_t hao_unpack_cigar(const hao_delivery_t *d, uint64_t j, uint64_t *out, uint32_t cap)
{
	if (!d || !d->ol || !d->fc_off || j >= d->n_ol) return 0;
	const uint32_t fl = d->ol[j].fc_len;
	if (fl > cap || !out || fl == 0) return fl;
	const uint64_t o = d->fc_off[j]; const uint32_t *w = d->fc + (o & ~HAO_FC_RAW);
	if (o & HAO_FC_RAW) { for (uint32_t k = 0; k < fl; ++k) out[k] = (uint64_t)w[2 * k + 1] << 32 | w[2 * k]; return fl; }
	uint32_t site = d->ol[j].x_pos_s; int64_t sh = 0;
	out[0] = (uint64_t)site << 32;
	for (uint32_t k = 1; k < fl; ++k) {
		const uint32_t x = w[k - 1], z = x >> 20;
		site += x & 0xfffffu; sh += (int64_t)(z >> 1) ^ -(int64_t)(z & 1);
		out[k] = (uint64_t)site << 32 | (sh < 0 ? ((uint32_t)(-sh) << 1 | 1u) : (uint32_t)sh << 1);
	}
	return fl;
}

// hao_batch_digest's value for every read of a DELIVERED batch, computed on the host from the bytes in the pinned arena: ol->list, the fake cigars and
// cl->list decoded out of the wire format by hao_unpack_hits.  A pure function of the view; the reads are spread over n_threads host threads.
int hao_delivery_digest(const hao_delivery_t *d, uint64_t *out, int n_threads)
{
	if (!d || (!out && d->n_reads)) return HAO_EINVAL;
	if (d->n_reads && (!d->ol_off || !d->cl_off)) return HAO_EINVAL;      // needs HAO_DELIVER_OL | HAO_DELIVER_CL
	const uint64_t n = d->n_reads;
	if (n_threads < 1) n_threads = 1;
	if ((uint64_t)n_threads > n) n_threads = (int)std::max<uint64_t>(1, n);
	std::atomic<uint64_t> next(0); std::atomic<int> bad(0);
	auto work = [&]() {
		std::vector<hao_hit_t> buf; std::vector<uint64_t> fcb; std::vector<hao_ovlp_t> olb;
		for (;;) {
			const uint64_t b0 = next.fetch_add(64); if (b0 >= n) break;
			for (uint64_t r = b0; r < std::min(n, b0 + 64); ++r) {
				const uint64_t o0 = d->ol_off[r], o1 = d->ol_off[r + 1], nh = d->cl_off[r + 1] - d->cl_off[r];
				if (buf.size() < nh) buf.resize(nh + nh / 4 + 64);
				if (hao_unpack_hits(d, d->rid_lo + r, buf.data(), nh) != nh) { bad = 1; out[r] = 0; continue; }
				if (olb.size() < o1 - o0) olb.resize(o1 - o0 + 64);
				if (hao_unpack_overlaps(d, d->rid_lo + r, olb.data(), o1 - o0) != o1 - o0) { bad = 1; out[r] = 0; continue; }
				uint64_t s = 0; const uint64_t *w = (const uint64_t*)olb.data();
				for (uint64_t i = 0; i < (o1 - o0) * 6; ++i) s += hao_dg_term(1, i, w[i]);
				{	uint64_t fi = 0;      // the fake cigars of the read's overlaps, entry by entry, through the decoder
					for (uint64_t j = o0; j < o1; ++j) {
						const uint32_t fl = d->ol[j].fc_len; if (fcb.size() < fl) fcb.resize(fl);
						if (hao_unpack_cigar(d, j, fcb.data(), fl) != fl) bad = 1;
						for (uint32_t k = 0; k < fl; ++k) s += hao_dg_term(2, fi++, fcb[k]);
					} }
				w = (const uint64_t*)buf.data();
				for (uint64_t i = 0; i < nh * 2; ++i) s += hao_dg_term(3, i, w[i]);
				out[r] = s;
			}
		}
	};
	std::vector<std::thread> th;
	for (int t = 1; t < n_threads; ++t) th.emplace_back(work);
	work();
	for (auto &t : th) t.join();
	return bad ? HAO_EINVAL : HAO_OK;
}

int hao_index_save(hao_ctx *c, const char *prefix, int32_t number_of_round, const char *const *names)
{
	if (!c || !prefix) return HAO_EINVAL;
	HAO_NOT_ON_VIEW(c, "hao_index_save");
	HIP_TRY(hipSetDevice(c->device));
	return hao_index_save_impl(c, prefix, number_of_round, names);
}

int hao_next_slot(hao_ctx *c, int *slot)
{
	if (!c || !slot) return HAO_EINVAL;
	*slot = c->batch ? (int)(c->batch->dl_seq & 1) : 0;
	return HAO_OK;
}

int hao_index_load_dist(hao_ctx *c, const char *prefix, const uint64_t *first_rid, int32_t *number_of_round)
{
	if (!c || !prefix) return HAO_EINVAL;
	HAO_NOT_ON_VIEW(c, "hao_index_load");
	HIP_TRY(hipSetDevice(c->device));
	return hao_index_load_impl(c, prefix, first_rid, number_of_round);      // (its local phases turn their exceptions into codes: none crosses the C boundary or leaves a peer waiting)
}

int hao_index_load(hao_ctx *c, const char *prefix, int32_t *number_of_round) { return hao_index_load_dist(c, prefix, nullptr, number_of_round); }

int hao_shard_layout(hao_ctx *c, uint64_t *n_reads, uint64_t *rid_base, uint64_t *n_total, const uint32_t **all_len)
{
	if (!c) return HAO_EINVAL;
	if (int rc = hao_view_refresh(c)) return rc;
	if (n_reads) *n_reads = c->n_reads;
	if (rid_base) *rid_base = c->rid_base;
	if (n_total) *n_total = c->n_total;
	if (all_len) *all_len = c->h_len_all.data();
	return HAO_OK;
}

int hao_exact_check(hao_ctx *c)
{
	if (!c || !c->batch || !c->batch->valid) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_exact_run(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HAO_OK;
}

int hao_window_ed_grid(hao_ctx *c, uint32_t window, uint32_t thre, uint64_t *n_tasks)
{
	if (!c || !n_tasks || !c->batch || !c->batch->valid) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_ed_grid_run(c, window, thre, n_tasks)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HAO_OK;
}

int hao_fetch_ed_grid(hao_ctx *c, hao_ed_task_t *tasks, hao_ed_result_t *res, uint64_t cap)
{
	if (!c) return HAO_EINVAL;
	if (!c->batch || !c->batch->valid || (c->win.scratch_pairs() == 0 && cap)) { hao_set_err(c, "hao_fetch_ed_grid: no pairs of hao_window_ed_grid are resident (a new batch or another window-alignment call has reused the scratch)"); return HAO_EINVAL; }
	HIP_TRY(hipSetDevice(c->device));
	const uint64_t n = std::min<uint64_t>(cap, c->win.scratch_pairs());
	if (n && tasks) HIP_TRY(hipMemcpyAsync(tasks, c->al_task.p, n * sizeof(hao_ed_task_t), hipMemcpyDeviceToHost, c->stream));
	if (n && res) HIP_TRY(hipMemcpyAsync(res, c->al_res.p, n * sizeof(hao_ed_result_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HAO_OK;
}

int hao_window_trace_grid(hao_ctx *c, uint32_t window, uint32_t thre, uint64_t out[4])
{
	if (!c || !out) return HAO_EINVAL;
	const int rc = hao_window_stage(c, nullptr, [&] { return hao_trace_grid_run(c, window, thre, out); });      // (hao_stage_times: ed_grid, ed_align, trace_sel, trace_align)
	if (!rc) hao_release_above(c->tg.path, HAO_SCRATCH_KEEP);      // (between blocking calls)
	return rc;
}

int hao_fetch_trace_grid(hao_ctx *c, hao_ed_task_t *tasks, hao_trace_result_t *res, uint64_t *cig_off, uint16_t *cigars, uint64_t cap_pairs, uint64_t cap_cigars)
{
	if (!c) return HAO_EINVAL;
	if (!c->batch || !c->batch->valid || !c->win.trace_resident()) { hao_set_err(c, "hao_fetch_trace_grid: no results of hao_window_trace_grid are resident (a new batch or another window-alignment call has reused the scratch)"); return HAO_EINVAL; }
	if (c->tg_n == 0) { if (cig_off) cig_off[0] = 0; return HAO_OK; }      // (an empty grid: nothing resident to read)
	HIP_TRY(hipSetDevice(c->device));
	const uint64_t n = std::min<uint64_t>(cap_pairs, c->tg_n);
	DevBuf<hao_ed_task_t> dt; DevBuf<hao_trace_result_t> dr; DevBuf<uint64_t> doff;
	auto done = [&](int rc) { HIP_TRY(hipStreamSynchronize(c->stream)); return rc; };
	if (n && (tasks || res)) {
		HIP_TRY(dt.reserve(n)); HIP_TRY(dr.reserve(n));
		if (int rc = hao_al_trace_grid_expand(c, c->batch->O().ol_out.p, n, dt.p, dr.p)) return done(rc);
		if (tasks) HIP_TRY(hipMemcpyAsync(tasks, dt.p, n * sizeof(hao_ed_task_t), hipMemcpyDeviceToHost, c->stream));
		if (res) HIP_TRY(hipMemcpyAsync(res, dr.p, n * sizeof(hao_trace_result_t), hipMemcpyDeviceToHost, c->stream));
	}
	uint64_t end = 0;      // cigar entries of the first n pairs
	HIP_TRY(doff.reserve(n + 2));
	if (int rc = hao_al_trace_grid_off(c, nullptr, n, c->tg_nsel, doff.p)) return done(rc);
	HIP_TRY(hipMemcpyAsync(&end, doff.p + n, 8, hipMemcpyDeviceToHost, c->stream));
	if (cig_off) HIP_TRY(hipMemcpyAsync(cig_off, doff.p, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint64_t nc = std::min<uint64_t>(end, cap_cigars);
	if (cigars && nc) HIP_TRY(hipMemcpyAsync(cigars, c->tg_cig.p, nc * 2, hipMemcpyDeviceToHost, c->stream));
	return done(HAO_OK);
}

// The view of one more part of a waited-for slot: the one body of hao_deliver_ed, hao_deliver_trace, hao_deliver_rescue and hao_deliver_wlist
// (this and the next are templates: C++ linkage inside this file's extern "C")
extern "C++" {
template <class V> static int hao_deliver_part(hao_ctx *c, int slot, V *out, V hao_ctx::Batch::Slot::*view, uint32_t part, const char *fn, const char *flag)
{
	if (!c || !out || slot < 0 || slot > 1 || !c->batch || !c->batch->dl_ready) return HAO_EINVAL;
	const hao_ctx::Batch::Slot &S = c->batch->slot[slot];
	if (!(S.parts & part)) { hao_set_err(c, std::string(fn) + ": the slot's batch did not ask for " + flag); return HAO_EINVAL; }
	if (S.pending) { hao_set_err(c, std::string(fn) + ": hao_deliver_wait has not been called on the slot"); return HAO_EINVAL; }
	*out = S.*view;
	return HAO_OK;
}
// The front hao_unpack_wlist and hao_unpack_rescue share (part_ok: the part's own view checks; win_off / wins / n_wins: its records by overlap): read rid's overlaps [*o0, *o0 + n) and their records lie
// inside the part, every record in a window its overlap covers, in ascending window order, inside the read's grid.  Returns n; 0: a read outside the batch or without overlaps; UINT64_MAX: malformed views.
template <class W> static uint64_t hao_unpack_records_ok(const hao_delivery_t *d, const hao_ed_delivery_t *e, const uint32_t *len, uint64_t rid, bool part_ok, uint64_t part_n_ol,
		const uint64_t *win_off, const W *wins, uint64_t n_wins, uint64_t *o0_out)
{
	if (rid < d->rid_lo || rid >= d->rid_lo + d->n_reads) return 0;
	if (!e->window || e->placement != HAO_PLACE_REF || !d->ol_off || !d->ol || part_n_ol != d->n_ol || !part_ok) return UINT64_MAX;
	const uint64_t q = rid - d->rid_lo, o0 = d->ol_off[q], o1 = d->ol_off[q + 1];
	if (o0 > o1 || o1 > part_n_ol) return UINT64_MAX;
	const uint64_t n = o1 - o0;
	if (n == 0) return 0;
	const uint64_t w1 = win_off[o1];
	if (win_off[o0] > w1 || w1 > n_wins) return UINT64_MAX;
	std::vector<hao_ovlp_t> zs(n);
	if (hao_unpack_overlaps(d, rid, zs.data(), n) != n) return UINT64_MAX;
	const uint32_t wl = e->window; const uint64_t nwin = ((uint64_t)len[rid] + wl - 1) / wl;
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t a = win_off[o0 + i], b = win_off[o0 + i + 1];
		if (a > b || b > w1) return UINT64_MAX;
		for (uint64_t k = a; k < b; ++k) {
			const uint32_t x = wins[k].win;
			if (x < zs[i].x_pos_s / wl || x > zs[i].x_pos_e / wl || x >= nwin || (k > a && wins[k - 1].win >= x)) return UINT64_MAX;
		}
	}
	*o0_out = o0;
	return n;
}
}

int hao_deliver_trace(hao_ctx *c, int slot, hao_trace_delivery_t *out) { return hao_deliver_part(c, slot, out, &hao_ctx::Batch::Slot::tr, HAO_DELIVER_TRACE, "hao_deliver_trace", "HAO_DELIVER_TRACE"); }

// pure function of the three views of a delivered batch: read rid's pairs and distance-only results as hao_unpack_ed gives them, with the traced part added
uint64_t hao_unpack_trace(const hao_trace_delivery_t *t, const hao_ed_delivery_t *e, const hao_delivery_t *d, const uint32_t *len, uint64_t rid,
		hao_ed_task_t *tasks, hao_trace_result_t *res, uint64_t *cig_off, uint16_t *cigars, uint64_t cap_pairs, uint64_t cap_cigars)
{
	if (!t || !e || !d || !len || !t->cg_off || !e->window || e->placement != HAO_PLACE_DIAG || !e->ed_off || rid < d->rid_lo || rid >= d->rid_lo + d->n_reads) return 0;
	const uint64_t r = rid - d->rid_lo, p0 = e->ed_off[r], np = e->ed_off[r + 1] - p0, c0 = t->cg_off[r], nc = t->cg_off[r + 1] - c0;
	if (np > cap_pairs || nc > cap_cigars || !tasks || !res || !cig_off || !cigars) return np;
	std::vector<hao_ed_result_t> er(np);
	const uint64_t k = hao_unpack_ed(e, d, len, rid, tasks, er.data(), np);
	if (k != np) return UINT64_MAX;
	uint64_t o = 0;
	for (uint64_t i = 0; i < np; ++i) {
		const uint16_t ps = t->ps[p0 + i], m = t->n_cig[p0 + i];
		hao_trace_result_t &x = res[i];
		x.err = er[i].err; x.pe = er[i].pe; x.ps = ps == 0xffff ? -1 : (int32_t)ps; x.ts = 0; x.te = (int32_t)tasks[i].t_len - 1; x.n_cigar = m;
		cig_off[i] = o; o += m;
	}
	cig_off[np] = o;
	if (o != nc) return UINT64_MAX;
	if (nc) memcpy(cigars, t->cigar + c0, nc * 2);
	return np;
}

int hao_deliver_ed_config(hao_ctx *c, uint32_t window, uint32_t thre)
{
	if (!c) return HAO_EINVAL;
	if (window == 0 || thre > HAO_ED_MAX_THRE || (uint64_t)window + 2 * (uint64_t)thre >= 0xffff) { hao_set_err(c, "hao_deliver_ed_config: window length 0, threshold beyond the widest band, or window + 2 thre beyond 16 bits"); return HAO_EINVAL; }
	c->ded_window = window; c->ded_thre = thre; c->ded_place = HAO_PLACE_DIAG; c->ded_erate = 0;
	return HAO_OK;
}

int hao_deliver_ed_config_ref(hao_ctx *c, uint32_t window, double e_rate)
{
	if (!c) return HAO_EINVAL;
	if (!hao_ed_ref_args_ok(window, e_rate)) { hao_set_err(c, "hao_deliver_ed_config_ref: window length 0, window + 62 beyond 16 bits, or e_rate outside (0, 1)"); return HAO_EINVAL; }
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(hipStreamSynchronize(c->stream));      // (a batch of this context may still read the previous table)
	if (int rc = hao_ed_ref_upload(c, window, e_rate, c->ded_tab)) return rc;
	uint8_t full = 0; { std::vector<uint8_t> h((size_t)window + 1); hao_ref_thre_table(window, e_rate, h.data()); full = h[window]; }
	c->ded_window = window; c->ded_thre = full; c->ded_place = HAO_PLACE_REF; c->ded_erate = e_rate;
	return HAO_OK;
}

void hao_ref_thresholds(uint32_t window, double e_rate, uint8_t *out) { if (out) hao_ref_thre_table(window, e_rate, out); }

int hao_window_ed_ref(hao_ctx *c, uint32_t window, double e_rate, uint64_t *n_tasks, uint64_t *unresolved)
{
	if (!c || !n_tasks) return HAO_EINVAL;
	return hao_window_stage(c, "ed_ref", [&] { return hao_ed_ref_run(c, window, e_rate, n_tasks, unresolved); });
}

int hao_fetch_ed_ovlp(hao_ctx *c, uint64_t rid, const hao_ed_ovlp_t **summary, uint64_t *n)
{
	if (!c || !summary || !n) return HAO_EINVAL;
	if (!c->batch || !c->batch->valid || !c->win.ed_resident()) { hao_set_err(c, "hao_fetch_ed_ovlp: no summaries of hao_window_ed_ref are resident (a new batch has run since)"); return HAO_EINVAL; }
	hao_ctx::Batch &B = *c->batch;
	if (rid < B.lo || rid >= B.lo + B.n) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_batch_download(c)) return rc;
	if (!c->win.host_current(WinResident::ED)) {
		c->rf_hsum.assign(B.n_ol + 1, hao_ed_ovlp_sum{0, 0, 0, 0});
		if (B.n_ol) HIP_TRY(hipMemcpy(c->rf_hsum.data(), c->rf_sum.p, B.n_ol * sizeof(hao_ed_ovlp_sum), hipMemcpyDeviceToHost));
		c->win.on_host_copy(WinResident::ED);
	}
	const uint64_t r = rid - B.lo, s_ = B.h_fin_off[r], e_ = B.h_fin_off[r + 1];
	*summary = (const hao_ed_ovlp_t*)(c->rf_hsum.data() + s_); *n = e_ - s_;
	return HAO_OK;
}

int hao_window_rescue_ref(hao_ctx *c, uint64_t *n_rescued)
{
	if (!c || !n_rescued) return HAO_EINVAL;
	return hao_window_stage(c, "rescue_ref", [&] { return hao_rescue_ref_run(c, n_rescued); });
}

int hao_fetch_rescue(hao_ctx *c, uint64_t rid, const hao_rescue_ovlp_t **ovlp, uint64_t *n, const uint64_t **win_off, const hao_rescue_win_t **wins)
{
	if (!c || !ovlp || !n || !win_off || !wins) return HAO_EINVAL;
	if (!c->batch || !c->batch->valid || !c->win.rescue_resident()) { hao_set_err(c, "hao_fetch_rescue: no results of hao_window_rescue_ref are resident (a new batch has run since)"); return HAO_EINVAL; }
	hao_ctx::Batch &B = *c->batch;
	if (rid < B.lo || rid >= B.lo + B.n) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_batch_download(c)) return rc;
	hao_ctx::Rescue &G = c->rs;
	if (!c->win.host_current(WinResident::RESCUE)) {      // the whole batch once: the per-overlap results, the record offsets per overlap and the records, as the stage left them
		const uint64_t m = B.n_ol;
		G.h_ovlp.assign(m + 1, hao_rs_ovlp{0, 0, 0, 0, 0}); G.h_win_off.assign(m + 1, 0); G.h_wins.assign(c->rs_nw + 1, hao_rs_win{0, 0, 0, 0});      // (never empty: the pointers handed out are valid)
		if (m) {
			HIP_TRY(hipMemcpy(G.h_ovlp.data(), G.ovlp.p, m * sizeof(hao_rs_ovlp), hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(G.h_win_off.data(), G.off.p, (m + 1) * 8, hipMemcpyDeviceToHost));
			if (c->rs_nw) HIP_TRY(hipMemcpy(G.h_wins.data(), G.wins.p, c->rs_nw * sizeof(hao_rs_win), hipMemcpyDeviceToHost));
		}
		c->win.on_host_copy(WinResident::RESCUE);
	}
	const uint64_t r = rid - B.lo, s_ = B.h_fin_off[r], e_ = B.h_fin_off[r + 1];
	*ovlp = (const hao_rescue_ovlp_t*)(G.h_ovlp.data() + s_); *n = e_ - s_;
	*win_off = G.h_win_off.data() + s_; *wins = (const hao_rescue_win_t*)G.h_wins.data();
	return HAO_OK;
}

int hao_window_wlist_ref(hao_ctx *c, uint64_t out[5])
{
	if (!c || !out) return HAO_EINVAL;
	return hao_window_stage(c, "wlist_ref", [&] { return hao_wlist_ref_run(c, out); });
}

int hao_fetch_wlist(hao_ctx *c, uint64_t rid, uint64_t *n_ol, const uint64_t **win_off, const hao_wlist_win_t **wins, const uint64_t **cig_off, const uint16_t **cigars)
{
	if (!c || !n_ol || !win_off || !wins || !cig_off || !cigars) return HAO_EINVAL;
	if (!c->batch || !c->batch->valid || !c->win.wlist_resident()) { hao_set_err(c, "hao_fetch_wlist: no results of hao_window_wlist_ref are resident (a new batch or another window-alignment stage has run since)"); return HAO_EINVAL; }
	hao_ctx::Batch &B = *c->batch;
	if (rid < B.lo || rid >= B.lo + B.n) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_batch_download(c)) return rc;
	hao_ctx::Wlist &G = c->wl;
	if (!c->win.host_current(WinResident::WLIST)) {      // the whole batch once
		const uint64_t m = B.n_ol, N = c->wl_out[0], E = c->wl_out[3];
		G.h_woff.assign(m + 1, 0); G.h_wins.assign(N + 1, hao_rs_win{0, 0, 0, 0}); G.h_cig_off.assign(N + 1, 0); G.h_cig.assign(E + 1, 0);
		if (N) {
			HIP_TRY(hipMemcpy(G.h_woff.data(), G.woff.p, (m + 1) * 8, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(G.h_wins.data(), G.wins.p, N * sizeof(hao_rs_win), hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(G.h_cig_off.data(), G.cig_off.p, (N + 1) * 8, hipMemcpyDeviceToHost));
			if (E) HIP_TRY(hipMemcpy(G.h_cig.data(), G.cig.p, E * 2, hipMemcpyDeviceToHost));
		}
		c->win.on_host_copy(WinResident::WLIST);
	}
	const uint64_t r = rid - B.lo, s_ = B.h_fin_off[r], e_ = B.h_fin_off[r + 1], n = e_ - s_, g0 = G.h_woff[s_], g1 = G.h_woff[e_];
	G.r_woff.resize(n + 1); G.r_cig_off.resize(g1 - g0 + 1);
	for (uint64_t i = 0; i <= n; ++i) G.r_woff[i] = G.h_woff[s_ + i] - g0;
	for (uint64_t g = g0; g <= g1; ++g) G.r_cig_off[g - g0] = G.h_cig_off[g] - G.h_cig_off[g0];
	*n_ol = n; *win_off = G.r_woff.data(); *wins = (const hao_wlist_win_t*)(G.h_wins.data() + g0); *cig_off = G.r_cig_off.data(); *cigars = G.h_cig.data() + G.h_cig_off[g0];
	return HAO_OK;
}

// the threshold ladder (hao_ladder.cuh, hao_f3.hip): requests up, the stage over the batch's final ol->list and fake cigars, results / offsets / entries down.
// adv: hao_window_ladder_adv (out: hao_ladder_adv_res_t records); else hao_window_ladder (out: hao_ladder_res_t records; wl and force_l unused)
static int hao_ladder_run(hao_ctx *c, bool adv, const hao_ladder_req_t *req, uint64_t n, double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l, void *out, uint64_t *cig_off, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar)
{
	const std::string who = adv ? "hao_window_ladder_adv" : "hao_window_ladder";
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::OutSet &O = B.O(); hao_ctx::Ladder &G = c->ld;
	*n_cigar = 0; c->ld_valid = false; c->ld_adv = adv; c->ld_ncig = 0; c->ld_n = 0; for (int j = 0; j < 5; ++j) c->ld_rounds[j] = 0;
	if (adv) { HAO_STAGE_VIEW(c, V, "hao_window_ladder_adv needs the bases of both reads"); (void)V; }
	else { HAO_STAGE_VIEW(c, V, "hao_window_ladder needs the bases of both reads"); (void)V; }
	if (!(e_rate >= 0 && e_rate <= 1) || maxl < 0 || maxe < 0 || maxe > HAO_ED_LONG_MAX_THRE || wl < 0 || force_l < 0) { hao_set_err(c, who + ": e_rate outside [0, 1], maxl" + (adv ? ", wl or force_l" : "") + " negative, or maxe negative or beyond HAO_ED_LONG_MAX_THRE"); return HAO_EINVAL; }
	if (n >= (1ULL << 32)) { hao_set_err(c, who + ": more than 2^32 requests in one call"); return HAO_EUNSUPP; }
	c->win.on_host_fed();      // (the task / result scratch is shared with the other window-alignment calls; the batch's window records stay: hao_ld_run reads them)
	if (n == 0) { cig_off[0] = 0; c->ld_valid = true; return HAO_OK; }
	HIP_TRY(G.req.reserve(n));
	HIP_TRY(hipMemcpyAsync(G.req.p, req, n * sizeof(hao_ladder_req_t), hipMemcpyHostToDevice, c->stream));
	if (int rc = adv ? hao_al_ladder_adv(c, O.ol_out.p, B.n_ol, O.fc_out.p, O.fc_out_off.p, n, e_rate, wl, maxl, maxe, force_l, n_cigar, c->ld_rounds)
	                 : hao_al_ladder(c, O.ol_out.p, B.n_ol, O.fc_out.p, O.fc_out_off.p, n, e_rate, maxl, maxe, n_cigar, c->ld_rounds)) return rc;
	if (adv) HIP_TRY(hipMemcpyAsync(out, G.res_adv.p, n * sizeof(hao_ladder_adv_res_t), hipMemcpyDeviceToHost, c->stream));
	else HIP_TRY(hipMemcpyAsync(out, G.res.p, n * sizeof(hao_ladder_res_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(cig_off, G.off.p, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
	if (*n_cigar && *n_cigar <= cigar_cap) HIP_TRY(hipMemcpyAsync(cigars, G.cig.p, *n_cigar * 2, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	hao_release_above(c->al_path, HAO_SCRATCH_KEEP);      // (the buffers that grow with the requests alone - requests, results, lists, offsets - keep their largest size, like every per-item buffer of the context)
	for (int j = 0; j < 5; ++j) hao_release_above(G.rows[j], HAO_SCRATCH_KEEP);
	c->ld_ncig = *n_cigar; c->ld_n = n; c->ld_valid = true;
	return HAO_OK;
}

// the resident entries and the per-round open counts of the last ladder call, which must have been the one this fetch belongs to (n_rounds: 4, or 5 for the adv call)
static int hao_fetch_ladder_of(hao_ctx *c, bool adv, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar, uint64_t *rounds, int n_rounds)
{
	if (!c) return HAO_EINVAL;
	const std::string who = adv ? "hao_fetch_ladder_adv" : "hao_fetch_ladder";
	if (!c->ld_valid || c->ld_adv != adv) { hao_set_err(c, who + ": no results of " + (adv ? "hao_window_ladder_adv" : "hao_window_ladder") + " are resident"); return HAO_EINVAL; }
	if (n_cigar) *n_cigar = c->ld_ncig;
	if (rounds) for (int j = 0; j < n_rounds; ++j) rounds[j] = c->ld_rounds[j];
	if (cigars && c->ld_ncig && c->ld_ncig <= cigar_cap) { HIP_TRY(hipSetDevice(c->device)); HIP_TRY(hipMemcpy(cigars, c->ld.cig.p, c->ld_ncig * 2, hipMemcpyDeviceToHost)); }
	return HAO_OK;
}
int hao_fetch_ladder(hao_ctx *c, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar, uint64_t rounds[4]) { return hao_fetch_ladder_of(c, false, cigars, cigar_cap, n_cigar, rounds, 4); }
int hao_fetch_ladder_adv(hao_ctx *c, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar, uint64_t rounds[5]) { return hao_fetch_ladder_of(c, true, cigars, cigar_cap, n_cigar, rounds, 5); }

uint64_t hao_fetch_ladder_adv_estimates(hao_ctx *c, int64_t *est, uint64_t cap)
{
	if (!c) return (uint64_t)(int64_t)HAO_EINVAL;
	if (!c->ld_valid || !c->ld_adv) { hao_set_err(c, "hao_fetch_ladder_adv_estimates: no results of hao_window_ladder_adv are resident"); return (uint64_t)(int64_t)HAO_EINVAL; }
	const uint64_t m = std::min<uint64_t>(cap, c->ld_n);
	if (est && m) {
		if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(est, c->ld.est.p, m * 8, hipMemcpyDeviceToHost) != hipSuccess) { hao_set_err(c, "hao_fetch_ladder_adv_estimates: the copy failed"); return (uint64_t)(int64_t)HAO_ENODEV; }
	}
	return c->ld_n;
}

// hao_window_estimate_err: cal_estimate_err over the batch's resident window lists, one value per request; its own buffers, no transition of c->win
static int hao_estimate_run(hao_ctx *c, const hao_ladder_req_t *req, uint64_t n, double e_rate, int64_t wl, int64_t *est)
{
	hao_ctx::Batch &B = *c->batch;
	if (!c->win.wlist_records_resident()) { hao_set_err(c, "hao_window_estimate_err: no window lists of hao_window_wlist_ref are on the device for this batch (the blocking chain has not completed on it, or a grid call has run since)"); return HAO_EINVAL; }
	if (wl <= 0 || wl != (int64_t)c->rf_tab_wl) { hao_set_err(c, "hao_window_estimate_err: wl is not the window length the lists were built on"); return HAO_EINVAL; }
	if (!(e_rate >= 0 && e_rate <= 1)) { hao_set_err(c, "hao_window_estimate_err: e_rate outside [0, 1]"); return HAO_EINVAL; }
	{ HAO_STAGE_VIEW(c, V, "hao_window_estimate_err needs the read lengths as the window stages see them"); (void)V; }      // (the gathered store has gone since hao_window_wlist_ref)
	if (n >= (1ULL << 32)) { hao_set_err(c, "hao_window_estimate_err: more than 2^32 requests in one call"); return HAO_EUNSUPP; }
	if (n == 0) return HAO_OK;
	hao_ctx::Ladder &G = c->ld;
	HIP_TRY(G.e_req.reserve(n));
	HIP_TRY(hipMemcpyAsync(G.e_req.p, req, n * sizeof(hao_ladder_req_t), hipMemcpyHostToDevice, c->stream));
	uint64_t bad = 0;
	if (int rc = hao_al_estimate(c, B.O().ol_out.p, B.n_ol, n, e_rate, wl, &bad)) return rc;
	if (bad) { hao_set_err(c, "hao_window_estimate_err: " + std::to_string(bad) + " requests out of range (overlap index, or qs / qe outside 0 <= qs <= qe <= q_tot)"); return HAO_EINVAL; }
	HIP_TRY(hipMemcpyAsync(est, G.e_est.p, n * 8, hipMemcpyDeviceToHost, c->stream));
	return HAO_OK;
}
int hao_window_estimate_err(hao_ctx *c, const hao_ladder_req_t *req, uint64_t n_req, double e_rate, int64_t wl, int64_t *est)
{
	if (!c || (n_req && (!req || !est))) return HAO_EINVAL;
	return hao_window_stage(c, nullptr, [&] { return hao_estimate_run(c, req, n_req, e_rate, wl, est); });
}

int hao_window_ladder(hao_ctx *c, const hao_ladder_req_t *req, uint64_t n_req, double e_rate, int64_t maxl, int64_t maxe, hao_ladder_res_t *out, uint64_t *cig_off, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar)
{
	if (!c || !cig_off || !n_cigar || (n_req && (!req || !out)) || (cigar_cap && !cigars)) return HAO_EINVAL;
	return hao_window_stage(c, "ladder", [&] { return hao_ladder_run(c, false, req, n_req, e_rate, 0, maxl, maxe, 0, out, cig_off, cigars, cigar_cap, n_cigar); });
}

int hao_window_ladder_adv(hao_ctx *c, const hao_ladder_req_t *req, uint64_t n_req, double e_rate, int64_t wl, int64_t maxl, int64_t maxe, int64_t force_l, hao_ladder_adv_res_t *out, uint64_t *cig_off, uint16_t *cigars, uint64_t cigar_cap, uint64_t *n_cigar)
{
	if (!c || !cig_off || !n_cigar || (n_req && (!req || !out)) || (cigar_cap && !cigars)) return HAO_EINVAL;
	return hao_window_stage(c, "ladder_adv", [&] { return hao_ladder_run(c, true, req, n_req, e_rate, wl, maxl, maxe, force_l, out, cig_off, cigars, cigar_cap, n_cigar); });
}

int hao_deliver_wlist(hao_ctx *c, int slot, hao_wlist_delivery_t *out) { return hao_deliver_part(c, slot, out, &hao_ctx::Batch::Slot::wl, HAO_DELIVER_WLIST, "hao_deliver_wlist", "HAO_DELIVER_WLIST"); }

uint64_t hao_unpack_wlist(const hao_delivery_t *d, const hao_ed_delivery_t *e, const hao_rescue_delivery_t *r, const hao_wlist_delivery_t *w, const uint32_t *len, uint64_t rid,
		uint64_t *win_off, hao_wlist_win_t *wins, uint64_t *cig_off, uint16_t *cigars, uint64_t cap_ovlp, uint64_t cap_wins, uint64_t cap_cigars)
{
	if (!d || !e || !r || !w || !len) return UINT64_MAX;
	uint64_t o0 = 0;
	const uint64_t n = hao_unpack_records_ok(d, e, len, rid, r->n_ol == d->n_ol && (!w->n_ol || (w->win_off && r->ovlp)) && (!w->n_wins || (w->wins && w->cig_off)) && (!w->n_cigar || w->cigars),
		w->n_ol, w->win_off, w->wins, w->n_wins, &o0);
	if (n == 0 || n == UINT64_MAX) return n;
	const uint64_t o1 = o0 + n, g0 = w->win_off[o0], g1 = w->win_off[o1];
	if (w->win_off[w->n_ol] != w->n_wins || (w->n_wins ? w->cig_off[w->n_wins] : 0) != w->n_cigar) return UINT64_MAX;      // (the counts add up)
	for (uint64_t i = o0; i < o1; ++i) {      // every record in an overlap that passed; entry offsets ascend
		if (w->win_off[i + 1] > w->win_off[i] && !r->ovlp[i].verdict) return UINT64_MAX;
		for (uint64_t k = w->win_off[i]; k < w->win_off[i + 1]; ++k) if (w->cig_off[k] > w->cig_off[k + 1] || w->cig_off[k + 1] > w->n_cigar) return UINT64_MAX;
	}
	const uint64_t c0 = g1 > g0 ? w->cig_off[g0] : 0, c1 = g1 > g0 ? w->cig_off[g1] : 0;
	if (n > cap_ovlp || g1 - g0 > cap_wins || c1 - c0 > cap_cigars || !win_off || !wins || !cig_off || !cigars) return n;
	for (uint64_t i = 0; i <= n; ++i) win_off[i] = w->win_off[o0 + i] - g0;
	for (uint64_t k = g0; k < g1; ++k) { wins[k - g0] = w->wins[k]; cig_off[k - g0] = w->cig_off[k] - c0; }
	cig_off[g1 - g0] = c1 - c0;
	for (uint64_t j = c0; j < c1; ++j) cigars[j - c0] = w->cigars[j];
	return n;
}

int hao_rescue_task(const hao_ovlp_t *z, uint32_t win, uint32_t window, int64_t toff, const uint8_t *tab, uint32_t target_len, hao_ed_task_t *out)
{
	if (!z || !tab || !out || window == 0) return 0;
	return hao_rescue_pair(*z, win, window, toff, tab, target_len, out) ? 1 : 0;
}

int hao_deliver_rescue(hao_ctx *c, int slot, hao_rescue_delivery_t *out) { return hao_deliver_part(c, slot, out, &hao_ctx::Batch::Slot::rs, HAO_DELIVER_RESCUE, "hao_deliver_rescue", "HAO_DELIVER_RESCUE"); }

uint64_t hao_unpack_rescue(const hao_delivery_t *d, const hao_ed_delivery_t *e, const hao_rescue_delivery_t *r, const uint32_t *len, uint64_t rid,
		hao_rescue_ovlp_t *ovlp, uint64_t *win_off, hao_rescue_win_t *wins, uint64_t cap_ovlp, uint64_t cap_wins)
{
	if (!d || !e || !r || !len) return UINT64_MAX;
	uint64_t o0 = 0;
	const uint64_t n = hao_unpack_records_ok(d, e, len, rid, r->n_ol == d->n_ol && (!r->n_ol || (r->ovlp && r->win_off)) && (!r->n_wins || r->wins), r->n_ol, r->win_off, r->wins, r->n_wins, &o0);
	if (n == 0 || n == UINT64_MAX) return n;
	const uint64_t o1 = o0 + n, w0 = r->win_off[o0], w1 = r->win_off[o1];
	if (n > cap_ovlp || w1 - w0 > cap_wins || !ovlp || !win_off || !wins) return n;
	for (uint64_t i = 0; i < n; ++i) { ovlp[i] = r->ovlp[o0 + i]; win_off[i] = r->win_off[o0 + i] - w0; }
	win_off[n] = w1 - w0;
	for (uint64_t k = w0; k < w1; ++k) wins[k - w0] = r->wins[k];
	return n;
}

int hao_deliver_ed(hao_ctx *c, int slot, hao_ed_delivery_t *out) { return hao_deliver_part(c, slot, out, &hao_ctx::Batch::Slot::ed, HAO_DELIVER_ED, "hao_deliver_ed", "HAO_DELIVER_ED"); }

// pure function of the two views of a delivered batch: read rid's grid pairs rebuilt from its delivered overlaps with the device's own hao_grid_pair, in the
// device's order (grid window, then position in ol->list), and their results widened
uint64_t hao_unpack_ed(const hao_ed_delivery_t *e, const hao_delivery_t *d, const uint32_t *len, uint64_t rid, hao_ed_task_t *tasks, hao_ed_result_t *res, uint64_t cap)
{
	if (!e || !d || !len || !e->window || !e->ed_off || rid < d->rid_lo || rid >= d->rid_lo + d->n_reads || !d->ol_off || !d->ol) return 0;
	const uint64_t r = rid - d->rid_lo, p0 = e->ed_off[r], np = e->ed_off[r + 1] - p0;
	if (np > cap || !tasks || !res) return np;
	const uint32_t wl = e->window, thre = e->thre, nword = (2 * thre + 1 + 63) / 64, nw = (uint32_t)(((uint64_t)len[rid] + wl - 1) / wl);
	const uint64_t o0 = d->ol_off[r], o1 = d->ol_off[r + 1];
	uint64_t k = 0;
	if (e->placement == HAO_PLACE_REF) {
		// reference placement: the shift of every (overlap, covered window) from the DELIVERED fake cigars (hao_unpack_cigar), then hao_ref_pair in the device's order
		if (!d->fc_off || !d->fc || !hao_ed_ref_args_ok(wl, e->e_rate)) return UINT64_MAX;
		std::vector<uint8_t> tab((size_t)wl + 1); hao_ref_thre_table(wl, e->e_rate, tab.data());
		std::vector<hao_ovlp_t> zs(o1 - o0); std::vector<uint64_t> so(o1 - o0 + 1, 0); std::vector<int32_t> sh; std::vector<uint64_t> fc;
		if (hao_unpack_overlaps(d, rid, zs.data(), zs.size()) != zs.size()) return UINT64_MAX;
		for (uint64_t i = 0; i < zs.size(); ++i) {
			const hao_ovlp_t &z = zs[i]; const uint32_t w0 = z.x_pos_s / wl, w1 = z.x_pos_e / wl;
			fc.resize((size_t)z.fc_len + 1);
			if (w1 < w0 || hao_unpack_cigar(d, o0 + i, fc.data(), z.fc_len) != z.fc_len) return UINT64_MAX;
			for (uint32_t w = w0; w <= w1; ++w) { const int64_t g0 = (int64_t)w * wl; sh.push_back(hao_ref_shift(fc.data(), z.fc_len, g0 > (int64_t)z.x_pos_s ? g0 : (int64_t)z.x_pos_s)); }
			so[i + 1] = sh.size();
		}
		for (uint32_t w = 0; w < nw; ++w)
			for (uint64_t i = 0; i < zs.size(); ++i) {
				const hao_ovlp_t &z = zs[i]; const uint32_t w0 = z.x_pos_s / wl;
				hao_ed_task_t t;
				if (w0 > w || z.x_pos_e / wl < w || !hao_ref_pair(z, w, wl, sh[so[i] + (w - w0)], tab.data(), len[z.y_id], &t)) continue;
				if (k == np) return UINT64_MAX;
				tasks[k] = t;
				const uint8_t er = e->err[p0 + k]; const uint16_t pe = e->pe[p0 + k];
				res[k].err = er == 0xff ? INT32_MAX : (int32_t)er; res[k].pe = pe == 0xffff ? -1 : (int32_t)pe;
				++k;
			}
		return k == np ? np : UINT64_MAX;
	}
	for (uint32_t w = 0; w < nw; ++w)
		for (uint64_t i = o0; i < o1; ++i) {
			const hao_ovlp_wire_t &x = d->ol[i]; hao_ovlp_t z;      // (hao_unpack_overlaps' record)
			z.x_id = (uint32_t)rid; z.x_pos_s = x.x_pos_s; z.x_pos_e = x.x_pos_e; z.x_pos_strand = 0; z.y_id = x.y & 0x7fffffffu; z.y_pos_s = x.y_pos_s; z.y_pos_e = x.y_pos_e;
			z.y_pos_strand = x.y >> 31; z.shared_seed = x.shared_seed; z.align_length = 0; z.non_homopolymer_errors = x.non_homopolymer_errors; z.fc_len = x.fc_len;
			hao_ed_task_t t;
			if (!hao_grid_pair(z, w, wl, thre, nword, len, &t)) continue;
			if (k == np) return UINT64_MAX;
			tasks[k] = t;
			const uint8_t er = e->err[p0 + k]; const uint16_t pe = e->pe[p0 + k];
			res[k].err = er == 0xff ? INT32_MAX : (int32_t)er; res[k].pe = pe == 0xffff ? -1 : (int32_t)pe;
			++k;
		}
	return k == np ? np : UINT64_MAX;
}

int hao_fetch_exact(hao_ctx *c, uint64_t rid, const uint8_t **flags, uint64_t *n)
{
	if (!c || !flags || !n || !c->batch || !c->batch->valid || rid < c->batch->lo || rid >= c->batch->lo + c->batch->n) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_exact_check(c)) return rc;
	if (int rc = hao_batch_download(c)) return rc;
	hao_ctx::Batch &B = *c->batch;
	if (B.h_exact.size() != B.n_ol + 1) { B.h_exact.assign(B.n_ol + 1, 0); if (B.n_ol) HIP_TRY(hipMemcpy(B.h_exact.data(), B.O().exact.p, B.n_ol, hipMemcpyDeviceToHost)); }
	const uint64_t r = rid - B.lo, s_ = B.h_fin_off[r], e_ = B.h_fin_off[r + 1];
	*flags = B.h_exact.data() + s_; *n = e_ - s_;
	return HAO_OK;
}

int hao_fetch_seed_hits(hao_ctx *c, uint64_t rid, const hao_hit_t **hits, uint64_t *n)
{
	if (!c || !c->batch || !c->batch->valid || rid < c->batch->lo || rid >= c->batch->lo + c->batch->n) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_batch_download(c)) return rc;
	hao_ctx::Batch &B = *c->batch; uint64_t r = rid - B.lo;
	*hits = B.h_hits.data() + B.h_seg[r]; *n = B.h_seg[r + 1] - B.h_seg[r];
	return HAO_OK;
}

int hao_fetch_overlaps(hao_ctx *c, uint64_t rid, const hao_ovlp_t **ol, uint64_t *n_ol, const uint64_t **fc, const uint64_t **fc_off, const hao_hit_t **cl, uint64_t *n_cl)
{
	if (!c || !c->batch || !c->batch->valid || rid < c->batch->lo || rid >= c->batch->lo + c->batch->n) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_batch_download(c)) return rc;
	hao_ctx::Batch &B = *c->batch; uint64_t r = rid - B.lo, s = B.h_fin_off[r], e = B.h_fin_off[r + 1];
	*ol = B.h_ol.data() + s; *n_ol = e - s;
	*fc = B.h_fc.data() + B.h_fc_out_off[s]; *fc_off = B.h_fc_out_off.data() + s;     // absolute offsets; entry i spans [fc_off[i]-fc_off[0], fc_off[i+1]-fc_off[0]) of *fc
	*cl = B.h_cl.data() + B.h_cl_off[r]; *n_cl = B.h_cl_off[r + 1] - B.h_cl_off[r];
	return HAO_OK;
}

int hao_batch_totals(hao_ctx *c, uint64_t out[8])
{
	if (!c || !c->batch || !c->batch->valid) return HAO_EINVAL;
	hao_ctx::Batch &B = *c->batch;
	memset(out, 0, 8 * sizeof(uint64_t));
	out[0] = B.n_ol; out[1] = B.n_cl; out[2] = B.n_anchor; out[3] = B.n_groups; out[4] = B.n_mz; out[5] = B.n_chains; out[6] = B.n_generic; out[7] = B.n_generic_hits;
	return HAO_OK;
}

int hao_batch_seed_path(hao_ctx *c, uint64_t out[4])
{
	if (!c || !out || !c->batch || !c->batch->valid) return HAO_EINVAL;
	hao_ctx::Batch &B = *c->batch;
	out[0] = B.seed_path; out[1] = B.seed_left[0]; out[2] = B.seed_left[1]; out[3] = B.seed_left[2];
	return HAO_OK;
}

int hao_batch_chain_path(hao_ctx *c, uint64_t out[16])
{
	if (!c || !out || !c->batch || !c->batch->valid) return HAO_EINVAL;
	hao_ctx::Batch &B = *c->batch;
	for (int x = 0; x < HAO_NCLS; ++x) { out[x] = B.cls_n[x]; out[HAO_NCLS + x] = B.slow_n[x]; }
	out[2 * HAO_NCLS] = B.n_generic_hits; out[2 * HAO_NCLS + 1] = 0;
	return HAO_OK;
}

int hao_batch_digest(hao_ctx *c, uint64_t *out, uint64_t *out_kh)
{
	if (!c || !out || !c->batch || !c->batch->valid) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	hao_ctx::Batch &B = *c->batch; const uint64_t n = B.n;
	if (n == 0) return HAO_OK;
	if (int rc = hao_batch_materialize_cl(c)) return rc;
	DevBuf<uint64_t> d; HIP_TRY(d.reserve(2 * n + 2));
	hao_digest_args a;
	a.fin_off = B.O().fin_off.p; a.fcf_off = B.fcf_off.p; a.g_off = B.g_off.p; a.cl_base = B.cl_base.p; a.seg = B.seg.p;
	a.ol = (const uint64_t*)B.O().ol_out.p; a.fc = B.O().fc_out.p; a.cl = (const uint64_t*)B.cl.p; a.hits = (const uint64_t*)B.hits.p;
	a.n_sel = n; a.dig = d.p; a.dig_kh = out_kh ? d.p + n : nullptr;
	hipLaunchKernelGGL(hao_digest_kernel, dim3((unsigned)n), dim3(256), 0, c->stream, a);
	HAO_CHECK_LAUNCH();
	HIP_TRY(hipMemcpyAsync(out, d.p, n * 8, hipMemcpyDeviceToHost, c->stream));
	if (out_kh) HIP_TRY(hipMemcpyAsync(out_kh, d.p + n, n * 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HAO_OK;
}

// Self-test of the two ways to group minimizer records by their 16 owner bits (hao_pt_run, sharded): out[0] = order violations of
// rocprim::radix_sort_pairs(begin_bit = 48, end_bit = 64) on (hash, index) pairs, out[1] = violations of the path the engine uses (separate 16-bit
// key, begin_bit = 0, then a gather).  A "violation" = a position whose owner bits decrease, or equal owner bits with a decreasing index (the
// sort must be stable).  tests/test_gpu_rocprim.py pins out[1] == 0 and logs out[0].
__global__ void hao_selftest_fill_kernel(uint64_t n, uint64_t *x, uint64_t *v)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) { x[i] = hao_hash64(i * 0x9E3779B97F4A7C15ULL + 12345); v[i] = i; }
}
// Self-test of the index sort on 40 hash bits (hao_index_sort): n keys built so that many 40-bit runs hold up to four distinct keys, interleaved in input
// order; sorted both ways on the device.  out = { positions where the two results differ, two-key runs the fix-up listed, scratch elements used, overflow flag }
__global__ void hao_selftest_s40_fill_kernel(uint64_t n, uint64_t *x)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) { const uint64_t g = i % (n / 5 + 1); x[i] = (hao_hash64(g + 99) & ~((1ULL << HAO_SORT40_LOWBITS) - 1)) | ((g & 255) ? 0x155ULL : ((hao_hash64(i) >> 7) & 3) * 0x2a5b7ULL); }      // one 40-bit group in 256 holds up to four keys, interleaved in input order
}
__global__ void hao_selftest_s40_cmp_kernel(const uint64_t *a, const uint64_t *b, const uint32_t *ia, const uint32_t *ib, uint64_t n, unsigned long long *bad)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && (a[i] != b[i] || ia[i] != ib[i])) atomicAdd(bad, 1ULL);
}
int hao_selftest_sortbits(hao_ctx *c, uint64_t n, uint64_t out[4])
{
	if (!c || !out || n < 16 || n >= (1ULL << 32)) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf<uint64_t> x, s1, s2; DevBuf<uint32_t> o, o1, o2; DevBuf<unsigned long long> bad;
	HIP_TRY(x.reserve(n)); HIP_TRY(s1.reserve(n)); HIP_TRY(s2.reserve(n)); HIP_TRY(o.reserve(n)); HIP_TRY(o1.reserve(n)); HIP_TRY(o2.reserve(n)); HIP_TRY(bad.reserve(1));
	HIP_TRY(hipMemsetAsync(bad.p, 0, 8, c->stream));
	hipLaunchKernelGGL(hao_selftest_s40_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, x.p); HAO_CHECK_LAUNCH();
	int rc = hao_index_sort(c, x.p, s1.p, o.p, o1.p, n, false);
	if (!rc) rc = hao_index_sort(c, x.p, s2.p, o.p, o2.p, n, true);
	if (!rc) {
		hipLaunchKernelGGL(hao_selftest_s40_cmp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, s1.p, s2.p, o1.p, o2.p, n, bad.p);
		unsigned long long hb = 0;
		if (hipMemcpyAsync(&hb, bad.p, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = HAO_ENODEV;
		out[0] = hb; for (int k = 0; k < 3; ++k) out[1 + k] = c->peeked(PK_SORT40, k);
	}
	return rc;
}

int hao_selftest_rocprim(uint64_t n, uint64_t out[2])
{
	hao_ctx tmp_ctx; hao_ctx *c = &tmp_ctx;      // only for the error-string macros
	if (!out || n == 0 || n >= (1ULL << 32)) return HAO_EINVAL;
	out[0] = out[1] = 0;
	hipStream_t st = nullptr;
	DevBuf<uint64_t> x, v, x2, v2, gx, gv; DevBuf<uint32_t> ok, ok2, oi, oi2; DevBuf<unsigned char> tmp;
	HIP_TRY(x.reserve(n)); HIP_TRY(v.reserve(n)); HIP_TRY(x2.reserve(n)); HIP_TRY(v2.reserve(n)); HIP_TRY(gx.reserve(n)); HIP_TRY(gv.reserve(n));
	HIP_TRY(ok.reserve(n)); HIP_TRY(ok2.reserve(n)); HIP_TRY(oi.reserve(n)); HIP_TRY(oi2.reserve(n));
	hipLaunchKernelGGL(hao_selftest_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, x.p, v.p);
	HIP_TRY(hipGetLastError());
	size_t tb = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, x.p, x2.p, v.p, v2.p, n, 48, 64, st)); HIP_TRY(tmp.reserve(tb + 256));
	HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tb, x.p, x2.p, v.p, v2.p, n, 48, 64, st));
	hipLaunchKernelGGL(hao_owner_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x.p, n, ok.p, oi.p);
	HIP_TRY(hipGetLastError());
	rocprim::double_buffer<uint32_t> dk(ok.p, ok2.p), dv(oi.p, oi2.p); tb = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, dk, dv, n, 0, 16, st)); HIP_TRY(tmp.reserve(tb + 256));
	HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tb, dk, dv, n, 0, 16, st));
	hipLaunchKernelGGL(hao_gather2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dv.current(), x.p, v.p, n, gx.p, gv.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipDeviceSynchronize());
	std::vector<uint64_t> hx(n), hv(n);
	for (int which = 0; which < 2; ++which) {
		HIP_TRY(hipMemcpy(hx.data(), which ? gx.p : x2.p, n * 8, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(hv.data(), which ? gv.p : v2.p, n * 8, hipMemcpyDeviceToHost));
		uint64_t bad = 0;
		for (uint64_t i = 1; i < n; ++i) { const uint64_t a = hx[i - 1] >> 48, b = hx[i] >> 48; if (a > b || (a == b && hv[i - 1] >= hv[i])) ++bad; }
		for (uint64_t i = 0; i < n; ++i) if (hv[i] >= n || hx[i] != hao_hash64(hv[i] * 0x9E3779B97F4A7C15ULL + 12345)) ++bad;      // a permutation of the input pairs
		out[which] = bad;
	}
	return HAO_OK;
}

// Self-test of the paths that see more than 2^32 items (the k-mer occurrences of a 250 Mb genome at 30x are 5.6 G): n u32 keys, key[i] = i / 8, written by
// the grid-stride launch shape the Bloom replay uses and run-length encoded by hao_rle.  out = { runs, sum of the run lengths, runs whose length is not 8 }:
// n / 8, n and 0 for n a multiple of 8.  (A launch of more than 2^32 work-items and rocprim::run_length_encode's `unsigned int size` both silently process
// n mod 2^32 items.)
__global__ void hao_selftest_fill32_kernel(uint64_t n, uint32_t *k)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) k[i] = (uint32_t)(i >> 3);
}
struct hao_not8 { __host__ __device__ uint64_t operator()(const uint32_t &v) const { return v != 8; } };
int hao_selftest_big(uint64_t n, uint64_t out[3])
{
	hao_ctx tmp_ctx; hao_ctx *c = &tmp_ctx;
	if (!out || n == 0 || (n >> 3) >= (1ULL << 32)) return HAO_EINVAL;
	out[0] = out[1] = out[2] = 0;
	DevBuf<uint32_t> k, uk, uc;
	HIP_TRY(k.reserve_exact(n)); HIP_TRY(uk.reserve_exact((n >> 3) + 2)); HIP_TRY(uc.reserve_exact((n >> 3) + 2)); HIP_TRY(c->d_cursor.reserve(2));
	hipLaunchKernelGGL(hao_selftest_fill32_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20)), dim3(256), 0, c->stream, n, k.p);
	HIP_TRY(hipGetLastError());
	if (int rc = hao_rle(c, (const uint32_t*)k.p, n, uk.p, uc.p, (uint64_t*)c->d_cursor.p)) return rc;
	HIP_TRY(hipMemcpy(&out[0], c->d_cursor.p, 8, hipMemcpyDeviceToHost));
	if (out[0] <= (n >> 3) + 1) {
		out[1] = hao_dbg_reduce(c, rocprim::make_transform_iterator(uc.p, U32ToU64()), out[0], rocprim::plus<uint64_t>());
		out[2] = hao_dbg_reduce(c, rocprim::make_transform_iterator(uc.p, hao_not8()), out[0], rocprim::plus<uint64_t>());
	}
	HIP_TRY(hipDeviceSynchronize());
	return HAO_OK;
}

int hao_pt_table(hao_ctx *c, uint64_t *n_keys, const uint64_t **keys, const uint64_t **off, const uint64_t **pos, uint64_t *n_pos)
{
	if (!c || !c->has_pt) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = hao_pt_download(c)) return rc;
	*n_keys = c->h_ix_keys.size(); *keys = c->h_ix_keys.data(); *off = c->h_ix_off.data(); *pos = c->h_ix_pos.data(); *n_pos = c->h_ix_pos.size();
	return HAO_OK;
}
}


int hao_ovlp_bin_read(const char *path, uint64_t *n_reads, uint8_t **flags, uint64_t **off, hao_ma_hit_t **hits)
{
	if (!path || !n_reads || !flags || !off || !hits) return HAO_EINVAL;
	try { return hao_ovlp_bin_read_impl(path, n_reads, flags, off, hits); }
	catch (const std::bad_alloc &) { return HAO_ENOMEM; }
	catch (const std::exception &) { return HAO_EINVAL; }
}
int hao_ovlp_bin_write(const char *path, uint64_t n_reads, const uint8_t *flags, const uint64_t *off, const hao_ma_hit_t *hits)
{ return hao_ovlp_bin_write_impl(path, n_reads, flags, off, hits); }
