// Host side of streamed delivery (hao_overlap_batch_async): the pinned arenas of the two delivery slots and their NUMA placement, the section list that lays a
// batch's results out in its slot's arena, and the queueing of the copy.  Included by hao_batch.hpp after hao_ctx::Batch (part of libhao.so).
#pragma once
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>
// The delivery arenas should live on the NUMA node the GPU hangs off: on a two-socket host a pinned buffer on the far socket costs the DMA ~40 % of its
// rate (measured: 29-35 GB/s instead of 51-56).  The pages of a hipHostMalloc are placed by the calling thread's memory policy, so the allocation is
// bracketed by set_mempolicy(MPOL_PREFERRED, gpu node) / MPOL_DEFAULT (raw syscalls: no libnuma in the image; failures - seccomp, no sysfs - are ignored).
static int hao_gpu_numa_node(int device)
{
	char bus[64] = {0};
	if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return -1;
	for (char *p = bus; *p; ++p) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');
	char path[160]; snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
	FILE *fp = fopen(path, "r"); int node = -1;
	if (fp) { if (fscanf(fp, "%d", &node) != 1) node = -1; fclose(fp); }
	return node;
}
// The calling thread's NUMA memory policy around one allocation.  The caller may be a thread of a host application (the shim inside hifiasm) that runs under a policy
// of its own (numactl --interleave ...): the policy found is saved and put back, never reset to the default.
struct hao_mempolicy_guard {
	int old_mode = 0; unsigned long old_mask[16]; bool saved = false, applied = false;
	// mode: 1 = MPOL_PREFERRED, 2 = MPOL_BIND
	hao_mempolicy_guard(int node, int mode) {
		memset(old_mask, 0, sizeof(old_mask));
		if (node < 0 || node >= 1024) return;
		saved = syscall(SYS_get_mempolicy, &old_mode, old_mask, 1024UL, nullptr, 0UL) == 0;
		if (!saved) return;      // cannot restore what cannot be read: leave the policy alone
		unsigned long mask[16]; memset(mask, 0, sizeof(mask)); mask[node / 64] |= 1UL << (node % 64);
		applied = syscall(SYS_set_mempolicy, mode, mask, 1024UL) == 0;
	}
	~hao_mempolicy_guard() {
		if (!applied) return;
		bool any = false; for (int i = 0; i < 16; ++i) any |= old_mask[i] != 0;
		(void)syscall(SYS_set_mempolicy, old_mode, any ? old_mask : (unsigned long*)nullptr, any ? 1024UL : 0UL);
	}
};
// how many of 32 sampled pages of [p, p + bytes) lie on `node` (move_pages with no target nodes only reports); -1: cannot tell
static int hao_pages_on_node(const void *p, size_t bytes, int node)
{
	const long ps = sysconf(_SC_PAGESIZE); if (ps <= 0 || bytes < (size_t)ps) return -1;
	void *pg[32]; int st[32]; const size_t np = bytes / (size_t)ps;
	for (int i = 0; i < 32; ++i) { pg[i] = (void*)(((uintptr_t)p + (np - 1) * (size_t)i / 31 * (size_t)ps) & ~(uintptr_t)(ps - 1)); st[i] = -1; }
	if (syscall(SYS_move_pages, 0, 32UL, pg, (const int*)nullptr, st, 0) != 0) return -1;
	int on = 0; for (int i = 0; i < 32; ++i) on += st[i] == node;
	return on;
}
// A pinned host buffer whose pages are ON `node`, whatever the allocator of hipHostMalloc does: anonymous mapping, mbind(MPOL_BIND) before the first touch (the kernel
// then reclaims that node's page cache instead of falling over to the far socket), touched, registered with the runtime.  nullptr when any step fails.
static unsigned char *hao_arena_alloc_bound(size_t bytes, int node)
{
	if (node < 0 || node >= 1024) return nullptr;
	// (2 MB-aligned and advised as huge pages: what round 6's slow arenas had in common was not their node - a fresh mapping on the SAME node copied at 56 GB/s where the
	// hipHostMalloc'ed one gave 30 - which leaves the page size the DMA translates through.  The caller passes a multiple of 2 MB.)
	const size_t HP = (size_t)2 << 20;
	void *m0 = mmap(nullptr, bytes + HP, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
	if (m0 == MAP_FAILED) return nullptr;
	void *m = (void*)(((uintptr_t)m0 + HP - 1) & ~(uintptr_t)(HP - 1));
	if (m != m0) (void)munmap(m0, (size_t)((uintptr_t)m - (uintptr_t)m0));
	{ const uintptr_t end0 = (uintptr_t)m0 + bytes + HP, end = (uintptr_t)m + ((bytes + 4095) & ~(size_t)4095); if (end0 > end) (void)munmap((void*)end, (size_t)(end0 - end)); }
	(void)madvise(m, bytes, MADV_HUGEPAGE);
	unsigned long mask[16]; memset(mask, 0, sizeof(mask)); mask[node / 64] |= 1UL << (node % 64);
	if (syscall(SYS_mbind, m, bytes, 2 /* MPOL_BIND */, mask, 1024UL, 0U) != 0) { (void)munmap(m, bytes); return nullptr; }
	const long ps = sysconf(_SC_PAGESIZE);
	for (size_t o = 0; o < bytes; o += (size_t)(ps > 0 ? ps : 4096)) ((volatile unsigned char*)m)[o] = 0;
	if (hipHostRegister(m, bytes, hipHostRegisterMapped | hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); (void)munmap(m, bytes); return nullptr; }
	return (unsigned char*)m;
}
// the NUMA node a probe found best for a device's delivery arenas, kept for the process (every engine and batch context of the device starts from it)
static int hao_arena_node_of[64] = { -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
	-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1 };
// GB/s of one device-to-host copy of nb bytes into `host` on the batch's copy stream (HIP events around it); -1 when it cannot be measured
static double hao_arena_rate(hipStream_t st, unsigned char *host, const void *dsrc, size_t nb)
{
	hipEvent_t e0 = nullptr, e1 = nullptr; double r = -1;
	if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess &&
		hipEventRecord(e0, st) == hipSuccess && hipMemcpyAsync(host, dsrc, nb, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess) {
		float ms = 0; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0) r = (double)nb / ((double)ms * 1e6);
	}
	if (e0) (void)hipEventDestroy(e0);
	if (e1) (void)hipEventDestroy(e1);
	(void)hipGetLastError();
	return r;
}

// The slot's arena holds `total` bytes and is worth keeping, or is allocated (again): grown by a quarter and 1 MB, placed on the GPU's NUMA node, its copy rate
// probed.  s in the messages: the slot's number.
static int hao_arena_ensure(hao_ctx *c, hao_ctx::Batch &B, hao_ctx::Batch::Slot &S, size_t total)
{
	if (total <= S.arena_cap && !S.arena_bad) return HAO_OK;
	const int s = (int)(&S - B.slot);
	const bool redo_ = S.arena_bad; S.arena_bad = false;      // (hao_deliver_wait saw this slot's last batch copied at less than 40 GB/s: the probe below tries every NUMA node)
	S.arena_free();
	const size_t want = (total + total / 4 + (1 << 20) + (((size_t)2 << 20) - 1)) & ~(((size_t)2 << 20) - 1);      // (a multiple of 2 MB: hao_arena_alloc_bound)
	const double t0_ = hao_now();
	const int node_ = c->sw.arena_numa ? hao_gpu_numa_node(c->device) : -1;
	// MPOL_BIND first: "preferred" silently falls over to the far socket when the GPU's node is short of FREE pages (a process that has just generated or
	// parsed gigabytes of reads leaves it full of page cache) - the same box then delivers at 36 instead of 52 GB/s; bound, the kernel reclaims instead.
	// If the bound allocation fails, once more with the preference only.
	hipError_t he_ = hipErrorOutOfMemory; const char *how_ = "default policy";
	if (B.arena_node >= 0) if (unsigned char *m_ = hao_arena_alloc_bound(want, B.arena_node)) { S.arena = m_; S.arena_reg = true; he_ = hipSuccess; how_ = "by hand on the node an earlier probe chose"; }
	if (he_ != hipSuccess && node_ >= 0 && c->sw.arena_numa != 1) {
		hao_mempolicy_guard g_(node_, 2 /* MPOL_BIND */);
		if (g_.applied) {
			he_ = hipHostMalloc((void**)&S.arena, want, (c->sw.arena_numa == 2) ? hipHostMallocNumaUser : hipHostMallocDefault);
			if (he_ != hipSuccess) { S.arena = nullptr; (void)hipGetLastError(); } else how_ = "bound";
		}
	}
	if (he_ != hipSuccess) {
		hao_mempolicy_guard g_(node_, 1 /* MPOL_PREFERRED */);
		he_ = hipHostMalloc((void**)&S.arena, want, (c->sw.arena_numa == 2 && g_.applied) ? hipHostMallocNumaUser : hipHostMallocDefault);
		if (he_ == hipSuccess && g_.applied) how_ = "preferred";
	}
	// where did the pages land?  hipHostMalloc does not always honour the calling thread's policy (one run of round 6 delivered configs[2] at 28.6 GB/s and, with
	// arenas allocated later in the same process, at 53.5): if fewer than 28 of 32 sampled pages are on the GPU's node, the arena is allocated again by hand
	int on_ = -1;
	if (he_ == hipSuccess && node_ >= 0) {
		on_ = hao_pages_on_node(S.arena, want, node_);
		if (!S.arena_reg && ((on_ >= 0 && on_ < 28) || c->sw.arena_numa == 4)) {      // (HAO_ARENA_NUMA=4: always by hand - tests)
			if (unsigned char *m_ = hao_arena_alloc_bound(want, node_)) { (void)hipHostFree(S.arena); S.arena = m_; S.arena_reg = true; how_ = "mmap + mbind + hipHostRegister"; on_ = hao_pages_on_node(m_, want, node_); }
		}
	}
	// What the placement is worth is MEASURED: one run in eight of round 6 still delivered at 28.7 instead of 50 GB/s (same box, next process: 49.8) with every page
	// reported on the GPU's node.  A 128 MB copy into the new arena is timed; below 50 GB/s a 128 MB buffer bound to each NUMA node in turn gets the same copy and the
	// arena moves to the best node when that is 10 % faster.  (Arenas of 64 MB and more; HAO_DBG_TEST=arena_probe=1: always and whatever the size - tests.)
	if (he_ == hipSuccess && c->sw.arena_numa && (want >= ((size_t)64 << 20) || c->sw.arena_probe) && B.hits.p) {
		const size_t nb = std::min<size_t>(std::min<size_t>(want, (size_t)128 << 20), B.hits.cap * sizeof(hao_hit_t)) & ~(size_t)4095;
		if (nb >= 4096) {
			(void)hao_arena_rate(B.copy_stream, S.arena, B.hits.p, nb);      // (first touch of the mapping)
			const double r0 = hao_arena_rate(B.copy_stream, S.arena, B.hits.p, nb);
			if ((r0 >= 0 && r0 < 50.0) || c->sw.arena_probe || redo_) {      // (a good arena: 55 - 57 GB/s with the device otherwise idle, as it is here)
				int best_k = -1; double best = r0;
				for (int k = 0; k < 16; ++k) {
					unsigned char *m_ = hao_arena_alloc_bound(nb, k); if (!m_) continue;
					(void)hao_arena_rate(B.copy_stream, m_, B.hits.p, nb);
					const double rk = hao_arena_rate(B.copy_stream, m_, B.hits.p, nb);
					(void)hipHostUnregister(m_); (void)munmap(m_, nb);
					if (c->sw.dltime || c->sw.arena_probe) fprintf(stderr, "[deliver] arena %d probe: NUMA node %d %.1f GB/s\n", s, k, rk);
					if (rk > best * 1.1) { best = rk; best_k = k; }
				}
				if (best_k >= 0) if (unsigned char *m_ = hao_arena_alloc_bound(want, best_k)) { S.arena_cap = want; S.arena_free(); S.arena = m_; S.arena_reg = true; B.arena_node = best_k; if (c->device >= 0 && c->device < 64) hao_arena_node_of[c->device] = best_k; how_ = "moved after the probe"; }      // (arena_free unmaps arena_cap bytes of a registered arena)
				fprintf(stderr, "[hao] delivery arena %d: %.1f GB/s from the device as allocated (GPU NUMA node %d, %s)%s\n", s, r0, node_, how_, best_k >= 0 ? "" : "; no NUMA node does better");
				if (best_k >= 0) fprintf(stderr, "[hao] delivery arena %d: moved to NUMA node %d (%.1f GB/s)\n", s, best_k, best);
			}
		}
	}
	if (c->sw.dltime) fprintf(stderr, "[deliver] arena %d: %zu MB, GPU NUMA node %d (requested mode %d, allocated %s, %d of 32 sampled pages on the node)\n", s, want >> 20, node_, c->sw.arena_numa, he_ == hipSuccess ? how_ : "FAILED", on_);
	HIP_TRY(he_);
	S.arena_cap = want; B.t_alloc += hao_now() - t0_;
	return HAO_OK;
}

// The first things a streamed batch does to its slot: the views zeroed, the parts it asked for noted, the ED view's grid named (an empty batch ends here)
inline void hao_ctx::Batch::Slot::begin(uint32_t parts_, uint64_t lo, uint64_t n, const hao_ctx *c)
{
	parts = parts_;
	dl = hao_delivery_t(); ed = hao_ed_delivery_t(); tr = hao_trace_delivery_t(); rs = hao_rescue_delivery_t(); wl = hao_wlist_delivery_t();
	dl.rid_lo = lo; dl.n_reads = n;
	if (parts & HAO_DELIVER_ED) { ed.window = c->ded_window; ed.thre = c->ded_thre; ed.placement = c->ded_place; ed.e_rate = c->ded_place == HAO_PLACE_REF ? c->ded_erate : 0; }
}
inline void hao_ctx::Batch::Slot::arena_free()
{
	if (!arena) return;
	if (arena_reg) { (void)hipHostUnregister(arena); (void)munmap(arena, arena_cap); } else (void)hipHostFree(arena);
	arena = nullptr; arena_cap = 0; arena_reg = false;
}

// The sections of one batch's arena, in the order they lie there.  put() names an array once: the view pointer that shows it, where it comes from on the device, the
// bytes copied and - where the region holds more than is copied - the bytes of the region.  size() gives every section its offset, the running sum of the regions
// padded to 64 bytes each, and returns the end; queue() queues the copies, points the views into the arena and adds the bytes copied to *bytes.
struct hao_sections {
	enum { CAP = 32 };
	struct Sec { void *view; const void *src; size_t copy, region, off; } sec[CAP];
	int n = 0;
	template <class T> void put(const T *&view, const void *src, size_t copy, size_t region = 0) { if (n < CAP) sec[n] = Sec{ &view, src, copy, region ? region : copy, 0 }; ++n; }
	size_t size() { size_t o = 0; for (int i = 0; i < n; ++i) { sec[i].off = o; o += (sec[i].region + 63) & ~(size_t)63; } return o; }
	hipError_t queue(unsigned char *arena, hipStream_t st, uint64_t *bytes) const
	{
		for (int i = 0; i < n; ++i) {
			const Sec &x = sec[i]; const unsigned char *at = arena + x.off;
			if (x.copy) { const hipError_t e = hipMemcpyAsync(arena + x.off, x.src, x.copy, hipMemcpyDeviceToHost, st); if (e != hipSuccess) return e; }
			memcpy(x.view, &at, sizeof(at)); *bytes += x.copy;
		}
		return hipSuccess;
	}
};

// Queue the copy of the current batch's results into the slot's pinned arena (copy stream, after everything on the compute stream so far).  A part that was not
// asked for has no section: the others lie where they would without it.  (hao_overlap_run returns before this for an empty batch: nothing queued, the views zeroed.)
static int hao_deliver_enqueue(hao_ctx *c)
{
	hao_ctx::Batch &B = *c->batch; hao_ctx::Batch::Slot &S = B.slot[B.cur]; hao_ctx::Batch::OutSet &O = S.out; const uint64_t n = B.n, m = B.n_ol; const uint32_t parts = S.parts;
	hao_delivery_t &d = S.dl; hao_ed_delivery_t &e = S.ed; hao_trace_delivery_t &t = S.tr; hao_rescue_delivery_t &r = S.rs; hao_wlist_delivery_t &w = S.wl;
	hao_sections L;
	if (parts & HAO_DELIVER_OL) {
		d.n_ol = m; d.n_fc = B.n_fcw;
		L.put(d.ol_off, O.fin_off.p, (n + 1) * 8);
		L.put(d.ol, O.ol_wire.p, m * sizeof(hao_ovlp_wire_t));
		L.put(d.fc_off, O.fcw_off.p, m * 8, (m + 1) * 8);      // (room for the end of the last cigar: a host-side word next to, not inside, what the copy writes)
		L.put(d.fc, O.fcw.p, B.n_fcw * 4);
	}
	if (parts & HAO_DELIVER_CL) {
		const uint64_t nw = (B.n_anchor + 63) / 64;      // 64-position words of the batch's bit stream (positions = seed hits)
		const uint64_t nr4 = nw / 4 + 1;                 // rank directory entries on the wire: one per 256 positions
		d.n_chains = B.n_chains; d.n_cl = B.n_cl; d.n_exc = B.n_exc; d.n_codes = B.n_codes; d.n_pos = B.n_anchor;
		L.put(d.ch_off, O.ch_off.p, (n + 1) * 8);
		L.put(d.cl_off, O.cl_off.p, (n + 1) * 8);
		L.put(d.qm_off, O.qm_off.p, (n + 1) * 8);
		L.put(d.chains, O.hdr.p, B.n_chains * sizeof(hao_chain_hdr_t));
		if (O.qmz16) {      // the minimizer tables in 2 + 2 bytes per minimizer (hao_qtab16_kernel) instead of 8
			L.put(d.qmz_pos, O.qmz_pos.p, B.n_mz * 2);
			L.put(d.qmz_cnt, O.qmz_cnt.p, B.n_mz * 2);
		} else
			L.put(d.qmz, O.qmz.p, B.n_mz * sizeof(hao_qmz_t));
		L.put(d.cl_bits, O.bits.p, nw * 8);
		L.put(d.cl_rank, O.rank4.p, nr4 * 4);
		L.put(d.cl_codes, O.codes.p, B.n_codes);
		L.put(d.cl_exc, O.exc.p, B.n_exc * sizeof(hao_exc_t));
	}
	if (parts & HAO_DELIVER_EXACT) {
		d.n_ol = m;
		L.put(d.exact, O.exact.p, m);
	}
	if (parts & HAO_DELIVER_ED) {
		e.n_pairs = B.ed_n;
		L.put(e.ed_off, O.ed_off.p, (n + 1) * 8);
		L.put(e.err, O.ed_err.p, B.ed_n);
		L.put(e.pe, O.ed_pe.p, B.ed_n * 2);
		if (e.placement == HAO_PLACE_REF) {      // (reference placement: the per-overlap summaries travel after the pairs' records)
			e.unresolved = B.ed_unres;
			L.put(e.ovlp, O.ed_sum.p, m * sizeof(hao_ed_ovlp_sum));
		}
	}
	if (parts & HAO_DELIVER_TRACE) {
		t.n_traced = B.tr_n; t.n_cigar = B.tr_ncig;
		L.put(t.cg_off, O.tr_off.p, (n + 1) * 8);
		L.put(t.ps, O.tr_ps.p, B.ed_n * 2);
		L.put(t.n_cig, O.tr_ncig.p, B.ed_n * 2);
		L.put(t.cigar, O.tr_cig.p, B.tr_ncig * 2);
	}
	if (parts & HAO_DELIVER_RESCUE) {
		r.n_ol = m; r.n_wins = c->rs_nw; r.n_rescued = c->rs_total;
		L.put(r.ovlp, O.rs_ovlp.p, m * sizeof(hao_rs_ovlp));
		L.put(r.win_off, O.rs_off.p, (m + 1) * 8);
		L.put(r.wins, O.rs_wins.p, c->rs_nw * sizeof(hao_rs_win));
	}
	if (parts & HAO_DELIVER_WLIST) {
		w.n_ol = m; w.n_wins = c->wl_out[0]; w.n_swept = c->wl_out[1]; w.n_replace = c->wl_out[2]; w.n_cigar = c->wl_out[3]; w.n_untraced = c->wl_out[4];
		L.put(w.win_off, O.wl_woff.p, (m + 1) * 8);
		L.put(w.wins, O.wl_wins.p, w.n_wins * sizeof(hao_rs_win));
		L.put(w.cig_off, O.wl_cigoff.p, (w.n_wins + 1) * 8);
		L.put(w.cigars, O.wl_cig.p, w.n_cigar * 2);
	}
	if (L.n > hao_sections::CAP) { hao_set_err(c, "hao_deliver_enqueue: more sections than hao_sections holds"); return HAO_EINVAL; }
	if (int rc = hao_arena_ensure(c, B, S, L.size())) return rc;
	HIP_TRY(hipEventRecord(S.ev_ready, c->stream));
	HIP_TRY(hipStreamWaitEvent(B.copy_stream, S.ev_ready, 0));
	HIP_TRY(hipEventRecord(S.ev_cstart, B.copy_stream));      // (the copy itself, without the wait behind the previous batch's: hao_deliver_wait checks its rate)
	HIP_TRY(L.queue(S.arena, B.copy_stream, &d.bytes));
	if (parts & HAO_DELIVER_OL) ((uint64_t*)d.fc_off)[m] = B.n_fcw;      // end of the last cigar (hao_deliver_wait writes it again once the copy has landed)
	HIP_TRY(hipEventRecord(S.ev_done, B.copy_stream));
	S.pending = true;
	return HAO_OK;
}

static int hao_deliver_init(hao_ctx *c, hao_ctx::Batch &B)
{
	if (B.dl_ready) return HAO_OK;
	HIP_TRY(hipStreamCreateWithFlags(&B.copy_stream, hipStreamNonBlocking));
	for (hao_ctx::Batch::Slot &S : B.slot) { HIP_TRY(hipEventCreate(&S.ev_ready)); HIP_TRY(hipEventCreate(&S.ev_done)); HIP_TRY(hipEventCreate(&S.ev_cstart)); }
	if (c->device >= 0 && c->device < 64) B.arena_node = hao_arena_node_of[c->device];
	B.dl_ready = true;
	return HAO_OK;
}
