// The gathered read store of a sharded engine (include/hao.h: hao_dist_gather_reads) and the digest of the reads a stage sees (hao_reads_digest).
//
// A rank of a sharded engine holds the lengths of all reads but the bases of its own slice, so nothing beyond the seam - the exact check, the window
// alignments - could run there.  DESIGN 6 replicates the index with one all-gather instead of exchanging per batch; the read store is the same kind of object
// and smaller, and hao_dist_gather_reads replicates it the same way, once and on request: every rank's packed bytes, pack offsets, N-site offsets and N sites
// travel through hao_comm_allgatherv in chunks of bounded size into their place in global read-id order, and one kernel turns the ranks' local offsets into
// global ones (the only per-read pass; it stays on the device).  The stages then read ONE store named by global ids (hao_ctx.hpp: hao_reads_view).
#pragma once
#include "hao_ctx.hpp"
#include "hao_comm.hpp"
#include "hao_deliver.cuh"      // (hao_dg_term)

// tab = start[W + 1] | pk_base[W + 1] | ns_base[W + 1] | has_n[W]: first global read, first packed byte and first N site of every rank (entry W: the totals), and
// whether the rank sent N-site offsets at all (a rank without N reads sends none: its reads' offsets are its base).  One lane per read, entry n_total included.
__global__ void hao_gather_rebase_kernel(const uint64_t *tab, int W, uint64_t n_total, uint64_t *pk_off, uint64_t *nsite_off)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n_total) return;
	const uint64_t *start = tab, *pkb = tab + (W + 1), *nsb = tab + 2 * (W + 1), *hn = tab + 3 * (W + 1);
	if (i == n_total) { pk_off[i] = pkb[W]; if (nsite_off) nsite_off[i] = nsb[W]; return; }
	int lo = 0, hi = W;      // start[lo] <= i < start[hi]: ends at the one rank that owns read i (ranks without a read have start[r] == start[r + 1])
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (start[mid] <= i) lo = mid; else hi = mid; }
	pk_off[i] += pkb[lo];
	if (nsite_off) nsite_off[i] = hn[lo] ? nsite_off[i] + nsb[lo] : nsb[lo];
}

// ---------------------------------------------------------------------------------------
// hao_reads_digest (include/hao.h).  With term() = hao_dg_term (hao_deliver.cuh), for read r of the view (its id), of L bases and m N sites:
//   bases(r) = term(5, 0, L) + sum_j term(5, j + 1, w_j)      w_j = the j-th little-endian 64-bit word of the read's L / 4 + 1 packed bytes, zero-padded
//   sites(r) = term(6, 0, m) + sum_k term(6, k + 1, site_k)
//   out[0] = sum_r term(7, r, bases(r)),   out[1] = sum_r term(8, r, sites(r))      (mod 2^64)
// Pack offsets only say where the bytes lie: any layout of the same reads gives the same value.  One wave per read: the lanes stride over the words (read
// as aligned words and shifted: a read starts at any byte; the 16 bytes of padding behind every store cover the last word's neighbour), a shuffle reduction,
// the four waves of a block through LDS, one atomic per block and output word.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hao_reads_digest_kernel(hao_read_view V, unsigned long long *out)
{
	const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); const uint32_t lane = threadIdx.x & 63;
	__shared__ uint64_t part[2][4];
	uint64_t b = 0, s = 0;
	if (r < V.n) {
		const uint32_t L = V.len[r]; const uint64_t nb = (uint64_t)L / 4 + 1, nw = (nb + 7) / 8;
		const uintptr_t a = (uintptr_t)(V.packed + V.pk_off[r]); const uint64_t *W = (const uint64_t*)(a & ~(uintptr_t)7); const uint32_t sh = (uint32_t)(a & 7) * 8;
		for (uint64_t j = lane; j < nw; j += 64) {
			uint64_t w = W[j] >> sh; if (sh) w |= W[j + 1] << (64 - sh);
			const uint64_t rem = nb - 8 * j; if (rem < 8) w &= (1ULL << (8 * rem)) - 1;
			b += hao_dg_term(5, j + 1, w);
		}
		uint64_t m = 0;
		if (V.nsite_off) {
			const uint64_t s0 = V.nsite_off[r]; m = V.nsite_off[r + 1] - s0;
			for (uint64_t k = lane; k < m; k += 64) s += hao_dg_term(6, k + 1, V.nsite[s0 + k]);
		}
#pragma unroll
		for (int dl = 32; dl >= 1; dl >>= 1) { b += __shfl_xor(b, dl); s += __shfl_xor(s, dl); }
		b = hao_dg_term(7, r, b + hao_dg_term(5, 0, L)); s = hao_dg_term(8, r, s + hao_dg_term(6, 0, m));
	}
	if (lane == 0) { part[0][threadIdx.x >> 6] = b; part[1][threadIdx.x >> 6] = s; }
	__syncthreads();
	if (threadIdx.x == 0) {
		atomicAdd(out, (unsigned long long)(part[0][0] + part[0][1] + part[0][2] + part[0][3]));
		atomicAdd(out + 1, (unsigned long long)(part[1][0] + part[1][1] + part[1][2] + part[1][3]));
	}
}

static void hao_gather_drop(hao_ctx *c)
{ c->gs_valid = false; c->gs_has_n = false; c->gs_pk_bytes = c->gs_nsites = 0; c->g_packed.release(); c->g_pk_off.release(); c->g_nsite_off.release(); c->g_nsite.release(); }

// all-gather-v of bytes whose parts land where the caller says: rank r's cnt[r] bytes at dst + at[r].  A rank sends at most `chunk` bytes per exchange
// (hao_comm_allgatherv into `stage`, world x chunk bytes; then one device copy per rank into place), so a share beyond 4 GB costs no buffer of its size.
static int hao_gather_bytes(hao_ctx *c, hao_comm &cm, const void *src, const std::vector<uint64_t> &cnt, const std::vector<uint64_t> &at, void *dst, uint64_t chunk, DevBuf<char> &stage)
{
	const int W = cm.world; uint64_t maxc = 0;
	for (int r = 0; r < W; ++r) maxc = std::max(maxc, cnt[r]);
	std::vector<uint64_t> part(W);
	for (uint64_t off = 0; off < maxc; off += chunk) {
		for (int r = 0; r < W; ++r) part[r] = cnt[r] > off ? std::min(chunk, cnt[r] - off) : 0;
		if (int rc = hao_comm_allgatherv(c, cm, (const char*)src + (part[cm.rank] ? off : 0), part[cm.rank], 1, stage.p, part)) return rc;
		uint64_t d = 0;
		for (int r = 0; r < W; ++r) if (part[r]) { HIP_TRY(hipMemcpyAsync((char*)dst + at[r] + off, stage.p + d, part[r], hipMemcpyDeviceToDevice, c->stream)); d += part[r]; }
	}
	return HAO_OK;
}

static int hao_gather_reads_run(hao_ctx *c)
{
	hao_comm &cm = *c->comm; const int W = cm.world;
	// what every rank holds: reads, first global read, packed bytes, N sites (0: it sends no N-site offsets either)
	const uint64_t mine[4] = { c->n_reads, c->rid_base, c->n_pk_bytes, c->has_n ? c->h_nsite_off[c->n_reads] : 0 };
	std::vector<uint64_t> all;
	if (int rc = hao_comm_allgather_u64n(c, cm, mine, 4, all)) return rc;
	std::vector<uint64_t> tab(4 * (size_t)W + 3, 0), c_pk(W), c_off(W), c_nso(W), c_ns(W), a_pk(W), a_off(W), a_ns(W);
	uint64_t *start = tab.data(), *pkb = start + W + 1, *nsb = pkb + W + 1, *hn = nsb + W + 1;
	int local_rc = HAO_OK;
	for (int r = 0; r < W; ++r) {
		const uint64_t *v = &all[4 * (size_t)r];
		if (v[1] != start[r]) { hao_set_err(c, "hao_dist_gather_reads: the shards are not contiguous slices of the reads in rank order (rank " + std::to_string(r) + ")"); local_rc = HAO_EINVAL; }
		start[r + 1] = start[r] + v[0]; pkb[r + 1] = pkb[r] + v[2]; nsb[r + 1] = nsb[r] + v[3]; hn[r] = v[3] != 0;
		c_pk[r] = v[2]; c_off[r] = v[0] * 8; c_nso[r] = v[3] ? v[0] * 8 : 0; c_ns[r] = v[3] * 4;
		a_pk[r] = pkb[r]; a_off[r] = start[r] * 8; a_ns[r] = nsb[r] * 4;
	}
	if (!local_rc && start[W] != c->n_total) { hao_set_err(c, "hao_dist_gather_reads: the shards hold " + std::to_string(start[W]) + " reads, hao_set_shard announced " + std::to_string(c->n_total)); local_rc = HAO_EINVAL; }
	const uint64_t n = c->n_total, PK = pkb[W], NS = nsb[W], chunk = c->sw.gather_chunk;
	uint64_t share = 0; for (int r = 0; r < W; ++r) share = std::max(share, std::max(std::max(c_pk[r], c_off[r]), c_ns[r]));
	DevBuf<char> stage; DevBuf<uint64_t> d_tab;
	auto alloc = [&]() -> int {
		HIP_TRY(c->g_packed.reserve_exact(PK + 16)); HIP_TRY(c->g_pk_off.reserve_exact(n + 1));
		if (NS) { HIP_TRY(c->g_nsite_off.reserve_exact(n + 1)); HIP_TRY(c->g_nsite.reserve_exact(NS + 1)); }
		HIP_TRY(stage.reserve_exact(std::min(chunk, share) * (uint64_t)W + 16)); HIP_TRY(d_tab.reserve_exact(tab.size()));
		HIP_TRY(hipMemsetAsync(c->g_packed.p + PK, 0, 16, c->stream));
		HIP_TRY(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
		return HAO_OK;
	};
	if (!local_rc) local_rc = alloc();
	{ std::vector<uint64_t> st; if (int rc = hao_comm_allgather_u64(c, cm, 0, st, local_rc)) return rc; }      // (the ranks fail together, before the bulk moves)
	if (int rc = hao_gather_bytes(c, cm, c->d_packed.p, c_pk, a_pk, c->g_packed.p, chunk, stage)) return rc;
	if (int rc = hao_gather_bytes(c, cm, c->d_pk_off.p, c_off, a_off, c->g_pk_off.p, chunk, stage)) return rc;
	if (NS) {
		if (int rc = hao_gather_bytes(c, cm, c->d_nsite_off.p, c_nso, a_off, c->g_nsite_off.p, chunk, stage)) return rc;
		if (int rc = hao_gather_bytes(c, cm, c->d_nsite.p, c_ns, a_ns, c->g_nsite.p, chunk, stage)) return rc;
	}
	hipLaunchKernelGGL(hao_gather_rebase_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, (const uint64_t*)d_tab.p, W, n, c->g_pk_off.p, NS ? c->g_nsite_off.p : nullptr);
	local_rc = hipGetLastError() == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess ? HAO_OK : HAO_ENODEV;
	if (local_rc) hao_set_err(c, "hao_dist_gather_reads: the offsets' kernel failed");
	{ std::vector<uint64_t> st; if (int rc = hao_comm_allgather_u64(c, cm, 0, st, local_rc)) return rc; }
	c->gs_valid = true; c->gs_has_n = NS != 0; c->gs_pk_bytes = PK; c->gs_nsites = NS;
	return HAO_OK;
}

extern "C" {

int hao_dist_gather_reads(hao_ctx *c)
{
	if (!c) return HAO_EINVAL;
	if (c->owner) { hao_set_err(c, "hao_dist_gather_reads: not on an attached batch context (hao_attach)"); return HAO_EINVAL; }
	if (!hao_is_sharded(c) || c->gs_valid) return HAO_OK;      // (unsharded: the local store is the whole store, nothing is allocated; valid: nothing to do)
	HIP_TRY(hipSetDevice(c->device));
	++c->index_gen;      // (attached views take the store at their next batch)
	const int rc = hao_gather_reads_run(c);
	if (rc) hao_gather_drop(c);
	return rc;
}

int hao_reads_digest(hao_ctx *c, uint64_t out[2])
{
	if (!c || !out) return HAO_EINVAL;
	if (int rc = hao_view_refresh(c)) return rc;
	HAO_STAGE_VIEW(c, V, "hao_reads_digest needs the bases of all reads");
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(c->d_cursor.reserve(2));
	HIP_TRY(hipMemsetAsync(c->d_cursor.p, 0, 16, c->stream));
	if (V.n) { hipLaunchKernelGGL(hao_reads_digest_kernel, dim3((unsigned)((V.n + 3) / 4)), dim3(256), 0, c->stream, V, c->d_cursor.p); HAO_CHECK_LAUNCH(); }
	HIP_TRY(hipMemcpyAsync(out, c->d_cursor.p, 16, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return HAO_OK;
}

}
