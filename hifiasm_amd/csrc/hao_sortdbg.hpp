// hao_dbg_sort_perm (include/hao.h): the selection's three replays of klib's introsort (hao_chain.cuh) run alone on given keys, so that tests can compare their
// permutations with the reference's own sort on arrays built to reach every path (tests/test_gpu_sortperm.py).  The kernels here only stage keys and call the
// device functions the product calls, inside the LDS declarations of the product's kernels; path 4 is the product's own selection launches.
#pragma once

struct hao_sortdbg_args { const uint64_t *off, *xs; const int32_t *sc; uint32_t *perm, *tmp; int *err; };

// path 0: the sequential replay on lane 0, keys in global memory
template<int MODE>
__global__ __launch_bounds__(64) void hao_sortdbg_seq_kernel(hao_sortdbg_args A)
{
	__shared__ int32_t l_stack[3 * 72];
	const uint64_t o0 = A.off[blockIdx.x]; const int64_t n = (int64_t)(A.off[blockIdx.x + 1] - o0); const int lane = hao_lane();
	uint32_t *pm = A.perm + o0;
	for (int64_t i = lane; i < n; i += 64) pm[i] = (uint32_t)i;
	__threadfence_block();
	hao_sel_ctx S; S.xs = A.xs + o0; S.sc = A.sc + o0; S.al = nullptr; S.pm = pm; S.stack = l_stack; S.pm2 = S.lpos = S.rasc = nullptr;
	if (lane == 0) hao_intro_sort<MODE>(S, n);
}

// path 1: one wave, keys in the wave's LDS slice as chain_select_kernel<1, CAP> holds them
template<int MODE, int CAP>
__global__ __launch_bounds__(64) void hao_sortdbg_wave_kernel(hao_sortdbg_args A)
{
	HAO_SELECT_LDS(1, CAP)
	const uint64_t o0 = A.off[blockIdx.x]; const int64_t n = (int64_t)(A.off[blockIdx.x + 1] - o0); const int lane = hao_lane();
	if (n > CAP) return;      // (the host refuses such a call)
	for (int64_t i = lane; i < n; i += 64) { l_xs[0][i] = A.xs[o0 + i]; l_sc[0][i] = A.sc[o0 + i]; l_al[0][i] = 0; l_pm[0][i] = (uint32_t)i; }
	__threadfence_block();
	hao_sel_ctx S; S.xs = l_xs[0]; S.sc = l_sc[0]; S.al = l_al[0]; S.pm = l_pm[0]; S.stack = l_stack[0]; S.pm2 = l_pm2[0]; S.lpos = l_lp[0]; S.rasc = l_rp[0];
	(void)l_cc;
	hao_wave_intro_sort<MODE>(S, n);
	__threadfence_block();
	for (int64_t i = lane; i < n; i += 64) A.perm[o0 + i] = l_pm[0][i];
}

// path 2: one wave, keys and the sort's three work arrays in global scratch, laid out as hao_select_body<CAP, false> lays out key_tmp (5 words per key)
template<int MODE>
__global__ __launch_bounds__(64) void hao_sortdbg_wave_global_kernel(hao_sortdbg_args A)
{
	__shared__ int32_t l_stack[3 * 72];
	const uint64_t o0 = A.off[blockIdx.x]; const int64_t n = (int64_t)(A.off[blockIdx.x + 1] - o0); const int lane = hao_lane();
	uint32_t *pm = A.perm + o0;
	for (int64_t i = lane; i < n; i += 64) pm[i] = (uint32_t)i;
	__threadfence_block();
	hao_sel_ctx S; S.xs = A.xs + o0; S.sc = A.sc + o0; S.al = nullptr; S.pm = pm; S.stack = l_stack;
	S.pm2 = A.tmp + 5 * o0; S.lpos = A.tmp + 5 * o0 + 2 * n; S.rasc = A.tmp + 5 * o0 + 4 * n;
	hao_wave_intro_sort<MODE>(S, n);
}

// path 3: four waves, keys in LDS as chain_select4_kernel<CAP> holds them; the arrays of the launch's tier only
template<int MODE, int CAP>
__global__ __launch_bounds__(256) void hao_sortdbg_block_kernel(hao_sortdbg_args A, int64_t n_lo, int64_t n_hi)
{
	HAO_SELECT4_LDS(CAP)
	const int tid = threadIdx.x;
	const uint64_t o0 = A.off[blockIdx.x]; const int64_t n = (int64_t)(A.off[blockIdx.x + 1] - o0);
	if (n < n_lo || n >= n_hi) return;
	for (int64_t i = tid; i < n; i += 256) { l_xs[i] = A.xs[o0 + i]; l_sc[i] = A.sc[o0 + i]; l_al[i] = 0; l_pm[i] = (uint32_t)i; }
	__syncthreads();
	hao_sel_ctx S; S.xs = l_xs; S.sc = l_sc; S.al = l_al; S.pm = l_pm; S.stack = l_stack; S.pm2 = l_pm2; S.lpos = l_lp; S.rasc = l_rp;
	(void)l_cc; (void)l_nf; (void)l_lch;
	hao_block_intro_sort<MODE, 4>(S, n, l_segs, HAO_BSORT_MAXSEG(CAP), l_segn, &l_flag, A.err);
	__syncthreads();
	for (int64_t i = tid; i < n; i += 256) A.perm[o0 + i] = l_pm[i];
}

template<int MODE> static hipError_t hao_sortdbg_block_launch(const hao_sortdbg_args &A, uint64_t n_arr, hipStream_t st)
{	// the tiers of the selection (hao_sel_tiers); arrays below the first four-wave tier run in its slice (a pruned read's position sort can be that short)
	hipError_t e; const hao_sel_tier *T = hao_sel_tiers;
	hipLaunchKernelGGL((hao_sortdbg_block_kernel<MODE, 512>), dim3((unsigned)n_arr), dim3(256), 0, st, A, (int64_t)0, T[1].n_hi);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL((hao_sortdbg_block_kernel<MODE, 1024>), dim3((unsigned)n_arr), dim3(256), 0, st, A, T[2].n_lo, T[2].n_hi);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL((hao_sortdbg_block_kernel<MODE, 2048>), dim3((unsigned)n_arr), dim3(256), 0, st, A, T[3].n_lo, T[3].n_hi);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL((hao_sortdbg_block_kernel<MODE, 4096>), dim3((unsigned)n_arr), dim3(256), 0, st, A, T[4].n_lo, T[4].n_hi);
	return hipGetLastError();
}

template<int MODE> static int hao_sortdbg_run(hao_ctx *c, int path, int variant, uint64_t n_arr, const hao_sortdbg_args &A)
{
	const dim3 g((unsigned)n_arr);
	if (path == HAO_SORTDBG_SEQ) hipLaunchKernelGGL((hao_sortdbg_seq_kernel<MODE>), g, dim3(64), 0, c->stream, A);
	else if (path == HAO_SORTDBG_WAVE_LDS && variant == 0) hipLaunchKernelGGL((hao_sortdbg_wave_kernel<MODE, 128>), g, dim3(64), 0, c->stream, A);
	else if (path == HAO_SORTDBG_WAVE_LDS) hipLaunchKernelGGL((hao_sortdbg_wave_kernel<MODE, 1024>), g, dim3(64), 0, c->stream, A);
	else if (path == HAO_SORTDBG_WAVE_GLOBAL) hipLaunchKernelGGL((hao_sortdbg_wave_global_kernel<MODE>), g, dim3(64), 0, c->stream, A);
	else HIP_TRY(hao_sortdbg_block_launch<MODE>(A, n_arr, c->stream));
	HAO_CHECK_LAUNCH();
	return HAO_OK;
}

extern "C" int hao_dbg_sort_perm(hao_ctx *c, int mode, int path, int variant, uint64_t n_arr, const uint64_t *off, const uint64_t *xs, const int32_t *sc, uint32_t *perm)
{
	if (!c || !off || !perm || mode < 0 || mode > 1 || path < HAO_SORTDBG_SEQ || path > HAO_SORTDBG_SELECT || variant < 0 || variant > 1 || n_arr >= (1ULL << 31)) return HAO_EINVAL;
	if (path == HAO_SORTDBG_SELECT && mode != 1) { hao_set_err(c, "hao_dbg_sort_perm: the selection without pruning runs the position sort only (mode 1)"); return HAO_EINVAL; }
	if (off[0] != 0) return HAO_EINVAL;
	const int64_t cap = path == HAO_SORTDBG_WAVE_LDS ? (variant ? 1024 : 128) : path == HAO_SORTDBG_BLOCK ? hao_sel_tiers[4].n_hi - 1 : (int64_t)1 << 24;
	for (uint64_t a = 0; a < n_arr; ++a) {
		if (off[a + 1] < off[a]) { hao_set_err(c, "hao_dbg_sort_perm: offsets do not ascend"); return HAO_EINVAL; }
		if ((int64_t)(off[a + 1] - off[a]) > cap) { hao_set_err(c, "hao_dbg_sort_perm: an array longer than the path holds"); return HAO_EINVAL; }
	}
	const uint64_t N = off[n_arr];
	if (n_arr == 0) return HAO_OK;
	if ((N && (!xs || !sc)) || N >= (1ULL << 31)) return HAO_EINVAL;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf<uint64_t> d_off, d_xs; DevBuf<int32_t> d_sc; DevBuf<uint32_t> d_perm, d_tmp; DevBuf<int> d_err;
	HIP_TRY(d_off.reserve(n_arr + 2)); HIP_TRY(d_xs.reserve(N + 1)); HIP_TRY(d_sc.reserve(N + 1)); HIP_TRY(d_perm.reserve(N + 1)); HIP_TRY(d_tmp.reserve(5 * N + 8)); HIP_TRY(d_err.reserve(2));
	HIP_TRY(hipMemcpyAsync(d_off.p, off, (n_arr + 1) * 8, hipMemcpyHostToDevice, c->stream));
	if (N) { HIP_TRY(hipMemcpyAsync(d_xs.p, xs, N * 8, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(d_sc.p, sc, N * 4, hipMemcpyHostToDevice, c->stream)); }
	HIP_TRY(hipMemsetAsync(d_err.p, 0, 8, c->stream)); HIP_TRY(hipMemsetAsync(d_perm.p, 0xff, (N + 1) * 4, c->stream));
	if (path != HAO_SORTDBG_SELECT) {
		hao_sortdbg_args A; A.off = d_off.p; A.xs = d_xs.p; A.sc = d_sc.p; A.perm = d_perm.p; A.tmp = d_tmp.p; A.err = d_err.p;
		if (int rc = mode == 0 ? hao_sortdbg_run<0>(c, path, variant, n_arr, A) : hao_sortdbg_run<1>(c, path, variant, n_arr, A)) return rc;
	} else {
		// the selection itself over one synthetic read per array: max_n_chain above every n (no score sort, no pruning), chain_cutoff 0 (no weak-chain filter):
		// perm / n_final are the position sort's result through the tiers' own kernels
		std::vector<hao_ovlp_t> rec(N + 1); std::vector<uint64_t> ident(n_arr + 2), zeros(n_arr + 2, 0); std::vector<uint32_t> len(n_arr + 1, 1u << 20);
		memset(rec.data(), 0, (N + 1) * sizeof(hao_ovlp_t));
		for (uint64_t i = 0; i < N; ++i) { rec[i].x_pos_s = (uint32_t)(xs[i] >> 32); rec[i].x_pos_e = (uint32_t)xs[i]; rec[i].shared_seed = sc[i]; rec[i].align_length = 1; }
		for (uint64_t a = 0; a < n_arr + 2; ++a) ident[a] = a;
		DevBuf<hao_ovlp_t> d_ol; DevBuf<uint64_t> d_goff, d_zero, d_kxs, d_fcf, d_cc; DevBuf<int32_t> d_ksc; DevBuf<uint32_t> d_kal, d_len, d_nf;
		HIP_TRY(d_ol.reserve(N + 1)); HIP_TRY(d_goff.reserve(n_arr + 2)); HIP_TRY(d_zero.reserve(n_arr + 2)); HIP_TRY(d_kxs.reserve(N + 1)); HIP_TRY(d_ksc.reserve(N + 1)); HIP_TRY(d_kal.reserve(N + 1));
		HIP_TRY(d_len.reserve(n_arr + 1)); HIP_TRY(d_nf.reserve(n_arr + 2)); HIP_TRY(d_fcf.reserve(n_arr + 2)); HIP_TRY(d_cc.reserve(8));
		HIP_TRY(hipMemcpyAsync(d_ol.p, rec.data(), (N + 1) * sizeof(hao_ovlp_t), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_goff.p, ident.data(), (n_arr + 2) * 8, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_zero.p, zeros.data(), (n_arr + 2) * 8, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_len.p, len.data(), (n_arr + 1) * 4, hipMemcpyHostToDevice, c->stream));
		hao_sel_args sa; memset(&sa, 0, sizeof(sa));
		sa.ol = d_ol.p; sa.g_off = d_goff.p; sa.ch_base = d_off.p; sa.cl_base = d_zero.p; sa.n_sel = n_arr; sa.rid_lo = 0; sa.len = d_len.p; sa.cc_off = d_zero.p; sa.cc = d_cc.p;
		sa.key_xs = d_kxs.p; sa.key_sc = d_ksc.p; sa.key_al = d_kal.p; sa.key_tmp = d_tmp.p; sa.perm = d_perm.p; sa.n_final = d_nf.p; sa.fc_final = d_fcf.p;
		sa.max_n_chain = 1ULL << 40; sa.ocv_w = 3072; sa.chain_cutoff = 0; sa.err = d_err.p;
		HIP_TRY(hao_select_launch(sa, n_arr, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));      // (rec and friends are read by the copies above)
		std::vector<uint32_t> nf(n_arr + 1);
		HIP_TRY(hipMemcpy(nf.data(), d_nf.p, n_arr * 4, hipMemcpyDeviceToHost));
		for (uint64_t a = 0; a < n_arr; ++a) if (nf[a] != off[a + 1] - off[a]) { hao_set_err(c, "hao_dbg_sort_perm: the selection dropped chains"); return HAO_EUNSUPP; }
	}
	int herr[2] = { 0, 0 };
	HIP_TRY(hipMemcpyAsync(herr, d_err.p, 8, hipMemcpyDeviceToHost, c->stream));
	if (N) HIP_TRY(hipMemcpyAsync(perm, d_perm.p, N * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (herr[0]) { hao_set_err(c, "selection sort: more sub-ranges alive in one level than its list holds"); return HAO_EUNSUPP; }
	return HAO_OK;
}
