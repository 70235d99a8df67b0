// mf_certified.hip.h -- host side of the certified matrix-core passes: top-1 (recommend_mfma2_kernel),
// top-N and similar items (topn_mfma_kernel), held-out ranks (rank_mfma_kernel).  What the three launches share is written
// here once -- the shape rule, the kernel instance of a shape, the norm prologue, the two-per-CU and item-split rules, the
// tail -- and each launch below states only what is its own.
#pragma once

namespace {

// ---- the shape rule: K -> instance <NC, QC, TU, WAVES> of a family, K = 4 * NC * QC.  waves == 0: no matrix-core form.
// K = 20 NC <= 100 in 20-deep chunks and K = 16 NC <= 96 in 16-deep ones, four waves of 32 users; K = 256 in 32-deep chunks,
// eight waves of 16 users.  K = 112 and 128 are the one difference between the families (`wide`): top-1 keeps them on four
// waves <7, 4> / <8, 4>; top-N and ranks move them to eight <7, 4, 1, 8> / <4, 8, 1, 8>, because at 32 users per wave
// the list walk (the counters) beside 224 / 256 VGPRs of L operand spills.  K % 20 is tested first: K = 80 is 4 x 20.
struct mfma_shape {
	int nc = 0, qc = 0, waves = 0;
};

inline mfma_shape certified_shape(int K, bool wide)
{
	if (K % 20 == 0 && K <= mf::kHKmax) return {K / 20, 5, 4};
	if (K % 16 == 0 && K <= 96) return {K / 16, 4, 4};
	if (K == 112) return {7, 4, wide ? 8 : 4};
	if (K == 128) return wide ? mfma_shape{4, 8, 8} : mfma_shape{8, 4, 4};
	if (K == 256) return {8, 8, 8};
	return {};
}

// ---- the families: the argument struct, where K = 112 and 128 go, and the kernel template under one name
struct top1_family {
	using Args = mf::RecMfmaArgs;
	static constexpr bool kWide = false;
	template <int NC, int QC = 5, int TU = 2, int WAVES = 4>
	static constexpr auto fn() { return &mf::recommend_mfma2_kernel<NC, QC, TU, WAVES>; }
};
struct topn_family {
	using Args = mf::TopnArgs;
	static constexpr bool kWide = true;
	template <int NC, int QC = 5, int TU = 2, int WAVES = 4>
	static constexpr auto fn() { return &mf::topn_mfma_kernel<NC, QC, TU, WAVES>; }
};
struct rank_family {
	using Args = mf::RankArgs;
	static constexpr bool kWide = true;
	template <int NC, int QC = 5, int TU = 2, int WAVES = 4>
	static constexpr auto fn() { return &mf::rank_mfma_kernel<NC, QC, TU, WAVES>; }
};

// the family's instance of a shape certified_shape(K, F::kWide) gave; exactly the instances named here are compiled
template <class F>
auto certified_kernel(const mfma_shape &s) -> void (*)(typename F::Args)
{
	typedef void (*Fn)(typename F::Args);
	if (s.qc == 5) {
		static const Fn f20[5] = {F::template fn<1>(), F::template fn<2>(), F::template fn<3>(), F::template fn<4>(),
		                          F::template fn<5>()};
		return f20[s.nc - 1];
	}
	if (s.waves == 4) {
		static const Fn f16[6] = {F::template fn<1, 4>(), F::template fn<2, 4>(), F::template fn<3, 4>(),
		                          F::template fn<4, 4>(), F::template fn<5, 4>(), F::template fn<6, 4>()};
		if constexpr (!F::kWide)
			if (s.nc > 6) return s.nc == 7 ? F::template fn<7, 4>() : F::template fn<8, 4>();
		return f16[s.nc - 1];
	}
	if constexpr (F::kWide) {
		if (s.qc == 4) return F::template fn<7, 4, 1, 8>();
		if (s.nc == 4) return F::template fn<4, 8, 1, 8>();
	}
	return F::template fn<8, 8, 1, 8>();
}

// the kernels compute row offsets into R in 32 bits
inline bool fits32(int items, int ldr) { return (unsigned long long) items * (unsigned long long) ldr * 8ull < (1ull << 32); }

// ---- the norm prologue: clears the largest-norm word and the exact-pass count, then the norm of every row of L and the
// largest norm of a row of R
inline int certified_norms(mf_plan *p, const double *L, int rows, int ldl, double *lnorm, const double *R, int items, int ldr,
                           unsigned long long *rmax_bits, int *ucount)
{
	MF_HIP(hipMemsetAsync(rmax_bits, 0, sizeof(unsigned long long), p->stream));
	MF_HIP(hipMemsetAsync(ucount, 0, sizeof(int), p->stream));
	hipLaunchKernelGGL(mf::row_norm_kernel, dim3((rows + 63) / 64), dim3(64), 0, p->stream, L, rows, p->K, ldl, lnorm,
	                   (unsigned long long *) nullptr);
	if (items > 0)
		hipLaunchKernelGGL(mf::row_norm_kernel, dim3((items + 63) / 64), dim3(64), 0, p->stream, R, items, p->K, ldr,
		                   (double *) nullptr, rmax_bits);
	return MF_OK;
}

// ---- two four-wave workgroups per CU while the ring, the pass's dynamic LDS beside it and its static arrays (the
// caller's allowance) fit half of the CU's 160 KB
inline bool two_per_cu(int waves, size_t lds, size_t static_allowance) { return waves == 4 && lds + static_allowance <= 80 * 1024; }

// ---- the item split of small problems.  A workgroup owns `blocks`' worth of rows and ALL items, so few rows leave most
// of the chip idle (cfg3: 48 workgroups on 256 CUs).  The items are then split over gridDim.y -- whole 128-item tiles,
// about `chip` workgroups in all (the number the chip holds at once, times two) -- and the per-split reports merged by
// the pass's own kernel.  MF_RECOMMEND_SPLIT: 0 never, n > 0 that many.
struct item_split {
	int nsplit = 1, split_items = 0;   // split_items 0: no split, else a multiple of 128
};

inline item_split certified_split(const mf_config &cfg, int blocks, int tiles, int chip)
{
	item_split s;
	if (cfg.rec_split != 0 && blocks < chip * 3 / 8 && tiles >= 2) {
		s.nsplit = cfg.rec_split > 0 ? cfg.rec_split : (chip + blocks - 1) / blocks;
		s.nsplit = std::max(1, std::min(s.nsplit, tiles));
	}
	if (s.nsplit > 1) {
		const int tiles_per = (tiles + s.nsplit - 1) / s.nsplit;
		s.nsplit = (tiles + tiles_per - 1) / tiles_per;
		s.split_items = tiles_per * mf::kMI;
	}
	return s;
}

// ---- the tail: the number of rows the pass could not decide, and the exact pass over them (`exact(count)` launches it)
template <class Exact>
int certified_tail(mf_plan *p, const int *ucount, int64_t *uncertain, Exact exact)
{
	int cnt = 0;
	MF_HIP(hipMemcpyAsync(&cnt, ucount, sizeof(int), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	*uncertain = cnt;
	if (cnt > 0) {
		exact(cnt);
		MF_HIP(hipGetLastError());
	}
	return MF_OK;
}

// the recommendation mask: item ids ascending inside every user's row
inline const int *mask_index(const mf_plan *p) { return p->mask_idx ? p->mask_idx : p->csr_idx; }

// recommend_kernel's arguments on this plan: `users` users (those of `ulist`, or all), the scan state into `cand` if given
inline mf::RecArgs exact_args(const mf_plan *p, int users, const int *ulist, mf_candidate *cand)
{
	mf::RecArgs ex;
	ex.users = users;
	ex.items = p->items;
	ex.K = p->K;
	ex.ldl = p->ldl;
	ex.ldr = p->ldr;
	ex.L = p->Lbuf[p->cur];
	ex.R = p->Rbuf[p->cur];
	ex.csr_ptr = p->csr_ptr;
	ex.csr_idx = mask_index(p);
	ex.best = p->best_dev;
	ex.ulist = ulist;
	ex.cand = cand;
	return ex;
}

// Pass 1 of the recommendation: row norms + recommend_mfma_kernel.  filt == nullptr: the kernel certifies per user
// against THIS plan's items (best / list of uncertain users); filt != nullptr: it only reports (best, second, arg,
// non-finite flag) per user, for a certification over several item blocks by the caller (2-D tiles).  The tail is the
// caller's (mf_plan_recommend): it copies `best` in the same synchronisation as the count.
int launch_recommend_pass1(mf_plan *p, mf_filter *filt)
{
	const double *Lc = p->Lbuf[p->cur], *Rc = p->Rbuf[p->cur];
	// pass 1: scores on the FP64 matrix cores + certification margin; pass 2: exact re-scoring of the rest
	const int rcn = certified_norms(p, Lc, p->uc, p->ldl, p->lnorm, Rc, p->items, p->ldr, p->rmax_bits, p->ucount);
	if (rcn != MF_OK) return rcn;
	mf::RecMfmaArgs m;
	m.users = p->uc;
	m.items = p->items;
	m.K = p->K;
	m.ldl = p->ldl;
	m.ldr = p->ldr;
	m.L = Lc;
	m.R = Rc;
	m.csr_ptr = p->csr_ptr;
	m.csr_idx = mask_index(p);
	m.lnorm = p->lnorm;
	m.rnorm_max_bits = p->rmax_bits;
	m.thr_scale = mf_backend_recommend_margin(p->K);
	m.best = p->best_dev;
	m.ulist = p->ulist;
	m.ucount = p->ucount;
	m.filt = filt;
	// Form.  The L block's image stays resident in LDS (it is the same for every item tile) whenever it fits
	// beside the two R buffers, and the R chunks then go global -> LDS by LDS-DMA (even K): K <= 64 with 32-deep
	// chunks, up to K = 100 with 24- or 20-deep ones -- the depth with the fewest chunks wins, an exact divisor
	// of K on ties (K=100: 5 x 20 instead of 32+32+32+4).  Larger K: both operands staged through registers.
	// Measured on 1e6 x 1e5 (profiles/r01/recommend_resident_L_ab.txt): K=100 55.4 vs 48.9 TFLOP/s, K=64 54.3
	// vs 50.2, K=30 41.1 vs 37.7.
	typedef void (*RecFn)(mf::RecMfmaArgs);
	const bool vec = (p->K & 1) == 0;
	const bool allow = p->cfg.rec_ares;              // MF_RECOMMEND_ARES=0 disables the resident-L form (tests, A/B)
	const bool allow_dma = vec && p->cfg.rec_bdma;   // MF_RECOMMEND_BDMA=0: stage R chunks through registers (A/B)
	const size_t static_lds = 8 * 1024, cu_lds = 160 * 1024;   // masks + merge arrays, rounded up
	int kc = 32;
	bool ares = false;
	if (allow) {
		int best_nch = 1 << 30;
		for (int cand : {32, 24, 20}) {
			if (cand == 24 && !allow_dma) continue;                    // 24 exists in the DMA form only
			if (cand == 20 && p->K % 20 != 0 && !allow_dma) continue;   // register form: exact multiples only
			if (mf::rec_mfma_lds(p->K, cand, true) + static_lds > cu_lds) continue;
			const int nch = (p->K + cand - 1) / cand;
			if (nch < best_nch || (nch == best_nch && p->K % cand == 0 && p->K % kc != 0)) {
				best_nch = nch;
				kc = cand;
				ares = true;
			}
		}
	}
	const bool bdma = ares && allow_dma;
	RecFn fn;
	if (kc == 24)
		fn = mf::recommend_mfma_kernel<true, 24, true, true>;
	else if (kc == 20)   // even K here
		fn = bdma ? mf::recommend_mfma_kernel<true, 20, true, true> : mf::recommend_mfma_kernel<true, 20, true, false>;
	else if (bdma)
		fn = mf::recommend_mfma_kernel<true, 32, true, true>;
	else
		fn = ares ? (vec ? mf::recommend_mfma_kernel<true, 32, true> : mf::recommend_mfma_kernel<false, 32, true>)
		          : (vec ? mf::recommend_mfma_kernel<true, 32, false> : mf::recommend_mfma_kernel<false, 32, false>);
	size_t lds = mf::rec_mfma_lds(p->K, kc, ares);
	// K = 20, 40, .. 100 (a wave's L operand fits its registers; whole 20-deep chunks): workgroups of 64 users, two per CU,
	// whose barriers / arg-max steps / mask walks overlap each other's matrix instructions, with a gapless matrix stream
	// per wave.  K=100: 64.7 vs 57.6 TFLOP/s on the 131072 x 100000 probe, K=80 64.3 vs 57.4, K=40 57.7 vs 52.1, K=20 49.7 vs
	// 45.0.  Its general form (any even K <= 100, MF_RECOMMEND_HALF=all) has branches on K in the tile body that defeat
	// hipcc's s_waitcnt placement and is slower than the 128-user kernel (K=64: 51.7 vs 58.5): not chosen by the rule.
	// The same kernel with 16-deep chunks for K = 16, 32, .. 128 (two per CU as well) and, for K = 256, with 16 users per
	// wave and eight waves per workgroup (one per CU): DESIGN.md 5.8.
	RecFn hfn = nullptr;
	mfma_shape hs;
	if (vec && allow_dma && p->cfg.rec_half && fits32(p->items, p->ldr)) {
		hs = certified_shape(p->K, top1_family::kWide);
		if (hs.waves)
			hfn = certified_kernel<top1_family>(hs);
		else if (p->cfg.rec_half == 2 && p->K <= mf::kHKmax) {
			hfn = mf::recommend_mfma2_kernel<0>;
			hs = {0, 5, 4};
		}
	}
	const bool half = hfn != nullptr;
	int block_users = mf::kMU, threads = mf::kMThreads;
	if (half) {
		fn = hfn;
		lds = mf::rec_mfma2_lds(hs.qc);
		block_users = mf::kHU;
		threads = 64 * hs.waves;
	}
	p->rec_half_used = half;
	MF_HIP(raise_lds_limit((const void *) fn, lds));
	// the half-size four-wave workgroups run two per CU; the per-split top-2 reports are merged and certified by
	// merge_splits_kernel
	const int ublocks = (p->uc + block_users - 1) / block_users, tiles = (p->items + mf::kMI - 1) / mf::kMI;
	const item_split sp = certified_split(p->cfg, ublocks, tiles, half && hs.waves == 4 ? 1024 : 512);
	m.split_items = sp.split_items;
	m.part = nullptr;
	if (sp.nsplit > 1) {
		const int rc = p->part_dev.grow((size_t) sp.nsplit * (size_t) p->uc);
		if (rc != MF_OK) return rc;
		m.part = p->part_dev;
	}
	hipLaunchKernelGGL(fn, dim3(ublocks, sp.nsplit), dim3(threads), lds, p->stream, m);
	MF_HIP(hipGetLastError());
	if (sp.nsplit > 1) {
		hipLaunchKernelGGL(mf::merge_splits_kernel, dim3((p->uc + 255) / 256), dim3(256), 0, p->stream, m, sp.nsplit);
		MF_HIP(hipGetLastError());
	}
	return MF_OK;
}

// Top-N on the device: rows of n items / scores per row of the operands' L in o.out->items / scores (nothing copied
// back).  Matrix-core pass (topn_mfma_kernel) with certification and exact re-scoring of the members, the exact pass
// (topn_exact_kernel) for every row it cannot decide; the exact pass for all rows under MF_RECOMMEND_IMPL=exact or
// when K has no matrix-core form.  The plan gives the device, the stream, K and the environment switches only: what is
// ranked against what, under which mask and into which buffers is the operands' (mf_plan_recommend_topn: the users
// against the items under the rated mask; mf_plan_similar_items: items against items under the self mask).
int launch_topn_core(mf_plan *p, const topn_operands &o, int n)
{
	MF_HIP(hipSetDevice(p->device));
	topn_buffers &b = *o.out;
	{
		const int rc = grow_all((size_t) o.rows * (size_t) n, b.items, b.scores);
		if (rc != MF_OK) return rc;
	}
	mf::TopnArgs a;
	memset(&a, 0, sizeof a);
	a.users = o.rows;
	a.items = o.items;
	a.K = p->K;
	a.ldl = o.ldl;
	a.ldr = o.ldr;
	a.L = o.L;
	a.R = o.R;
	a.csr_ptr = o.mask_ptr;
	a.csr_idx = o.mask_idx;
	a.lnorm = o.lnorm;
	a.rnorm_max_bits = o.rmax_bits;
	a.thr_scale = mf_backend_recommend_margin(p->K);
	a.n = n;
	a.out_items = b.items;
	a.out_scores = b.scores;
	a.olist = o.ulist;
	a.ocount = o.ucount;

	mfma_shape s;
	if (!p->cfg.rec_exact && fits32(o.items, o.ldr) && o.items > 0) s = certified_shape(p->K, topn_family::kWide);
	if (!s.waves) {
		hipLaunchKernelGGL(mf::topn_exact_kernel, dim3(o.rows), dim3(64), 0, p->stream, a);
		MF_HIP(hipGetLastError());
		b.last_uncertain = -1;
		b.form = 0;
		return MF_OK;
	}
	void (*const fn)(mf::TopnArgs) = certified_kernel<topn_family>(s);

	int rc = certified_norms(p, a.L, o.rows, o.ldl, o.lnorm, a.R, o.items, o.ldr, o.rmax_bits, o.ucount);
	if (rc != MF_OK) return rc;
	const size_t lds = mf::rec_mfma2_lds(s.qc) + mf::topn_list_lds(n);   // the lists sit beside the ring
	MF_HIP(raise_lds_limit((const void *) fn, lds));
	constexpr size_t kStaticLds = 3 * 1024;   // topn_mfma_kernel's static arrays, rounded up
	const bool two = two_per_cu(s.waves, lds, kStaticLds);
	b.form = two ? 1 : 2;

	const int ublocks = (o.rows + mf::kHU - 1) / mf::kHU, tiles = (o.items + mf::kMI - 1) / mf::kMI;
	const item_split sp = certified_split(p->cfg, ublocks, tiles, two ? 1024 : 512);
	if (sp.nsplit > 1) {
		a.split_items = sp.split_items;
		a.nsplit = sp.nsplit;
		rc = grow_all((size_t) o.rows * (size_t) (sp.nsplit + 1) * (size_t) (n + 1), b.part_v, b.part_i);
		if (rc == MF_OK) rc = b.part_bad.grow((size_t) o.rows * (size_t) sp.nsplit);
		if (rc != MF_OK) return rc;
		a.part_v = b.part_v;
		a.part_i = b.part_i;
		a.part_bad = b.part_bad;
	}
	hipLaunchKernelGGL(fn, dim3(ublocks, sp.nsplit), dim3(64 * s.waves), lds, p->stream, a);
	MF_HIP(hipGetLastError());
	if (sp.nsplit > 1) {
		hipLaunchKernelGGL(mf::topn_merge_kernel, dim3((o.rows + 255) / 256), dim3(256), 0, p->stream, a);
		MF_HIP(hipGetLastError());
	}
	return certified_tail(p, o.ucount, &b.last_uncertain, [&](int cnt) {
		a.ulist = o.ulist;
		hipLaunchKernelGGL(mf::topn_exact_kernel, dim3(cnt), dim3(64), 0, p->stream, a);
	});
}

// mf_plan_recommend_topn's operands: this shard's users against the items under the rated mask
int launch_topn(mf_plan *p, int n)
{
	topn_operands o;
	o.rows = p->uc;
	o.items = p->items;
	o.L = p->Lbuf[p->cur];
	o.R = p->Rbuf[p->cur];
	o.ldl = p->ldl;
	o.ldr = p->ldr;
	o.mask_ptr = p->csr_ptr;
	o.mask_idx = mask_index(p);
	o.lnorm = p->lnorm;
	o.rmax_bits = p->rmax_bits;
	o.ulist = p->ulist;
	o.ucount = p->ucount;
	o.out = &p->topn;
	return launch_topn_core(p, o, n);
}

// mf_plan_similar_items on the device: Q (cosine: similar_normalize_kernel into the plan's buffer; dot: R itself), the
// self mask and, for a listed query, the gathered rows (similar_gather_kernel), then the top-N pass on those operands.
// Rows of n items / scores per query in p->sim.items / p->sim.scores.
int launch_similar(mf_plan *p, int metric, const int32_t *query, int nq, int n)
{
	MF_HIP(hipSetDevice(p->device));
	const double *Q = p->Rbuf[p->cur];
	if (metric == MF_SIMILAR_COSINE) {
		const int rc = p->sim_q.grow((size_t) p->items * (size_t) p->ldr);
		if (rc != MF_OK) return rc;
		hipLaunchKernelGGL(mf::similar_normalize_kernel, dim3((p->items + mf::kSimRows - 1) / mf::kSimRows), dim3(mf::kSimThreads), 0,
		                   p->stream, p->Rbuf[p->cur], p->items, p->K, p->ldr, p->sim_q);
		MF_HIP(hipGetLastError());
		Q = p->sim_q;
	}
	const int ldb = row_pitch(p->cfg, p->K, p->sweep.dma != 0);   // the pitch the plan gives an L buffer of its own
	int rc = p->sim_ptr.grow((size_t) nq + 1);
	if (rc == MF_OK) rc = grow_all((size_t) nq, p->sim_idx, p->sim_lnorm, p->sim_ulist);
	if (rc == MF_OK && query) rc = p->sim_query.grow((size_t) nq);
	if (rc == MF_OK && query) rc = p->sim_block.grow((size_t) nq * (size_t) ldb);
	if (rc != MF_OK) return rc;
	if (query) MF_HIP(hipMemcpyAsync(p->sim_query, query, (size_t) nq * sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
	hipLaunchKernelGGL(mf::similar_gather_kernel, dim3((nq + 63) / 64), dim3(64), 0, p->stream, Q, p->ldr, p->K,
	                   query ? p->sim_query : (const int *) nullptr, nq, p->sim_block, ldb, p->sim_ptr, p->sim_idx);
	MF_HIP(hipGetLastError());
	topn_operands o;
	o.rows = nq;
	o.items = p->items;
	o.L = query ? p->sim_block : Q;
	o.R = Q;
	o.ldl = query ? ldb : p->ldr;
	o.ldr = p->ldr;
	o.mask_ptr = p->sim_ptr;
	o.mask_idx = p->sim_idx;
	o.lnorm = p->sim_lnorm;
	o.rmax_bits = p->rmax_bits;   // one word each, reset by every pass that uses them
	o.ulist = p->sim_ulist;
	o.ucount = p->ucount;
	o.out = &p->sim;
	return launch_topn_core(p, o, n);
}

// Ranks of the held-out entries on the device, in the plan's bucketed order, in p->rank_out (nothing copied back).
// Thresholds (rank_threshold_kernel), the matrix-core counting pass over blocks of 64 entries (rank_mfma_kernel),
// certification (rank_finish_kernel) and the exact pass (rank_exact_kernel) for the entries it cannot decide; the exact
// pass for all entries under MF_RECOMMEND_IMPL=exact, when K has no matrix-core form or when R exceeds 32-bit row offsets.
int launch_rank(mf_plan *p)
{
	MF_HIP(hipSetDevice(p->device));
	const size_t n = (size_t) p->ho_nnz;
	int rc = grow_all(n, p->rank_score, p->rank_state, p->rank_out, p->rank_above, p->rank_band, p->rank_list);
	if (rc != MF_OK) return rc;
	mf::RankArgs a;
	memset(&a, 0, sizeof a);
	a.rows = (int) n;
	a.items = p->items;
	a.K = p->K;
	a.ldl = p->ldl;
	a.ldr = p->ldr;
	a.L = p->Lbuf[p->cur];
	a.R = p->Rbuf[p->cur];
	a.csr_ptr = p->csr_ptr;
	a.csr_idx = mask_index(p);
	a.ent_user = p->ho_user;
	a.ent_item = p->ho_idx;
	a.lnorm = p->lnorm;
	a.rnorm_max_bits = p->rmax_bits;
	a.thr_scale = mf_backend_recommend_margin(p->K);
	a.score = p->rank_score;
	a.state = p->rank_state;
	a.rank = p->rank_out;
	a.above = p->rank_above;
	a.band = p->rank_band;
	a.olist = p->rank_list;
	a.ocount = p->ucount;
	const unsigned eblocks = (unsigned) ((n + 255) / 256);
	hipLaunchKernelGGL(mf::rank_threshold_kernel, dim3(eblocks), dim3(256), 0, p->stream, a);
	MF_HIP(hipGetLastError());

	mfma_shape s;
	if (!p->cfg.rec_exact && fits32(p->items, p->ldr)) s = certified_shape(p->K, rank_family::kWide);
	if (!s.waves) {
		hipLaunchKernelGGL(mf::rank_exact_kernel, dim3((unsigned) n), dim3(64), 0, p->stream, a);
		MF_HIP(hipGetLastError());
		p->last_rank_uncertain = -1;
		p->rank_form = 0;
		return MF_OK;
	}
	void (*const fn)(mf::RankArgs) = certified_kernel<rank_family>(s);

	rc = certified_norms(p, a.L, p->uc, p->ldl, p->lnorm, a.R, p->items, p->ldr, p->rmax_bits, p->ucount);
	if (rc != MF_OK) return rc;
	const size_t lds = mf::rec_mfma2_lds(s.qc);
	MF_HIP(raise_lds_limit((const void *) fn, lds));
	constexpr size_t kStaticLds = 4 * 1024;   // rank_mfma_kernel's static arrays, rounded up
	const bool two = two_per_cu(s.waves, lds, kStaticLds);
	p->rank_form = two ? 1 : 2;

	const int rblocks = (int) ((n + mf::kHU - 1) / mf::kHU), tiles = (p->items + mf::kMI - 1) / mf::kMI;
	const item_split sp = certified_split(p->cfg, rblocks, tiles, two ? 1024 : 512);
	a.split_items = sp.split_items;
	hipLaunchKernelGGL(fn, dim3(rblocks, sp.nsplit), dim3(64 * s.waves), lds, p->stream, a);
	MF_HIP(hipGetLastError());
	hipLaunchKernelGGL(mf::rank_finish_kernel, dim3(eblocks), dim3(256), 0, p->stream, a);
	MF_HIP(hipGetLastError());
	return certified_tail(p, p->ucount, &p->last_rank_uncertain, [&](int cnt) {
		a.elist = p->rank_list;
		hipLaunchKernelGGL(mf::rank_exact_kernel, dim3(cnt), dim3(64), 0, p->stream, a);
	});
}

}  // namespace
