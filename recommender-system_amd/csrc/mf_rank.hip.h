// mf_rank.hip.h -- where the held-out items land in each user's recommendation order (mf_plan_rank_heldout): the exact
// score of every held-out pair as its threshold, a matrix-core pass over L R^T that COUNTS the open items above each
// threshold instead of selecting, certification of the counts with the margin of the top-1 step, and an exact pass for
// every entry the matrix cores cannot decide.
//
// Semantics (include/matfact_hip.h, mf_plan_rank_heldout): for entry (i, j) with j among the items user i has not rated
// and B[i][j] not NaN, rank = #{ open j' != j : B[i][j'] > B[i][j] or (B[i][j'] == B[i][j] and j' < j) }, B exactly as
// mat2d_prod forms it; MF_RANK_MASKED when j is rated, MF_RANK_NAN when B[i][j] is NaN.
//
// A kernel row is one held-out entry (the entries in the plan's bucketed order, so the rows of a user are neighbours and
// load the same L row).  Matrix-core form: the K families of topn_mfma_kernel; every other K runs the exact form.
#pragma once
#include "mf_common.hip.h"
#include "mf_ring.hip.h"
#include "mf_topn.hip.h"        // topn_exact_score

namespace mf {

constexpr int kRankMasked = -1, kRankNan = -2;   // MF_RANK_MASKED, MF_RANK_NAN

struct RankArgs {
	int rows;                                  // held-out entries
	int items, K;
	int ldl, ldr;                              // row pitch of L and of R in doubles (>= K)
	const double *__restrict__ L;
	const double *__restrict__ R;
	const int *__restrict__ csr_ptr;
	const int *__restrict__ csr_idx;           // item ids ascending within a user (the recommend mask)
	const int *__restrict__ ent_user;          // local user of entry e (ascending)
	const int *__restrict__ ent_item;
	const double *__restrict__ lnorm;          // ||L[i]||_2 per user
	const unsigned long long *__restrict__ rnorm_max_bits;   // max_j ||R[j]||_2 as the bits of a double
	double thr_scale;                          // mf_backend_recommend_margin(K)
	double *__restrict__ score;                // B[i][j] of entry e: the threshold
	int *__restrict__ state;                   // 0: to be counted; 1: decided by rank_threshold_kernel (a training pair)
	int *__restrict__ rank;                    // per entry, the plan's bucketed order
	int *__restrict__ above;                   // matrix-core pass: open items certainly above the threshold, summed over the splits
	int *__restrict__ band;                    // ... != 0: a score too close to the threshold to decide, or a non-finite one
	const int *__restrict__ elist;             // exact pass: only these entries (nullptr: all)
	int *__restrict__ olist;                   // rank_finish_kernel, out: entries that need the exact pass
	int *__restrict__ ocount;
	int split_items;                           // item split (small problems): blockIdx.y = split s counts items
	                                           // [s * split_items, (s + 1) * split_items); 0: no split
};

// Thresholds: t_e = B[i][j] exactly and the masked test (binary search of j in the user's ascending mask list); clears the
// counters of the matrix-core pass.  A NaN threshold is left to the exact pass: the matrix-core pass cannot certify it
// (every comparison with its band fails, and a NaN score needs a non-finite factor, so the norm bound fails too).
__global__ void __launch_bounds__(256) rank_threshold_kernel(RankArgs a)
{
	const int e = blockIdx.x * 256 + threadIdx.x;
	if (e >= a.rows) return;
	const int u = a.ent_user[e], j = a.ent_item[e];
	int lo = a.csr_ptr[u], hi = a.csr_ptr[u + 1];
	while (lo < hi) {
		const int mid = lo + (hi - lo) / 2;
		if (a.csr_idx[mid] < j)
			lo = mid + 1;
		else
			hi = mid;
	}
	const bool rated = lo < a.csr_ptr[u + 1] && a.csr_idx[lo] == j;
	const double t = rated ? 0.0 : topn_exact_score(a.L + (size_t) u * a.ldl, a.R + (size_t) j * a.ldr, a.K);
	a.score[e] = t;
	a.state[e] = rated;
	a.rank[e] = rated ? kRankMasked : 0;
	a.above[e] = 0;
	a.band[e] = 0;
}

// ------------------------------------------------------------------------------------------------
// Matrix-core counting pass.  The operand path (RRing: L in registers, a ring of three R chunks by LDS-DMA, fragment reads
// one k-step ahead, 128-item tiles) and item masks of topn_mfma_kernel; the epilogue of a tile counts.  Every approximate
// score s' of an open item is within thr / 2 of B[i][j'] (thr = cert_margin, as in topn_finish), and the threshold t is
// exact, so
//   s' > t + thr  =>  B[i][j'] > t: counted in `above`;      s' < t - thr  =>  B[i][j'] < t: not counted;
//   anything else (NaN included) sets `band`: the entry goes to the exact pass.
// Item j itself is closed through the row's mask.  The counts live per lane in VGPRs and are summed over the 16 lanes and
// the two item halves after the last tile; an item split adds its part with atomics (integers: no order dependence).
// ------------------------------------------------------------------------------------------------
template <int NC, int QC = 5, int TU = 2, int WAVES = 4>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) rank_mfma_kernel(RankArgs a)
{
	static_assert(NC > 0, "compile-time K only");
	using Ring = RRing<NC, QC, TU, WAVES>;
	extern __shared__ double2 rec_lds[];   // ring of kHNB R chunks: [k-pair][128 items]
	__shared__ unsigned long long maskw[2][kHU][2];   // [tile parity][row][item half]
	__shared__ double sh_lo[kHU], sh_hi[kHU];
	__shared__ int red_above[kHU], red_band[kHU];
	__shared__ unsigned long long lmax_bits;

	const int tid = threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int wr = wave >> 1, wc = wave & 1;
	const int lr = lane & 15, lq = lane >> 4;
	const int e0 = blockIdx.x * kHU;
	const double pinf = __builtin_inf();

	int cur = 0, cend = 0, nextcol = INT32_MAX, nextcol2 = INT32_MAX, myj = -1;
	bool live = false;
	if (tid < kHU) {
		const int e = e0 + tid;
		double lo = pinf, hi = pinf;   // a row that is not counted: nothing is above, nothing in the band
		unsigned long long b = 0ull;
		if (e < a.rows && a.state[e] == 0) {
			live = true;
			const int u = a.ent_user[e];
			myj = a.ent_item[e];
			cur = a.csr_ptr[u];
			cend = a.csr_ptr[u + 1];
			nextcol = cur < cend ? a.csr_idx[cur] : INT32_MAX;
			nextcol2 = cur + 1 < cend ? a.csr_idx[cur + 1] : INT32_MAX;
			const double ln = a.lnorm[u];
			const double thr = cert_margin(a.thr_scale, ln, rnorm_max(a.rnorm_max_bits));
			const double t = a.score[e];
			lo = t - thr;
			hi = t + thr;
			b = (unsigned long long) __double_as_longlong(ln);
		}
		sh_lo[tid] = lo;
		sh_hi[tid] = hi;
		red_above[tid] = 0;
		red_band[tid] = 0;
		b = wave_max_bits(b);
		if (lane == 0) lmax_bits = b;
	}
	Ring::clear(rec_lds, tid);
	double fa[Ring::KSTEPS][TU];
#pragma unroll
	for (int tu = 0; tu < TU; ++tu) {
		const int row = e0 + 16 * TU * wr + 16 * tu + lr;
		const double *l = a.L + (size_t) (row < a.rows ? a.ent_user[row] : 0) * a.ldl;
#pragma unroll
		for (int ks = 0; ks < Ring::KSTEPS; ++ks) {
			const int k = 4 * ks + lq;
			fa[ks][tu] = row < a.rows && k < a.K ? l[k] : 0.0;
		}
	}
	__syncthreads();
	double tlo[4 * TU], thi[4 * TU];   // t -/+ thr of each of the lane's rows
	int above[4 * TU];
	unsigned bandm = 0;                // bit x: row x saw a score it cannot decide
#pragma unroll
	for (int tu = 0; tu < TU; ++tu)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int row = 16 * TU * wr + 16 * tu + lq + 4 * r;
			tlo[tu * 4 + r] = sh_lo[row];
			thi[tu * 4 + r] = sh_hi[row];
			above[tu * 4 + r] = 0;
		}

	const int j_first = a.split_items ? (int) blockIdx.y * a.split_items : 0;
	const int j_end = a.split_items ? min(a.items, j_first + a.split_items) : a.items;
	Ring ring(rec_lds, a, j_first, j_end, lane, wave);
	ring.issue_next();
	ring.prime();
	const bool all_finite = all_scores_finite(lmax_bits, a.rnorm_max_bits);
	for (int j0 = j_first; j0 < j_end; j0 += kMI) {
		mf_d4 acc[TU][4];

		const int par = ((j0 - j_first) / kMI) & 1;
		if (tid < kHU) {
			unsigned long long m0 = 0, m1 = 0;
			while (nextcol < j0 + kMI) {
				const int o = nextcol - j0;
				if (o >= 64)
					m1 |= 1ull << (o - 64);
				else if (o >= 0)
					m0 |= 1ull << o;
				++cur;
				nextcol = nextcol2;
				nextcol2 = cur + 1 < cend ? a.csr_idx[cur + 1] : INT32_MAX;
			}
			const int oj = myj - j0;   // the entry's own item is no candidate
			if (oj >= 64 && oj < 128)
				m1 |= 1ull << (oj - 64);
			else if (oj >= 0 && oj < 64)
				m0 |= 1ull << oj;
			const int left = j_end - j0;   // > 0
			if (left < 64) {
				m0 |= ~0ull << left;
				m1 = ~0ull;
			} else if (left < 128) {
				m1 |= ~0ull << (left - 64);
			}
			maskw[par][tid][0] = m0;
			maskw[par][tid][1] = m1;
		}

		ring.tile(fa, acc);

		// counting epilogue: the lane's four scores of each of its rows against the row's t -/+ thr
#pragma unroll
		for (int tu = 0; tu < TU; ++tu)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int x = tu * 4 + r;
				const int row = 16 * TU * wr + 16 * tu + lq + 4 * r;
				const unsigned long long m = maskw[par][row][wc] >> lr;
				bool bd = false;
#pragma unroll
				for (int ti = 0; ti < 4; ++ti) {
					const double v = acc[tu][ti][r];
					const bool open = !((m >> (16 * ti)) & 1ull);
					const bool gt = v > thi[x];
					above[x] += open && gt;
					bd |= open && !gt && !(v < tlo[x]);   // NaN: in the band
					if (!all_finite) bd |= open && !(fabs(v) <= 1.7976931348623157e308);
				}
				bandm |= bd ? 1u << x : 0u;
			}
	}

	// sum over the 16 lanes of a row and the two item halves, then add this split's part
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
	for (int tu = 0; tu < TU; ++tu)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int x = tu * 4 + r;
			const int row = 16 * TU * wr + 16 * tu + lq + 4 * r;
			int c = above[x], b = (int) ((bandm >> x) & 1u);
#pragma unroll
			for (int d = 1; d < 16; d <<= 1) {
				c += __shfl_xor(c, d, 16);
				b |= __shfl_xor(b, d, 16);
			}
			if (lr == 0) {
				atomicAdd(&red_above[row], c);
				if (b) atomicOr(&red_band[row], 1);
			}
		}
	__syncthreads();
	if (live) {
		atomicAdd(a.above + e0 + tid, red_above[tid]);
		if (red_band[tid]) atomicOr(a.band + e0 + tid, 1);
	}
}

// Certification: no undecided score in any split and ||L_i|| * max ||R_j|| <= 1e300 (every partial sum of every exact score
// is then finite and the error bound holds) => rank = above.  Everyone else onto the list of the exact pass.
__global__ void __launch_bounds__(256) rank_finish_kernel(RankArgs a)
{
	const int e = blockIdx.x * 256 + threadIdx.x;
	if (e >= a.rows || a.state[e] != 0) return;
	const double bound = a.lnorm[a.ent_user[e]] * rnorm_max(a.rnorm_max_bits);
	const double t = a.score[e];
	if (a.band[e] == 0 && bound <= 1e300 && t == t)
		a.rank[e] = a.above[e];
	else
		a.olist[atomicAdd(a.ocount, 1)] = e;
}

// ------------------------------------------------------------------------------------------------
// Exact pass: one wave per entry (the listed ones, or all).  Lane l scores item j0 + l exactly (topn_exact_score) over
// the open items and the wave counts by the definition: IEEE comparisons, so a NaN score never counts; a NaN threshold
// is MF_RANK_NAN.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) rank_exact_kernel(RankArgs a)
{
	const int lane = threadIdx.x;
	const int e = a.elist ? a.elist[blockIdx.x] : (int) blockIdx.x;
	if (a.state[e] != 0) return;
	const int u = a.ent_user[e], mine = a.ent_item[e];
	const double t = a.score[e];
	const double *l = a.L + (size_t) u * a.ldl;
	int cur = a.csr_ptr[u];
	const int cend = a.csr_ptr[u + 1];
	int cnt = 0;
	for (int j0 = 0; j0 < a.items; j0 += 64) {
		unsigned long long m = 0;   // rated items of this batch (every lane walks the same cursor)
		while (cur < cend) {
			const int c = a.csr_idx[cur];
			if (c >= j0 + 64) break;
			if (c >= j0) m |= 1ull << (c - j0);
			++cur;
		}
		const int j = j0 + lane;
		const bool open = j < a.items && j != mine && !((m >> lane) & 1ull);
		const double s = open ? topn_exact_score(l, a.R + (size_t) j * a.ldr, a.K) : 0.0;
		cnt += open && (s > t || (s == t && j < mine));
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
	if (lane == 0) a.rank[e] = t != t ? kRankNan : cnt;
}

}  // namespace mf
