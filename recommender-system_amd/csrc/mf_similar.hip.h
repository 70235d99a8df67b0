// mf_similar.hip.h -- operand preparation of mf_plan_similar_items: the top-N nearest neighbours of an item's row of R
// among the other items, by dot product or by cosine.  The query is the top-N problem of mf_topn.hip.h on other operands:
//   rows    = Q (all items) or the gathered rows Q[query[t]],
//   columns = Q,
//   mask    = one masked item per row, the query item itself (a CSR with ptr[t] = t, idx[t] = query[t]),
// where Q = R (dot) or R with every row divided by its norm (cosine).  The kernels here build Q, the gathered block and
// the mask; the passes themselves are topn_mfma_kernel, topn_merge_kernel and topn_exact_kernel, unchanged.
//
// The bits of Q are part of the contract (include/matfact_hip.h): s_j = the squares of row j added in ascending k from
// 0.0, multiply and add unfused; n_j = sqrt(s_j); Q[j][k] = R[j][k] / n_j -- square root and division correctly rounded,
// nothing special-cased (a zero row is 0/0 = NaN, an underflowed sum gives +-inf, an infinite norm 0 or NaN).
#pragma once
#include "mf_common.hip.h"

namespace mf {

constexpr int kSimRows = 16;      // rows of a workgroup of similar_normalize_kernel (one wave: row r's sum is lane r's)
constexpr int kSimThreads = 64;
constexpr int kSimKC = 32;        // columns staged per step; the LDS pitch kSimKC + 1 keeps the row walk conflict-free

// Q[j][k] = R[j][k] / sqrt(sum_k R[j][k]^2) for the 16 rows of the workgroup.  A stream over the rows: every element is
// read twice (the second time from L2) and written once, all three in 256-byte runs per row; the serial sum of a row is
// formed by one lane from LDS, so its order is the definition's whatever the layout of the loads.  16 rows per wave and
// not 64: the serial sums are latency, so the launch wants many waves (17 770 rows are 1111 of them, not 278), and the
// divisions -- the bulk of the instructions -- are spread over four times as many.
__global__ void __launch_bounds__(kSimThreads) similar_normalize_kernel(const double *__restrict__ R, int items, int K, int ld,
                                                                      double *__restrict__ Q)
{
	__shared__ double tile[kSimRows][kSimKC + 1];
	__shared__ double nrm[kSimRows];
	const int lane = threadIdx.x;
	const int j0 = blockIdx.x * kSimRows;
	const int rows = min(kSimRows, items - j0);
	double s = 0.0;
	for (int k0 = 0; k0 < K; k0 += kSimKC) {
		const int kc = min(kSimKC, K - k0);
		for (int e = lane; e < rows * kSimKC; e += kSimThreads) {
			const int r = e / kSimKC, k = e % kSimKC;
			if (k < kc) tile[r][k] = R[(size_t) (j0 + r) * ld + k0 + k];
		}
		__syncthreads();
		if (lane < rows)
			for (int k = 0; k < kc; ++k) {
				const double v = tile[lane][k];
				s = s + v * v;   // unfused: the library is built with -ffp-contract=off
			}
		__syncthreads();
	}
	if (lane < kSimRows) nrm[lane] = sqrt(s);
	__syncthreads();
	for (int k0 = 0; k0 < K; k0 += kSimKC) {
		const int kc = min(kSimKC, K - k0);
		for (int e = lane; e < rows * kSimKC; e += kSimThreads) {
			const int r = e / kSimKC, k = e % kSimKC;
			if (k < kc) {
				const size_t at = (size_t) (j0 + r) * ld + k0 + k;
				Q[at] = R[at] / nrm[r];
			}
		}
	}
}

// The operands of a query: the mask ptr[t] = t (t = 0 .. nq), idx[t] = query[t] -- one masked item per row, the query
// item itself -- and, for a listed query, row t of the block = row query[t] of Q (K doubles at pitch ldb).  query ==
// nullptr is the query of all items in ascending order: the mask is the identity and nothing is copied (the row operand
// is Q itself).  One wave per 64 rows of the mask, then the same wave copies its rows.
__global__ void __launch_bounds__(64) similar_gather_kernel(const double *__restrict__ Q, int ld, int K,
                                                             const int *__restrict__ query, int nq,
                                                             double *__restrict__ block, int ldb, int *__restrict__ ptr,
                                                             int *__restrict__ idx)
{
	const int lane = threadIdx.x;
	const int t0 = blockIdx.x * 64;
	const int t = t0 + lane;
	if (t < nq) {
		ptr[t] = t;
		idx[t] = query ? query[t] : t;
	}
	if (t == nq - 1) ptr[nq] = nq;
	if (!query) return;
	const int rows = min(64, nq - t0);
	for (int r = 0; r < rows; ++r) {
		const double *__restrict__ src = Q + (size_t) query[t0 + r] * ld;
		double *__restrict__ dst = block + (size_t) (t0 + r) * ldb;
		for (int k = lane; k < K; k += 64) dst[k] = src[k];
	}
}

}  // namespace mf
