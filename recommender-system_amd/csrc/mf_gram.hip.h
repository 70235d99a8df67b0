// mf_gram.hip.h -- the Gram matrix of a whole side, S = X^T X over ALL rows of X, in a fixed order of every operation
// (include/matfact_hip.h, mf_plan_gram), and the observed part of the implicit-feedback objective.
//
// The rows of X are cut into blocks of kLossBlock consecutive rows counted from row 0 of the buffer.  Per block b and
// element p >= q of the lower triangle
//   T_b[p][q] = (((0.0 + x_i0[p] * x_i0[q]) + x_i1[p] * x_i1[q]) + ...)      i ascending inside the block, unfused
//   S[p][q]   = ((0.0 + T_0[p][q]) + T_1[p][q]) + ...                        b ascending
// gram_block_kernel: one workgroup per block.  It streams its rows through an LDS tile of kGramChunk rows, and every thread
// owns up to NB square BS x BS blocks of the triangle in registers exactly as phase 2 of the ALS solve does (mf_als.hip.h:
// the same ownership, 2 BS LDS reads -- all lanes of a block row read the same addresses, broadcast -- feed BS^2 products).
// gram_sum_kernel: one thread per element of the triangle adds the T_b in ascending b.
// A row's padding (columns K .. ld) is never read; the tile's columns K .. Kp are zeros and feed only register elements
// that are never stored.  No FP64 matrix instruction, no fused multiply-add (-ffp-contract=off).
#pragma once
#include "mf_als.hip.h"
#include "mf_loss.hip.h"

namespace mf {

constexpr int kGramThreads = 256;
constexpr int kGramBS = 4;        // the register blocks of als_kernel<256, 4, NB>
constexpr int kGramChunk = 32;    // rows of X in the LDS tile: 32 KiB at K = 128

struct GramArgs {
	int rows, K, ld;                     // rows of X, columns, row pitch in doubles
	const double *__restrict__ X;
	double *__restrict__ partial;        // blocks x K (K + 1) / 2: the T_b, each packed row by row (als_tri)
};

template <int NB>
__global__ void __launch_bounds__(kGramThreads) gram_block_kernel(GramArgs a)
{
	constexpr int BS = kGramBS, THREADS = kGramThreads, NCH = kGramChunk;
	extern __shared__ double gram_tile[];   // NCH x Kp

	const int K = a.K, Kp = als_padded_k(K, BS);
	const int tid = (int) threadIdx.x;
	const long long row0 = (long long) blockIdx.x * kLossBlock;
	if (row0 >= a.rows) return;   // the whole workgroup
	const int nr = (int) (a.rows - row0 < kLossBlock ? a.rows - row0 : kLossBlock);

	// the blocks of this thread: block e = tid + i * THREADS of the triangle of blocks, rows bp >= columns bq
	const int nblocks = als_blocks(K, BS);
	int bp[NB], bq[NB];
	double acc[NB][BS][BS];
#pragma unroll
	for (int i = 0; i < NB; ++i) {
		const int e = tid + i * THREADS;
		int p = (int) ((sqrtf(8.0f * (float) e + 1.0f) - 1.0f) * 0.5f);
		while (p * (p + 1) / 2 > e) --p;
		while ((p + 1) * (p + 2) / 2 <= e) ++p;
		bp[i] = e < nblocks ? p * BS : 0;
		bq[i] = e < nblocks ? (e - p * (p + 1) / 2) * BS : 0;
#pragma unroll
		for (int u = 0; u < BS; ++u)
#pragma unroll
			for (int v = 0; v < BS; ++v) acc[i][u][v] = 0.0;
	}

	for (int c0 = 0; c0 < nr; c0 += NCH) {
		const int cc = min(NCH, nr - c0);
		// the chunk's rows, zero beyond column K
		{
			int n = tid / Kp, k = tid - n * Kp;
			const int dn = THREADS / Kp, dk = THREADS - dn * Kp;
			while (n < cc) {
				gram_tile[n * Kp + k] = k < K ? a.X[(size_t) (row0 + c0 + n) * a.ld + k] : 0.0;
				n += dn, k += dk;
				if (k >= Kp) k -= Kp, ++n;
			}
		}
		__syncthreads();
		// T[p][q] = T[p][q] + (x_n[p] * x_n[q]), n ascending
		for (int n = 0; n < cc; ++n) {
			const double *xr = gram_tile + n * Kp;
#pragma unroll
			for (int i = 0; i < NB; ++i) {
				if (tid + i * THREADS < nblocks) {
					double xp[BS], xq[BS];
#pragma unroll
					for (int u = 0; u < BS; ++u) xp[u] = xr[bp[i] + u], xq[u] = xr[bq[i] + u];
#pragma unroll
					for (int u = 0; u < BS; ++u)
#pragma unroll
						for (int v = 0; v < BS; ++v) {
							const double t = xp[u] * xq[v];
							acc[i][u][v] = acc[i][u][v] + t;
						}
				}
			}
		}
		__syncthreads();
	}

	double *T = a.partial + (size_t) blockIdx.x * als_triangle(K);
#pragma unroll
	for (int i = 0; i < NB; ++i) {
		if (tid + i * THREADS < nblocks) {
#pragma unroll
			for (int u = 0; u < BS; ++u)
#pragma unroll
				for (int v = 0; v < BS; ++v) {
					const int p = bp[i] + u, q = bq[i] + v;
					if (p < K && q <= p) T[als_tri(p, q)] = acc[i][u][v];
				}
		}
	}
}

// S[e] = ((0.0 + T_0[e]) + T_1[e]) + ..., one thread per element of the triangle
__global__ void __launch_bounds__(kGramThreads) gram_sum_kernel(const double *__restrict__ partial, int nblocks, int triangle,
                                                                 double *__restrict__ S)
{
	const int e = (int) blockIdx.x * kGramThreads + (int) threadIdx.x;
	if (e >= triangle) return;
	double s = 0.0;
	for (int b = 0; b < nblocks; ++b) s = s + partial[(size_t) b * triangle + e];
	S[e] = s;
}

// ------------------------------------------------------------------------------------------------
// The observed part of the implicit objective (mf_plan_implicit_objective): loss_reg_kernel's row sums with
//   e_n = conf * w_n (conf without weights),  c_n = 1.0 + e_n,  q_n = (c_n * (d_n * d_n)) - (p_n * p_n)
// -- what an observed pair adds to the all-pairs sum of squares, which counted it as a zero at confidence 1.  One instance
// serves every K and both kinds of plan (a.wgt null: unweighted).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave) implicit_rows_kernel(LossArgs a, double conf)
{
	extern __shared__ double loss_tile[];
	const int K = a.K;
	const int stride = a.stride;
	const int nch = a.nch;
	const int lane = threadIdx.x;

	for (int it = blockIdx.x; it < a.nrows; it += gridDim.x) {
		const int r = a.rowlist ? a.rowlist[it] : it;
		const int beg = a.ptr[r], end = a.ptr[r + 1];
		const double *__restrict__ xrow = a.L + (size_t) r * a.ldl;
		double s = 0.0;
		for (int c = beg; c < end; c += nch) {
			const int cnt = min(nch, end - c);
			int my_idx = 0;
			double my_val = 0.0;
			double my_e = conf;
			if (lane < cnt) {
				my_idx = a.idx[c + lane];
				my_val = a.val[c + lane];
				if (a.wgt) my_e = conf * a.wgt[c + lane];
			}
			for (int n = 0; n < cnt; ++n) {
				const int j = __builtin_amdgcn_readlane(my_idx, n);
				const double *__restrict__ yrow = a.R + (size_t) j * a.ldr;
				double *trow = loss_tile + n * stride;
				for (int k = lane; k < K; k += kWave)
					trow[k] = yrow[k];
			}
			__syncthreads();
			const double *t = loss_tile + (lane < nch ? lane : 0) * stride;   // lanes beyond the tile re-read row 0
			double dot = 0.0;
#pragma unroll 8
			for (int k = 0; k < K; ++k)
				dot = dot + xrow[k] * t[k];
			const double cn = 1.0 + my_e;
			const double cd = cn * loss_square(my_val, dot);
			const double pp = dot * dot;
			s = loss_chain(s, cd - pp, cnt);
			__syncthreads();
		}
		if (lane == 0) a.row_sse[r] = s;
	}
}

}  // namespace mf
