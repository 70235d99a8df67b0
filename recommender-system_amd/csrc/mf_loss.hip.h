// mf_loss.hip.h -- squared error of L * R^T over an entry set (the training entries or a held-out set), in a fixed
// order of every floating-point operation (include/matfact_hip.h, mf_plan_loss):
//   p_n = dot(L[i_n], R[j_n])      sequential k from 0.0, multiply and add unfused  (mat2d.c:126-139, as phase A of the sweeps)
//   q_n = (a_n - p_n) * (a_n - p_n)                  times w_n, one more rounded multiply, in the weighted instances (the
//                                                    training loss of a plan created with per-entry weights)
//   s_i = ((0.0 + q_n0) + q_n1) + ...   over the entries of user i in the order of the CSR (the caller's order)
//   T_b = the s_i of the users [1024 b, 1024 (b + 1)) (GLOBAL user ids) added in ascending i from 0.0
//   SSE = the T_b added in ascending b from 0.0
// Kernels: the row sums (one wave per user: the sweeps' gather and phase A, then the ordered chain over the lanes of the
// chunk; LDS-DMA form for even K, register-staged form for the rest), the block sums and the total.
// Build with -ffp-contract=off, as the sweeps.
#pragma once
#include "mf_sweep.hip.h"

namespace mf {

constexpr int kLossBlock = 1024;   // == MF_LOSS_BLOCK

struct LossArgs {
	int nrows;
	int K;
	int nch;      // entries per chunk (<= 64)
	int stride;   // register-staged form: LDS row stride in doubles (odd)
	int ldl, ldr; // row pitch of L and of R in doubles
	const int *__restrict__ ptr;
	const int *__restrict__ idx;
	const double *__restrict__ val;
	const double *__restrict__ L;
	const double *__restrict__ R;
	double *__restrict__ row_sse;
	const int *__restrict__ rowlist;   // optional: the order in which the workgroups take the rows (all of them)
	const double *__restrict__ wgt;    // weighted instances only: the entries' weights in the order of (idx, val)
};

// q = (a - p) * (a - p), formed as (p - a) * (p - a): the same bits for every a and p that are not NaN (IEEE subtraction is
// symmetric in sign and the square drops it).  The hardware subtracts by adding a negated operand, and negating a NaN flips
// its sign bit; with the negation on the rating, a NaN that comes from a factor row reaches the sums with the bits it had.
__device__ __forceinline__ double loss_square(double a, double p)
{
	const double d = p - a;
	return d * d;
}

// The ordered chain: s = (...((s + q_0) + q_1) + ...) + q_{cnt-1}, q_n taken from lane n as a scalar operand.  Lanes at
// or past cnt never enter it.  s is the same in every lane.
__device__ __forceinline__ double loss_chain(double s, double q, int cnt)
{
	int n = 0;
	for (; n + 4 <= cnt; n += 4) {
		double qn[4];
#pragma unroll
		for (int u = 0; u < 4; ++u)
			qn[u] = readlane_f64(q, n + u);
#pragma unroll
		for (int u = 0; u < 4; ++u)
			s = s + qn[u];
	}
	for (; n < cnt; ++n)
		s = s + readlane_f64(q, n);
	return s;
}

// ------------------------------------------------------------------------------------------------
// Row sums, LDS-DMA form: stage and phase A of sweep_dma_kernel (same tile geometry, same arithmetic), no phase B, no
// write of a factor row.  LDS: [ L row: xs_bytes ][ tile: nch rows x S bytes ].
// KT > 0: compile-time K; KT == 0: any even K up to 128 * NPASS at run time.
// ------------------------------------------------------------------------------------------------
template <int KT, int NPASS>
__global__ void __launch_bounds__(kWave) loss_dma_kernel(LossArgs a)
{
	const int K = KT > 0 ? KT : a.K;
	const int P = dma_pieces(K);
	constexpr int NP = NPASS;
	const int S = dma_row_stride(K);
	const int xs_bytes = dma_xs_bytes(K);
	extern __shared__ __attribute__((aligned(16))) char lds[];
	double2 *xs = reinterpret_cast<double2 *>(lds);
	char *tile = lds + xs_bytes;
	const int nch = a.nch;
	const int lane = threadIdx.x;
	const unsigned voff = (unsigned) lane * 16u;
	const unsigned long long ybase = (unsigned long long) a.R;
	const size_t ybytes = (size_t) a.ldr * 8;   // bytes between rows of R

	for (int it = blockIdx.x; it < a.nrows; it += gridDim.x) {
		const int r = a.rowlist ? a.rowlist[it] : it;
		const int beg = a.ptr[r], end = a.ptr[r + 1];
		const double2 *__restrict__ xrow2 = reinterpret_cast<const double2 *>(a.L + (size_t) r * a.ldl);
#pragma unroll
		for (int p = 0; p < NP; ++p) {
			const int q = lane + kWave * p;
			if (q < P) xs[q] = xrow2[q];
		}

		double s = 0.0;
		// (idx, val) of a chunk are loaded one chunk ahead, so the gather of chunk c never waits on them
		int nx_idx = 0;
		double nx_val = 0.0;
		if (beg + lane < min(end, beg + nch)) {
			nx_idx = a.idx[beg + lane];
			nx_val = a.val[beg + lane];
		}
		for (int c = beg; c < end; c += nch) {
			const int cnt = min(nch, end - c);
			const int my_idx = nx_idx;
			const double my_val = nx_val;
			if (c + nch + lane < min(end, c + 2 * nch)) {
				nx_idx = a.idx[c + nch + lane];
				nx_val = a.val[c + nch + lane];
			}
			// ---- stage (as sweep_dma_kernel): short rows several per instruction, the others one instruction per row and pass
			if constexpr (KT > 0 && dma_multi_row(KT))
				gather_multi_row<KT>(ybase, ybytes, my_idx, cnt, lane, tile);
			else
				gather_rows<NP>(ybase, ybytes, my_idx, cnt, lane, voff, P, S, tile);
			__syncthreads();   // single-wave workgroup: this is the vmcnt(0)/lgkmcnt(0) that retires the DMA
			// ---- phase A (lanes beyond the tile re-read row 0; lanes >= cnt produce garbage that never enters the chain)
			const double2 *t2 = reinterpret_cast<const double2 *>(tile + (lane < nch ? lane : 0) * S);
			double dot = 0.0;
			if constexpr (KT > 0) {
				dot = phase_a_dot<KT>(t2, xs);
			} else {
				int i = 0;
				for (; i + 4 <= P; i += 4) {
					double2 t[4], x[4];
#pragma unroll
					for (int u = 0; u < 4; ++u) {
						t[u] = t2[i + u];
						x[u] = xs[i + u];
					}
#pragma unroll
					for (int u = 0; u < 4; ++u) {
						dot = dot + x[u].x * t[u].x;
						dot = dot + x[u].y * t[u].y;
					}
				}
				for (; i < P; ++i) {
					const double2 t = t2[i];
					const double2 x = xs[i];
					dot = dot + x.x * t.x;
					dot = dot + x.y * t.y;
				}
			}
			const double q = loss_square(my_val, dot);
			s = loss_chain(s, q, cnt);
			__syncthreads();   // tile is overwritten by the next chunk's DMA
		}
		if (lane == 0) a.row_sse[r] = s;
		__syncthreads();   // xs is overwritten by the next row
	}
}

// The weighted twin: the kernel above with q_n * w_n, the weight loaded where val is (a name of its own: the unweighted
// instances are counted by name, and their code stays exactly what it was).
template <int KT, int NPASS>
__global__ void __launch_bounds__(kWave) loss_dma_w_kernel(LossArgs a)
{
	const int K = KT > 0 ? KT : a.K;
	const int P = dma_pieces(K);
	constexpr int NP = NPASS;
	const int S = dma_row_stride(K);
	const int xs_bytes = dma_xs_bytes(K);
	extern __shared__ __attribute__((aligned(16))) char lds[];
	double2 *xs = reinterpret_cast<double2 *>(lds);
	char *tile = lds + xs_bytes;
	const int nch = a.nch;
	const int lane = threadIdx.x;
	const unsigned voff = (unsigned) lane * 16u;
	const unsigned long long ybase = (unsigned long long) a.R;
	const size_t ybytes = (size_t) a.ldr * 8;   // bytes between rows of R

	for (int it = blockIdx.x; it < a.nrows; it += gridDim.x) {
		const int r = a.rowlist ? a.rowlist[it] : it;
		const int beg = a.ptr[r], end = a.ptr[r + 1];
		const double2 *__restrict__ xrow2 = reinterpret_cast<const double2 *>(a.L + (size_t) r * a.ldl);
#pragma unroll
		for (int p = 0; p < NP; ++p) {
			const int q = lane + kWave * p;
			if (q < P) xs[q] = xrow2[q];
		}

		double s = 0.0;
		// (idx, val) of a chunk are loaded one chunk ahead, so the gather of chunk c never waits on them
		int nx_idx = 0;
		double nx_val = 0.0;
		double nx_wgt = 0.0;
		if (beg + lane < min(end, beg + nch)) {
			nx_idx = a.idx[beg + lane];
			nx_val = a.val[beg + lane];
			nx_wgt = a.wgt[beg + lane];
		}
		for (int c = beg; c < end; c += nch) {
			const int cnt = min(nch, end - c);
			const int my_idx = nx_idx;
			const double my_val = nx_val;
			const double my_wgt = nx_wgt;
			if (c + nch + lane < min(end, c + 2 * nch)) {
				nx_idx = a.idx[c + nch + lane];
				nx_val = a.val[c + nch + lane];
				nx_wgt = a.wgt[c + nch + lane];
			}
			// ---- stage (as sweep_dma_kernel): short rows several per instruction, the others one instruction per row and pass
			if constexpr (KT > 0 && dma_multi_row(KT))
				gather_multi_row<KT>(ybase, ybytes, my_idx, cnt, lane, tile);
			else
				gather_rows<NP>(ybase, ybytes, my_idx, cnt, lane, voff, P, S, tile);
			__syncthreads();   // single-wave workgroup: this is the vmcnt(0)/lgkmcnt(0) that retires the DMA
			// ---- phase A (lanes beyond the tile re-read row 0; lanes >= cnt produce garbage that never enters the chain)
			const double2 *t2 = reinterpret_cast<const double2 *>(tile + (lane < nch ? lane : 0) * S);
			double dot = 0.0;
			if constexpr (KT > 0) {
				dot = phase_a_dot<KT>(t2, xs);
			} else {
				int i = 0;
				for (; i + 4 <= P; i += 4) {
					double2 t[4], x[4];
#pragma unroll
					for (int u = 0; u < 4; ++u) {
						t[u] = t2[i + u];
						x[u] = xs[i + u];
					}
#pragma unroll
					for (int u = 0; u < 4; ++u) {
						dot = dot + x[u].x * t[u].x;
						dot = dot + x[u].y * t[u].y;
					}
				}
				for (; i < P; ++i) {
					const double2 t = t2[i];
					const double2 x = xs[i];
					dot = dot + x.x * t.x;
					dot = dot + x.y * t.y;
				}
			}
			double q = loss_square(my_val, dot);
			q = q * my_wgt;
			s = loss_chain(s, q, cnt);
			__syncthreads();   // tile is overwritten by the next chunk's DMA
		}
		if (lane == 0) a.row_sse[r] = s;
		__syncthreads();   // xs is overwritten by the next row
	}
}

// ------------------------------------------------------------------------------------------------
// Row sums, register-staged form (odd K, K beyond the LDS-DMA geometry, MF_SWEEP_IMPL=reg): stage and phase A of
// sweep_kernel.  It keeps no accumulators, so one instance serves every K.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave) loss_reg_kernel(LossArgs a)
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
			if (lane < cnt) {
				my_idx = a.idx[c + lane];
				my_val = a.val[c + lane];
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
			s = loss_chain(s, loss_square(my_val, dot), cnt);
			__syncthreads();
		}
		if (lane == 0) a.row_sse[r] = s;
	}
}

// the weighted twin of loss_reg_kernel: q_n * w_n
__global__ void __launch_bounds__(kWave) loss_reg_w_kernel(LossArgs a)
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
			double my_wgt = 0.0;
			if (lane < cnt) {
				my_idx = a.idx[c + lane];
				my_val = a.val[c + lane];
				my_wgt = a.wgt[c + lane];
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
			double q = loss_square(my_val, dot);
			q = q * my_wgt;
			s = loss_chain(s, q, cnt);
			__syncthreads();
		}
		if (lane == 0) a.row_sse[r] = s;
	}
}

// Row sums of the weights (mf_plan_weight_total): s_i = ((0.0 + w_n0) + w_n1) + ... over the entries of user i in the order
// of the CSR, one wave per user; loss_block_kernel and loss_total_kernel then add the rows up (step 4 of the loss).
__global__ void __launch_bounds__(kWave) weight_rows_kernel(const int *__restrict__ ptr, const double *__restrict__ wgt, int nrows,
                                                             double *__restrict__ row_w)
{
	const int lane = threadIdx.x;
	for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
		const int beg = ptr[r], end = ptr[r + 1];
		double s = 0.0;
		for (int c = beg; c < end; c += kWave) {
			const int cnt = min(kWave, end - c);
			const double v = lane < cnt ? wgt[c + lane] : 0.0;
			s = loss_chain(s, v, cnt);
		}
		if (lane == 0) row_w[r] = s;
	}
}

// ------------------------------------------------------------------------------------------------
// Total.  Blocks are cut at GLOBAL multiples of kLossBlock: user_begin may sit inside a block, the sums then run over
// the plan's users only.  loss_block_kernel: one wave per block (one chain); loss_total_kernel: one wave (one chain)
// over the block sums.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave) loss_block_kernel(const double *__restrict__ row_sse, int user_begin, int users, int nblocks,
                                                            double *__restrict__ block_sum)
{
	const int b = blockIdx.x, lane = threadIdx.x;
	if (b >= nblocks) return;
	const long long g0 = ((long long) (user_begin / kLossBlock) + b) * kLossBlock;   // first global user of the block
	const long long lo = g0 > user_begin ? g0 - user_begin : 0;
	const long long hi = g0 + kLossBlock - user_begin < users ? g0 + kLossBlock - user_begin : users;
	double t = 0.0;
	for (long long i = lo; i < hi; i += kWave) {   // 64 row sums per coalesced load, then the chain over them
		const int cnt = (int) (hi - i < kWave ? hi - i : kWave);
		const double v = lane < cnt ? row_sse[i + lane] : 0.0;
		t = loss_chain(t, v, cnt);
	}
	if (lane == 0) block_sum[b] = t;
}

__global__ void __launch_bounds__(kWave) loss_total_kernel(const double *__restrict__ block_sum, int nblocks, double *__restrict__ total)
{
	const int lane = threadIdx.x;
	if (blockIdx.x != 0) return;
	double t = 0.0;
	for (int b = 0; b < nblocks; b += kWave) {
		const int cnt = nblocks - b < kWave ? nblocks - b : kWave;
		const double v = lane < cnt ? block_sum[b + lane] : 0.0;
		t = loss_chain(t, v, cnt);
	}
	if (lane == 0) total[0] = t;
}

// ------------------------------------------------------------------------------------------------
// Penalty (mf_plan_penalty): the squared Frobenius norm of a factor in a fixed order.  Row sums of squares
//   s_r = ((0.0 + X[r][0]*X[r][0]) + X[r][1]*X[r][1]) + ...   k ascending, multiply and add unfused
// (the s_j of MF_SIMILAR_COSINE, staged the way similar_normalize_kernel stages them: coalesced runs of a row into LDS,
// the serial sum of row r formed by lane r), then loss_block_kernel and loss_total_kernel over them: step 4 of the loss.
// ------------------------------------------------------------------------------------------------
constexpr int kPenRows = 16;      // rows of a workgroup (one wave)
constexpr int kPenKC = 32;        // columns staged per step; the LDS pitch kPenKC + 1 keeps the row walk conflict-free

__global__ void __launch_bounds__(kWave) penalty_rows_kernel(const double *__restrict__ X, int rows, int K, int ld,
                                                              double *__restrict__ row_sq)
{
	__shared__ double tile[kPenRows][kPenKC + 1];
	const int lane = threadIdx.x;
	const int r0 = blockIdx.x * kPenRows;
	const int n = min(kPenRows, rows - r0);
	double s = 0.0;
	for (int k0 = 0; k0 < K; k0 += kPenKC) {
		const int kc = min(kPenKC, K - k0);
		for (int e = lane; e < n * kPenKC; e += kWave) {
			const int r = e / kPenKC, k = e % kPenKC;
			if (k < kc) tile[r][k] = X[(size_t) (r0 + r) * ld + k0 + k];
		}
		__syncthreads();
		if (lane < n)
			for (int k = 0; k < kc; ++k) {
				const double v = tile[lane][k];
				s = s + v * v;   // unfused: the library is built with -ffp-contract=off
			}
		__syncthreads();
	}
	if (lane < n) row_sq[r0 + lane] = s;
}

// ------------------------------------------------------------------------------------------------
// Box constraint outside a sweep (mf_plan_project, mf_plan_bounds_active): one pass over the bounded columns k < columns,
// k != frozen, of every row of a factor.  A workgroup takes kBoxRows rows at a time, its threads the elements of those
// rows' leading `columns` columns; rows use the plan's pitch `ld`, and nothing at or beyond column `columns` (<= K) -- the
// unbounded columns, the padding -- is read or written.
//   box_project_kernel   X[r][k] = box_clamp(X[r][k]) in place: the projection a seeded sweep applies (mf_sweep.hip.h)
//   box_count_kernel     counts[0] += elements == lo, [1] += elements == hi, [2] += elements strictly between: IEEE
//                        comparisons, so a NaN is in none; integers, so the order of the count is free (atomic adds)
// ------------------------------------------------------------------------------------------------
constexpr int kBoxRows = 64;       // rows of a workgroup per step
constexpr int kBoxThreads = 256;

struct BoxArgs {
	double *X;
	int rows, ld, columns, frozen;
	double lo, hi;
	unsigned long long *counts;   // box_count_kernel: at_lo, at_hi, inside
};

__global__ void __launch_bounds__(kBoxThreads) box_project_kernel(BoxArgs a)
{
	for (int r0 = blockIdx.x * kBoxRows; r0 < a.rows; r0 += gridDim.x * kBoxRows) {
		const int n = min(kBoxRows, a.rows - r0) * a.columns;   // <= 64 K
		for (int e = threadIdx.x; e < n; e += kBoxThreads) {
			const int r = e / a.columns, k = e - r * a.columns;
			if (k == a.frozen) continue;
			double *x = a.X + (size_t) (r0 + r) * a.ld + k;
			*x = box_clamp(*x, a.lo, a.hi);
		}
	}
}

__global__ void __launch_bounds__(kBoxThreads) box_count_kernel(BoxArgs a)
{
	unsigned long long at_lo = 0, at_hi = 0, inside = 0;
	for (int r0 = blockIdx.x * kBoxRows; r0 < a.rows; r0 += gridDim.x * kBoxRows) {
		const int n = min(kBoxRows, a.rows - r0) * a.columns;
		for (int e = threadIdx.x; e < n; e += kBoxThreads) {
			const int r = e / a.columns, k = e - r * a.columns;
			if (k == a.frozen) continue;
			const double x = a.X[(size_t) (r0 + r) * a.ld + k];
			at_lo += x == a.lo ? 1 : 0;
			at_hi += x == a.hi ? 1 : 0;
			inside += (x > a.lo && x < a.hi) ? 1 : 0;
		}
	}
#pragma unroll
	for (int off = kWave / 2; off > 0; off >>= 1) {
		at_lo += __shfl_xor(at_lo, off);
		at_hi += __shfl_xor(at_hi, off);
		inside += __shfl_xor(inside, off);
	}
	if ((threadIdx.x & (kWave - 1)) == 0) {
		if (at_lo) atomicAdd(a.counts + 0, at_lo);
		if (at_hi) atomicAdd(a.counts + 1, at_hi);
		if (inside) atomicAdd(a.counts + 2, inside);
	}
}

}  // namespace mf
