// mf_als_cg.hip.h -- alternating least squares by conjugate gradient: a fixed number of CG steps per row, FP64.
//
// With the other side Y frozen, row r of X moves `steps` conjugate-gradient steps from its current value towards the
// solution of (sum_n w_n y_n y_n^T + ridge I) x = sum_n w_n a_n y_n, and include/matfact_hip.h defines every operation of it
// (C0 .. C5).  The matrix is never formed: its product with a vector v is sum_n w_n y_n (y_n . v) + ridge v, per entry one
// K-length dot against a broadcast vector and one scaled add of the entry's row in entry order -- phase A and phase B of
// sweep_dma_kernel, and this kernel is assembled from that kernel's pieces (mf_sweep.hip.h).  One wave owns one row:
//   pass     over the row's entries in chunks of nch (once for the residual, once per step): the chunk's Y rows go to the LDS
//            tile; phase A, lane = entry, forms t_n = y_n . v against the vector published in LDS (x, then p); phase B,
//            lane = column pair, adds e_n * y_n entry by entry, e_n = (a_n - t_n) [* w_n] in the first pass and t_n [* w_n]
//            in the others.  A row longer than the tile is gathered again in every pass;
//   vectors  x, r, p, q live in the column-pair lanes' registers, lane l holding columns 2l, 2l+1 (+128 per pass);
//   dots     the three K-length dots of a step are serial chains by definition: the K products go to LDS and every lane
//            adds them in column order from broadcast reads, so the sum is wave-uniform and so is every branch on it.
// Three forms, the same operations in the same order and so the same bits:
//   als_cg_kernel<KT, NP, true>   compile-time even K, LDS-DMA gather (several rows per instruction at K <= 62);
//   als_cg_kernel<0, NP, true>    run-time even K up to 128 * NP, LDS-DMA gather, one group of NP instructions per row;
//   als_cg_kernel<0, NP, false>   any K up to 128 * NP, odd K included: the rows go through registers, column by column,
//                                 because a row of an odd K is neither 16-byte aligned nor a whole number of pieces.
// No FP64 matrix instruction and nothing fused (the library is built with -ffp-contract=off); `/` is the correctly rounded
// division.  Nothing here reads or writes the padding of a row of X or Y.
#pragma once
#include "mf_common.hip.h"
#include "mf_sweep.hip.h"
#include "mf_als.hip.h"

namespace mf {

// ---- geometry shared by the kernel and the launch: 16-B pieces of a row (the last one half empty at an odd K), the bytes
// of the published vector and of the products of a dot (one region each in front of the tile), the LDS request
__host__ __device__ constexpr int als_cg_pieces(int K) { return (K + 1) >> 1; }
__host__ __device__ constexpr int als_cg_passes(int K) { return (als_cg_pieces(K) + kWave - 1) / kWave; }
__host__ __device__ constexpr int als_cg_row_stride(int K) { return dma_row_stride_of(als_cg_pieces(K)); }
__host__ __device__ constexpr int als_cg_vec_bytes(int K) { return dma_xs_bytes(2 * als_cg_pieces(K)); }
__host__ __device__ constexpr size_t als_cg_lds_bytes(int K, int nch) { return 2 * (size_t) als_cg_vec_bytes(K) + (size_t) nch * als_cg_row_stride(K); }

// column `col` (-1: none) of a vector held as pieces: the lane that owns it takes `v`
template <int NP>
__device__ __forceinline__ void als_cg_set_column(double2 (&u)[NP], int lane, int col, double v)
{
	const int q = col >> 1;
#pragma unroll
	for (int p = 0; p < NP; ++p)
		if (col >= 0 && q == lane + kWave * p) {
			if (col & 1)
				u[p].y = v;
			else
				u[p].x = v;
		}
}

// The row `src` of K doubles as pieces: whole 16-byte loads where the rows are aligned (ALIGNED: an even K), element by
// element otherwise; the lanes and halves beyond the row hold 0.0
template <int NP, bool ALIGNED>
__device__ __forceinline__ void als_cg_load_row(const double *__restrict__ src, int lane, int K, double2 (&u)[NP])
{
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		const int q = lane + kWave * p;
		u[p] = make_double2(0.0, 0.0);
		if constexpr (ALIGNED) {
			if (2 * q < K) u[p] = reinterpret_cast<const double2 *>(src)[q];
		} else {
			if (2 * q < K) u[p].x = src[2 * q];
			if (2 * q + 1 < K) u[p].y = src[2 * q + 1];
		}
	}
}

template <int NP, bool ALIGNED>
__device__ __forceinline__ void als_cg_store_row(double *__restrict__ dst, int lane, int K, const double2 (&u)[NP])
{
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		const int q = lane + kWave * p;
		if constexpr (ALIGNED) {
			if (2 * q < K) reinterpret_cast<double2 *>(dst)[q] = u[p];
		} else {
			if (2 * q < K) dst[2 * q] = u[p].x;
			if (2 * q + 1 < K) dst[2 * q + 1] = u[p].y;
		}
	}
}

// A vector to LDS for phase A's broadcast reads.  The barrier in front keeps the reads of the previous pass ahead of it; the
// one behind the gather of the next pass stands between it and that pass's reads.
template <int NP>
__device__ __forceinline__ void als_cg_publish(double2 *vs, int lane, int P, const double2 (&u)[NP])
{
	__syncthreads();
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		const int q = lane + kWave * p;
		if (q < P) vs[q] = u[p];
	}
}

// dot(u, v) of the definition: s = 0.0, then s = s + (u[k] * v[k]) for k ascending.  The products go to LDS, every lane adds
// all K of them in order (broadcast reads, eight pieces' reads in front of their sixteen adds); the result is taken from lane
// 0 into scalar registers, so what branches on it is uniform for the compiler too.
template <int NP>
__device__ __forceinline__ double als_cg_dot(double *pr, int lane, int K, const double2 (&u)[NP], const double2 (&v)[NP])
{
	double2 *pr2 = reinterpret_cast<double2 *>(pr);
	const int P = als_cg_pieces(K);
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		const int q = lane + kWave * p;
		if (q < P) pr2[q] = make_double2(u[p].x * v[p].x, u[p].y * v[p].y);
	}
	__syncthreads();
	double s = 0.0;
	const int full = K >> 1;
	int q = 0;
	for (; q + 8 <= full; q += 8) {
		double2 t[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) t[i] = pr2[q + i];
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			s = s + t[i].x;
			s = s + t[i].y;
		}
	}
	for (; q < full; ++q) {
		const double2 t = pr2[q];
		s = s + t.x;
		s = s + t.y;
	}
	if (K & 1) s = s + pr[K - 1];
	__syncthreads();   // the next dot overwrites the products
	return readlane_f64(s, 0);
}

// One pass over the row's entries [beg, beg + cnt): acc[k] = sum_n e_n * y_n[k], n ascending, with t_n = dot(y_n, vs) and
// e_n = a_n - t_n (RESIDUAL) or t_n, times w_n on a weighted plan.  IMPLICIT (mf_als_icg.hip.h) changes the entry's factor
// alone: with c_n = conf * w_n (conf without weights) it is (a_n * (1.0 + c_n)) - (c_n * t_n) (RESIDUAL) or t_n * c_n.
template <int KT, int NP, bool DMA, bool RESIDUAL, bool IMPLICIT = false>
__device__ __forceinline__ void als_cg_pass(const AlsArgs &a, int K, int nch, int beg, int cnt, int lane, const double2 *vs, char *tile,
                                            double2 (&acc)[NP], double conf = 0.0)
{
	const int P = als_cg_pieces(K), S = als_cg_row_stride(K);
	const unsigned voff = (unsigned) lane * 16u;
	const unsigned long long ybase = (unsigned long long) a.Y;
	const size_t ybytes = (size_t) a.ldy * 8;
#pragma unroll
	for (int p = 0; p < NP; ++p) acc[p] = make_double2(0.0, 0.0);
	for (int c0 = 0; c0 < cnt; c0 += nch) {
		const int cc = min(nch, cnt - c0);
		int my_idx = 0;
		double my_val = 0.0, my_wgt = 1.0;
		if (lane < cc) {
			const int e = beg + c0 + lane;
			my_idx = a.idx[e];
			if constexpr (RESIDUAL) my_val = a.val[e];
			if constexpr (IMPLICIT)
				my_wgt = a.wgt ? conf * a.wgt[e] : conf;
			else if (a.wgt)
				my_wgt = a.wgt[e];
		}
		// ---- the chunk's Y rows into the tile
		if constexpr (DMA) {
			if constexpr (KT > 0 && dma_multi_row(KT))
				gather_multi_row<KT>(ybase, ybytes, my_idx, cc, lane, tile);
			else
				gather_rows<NP>(ybase, ybytes, my_idx, cc, lane, voff, P, S, tile);
		} else {
			for (int n = 0; n < cc; ++n) {
				const int j = __builtin_amdgcn_readlane(my_idx, n);
				const double *__restrict__ yrow = a.Y + (size_t) (unsigned) j * a.ldy;
				double *trow = reinterpret_cast<double *>(tile + n * S);
#pragma unroll
				for (int p = 0; p < 2 * NP; ++p) {
					const int k = lane + kWave * p;
					if (k < K) trow[k] = yrow[k];
				}
				if ((K & 1) && lane == 0) trow[K] = 0.0;   // the empty half of the last piece: phase B reads it, no sum keeps it
			}
		}
		__syncthreads();   // single-wave workgroup: the wait that retires the transfers, and the published vector's too
		// ---- phase A: lane n against row n (the lanes beyond the chunk re-read row 0; nothing reads their result)
		double e;
		{
			const double2 *t2 = reinterpret_cast<const double2 *>(tile + (lane < cc ? lane : 0) * S);
			double dot = 0.0;
			if constexpr (KT > 0) {
				dot = phase_a_dot<KT, 8>(t2, vs);
			} else {
				const int full = K >> 1;
				int q = 0;
				for (; q + 4 <= full; q += 4) {
					double2 t[4], x[4];
#pragma unroll
					for (int u = 0; u < 4; ++u) {
						t[u] = t2[q + u];
						x[u] = vs[q + u];
					}
#pragma unroll
					for (int u = 0; u < 4; ++u) {
						dot = dot + x[u].x * t[u].x;
						dot = dot + x[u].y * t[u].y;
					}
				}
				for (; q < full; ++q) {
					const double2 t = t2[q];
					const double2 x = vs[q];
					dot = dot + x.x * t.x;
					dot = dot + x.y * t.y;
				}
				if constexpr (!DMA) {
					if (K & 1) dot = dot + vs[full].x * t2[full].x;
				}
			}
			if constexpr (IMPLICIT) {
				if constexpr (RESIDUAL) {
					const double cn = 1.0 + my_wgt;
					const double ac = my_val * cn, et = my_wgt * dot;
					e = ac - et;
				} else {
					e = dot * my_wgt;
				}
			} else {
				e = RESIDUAL ? my_val - dot : dot;
				if (a.wgt) e = e * my_wgt;
			}
		}
		// ---- phase B
		const char *tb = tile + voff;
		int n = phase_b_four<NP>(tb, S, e, 0, cc, lane, P, acc);
		phase_b_tail<NP, true>(tb, S, e, n, cc, lane, P, acc);
		__syncthreads();   // the tile is overwritten by the next chunk's gather
	}
}

template <int KT, int NP, bool DMA>
__global__ void __launch_bounds__(kWave) als_cg_kernel(AlsArgs a, int steps, int nch)
{
	static_assert(KT == 0 || (DMA && KT % 2 == 0 && als_cg_passes(KT) == NP), "a compile-time K is an even K of the LDS-DMA gather");
	const int K = KT > 0 ? KT : a.K;
	const int P = als_cg_pieces(K);
	extern __shared__ __attribute__((aligned(16))) char lds[];
	double2 *vs = reinterpret_cast<double2 *>(lds);
	double *pr = reinterpret_cast<double *>(lds + als_cg_vec_bytes(K));
	char *tile = lds + 2 * als_cg_vec_bytes(K);
	const int lane = threadIdx.x;

	const int r = a.rowlist ? a.rowlist[blockIdx.x] : (int) blockIdx.x;
	const int beg = a.ptr[r], cnt = a.ptr[r + 1] - beg;
	const size_t xrow = (size_t) r * a.ldx;
	double2 xold[NP];
	als_cg_load_row<NP, DMA>(a.X_old + xrow, lane, K, xold);
	if (cnt <= 0) {   // a row without entries keeps X_old's bits and is not projected
		als_cg_store_row<NP, DMA>(a.X_new + xrow, lane, K, xold);
		if (lane == 0) atomicAdd(&a.counts[1], 1ull);
		return;
	}
	const double ridge = a.count_scaled ? a.lambda * (double) cnt : a.lambda;
	const int f = a.frozen;

	// C0 .. C3
	double2 x[NP], rr[NP], pp[NP], qq[NP];
#pragma unroll
	for (int p = 0; p < NP; ++p) x[p] = xold[p];
	als_cg_publish<NP>(vs, lane, P, x);
	als_cg_pass<KT, NP, DMA, true>(a, K, nch, beg, cnt, lane, vs, tile, rr);
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		const double tx = ridge * x[p].x, ty = ridge * x[p].y;
		rr[p].x = rr[p].x - tx;
		rr[p].y = rr[p].y - ty;
	}
	als_cg_set_column<NP>(rr, lane, f, 0.0);
#pragma unroll
	for (int p = 0; p < NP; ++p) pp[p] = rr[p];
	double rs = als_cg_dot<NP>(pr, lane, K, rr, rr);

	// C4
	bool pd = true;
	for (int s = 1; s <= steps; ++s) {
		if (rs == 0.0) break;
		als_cg_publish<NP>(vs, lane, P, pp);
		als_cg_pass<KT, NP, DMA, false>(a, K, nch, beg, cnt, lane, vs, tile, qq);
#pragma unroll
		for (int p = 0; p < NP; ++p) {
			const double tx = ridge * pp[p].x, ty = ridge * pp[p].y;
			qq[p].x = qq[p].x + tx;
			qq[p].y = qq[p].y + ty;
		}
		als_cg_set_column<NP>(qq, lane, f, 0.0);
		const double pq = als_cg_dot<NP>(pr, lane, K, pp, qq);
		if (!(pq > 0.0)) {
			pd = false;
			break;
		}
		const double alpha = rs / pq;
#pragma unroll
		for (int p = 0; p < NP; ++p) {
			const double ax = alpha * pp[p].x, ay = alpha * pp[p].y;
			x[p].x = x[p].x + ax;
			x[p].y = x[p].y + ay;
			const double bx = alpha * qq[p].x, by = alpha * qq[p].y;
			rr[p].x = rr[p].x - bx;
			rr[p].y = rr[p].y - by;
		}
		if (s == steps) break;   // C4f of the last step does not reach the stored row
		const double rn = als_cg_dot<NP>(pr, lane, K, rr, rr);
		const double beta = rn / rs;
#pragma unroll
		for (int p = 0; p < NP; ++p) {
			const double bx = beta * pp[p].x, by = beta * pp[p].y;
			pp[p].x = rr[p].x + bx;
			pp[p].y = rr[p].y + by;
		}
		rs = rn;
	}

	// C5: the box on the bounded columns, then the frozen select; a row that is not positive definite keeps X_old's bits
	if (pd) {
		const Box box = load_box(offsetof(AlsArgs, box));   // read here, not held in scalar registers across the passes
#pragma unroll
		for (int p = 0; p < NP; ++p) {
			const int q = lane + kWave * p;
			if (2 * q < box.columns) x[p].x = box_clamp(x[p].x, box.lo, box.hi);
			if (2 * q + 1 < box.columns) x[p].y = box_clamp(x[p].y, box.lo, box.hi);
			if (f >= 0 && (f >> 1) == q) {
				if (f & 1)
					x[p].y = xold[p].y;
				else
					x[p].x = xold[p].x;
			}
		}
	}
	if (pd)
		als_cg_store_row<NP, DMA>(a.X_new + xrow, lane, K, x);
	else
		als_cg_store_row<NP, DMA>(a.X_new + xrow, lane, K, xold);
	if (lane == 0) atomicAdd(&a.counts[pd ? 0 : 2], 1ull);
}

}  // namespace mf
