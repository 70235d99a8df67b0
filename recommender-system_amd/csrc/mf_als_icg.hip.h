// mf_als_icg.hip.h -- implicit-feedback alternating least squares by conjugate gradient: a fixed number of CG steps per row,
// FP64, no Cholesky.
//
// With the other side Y frozen, row r of X moves `steps` conjugate-gradient steps from its current value towards the
// solution of (S + sum_n e_n y_n y_n^T + ridge I) x = sum_n ac_n y_n, S = Y^T Y over ALL rows of Y (mf_gram.hip.h), and
// include/matfact_hip.h defines every operation of it (J0 .. J5).  The matrix is never formed: its product with a vector v
// is  sum_n e_n y_n (y_n . v)  +  S v  +  ridge v.  The first term is a pass of mf_als_cg.hip.h with the entry's factor
// changed (als_cg_pass<..., IMPLICIT>), and this kernel is assembled from that file's pieces: one wave per row, the vectors
// x, r, p, q in the column-pair lanes' registers, the same LDS layout and the same chunk.  The all-pairs term is new:
//   S v      S comes as a K x K square with an even row stride (gram_square_kernel below copies the packed triangle there,
//            the pad column of an odd K is +0.0), so lane l, which owns columns 2l and 2l+1, takes piece l of row j with ONE
//            16-byte load -- the lanes of a wave read a row of the square side by side -- and v[j] with a broadcast read of
//            the vector the pass published in LDS.  Two unfused multiplies and two adds per row, j ascending: a chain per
//            column, no sum across lanes, so the definition fixes the bits.  The loads run kIcgAhead rows ahead of their
//            adds.
// A row without entries is solved like any other: its entry sums are empty.  No frozen column (the launch refuses it).
// Three forms as in mf_als_cg.hip.h, NP = 1 throughout (K <= 128), the same operations in the same order and so the same
// bits.  No FP64 matrix instruction and nothing fused (-ffp-contract=off).  Nothing here reads or writes the padding of a
// row of X or Y.
#pragma once
#include "mf_als_cg.hip.h"
#include "mf_gram.hip.h"

namespace mf {

constexpr int kIcgAhead = 8;   // rows of the square in flight in front of their adds

// the square of S: K rows of als_icg_ld(K) doubles, row j holding S(j, 0..K) and, at an odd K, one +0.0
__host__ __device__ constexpr int als_icg_ld(int K) { return 2 * als_cg_pieces(K); }

// sq[j][k] = S[max(j,k)][min(j,k)] of the packed triangle, the pad column +0.0: one thread per element, no arithmetic
__global__ void __launch_bounds__(kGramThreads) gram_square_kernel(const double *__restrict__ tri, int K, int ld, double *__restrict__ sq)
{
	const int e = (int) blockIdx.x * kGramThreads + (int) threadIdx.x;
	if (e >= K * ld) return;
	const int j = e / ld, k = e - j * ld;
	sq[e] = k < K ? tri[j >= k ? als_tri(j, k) : als_tri(k, j)] : 0.0;
}

// acc[k] = (((0.0 + S(k,0) * v[0]) + S(k,1) * v[1]) + ...) for the two columns of this lane; v is what the pass published
// in LDS (vs), `row` points at this lane's piece of row 0 of the square.  The lanes beyond the row read piece 0: nothing
// keeps their sums.
template <int KT>
__device__ __forceinline__ void als_icg_sv(const double2 *__restrict__ row, int ld2, int K, const double *vs, double2 &acc)
{
	acc = make_double2(0.0, 0.0);
	const int n = KT > 0 ? KT : K;
	int j = 0;
	// a loop at a compile-time K too: unrolled whole it would hold every row of the square in registers
#pragma nounroll
	for (; j + kIcgAhead <= n; j += kIcgAhead) {
		double2 s[kIcgAhead];
		double v[kIcgAhead];
#pragma unroll
		for (int i = 0; i < kIcgAhead; ++i) s[i] = row[(size_t) (j + i) * ld2];
#pragma unroll
		for (int i = 0; i < kIcgAhead; ++i) v[i] = vs[j + i];
#pragma unroll
		for (int i = 0; i < kIcgAhead; ++i) {
			const double tx = s[i].x * v[i], ty = s[i].y * v[i];
			acc.x = acc.x + tx;
			acc.y = acc.y + ty;
		}
	}
	for (; j < n; ++j) {
		const double2 s = row[(size_t) j * ld2];
		const double v = vs[j];
		const double tx = s.x * v, ty = s.y * v;
		acc.x = acc.x + tx;
		acc.y = acc.y + ty;
	}
}

template <int KT, int NP, bool DMA>
__global__ void __launch_bounds__(kWave) als_icg_kernel(AlsArgs a, AlsImplicit im, int steps, int nch)
{
	static_assert(NP == 1, "the implicit kind stops at K = 128: one piece per lane");
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
	const double ridge = a.lambda;
	const double conf = im.conf;
	// this lane's piece of row 0 of the square (in pieces); a lane beyond the row takes piece 0
	const int ld2 = P;
	const double2 *__restrict__ srow = reinterpret_cast<const double2 *>(im.S) + (lane < P ? lane : 0);
	const double *vd = reinterpret_cast<const double *>(vs);

	// J0 .. J3
	double2 x[NP], rr[NP], pp[NP], qq[NP], sv;
#pragma unroll
	for (int p = 0; p < NP; ++p) x[p] = xold[p];
	als_cg_publish<NP>(vs, lane, P, x);
	als_cg_pass<KT, NP, DMA, true, true>(a, K, nch, beg, cnt, lane, vs, tile, rr, conf);
	__syncthreads();   // a row without entries has not waited for the published vector yet
	als_icg_sv<KT>(srow, ld2, K, vd, sv);
	{
		const double tx = ridge * x[0].x, ty = ridge * x[0].y;
		rr[0].x = (rr[0].x - sv.x) - tx;
		rr[0].y = (rr[0].y - sv.y) - ty;
	}
	pp[0] = rr[0];
	double rs = als_cg_dot<NP>(pr, lane, K, rr, rr);

	// J4
	bool pd = true;
	for (int s = 1; s <= steps; ++s) {
		if (rs == 0.0) break;
		als_cg_publish<NP>(vs, lane, P, pp);
		als_cg_pass<KT, NP, DMA, false, true>(a, K, nch, beg, cnt, lane, vs, tile, qq, conf);
		__syncthreads();
		als_icg_sv<KT>(srow, ld2, K, vd, sv);
		{
			const double tx = ridge * pp[0].x, ty = ridge * pp[0].y;
			qq[0].x = (qq[0].x + sv.x) + tx;
			qq[0].y = (qq[0].y + sv.y) + ty;
		}
		const double pq = als_cg_dot<NP>(pr, lane, K, pp, qq);
		if (!(pq > 0.0)) {
			pd = false;
			break;
		}
		const double alpha = rs / pq;
		{
			const double ax = alpha * pp[0].x, ay = alpha * pp[0].y;
			x[0].x = x[0].x + ax;
			x[0].y = x[0].y + ay;
			const double bx = alpha * qq[0].x, by = alpha * qq[0].y;
			rr[0].x = rr[0].x - bx;
			rr[0].y = rr[0].y - by;
		}
		if (s == steps) break;   // the last step's f does not reach the stored row
		const double rn = als_cg_dot<NP>(pr, lane, K, rr, rr);
		const double beta = rn / rs;
		{
			const double bx = beta * pp[0].x, by = beta * pp[0].y;
			pp[0].x = rr[0].x + bx;
			pp[0].y = rr[0].y + by;
		}
		rs = rn;
	}

	// J5: the box on the bounded columns; a row that is not positive definite keeps X_old's bits
	if (pd) {
		const Box box = load_box(offsetof(AlsArgs, box));   // read here, not held in scalar registers across the passes
		if (2 * lane < box.columns) x[0].x = box_clamp(x[0].x, box.lo, box.hi);
		if (2 * lane + 1 < box.columns) x[0].y = box_clamp(x[0].y, box.lo, box.hi);
		als_cg_store_row<NP, DMA>(a.X_new + xrow, lane, K, x);
	} else {
		als_cg_store_row<NP, DMA>(a.X_new + xrow, lane, K, xold);
	}
	if (lane == 0) atomicAdd(&a.counts[pd ? 0 : 2], 1ull);
}

}  // namespace mf
