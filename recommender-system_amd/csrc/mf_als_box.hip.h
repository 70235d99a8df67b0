// mf_als_box.hip.h -- box-constrained ALS: cyclic coordinate descent on a row's normal equations in place of the Cholesky
// solve and the clamp behind it (include/matfact_hip.h, "Box-constrained ALS": steps B0-B4).
//
// The row's Gram triangle and right-hand side are formed exactly as als_kernel forms them (mf_als.hip.h: the same slab, the
// same thread-to-block map, the same functions, so every element is the same serial chain); what differs is the solver
// behind them, stated once in als_box_solve_store and run by both kernels:
//   als_box_kernel<THREADS, BS, NB, IM...>   phases 1-3 of als_kernel, then the box solver: the forms and instances of als_kernel;
//   als_box_solve_normal_kernel<THREADS>     the record of mf_als_normal.hip.h back into LDS, then the box solver.
// The solver is one serial chain of sweeps * K coordinate steps -- one division, one broadcast, one multiply-subtract per
// residual element -- so ONE WAVE owns it: lane l holds x and res of the columns l and l + 64 in registers, the step's
// res[j] and x[j] reach every lane through v_readlane, every lane forms d, y and dl redundantly (no second broadcast), and
// column j of Gs comes from the packed triangle in LDS (rows p < j: contiguous; rows p >= j: one element per row).  No
// workgroup barrier sits inside the phase: the other three waves of the workgroup form leave behind the barrier in front of it,
// they hold nothing the solver reads.
// LDS: nothing grows.  Of the slab's 3 K doubles behind the triangle the solver uses dg (the diagonal after the ridge and the
// frozen cut), zs (b, handed from thread p to the owning lane) and xs (the start x, read as x[t] by the residual); the
// launch asks for als_group_doubles / als_solve_normal_doubles, as the direct solve does.
// No FP64 matrix instruction, no fused multiply-add outside the correctly rounded division (-ffp-contract=off).  Nothing here
// writes outside its own row of X_new.
#pragma once
#include "mf_als.hip.h"
#include "mf_als_normal.hip.h"

namespace mf {

constexpr int kAlsBoxVectors = 3;   // dg, zs, xs: the K-vectors of the slab the solver uses
static_assert(als_group_doubles(128, 4, kAlsChunkWg, true) == 2 * kAlsChunkWg * 128 + 2 * kAlsChunkWg + (kAlsChunkWg + 1) / 2 + als_triangle(128) + kAlsBoxVectors * 128 &&
                  als_solve_normal_doubles(128) == als_triangle(128) + kAlsBoxVectors * 128,
              "the box solver lives in the K-vectors the direct solve has");

// Gs[p][j]: the symmetric read of the packed lower triangle
__device__ __forceinline__ double als_box_gs(const double *G, int p, int j) { return G[p >= j ? als_tri(p, j) : als_tri(j, p)]; }

// One coordinate step of B3 at column j = 64 * SLOT + (its lane): x, res and diag are the lane's elements of slot 0 and slot 1.
// Column j of Gs is read first: it does not depend on the chain, so its LDS latency passes under the division.  row[s] is the
// lane's row of slot s, clamped to K - 1: a lane without an element repeats the last row's work on a residual it never stores,
// and no read hangs on a lane mask.
template <int SLOT, bool TWO>
__device__ __forceinline__ void als_box_step(int lane, int j, const Box &box, const double *G, const int (&row)[2], const double (&diag)[2], double (&x)[2],
                                             double (&res)[2])
{
	const int src = j - 64 * SLOT;
	const double g0 = als_box_gs(G, row[0], j);
	double g1 = 0.0;
	if constexpr (TWO) g1 = als_box_gs(G, row[1], j);
	const double rj = readlane_f64(res[SLOT], src), xj = readlane_f64(x[SLOT], src), gjj = readlane_f64(diag[SLOT], src);
	const double d = rj / gjj;
	double y = xj + d;
	if (j < box.columns) y = box_clamp(y, box.lo, box.hi);
	const double dl = y - xj;
	if (lane == src) x[SLOT] = y;
	const double t0 = g0 * dl;
	res[0] = res[0] - t0;
	if constexpr (TWO) {
		const double t1 = g1 * dl;
		res[1] = res[1] - t1;
	}
}

// Behind phase 3's first half: the triangle is in G and the group has synchronised; thread p < K holds b[p] in bacc and
// X_old[r][p] in xold, thread l < 64 of the workgroup form X_old[r][l + 64] in xold1 (l + 64 < K).  The ridge (cntd: the row's
// entry count as a double), the frozen cut, B0-B4 and the row's counter.
template <int THREADS>
__device__ __forceinline__ void als_box_solve_store(const AlsArgs &a, int K, int tid, int f, double xf, double xold, double xold1, size_t xrow, double cntd,
                                                    double bacc, int sweeps, double *G, double *dg, double *zs, double *xs)
{
	constexpr bool TWO = THREADS == kAlsThreads;   // K > 64 has a second element per lane; the one-wave form ends at kAlsWaveMaxK
	static_assert(TWO || kAlsWaveMaxK <= 64, "one element per lane");
	if (tid < K) {
		const double ridge = a.count_scaled ? a.lambda * cntd : a.lambda;
		double g = G[als_tri(tid, tid)] + ridge;
		if (f >= 0) {
			if (tid < f) G[als_tri(f, tid)] = 0.0;
			if (tid > f) G[als_tri(tid, f)] = 0.0;
			if (tid == f) g = 1.0, bacc = xf;
		}
		G[als_tri(tid, tid)] = g;
		dg[tid] = g;
		zs[tid] = bacc;
	}
	als_sync<THREADS>();
	if (tid >= 64) return;   // the solver is one wave's

	const int lane = tid;
	const bool has[2] = {lane < K, TWO && lane + 64 < K};
	const double xo[2] = {xold, xold1};
	const int row[2] = {min(lane, K - 1), min(lane + 64, K - 1)};   // the rows whose column elements the lane reads (als_box_step)

	// B0: the diagonal test
	bool bad = false;
	double diag[2] = {1.0, 1.0};   // the lane's diagonal elements: a step takes G[j][j] from its owner, as it takes res[j]
#pragma unroll
	for (int s = 0; s < (TWO ? 2 : 1); ++s)
		if (has[s]) {
			diag[s] = dg[lane + 64 * s];
			if (!(diag[s] > 0.0)) bad = true;
		}
	const bool pd = __builtin_amdgcn_ballot_w64(bad) == 0ull;

	double x[2] = {xo[0], xo[1]};
	if (pd) {
		// B1: the start, in the box but for the frozen column
		double res[2] = {0.0, 0.0};
#pragma unroll
		for (int s = 0; s < (TWO ? 2 : 1); ++s) {
			const int p = lane + 64 * s;
			if (has[s]) {
				if (p < a.box.columns) x[s] = box_clamp(x[s], a.box.lo, a.box.hi);
				if (p == f) x[s] = xf;
				xs[p] = x[s];
				res[s] = zs[p];
			}
		}
		als_sync<64>();
		// B2: res[p] = b[p] - sum_t Gs[p][t] * x[t], t ascending
		for (int t = 0; t < K; ++t) {
			const double xt = xs[t];
			const double m0 = als_box_gs(G, row[0], t) * xt;
			res[0] = res[0] - m0;
			if constexpr (TWO) {
				const double m1 = als_box_gs(G, row[1], t) * xt;
				res[1] = res[1] - m1;
			}
		}
		// B3: the sweeps
		const int k0 = min(K, 64);
		for (int s = 0; s < sweeps; ++s) {
			for (int j = 0; j < k0; ++j)
				if (j != f) als_box_step<0, TWO>(lane, j, a.box, G, row, diag, x, res);
			if constexpr (TWO)
				for (int j = 64; j < K; ++j)
					if (j != f) als_box_step<1, TWO>(lane, j, a.box, G, row, diag, x, res);
		}
		// B4: the frozen column keeps X_old's bits
#pragma unroll
		for (int s = 0; s < (TWO ? 2 : 1); ++s)
			if (lane + 64 * s == f) x[s] = xo[s];
	}
#pragma unroll
	for (int s = 0; s < (TWO ? 2 : 1); ++s)
		if (has[s]) a.X_new[xrow + lane + 64 * s] = x[s];
	if (lane == 0) atomicAdd(&a.counts[pd ? 0 : 2], 1ull);
}

// als_box_kernel<THREADS, BS, NB>(AlsArgs, sweeps) under the explicit kinds, als_box_kernel<THREADS, BS, NB, AlsImplicit>(AlsArgs,
// sweeps, AlsImplicit) under the implicit one: als_kernel's steps 1-4 (the triangle from S there, and a row without entries
// solved like any other), then the box solver.
template <int THREADS, int BS, int NB, class... IM>
__global__ void __launch_bounds__(kAlsThreads) als_box_kernel(AlsArgs a, int sweeps, IM... im)
{
	constexpr bool IMPLICIT = sizeof...(IM) == 1;
	constexpr int kGroups = kAlsThreads / THREADS;
	constexpr int NCH = THREADS == kAlsThreads ? kAlsChunkWg : kAlsChunkWave;
	extern __shared__ double als_lds[];

	const int K = a.K, Kp = als_padded_k(K, BS);
	const bool weighted = IMPLICIT || a.wgt != nullptr;
	const int grp = (int) threadIdx.x / THREADS, tid = (int) threadIdx.x % THREADS;
	const int slot = (int) blockIdx.x * kGroups + grp;
	if (slot >= a.nrows) return;   // a whole group
	const int r = a.rowlist ? a.rowlist[slot] : slot;
	const AlsSlab s = als_slab(als_lds + (size_t) grp * als_group_doubles(K, BS, NCH, weighted), Kp, NCH, K, weighted);

	const int beg = a.ptr[r], cnt = a.ptr[r + 1] - beg;
	const int f = IMPLICIT ? -1 : a.frozen;
	const size_t xrow = (size_t) r * a.ldx;
	const double xold = tid < K ? a.X_old[xrow + tid] : 0.0;
	const double xold1 = tid < 64 && tid + 64 < K ? a.X_old[xrow + tid + 64] : 0.0;

	if constexpr (!IMPLICIT) {
		if (cnt <= 0) {   // a row without entries keeps X_old's bits and is not projected
			if (tid < K) a.X_new[xrow + tid] = xold;
			if (tid == 0) atomicAdd(&a.counts[1], 1ull);
			return;
		}
	}
	const double xf = f >= 0 ? a.X_old[xrow + f] : 0.0;

	const int nblocks = als_blocks(K, BS);
	int bp[NB], bq[NB];
	double acc[NB][BS][BS];
	als_own_blocks<THREADS, BS, NB>(tid, nblocks, bp, bq);
#pragma unroll
	for (int i = 0; i < NB; ++i)
#pragma unroll
		for (int u = 0; u < BS; ++u)
#pragma unroll
			for (int v = 0; v < BS; ++v) {
				if constexpr (IMPLICIT) {
					// step 3 starts at S[p][q].  An element outside the triangle (the padding of K, the upper half of a diagonal
					// block) is never stored, so it takes the nearest element's value: a clamped index, where a predicate would
					// be the one of als_blocks_to_lds and live, as a lane mask, across the whole accumulation
					const int gp = min(bp[i] + u, K - 1), gq = min(bq[i] + v, gp);
					acc[i][u][v] = als_implicit_of(im...).S[als_tri(gp, gq)];
				} else {
					acc[i][u][v] = 0.0;
				}
			}
	double bacc = 0.0;
	als_accumulate<THREADS, BS, NB, IMPLICIT>(a, als_implicit_of(im...).conf, K, Kp, tid, beg, cnt, f, xf, weighted, nblocks, s.ytile, s.ywtile, s.ap, s.wl,
	                                          s.ids, bp, bq, acc, bacc);
	als_blocks_to_lds<THREADS, BS, NB>(K, tid, nblocks, bp, bq, acc, s.G);
	als_sync<THREADS>();
	als_box_solve_store<THREADS>(a, K, tid, f, xf, xold, xold1, xrow, (double) cnt, bacc, sweeps, s.G, s.dg, s.zs, s.xs);
}

// als_solve_normal_kernel with the box solver behind the record
template <int THREADS>
__global__ void __launch_bounds__(kAlsThreads) als_box_solve_normal_kernel(AlsArgs a, AlsNormal nr, int sweeps)
{
	constexpr int kGroups = kAlsThreads / THREADS;
	extern __shared__ double als_lds[];

	const int K = a.K, T = als_triangle(K);
	const int grp = (int) threadIdx.x / THREADS, tid = (int) threadIdx.x % THREADS;
	const int slot = (int) blockIdx.x * kGroups + grp;
	if (slot >= a.nrows) return;   // a whole group
	const int r = a.rowlist ? a.rowlist[slot] : slot;
	double *G = als_lds + (size_t) grp * als_solve_normal_doubles(K);
	double *dg = G + T, *zs = dg + K, *xs = zs + K;

	const double *rec = nr.N + (size_t) r * (size_t) nr.pitch;
	const int f = a.frozen;   // -1 under the implicit kind: the caller has refused a frozen column
	const size_t xrow = (size_t) r * a.ldx;
	const double xold = tid < K ? a.X_old[xrow + tid] : 0.0;
	const double xold1 = tid < 64 && tid + 64 < K ? a.X_old[xrow + tid + 64] : 0.0;
	const double cntd = rec[T + K];

	if (!nr.implicit && !(cntd > 0.0)) {   // a row nobody has entries for keeps X_old's bits and is not projected
		if (tid < K) a.X_new[xrow + tid] = xold;
		if (tid == 0) atomicAdd(&a.counts[1], 1ull);
		return;
	}
	const double xf = f >= 0 ? a.X_old[xrow + f] : 0.0;

	// the triangle: pairs of the record, the pair that straddles its end keeps only the triangle's half
	const double *S = nr.N + (size_t) nr.rows * (size_t) nr.pitch;
	for (int i = 2 * tid; i < T; i += 2 * THREADS) {
		double2 v = *reinterpret_cast<const double2 *>(rec + i);
		if (nr.implicit) {
			const double2 sv = *reinterpret_cast<const double2 *>(S + i);
			v.x = sv.x + v.x, v.y = sv.y + v.y;
		}
		G[i] = v.x;
		if (i + 1 < T) G[i + 1] = v.y;
	}
	const double bacc = tid < K ? rec[T + tid] : 0.0;
	als_sync<THREADS>();

	als_box_solve_store<THREADS>(a, K, tid, f, xf, xold, xold1, xrow, cntd, bacc, sweeps, G, dg, zs, xs);
}

}  // namespace mf
