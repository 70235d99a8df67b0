// mf_als.hip.h -- alternating least squares: per row of a side one K x K ridge system, formed and solved in FP64.
//
// With the other side Y frozen, row r of X is the solution of (sum_n y_n yw_n^T + ridge I) x = sum_n a'_n yw_n over the
// row's entries, and include/matfact_hip.h defines every operation of it: the Gram matrix and the right-hand side as serial
// sums in the side's entry order, the Cholesky factorisation, the two column-oriented triangular solves, the box, the frozen
// select.  One kernel body does all of it for one row, run by a GROUP of threads that owns a slab of LDS:
//   phase 1  the row's entries in chunks: {idx, a', w} of a chunk, then its Y rows gathered into an LDS tile (and the tile
//            of yw = y * w beside it on a weighted plan; without weights the one tile is both);
//   phase 2  every thread owns up to NB square BS x BS blocks of the lower triangle in registers and adds the chunk's
//            products onto them entry by entry -- 2 BS LDS reads feed BS^2 products --, thread p < K also b[p];
//   phase 3  the triangle goes to LDS (packed by rows), the ridge goes onto the diagonal, the frozen column is cut out;
//   phase 4  right-looking Cholesky in LDS: column j is scaled, then its rank-1 update is applied to the trailing triangle,
//            j ascending -- per element the chain s = s - C[i][t] * C[j][t], t ascending, of the definition;
//   phase 5  forward and backward solve, thread p holding b[p] / z[p] in a register and taking column j's term as soon as
//            z[j] / x[j] exists: the column-oriented orders of the definition;
//   phase 6  box, frozen select, store; one of the side's three counters.
// Two forms, the same body and so the same bits:
//   als_kernel<256, 4, NB>  one 256-thread workgroup per row, 4 x 4 blocks, chunks of kAlsChunkWg entries: any K <= 128;
//   als_kernel<64, 2, NB>   one wave per row and four rows per workgroup, 2 x 2 blocks, chunks of kAlsChunkWave entries,
//                           the group synchronised without a workgroup barrier: K <= kAlsWaveMaxK.
// No FP64 matrix instruction (its accumulation order is not ours to state), no fused multiply-add outside the correctly
// rounded sqrt and division (the library is built with -ffp-contract=off).  Nothing here writes outside its own row of
// X_new: the padding of a row is never touched.
#pragma once
#include "mf_common.hip.h"
#include "mf_sweep.hip.h"

namespace mf {

constexpr int kAlsMaxK = 128;        // the triangle of a row lives in LDS: 8256 doubles at K = 128
constexpr int kAlsWaveMaxK = 32;     // widest row of the one-wave-per-row form
constexpr int kAlsThreads = 256;     // workgroup size of both forms
constexpr int kAlsChunkWg = 16;      // entries per gather chunk, workgroup form
constexpr int kAlsChunkWave = 8;     // ... one-wave form

struct AlsArgs {
	int nrows, K;
	int ldx, ldy;                        // row pitch of X and of Y in doubles
	int frozen;                          // frozen column of the side or -1
	int count_scaled;                    // 1: ridge = lambda * (double) cnt, 0: ridge = lambda
	double lambda;
	const int *__restrict__ ptr;
	const int *__restrict__ idx;
	const double *__restrict__ val;
	const double *__restrict__ wgt;      // per-entry weights in the order of (idx, val), or null
	const double *__restrict__ X_old;
	const double *__restrict__ Y;
	double *__restrict__ X_new;
	const int *__restrict__ rowlist;     // optional: the launch covers rows rowlist[0..nrows) instead of 0..nrows
	unsigned long long *__restrict__ counts;   // solved, kept_empty, kept_not_pd
	Box box;                             // columns = 0: no projection
};

// geometry shared by the kernel and the launch (host and device)
__host__ __device__ constexpr int als_padded_k(int K, int BS) { return (K + BS - 1) / BS * BS; }
__host__ __device__ constexpr int als_blocks(int K, int BS)
{
	const int kb = (K + BS - 1) / BS;
	return kb * (kb + 1) / 2;
}
__host__ __device__ constexpr int als_triangle(int K) { return K * (K + 1) / 2; }
// LDS doubles of one group: the y tile, the yw tile (weighted), a' and w of a chunk, idx of a chunk (ints, two to a
// double), the triangle, the diagonal of C, z and x
__host__ __device__ constexpr int als_group_doubles(int K, int BS, int nch, bool weighted)
{
	return (weighted ? 2 : 1) * nch * als_padded_k(K, BS) + 2 * nch + (nch + 1) / 2 + als_triangle(K) + 3 * K;
}

// a barrier of the group: the workgroup's, or -- one wave -- nothing but the order of its own LDS accesses
template <int THREADS>
__device__ __forceinline__ void als_sync()
{
	if constexpr (THREADS == kAlsThreads) {
		__syncthreads();
	} else {
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
	}
}

__device__ __forceinline__ int als_tri(int p, int q) { return p * (p + 1) / 2 + q; }

// What the implicit instances take beside AlsArgs (mf_plan_set_als: MF_ALS_IMPLICIT): the Gram of the whole other side
// (mf_gram.hip.h), a packed lower triangle, and the confidence scale.
struct AlsImplicit {
	const double *__restrict__ S;
	double conf;
};
__device__ __forceinline__ AlsImplicit als_implicit_of() { return AlsImplicit{nullptr, 0.0}; }
__device__ __forceinline__ AlsImplicit als_implicit_of(AlsImplicit im) { return im; }

// ---- the phases as functions: als_normal_kernel and als_solve_normal_kernel (mf_als_normal.hip.h) run the two halves of the
// solve with a record in global memory in between.  They restate the body of als_kernel below statement for statement;
// als_kernel keeps its own text because calling these functions from it changed the instruction lists of all its twelve
// instances (integer address arithmetic; profiles/als_shards/kernels_parent_vs_new.txt).  A change of a phase goes into both.

// the LDS slab of one group: als_group_doubles doubles from `base`
struct AlsSlab {
	double *ytile, *ywtile, *ap, *wl;
	int *ids;
	double *G, *dg, *zs, *xs;
};
__device__ __forceinline__ AlsSlab als_slab(double *base, int Kp, int NCH, int K, bool weighted)
{
	AlsSlab s;
	s.ytile = base;
	s.ywtile = weighted ? s.ytile + NCH * Kp : s.ytile;
	s.ap = s.ywtile + NCH * Kp;
	s.wl = s.ap + NCH;
	s.ids = (int *) (s.wl + NCH);
	s.G = s.wl + NCH + (NCH + 1) / 2;
	s.dg = s.G + als_triangle(K);
	s.zs = s.dg + K;
	s.xs = s.zs + K;
	return s;
}

// the blocks of a thread: block e = tid + i * THREADS of the triangle of blocks, rows bp >= columns bq
template <int THREADS, int BS, int NB>
__device__ __forceinline__ void als_own_blocks(int tid, int nblocks, int (&bp)[NB], int (&bq)[NB])
{
#pragma unroll
	for (int i = 0; i < NB; ++i) {
		const int e = tid + i * THREADS;
		int p = (int) ((sqrtf(8.0f * (float) e + 1.0f) - 1.0f) * 0.5f);
		while (p * (p + 1) / 2 > e) --p;
		while ((p + 1) * (p + 2) / 2 <= e) ++p;
		bp[i] = e < nblocks ? p * BS : 0;
		bq[i] = e < nblocks ? (e - p * (p + 1) / 2) * BS : 0;
	}
}

// phases 1 and 2 over the row's entries beg .. beg + cnt: every acc[i][u][v] and bacc is one serial chain in entry order
template <int THREADS, int BS, int NB, bool IMPLICIT>
__device__ __forceinline__ void als_accumulate(const AlsArgs &a, double conf, int K, int Kp, int tid, int beg, int cnt, int f, double xf,
                                               bool weighted, int nblocks, double *ytile, double *ywtile, double *ap, double *wl, int *ids,
                                               const int (&bp)[NB], const int (&bq)[NB], double (&acc)[NB][BS][BS], double &bacc)
{
	constexpr int NCH = THREADS == kAlsThreads ? kAlsChunkWg : kAlsChunkWave;
	for (int c0 = 0; c0 < cnt; c0 += NCH) {
		const int cc = min(NCH, cnt - c0);
		// phase 1a: idx, a' and w of the chunk's entries
		if (tid < cc) {
			const int e = beg + c0 + tid, id = a.idx[e];
			double av = a.val[e];
			if (f >= 0) {
				const double t = xf * a.Y[(size_t) id * a.ldy + f];
				av = av - t;
			}
			ids[tid] = id;
			if constexpr (IMPLICIT) {   // e_n, and ac_n = a_n * c_n with c_n = 1.0 + e_n
				const double en = a.wgt ? conf * a.wgt[e] : conf;
				const double cn = 1.0 + en;
				ap[tid] = av * cn;
				wl[tid] = en;
			} else {
				ap[tid] = av;
				wl[tid] = weighted ? a.wgt[e] : 1.0;
			}
		}
		als_sync<THREADS>();
		// phase 1b: the Y rows of the chunk, zero beyond column K
		{
			int n = tid / Kp, k = tid - n * Kp;
			const int dn = THREADS / Kp, dk = THREADS - dn * Kp;
			while (n < cc) {
				const double y = k < K ? a.Y[(size_t) ids[n] * a.ldy + k] : 0.0;
				ytile[n * Kp + k] = y;
				if (weighted) ywtile[n * Kp + k] = y * wl[n];
				n += dn, k += dk;
				if (k >= Kp) k -= Kp, ++n;
			}
		}
		als_sync<THREADS>();
		// phase 2: G[p][q] = G[p][q] + (y_n[p] * yw_n[q]) and b[p] = b[p] + (a'_n * yw_n[p]), n ascending
		for (int n = 0; n < cc; ++n) {
			const double *yr = ytile + n * Kp, *ywr = ywtile + n * Kp;
#pragma unroll
			for (int i = 0; i < NB; ++i) {
				if (tid + i * THREADS < nblocks) {
					double yp[BS], yq[BS];
#pragma unroll
					for (int u = 0; u < BS; ++u) yp[u] = yr[bp[i] + u], yq[u] = ywr[bq[i] + u];
#pragma unroll
					for (int u = 0; u < BS; ++u)
#pragma unroll
						for (int v = 0; v < BS; ++v) {
							const double t = yp[u] * yq[v];
							acc[i][u][v] = acc[i][u][v] + t;
						}
				}
			}
			if (tid < K) {
				const double t = ap[n] * (IMPLICIT ? yr[tid] : ywr[tid]);
				bacc = bacc + t;
			}
		}
		als_sync<THREADS>();
	}
}

// phase 3, first half: the register blocks into the packed triangle in LDS
template <int THREADS, int BS, int NB>
__device__ __forceinline__ void als_blocks_to_lds(int K, int tid, int nblocks, const int (&bp)[NB], const int (&bq)[NB],
                                                  const double (&acc)[NB][BS][BS], double *G)
{
#pragma unroll
	for (int i = 0; i < NB; ++i) {
		if (tid + i * THREADS < nblocks) {
#pragma unroll
			for (int u = 0; u < BS; ++u)
#pragma unroll
				for (int v = 0; v < BS; ++v) {
					const int p = bp[i] + u, q = bq[i] + v;
					if (p < K && q <= p) G[als_tri(p, q)] = acc[i][u][v];
				}
		}
	}
}

// phase 3, second half, to phase 6: the triangle is in G and the group has synchronised; thread p < K holds b[p] in bacc.
// The ridge (cntd: the row's entry count as a double), the frozen cut, Cholesky, the two solves, the box, the frozen select, the store and the row's counter.
template <int THREADS>
__device__ __forceinline__ void als_ridge_solve_store(const AlsArgs &a, int K, int tid, int f, double xf, double xold, size_t xrow, double cntd,
                                                      double bacc, double *G, double *dg, double *zs, double *xs)
{
	constexpr int TD = THREADS == kAlsThreads ? 16 : 8;   // the trailing update walks the triangle as TD x TD threads
	if (tid < K) {
		const double ridge = a.count_scaled ? a.lambda * cntd : a.lambda;
		G[als_tri(tid, tid)] = G[als_tri(tid, tid)] + ridge;
		if (f >= 0) {
			if (tid < f) G[als_tri(f, tid)] = 0.0;
			if (tid > f) G[als_tri(tid, f)] = 0.0;
			if (tid == f) G[als_tri(f, f)] = 1.0, bacc = xf;
		}
	}
	als_sync<THREADS>();

	// phase 4: Cholesky, right-looking.  Every thread of the group reads the same pivot, so the exit is uniform
	bool pd = true;
	const int ti = tid / TD, tq = tid % TD;
	for (int j = 0; j < K; ++j) {
		const double s = G[als_tri(j, j)];
		if (!(s > 0.0)) {
			pd = false;
			break;
		}
		const double d = sqrt(s);
		if (tid == 0) dg[j] = d;
		for (int i = j + 1 + tid; i < K; i += THREADS) G[als_tri(i, j)] = G[als_tri(i, j)] / d;
		als_sync<THREADS>();
		for (int i = j + 1 + ti; i < K; i += TD) {
			const double cij = G[als_tri(i, j)];
			for (int q = j + 1 + tq; q <= i; q += TD) {
				const double t = cij * G[als_tri(q, j)];
				G[als_tri(i, q)] = G[als_tri(i, q)] - t;
			}
		}
		als_sync<THREADS>();
	}

	double x = xold;
	if (pd) {
		// phase 5: C z = b, j ascending; C^T x = z, j descending
		double bi = bacc;
		for (int j = 0; j < K; ++j) {
			if (tid == j) zs[j] = bi / dg[j];
			als_sync<THREADS>();
			if (tid > j && tid < K) {
				const double t = G[als_tri(tid, j)] * zs[j];
				bi = bi - t;
			}
		}
		double zi = tid < K ? zs[tid] : 0.0;   // its own store
		for (int j = K - 1; j >= 0; --j) {
			if (tid == j) xs[j] = zi / dg[j];
			als_sync<THREADS>();
			if (tid < j) {
				const double t = G[als_tri(j, tid)] * xs[j];
				zi = zi - t;
			}
		}
		// phase 6: the box on the bounded columns, then the frozen select
		if (tid < K) {
			x = xs[tid];
			if (tid < a.box.columns) x = box_clamp(x, a.box.lo, a.box.hi);
			if (tid == f) x = xold;
		}
	}
	if (tid < K) a.X_new[xrow + tid] = x;
	if (tid == 0) atomicAdd(&a.counts[pd ? 0 : 2], 1ull);
}

// als_kernel<THREADS, BS, NB>(AlsArgs) is the explicit solve; als_kernel<THREADS, BS, NB, AlsImplicit>(AlsArgs, AlsImplicit) the
// implicit one: the same body with steps 1-5 changed as the header states them -- e_n = conf * w_n (conf without weights) is
// what the second tile is scaled by, a_n goes in as a_n * (1.0 + e_n), the triangle starts at S where it otherwise starts at
// 0.0, b sums against y_n, not ye_n, and a row without entries is solved like any other (its sums are empty).  No frozen
// column there: the launch refuses it.
template <int THREADS, int BS, int NB, class... IM>
__global__ void __launch_bounds__(kAlsThreads) als_kernel(AlsArgs a, IM... im)
{
	constexpr bool IMPLICIT = sizeof...(IM) == 1;
	constexpr int kGroups = kAlsThreads / THREADS;
	constexpr int NCH = THREADS == kAlsThreads ? kAlsChunkWg : kAlsChunkWave;
	constexpr int TD = THREADS == kAlsThreads ? 16 : 8;   // the trailing update walks the triangle as TD x TD threads
	extern __shared__ double als_lds[];

	const int K = a.K, Kp = als_padded_k(K, BS);
	const bool weighted = IMPLICIT || a.wgt != nullptr;   // the implicit solve always keeps two tiles, y and ye
	const int grp = (int) threadIdx.x / THREADS, tid = (int) threadIdx.x % THREADS;
	const int slot = (int) blockIdx.x * kGroups + grp;
	if (slot >= a.nrows) return;   // a whole group: the one-wave form has no workgroup barrier, the other one row per workgroup
	const int r = a.rowlist ? a.rowlist[slot] : slot;

	double *ytile = als_lds + (size_t) grp * als_group_doubles(K, BS, NCH, weighted);
	double *ywtile = weighted ? ytile + NCH * Kp : ytile;
	double *ap = ywtile + NCH * Kp;
	double *wl = ap + NCH;
	int *ids = (int *) (wl + NCH);
	double *G = wl + NCH + (NCH + 1) / 2;
	double *dg = G + als_triangle(K);
	double *zs = dg + K;
	double *xs = zs + K;

	const int beg = a.ptr[r], cnt = a.ptr[r + 1] - beg;
	const int f = IMPLICIT ? -1 : a.frozen;
	const size_t xrow = (size_t) r * a.ldx;
	const double xold = tid < K ? a.X_old[xrow + tid] : 0.0;

	if constexpr (!IMPLICIT) {
		if (cnt <= 0) {   // a row without entries keeps X_old's bits and is not projected
			if (tid < K) a.X_new[xrow + tid] = xold;
			if (tid == 0) atomicAdd(&a.counts[1], 1ull);
			return;
		}
	}
	const double xf = f >= 0 ? a.X_old[xrow + f] : 0.0;

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
			for (int v = 0; v < BS; ++v) {
				if constexpr (IMPLICIT) {   // step 3 starts at S[p][q]
					const int gp = bp[i] + u, gq = bq[i] + v;
					acc[i][u][v] = e < nblocks && gp < K && gq <= gp ? als_implicit_of(im...).S[als_tri(gp, gq)] : 0.0;
				} else {
					acc[i][u][v] = 0.0;
				}
			}
	}
	double bacc = 0.0;

	for (int c0 = 0; c0 < cnt; c0 += NCH) {
		const int cc = min(NCH, cnt - c0);
		// phase 1a: idx, a' and w of the chunk's entries
		if (tid < cc) {
			const int e = beg + c0 + tid, id = a.idx[e];
			double av = a.val[e];
			if (f >= 0) {
				const double t = xf * a.Y[(size_t) id * a.ldy + f];
				av = av - t;
			}
			ids[tid] = id;
			if constexpr (IMPLICIT) {   // e_n, and ac_n = a_n * c_n with c_n = 1.0 + e_n
				const double conf = als_implicit_of(im...).conf;
				const double en = a.wgt ? conf * a.wgt[e] : conf;
				const double cn = 1.0 + en;
				ap[tid] = av * cn;
				wl[tid] = en;
			} else {
				ap[tid] = av;
				wl[tid] = weighted ? a.wgt[e] : 1.0;
			}
		}
		als_sync<THREADS>();
		// phase 1b: the Y rows of the chunk, zero beyond column K
		{
			int n = tid / Kp, k = tid - n * Kp;
			const int dn = THREADS / Kp, dk = THREADS - dn * Kp;
			while (n < cc) {
				const double y = k < K ? a.Y[(size_t) ids[n] * a.ldy + k] : 0.0;
				ytile[n * Kp + k] = y;
				if (weighted) ywtile[n * Kp + k] = y * wl[n];
				n += dn, k += dk;
				if (k >= Kp) k -= Kp, ++n;
			}
		}
		als_sync<THREADS>();
		// phase 2: G[p][q] = G[p][q] + (y_n[p] * yw_n[q]) and b[p] = b[p] + (a'_n * yw_n[p]), n ascending
		for (int n = 0; n < cc; ++n) {
			const double *yr = ytile + n * Kp, *ywr = ywtile + n * Kp;
#pragma unroll
			for (int i = 0; i < NB; ++i) {
				if (tid + i * THREADS < nblocks) {
					double yp[BS], yq[BS];
#pragma unroll
					for (int u = 0; u < BS; ++u) yp[u] = yr[bp[i] + u], yq[u] = ywr[bq[i] + u];
#pragma unroll
					for (int u = 0; u < BS; ++u)
#pragma unroll
						for (int v = 0; v < BS; ++v) {
							const double t = yp[u] * yq[v];
							acc[i][u][v] = acc[i][u][v] + t;
						}
				}
			}
			if (tid < K) {
				const double t = ap[n] * (IMPLICIT ? yr[tid] : ywr[tid]);
				bacc = bacc + t;
			}
		}
		als_sync<THREADS>();
	}

	// phase 3: the triangle to LDS, the ridge, the frozen column
#pragma unroll
	for (int i = 0; i < NB; ++i) {
		if (tid + i * THREADS < nblocks) {
#pragma unroll
			for (int u = 0; u < BS; ++u)
#pragma unroll
				for (int v = 0; v < BS; ++v) {
					const int p = bp[i] + u, q = bq[i] + v;
					if (p < K && q <= p) G[als_tri(p, q)] = acc[i][u][v];
				}
		}
	}
	als_sync<THREADS>();
	if (tid < K) {
		const double ridge = a.count_scaled ? a.lambda * (double) cnt : a.lambda;
		G[als_tri(tid, tid)] = G[als_tri(tid, tid)] + ridge;
		if (f >= 0) {
			if (tid < f) G[als_tri(f, tid)] = 0.0;
			if (tid > f) G[als_tri(tid, f)] = 0.0;
			if (tid == f) G[als_tri(f, f)] = 1.0, bacc = xf;
		}
	}
	als_sync<THREADS>();

	// phase 4: Cholesky, right-looking.  Every thread of the group reads the same pivot, so the exit is uniform
	bool pd = true;
	const int ti = tid / TD, tq = tid % TD;
	for (int j = 0; j < K; ++j) {
		const double s = G[als_tri(j, j)];
		if (!(s > 0.0)) {
			pd = false;
			break;
		}
		const double d = sqrt(s);
		if (tid == 0) dg[j] = d;
		for (int i = j + 1 + tid; i < K; i += THREADS) G[als_tri(i, j)] = G[als_tri(i, j)] / d;
		als_sync<THREADS>();
		for (int i = j + 1 + ti; i < K; i += TD) {
			const double cij = G[als_tri(i, j)];
			for (int q = j + 1 + tq; q <= i; q += TD) {
				const double t = cij * G[als_tri(q, j)];
				G[als_tri(i, q)] = G[als_tri(i, q)] - t;
			}
		}
		als_sync<THREADS>();
	}

	double x = xold;
	if (pd) {
		// phase 5: C z = b, j ascending; C^T x = z, j descending
		double bi = bacc;
		for (int j = 0; j < K; ++j) {
			if (tid == j) zs[j] = bi / dg[j];
			als_sync<THREADS>();
			if (tid > j && tid < K) {
				const double t = G[als_tri(tid, j)] * zs[j];
				bi = bi - t;
			}
		}
		double zi = tid < K ? zs[tid] : 0.0;   // its own store
		for (int j = K - 1; j >= 0; --j) {
			if (tid == j) xs[j] = zi / dg[j];
			als_sync<THREADS>();
			if (tid < j) {
				const double t = G[als_tri(j, tid)] * xs[j];
				zi = zi - t;
			}
		}
		// phase 6: the box on the bounded columns, then the frozen select
		if (tid < K) {
			x = xs[tid];
			if (tid < a.box.columns) x = box_clamp(x, a.box.lo, a.box.hi);
			if (tid == f) x = xold;
		}
	}
	if (tid < K) a.X_new[xrow + tid] = x;
	if (tid == 0) atomicAdd(&a.counts[pd ? 0 : 2], 1ull);
}

}  // namespace mf
