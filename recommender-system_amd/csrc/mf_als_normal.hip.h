// mf_als_normal.hip.h -- the ALS solve cut in two at the normal equations (include/matfact_hip.h, mf_plan_als_normal and
// mf_plan_als_solve_normal): what user shards need for the item side, whose Gram matrices are sums over all users.
//
// A NORMAL RECORD of a row is `pitch` doubles in caller-owned device memory: the packed lower triangle of G (als_tri), b, the
// row's entry count as a double, +0.0 pads up to als_normal_pitch(K).  The records are linear in the entries, so the
// buffers of the plans that partition the other side are summed elementwise and every plan solves the sums.
//   als_normal_kernel        phases 1-2 of als_kernel (mf_als.hip.h: the same functions, the same slab, the same
//                            thread-to-block map, so every element is the same serial chain), the triangle always from 0.0;
//                            then the triangle, b, the count and the pad staged in the LDS G region (b, count and pad land on
//                            the dg / zs slots behind it) and streamed out as 16-byte stores, contiguous over the group;
//   als_normal_gram_kernel   record `rows`: the Gram of the other side under the implicit kind, +0.0 otherwise;
//   als_solve_normal_kernel  the record back into LDS by 16-byte loads -- under the implicit kind S + N, S on the left --,
//                            b[p] into thread p's register, then phases 3-6 of als_kernel.  No gather tile: T + 3 K doubles
//                            of LDS per group.
// Every record is addressed as (size_t) r * pitch: the user side of a large problem is beyond 2^32 bytes.
#pragma once
#include "mf_als.hip.h"

namespace mf {

struct AlsNormal {
	double *__restrict__ N;   // (rows + 1) records of `pitch` doubles, 16-byte aligned, pitch even
	long long pitch;
	int rows;                 // the side's row count: record `rows` is the Gram record
	int implicit;             // the solve adds the Gram record's triangle (left operand) to every row's
};

// the smallest even number of doubles that holds the triangle, b and the count
__host__ __device__ constexpr int als_normal_pitch(int K) { return (als_triangle(K) + K + 1 + 1) / 2 * 2; }
// LDS doubles of one group of the solve: the triangle, the diagonal of C, z and x
__host__ __device__ constexpr int als_solve_normal_doubles(int K) { return als_triangle(K) + 3 * K; }

template <int THREADS, int BS, int NB, class... IM>
__global__ void __launch_bounds__(kAlsThreads) als_normal_kernel(AlsArgs a, AlsNormal nr, IM... im)
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
	const double xf = f >= 0 ? a.X_old[(size_t) r * a.ldx + f] : 0.0;

	// a row without local entries runs no chunk: every chain stays at its +0.0
	const int nblocks = als_blocks(K, BS);
	int bp[NB], bq[NB];
	double acc[NB][BS][BS];
	als_own_blocks<THREADS, BS, NB>(tid, nblocks, bp, bq);
#pragma unroll
	for (int i = 0; i < NB; ++i)
#pragma unroll
		for (int u = 0; u < BS; ++u)
#pragma unroll
			for (int v = 0; v < BS; ++v) acc[i][u][v] = 0.0;
	double bacc = 0.0;
	als_accumulate<THREADS, BS, NB, IMPLICIT>(a, als_implicit_of(im...).conf, K, Kp, tid, beg, cnt, f, xf, weighted, nblocks, s.ytile, s.ywtile, s.ap, s.wl,
	                                          s.ids, bp, bq, acc, bacc);

	// the record in LDS: the triangle as phase 3 packs it, b, the count and the pad behind it (T + K + 2 <= T + 3 K)
	const int T = als_triangle(K), np = als_normal_pitch(K);
	als_blocks_to_lds<THREADS, BS, NB>(K, tid, nblocks, bp, bq, acc, s.G);
	if (tid < K) s.G[T + tid] = bacc;
	if (tid == 0) {
		s.G[T + K] = (double) cnt;
		if (T + K + 1 < np) s.G[T + K + 1] = 0.0;
	}
	als_sync<THREADS>();
	double *rec = nr.N + (size_t) r * (size_t) nr.pitch;
	for (int i = 2 * tid; i < np; i += 2 * THREADS) {   // np is even: whole pairs
		double2 v;
		v.x = s.G[i], v.y = s.G[i + 1];
		*reinterpret_cast<double2 *>(rec + i) = v;
	}
}

// Record `rows`: S's triangle (null: none) and +0.0 in every other slot of the minimum pitch.
__global__ void __launch_bounds__(kAlsThreads) als_normal_gram_kernel(const double *__restrict__ S, int triangle, int np, double *__restrict__ rec)
{
	const int e = (int) blockIdx.x * kAlsThreads + (int) threadIdx.x;
	if (e < np) rec[e] = S && e < triangle ? S[e] : 0.0;
}

template <int THREADS>
__global__ void __launch_bounds__(kAlsThreads) als_solve_normal_kernel(AlsArgs a, AlsNormal nr)
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

	als_ridge_solve_store<THREADS>(a, K, tid, f, xf, xold, xrow, cntd, bacc, G, dg, zs, xs);
}

}  // namespace mf
