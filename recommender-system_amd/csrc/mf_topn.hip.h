// mf_topn.hip.h -- top-N recommendations per user: a matrix-core pass that keeps the N+1 best approximate scores per user,
// certification of the N-member set with the margin of the top-1 step, exact re-scoring of the members, and an exact
// pass (the repeated print_output rule over all items) for every user the matrix cores cannot decide.
//
// Semantics (include/matfact_hip.h, mf_plan_recommend_topn): T_i = print_output's rule applied N times, each pick
// removed from the unrated set.  One application to a set S: S empty -> -1; first = min S; B[i][first] NaN -> first;
// otherwise the arg-max over the non-NaN scores of S, the lowest index on ties.  t_1 is exactly mf_plan_recommend's.
//
// Matrix-core form: K = 20 NC <= 100 and K = 16 NC <= 96 (64-user workgroups of four waves), K = 112, 128 and 256 (eight
// waves of 16 users: at 32 users per wave the L operand of K = 112 / 128 leaves the list walk no registers); every other
// K runs the exact form for all users (mf_plan_recommend_topn_info reports which form ran).
#pragma once
#include "mf_common.hip.h"
#include "mf_ring.hip.h"        // kHU, kHNB, kMI, mf_d4, rec_mfma2_lds, cert_margin

namespace mf {

constexpr int kTopnMax = 32;   // MF_TOPN_MAX

struct TopnArgs {
	int users, items, K;
	int ldl, ldr;                              // row pitch of L and of R in doubles (>= K)
	const double *__restrict__ L;
	const double *__restrict__ R;
	const int *__restrict__ csr_ptr;
	const int *__restrict__ csr_idx;           // item ids ascending within a user (the recommend mask)
	const double *__restrict__ lnorm;          // ||L[i]||_2 per user
	const unsigned long long *__restrict__ rnorm_max_bits;   // max_j ||R[j]||_2 as the bits of a double
	double thr_scale;                          // mf_backend_recommend_margin(K)
	int n;                                     // N, 1 .. kTopnMax
	int *__restrict__ out_items;               // users x n
	double *__restrict__ out_scores;           // users x n (NaN where the item is -1)
	const int *__restrict__ ulist;             // exact pass: only these users (nullptr: all)
	int *__restrict__ olist;                   // matrix-core pass, out: users that need the exact pass
	int *__restrict__ ocount;
	// item split (small problems): blockIdx.y = split s scores items [s * split_items, (s + 1) * split_items) and writes its
	// top-(N+1) list to part slot s of the user; topn_merge_kernel merges the nsplit lists and certifies
	int split_items, nsplit;                   // split_items 0: no split
	double *__restrict__ part_v;               // users x (nsplit + 1) x (n + 1); slot nsplit is the merge's scratch
	int *__restrict__ part_i;
	int *__restrict__ part_bad;                // users x nsplit
};

// B[i][j] exactly as mat2d_prod forms it (mat2d.c:100-113): sequential k from 0.0, separate multiply and add
__device__ __forceinline__ double topn_exact_score(const double *__restrict__ l, const double *__restrict__ r, int K)
{
	double b = 0.0;
	for (int k = 0; k < K; ++k) b = b + l[k] * r[k];
	return b;
}

// Two lists sorted by descending approximate score (item -1: empty slot, score -inf) -> the first m of their merge
__device__ __forceinline__ void topn_merge_lists(const double *av, const int *ai, const double *bv, const int *bi, int m,
                                                 double *ov, int *oi)
{
	int x = 0, y = 0;
	for (int r = 0; r < m; ++r) {
		const bool ta = !(bv[y] > av[x]);
		ov[r] = ta ? av[x] : bv[y];
		oi[r] = ta ? ai[x] : bi[y];
		x += ta;
		y += !ta;
	}
}

// Certification of user u from its merged approximate list v/it[0 .. N] (descending) and the non-finite flag.  Every
// matrix-core score is within err_i <= thr_i / 2 of B[i][j] (mf_recommend.hip.h, recommend_mfma_kernel), so with
// a_N - a_{N+1} > thr_i every member's exact score is strictly greater than every other unrated item's: the N members
// ARE the set of T_i.  A user with at most N unrated items (the list never filled) holds all of them.  ||L_i|| * max ||R_j||
// <= 1e300 bounds every partial sum of every exact score: they are all finite, so no NaN rule is involved.  Certified
// users get their members re-scored exactly and ordered by (score descending, index ascending); returns false for the rest.
__device__ bool topn_finish(const TopnArgs &a, int u, double *v, int *it, int bad, double rmax)
{
	const int N = a.n;
	int valid = 0;
	for (int r = 0; r <= N; ++r) valid += it[r] >= 0;
	const double ln = a.lnorm[u];
	const double thr = cert_margin(a.thr_scale, ln, rmax);
	if (bad || !(ln * rmax <= 1e300) || (valid > N && !((v[N - 1] - v[N]) > thr))) return false;
	const int n = min(valid, N);
	const double *l = a.L + (size_t) u * a.ldl;
	for (int r = 0; r < n; ++r) v[r] = topn_exact_score(l, a.R + (size_t) it[r] * a.ldr, a.K);
	for (int r = 1; r < n; ++r) {
		const double x = v[r];
		const int j = it[r];
		int p = r;
		while (p > 0 && (v[p - 1] < x || (v[p - 1] == x && it[p - 1] > j))) {
			v[p] = v[p - 1];
			it[p] = it[p - 1];
			--p;
		}
		v[p] = x;
		it[p] = j;
	}
	const double qnan = __longlong_as_double(0x7ff8000000000000ll);
	for (int r = 0; r < N; ++r) {
		a.out_items[(size_t) u * N + r] = r < n ? it[r] : -1;
		a.out_scores[(size_t) u * N + r] = r < n ? v[r] : qnan;
	}
	return true;
}

// ------------------------------------------------------------------------------------------------
// Matrix-core pass.  The operand path, masks and cheap reject of recommend_mfma2_kernel (L in registers, a ring of three
// R chunks by LDS-DMA, fragment reads one k-step ahead); what differs is the bookkeeping behind the reject.  Per row and
// item half (wc) the N+1 best approximate scores with their items live in LDS, sorted descending (the dynamic LDS behind
// the ring: 64 users x 2 halves x (N+1) x 12 B); the lane keeps the (N+1)-th of each of its rows as the reject threshold
// thr[x] -- the same 32 compares per tile as the top-1 kernel, against a lower bar.  A row with survivors walks its
// candidate lanes (the lowest first, all four lane groups of the wave at once) and inserts each score that still beats the
// bar, the 16 lanes of the group shifting the list in one step.  After the last tile the two halves are merged, then
// certified and re-scored (topn_finish) -- or, under an item split, written to the user's part slot for topn_merge_kernel.
// This kernel does NOT use RRing of mf_ring.hip.h: with the ring's state in that struct hipcc addressed the lists below with
// other instructions in all 14 instances and took two more VGPRs in the eight-wave ones (profiles/certified_parts).  Its
// ring text is a copy of RRing's: a change to either is a change to both.
// ------------------------------------------------------------------------------------------------
constexpr size_t topn_list_lds(int n) { return (size_t) kHU * 2 * (size_t) (n + 1) * (sizeof(double) + sizeof(int)); }

template <int NC, int QC = 5, int TU = 2, int WAVES = 4>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) topn_mfma_kernel(TopnArgs a)
{
	static_assert(NC > 0 && 16 * TU * (WAVES / 2) == kHU && (2 * QC) % (WAVES / 2) == 0 && (2 * QC) / (WAVES / 2) <= 5, "shape");
	constexpr int kHThreads = 64 * WAVES, kHKC = 4 * QC, kHPC = 2 * QC, kHQ = QC, kHChunkD2 = kHPC * kMI;
	constexpr int NCH = NC, KSTEPS = NCH * kHQ;
	extern __shared__ double2 rec_lds[];   // ring of kHNB R chunks: [k-pair][128 items], then the lists
	const int K = a.K;
	const int M = a.n + 1;
	// lists: [user][half][M] scores, then the same of items
	double *const lst_v = reinterpret_cast<double *>(rec_lds + kHNB * kHChunkD2);
	int *const lst_i = reinterpret_cast<int *>(lst_v + kHU * 2 * M);
	__shared__ unsigned long long maskw[2][kHU][2];   // [tile parity][user][item half]
	__shared__ int red_bad[kHU][2];
	__shared__ unsigned long long lmax_bits;

	const int tid = threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int wr = wave >> 1, wc = wave & 1;
	const int lr = lane & 15, lq = lane >> 4;
	const int i0 = blockIdx.x * kHU;
	const double ninf = -__builtin_inf();

	int cur = 0, cend = 0, nextcol = INT32_MAX, nextcol2 = INT32_MAX;
	if (tid < kHU && i0 + tid < a.users) {
		cur = a.csr_ptr[i0 + tid];
		cend = a.csr_ptr[i0 + tid + 1];
		nextcol = cur < cend ? a.csr_idx[cur] : INT32_MAX;
		nextcol2 = cur + 1 < cend ? a.csr_idx[cur + 1] : INT32_MAX;
	}
	double thr[4 * TU];   // (N+1)-th best of each of the lane's rows and this wave's item half
#pragma unroll
	for (int x = 0; x < 4 * TU; ++x) thr[x] = ninf;
	for (int sl = tid; sl < kHU * 2 * M; sl += kHThreads) {
		lst_v[sl] = ninf;
		lst_i[sl] = -1;
	}
	if (tid < kHU) {
		red_bad[tid][0] = red_bad[tid][1] = 0;
		const unsigned long long b = wave_max_bits(i0 + tid < a.users ? (unsigned long long) __double_as_longlong(a.lnorm[i0 + tid]) : 0ull);
		if (lane == 0) lmax_bits = b;
	}
	for (int sl = tid; sl < kHNB * kHChunkD2; sl += kHThreads) rec_lds[sl] = make_double2(0.0, 0.0);
	double fa[KSTEPS][TU];
#pragma unroll
	for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
		for (int tu = 0; tu < TU; ++tu) {
			const int row = i0 + 16 * TU * wr + 16 * tu + lr, k = 4 * ks + lq;
			fa[ks][tu] = row < a.users && k < K ? a.L[(size_t) row * a.ldl + k] : 0.0;
		}
	__syncthreads();

	const unsigned bs_lds = (unsigned) (unsigned long long) (__attribute__((address_space(3))) char *) rec_lds;
	unsigned voff = 0;
	auto set_rows = [&](int jt) {
		const int item = ((lane >> 4) & 1) * 64 + (2 * wc + (lane >> 5)) * 16 + (lane & 15);
		const int row = min(jt + item, a.items - 1);
		voff = (unsigned) row * (unsigned) (a.ldr * 8);   // the host admits R below 4 GB only
	};
	auto dma_chunk = [&](int kc, int slot) -> int {
		int n = 0;
#pragma unroll
		for (int h = 0; h < kHPC / (WAVES / 2); ++h) {
			const int pr = wr + (WAVES / 2) * h, k = kc + 2 * pr;
			if (k < K) {   // wave-uniform
				const char *sbase = reinterpret_cast<const char *>(a.R + k);
				const unsigned m0 = bs_lds + (unsigned) ((slot * kHChunkD2 + pr * kMI + 64 * wc) * 16);
				asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(m0));
				++n;
			}
		}
		return n;
	};
	auto wait_vm = [&](int n) {
		switch (n) {
		case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
		case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
		case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
		case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
		case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
		default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
		}
	};

	const int j_first = a.split_items ? (int) blockIdx.y * a.split_items : 0;
	const int j_end = a.split_items ? min(a.items, j_first + a.split_items) : a.items;
	int pj = j_first, pk = 0, pslot = 0;
	auto issue_next = [&]() -> int {
		if (pj >= j_end) return 0;
		if (pk == 0) set_rows(pj);
		const int n = dma_chunk(pk, pslot);
		pk += kHKC;
		if (pk >= K) {
			pk = 0;
			pj += kMI;
		}
		pslot = pslot == kHNB - 1 ? 0 : pslot + 1;
		return n;
	};
	issue_next();
	wait_vm(issue_next());
	__syncthreads();
	const bool all_finite = all_scores_finite(lmax_bits, a.rnorm_max_bits);
	const int boff = (lq >> 1) * (kMI * 2) + wc * 32 + lr * 2 + (lq & 1);
	auto frag = [&](int s, int q, double (&f)[4]) {
		const double *Bb = reinterpret_cast<const double *>(rec_lds) + s * (kHChunkD2 * 2) + boff;
#pragma unroll
		for (int ti = 0; ti < 4; ++ti) f[ti] = Bb[(8 * q + ti) * 64];
	};
	double fc[4];
	frag(0, 0, fc);
	int slot = 0, pending = 0;
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

#pragma unroll
		for (int c = 0; c < NCH; ++c) {
			const int nslot = slot == kHNB - 1 ? 0 : slot + 1;
#pragma unroll
			for (int q = 0; q < kHQ; ++q) {
				double fn[4];
				if (q == kHQ - 1) {
					wait_vm(pending);
					pending = 0;
					__syncthreads();
					frag(nslot, 0, fn);
				} else {
					frag(slot, q + 1, fn);
				}
				__builtin_amdgcn_sched_barrier(0);
#pragma unroll
				for (int tu = 0; tu < TU; ++tu)
#pragma unroll
					for (int ti = 0; ti < 4; ++ti)
						acc[tu][ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[c * kHQ + q][tu], fc[ti],
						                                                   c + q == 0 ? mf_d4{0.0, 0.0, 0.0, 0.0} : acc[tu][ti], 0, 0, 0);
				if (q == 0) {
					const int n = issue_next();
					if (q != kHQ - 1) pending = n;
				}
#pragma unroll
				for (int ti = 0; ti < 4; ++ti) fc[ti] = fn[ti];
			}
			slot = nslot;
		}

		// cheap reject against the (N+1)-th best of the row half (recommend_mfma2_kernel's 32 compares)
		constexpr int kUGT = 10;   // llvm::FCmpInst::FCMP_UGT: unordered or greater than
		unsigned long long rowm[4 * TU];
		unsigned long long anym = 0;
#pragma unroll
		for (int tu = 0; tu < TU; ++tu)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int x = tu * 4 + r;
				rowm[x] = __builtin_amdgcn_fcmp(acc[tu][0][r], thr[x], kUGT) | __builtin_amdgcn_fcmp(acc[tu][1][r], thr[x], kUGT) |
				          __builtin_amdgcn_fcmp(acc[tu][2][r], thr[x], kUGT) | __builtin_amdgcn_fcmp(acc[tu][3][r], thr[x], kUGT);
				anym |= rowm[x];
			}
		if (!all_finite) {
#pragma unroll
			for (int tu = 0; tu < TU; ++tu)
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const double sum = (acc[tu][0][r] + acc[tu][1][r]) + (acc[tu][2][r] + acc[tu][3][r]);
					rowm[tu * 4 + r] |= __builtin_amdgcn_fcmp(fabs(sum), 1.7976931348623157e308, kUGT);
					anym |= rowm[tu * 4 + r];
				}
		}
		if (anym != 0)
#pragma unroll
		for (int tu = 0; tu < TU; ++tu)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int x = tu * 4 + r;
				if (rowm[x] != 0) {
					// slow path: this lane's survivors among its four scores of the row (open, finite, above the bar)
					const int row = 16 * TU * wr + 16 * tu + lq + 4 * r;
					const unsigned long long m = maskw[par][row][wc] >> lr;
					double *const lv = lst_v + (row * 2 + wc) * M;
					int *const li = lst_i + (row * 2 + wc) * M;
					double t = thr[x];
					int bd = 0;
					unsigned cm = 0;
#pragma unroll
					for (int ti = 0; ti < 4; ++ti) {
						const double v = acc[tu][ti][r];
						const bool open = !((m >> (16 * ti)) & 1ull);
						const bool fin = fabs(v) <= 1.7976931348623157e308;
						bd |= open && !fin;
						cm |= (open && fin && v > t) ? 1u << ti : 0u;
					}
#pragma unroll
					for (int d = 1; d < 16; d <<= 1) bd |= __shfl_xor(bd, d, 16);
					if (lr == 0 && bd) red_bad[row][wc] = 1;
					// candidate lanes, the lowest of each lane group per round (all four groups of the wave at once)
					unsigned long long left = __ballot(cm != 0);
					while (left) {
						unsigned long long low = 0;
#pragma unroll
						for (int g = 0; g < 4; ++g) {
							const unsigned long long w = (left >> (16 * g)) & 0xffffull;
							low |= (w & (~w + 1)) << (16 * g);
						}
						left &= ~low;
						const unsigned long long gw = (low >> (lane & 48)) & 0xffffull;
						const int src = gw ? (lane & 48) + __builtin_ctzll(gw) : lane;
						const unsigned cd = __shfl(cm, src);
						if (gw) {
#pragma unroll
							for (int ti = 0; ti < 4; ++ti) {
								const double v = __shfl(acc[tu][ti][r], src);
								if (((cd >> ti) & 1u) && v > t) {   // group-uniform: the 16 lanes insert together
									// lane lr holds slots lr, lr + 16, lr + 32: every entry below v moves down one slot, v lands
									// in the first of them (all reads before any write: one wave, LDS in program order)
									double w[3];
									int wi[3];
#pragma unroll
									for (int sl = 0; sl < 3; ++sl) {
										const int e = lr + 16 * sl;
										w[sl] = e < M ? lv[e] : 0.0;
										wi[sl] = e < M ? li[e] : -1;
									}
									const unsigned long long b0 = __ballot(lr < M && w[0] < v), b1 = __ballot(lr + 16 < M && w[1] < v),
									                         b2 = __ballot(lr + 32 < M && w[2] < v);
									const unsigned g0 = (unsigned) (b0 >> (lane & 48)) & 0xffffu, g1 = (unsigned) (b1 >> (lane & 48)) & 0xffffu,
									               g2 = (unsigned) (b2 >> (lane & 48)) & 0xffffu;
									const int pos = g0 ? __builtin_ctz(g0) : g1 ? 16 + __builtin_ctz(g1) : 32 + __builtin_ctz(g2);
#pragma unroll
									for (int sl = 0; sl < 3; ++sl) {
										const int e = lr + 16 * sl;
										if (e < M && w[sl] < v && e + 1 < M) {
											lv[e + 1] = w[sl];
											li[e + 1] = wi[sl];
										}
										if (e == pos) {
											lv[e] = v;
											li[e] = j0 + 64 * wc + 16 * ti + (src & 15);
										}
									}
									t = lv[M - 1];
								}
							}
						}
					}
					thr[x] = __shfl(t, lane & ~15);
				}
			}
	}

	// merge the two item halves of every user into the (now idle) ring, then certify or hand over to the merge
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	double *const mv = reinterpret_cast<double *>(rec_lds);
	int *const mi = reinterpret_cast<int *>(mv + kHU * M);
	if (tid < kHU && i0 + tid < a.users) {
		const int u = i0 + tid;
		double *const ov = mv + tid * M;
		int *const oi = mi + tid * M;
		topn_merge_lists(lst_v + tid * 2 * M, lst_i + tid * 2 * M, lst_v + (tid * 2 + 1) * M, lst_i + (tid * 2 + 1) * M, M, ov, oi);
		const int bd = red_bad[tid][0] | red_bad[tid][1];
		if (a.split_items) {
			const size_t base = ((size_t) u * (a.nsplit + 1) + blockIdx.y) * M;
			for (int r = 0; r < M; ++r) {
				a.part_v[base + r] = ov[r];
				a.part_i[base + r] = oi[r];
			}
			a.part_bad[(size_t) u * a.nsplit + blockIdx.y] = bd;
		} else {
			const double rmax = __longlong_as_double((long long) *a.rnorm_max_bits);
			if (!topn_finish(a, u, ov, oi, bd, rmax)) a.olist[atomicAdd(a.ocount, 1)] = u;
		}
	}
}

// Item split of a small problem: the nsplit top-(N+1) lists of a user merged in item order, then certified as above.
__global__ void __launch_bounds__(256) topn_merge_kernel(TopnArgs a)
{
	const int u = blockIdx.x * 256 + threadIdx.x;
	if (u >= a.users) return;
	const int M = a.n + 1;
	double *const v = a.part_v + (size_t) u * (a.nsplit + 1) * M;
	int *const it = a.part_i + (size_t) u * (a.nsplit + 1) * M;
	double *const tv = v + (size_t) a.nsplit * M;
	int *const ti = it + (size_t) a.nsplit * M;
	int bd = a.part_bad[(size_t) u * a.nsplit];
	for (int s = 1; s < a.nsplit; ++s) {
		topn_merge_lists(v, it, v + (size_t) s * M, it + (size_t) s * M, M, tv, ti);
		for (int r = 0; r < M; ++r) {
			v[r] = tv[r];
			it[r] = ti[r];
		}
		bd |= a.part_bad[(size_t) u * a.nsplit + s];
	}
	const double rmax = __longlong_as_double((long long) *a.rnorm_max_bits);
	if (!topn_finish(a, u, v, it, bd, rmax)) a.olist[atomicAdd(a.ocount, 1)] = u;
}

// ------------------------------------------------------------------------------------------------
// Exact pass: one wave per user (the listed ones, or all).  Lane l scores item j0 + l exactly (topn_exact_score) over
// the unrated items, and the wave keeps two short lists in LDS: the N best non-NaN scores by (score descending, index
// ascending) and the first N+1 unrated items with their scores.  They decide the repeated rule: after r picks the first
// remaining item is among the first r+1 unrated ones; when its score is NaN it is the pick, otherwise the best remaining
// non-NaN score is (all non-NaN picks come from the best list in its order).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) topn_exact_kernel(TopnArgs a)
{
	__shared__ double dv[kTopnMax];
	__shared__ int di[kTopnMax];
	__shared__ double fv[kTopnMax + 1];
	__shared__ int fi[kTopnMax + 1];
	const int lane = threadIdx.x;
	const int u = a.ulist ? a.ulist[blockIdx.x] : (int) blockIdx.x;
	const int N = a.n;
	const double *l = a.L + (size_t) u * a.ldl;
	int cur = a.csr_ptr[u];
	const int cend = a.csr_ptr[u + 1];
	int nd = 0, nf = 0;   // entries of the two lists (wave-uniform)
	for (int j0 = 0; j0 < a.items; j0 += 64) {
		unsigned long long m = 0;   // rated items of this batch (every lane walks the same cursor)
		while (cur < cend) {
			const int c = a.csr_idx[cur];
			if (c >= j0 + 64) break;
			if (c >= j0) m |= 1ull << (c - j0);
			++cur;
		}
		const int j = j0 + lane;
		const bool open = j < a.items && !((m >> lane) & 1ull);
		const double s = open ? topn_exact_score(l, a.R + (size_t) j * a.ldr, a.K) : 0.0;
		const unsigned long long ob = __ballot(open);
		if (nf <= N) {
			const int pos = nf + __popcll(ob & ((1ull << lane) - 1ull));
			if (open && pos <= N) {
				fv[pos] = s;
				fi[pos] = j;
			}
			nf = min(N + 1, nf + __popcll(ob));
		}
		const double tv = nd == N ? dv[N - 1] : 0.0;
		const int tj = nd == N ? di[N - 1] : 0;
		unsigned long long cb = __ballot(open && s == s && (nd < N || s > tv || (s == tv && j < tj)));
		while (cb) {
			const int src = __builtin_ctzll(cb);
			cb &= cb - 1;
			const double v = __shfl(s, src);
			const int jj = j0 + src;
			if (lane == 0 && (nd < N || v > dv[N - 1] || (v == dv[N - 1] && jj < di[N - 1]))) {
				int p = nd < N ? nd : N - 1;
				while (p > 0 && (dv[p - 1] < v || (dv[p - 1] == v && di[p - 1] > jj))) {
					dv[p] = dv[p - 1];
					di[p] = di[p - 1];
					--p;
				}
				dv[p] = v;
				di[p] = jj;
				nd += nd < N;
			}
			nd = __shfl(nd, 0);
		}
		__syncthreads();   // the lists are read by every lane of the next batch
	}
	if (lane == 0) {
		const double qnan = __longlong_as_double(0x7ff8000000000000ll);
		unsigned long long picked = 0;
		const unsigned long long inlist = nf == 64 ? ~0ull : (1ull << nf) - 1ull;
		int d = 0;
		for (int r = 0; r < N; ++r) {
			const unsigned long long rest = inlist & ~picked;
			int t = -1;
			double sc = qnan;
			if (rest) {
				const int q = __builtin_ctzll(rest);
				if (fv[q] != fv[q]) {
					t = fi[q];
					sc = fv[q];
					picked |= 1ull << q;
				} else {   // d < nd: the first remaining item is a non-NaN one not picked yet
					t = di[d];
					sc = dv[d];
					++d;
					for (int x = 0; x < nf; ++x)
						if (fi[x] == t) picked |= 1ull << x;
				}
			}
			a.out_items[(size_t) u * N + r] = t;
			a.out_scores[(size_t) u * N + r] = sc;
		}
	}
}

}  // namespace mf
