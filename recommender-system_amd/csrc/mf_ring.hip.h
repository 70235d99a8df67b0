// mf_ring.hip.h -- what the certified matrix-core passes share (recommend_mfma_kernel, recommend_mfma2_kernel,
// topn_mfma_kernel, rank_mfma_kernel), each stated once: the geometry, the ring of R chunks filled by LDS-DMA with the
// tile's matrix stream (RRing), the norm prologue, the cheap reject, and the top-2 merge and certification of the top-1
// passes.  Every piece is __forceinline__, and still a piece is not always the code its text would be written out: hipcc
// allocates registers and places waits differently around some of them, so a kernel uses a piece only where its code
// object stayed that of the written-out text (tools/isa.py --compare; profiles/certified_parts/README.md says which).
#pragma once
#include "mf_common.hip.h"
#include "../../include/matfact_hip.h"   // mf_filter

namespace mf {

// ---- Geometry.  A workgroup owns kHU rows (users, or held-out entries) and walks the items in tiles of kMI; LDS holds a
// ring of kHNB chunks of R.
constexpr int kHU = 64, kHNB = 3, kHKmax = 100, kMI = 128;
// dynamic LDS: the ring of kHNB chunks of QC k-steps (2 QC k-pairs x 128 items x 16 B each)
inline size_t rec_mfma2_lds(int qc) { return (size_t) kHNB * (2 * qc) * kMI * sizeof(double2); }

typedef double mf_d4 __attribute__((ext_vector_type(4)));

// ---- Top-2 of a row: b1 = -inf / i1 = -1 encode "no candidate"; all values are finite or -inf, so plain comparisons suffice
struct Top2 {
	double b1, b2;
	int i1;
};

__device__ __forceinline__ void top2_merge(Top2 &a, const Top2 &b)
{
	const bool take = b.b1 > a.b1;
	const double lo1 = take ? a.b1 : b.b1;          // the smaller of the two bests
	const double hi2 = take ? b.b2 : a.b2;          // the winner's own runner-up
	a.b2 = lo1 > hi2 ? lo1 : hi2;
	a.b1 = take ? b.b1 : a.b1;
	a.i1 = take ? b.i1 : a.i1;
}

// ---- Prologue pieces.
// the largest of a wave's bit patterns (norms as bits: a NaN is the largest value)
__device__ __forceinline__ unsigned long long wave_max_bits(unsigned long long b)
{
	for (int d = 32; d >= 1; d >>= 1) {
		const unsigned long long o = __shfl_xor(b, d);
		b = o > b ? o : b;
	}
	return b;
}

__device__ __forceinline__ double rnorm_max(const unsigned long long *__restrict__ rnorm_max_bits)
{
	return __longlong_as_double((long long) *rnorm_max_bits);
}

// Can a score of this workgroup be non-finite at all?  |score| <= ||L[i]|| * ||R[j]|| (Cauchy-Schwarz): when the largest
// of its row norms times the largest item norm is a finite number well below the overflow threshold, every partial sum of
// every score is finite and the epilogue needs no NaN / inf screening.  A NaN or inf anywhere in the rows involved makes a
// norm NaN or inf (compared as bit patterns, a NaN is the largest value).
__device__ __forceinline__ bool all_scores_finite(unsigned long long lmax_bits, const unsigned long long *__restrict__ rnorm_max_bits)
{
	const double bound = __longlong_as_double((long long) lmax_bits) * rnorm_max(rnorm_max_bits);
	return bound <= 1e300;   // false for NaN
}

// the certification margin of a row with norm ln (recommend_mfma_kernel's header: thr_i)
__device__ __forceinline__ double cert_margin(double thr_scale, double ln, double rmax) { return thr_scale * (ln * rmax) + 1e-300; }

// ---- Cheap reject: after the first tiles almost no score beats its row's bar thr[x] (row x = 4*tu + r of the lane).  Every
// vector instruction of this step costs matrix-pipe time (nothing else of the SIMD runs while an FP64 matrix instruction
// executes, and vice versa), so the common case is ONE compare per score register, masks not even looked at -- 32 v_cmp
// whose lane masks land in scalar registers and are OR-ed there -- and one scalar branch on the result; fmax() would add a
// canonicalising v_max per operand and a ballot two more vector instructions per row.  !(v <= thr) is also true for a NaN.
// Only when the norms do not rule out non-finite scores (all_finite) a sum per row is formed as well: it is non-finite
// whenever a score is NaN or +-inf (a sum that merely overflows only costs the slow path).
template <int TU>
__device__ __forceinline__ bool cheap_reject(const mf_d4 (&acc)[TU][4], const double (&thr)[4 * TU], bool all_finite,
                                             unsigned long long (&rowm)[4 * TU])
{
	constexpr int kUGT = 10;   // llvm::FCmpInst::FCMP_UGT: unordered or greater than
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
	return anym != 0;
}

// ---- Top-1 bookkeeping.
// The certification of user u from its top-2 over all items and the non-finite flag: the arg-max, or -2 and a place on the
// list of the exact pass.  (The reports to `part` / `filt` stay with the kernels: as part of this function they moved
// registers in recommend_mfma_kernel.)
template <class Args>
__device__ __forceinline__ void top1_certify(const Args &a, int u, const Top2 &t, int bd)
{
	const double thr = cert_margin(a.thr_scale, a.lnorm[u], rnorm_max(a.rnorm_max_bits));
	const bool certain = !bd && (t.i1 < 0 || (t.b1 - t.b2) > thr);
	if (certain) {
		a.best[u] = t.i1;
	} else {
		a.best[u] = -2;
		a.ulist[atomicAdd(a.ucount, 1)] = u;
	}
}

// ---- The R ring and the matrix stream of a tile, for a workgroup of WAVES waves as (WAVES / 2 row groups) x (2 item halves
// of 64), each wave with TU 16-row tiles against its 64 items.  LDS holds a ring of kHNB chunks of QC k-steps, [k-pair][128
// items] of 16 B, written only by LDS-DMA (1 KB contiguous per instruction, no padding rows; the fragment read of 32 lanes
// is 256 contiguous bytes); the wave's L operand lives in registers.  The transfer of chunk s+2 is issued under the matrix
// instructions of chunk s -- a chunk has two chunk times to land.
// NC > 0: K == 4 QC NC exactly -- every chunk whole, no branch of the tile body depends on K (hipcc's s_waitcnt placement
// follows the fragment pipeline only through straight-line code); NC == 0: any even K <= kHKmax.
template <int NC, int QC, int TU, int WAVES>
struct RRing {
	static_assert(16 * TU * (WAVES / 2) == kHU && (2 * QC) % (WAVES / 2) == 0 && (2 * QC) / (WAVES / 2) <= 5, "shape");
	static_assert(NC > 0 || (QC == 5 && TU == 2 && WAVES == 4), "the general form exists for the 20-deep chunks only");
	static constexpr int kThreads = 64 * WAVES, kKC = 4 * QC, kPC = 2 * QC, kChunkD2 = kPC * kMI;
	static constexpr int NCH = NC ? NC : kHKmax / kKC, KSTEPS = NCH * QC;

	double2 *const lds;            // the ring
	const double *__restrict__ const R;
	const int K, items, ldr;       // the host admits R below 4 GB only
	const int j_end;               // the tiles end here (the split's end)
	const int lane, wr, wc;
	const unsigned bs_lds;
	unsigned voff = 0;             // byte offset of the lane's row of the tile being transferred
	int pj, pk = 0, pslot = 0;     // the chunk sequence: tiles in ascending order, k-chunks within; the next chunk to transfer
	int boff = 0, slot = 0;
	int pending = 0;               // this wave's transfers issued AFTER those of the chunk the next barrier publishes
	double fc[4];                  // the R fragment of the next k-step: prime() reads the first, tile() hands it on

	template <class Args>
	__device__ __forceinline__ RRing(double2 *ring, const Args &a, int j_first, int j_end_, int lane_, int wave)
	    : lds(ring), R(a.R), K(a.K), items(a.items), ldr(a.ldr), j_end(j_end_), lane(lane_), wr(wave >> 1), wc(wave & 1),
	      bs_lds(lds_address(reinterpret_cast<const char *>(ring))), pj(j_first)
	{
	}

	// pairs beyond K are never transferred: the ring holds zeros there at first, not NaN patterns
	__device__ __forceinline__ static void clear(double2 *ring, int tid)
	{
		for (int sl = tid; sl < kHNB * kChunkD2; sl += kThreads) ring[sl] = make_double2(0.0, 0.0);
	}
	__device__ __forceinline__ void set_rows(int jt)
	{
		// lane i of a transfer lands at byte 16 i of window w = wc of its k-pair's row: the item the chunk image keeps there
		const int item = ((lane >> 4) & 1) * 64 + (2 * wc + (lane >> 5)) * 16 + (lane & 15);
		const int row = min(jt + item, items - 1);    // rows beyond the matrix are masked
		voff = (unsigned) row * (unsigned) (ldr * 8);
	}
	// LDS-DMA of one R chunk (k offset kc of the tile `voff` points into) into ring slot `s`: 4 QC instructions of 64 rows x
	// 16 B, up to five per wave (k-pair wr + (WAVES / 2) h, rows 64*wc..+63).  Scalar base + per-lane row offset: no vector
	// arithmetic per transfer -- every VALU instruction of a wave waits for the matrix pipe of its SIMD to drain
	// (tools/micro/valu_under_mfma.hip).  Returns how many this wave issued (pairs beyond K: none).
	__device__ __forceinline__ int dma_chunk(int kc, int s)
	{
		int n = 0;
#pragma unroll
		for (int h = 0; h < kPC / (WAVES / 2); ++h) {
			const int pr = wr + (WAVES / 2) * h, k = kc + 2 * pr;
			if (k < K) {   // wave-uniform
				const char *sbase = reinterpret_cast<const char *>(R + k);
				const unsigned m0 = bs_lds + (unsigned) ((s * kChunkD2 + pr * kMI + 64 * wc) * 16);
				asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(m0));
				++n;
			}
		}
		return n;
	}
	// at most n of this wave's transfers still in flight (hipcc does not count the asm transfers)
	__device__ __forceinline__ static void wait_vm(int n)
	{
		switch (n) {
		case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
		case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
		case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
		case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
		case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
		default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
		}
	}
	__device__ __forceinline__ int issue_next()
	{
		if (pj >= j_end) return 0;
		if (pk == 0) set_rows(pj);
		const int n = dma_chunk(pk, pslot);
		pk += kKC;
		if (pk >= K) {
			pk = 0;
			pj += kMI;
		}
		pslot = pslot == kHNB - 1 ? 0 : pslot + 1;
		return n;
	}
	// R fragment of k-step q of the chunk in ring slot s: k = 4q + lq -> pair 2q + (lq >> 1), half lq & 1.  Within the 2 KB
	// row of a k-pair, item 64 wc + 16 ti + lr sits at byte 512 ti + 256 wc + 16 lr: a wave's four fragments of a k-step are
	// 512 B apart, the k-steps 4 KB, the slots 4 QC KB -- all multiples of 512, so every fragment read of a chunk is one base
	// register plus an immediate (ds_read2st64_b64) and the k-loop holds no vector arithmetic at all.
	__device__ __forceinline__ void frag(int s, int q, double (&f)[4]) const
	{
		const double *Bb = reinterpret_cast<const double *>(lds) + s * (kChunkD2 * 2) + boff;
#pragma unroll
		for (int ti = 0; ti < 4; ++ti) f[ti] = Bb[(8 * q + ti) * 64];
	}
	// The primed start.  Precondition: the barrier behind clear() has been passed and the caller has issued chunk 0 with
	// ONE issue_next() (with both issues in here hipcc lays the prologue's transfers out behind the tile loop).  Issues
	// chunk 1, waits until chunk 0 has landed for every wave and reads its first fragment into fc.
	__device__ __forceinline__ void prime()
	{
		wait_vm(issue_next());   // chunk 0 has landed; chunk 1 may still be in flight
		__syncthreads();
		const int lr = lane & 15, lq = lane >> 4;
		boff = (lq >> 1) * (kMI * 2) + wc * 32 + lr * 2 + (lq & 1);
		frag(0, 0, fc);
	}
	// The matrix stream of a tile: acc = (the wave's rows of L, in fa) x (its 64 items of the next tile of R)^T.
	// Called by rank_mfma_kernel only.  recommend_mfma2_kernel runs a COPY of this loop over the members (wait_vm, frag,
	// issue_next, slot, pending) with the fragment in registers of its own, and topn_mfma_kernel a copy over its own ring
	// text: as this call both came out with other registers and waits.  A CHANGE HERE IS A CHANGE TO ALL THREE.
	// The stream of a wave has no gap of its own: the fragment of the NEXT k-step -- of this chunk, of the next chunk, of
	// the next tile -- is read in front of the matrix instructions of the current one.  For that the barrier that publishes
	// chunk s+1 stands in front of the LAST k-step of chunk s (whose transfer, issued under the first k-step of chunk s-1,
	// has had almost two chunk times), and the transfer of chunk s+2 goes into the slot of chunk s-1 -- whose last fragment
	// every wave had read before it passed that barrier one chunk ago.
	__device__ __forceinline__ void tile(const double (&fa)[KSTEPS][TU], mf_d4 (&acc)[TU][4])
	{
#pragma unroll
		for (int c = 0; c < NCH; ++c) {
			const int kc = c * kKC;
			if (NC || kc < K) {   // wave-uniform
				const int nq = NC ? QC : min(QC, (K - kc + 3) >> 2);   // k-steps of this chunk (only the last chunk can be short)
				const int nslot = slot == kHNB - 1 ? 0 : slot + 1;
#pragma unroll
				for (int q = 0; q < QC; ++q) {
					if (NC || q < nq) {   // wave-uniform
						const bool last = NC ? q == QC - 1 : q == nq - 1;
						double fn[4];
						if (last) {
							wait_vm(pending);   // chunk s+1 has landed ...
							pending = 0;
							__syncthreads();    // ... for every wave
							frag(nslot, 0, fn);
						} else {
							frag(slot, q + 1, fn);
						}
						// the reads stay in front of the matrix instructions (the scheduler would sink them behind the last
						// use of the current fragment's registers to save eight VGPRs -- and expose the LDS latency per k-step)
						__builtin_amdgcn_sched_barrier(0);
#pragma unroll
						for (int tu = 0; tu < TU; ++tu)
#pragma unroll
							for (int ti = 0; ti < 4; ++ti)
								acc[tu][ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[c * QC + q][tu], fc[ti],
								                                                   c + q == 0 ? mf_d4{0.0, 0.0, 0.0, 0.0} : acc[tu][ti], 0, 0, 0);
						if (q == 0) {   // chunk s+2 under the matrix instructions just issued
							const int n = issue_next();
							if (!last) pending = n;
						}
#pragma unroll
						for (int ti = 0; ti < 4; ++ti) fc[ti] = fn[ti];
					}
				}
				slot = nslot;
			}
		}
	}
};

}  // namespace mf
