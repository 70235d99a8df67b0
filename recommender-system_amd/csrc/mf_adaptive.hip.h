// mf_adaptive.hip.h -- per-element adaptive step sizes (AdaGrad, RMSProp, Adam) behind every sweep form.
//
// A seeded sweep of an adaptive side is the side's UNSEEDED sweep -- X_new = g = 0.0 + sum e_n * y_n in the side's entry
// order, the bits every sweep form already produces -- followed by the finishing kernel of this file, which turns g into
// the new row from X_old and the side's accumulators (include/matfact_hip.h has the definition, operation by operation).
// The correctly rounded division and square root of the step expand into fused multiply-adds on gfx950, so they live here
// and never inside a sweep kernel: those stay free of any FP64 fma.  Everything else of the formula is one rounded
// operation per line (the library is built with -ffp-contract=off; a contracted v + g * g is a wrong bit).
#pragma once
#include "mf_common.hip.h"
#include "mf_sweep.hip.h"

namespace mf {

// The per-side record of the step scalars on the device.  Launch arguments are frozen in a captured graph, so what
// changes from step to step is read from here: adaptive_tick_kernel advances it in front of the side's finish.
struct AdaptiveStep {
	double p1, p2;     // beta1^t and beta2^t as sequential products from 1.0 (ADAM; 1.0 for the other kinds)
	double c1, c2;     // 1.0 - p1 and 1.0 - p2 of the step in flight
	long long steps;   // seeded adaptive sweeps of the side since rest
};

// puts the record where the caller says: at rest (1.0, 1.0, 0) or at an uploaded state
__global__ void adaptive_set_kernel(AdaptiveStep *s, double p1, double p2, long long steps)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		s->p1 = p1;
		s->p2 = p2;
		s->c1 = 1.0 - p1;
		s->c2 = 1.0 - p2;
		s->steps = steps;
	}
}

// one step: p1 = p1 * beta1, p2 = p2 * beta2 (ADAM only), the two bias corrections, the count
__global__ void adaptive_tick_kernel(AdaptiveStep *s, double beta1, double beta2, int adam)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		if (adam) {
			const double p1 = s->p1 * beta1, p2 = s->p2 * beta2;
			s->p1 = p1;
			s->p2 = p2;
			s->c1 = 1.0 - p1;
			s->c2 = 1.0 - p2;
		}
		s->steps = s->steps + 1;
	}
}

constexpr int kAdaptiveRows = 64;       // most rows of a workgroup per step
constexpr int kAdaptiveThreads = 256;

struct AdaptiveArgs {
	int nrows, K, ld, frozen;            // rows of the launch, columns, row pitch of X, m and v in doubles, frozen column or -1
	int rows_per_step;                   // rows a workgroup takes at a time, 1 .. kAdaptiveRows (fewer the wider a row is)
	const int *__restrict__ rowlist;     // optional: the launch covers rows rowlist[0..nrows) instead of 0..nrows
	const double *__restrict__ X_old;
	double *__restrict__ X_new;          // g in, the new row out
	double *__restrict__ m;              // ADAM only
	double *__restrict__ v;
	const AdaptiveStep *__restrict__ step;
	double d;                            // the side's decay, as side_update forms it
	double eta, eps, beta1, beta2, ob1, ob2;   // ob = 1.0 - beta, formed once on the host
	Box box;                             // columns = 0: no projection
};

// one element: every line one rounded operation
template <int KIND>
__device__ __forceinline__ double adaptive_element(const AdaptiveArgs &a, double c1, double c2, double g, double x, double &m, double &v)
{
	const double q = g * g;
	double mh = g, vh;
	if constexpr (KIND == MF_OPT_ADAGRAD) {
		v = v + q;
		vh = v;
	} else {
		const double bv = a.beta2 * v;
		const double oq = a.ob2 * q;
		v = bv + oq;
		vh = v;
	}
	if constexpr (KIND == MF_OPT_ADAM) {
		const double bm = a.beta1 * m;
		const double og = a.ob1 * g;
		m = bm + og;
		mh = m / c1;
		vh = v / c2;
	}
	const double s = sqrt(vh);
	const double den = s + a.eps;
	const double u = mh / den;
	const double step = a.eta * u;
	const double xd = x * a.d;
	return xd + step;
}

// Elementwise over the launch's rows x K: reads g (X_new), x (X_old), v (and m), writes X_new, v (and m) -- 5 streams of 8
// bytes per element, 7 for ADAM, and nothing else: memory-bound.  Rows of an even pitch go as 16-byte pieces with a scalar
// column behind an odd K; rows of an odd pitch element by element.  A workgroup takes rows_per_step rows at a time.
template <int KIND>
__global__ void __launch_bounds__(kAdaptiveThreads) adaptive_finish_kernel(AdaptiveArgs a)
{
	const int P = (a.ld & 1) ? 0 : a.K >> 1;   // 16-byte pieces of a row
	const int per = P + (a.K - 2 * P);         // pieces plus scalar columns
	double c1 = 1.0, c2 = 1.0;
	if constexpr (KIND == MF_OPT_ADAM) {
		c1 = a.step->c1;
		c2 = a.step->c2;
	}
	for (int r0 = blockIdx.x * a.rows_per_step; r0 < a.nrows; r0 += gridDim.x * a.rows_per_step) {
		const int n = min(a.rows_per_step, a.nrows - r0) * per;
		for (int e = threadIdx.x; e < n; e += kAdaptiveThreads) {
			const int i = e / per, j = e - i * per;
			const int r = a.rowlist ? a.rowlist[r0 + i] : r0 + i;
			const size_t row = (size_t) r * a.ld;
			if (j < P) {
				const int k = 2 * j;
				const size_t at = row + k;
				const double2 g = *reinterpret_cast<const double2 *>(a.X_new + at);
				const double2 x = *reinterpret_cast<const double2 *>(a.X_old + at);
				double2 v = *reinterpret_cast<const double2 *>(a.v + at), v0 = v;
				double2 m = make_double2(0.0, 0.0), m0 = m;
				if constexpr (KIND == MF_OPT_ADAM) m0 = m = *reinterpret_cast<const double2 *>(a.m + at);
				double2 y;
				y.x = adaptive_element<KIND>(a, c1, c2, g.x, x.x, m.x, v.x);
				y.y = adaptive_element<KIND>(a, c1, c2, g.y, x.y, m.y, v.y);
				// the box on the bounded columns, then the frozen select: frozen wins, and its m and v keep their bits
				if (k < a.box.columns) y.x = box_clamp(y.x, a.box.lo, a.box.hi);
				if (k + 1 < a.box.columns) y.y = box_clamp(y.y, a.box.lo, a.box.hi);
				if (k == a.frozen) y.x = x.x, v.x = v0.x, m.x = m0.x;
				if (k + 1 == a.frozen) y.y = x.y, v.y = v0.y, m.y = m0.y;
				*reinterpret_cast<double2 *>(a.X_new + at) = y;
				*reinterpret_cast<double2 *>(a.v + at) = v;
				if constexpr (KIND == MF_OPT_ADAM) *reinterpret_cast<double2 *>(a.m + at) = m;
			} else {
				const int k = 2 * P + (j - P);
				const size_t at = row + k;
				const double x = a.X_old[at];
				if (k == a.frozen) {
					a.X_new[at] = x;
					continue;
				}
				double v = a.v[at], m = 0.0;
				if constexpr (KIND == MF_OPT_ADAM) m = a.m[at];
				double y = adaptive_element<KIND>(a, c1, c2, a.X_new[at], x, m, v);
				if (k < a.box.columns) y = box_clamp(y, a.box.lo, a.box.hi);
				a.X_new[at] = y;
				a.v[at] = v;
				if constexpr (KIND == MF_OPT_ADAM) a.m[at] = m;
			}
		}
	}
}

}  // namespace mf
