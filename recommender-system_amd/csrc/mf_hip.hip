// mf_hip.hip -- C ABI (include/matfact_hip.h) of the MI355X backend: plan management, CSR/CSC build,
// kernel dispatch.  HIP only -- there is no CPU compute path in this library.
#include <cstring>
#include <map>
#include <mutex>

#include "../../include/matfact_hip.h"
#include "mf_kernels.hip.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mf_config.hip.h"
#include "mf_device.hip.h"
#include "mf_plan.hip.h"
#include "mf_schedule.h"
#include "mf_launch.hip.h"
#include "mf_build.hip.h"
#include "mf_certified.hip.h"
#include "mf_loss_host.hip.h"

extern "C" {

const char *mf_backend_strerror(int status)
{
	switch (status) {
	case MF_OK: return "ok";
	case MF_ERR_ARGUMENT: return "invalid argument";
	case MF_ERR_NO_DEVICE: return "no usable HIP device";
	case MF_ERR_HIP: return "HIP runtime error";
	case MF_ERR_NO_MEMORY: return "out of memory";
	case MF_ERR_UNSUPPORTED: return "unsupported shape";
	case MF_ERR_STATE: return "plan is not in a state that allows this call";
	default: return "unknown status";
	}
}

const char *mf_backend_last_hip_error(void) { return g_last_hip_error.c_str(); }

int mf_backend_abi_version(void) { return MATFACT_HIP_ABI_VERSION; }

int mf_backend_device_count(void)
{
	int n = 0;
	const hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) {
		g_last_hip_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
		return e == hipErrorNoDevice ? 0 : MF_ERR_NO_DEVICE;
	}
	return n;
}

}   // extern "C"

// One factor's two generations: the caller's buffers at the caller's pitch, or the plan's own at the padded pitch `own`.
// Row pitch of the buffers the plan owns: rows of 8K bytes are gathered in whole 128-byte lines, so when 8K
// is not a multiple of 128 a row costs a line more than its bytes wherever it happens to start (80-byte rows:
// 1.5 lines on average instead of 1; 240-byte rows: 2.75 instead of 2).  The plan pads its own rows to whole
// lines where that saves at least a tenth of the lines; caller-owned buffers keep the caller's pitch K.
static int factor_buffers(mf_plan *p, void *const ext[2], int ext_pitch, int own, int rows, double *buf[2], dev_buf<double> mine[2],
                          int *ld, bool *external)
{
	*external = ext[0] && ext[1];
	*ld = *external ? (ext_pitch ? ext_pitch : p->K) : own;
	for (int g = 0; g < 2; ++g) {
		if (*external) {
			buf[g] = (double *) ext[g];
			continue;
		}
		const size_t n = (size_t) rows * *ld;
		MF_TRY(mine[g].alloc(n));
		buf[g] = mine[g];
		if (*ld != p->K)   // the padding is never read by a kernel, but it is summed by the multi-GPU reducers
			MF_HIP(hipMemsetAsync(buf[g], 0, std::max<size_t>(n, 1) * sizeof(double), p->stream));
	}
	return MF_OK;
}

// everything of a new plan that can fail: the caller destroys the plan when it does
static int plan_fill(mf_plan *p, const mf_shard *s, const mf_entry *aos, bool swap, const double *weight)
{
	MF_TRY(choose_sweep(p));
	MF_TRY(choose_loss(p));
	if (hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) != hipSuccess) return MF_ERR_HIP;
	p->stream = p->own_stream;
	{
		std::vector<int> rptr, cptr;
		MF_TRY(build_sparse(p, s, aos, swap, weight, rptr, cptr));
		MF_TRY(plan_row_schedule(p, rptr, cptr));
		MF_TRY(plan_es_schedule(p, rptr, cptr));
	}
	const int own = row_pitch(p->cfg, p->K, p->sweep.dma != 0);
	MF_TRY(factor_buffers(p, s->users_ext, s->users_pitch, own, p->uc, p->Lbuf, p->Lown, &p->ldl, &p->l_external));
	MF_TRY(factor_buffers(p, s->items_ext, s->items_pitch, own, p->items, p->Rbuf, p->Rown, &p->ldr, &p->r_external));
	MF_TRY(plan_band_tables(p));
	MF_HIP(hipStreamSynchronize(p->stream));   // the plan is complete when the call returns
	MF_TRY(p->best_dev.alloc((size_t) p->uc));
	MF_TRY(p->lnorm.alloc((size_t) p->uc));
	MF_TRY(p->rmax_bits.alloc(1));
	MF_TRY(p->ulist.alloc((size_t) p->uc));
	MF_TRY(p->ucount.alloc(1));
	return MF_OK;
}

// `aos` (optional): the entries as the reference's array of (row, col, value) structs; they are then uploaded as they
// are and split into the three arrays on the device (the level-1 entry points: no host-side copy of 1e8 entries).
// `swap`: read the structs with row and col exchanged (the item-cut form of mf_backend_run_multi).
// `weight` (optional): one confidence weight per entry, in the entries' order; null makes the plan of today in every respect.
static int plan_create_impl(mf_plan **out, const mf_shard *s, const mf_entry *aos, bool swap = false, const double *weight = nullptr)
{
	if (!out) return MF_ERR_ARGUMENT;
	*out = nullptr;
	if (!s || s->users_total < 0 || s->items < 0 || s->features < 1 || s->nnz < 0 || s->user_begin < 0 ||
	    s->user_count < 0 || (int64_t) s->user_begin + s->user_count > s->users_total ||
	    s->nnz > INT32_MAX - 64 || (s->nnz > 0 && !aos && (!s->row || !s->col || !s->val)))
		return MF_ERR_ARGUMENT;
	// caller-owned R buffers: both or neither, and 16-B aligned (the gather moves 16-byte pieces of rows)
	if ((s->items_ext[0] == nullptr) != (s->items_ext[1] == nullptr) || ((uintptr_t) s->items_ext[0] & 15) ||
	    ((uintptr_t) s->items_ext[1] & 15) || (s->items_ext[0] && s->items_ext[0] == s->items_ext[1]))
		return MF_ERR_ARGUMENT;
	if ((s->users_ext[0] == nullptr) != (s->users_ext[1] == nullptr) || ((uintptr_t) s->users_ext[0] & 15) ||
	    ((uintptr_t) s->users_ext[1] & 15) || (s->users_ext[0] && s->users_ext[0] == s->users_ext[1]))
		return MF_ERR_ARGUMENT;
	// declared pitch of caller-owned buffers: even (16-byte aligned rows) and at least K
	if (s->items_pitch < 0 || s->users_pitch < 0 || (s->items_pitch && (s->items_pitch < s->features || (s->items_pitch & 1))) ||
	    (s->users_pitch && (s->users_pitch < s->features || (s->users_pitch & 1))))
		return MF_ERR_ARGUMENT;
	const int ndev = mf_backend_device_count();
	if (ndev <= 0 || s->device < 0 || s->device >= ndev) return MF_ERR_NO_DEVICE;
	MF_HIP(hipSetDevice(s->device));

	mf_plan *p = new (std::nothrow) mf_plan();
	if (!p) return MF_ERR_NO_MEMORY;
	p->device = s->device;
	p->users_total = s->users_total;
	p->items = s->items;
	p->K = s->features;
	p->u0 = s->user_begin;
	p->uc = s->user_count;
	p->side[0].nrows = p->items;
	p->side[1].nrows = p->uc;
	p->nnz = s->nnz;
	p->alpha = s->alpha;
	p->flags = s->flags;
	p->cfg = mf_config::from_env();
	p->weighted = weight != nullptr;   // in front of choose_sweep: it picks the launch limits of the weighted twins
	const int rc = plan_fill(p, s, aos, swap, weight);
	if (rc != MF_OK) {
		mf_plan_destroy(p);
		return rc;
	}
	*out = p;
	return MF_OK;
}

// a shard that is the whole problem: every user, no caller-owned buffers
static mf_shard whole_shard(int32_t users, int32_t items, int32_t features, int64_t nnz, double alpha, int device)
{
	mf_shard s;
	memset(&s, 0, sizeof s);
	s.users_total = s.user_count = users;
	s.items = items;
	s.features = features;
	s.nnz = nnz;
	s.alpha = alpha;
	s.device = device;
	return s;
}

extern "C" {

int mf_plan_create(mf_plan **out, const mf_shard *s) { return plan_create_impl(out, s, nullptr); }

int mf_plan_create_weighted(mf_plan **out, const mf_shard *s, const double *weight)
{
	return plan_create_impl(out, s, nullptr, false, weight);
}

int mf_plan_weight_total(mf_plan *p, double *sum_w, double *row_w)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (!p->weighted) return MF_ERR_STATE;
	return weight_total_eval(p, sum_w, row_w);
}

int mf_backend_row_pitch(int features)
{
	if (features < 1) return MF_ERR_ARGUMENT;
	const mf_config cfg = mf_config::from_env();
	return row_pitch(cfg, features, sweep_is_dma(cfg, features));   // rows are padded for the LDS-DMA forms only
}

int mf_plan_row_pitch(mf_plan *p, int32_t *users_pitch, int32_t *items_pitch)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (users_pitch) *users_pitch = p->ldl;
	if (items_pitch) *items_pitch = p->ldr;
	return MF_OK;
}

void mf_plan_destroy(mf_plan *p)
{
	if (!p) return;
	(void) hipSetDevice(p->device);
	if (p->stream) (void) hipStreamSynchronize(p->stream);
	for (auto &t : p->timed) {
		if (!t.shared_start) (void) hipEventDestroy(t.t0);
		(void) hipEventDestroy(t.t1);
	}
	if (p->side_stream) (void) hipStreamDestroy(p->side_stream);
	if (p->ev_fork) (void) hipEventDestroy(p->ev_fork);
	if (p->ev_join) (void) hipEventDestroy(p->ev_join);
	if (p->own_stream) (void) hipStreamDestroy(p->own_stream);
	delete p;   // frees the device memory: every buffer is a dev_buf member
}

int mf_plan_set_stream(mf_plan *p, void *hip_stream)
{
	if (!p) return MF_ERR_ARGUMENT;
	MF_HIP(hipSetDevice(p->device));
	MF_HIP(hipStreamSynchronize(p->stream));
	p->stream = hip_stream ? (hipStream_t) hip_stream : p->own_stream;
	return MF_OK;
}

int mf_plan_upload_factors(mf_plan *p, const double *L_block, const double *R)
{
	if (!p || (!L_block && p->uc > 0) || (!R && p->items > 0)) return MF_ERR_ARGUMENT;
	MF_HIP(hipSetDevice(p->device));
	// the caller's rows are K doubles apart, the device rows ldl / ldr
	const size_t w = (size_t) p->K * sizeof(double);
	if (p->uc)
		MF_HIP(hipMemcpy2DAsync(p->Lbuf[p->cur], (size_t) p->ldl * sizeof(double), L_block, w, w, (size_t) p->uc,
		                        hipMemcpyHostToDevice, p->stream));
	if (p->items)
		MF_HIP(hipMemcpy2DAsync(p->Rbuf[p->cur], (size_t) p->ldr * sizeof(double), R, w, w, (size_t) p->items,
		                        hipMemcpyHostToDevice, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	p->have_factors = true;
	p->rule[0].at_rest = p->rule[1].at_rest = true;   // new factors have no history
	p->opt[0].rest = p->opt[1].rest = true;            // and no accumulated gradients
	return MF_OK;
}

int mf_plan_upload_previous(mf_plan *p, const double *L_prev_block, const double *R_prev)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	const size_t w = (size_t) p->K * sizeof(double);
	if (L_prev_block && p->uc)
		MF_HIP(hipMemcpy2DAsync(p->Lbuf[p->cur ^ 1], (size_t) p->ldl * sizeof(double), L_prev_block, w, w, (size_t) p->uc,
		                        hipMemcpyHostToDevice, p->stream));
	if (R_prev && p->items)
		MF_HIP(hipMemcpy2DAsync(p->Rbuf[p->cur ^ 1], (size_t) p->ldr * sizeof(double), R_prev, w, w, (size_t) p->items,
		                        hipMemcpyHostToDevice, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	if (L_prev_block) p->rule[1].at_rest = false;
	if (R_prev) p->rule[0].at_rest = false;
	return MF_OK;
}

int mf_plan_download_previous(mf_plan *p, double *L_prev_block, double *R_prev)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	const size_t w = (size_t) p->K * sizeof(double);
	// a side at rest has no history of its own: X_prev = X_old
	if (L_prev_block && p->uc)
		MF_HIP(hipMemcpy2DAsync(L_prev_block, w, p->Lbuf[p->rule[1].at_rest ? p->cur : p->cur ^ 1], (size_t) p->ldl * sizeof(double), w,
		                        (size_t) p->uc, hipMemcpyDeviceToHost, p->stream));
	if (R_prev && p->items)
		MF_HIP(hipMemcpy2DAsync(R_prev, w, p->Rbuf[p->rule[0].at_rest ? p->cur : p->cur ^ 1], (size_t) p->ldr * sizeof(double), w,
		                        (size_t) p->items, hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

int mf_plan_download_factors(mf_plan *p, double *L_block, double *R)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	const size_t w = (size_t) p->K * sizeof(double);
	if (L_block && p->uc)
		MF_HIP(hipMemcpy2DAsync(L_block, w, p->Lbuf[p->cur], (size_t) p->ldl * sizeof(double), w, (size_t) p->uc,
		                        hipMemcpyDeviceToHost, p->stream));
	if (R && p->items)
		MF_HIP(hipMemcpy2DAsync(R, w, p->Rbuf[p->cur], (size_t) p->ldr * sizeof(double), w, (size_t) p->items,
		                        hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

int mf_plan_sweep_items(mf_plan *p, int seed_from_old)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	return launch_sweep(p, 0, seed_from_old ? 1 : 0);
}

int mf_plan_sweep_users_seeded(mf_plan *p, int seed_from_old)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	return launch_sweep(p, 1, seed_from_old ? 1 : 0);
}

int mf_plan_sweep_users(mf_plan *p) { return mf_plan_sweep_users_seeded(p, 1); }

void *mf_plan_items_next(mf_plan *p) { return p ? p->Rbuf[p->cur ^ 1] : nullptr; }
void *mf_plan_items_current(mf_plan *p) { return p ? p->Rbuf[p->cur] : nullptr; }
void *mf_plan_users_next(mf_plan *p) { return p ? p->Lbuf[p->cur ^ 1] : nullptr; }
void *mf_plan_users_current(mf_plan *p) { return p ? p->Lbuf[p->cur] : nullptr; }

int mf_plan_flip(mf_plan *p)
{
	if (!p) return MF_ERR_ARGUMENT;
	p->cur ^= 1;
	return MF_OK;
}

// the implicit solve of a side with a frozen column: its all-pairs term needs a correction the header does not define
static bool implicit_refuses(const mf_plan *p, int side) { return als_solver(p).implicit && p->rule[side].frozen >= 0; }

int mf_plan_iterate(mf_plan *p, int iters)
{
	if (!p || iters < 0) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	if (iters > 0 && (implicit_refuses(p, 0) || implicit_refuses(p, 1))) return MF_ERR_UNSUPPORTED;   // before any HIP call
	MF_HIP(hipSetDevice(p->device));
	const mf_sched::IterateInput in = iterate_input(p, iters);
	if (in.als && iters > 0 && !in.whole) return MF_ERR_UNSUPPORTED;   // the item solve of a shard
	// A momentum side at rest gets its history (X_prev = X_old) and an adaptive side its accumulators here: in front of every
	// launch and outside any capture.  Not under ALS, which reads neither.
	if (iters > 0 && !in.als) {
		MF_TRY(leave_rest(p, 0));
		MF_TRY(leave_rest(p, 1));
		MF_TRY(adaptive_ready(p, 0));
		MF_TRY(adaptive_ready(p, 1));
	}
	// which loop runs, and how much of it as graph replays: the one rule of mf_schedule.h
	const mf_sched::IteratePath path = mf_sched::iterate_path(in);
	switch (path.loop) {
	case mf_sched::kLoopAls: return iterate_als(p, path.eager);
	case mf_sched::kLoopToy: return launch_toy_loop(p, path.eager);
	case mf_sched::kLoopEs:
	case mf_sched::kLoopSweeps: break;
	}
	if (path.replays > 0) MF_TRY(replay_graph(p, path.loop, path.replays));
	return iterate_eager(p, path.loop, path.eager);
}

// a regularisation weight is finite and >= 0 (a NaN fails both comparisons' complement)
static bool lambda_ok(double v) { return std::isfinite(v) && v >= 0.0; }

int mf_plan_set_regularization(mf_plan *p, double lambda_users, double lambda_items)
{
	if (!p || !lambda_ok(lambda_users) || !lambda_ok(lambda_items)) return MF_ERR_ARGUMENT;
	// read by side_update at every launch (the graph path captures per call): nothing is cached from an earlier value
	p->rule[1].lambda = lambda_users;
	p->rule[0].lambda = lambda_items;
	return MF_OK;
}

int mf_plan_get_regularization(mf_plan *p, double *lambda_users, double *lambda_items)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (lambda_users) *lambda_users = p->rule[1].lambda;
	if (lambda_items) *lambda_items = p->rule[0].lambda;
	return MF_OK;
}

int mf_plan_set_momentum(mf_plan *p, double beta_users, double beta_items)
{
	if (!p || !lambda_ok(beta_users) || !lambda_ok(beta_items)) return MF_ERR_ARGUMENT;   // finite and >= 0, like a weight
	// not on an adaptive side: its X_new carries g, so there is no X_prev
	if ((beta_users != 0.0 && adaptive_side(p, 1)) || (beta_items != 0.0 && adaptive_side(p, 0))) return MF_ERR_UNSUPPORTED;
	if ((beta_users != 0.0 || beta_items != 0.0) && p->als_kind != MF_ALS_OFF) return MF_ERR_UNSUPPORTED;   // nor under ALS
	// read at every launch (the graph path captures per call).  A side whose beta leaves 0 has maintained no history: it
	// is at rest; a change between two non-zero values keeps the history
	if (p->rule[1].beta == 0.0 && beta_users != 0.0) p->rule[1].at_rest = true;
	if (p->rule[0].beta == 0.0 && beta_items != 0.0) p->rule[0].at_rest = true;
	p->rule[1].beta = beta_users;
	p->rule[0].beta = beta_items;
	return MF_OK;
}

int mf_plan_get_momentum(mf_plan *p, double *beta_users, double *beta_items)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (beta_users) *beta_users = p->rule[1].beta;
	if (beta_items) *beta_items = p->rule[0].beta;
	return MF_OK;
}

int mf_plan_set_frozen_columns(mf_plan *p, int32_t users_col, int32_t items_col)
{
	if (!p || users_col < -1 || items_col < -1 || users_col >= p->K || items_col >= p->K) return MF_ERR_ARGUMENT;
	// read at every launch, like the decay: the graph path captures per call, so no replay sees an earlier value
	p->rule[1].frozen = users_col;
	p->rule[0].frozen = items_col;
	return MF_OK;
}

int mf_plan_get_frozen_columns(mf_plan *p, int32_t *users_col, int32_t *items_col)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (users_col) *users_col = p->rule[1].frozen;
	if (items_col) *items_col = p->rule[0].frozen;
	return MF_OK;
}

// a box [lo, hi] over a leading range of columns: no NaN bound, lo <= hi, columns >= -1 (K is checked where it is known)
static bool bounds_ok(double lo, double hi, int32_t columns) { return !std::isnan(lo) && !std::isnan(hi) && !(lo > hi) && columns >= -1; }

int mf_plan_set_bounds(mf_plan *p, int side, double lo, double hi, int32_t columns)
{
	// the plan is looked at last: everything else is refused without it
	if (!p || (side != 0 && side != 1) || !bounds_ok(lo, hi, columns) || columns > p->K) return MF_ERR_ARGUMENT;
	// read at every launch, like the decay: the graph path captures per call, so no replay sees an earlier value
	p->rule[side].lo = lo;
	p->rule[side].hi = hi;
	p->rule[side].columns = columns;
	return MF_OK;
}

int mf_plan_get_bounds(mf_plan *p, int side, double *lo, double *hi, int32_t *columns)
{
	if (!p || (side != 0 && side != 1)) return MF_ERR_ARGUMENT;
	if (lo) *lo = p->rule[side].lo;
	if (hi) *hi = p->rule[side].hi;
	if (columns) *columns = p->rule[side].columns;
	return MF_OK;
}

// the arguments of the two box passes over one buffer of a side: every row, the bounded columns but the frozen one
static mf::BoxArgs box_args(mf_plan *p, int side, int generation)
{
	mf::BoxArgs a;
	a.X = side == 0 ? p->Rbuf[p->cur ^ generation] : p->Lbuf[p->cur ^ generation];
	a.rows = side == 0 ? p->items : p->uc;
	a.ld = side == 0 ? p->ldr : p->ldl;
	const SideUpdate u = side_update(p, side, 1);
	// the side's own column range, whatever its bounds: the count of an unbounded side puts every entry `inside`
	a.columns = p->rule[side].columns < 0 ? p->K : p->rule[side].columns;
	a.frozen = u.frozen;
	a.lo = u.box.lo;
	a.hi = u.box.hi;
	a.counts = nullptr;
	return a;
}

static int box_grid(const mf::BoxArgs &a) { return std::min((a.rows + mf::kBoxRows - 1) / mf::kBoxRows, 1 << 16); }

int mf_plan_project(mf_plan *p, int side, int generation)
{
	if (!p || (side != 0 && side != 1) || (generation != 0 && generation != 1)) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	const mf::BoxArgs a = box_args(p, side, generation);
	if (a.rows <= 0 || a.columns <= 0 || !a.X) return MF_OK;
	hipLaunchKernelGGL(mf::box_project_kernel, dim3(box_grid(a)), dim3(mf::kBoxThreads), 0, p->stream, a);
	MF_HIP(hipGetLastError());
	return MF_OK;
}

int mf_plan_bounds_active(mf_plan *p, int side, int64_t *at_lo, int64_t *at_hi, int64_t *inside)
{
	if (!p || (side != 0 && side != 1)) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	unsigned long long c[3] = {0, 0, 0};
	mf::BoxArgs a = box_args(p, side, 0);
	if (a.rows > 0 && a.columns > 0) {
		if (!p->box_counts) MF_TRY(p->box_counts.alloc(3));
		a.counts = p->box_counts;
		MF_HIP(hipMemsetAsync(a.counts, 0, sizeof c, p->stream));
		hipLaunchKernelGGL(mf::box_count_kernel, dim3(box_grid(a)), dim3(mf::kBoxThreads), 0, p->stream, a);
		MF_HIP(hipGetLastError());
		MF_HIP(hipMemcpyAsync(c, a.counts, sizeof c, hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipStreamSynchronize(p->stream));
	}
	if (at_lo) *at_lo = (int64_t) c[0];
	if (at_hi) *at_hi = (int64_t) c[1];
	if (inside) *inside = (int64_t) c[2];
	return MF_OK;
}

// an adaptive rule: NULL or kind NONE (no rule), or a known kind with eta and eps finite and > 0 and the betas the kind
// reads in [0, 1)
static bool unit_ok(double v) { return v >= 0.0 && v < 1.0; }
static bool adaptive_ok(const mf_adaptive *o)
{
	if (!o || o->kind == MF_OPT_NONE) return true;
	if (o->kind != MF_OPT_ADAGRAD && o->kind != MF_OPT_RMSPROP && o->kind != MF_OPT_ADAM) return false;
	if (!std::isfinite(o->eta) || !(o->eta > 0.0) || !std::isfinite(o->eps) || !(o->eps > 0.0)) return false;
	if (o->kind != MF_OPT_ADAGRAD && !unit_ok(o->beta2)) return false;
	return o->kind != MF_OPT_ADAM || unit_ok(o->beta1);
}
static const mf_adaptive kNoAdaptive = {MF_OPT_NONE, 0.0, 0.0, 0.0, 0.0};
static mf_adaptive adaptive_rule(const mf_adaptive *o) { return o && o->kind != MF_OPT_NONE ? *o : kNoAdaptive; }

int mf_plan_set_adaptive(mf_plan *p, int side, const mf_adaptive *rule)
{
	if (!p || (side != 0 && side != 1) || !adaptive_ok(rule)) return MF_ERR_ARGUMENT;
	const mf_adaptive o = adaptive_rule(rule);
	if (o.kind != MF_OPT_NONE && p->rule[side].beta != 0.0) return MF_ERR_UNSUPPORTED;   // momentum came first
	if (o.kind != MF_OPT_NONE && p->als_kind != MF_ALS_OFF) return MF_ERR_UNSUPPORTED;    // ... or ALS did
	// read at every launch (the graph path captures per call).  A change of kind puts the side at rest; a change of the
	// numbers alone keeps what it has accumulated
	if (o.kind != p->rule[side].opt.kind) p->opt[side].rest = true;
	p->rule[side].opt = o;
	return MF_OK;
}

int mf_plan_get_adaptive(mf_plan *p, int side, mf_adaptive *rule)
{
	if (!p || (side != 0 && side != 1)) return MF_ERR_ARGUMENT;
	if (rule) *rule = p->rule[side].opt;
	return MF_OK;
}

int mf_plan_reset_adaptive(mf_plan *p, int side)
{
	if (!p || (side != 0 && side != 1)) return MF_ERR_ARGUMENT;
	p->opt[side].rest = true;
	return MF_OK;
}

int mf_plan_adaptive_finish(mf_plan *p, int side)
{
	if (!p || (side != 0 && side != 1)) return MF_ERR_ARGUMENT;
	if (!p->have_factors || !adaptive_side(p, side)) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	if (p->side[side].nrows <= 0) return MF_OK;
	MF_TRY(adaptive_ready(p, side));
	MF_TRY(launch_adaptive_tick(p, side));
	return launch_adaptive_finish(p, side, nullptr, p->side[side].nrows, p->stream);
}

int mf_plan_download_adaptive_state(mf_plan *p, int side, double *m, double *v, int64_t *steps, double *p1, double *p2)
{
	if (!p || (side != 0 && side != 1)) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	const AdaptiveState &s = p->opt[side];
	const int rows = side == 0 ? p->items : p->uc, ld = side == 0 ? p->ldr : p->ldl;
	const size_t n = (size_t) rows * p->K, w = (size_t) p->K * sizeof(double);
	const bool rest = !adaptive_side(p, side) || s.rest || !s.step || !s.v;
	const bool have_m = !rest && p->rule[side].opt.kind == MF_OPT_ADAM && s.m;
	mf::AdaptiveStep rec{1.0, 1.0, 0.0, 0.0, 0};
	if (m && !have_m) std::fill(m, m + n, 0.0);
	if (v && rest) std::fill(v, v + n, 0.0);
	if (!rest) {
		MF_HIP(hipSetDevice(p->device));
		if (m && have_m && rows) MF_HIP(hipMemcpy2DAsync(m, w, s.m, (size_t) ld * sizeof(double), w, (size_t) rows, hipMemcpyDeviceToHost, p->stream));
		if (v && rows) MF_HIP(hipMemcpy2DAsync(v, w, s.v, (size_t) ld * sizeof(double), w, (size_t) rows, hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipMemcpyAsync(&rec, s.step, sizeof rec, hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipStreamSynchronize(p->stream));
	}
	if (steps) *steps = (int64_t) rec.steps;
	if (p1) *p1 = rec.p1;
	if (p2) *p2 = rec.p2;
	return MF_OK;
}

int mf_plan_upload_adaptive_state(mf_plan *p, int side, const double *m, const double *v, const int64_t *steps, const double *p1,
                                  const double *p2)
{
	if (!p || (side != 0 && side != 1) || (steps && *steps < 0) || (p1 && std::isnan(*p1)) || (p2 && std::isnan(*p2))) return MF_ERR_ARGUMENT;
	if (!p->have_factors || !adaptive_side(p, side)) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	MF_TRY(adaptive_ready(p, side));   // what is not given starts from rest, or stays as it is
	AdaptiveState &s = p->opt[side];
	const int rows = side == 0 ? p->items : p->uc, ld = side == 0 ? p->ldr : p->ldl;
	const size_t w = (size_t) p->K * sizeof(double);
	if (m && rows && p->rule[side].opt.kind == MF_OPT_ADAM)
		MF_HIP(hipMemcpy2DAsync(s.m, (size_t) ld * sizeof(double), m, w, w, (size_t) rows, hipMemcpyHostToDevice, p->stream));
	if (v && rows) MF_HIP(hipMemcpy2DAsync(s.v, (size_t) ld * sizeof(double), v, w, w, (size_t) rows, hipMemcpyHostToDevice, p->stream));
	if (steps || p1 || p2) {
		mf::AdaptiveStep rec;
		MF_HIP(hipMemcpyAsync(&rec, s.step, sizeof rec, hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipStreamSynchronize(p->stream));
		MF_TRY(adaptive_set_record(p, side, p1 ? *p1 : rec.p1, p2 ? *p2 : rec.p2, steps ? (long long) *steps : rec.steps));
	}
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

// the kinds of the explicit solve (mf_backend_run_als takes these); the implicit one comes with a confidence
static bool als_kind_ok(int kind) { return kind == MF_ALS_OFF || kind == MF_ALS_RIDGE || kind == MF_ALS_RIDGE_COUNT; }

int mf_plan_set_als(mf_plan *p, int kind)
{
	if (!p || !(als_kind_ok(kind) || kind == MF_ALS_IMPLICIT)) return MF_ERR_ARGUMENT;
	if (kind != MF_ALS_OFF) {
		// the solve this kind would run (als_solver, mf_schedule.h) takes the plan's K and, under the implicit kind, is implicit
		const mf_sched::AlsSolver s = mf_sched::als_solver(kind, p->als_cg, p->implicit_cg, p->als_box);
		if (p->K > s.max_k || (kind == MF_ALS_IMPLICIT && !s.implicit)) return MF_ERR_UNSUPPORTED;
		if (s.cg && p->als_box > 0) return MF_ERR_UNSUPPORTED;   // box sweeps and the implicit kind's CG steps, both waiting for it
		// a solve has neither a previous step nor a gradient: momentum or an adaptive side came first
		if (p->rule[0].beta != 0.0 || p->rule[1].beta != 0.0 || adaptive_any(p)) return MF_ERR_UNSUPPORTED;
	}
	// the counters exist from here on: a solve only enqueues and allocates nothing
	if (kind != MF_ALS_OFF && !p->als_counts) {
		MF_HIP(hipSetDevice(p->device));
		MF_TRY(p->als_counts.alloc(6));
		MF_HIP(hipMemsetAsync(p->als_counts.get(), 0, 6 * sizeof(unsigned long long), p->stream));
	}
	if (kind == MF_ALS_IMPLICIT) {   // and so do the Gram buffers
		MF_HIP(hipSetDevice(p->device));
		MF_TRY(gram_buffers(p));
	}
	p->als_kind = kind;   // read at every launch
	return MF_OK;
}

int mf_plan_get_als(mf_plan *p, int *kind)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (kind) *kind = p->als_kind;
	return MF_OK;
}

int mf_plan_set_als_cg(mf_plan *p, int steps)
{
	if (!p || steps < 0 || steps > MF_ALS_CG_MAX_STEPS) return MF_ERR_ARGUMENT;
	// the solve these steps would run (als_solver, mf_schedule.h): implicit under the implicit kind, and K within its limit
	const mf_sched::AlsSolver s = mf_sched::als_solver(p->als_kind, steps, p->implicit_cg);
	if (p->als_kind == MF_ALS_IMPLICIT && !s.implicit) return MF_ERR_UNSUPPORTED;
	if (steps > 0 && p->als_box > 0) return MF_ERR_UNSUPPORTED;   // box sweeps came first (mf_plan_set_als_box)
	if (p->K > s.max_k && (s.cg || p->als_kind != MF_ALS_OFF)) return MF_ERR_UNSUPPORTED;
	p->als_cg = steps;   // read at every launch
	return MF_OK;
}

int mf_plan_get_als_cg(mf_plan *p, int *steps)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (steps) *steps = p->als_cg;
	return MF_OK;
}

int mf_plan_set_implicit_cg(mf_plan *p, int steps)
{
	if (!p || steps < 0 || steps > MF_ALS_CG_MAX_STEPS) return MF_ERR_ARGUMENT;
	// under the implicit kind the steps are in force: box sweeps came first (mf_plan_set_als_box)
	if (steps > 0 && p->als_box > 0 && p->als_kind == MF_ALS_IMPLICIT) return MF_ERR_UNSUPPORTED;
	p->implicit_cg = steps;   // read at every launch, and only while the kind is MF_ALS_IMPLICIT
	return MF_OK;
}

int mf_plan_set_als_box(mf_plan *p, int sweeps)
{
	if (!p || sweeps < 0 || sweeps > MF_ALS_BOX_MAX_SWEEPS) return MF_ERR_ARGUMENT;
	if (sweeps > 0) {
		// the solve the plan runs without them (als_solver, mf_schedule.h) has to be the direct one, at a K it takes
		const mf_sched::AlsSolver s = als_solver(p);
		if (s.cg || p->als_cg > 0) return MF_ERR_UNSUPPORTED;
		if (p->als_kind != MF_ALS_OFF && p->K > mf_sched::kAlsDirectMaxK) return MF_ERR_UNSUPPORTED;
	}
	p->als_box = sweeps;   // read at every launch
	return MF_OK;
}

int mf_plan_get_als_box(mf_plan *p, int *sweeps)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (sweeps) *sweeps = p->als_box;
	return MF_OK;
}

int mf_plan_get_implicit_cg(mf_plan *p, int *steps)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (steps) *steps = p->implicit_cg;
	return MF_OK;
}

int mf_plan_als_solve(mf_plan *p, int side, int other_generation)
{
	if (!p || (side != 0 && side != 1) || (other_generation != 0 && other_generation != 1)) return MF_ERR_ARGUMENT;
	if (!p->have_factors || p->als_kind == MF_ALS_OFF) return MF_ERR_STATE;
	// an item's Gram matrix is a sum over ALL users: a plan that holds a block of them (a shard, a 2-D tile) has a part of it
	if (side == 0 && (p->u0 != 0 || p->uc != p->users_total)) return MF_ERR_UNSUPPORTED;
	if (implicit_refuses(p, side)) return MF_ERR_UNSUPPORTED;
	MF_HIP(hipSetDevice(p->device));
	return launch_als(p, side, other_generation);
}

int64_t mf_backend_als_normal_pitch(int32_t features)
{
	if (features < 1) return 0;
	const int64_t K = features;
	return (K * (K + 1) / 2 + K + 1 + 1) / 2 * 2;   // mf::als_normal_pitch in 64 bits, for any K
}

// what both halves of the cut solve refuse, before any HIP call
static int als_normal_check(const mf_plan *p, int side, int other_generation, const void *device_normal, int64_t pitch)
{
	if (!p || (side != 0 && side != 1) || (other_generation != 0 && other_generation != 1)) return MF_ERR_ARGUMENT;
	if (!device_normal || ((uintptr_t) device_normal & 15) != 0 || (pitch & 1) != 0) return MF_ERR_ARGUMENT;
	if (p->K <= mf::kAlsMaxK && pitch < mf::als_normal_pitch(p->K)) return MF_ERR_ARGUMENT;
	if (!p->have_factors || p->als_kind == MF_ALS_OFF) return MF_ERR_STATE;
	if (als_solver(p).cg || p->K > mf::kAlsMaxK) return MF_ERR_UNSUPPORTED;   // CG on shards needs a sum per step
	if (implicit_refuses(p, side)) return MF_ERR_UNSUPPORTED;
	return MF_OK;
}

int mf_plan_als_normal(mf_plan *p, int side, int other_generation, void *device_normal, int64_t pitch)
{
	MF_TRY(als_normal_check(p, side, other_generation, device_normal, pitch));
	MF_HIP(hipSetDevice(p->device));
	return launch_als_normal(p, side, other_generation, (double *) device_normal, (long long) pitch, false);
}

int mf_plan_als_solve_normal(mf_plan *p, int side, const void *device_normal, int64_t pitch)
{
	MF_TRY(als_normal_check(p, side, 0, device_normal, pitch));
	MF_HIP(hipSetDevice(p->device));
	return launch_als_normal(p, side, 0, (double *) const_cast<void *>(device_normal), (long long) pitch, true);
}

int mf_plan_set_confidence(mf_plan *p, double conf)
{
	if (!p || !std::isfinite(conf) || conf < 0.0) return MF_ERR_ARGUMENT;
	p->confidence = conf;   // read at every launch
	return MF_OK;
}

int mf_plan_get_confidence(mf_plan *p, double *conf)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (conf) *conf = p->confidence;
	return MF_OK;
}

int mf_plan_gram(mf_plan *p, int side, int generation, double *triangle)
{
	if (!p || (side != 0 && side != 1) || (generation != 0 && generation != 1)) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	if (p->K > mf::kAlsMaxK) return MF_ERR_UNSUPPORTED;
	MF_HIP(hipSetDevice(p->device));
	MF_TRY(gram_buffers(p));
	MF_TRY(launch_gram(p, side, generation));
	if (triangle) {
		const size_t tri = (size_t) mf::als_triangle(p->K);
		MF_HIP(hipMemcpyAsync(triangle, p->gram.get() + (size_t) side * tri, tri * sizeof(double), hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipStreamSynchronize(p->stream));
	}
	return MF_OK;
}

int mf_backend_gram_dot(const double *left, const double *right, int32_t features, double *out)
{
	if (!left || !right || !out || features < 1) return MF_ERR_ARGUMENT;
	double t = 0.0;
	for (int p = 0; p < features; ++p)
		for (int q = 0; q < features; ++q) {
			const size_t e = p >= q ? (size_t) p * (p + 1) / 2 + q : (size_t) q * (q + 1) / 2 + p;   // the upper triangle by symmetry
			const double m = left[e] * right[e];
			t = t + m;
		}
	*out = t;
	return MF_OK;
}

int mf_plan_implicit_objective(mf_plan *p, mf_implicit_objective *out)
{
	if (!p || !out) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	if (p->K > mf::kAlsMaxK) return MF_ERR_UNSUPPORTED;
	return implicit_objective_eval(p, out);
}

int mf_plan_als_info(mf_plan *p, int side, int64_t *solved, int64_t *kept_empty, int64_t *kept_not_pd)
{
	if (!p || (side != 0 && side != 1)) return MF_ERR_ARGUMENT;
	unsigned long long c[3] = {0, 0, 0};
	if (p->als_counts) {   // no solve yet: zeros
		MF_HIP(hipSetDevice(p->device));
		MF_HIP(hipMemcpyAsync(c, p->als_counts.get() + 3 * side, sizeof c, hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipStreamSynchronize(p->stream));
	}
	if (solved) *solved = (int64_t) c[0];
	if (kept_empty) *kept_empty = (int64_t) c[1];
	if (kept_not_pd) *kept_not_pd = (int64_t) c[2];
	return MF_OK;
}

int mf_plan_penalty(mf_plan *p, double *users_sq, double *items_sq, double *user_rows, double *item_rows)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	return penalty_eval(p, users_sq, items_sq, user_rows, item_rows);
}

int mf_plan_recommend(mf_plan *p, int32_t *best)
{
	if (!p || (!best && p->uc > 0)) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	if (p->uc == 0) return MF_OK;
	const bool use_mfma = !p->cfg.rec_exact;   // MF_RECOMMEND_IMPL=mfma (default) | exact
	mf::RecArgs ex = exact_args(p, p->uc, nullptr, nullptr);
	if (!use_mfma) {
		const int grid = (p->uc + mf::kRT - 1) / mf::kRT;
		hipLaunchKernelGGL(mf::recommend_kernel, dim3(grid), dim3(256), 0, p->stream, ex);
		MF_HIP(hipGetLastError());
		p->last_uncertain = -1;
	} else {
		// pass 1: scores on the FP64 matrix cores + certification margin; pass 2: exact re-scoring of the rest
		{
			const int rc1 = launch_recommend_pass1(p, nullptr);
			if (rc1 != MF_OK) return rc1;
		}
		// the list travels with the count of uncertified users: one synchronisation when nobody needs the exact pass
		// (the common case: 0 of 1e6 users at cfg4), a second copy of the list only behind an exact pass
		int cnt = 0;
		MF_HIP(hipMemcpyAsync(&cnt, p->ucount, sizeof(int), hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipMemcpyAsync(best, p->best_dev, (size_t) p->uc * sizeof(int), hipMemcpyDeviceToHost, p->stream));
		MF_HIP(hipStreamSynchronize(p->stream));
		p->last_uncertain = cnt;
		if (cnt == 0) return MF_OK;
		ex.users = cnt;
		ex.ulist = p->ulist;
		hipLaunchKernelGGL(mf::recommend_kernel, dim3((cnt + mf::kRT - 1) / mf::kRT), dim3(256), 0, p->stream, ex);
		MF_HIP(hipGetLastError());
	}
	MF_HIP(hipMemcpyAsync(best, p->best_dev, (size_t) p->uc * sizeof(int), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

int mf_plan_recommend_scored(mf_plan *p, mf_candidate *out)
{
	if (!p || (!out && p->uc > 0)) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	if (p->uc == 0) return MF_OK;
	{
		const int rc = p->cand_dev.grow((size_t) p->uc);
		if (rc != MF_OK) return rc;
	}
	const mf::RecArgs ex = exact_args(p, p->uc, nullptr, p->cand_dev);
	hipLaunchKernelGGL(mf::recommend_kernel, dim3((p->uc + mf::kRT - 1) / mf::kRT), dim3(256), 0, p->stream, ex);
	MF_HIP(hipGetLastError());
	MF_HIP(hipMemcpyAsync(out, p->cand_dev, (size_t) p->uc * sizeof(mf_candidate), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

int mf_plan_recommend_scored_users(mf_plan *p, const int32_t *users, int32_t n, mf_candidate *out)
{
	if (!p || n < 0 || (n > 0 && (!users || !out)) || n > p->uc) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	for (int32_t t = 0; t < n; ++t)
		if (users[t] < 0 || users[t] >= p->uc) return MF_ERR_ARGUMENT;
	MF_HIP(hipSetDevice(p->device));
	if (n == 0) return MF_OK;
	{
		const int rc = p->cand_dev.grow((size_t) p->uc);
		if (rc != MF_OK) return rc;
	}
	MF_HIP(hipMemcpyAsync(p->ulist, users, (size_t) n * sizeof(int), hipMemcpyHostToDevice, p->stream));
	const mf::RecArgs ex = exact_args(p, n, p->ulist, p->cand_dev);   // cand is written at the user's own index
	hipLaunchKernelGGL(mf::recommend_kernel, dim3((n + mf::kRT - 1) / mf::kRT), dim3(256), 0, p->stream, ex);
	MF_HIP(hipGetLastError());
	// only the n requested records travel: packed on the device in list order
	{
		const int rc = p->cand_pack.grow((size_t) p->uc);
		if (rc != MF_OK) return rc;
	}
	hipLaunchKernelGGL(mf::pack_candidates_kernel, dim3((n + 255) / 256), dim3(256), 0, p->stream, p->cand_dev, p->ulist,
	                   n, p->cand_pack);
	MF_HIP(hipGetLastError());
	MF_HIP(hipMemcpyAsync(out, p->cand_pack, (size_t) n * sizeof(mf_candidate), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

double mf_backend_recommend_margin(int features) { return 8.0 * (double) (features + 8) * 1.1102230246251565e-16; }

int mf_plan_recommend_filter(mf_plan *p, mf_filter *out, double *norm, double *rmax)
{
	if (!p || (p->uc > 0 && (!out || !norm)) || !rmax) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	MF_HIP(hipSetDevice(p->device));
	*rmax = 0.0;
	if (p->uc == 0) return MF_OK;
	int rc = p->filt_dev.grow((size_t) p->uc);
	if (rc == MF_OK) rc = launch_recommend_pass1(p, p->filt_dev);
	if (rc != MF_OK) return rc;
	unsigned long long bits = 0;
	MF_HIP(hipMemcpyAsync(out, p->filt_dev, (size_t) p->uc * sizeof(mf_filter), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipMemcpyAsync(norm, p->lnorm, (size_t) p->uc * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipMemcpyAsync(&bits, p->rmax_bits, sizeof bits, hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	memcpy(rmax, &bits, sizeof bits);   // a NaN norm arrives as NaN: the caller then certifies nobody
	return MF_OK;
}

int mf_plan_recommend_info(mf_plan *p, int64_t *exact_pass_users)
{
	if (!p || !exact_pass_users) return MF_ERR_ARGUMENT;
	*exact_pass_users = p->last_uncertain;
	return MF_OK;
}

int mf_plan_recommend_topn(mf_plan *p, int32_t n, int32_t *items, double *scores)
{
	if (!p || n < 1 || !items) return MF_ERR_ARGUMENT;
	if (n > MF_TOPN_MAX) return MF_ERR_UNSUPPORTED;
	if (!p->have_factors) return MF_ERR_STATE;
	if (p->uc == 0) {   // nothing to rank: no pass ran
		p->topn.last_uncertain = 0;
		p->topn.form = 0;
		return MF_OK;
	}
	const int rc = launch_topn(p, n);
	if (rc != MF_OK) return rc;
	const size_t cnt = (size_t) p->uc * (size_t) n;
	MF_HIP(hipMemcpyAsync(items, p->topn.items, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
	if (scores) MF_HIP(hipMemcpyAsync(scores, p->topn.scores, cnt * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

int mf_plan_recommend_topn_info(mf_plan *p, int64_t *exact_pass_users, int32_t *mfma_form)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (exact_pass_users) *exact_pass_users = p->topn.last_uncertain;
	if (mfma_form) *mfma_form = p->topn.form;
	return MF_OK;
}

// the argument rules of the two similar-items entry points, checked before any HIP call
static int similar_check(int32_t items_total, int metric, const int32_t *query, int32_t nq, int32_t n, const int32_t *out_items)
{
	if (!out_items || n < 1 || nq < 0 || (metric != MF_SIMILAR_DOT && metric != MF_SIMILAR_COSINE)) return MF_ERR_ARGUMENT;
	if (!query && nq != items_total) return MF_ERR_ARGUMENT;
	if (query)
		for (int32_t t = 0; t < nq; ++t)
			if (query[t] < 0 || query[t] >= items_total) return MF_ERR_ARGUMENT;
	if (n > MF_TOPN_MAX) return MF_ERR_UNSUPPORTED;
	return MF_OK;
}

int mf_plan_similar_items(mf_plan *p, int metric, const int32_t *query, int32_t nq, int32_t n, int32_t *items, double *scores)
{
	if (!p) return MF_ERR_ARGUMENT;
	const int chk = similar_check(p->items, metric, query, nq, n, items);
	if (chk != MF_OK) return chk;
	if (!p->have_factors) return MF_ERR_STATE;
	if (nq == 0) {   // nothing to rank: no pass ran
		p->sim.last_uncertain = 0;
		p->sim.form = 0;
		return MF_OK;
	}
	const int rc = launch_similar(p, metric, query, nq, n);
	if (rc != MF_OK) return rc;
	const size_t cnt = (size_t) nq * (size_t) n;
	MF_HIP(hipMemcpyAsync(items, p->sim.items, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
	if (scores) MF_HIP(hipMemcpyAsync(scores, p->sim.scores, cnt * sizeof(double), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

int mf_plan_similar_items_info(mf_plan *p, int64_t *exact_pass_queries, int32_t *mfma_form)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (exact_pass_queries) *exact_pass_queries = p->sim.last_uncertain;
	if (mfma_form) *mfma_form = p->sim.form;
	return MF_OK;
}

int mf_plan_predict(mf_plan *p, double *B)
{
	if (!p || !B) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	const size_t n = (size_t) p->uc * (size_t) p->items;
	if (n > ((size_t) 1 << 26)) return MF_ERR_UNSUPPORTED;
	if (n == 0) return MF_OK;
	MF_HIP(hipSetDevice(p->device));
	dev_buf<double> dB;
	{
		const int rc = dB.alloc(n);
		if (rc != MF_OK) return rc;
	}
	hipLaunchKernelGGL(mf::predict_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, p->stream,
	                   p->Lbuf[p->cur], p->Rbuf[p->cur], p->uc, p->items, p->K, p->ldl, p->ldr, dB);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(B, dB, n * sizeof(double), hipMemcpyDeviceToHost, p->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
	if (e != hipSuccess) {
		g_last_hip_error = std::string("mf_plan_predict: ") + hipGetErrorString(e);
		return MF_ERR_HIP;
	}
	return MF_OK;
}

int mf_plan_synchronize(mf_plan *p)
{
	if (!p) return MF_ERR_ARGUMENT;
	MF_HIP(hipSetDevice(p->device));
	MF_HIP(hipStreamSynchronize(p->stream));
	return MF_OK;
}

int mf_plan_timing(mf_plan *p, int enable)
{
	if (!p) return MF_ERR_ARGUMENT;
	p->timing = enable != 0;
	return MF_OK;
}

int mf_plan_timing_read(mf_plan *p, int64_t *item_launches, double *item_ms, int64_t *user_launches,
                        double *user_ms)
{
	if (!p) return MF_ERR_ARGUMENT;
	MF_HIP(hipSetDevice(p->device));
	const int rc = drain_timing(p);
	if (rc != MF_OK) return rc;
	if (item_launches) *item_launches = p->acc_launch[0];
	if (item_ms) *item_ms = p->acc_ms[0];
	if (user_launches) *user_launches = p->acc_launch[1];
	if (user_ms) *user_ms = p->acc_ms[1];
	p->acc_launch[0] = p->acc_launch[1] = 0;
	p->acc_ms[0] = p->acc_ms[1] = 0.0;
	return MF_OK;
}

// printf at the end of the text in buf, while there is room for any of it
__attribute__((format(printf, 3, 4))) static void append(char *buf, int buflen, const char *fmt, ...)
{
	const size_t at = strlen(buf);
	if (at + 1 >= (size_t) buflen) return;
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf + at, (size_t) buflen - at, fmt, ap);
	va_end(ap);
}

int mf_plan_describe(mf_plan *p, char *buf, int buflen)
{
	if (!p || !buf || buflen <= 0) return MF_ERR_ARGUMENT;
	int n;
	const SweepSide &it = p->side[0], &us = p->side[1];
	if (p->sweep.dma)
		n = snprintf(buf, (size_t) buflen,
		             "sweep_dma_kernel<KT=%d,NPASS=%d> K=%d pitch=%d/%d nch=%d row_bytes=%d lds=%zu long_rows=%d/%d coop_nch=%d double_buffered=%d/%d(nch=%d) wave_pair=%d/%d(nch=%d)",
		             p->sweep.kt, p->sweep.kt ? mf::dma_passes(p->K) : p->sweep.kpmax, p->K, p->ldl, p->ldr, p->single.nch, p->sweep.row_bytes,
		             p->single.lds, it.n_long + (it.coop_all ? it.nrows : 0), us.n_long + (us.coop_all ? us.nrows : 0),
		             it.coop_all || us.coop_all ? p->coop.nch : 0, (int) it.use_db, (int) us.use_db, p->db.nch, (int) it.use_pair, (int) us.use_pair, p->pair.nch);
	else
		n = snprintf(buf, (size_t) buflen, "sweep_kernel<KT=%d,KPMAX=%d> K=%d nch=%d stride=%d lds=%zu",
		             p->sweep.kt, p->sweep.kpmax, p->K, p->single.nch, p->stride, p->single.lds);
	// accumulate form of the single-wave launch of the item / user sweep (the rule of launch_sweep, mf_launch.hip.h)
	if (n > 0 && n < buflen)
		n += snprintf(buf + n, (size_t) (buflen - n), " accumulate=%s/%s", single_wave_pipelined(p, 0) ? "pf" : "plain",
		              single_wave_pipelined(p, 1) ? "pf" : "plain");
	// item bands of the user sweep (mf_schedule.h: band_count and bands_at_launch), told only when there are any: what a
	// seeded sweep would run in now, under the update rule in force
	int user_bands = 0;
	if (p->als_kind == MF_ALS_OFF) {
		const SideUpdate u = side_update(p, 1, 1);
		const Flavour fl = mf_sched::launch_flavour(p->weighted, u.beta != 0.0, u.d != 1.0 || u.frozen >= 0 || u.box.columns > 0);
		if (mf_sched::bands_at_launch(us.bands, 1, fl, adaptive_side(p, 1))) user_bands = us.bands;
		// ... and none where the side's last sweep was launched unseeded (a sharded driver's non-root contribution)
		if (us.last_unseeded) user_bands = 0;
	}
	if (user_bands > 0 && n > 0 && n < buflen) n += snprintf(buf + n, (size_t) (buflen - n), " user_bands=%d", user_bands);
	// how mf_plan_iterate runs an iteration: the two sweeps above, or errors + streams (mf_stream.hip.h)
	if (n > 0 && n < buflen) {
		if (!p->es_mode)
			snprintf(buf + n, (size_t) (buflen - n), " iterate=sweeps");
		else
			snprintf(buf + n, (size_t) (buflen - n),
			         " iterate=errors+resident-streams(segments=%d x<=%d, %d-column slices of Y in LDS, %d workgroups, lds=%zu/%zu)",
			         p->es_nseg, p->es_nch, p->res_sw, p->res_nwg, p->es_lds_errors, p->res_lds);
	}
	// the row-sum launch of mf_plan_loss: form, chunk sizes (ordinary / few rows) and LDS requests
	append(buf, buflen, " loss=%s(nch=%d/%d lds=%zu/%zu)", p->sweep.dma ? "loss_dma_kernel" : "loss_reg_kernel", p->loss_nch[0], p->loss_nch[1],
	       p->loss_lds[0], p->loss_lds[1]);
	// the update rule in force, users / items, each part when a side has any: regularisation, momentum, frozen columns
	const SideRule &ri = p->rule[0], &ru = p->rule[1];
	if (ri.lambda != 0.0 || ru.lambda != 0.0) append(buf, buflen, " lambda=%g/%g", ru.lambda, ri.lambda);
	if (ri.beta != 0.0 || ru.beta != 0.0) append(buf, buflen, " momentum=%g/%g", ru.beta, ri.beta);
	if (ri.frozen >= 0 || ru.frozen >= 0) append(buf, buflen, " frozen=%d/%d", ru.frozen, ri.frozen);
	// the box constraints in force, when a side has one: bounds=<users>/<items>, a side as [lo,hi]x<columns> with the bounds
	// in %.17g (they read back exactly) and the columns counted (-1 told: K), or - for a side without
	const mf::Box box[2] = {side_update(p, 0, 1).box, side_update(p, 1, 1).box};
	if (box[0].columns > 0 || box[1].columns > 0) {
		char sd[2][96];
		for (int k = 0; k < 2; ++k) {
			if (box[k].columns > 0)
				snprintf(sd[k], sizeof sd[k], "[%.17g,%.17g]x%d", box[k].lo, box[k].hi, box[k].columns);
			else
				snprintf(sd[k], sizeof sd[k], "-");
		}
		append(buf, buflen, " bounds=%s/%s", sd[1], sd[0]);
	}
	// per-entry weights, when the plan was created with them
	if (p->weighted) append(buf, buflen, " weighted=1");
	// the adaptive rules in force, when a side has one: adaptive=<users>/<items>, the numbers in %.17g (they read back
	// exactly).  What a side with one means for the loop mf_plan_iterate runs, whatever iterate= says above, is
	// mf_sched::iterate_path's to say (mf_schedule.h)
	if (adaptive_any(p)) {
		char sd[2][160];
		for (int k = 0; k < 2; ++k) {
			const mf_adaptive &o = p->rule[k].opt;
			if (o.kind == MF_OPT_ADAM)
				snprintf(sd[k], sizeof sd[k], "adam(%.17g,%.17g,%.17g,%.17g)", o.eta, o.beta1, o.beta2, o.eps);
			else if (o.kind == MF_OPT_RMSPROP)
				snprintf(sd[k], sizeof sd[k], "rmsprop(%.17g,%.17g,%.17g)", o.eta, o.beta2, o.eps);
			else if (o.kind == MF_OPT_ADAGRAD)
				snprintf(sd[k], sizeof sd[k], "adagrad(%.17g,%.17g)", o.eta, o.eps);
			else
				snprintf(sd[k], sizeof sd[k], "-");
		}
		append(buf, buflen, " adaptive=%s/%s", sd[1], sd[0]);
	}
	// the solver of mf_plan_iterate when it is not the gradient step, and the form its solves launch
	if (p->als_kind != MF_ALS_OFF) {
		const mf_sched::AlsSolver s = als_solver(p);
		if (s.implicit)
			append(buf, buflen, " als=implicit conf=%.17g", p->confidence);
		else
			append(buf, buflen, " als=%s", p->als_kind == MF_ALS_RIDGE ? "ridge" : "ridge-count");
		if (s.cg) {
			append(buf, buflen, " %s=%d als_cg_form=%s(chunk=%d)", s.implicit ? "implicit_cg" : "als_cg", s.steps,
			       kAlsCgFormName[als_cg_form(p->K, p->cfg.als_cg_form)], als_cg_chunk(p->K));
		} else {
			const AlsForm &form = kAlsForm[als_form(p->K, p->cfg.als_form)];
			append(buf, buflen, " als_form=%s(chunk=%d)", form.name, form.nch);
			if (s.box_sweeps > 0) append(buf, buflen, " als_box=%d", s.box_sweeps);
		}
	}
	// the environment switches this plan was created under, when any differs from its default (mf_config.hip.h)
	const std::string cfg = p->cfg.describe();
	if (!cfg.empty()) append(buf, buflen, " config{%s}", cfg.c_str());
	return MF_OK;
}

}   // extern "C"

/* ---------------------------------------------------------------------------------------- LEVEL 1 */

static int make_single_plan(const mf_problem *pr, int device, mf_plan **out, const double *weight = nullptr)
{
	if (!pr || pr->users < 0 || pr->items < 0 || pr->features < 1 || pr->nnz < 0 || pr->iters < 0 ||
	    (pr->nnz > 0 && !pr->entries))
		return MF_ERR_ARGUMENT;
	const mf_shard s = whole_shard(pr->users, pr->items, pr->features, pr->nnz, pr->alpha, device);
	return plan_create_impl(out, &s, pr->entries, false, weight);
}

// The level-1 sequence: a plan over the whole problem, the factors up, `work(plan)`, the plan destroyed.  Every entry
// point checks its own arguments first.
template <class Work>
static int with_single_plan(const mf_problem *pr, int device, const double *L, const double *R, Work work, const double *weight = nullptr)
{
	mf_plan *p = nullptr;
	int rc = make_single_plan(pr, device, &p, weight);
	if (rc != MF_OK) return rc;
	rc = mf_plan_upload_factors(p, L, R);
	if (rc == MF_OK) rc = work(p);
	mf_plan_destroy(p);
	return rc;
}

// a level-1 bounds record: NULL (no bounds) or a box that mf_plan_set_bounds would take at this K
static bool bounds_record_ok(const mf_bounds *b, int K) { return !b || (bounds_ok(b->lo, b->hi, b->columns) && b->columns <= K); }

// the update rules of a level-1 run, [0] = items, [1] = users: what the entry point was given, the defaults for the rest
using RulePair = std::array<SideRule, 2>;
static RulePair level1_rules(double lambda_users, double lambda_items, double beta_users = 0.0, double beta_items = 0.0,
                             const mf_bounds *bounds_users = nullptr, const mf_bounds *bounds_items = nullptr)
{
	RulePair r;
	r[1].lambda = lambda_users, r[0].lambda = lambda_items;
	r[1].beta = beta_users, r[0].beta = beta_items;
	if (bounds_users) r[1].lo = bounds_users->lo, r[1].hi = bounds_users->hi, r[1].columns = bounds_users->columns;
	if (bounds_items) r[0].lo = bounds_items->lo, r[0].hi = bounds_items->hi, r[0].columns = bounds_items->columns;
	return r;
}

// The level-1 run: a plan over the whole problem (weighted when `weight` is given), the factors up, the update rules the
// entry point checked, `setup(plan)` where the entry point has more to set (the ALS runs: their solver), pr->iters
// iterations, the recommendations when asked for, the factors back into L and R.
using PlanSetup = std::function<int(mf_plan *)>;
static int run_single_plan(const mf_problem *pr, const double *weight, const RulePair &rule, double *L, double *R, int32_t *best, int device,
                           const PlanSetup &setup = nullptr)
{
	return with_single_plan(pr, device, L, R, [&](mf_plan *p) {
		p->rule[0] = rule[0], p->rule[1] = rule[1];   // both sides at rest, as the upload left them
		int rc = setup ? setup(p) : MF_OK;
		if (rc == MF_OK) rc = mf_plan_iterate(p, pr->iters);
		if (rc == MF_OK && best) rc = mf_plan_recommend(p, best);
		if (rc == MF_OK) rc = mf_plan_download_factors(p, L, R);
		return rc;
	}, weight);
}

// what every mf_backend_run_* checks: the problem, L and R (they carry the initial factors in), its weights, its bounds
static bool run_args_ok(const mf_problem *pr, const double *L, const double *R, std::initializer_list<double> weights = {},
                        const mf_bounds *bounds_users = nullptr, const mf_bounds *bounds_items = nullptr)
{
	return pr && L && R && std::all_of(weights.begin(), weights.end(), lambda_ok) && bounds_record_ok(bounds_users, pr->features) &&
	       bounds_record_ok(bounds_items, pr->features);
}

extern "C" {

int mf_backend_run(const mf_problem *pr, double *L, double *R, int32_t *best, int device)
{
	if (!run_args_ok(pr, L, R)) return MF_ERR_ARGUMENT;
	return run_single_plan(pr, nullptr, RulePair{}, L, R, best, device);
}

int mf_backend_run_reg(const mf_problem *pr, double *L, double *R, int32_t *best, double lambda_users, double lambda_items,
                       int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items})) return MF_ERR_ARGUMENT;
	return run_single_plan(pr, nullptr, level1_rules(lambda_users, lambda_items), L, R, best, device);
}

int mf_backend_run_momentum(const mf_problem *pr, double *L, double *R, int32_t *best, double lambda_users, double lambda_items,
                            double beta_users, double beta_items, int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items, beta_users, beta_items})) return MF_ERR_ARGUMENT;
	return run_single_plan(pr, nullptr, level1_rules(lambda_users, lambda_items, beta_users, beta_items), L, R, best, device);
}

int mf_backend_run_weighted(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                            double lambda_items, double beta_users, double beta_items, int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items, beta_users, beta_items})) return MF_ERR_ARGUMENT;
	return run_single_plan(pr, weight, level1_rules(lambda_users, lambda_items, beta_users, beta_items), L, R, best, device);
}

int mf_backend_run_bounded(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                           double lambda_items, double beta_users, double beta_items, const mf_bounds *bounds_users,
                           const mf_bounds *bounds_items, int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items, beta_users, beta_items}, bounds_users, bounds_items)) return MF_ERR_ARGUMENT;
	return run_single_plan(pr, weight, level1_rules(lambda_users, lambda_items, beta_users, beta_items, bounds_users, bounds_items), L, R,
	                       best, device);
}

// the plain rule's betas are absent: a side cannot have momentum and an adaptive kind
int mf_backend_run_adaptive(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                            double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items,
                            const mf_adaptive *adaptive_users, const mf_adaptive *adaptive_items, int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items}, bounds_users, bounds_items) || !adaptive_ok(adaptive_users) || !adaptive_ok(adaptive_items))
		return MF_ERR_ARGUMENT;
	RulePair rule = level1_rules(lambda_users, lambda_items, 0.0, 0.0, bounds_users, bounds_items);
	rule[1].opt = adaptive_rule(adaptive_users), rule[0].opt = adaptive_rule(adaptive_items);
	return run_single_plan(pr, weight, rule, L, R, best, device);
}

// ---- biases on frozen columns: a ~ mu + b_user + b_item + l.r as the K = F + 2 product of
//   L' = [ L | b_user | 1.0 ] (users' column F+1 frozen)  and  R' = [ R | 1.0 | b_item ] (items' column F frozen)
// the ALS run: the gradient rule's alpha, betas and adaptive kinds have no part in it
int mf_backend_run_als(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                       double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, int kind, int device)
{
	return mf_backend_run_als_cg(pr, weight, L, R, best, lambda_users, lambda_items, bounds_users, bounds_items, kind, 0, device);
}

// ... with the steps of the conjugate-gradient solve (0: the direct one), set before the kind: K may lie in 129 .. 256
int mf_backend_run_als_cg(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                          double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, int kind, int steps,
                          int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items}, bounds_users, bounds_items) || !als_kind_ok(kind) || steps < 0 || steps > MF_ALS_CG_MAX_STEPS)
		return MF_ERR_ARGUMENT;
	const RulePair rule = level1_rules(lambda_users, lambda_items, 0.0, 0.0, bounds_users, bounds_items);
	return run_single_plan(pr, weight, rule, L, R, best, device, [&](mf_plan *p) {
		const int rc = mf_plan_set_als_cg(p, steps);
		return rc == MF_OK ? mf_plan_set_als(p, kind) : rc;
	});
}

// the implicit-feedback run: mf_backend_run_als with the implicit kind and its confidence
int mf_backend_run_implicit(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                            double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, double conf, int device)
{
	return mf_backend_run_implicit_cg(pr, weight, L, R, best, lambda_users, lambda_items, bounds_users, bounds_items, conf, 0, device);
}

// ... with the steps of its conjugate-gradient solve (0: the direct one)
int mf_backend_run_implicit_cg(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                               double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, double conf, int steps,
                               int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items}, bounds_users, bounds_items) || !std::isfinite(conf) || conf < 0.0 || steps < 0 ||
	    steps > MF_ALS_CG_MAX_STEPS)
		return MF_ERR_ARGUMENT;
	const RulePair rule = level1_rules(lambda_users, lambda_items, 0.0, 0.0, bounds_users, bounds_items);
	return run_single_plan(pr, weight, rule, L, R, best, device, [&](mf_plan *p) {
		int rc = mf_plan_set_confidence(p, conf);
		if (rc == MF_OK) rc = mf_plan_set_implicit_cg(p, steps);
		return rc == MF_OK ? mf_plan_set_als(p, MF_ALS_IMPLICIT) : rc;
	});
}

// the ALS run of any kind with the box-constrained row solve (0 sweeps: the direct one); conf counts under the implicit kind
int mf_backend_run_als_box(const mf_problem *pr, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                           double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, int kind, double conf,
                           int sweeps, int device)
{
	const bool implicit = kind == MF_ALS_IMPLICIT;
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items}, bounds_users, bounds_items) || !(als_kind_ok(kind) || implicit) || sweeps < 0 ||
	    sweeps > MF_ALS_BOX_MAX_SWEEPS || (implicit && (!std::isfinite(conf) || conf < 0.0)))
		return MF_ERR_ARGUMENT;
	const RulePair rule = level1_rules(lambda_users, lambda_items, 0.0, 0.0, bounds_users, bounds_items);
	return run_single_plan(pr, weight, rule, L, R, best, device, [&](mf_plan *p) {
		int rc = implicit ? mf_plan_set_confidence(p, conf) : MF_OK;
		if (rc == MF_OK) rc = mf_plan_set_als_box(p, sweeps);
		return rc == MF_OK ? mf_plan_set_als(p, kind) : rc;
	});
}

int mf_backend_bias_mean(const double *val, int64_t n, double *mu)
{
	if (!mu || n < 0 || (n > 0 && !val)) return MF_ERR_ARGUMENT;
	double s = 0.0;
	for (int64_t i = 0; i < n; ++i) s = s + val[i];
	*mu = n > 0 ? s / (double) n : 0.0;
	return MF_OK;
}

int mf_backend_bias_pack(const double *X, const double *bias, int32_t rows, int32_t F, int side, double *out)
{
	if (rows < 0 || F < 1 || (side != 0 && side != 1) || (rows > 0 && (!X || !out))) return MF_ERR_ARGUMENT;
	const size_t K = (size_t) F + 2;
	for (int32_t r = 0; r < rows; ++r) {
		double *o = out + (size_t) r * K;
		for (int32_t k = 0; k < F; ++k) o[k] = X[(size_t) r * F + k];
		const double b = bias ? bias[r] : 0.0;
		o[F] = side == 1 ? b : 1.0;
		o[F + 1] = side == 1 ? 1.0 : b;
	}
	return MF_OK;
}

int mf_backend_bias_unpack(const double *in, int32_t rows, int32_t F, int side, double *X, double *bias)
{
	if (rows < 0 || F < 1 || (side != 0 && side != 1) || (rows > 0 && !in)) return MF_ERR_ARGUMENT;
	const size_t K = (size_t) F + 2;
	for (int32_t r = 0; r < rows; ++r) {
		const double *i = in + (size_t) r * K;
		if (X)
			for (int32_t k = 0; k < F; ++k) X[(size_t) r * F + k] = i[k];
		if (bias) bias[r] = i[side == 1 ? F : F + 1];
	}
	return MF_OK;
}

int mf_backend_run_biased(const mf_problem *pr, double *L, double *R, double *user_bias, double *item_bias, double *mu,
                          int32_t *best, double lambda_users, double lambda_items, int device)
{
	if (!run_args_ok(pr, L, R, {lambda_users, lambda_items}) || !user_bias || !item_bias || !mu || pr->users < 0 || pr->items < 0 ||
	    pr->features < 1 || pr->nnz < 0 || pr->iters < 0 || (pr->nnz > 0 && !pr->entries))
		return MF_ERR_ARGUMENT;
	if (pr->features > kLargestK - 2) return MF_ERR_UNSUPPORTED;
	const int32_t F = pr->features, K = F + 2;
	// mu in the entries' order, then every value centred with one rounding
	std::vector<mf_entry> ent((size_t) pr->nnz);
	{
		std::vector<double> v((size_t) pr->nnz);
		for (int64_t n = 0; n < pr->nnz; ++n) v[(size_t) n] = pr->entries[n].value;
		(void) mf_backend_bias_mean(v.data(), pr->nnz, mu);
		for (int64_t n = 0; n < pr->nnz; ++n) {
			ent[(size_t) n] = pr->entries[n];
			ent[(size_t) n].value = v[(size_t) n] - *mu;
		}
	}
	std::vector<double> Lp((size_t) pr->users * K), Rp((size_t) pr->items * K);
	(void) mf_backend_bias_pack(L, user_bias, pr->users, F, 1, Lp.data());
	(void) mf_backend_bias_pack(R, item_bias, pr->items, F, 0, Rp.data());
	mf_problem q = *pr;
	q.features = K;
	q.entries = ent.data();
	RulePair rule = level1_rules(lambda_users, lambda_items);
	rule[1].frozen = F + 1, rule[0].frozen = F;
	const int rc = run_single_plan(&q, nullptr, rule, Lp.data(), Rp.data(), best, device);
	if (rc != MF_OK) return rc;
	(void) mf_backend_bias_unpack(Lp.data(), pr->users, F, 1, L, user_bias);
	(void) mf_backend_bias_unpack(Rp.data(), pr->items, F, 0, R, item_bias);
	return MF_OK;
}

int mf_backend_run_top1(const mf_problem *pr, const double *L0, const double *R0, int32_t *best, int device)
{
	if (!pr || !L0 || !R0 || (!best && pr->users > 0)) return MF_ERR_ARGUMENT;
	return with_single_plan(pr, device, L0, R0, [&](mf_plan *p) {
		const int rc = mf_plan_iterate(p, pr->iters);
		return rc == MF_OK ? mf_plan_recommend(p, best) : rc;
	});
}

int mf_backend_run_topn(const mf_problem *pr, const double *L0, const double *R0, int32_t n, int32_t *items, double *scores,
                        int device)
{
	if (!pr || !L0 || !R0 || n < 1 || !items) return MF_ERR_ARGUMENT;
	if (n > MF_TOPN_MAX) return MF_ERR_UNSUPPORTED;
	return with_single_plan(pr, device, L0, R0, [&](mf_plan *p) {
		const int rc = mf_plan_iterate(p, pr->iters);
		return rc == MF_OK ? mf_plan_recommend_topn(p, n, items, scores) : rc;
	});
}

int mf_backend_recommend_topn(const mf_problem *pr, const double *L, const double *R, int32_t n, int32_t *items,
                              double *scores, int device)
{
	if (!pr || !L || !R || n < 1 || !items) return MF_ERR_ARGUMENT;
	if (n > MF_TOPN_MAX) return MF_ERR_UNSUPPORTED;
	return with_single_plan(pr, device, L, R, [&](mf_plan *p) { return mf_plan_recommend_topn(p, n, items, scores); });
}

int mf_backend_similar_items(const double *R, int32_t items, int32_t features, int metric, const int32_t *query, int32_t nq,
                             int32_t n, int32_t *out_items, double *out_scores, int device)
{
	if (items < 0 || features < 1 || (!R && items > 0)) return MF_ERR_ARGUMENT;
	const int chk = similar_check(items, metric, query, nq, n, out_items);
	if (chk != MF_OK) return chk;
	// a throw-away plan of one user without entries: the query reads nothing of it but R
	const mf_shard s = whole_shard(1, items, features, 0, 0.0, device);
	mf_plan *p = nullptr;
	int rc = mf_plan_create(&p, &s);
	if (rc != MF_OK) return rc;
	const std::vector<double> l0((size_t) features, 0.0);
	rc = mf_plan_upload_factors(p, l0.data(), R);
	if (rc == MF_OK) rc = mf_plan_similar_items(p, metric, query, nq, n, out_items, out_scores);
	mf_plan_destroy(p);
	return rc;
}

}   // extern "C"

static double loss_rmse(const mf_loss &l) { return l.count > 0 ? std::sqrt(l.sse / (double) l.count) : std::nan(""); }

extern "C" {

int mf_backend_loss_total(const double *row_sse, int32_t user_begin, int32_t users, double *sse)
{
	if (!sse || user_begin < 0 || users < 0 || (users > 0 && !row_sse)) return MF_ERR_ARGUMENT;
	double total = 0.0;
	int64_t i = 0;
	while (i < users) {   // blocks are cut at global multiples of MF_LOSS_BLOCK
		const int64_t stop = std::min<int64_t>(users, (((int64_t) user_begin + i) / MF_LOSS_BLOCK + 1) * MF_LOSS_BLOCK - user_begin);
		double t = 0.0;
		for (; i < stop; ++i) t = t + row_sse[i];
		total = total + t;
	}
	*sse = total;
	return MF_OK;
}

int mf_plan_set_heldout(mf_plan *p, int64_t n, const int32_t *row, const int32_t *col, const double *val)
{
	if (!p || n < 0 || n > INT32_MAX - 64 || (n > 0 && (!row || !col || !val))) return MF_ERR_ARGUMENT;
	for (int64_t i = 0; i < n; ++i)
		if (row[i] < p->u0 || row[i] >= p->u0 + p->uc || col[i] < 0 || col[i] >= p->items) return MF_ERR_ARGUMENT;
	MF_HIP(hipSetDevice(p->device));
	dev_buf<int> nptr, nidx, nuser;
	dev_buf<double> nval;
	std::vector<int> pos;   // bucketed position of the caller's entry n (mf_plan_rank_heldout reports in the caller's order)
	if (n > 0) {
		// stable counting sort by user on the host: the caller's order inside a user is the order of the row sum
		std::vector<int> ptr, idx, user;
		std::vector<double> v;
		try {
			bucket(n, p->uc, row, p->u0, col, 0, val, ptr, idx, v, &pos);
			user.resize((size_t) n);
			for (int u = 0; u < p->uc; ++u) std::fill(user.begin() + ptr[(size_t) u], user.begin() + ptr[(size_t) u + 1], u);
		} catch (const std::bad_alloc &) {
			return MF_ERR_NO_MEMORY;
		}
		int rc = nptr.alloc((size_t) p->uc + 1);
		if (rc == MF_OK) rc = nidx.alloc((size_t) n + 64);
		if (rc == MF_OK) rc = nval.alloc((size_t) n + 64);
		if (rc == MF_OK) rc = nuser.alloc((size_t) n);
		if (rc != MF_OK) return rc;
		hipError_t e = h2d(p, nptr, ptr.data(), ptr.size() * sizeof(int));
		if (e == hipSuccess) e = h2d(p, nidx, idx.data(), idx.size() * sizeof(int));
		if (e == hipSuccess) e = h2d(p, nval, v.data(), v.size() * sizeof(double));
		if (e == hipSuccess) e = h2d(p, nuser, user.data(), user.size() * sizeof(int));
		if (e != hipSuccess) {
			g_last_hip_error = std::string("mf_plan_set_heldout: ") + hipGetErrorString(e);
			return e == hipErrorOutOfMemory ? MF_ERR_NO_MEMORY : MF_ERR_HIP;
		}
	}
	MF_HIP(hipStreamSynchronize(p->stream));   // no launch still reads the set that is replaced
	p->ho_ptr = std::move(nptr);   // the set that is replaced is freed here
	p->ho_idx = std::move(nidx);
	p->ho_val = std::move(nval);
	p->ho_user = std::move(nuser);
	p->ho_pos.swap(pos);
	p->ho_nnz = n;
	p->have_heldout = n > 0;
	return MF_OK;
}

int mf_plan_loss(mf_plan *p, int which, mf_loss *out, double *row_sse)
{
	if (!p || !out || (which != MF_LOSS_TRAIN && which != MF_LOSS_HELDOUT)) return MF_ERR_ARGUMENT;
	if (!p->have_factors || (which == MF_LOSS_HELDOUT && !p->have_heldout)) return MF_ERR_STATE;
	return loss_eval(p, which, out, row_sse);
}

int mf_plan_rank_heldout(mf_plan *p, int32_t *rank)
{
	if (!p || !rank) return MF_ERR_ARGUMENT;
	if (!p->have_factors || !p->have_heldout) return MF_ERR_STATE;
	const int rc = launch_rank(p);
	if (rc != MF_OK) return rc;
	const size_t n = (size_t) p->ho_nnz;
	std::vector<int> bucketed;
	try {
		bucketed.resize(n);
	} catch (const std::bad_alloc &) {
		return MF_ERR_NO_MEMORY;
	}
	MF_HIP(hipMemcpyAsync(bucketed.data(), p->rank_out, n * sizeof(int), hipMemcpyDeviceToHost, p->stream));
	MF_HIP(hipStreamSynchronize(p->stream));
	for (size_t i = 0; i < n; ++i) rank[i] = bucketed[(size_t) p->ho_pos[i]];
	return MF_OK;
}

int mf_plan_rank_heldout_info(mf_plan *p, int64_t *exact_pass_entries, int32_t *mfma_form)
{
	if (!p) return MF_ERR_ARGUMENT;
	if (exact_pass_entries) *exact_pass_entries = p->last_rank_uncertain;
	if (mfma_form) *mfma_form = p->rank_form;
	return MF_OK;
}

int mf_backend_rank_metrics(const int32_t *rank, const int32_t *row, int64_t n, int32_t cutoff, mf_rank_metrics *out)
{
	if (!out || n < 0 || cutoff < 1 || (n > 0 && (!rank || !row))) return MF_ERR_ARGUMENT;
	for (int64_t i = 0; i < n; ++i)
		if (rank[i] < MF_RANK_NAN || row[i] < 0) return MF_ERR_ARGUMENT;
	mf_rank_metrics m;
	memset(&m, 0, sizeof m);
	double rr = 0.0;
	std::map<int32_t, std::pair<int64_t, double>> per_user;   // user -> (evaluated entries, DCG), ascending user id
	try {
		for (int64_t i = 0; i < n; ++i) {
			const int32_t r = rank[i];
			if (r == MF_RANK_MASKED) {
				++m.masked;
			} else if (r == MF_RANK_NAN) {
				++m.nan;
			} else {
				++m.evaluated;
				rr = rr + 1.0 / (double) ((int64_t) r + 1);
				std::pair<int64_t, double> &u = per_user[row[i]];
				++u.first;
				if (r < cutoff) {
					++m.hits;
					u.second = u.second + 1.0 / std::log2((double) ((int64_t) r + 2));
				}
			}
		}
	} catch (const std::bad_alloc &) {
		return MF_ERR_NO_MEMORY;
	}
	m.users = (int64_t) per_user.size();
	if (m.evaluated == 0) {
		m.hit_rate = m.mrr = m.ndcg = std::nan("");
	} else {
		m.hit_rate = (double) m.hits / (double) m.evaluated;
		m.mrr = rr / (double) m.evaluated;
		// the ideal DCG depends on min(h, cutoff) only: a running prefix sum serves every user
		std::vector<double> ideal(1, 0.0);
		double total = 0.0;
		for (const auto &kv : per_user) {
			const int64_t h = std::min<int64_t>(kv.second.first, cutoff);
			while ((int64_t) ideal.size() <= h) ideal.push_back(ideal.back() + 1.0 / std::log2((double) (ideal.size() + 1)));
			total = total + kv.second.second / ideal[(size_t) h];
		}
		m.ndcg = total / (double) m.users;
	}
	*out = m;
	return MF_OK;
}

int mf_plan_iterate_monitored(mf_plan *p, int iters, int every, double tol, mf_loss_point *trace, int cap, int *points,
                              int *iters_done)
{
	if (!p || iters < 0 || every < 1 || cap < 0 || (cap > 0 && !trace)) return MF_ERR_ARGUMENT;
	if (!p->have_factors) return MF_ERR_STATE;
	if (iters > 0 && (implicit_refuses(p, 0) || implicit_refuses(p, 1))) return MF_ERR_UNSUPPORTED;   // before any HIP call
	int done = 0, npoints = 0;
	double prev = 0.0;
	for (;;) {
		mf_loss_point pt;
		memset(&pt, 0, sizeof pt);
		pt.iter = done;
		int rc = loss_eval(p, MF_LOSS_TRAIN, &pt.train, nullptr);
		if (rc == MF_OK && p->have_heldout) rc = loss_eval(p, MF_LOSS_HELDOUT, &pt.heldout, nullptr);
		if (rc != MF_OK) return rc;
		if (npoints < cap) trace[npoints] = pt;
		++npoints;
		const double rmse = loss_rmse(p->have_heldout ? pt.heldout : pt.train);
		// the stopping rule (tol > 0 only): a NaN stops; from the second point on, an improvement of at most tol * previous
		bool stop = done >= iters;
		if (tol > 0.0 && (std::isnan(rmse) || (npoints > 1 && prev - rmse <= tol * prev))) stop = true;
		prev = rmse;
		if (stop) break;
		const int step = std::min(every, iters - done);
		rc = mf_plan_iterate(p, step);
		if (rc != MF_OK) return rc;
		done += step;
	}
	if (points) *points = npoints;
	if (iters_done) *iters_done = done;
	return MF_OK;
}

int mf_backend_loss(const mf_problem *pr, const double *L, const double *R, mf_loss *out, double *row_sse, int device)
{
	if (!pr || !L || !R || !out) return MF_ERR_ARGUMENT;
	return with_single_plan(pr, device, L, R, [&](mf_plan *p) { return mf_plan_loss(p, MF_LOSS_TRAIN, out, row_sse); });
}

int mf_backend_factorize(const mf_problem *pr, double *L, double *R, int device)
{
	return mf_backend_run(pr, L, R, nullptr, device);
}

int mf_backend_recommend(const mf_problem *pr, const double *L, const double *R, int32_t *best, int device)
{
	if (!pr || !L || !R || (!best && pr->users > 0)) return MF_ERR_ARGUMENT;
	return with_single_plan(pr, device, L, R, [&](mf_plan *p) { return mf_plan_recommend(p, best); });
}

#ifdef MF_STAMPS
// diagnostic build only: read and clear the phase clocks of sweep_dma_kernel (tools/stamps.py)
int mf_debug_read_stamps(unsigned long long *out8)
{
	unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	MF_HIP(hipDeviceSynchronize());
	MF_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(mf::mf_stamp_buf), sizeof zero));
	MF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mf::mf_stamp_buf), zero, sizeof zero));
	return MF_OK;
}

// per-wave clocks of the streams launch of the errors + streams iteration (tools/es_stamps.py)
int mf_debug_read_es_stamps(unsigned long long *out, int words)
{
	MF_HIP(hipDeviceSynchronize());
	MF_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(mf::mf_es_stamp_buf), sizeof(unsigned long long) * (size_t) words));
	return MF_OK;
}

// the same for recommend_mfma_kernel (tools/rec_stamps.py): waves 0 and 7 of workgroup 0
int mf_debug_read_rec_stamps(unsigned long long *out32)
{
	unsigned long long zero[32] = {};
	MF_HIP(hipDeviceSynchronize());
	MF_HIP(hipMemcpyFromSymbol(out32, HIP_SYMBOL(mf::mf_rec_stamp_buf), sizeof zero));
	MF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mf::mf_rec_stamp_buf), zero, sizeof zero));
	return MF_OK;
}
#endif

}  // extern "C"

#include "mf_multi.hip.h"
