// mf_launch.hip.h -- choice of the sweep kernel variant / chunk size, the launch of one sweep, and the loops of mf_plan_iterate.
#pragma once

namespace {

// Slice width (columns) of the LDS-resident streams launch, 0 when a slice of the larger factor does not fit the
// LDS of a CU beside the waves' buffers or K would need more than eight slices (every slice re-reads the records).
int resident_slice_width(const mf_config &cfg, int K, int yrows_max)
{
	if (K & 1) return 0;
	for (int sw : {cfg.es_sw ? cfg.es_sw : 8, 8, 4, 2})   // MF_ES_SW: slice width to try first (A/B)
		if ((sw == 8 || sw == 4 || sw == 2) && (K + sw - 1) / sw <= 8 && (size_t) yrows_max * sw * 8 + mf::kResidentWaves * mf::kResidentWaveLds + 1024 <= kLdsPerCu) return sw;
	return 0;
}

// Row pitch (doubles) of a factor buffer the plan owns: 8K bytes rounded up to whole 128-byte lines when that saves
// at least a tenth of the lines a gathered row touches on average (rows start wherever 8K * r falls: a row of B bytes
// touches B/128 + 1 - gcd(B, 128)/128 lines).  LDS-DMA forms only; MF_ROW_PITCH=0 keeps K (A/B).
int row_pitch(const mf_config &cfg, int K, bool dma)
{
	if (!dma || !cfg.row_pitch) return K;
	const int bytes = 8 * K;
	if (bytes % 128 == 0) return K;
	int g = 128, b = bytes;
	while (b) {
		const int t = g % b;
		g = b;
		b = t;
	}
	const double plain = bytes / 128.0 + 1.0 - g / 128.0, padded = (bytes + 127) / 128;
	return plain >= 1.1 * padded ? ((bytes + 127) / 128) * 16 : K;
}

// does this K run on an LDS-DMA form of the sweep (even K up to 1024, unless MF_SWEEP_IMPL=reg)?  Mirrors choose_sweep.
bool sweep_is_dma(const mf_config &cfg, int K)
{
	return !cfg.sweep_reg && (K & 1) == 0 && K >= 2 && K <= 128 * 8;
}

// Entries per chunk of a single-wave launch: {nch, nch_few}, or {0, 0} when not even one row fits.  `head` = LDS bytes in
// front of the tile, `row_bytes` = tile row stride.
// Chunk size = latency hiding vs fixed cost.  Each single-wave workgroup alternates "gather a chunk"
// and "compute on it", so the bytes in flight per CU come from OTHER resident workgroups: small tiles
// (~13 KB -> ~11 workgroups per CU) beat big ones (measured on cfg4, K=100: nch 64/32/16/8 ->
// 37.1/29.3/24.1/25.5 ms per iteration); phase A costs K steps per chunk whatever its size, which is
// what stops the trend below ~12 entries.
// K=256: nch 8/12/16/24 -> 71/66/78/82 ms (12 rows = 6 workgroups per CU); K=30: nch 16..32 best.
// nch_few: a sweep over FEW rows (ML100k: 943 x 1682) cannot fill 256 CUs whatever the chunk size; its time is the
// longest row's serial chain of chunks, so use the largest chunk there (737 entries: 47 -> 12 chunks).
// MF_SWEEP_NCH sets both.
struct ChunkSizes {
	int nch, nch_few;
};
// "Few rows": the launch cannot fill the chip whatever the chunk size, its time is the longest row's serial chain of
// chunks -> the largest chunk.  Only below ~2048 rows: at 3952 rows (the cfg3 item sweep) the large chunk's LDS
// footprint cost more occupancy than it saved (item sweep 0.189 -> 0.123 ms with the ordinary chunk).  The sweeps
// (launch_sweep) and the loss (launch_loss) share the bound.
constexpr int kSweepFewRows = 2048;
ChunkSizes chunk_rule(size_t head, size_t row_bytes, const mf_config &cfg)
{
	auto fit = [&](size_t budget) {
		return budget > head ? (int) std::min<size_t>(64, (budget - head) / row_bytes) : 0;
	};
	int nch = 16;
	if (head + (size_t) nch * row_bytes > kLdsPerCu / 6) nch = std::max(12, fit(kLdsPerCu / 6));
	nch = std::min(nch, fit(kLdsPerCu));
	if (const int v = cfg.sweep_nch; v >= 1 && head + (size_t) v * row_bytes <= kLdsPerCu) nch = v;
	if (nch < 1) return {0, 0};
	int few = std::max(nch, std::min(64, fit(kLdsPerCu / 2)));
	if (cfg.sweep_nch) few = nch;
	return {nch, few};
}

// LDS tile row stride and the bytes in front of the tile, for the form choose_sweep picked
size_t tile_row_bytes(const mf_plan *p) { return p->sweep.dma ? (size_t) p->sweep.row_bytes : (size_t) p->stride * sizeof(double); }
size_t tile_head_bytes(const mf_plan *p) { return p->sweep.dma ? (size_t) p->sweep.xs_bytes : 0; }

// What a side's update reads and writes: side 0 (items) has X = R, Y = L and walks the CSC; side 1 (users) has X = L,
// Y = R and walks the CSR.  X_new is the next generation of X.
struct SideOperands {
	const int *ptr, *idx;
	const double *val;
	const double *wgt;          // the entries' weights in the order of (idx, val); null on an unweighted plan
	const mf::StreamRec *rec;   // the side's {idx, e_n} records (errors + streams iteration)
	const double *X_old, *Y_old;
	double *X_new;
	int ldx, ldy;   // row pitch of X and of Y in doubles
	int yrows;      // rows of Y
};
SideOperands side_operands(const mf_plan *p, int kind)
{
	const int cur = p->cur, nxt = p->cur ^ 1;
	if (kind == 0)
		return {p->csc_ptr, p->csc_idx, p->csc_val, p->csc_wgt, p->rec_csc, p->Rbuf[cur], p->Lbuf[cur], p->Rbuf[nxt], p->ldr, p->ldl, p->uc};
	return {p->csr_ptr, p->csr_idx, p->csr_val, p->csr_wgt, p->rec_csr, p->Lbuf[cur], p->Rbuf[cur], p->Lbuf[nxt], p->ldl, p->ldr, p->items};
}

// the ordered-sum kernel (MF_OS_DPP) and the resident streams kernel of a slice width
const void *ordered_sum_fn(const mf_config &cfg)
{
	return cfg.os_dpp ? (const void *) mf::ordered_sum_kernel<true> : (const void *) mf::ordered_sum_kernel<false>;
}
const void *stream_resident_fn(int sw, bool momentum = false)
{
	return (const void *) kStreamResidentFn[sw == 8 ? 0 : sw == 4 ? 1 : 2][momentum];
}

// Raises the LDS limit of every instance of one form that this plan may launch: the non-null cells of the form's row of
// the grid -- the unweighted flavours, and on a weighted plan the weighted ones too (an unweighted plan touches none of
// them).  Called once per form, where the form's geometry is decided.
int raise_form_limits(const mf_plan *p, Form form, size_t bytes)
{
	const int flavours = p->weighted ? (int) kFlavours : mf_sched::kUnweightedFlavours;
	for (int fl = 0; fl < flavours; ++fl)
		if (const SweepFn fn = p->sweep.fn[form][fl]) MF_HIP(raise_lds_limit((const void *) fn, bytes));
	return MF_OK;
}

int choose_sweep(mf_plan *p)
{
	const int K = p->K;
	p->sweep = SweepVariant{};
	const bool allow_dma = !p->cfg.sweep_reg;   // MF_SWEEP_IMPL=dma (default) | reg: register-staged form only
	if (allow_dma)
		for (const auto &v : kDma)
			if (v.kt == K) p->sweep = v;
	if (!p->sweep.has(kPlain) && allow_dma && (K & 1) == 0)
		for (const auto &v : kDmaGeneric)
			if (K <= 128 * v.kpmax && !p->sweep.has(kPlain)) {
				p->sweep = v;
				p->sweep.row_bytes = mf::dma_row_stride(K);
				p->sweep.xs_bytes = mf::dma_xs_bytes(K);
			}
	if (!p->sweep.has(kPlain))
		for (const auto &v : kSpecialised)
			if (v.kt == K) p->sweep = v;
	if (!p->sweep.has(kPlain))
		for (const auto &v : kGeneric)
			if (K <= v.kpmax * mf::kWave) {
				p->sweep = v;
				break;
			}
	if (!p->sweep.has(kPlain)) return MF_ERR_UNSUPPORTED;

	p->stride = mf::reg_row_stride(K);
	const size_t row_bytes = tile_row_bytes(p), head = tile_head_bytes(p);
	const ChunkSizes cs = chunk_rule(head, row_bytes, p->cfg);
	if (cs.nch < 1) return MF_ERR_UNSUPPORTED;
	p->single = LaunchGeometry{cs.nch, head + (size_t) cs.nch * row_bytes, mf::kWave};
	p->few = LaunchGeometry{cs.nch_few, head + (size_t) cs.nch_few * row_bytes, mf::kWave};
	MF_TRY(raise_form_limits(p, kPlain, std::max(p->single.lds, p->few.lds)));
	MF_TRY(raise_form_limits(p, kPipelined, std::max(p->single.lds, p->few.lds)));
	// the two-tile forms: `dflt` entries per chunk (MF_SWEEP_NCH overrides) while two tiles stay within half a CU's LDS
	auto two_tiles = [&](int dflt, int block) {
		int n = p->cfg.sweep_nch ? p->cfg.sweep_nch : dflt;
		while (n > 1 && head + 2 * (size_t) n * row_bytes > kLdsPerCu / 2) --n;
		return LaunchGeometry{n, head + 2 * (size_t) n * row_bytes, block};
	};
	if (p->sweep.has(kPair)) {   // wave-pair form
		// 32-entry chunks: the loader's ~90 cycles per gathered row are what a pair is bound by, the K steps of phase A are
		// paid per chunk -- a lone 5993-entry row: 0.526 ms at 16, 0.332 at 32; cfg3 power-law 0.311 / 0.268 / 0.314 at 24 / 32 / 40
		p->pair = two_tiles(32, 2 * mf::kWave);
		MF_TRY(raise_form_limits(p, kPair, p->pair.lds));
	}
	if (p->sweep.has(kDb)) {   // double-buffered form (few rows per CU: the wave hides its own gather)
		p->db = two_tiles(16, mf::kWave);
		MF_TRY(raise_form_limits(p, kDb, p->db.lds));
	}
	// ---- errors + streams iteration (mf_stream.hip.h) for instances whose factors stay in L2 / Infinity Cache: the
	// two sweeps are then bound by the latency of one wave walking a row chunk by chunk, not by bandwidth.  It costs a
	// third gather of every entry's row, so it is only chosen while the factors are cache-resident; MF_ITER_MODE=es |
	// sweeps overrides.
	p->want_map = false;
	p->res_sw = resident_slice_width(p->cfg, K, std::max(p->uc, p->items));
	if (p->sweep.errs[0] && p->nnz > 0) {
		// Used where the streams launch can keep a slice of Y resident in LDS (mf_resident.hip.h; instML100k 84 -> 39 us
		// per iteration); MF_ITER_MODE=sweeps keeps the two sweeps, =es asks for it explicitly (same condition).
		// Not below a few thousand entries: there two graph-replayed single-wave sweeps are quicker than a launch that
		// first copies a slice of Y into every CU's LDS (inst30-40, 170 entries: 17 vs 20 us per iteration).
		const bool forced = p->cfg.iter_mode == mf_config::kIterEs;
		p->want_map = p->res_sw > 0 && p->cfg.iter_mode != mf_config::kIterSweeps && (forced || p->nnz >= 4096);
	}
	return MF_OK;
}

// Row-sum kernel of mf_plan_loss for this plan's K (the geometry choose_sweep picked) and its chunk sizes.  One tile and
// no second buffer: the request is the L row plus nch gathered rows, at the sweeps' chunk rule (chunk_rule).
int choose_loss(mf_plan *p)
{
	const size_t row_bytes = tile_row_bytes(p), head = tile_head_bytes(p);
	const ChunkSizes cs = chunk_rule(head, row_bytes, p->cfg);
	if (cs.nch < 1) return MF_ERR_UNSUPPORTED;
	p->loss_nch[0] = cs.nch;
	p->loss_nch[1] = cs.nch_few;
	p->loss_lds[0] = head + (size_t) cs.nch * row_bytes;
	p->loss_lds[1] = head + (size_t) cs.nch_few * row_bytes;
	const LossFn reg[2] = {mf::loss_reg_kernel, mf::loss_reg_w_kernel};
	// [1], the training loss of a weighted plan: the weighted twin in the same geometry, on weighted plans only
	for (int w = 0; w <= (int) p->weighted; ++w) {
		p->loss_fn[w] = p->sweep.dma ? p->sweep.loss[w] : reg[w];
		if (!p->loss_fn[w]) return MF_ERR_UNSUPPORTED;
		MF_HIP(raise_lds_limit((const void *) p->loss_fn[w], std::max(p->loss_lds[0], p->loss_lds[1])));
	}
	return MF_OK;
}

// Accumulate form of a side's single-wave launch, pipelined or plain (mf_schedule.h): main_form's and mf_plan_describe's.
bool single_wave_pipelined(const mf_plan *p, int kind)
{
	return mf_sched::single_wave_pipelined(p->sweep.has(kPipelined), p->K, p->side[kind].n_short, p->side[kind].nrows);
}

// The resume instance the band launches of the user sweep run: that of its single-wave form, null where the K has none
SweepFn band_resume_fn(const mf_plan *p) { return p->sweep.resume[single_wave_pipelined(p, 1) ? 1 : 0]; }

// The main launch of one side (kind 0: items, 1: users) by the rules of mf_schedule.h: its form, that form's geometry and
// the instance of `flavour`.  A cell the K does not have leaves fn null: launch_sweep refuses rather than run another.
SweepForm main_form(const mf_plan *p, int kind, bool few_rows, Flavour flavour)
{
	const SweepSide &sd = p->side[kind];
	const Form form = mf_sched::launch_form(sd.coop_all, sd.use_db, sd.use_pair, single_wave_pipelined(p, kind));
	LaunchGeometry lg = p->coop;
	switch (mf_sched::launch_geometry(form, few_rows)) {
	case mf_sched::kGeomSingle: lg = p->single; break;
	case mf_sched::kGeomFew: lg = p->few; break;
	case mf_sched::kGeomPair: lg = p->pair; break;
	case mf_sched::kGeomDb: lg = p->db; break;
	case mf_sched::kGeomCoop: break;
	case mf_sched::kGeomCoopSingleNch: lg.nch = p->single.nch; break;
	}
	return SweepForm{lg, p->sweep.fn[form][flavour]};
}

// The update rule of one launch of a side (kind 0: items, 1: users), from the side's record.  Read at every launch (a
// captured graph is built per call), so a change holds from the next sweep on.
//   d: weight decay of the seed, 1.0 - (alpha * 2) * lambda, two roundings in double -- the product, then the subtraction;
//      lambda = 0 is 1.0 whatever alpha is (a non-finite alpha times 0 would be NaN), and x * 1.0 is x bit for bit.
//   beta: the side's heavy-ball momentum for a seeded sweep, 0.0 -- no term -- for an unseeded one.
//   box.columns: how many leading columns of a finished row are projected onto [lo, hi] -- the side's (-1: all K) for a
//      seeded sweep of a side with a finite bound, 0 for an unseeded one (a partial sum is not clamped) and for a side whose
//      bounds are both infinite (the clamp would change no bit).
struct SideUpdate {
	double d, beta;
	int frozen;
	mf::Box box;
};
SideUpdate side_update(const mf_plan *p, int kind, int seed)
{
	const SideRule &r = p->rule[kind];
	SideUpdate u{1.0, seed ? r.beta : 0.0, r.frozen, mf::Box{r.lo, r.hi, 0}};
	if (r.lambda != 0.0) {
		const double t = (p->alpha * 2) * r.lambda;
		u.d = 1.0 - t;
	}
	if (seed && !(r.lo == -INFINITY && r.hi == INFINITY)) u.box.columns = r.columns < 0 ? p->K : r.columns;
	return u;
}

// A side at rest that is about to run a seeded momentum sweep: X_prev = X_old by definition, literally -- one device copy
// current -> next over rows x pitch on the plan's stream, and the side has a history.  mf_plan_iterate calls it before it
// captures or launches anything, so no graph and no kernel sees a special first step.
int leave_rest(mf_plan *p, int kind)
{
	if (!p->rule[kind].at_rest || p->rule[kind].beta == 0.0) return MF_OK;
	const int rows = kind == 0 ? p->items : p->uc, ld = kind == 0 ? p->ldr : p->ldl;
	double *const *buf = kind == 0 ? p->Rbuf : p->Lbuf;
	if (rows > 0)
		MF_HIP(hipMemcpyAsync(buf[p->cur ^ 1], buf[p->cur], (size_t) rows * ld * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
	p->rule[kind].at_rest = false;
	return MF_OK;
}

// ---- adaptive sides (mf_adaptive.hip.h): a seeded sweep is the unseeded one, a tick of the side's step record in front of
// it and the finishing kernel behind it.
bool adaptive_side(const mf_plan *p, int kind) { return p->rule[kind].opt.kind != MF_OPT_NONE; }
bool adaptive_any(const mf_plan *p) { return adaptive_side(p, 0) || adaptive_side(p, 1); }

// elements of a side's accumulators: its rows x its pitch
size_t adaptive_elements(const mf_plan *p, int kind) { return kind == 0 ? (size_t) p->items * p->ldr : (size_t) p->uc * p->ldl; }

// puts the side's step record at (p1, p2, steps), on the plan's stream
int adaptive_set_record(mf_plan *p, int kind, double p1, double p2, long long steps)
{
	hipLaunchKernelGGL(mf::adaptive_set_kernel, dim3(1), dim3(1), 0, p->stream, p->opt[kind].step.get(), p1, p2, steps);
	MF_HIP(hipGetLastError());
	return MF_OK;
}

// The accumulators of an adaptive side exist and, where the side is at rest, say so: v (and ADAM's m) zeroed with
// hipMemsetAsync on the plan's stream, the record at 1.0, 1.0, 0.  mf_plan_iterate calls it before it captures or launches
// anything, so no graph sees an allocation or a special first step; a buffer is only ever new on a side at rest (a change
// of kind puts the side there).
int adaptive_ready(mf_plan *p, int kind)
{
	const mf_adaptive &o = p->rule[kind].opt;
	if (o.kind == MF_OPT_NONE) return MF_OK;
	AdaptiveState &s = p->opt[kind];
	const size_t n = adaptive_elements(p, kind);
	if (!s.step || !s.v || (o.kind == MF_OPT_ADAM && !s.m)) s.rest = true;
	if (!s.step) MF_TRY(s.step.alloc(1));
	if (!s.v) MF_TRY(s.v.alloc(n));
	if (o.kind == MF_OPT_ADAM && !s.m) MF_TRY(s.m.alloc(n));
	if (!s.rest) return MF_OK;
	if (n) MF_HIP(hipMemsetAsync(s.v, 0, n * sizeof(double), p->stream));
	if (n && o.kind == MF_OPT_ADAM) MF_HIP(hipMemsetAsync(s.m, 0, n * sizeof(double), p->stream));
	MF_TRY(adaptive_set_record(p, kind, 1.0, 1.0, 0));
	s.rest = false;
	return MF_OK;
}

// one step of the side's record, on the plan's stream: in front of the sweep's fork, so both streams are behind it
int launch_adaptive_tick(mf_plan *p, int kind)
{
	const mf_adaptive &o = p->rule[kind].opt;
	hipLaunchKernelGGL(mf::adaptive_tick_kernel, dim3(1), dim3(1), 0, p->stream, p->opt[kind].step.get(), o.beta1, o.beta2,
	                   (int) (o.kind == MF_OPT_ADAM));
	MF_HIP(hipGetLastError());
	return MF_OK;
}

// The finish of `nrows` rows of the side (rowlist, or rows 0..nrows when null) on `stream`: X_new holds g.  The decay,
// the frozen column and the box are the seeded sweep's (side_update).
int launch_adaptive_finish(mf_plan *p, int kind, const int *rowlist, int nrows, hipStream_t stream)
{
	if (nrows <= 0) return MF_OK;
	const mf_adaptive &o = p->rule[kind].opt;
	const SideOperands x = side_operands(p, kind);
	const SideUpdate u = side_update(p, kind, 1);
	mf::AdaptiveArgs a;
	a.nrows = nrows;
	a.K = p->K;
	a.ld = x.ldx;
	a.frozen = u.frozen;
	// rows of a workgroup per step: about eight pieces per thread
	const int per = (a.ld & 1) ? a.K : (a.K >> 1) + (a.K & 1);
	a.rows_per_step = std::max(1, std::min(mf::kAdaptiveRows, 8 * mf::kAdaptiveThreads / per));
	a.rowlist = rowlist;
	a.X_old = x.X_old;
	a.X_new = x.X_new;
	a.m = p->opt[kind].m;
	a.v = p->opt[kind].v;
	a.step = p->opt[kind].step;
	a.d = u.d;
	a.eta = o.eta;
	a.eps = o.eps;
	a.beta1 = o.beta1;
	a.beta2 = o.beta2;
	a.ob1 = 1.0 - o.beta1;
	a.ob2 = 1.0 - o.beta2;
	a.box = u.box;
	void (*fn)(mf::AdaptiveArgs) = o.kind == MF_OPT_ADAM      ? mf::adaptive_finish_kernel<MF_OPT_ADAM>
	                               : o.kind == MF_OPT_RMSPROP ? mf::adaptive_finish_kernel<MF_OPT_RMSPROP>
	                                                          : mf::adaptive_finish_kernel<MF_OPT_ADAGRAD>;
	const int grid = std::min((nrows + a.rows_per_step - 1) / a.rows_per_step, 1 << 16);
	hipLaunchKernelGGL(fn, dim3(grid), dim3(mf::kAdaptiveThreads), 0, stream, a);
	MF_HIP(hipGetLastError());
	return MF_OK;
}

// defer_join: leave the ordered sums of the extreme rows running on the side stream when the call returns
// (p->join_pending); the caller joins before anything reads the new generation.
// A seeded sweep of an adaptive side launches exactly what the unseeded one does -- the same form and flavour, box columns
// 0, beta 0 -- with the tick in front and the finish behind: over the short rows (or all rows) on the plan's stream, over
// the extreme rows behind their ordered sum on the side stream, in front of ev_join.
int launch_sweep(mf_plan *p, int kind, int seed, bool defer_join = false)
{
	const SweepSide &sd = p->side[kind];
	p->side[kind].last_unseeded = seed == 0;
	const SideOperands x = side_operands(p, kind);
	const bool adaptive = seed && adaptive_side(p, kind) && sd.nrows > 0;
	if (adaptive) {
		MF_TRY(adaptive_ready(p, kind));
		seed = 0;
	}
	mf::SweepArgs a;
	a.K = p->K;
	a.stride = p->stride;
	a.seed = seed;
	a.prio_len = sd.prio_len;
	a.c2 = p->alpha * 2;
	const SideUpdate u = side_update(p, kind, seed);
	a.d = u.d;
	a.frozen = u.frozen;
	a.beta = u.beta;
	a.box = u.box;
	const bool momentum = u.beta != 0.0;
	if (momentum) MF_TRY(leave_rest(p, kind));
	a.ldx = x.ldx;
	a.ldy = x.ldy;
	a.nrows = sd.nrows;
	a.ptr = x.ptr;
	a.idx = x.idx;
	a.val = x.val;
	a.wgt = x.wgt;
	a.X_old = x.X_old;
	a.Y_old = x.Y_old;
	a.X_new = x.X_new;
	a.rowlist = sd.lpt ? sd.short_rows.get() : nullptr;
	a.seg_row = a.seg_beg = a.seg_end = nullptr;
	a.seg_out = nullptr;
	a.scratch = nullptr;
	a.scratch_entries = 0;
	if (a.nrows <= 0) return MF_OK;
	const bool extreme = sd.n_long > 0;
	// the large chunk below kSweepFewRows rows.  Never beside the extreme-row path: with the extreme rows gone the
	// occupancy-friendly chunk size is right again.
	const Flavour flavour = mf_sched::launch_flavour(p->weighted, momentum, u.d != 1.0 || u.frozen >= 0 || u.box.columns > 0);
	const SweepForm f = main_form(p, kind, !extreme && a.nrows < kSweepFewRows, flavour);
	if (!f.fn) return MF_ERR_UNSUPPORTED;
	a.nch = f.nch;
	// the user sweep in item bands (mf_schedule.h): the launches below in place of the one main launch, in the same geometry
	const int bands = mf_sched::bands_at_launch(sd.bands, seed, flavour, adaptive) ? sd.bands : 0;
	a.end = nullptr;
	a.resume = 0;
	TimedLaunch t{};
	if (p->timing) {
		MF_HIP(hipEventCreate(&t.t0));
		MF_HIP(hipEventCreate(&t.t1));
		t.kind = kind;
		MF_HIP(hipEventRecord(t.t0, p->stream));
	}
	if (adaptive) MF_TRY(launch_adaptive_tick(p, kind));
	void *args[] = {&a};
	if (extreme) {
		// extreme rows: products kernel over their 64-entry segments -> ordered sum per (row, column slice),
		// beside the sweep of the other rows (schedule below)
		mf::SweepArgs b = a;
		b.nrows = sd.n_seg;
		b.prio_len = 0;
		b.rowlist = nullptr;
		b.nch = p->prod.nch;
		b.seg_row = sd.seg_row;
		b.seg_beg = sd.seg_beg;
		b.seg_end = sd.seg_end;
		b.seg_out = sd.seg_out;
		b.scratch = p->scratch;
		b.scratch_entries = p->scratch_entries;
		void *bargs[] = {&b};
		mf::OrderedSumArgs o;
		o.nrows = sd.n_long;
		o.K = p->K;
		o.ldx = a.ldx;
		o.seed = seed;
		o.d = u.d;
		o.frozen = u.frozen;
		o.box = u.box;
		o.nslices = (int) mf_sched::slice_count(p->K, mf::kSliceCols);
		o.row = sd.long_rows;
		o.sbeg = sd.lr_sbeg;
		o.cnt = sd.lr_cnt;
		o.scratch = p->scratch;
		o.scratch_entries = p->scratch_entries;
		o.X_old = a.X_old;
		o.X_new = a.X_new;
		o.stamps = nullptr;
		o.max_cnt = sd.max_row_len;
		void *oargs[] = {&o};
		// Schedule: products kernel and ordered sums on the side stream while the remaining rows run on the main stream.
		MF_HIP(hipEventRecord(p->ev_fork, p->stream));
		MF_HIP(hipStreamWaitEvent(p->side_stream, p->ev_fork, 0));
		MF_HIP(hipLaunchKernel((const void *) p->prod.fn, dim3(b.nrows), dim3(p->prod.block), bargs, p->prod.lds, p->side_stream));
		if (momentum) {
			// the finished seeds of the extreme rows go into their X_new rows, and the ordered sum starts from those
			mf::SeedPrepArgs s;
			s.nrows = sd.n_long;
			s.K = p->K;
			s.ldx = a.ldx;
			s.frozen = u.frozen;
			s.d = u.d;
			s.beta = u.beta;
			s.row = sd.long_rows;
			s.X_old = a.X_old;
			s.X_new = a.X_new;
			void *sargs[] = {&s};
			MF_HIP(hipLaunchKernel((const void *) mf::momentum_seed_kernel, dim3(s.nrows), dim3(mf::kWave), sargs, 0, p->side_stream));
			o.X_old = a.X_new;
			o.d = 1.0;
		}
		MF_HIP(hipLaunchKernel(ordered_sum_fn(p->cfg), dim3(o.nrows * o.nslices), dim3(mf::kWave), oargs, p->lds_bytes_osum, p->side_stream));
		if (adaptive) MF_TRY(launch_adaptive_finish(p, kind, sd.long_rows, sd.n_long, p->side_stream));
		MF_HIP(hipEventRecord(p->ev_join, p->side_stream));
		a.nrows = sd.n_short;
		a.rowlist = sd.short_rows;
	}
	if (bands > 0) {
		// band b walks the entries [off[b][r], off[b + 1][r]) of every row r, in order on the plan's stream: band 0 seeds with
		// X_old[r], a later one with the partial row in X_new[r]; every band stores the row.  The arguments are read at the launch.
		const SweepFn rfn = band_resume_fn(p);
		if (!rfn) return MF_ERR_UNSUPPORTED;
		const int *off = sd.band_off;
		for (int b = 0; b < bands; ++b) {
			a.ptr = off + (size_t) b * sd.nrows;
			a.end = off + (size_t) (b + 1) * sd.nrows;
			a.resume = b > 0;
			MF_HIP(hipLaunchKernel((const void *) rfn, dim3(std::min(a.nrows, 1 << 20)), dim3(f.block), args, f.lds, p->stream));
		}
	} else if (a.nrows > 0)
		MF_HIP(hipLaunchKernel((const void *) f.fn, dim3(std::min(a.nrows, 1 << 20)), dim3(f.block), args, f.lds, p->stream));
	if (adaptive) MF_TRY(launch_adaptive_finish(p, kind, extreme ? sd.short_rows.get() : nullptr, a.nrows, p->stream));
	if (extreme) {
		if (defer_join)
			p->join_pending = true;
		else
			MF_HIP(hipStreamWaitEvent(p->stream, p->ev_join, 0));
	}
	if (p->timing) {
		MF_HIP(hipEventRecord(t.t1, p->stream));
		p->timed.push_back(t);
	}
	return MF_OK;
}

// One iteration in the errors + streams form: errors launch over the CSR segments (e_n in CSR and CSC order), then
// ONE streams launch that adds up both factors' rows (timed as kind 0 / kind 1 like the two sweeps).
int launch_es_iteration(mf_plan *p)
{
	const SideOperands items = side_operands(p, 0), users = side_operands(p, 1);
	mf::SweepArgs a;
	memset(&a, 0, sizeof a);
	a.nrows = p->es_nseg;
	a.K = p->K;
	a.nch = p->es_nch;
	a.stride = p->stride;
	a.ldx = users.ldx;   // the errors launch walks the CSR
	a.ldy = users.ldy;
	a.seed = 1;
	a.c2 = p->alpha * 2;
	a.d = 1.0;           // the errors launch seeds nothing: e_n does not see the decay
	a.frozen = -1;       // and stores no factor row
	a.box = mf::Box{-INFINITY, INFINITY, 0};   // nor projects one
	a.ptr = users.ptr;
	a.idx = users.idx;
	a.val = users.val;
	a.wgt = users.wgt;   // folded into e_n by the errors launch: the records and the streams launch need nothing new
	a.X_old = users.X_old;
	a.Y_old = users.Y_old;
	a.X_new = nullptr;
	a.seg_row = p->es_seg_row;
	a.seg_beg = p->es_seg_beg;
	a.seg_end = p->es_seg_end;
	a.err_a = reinterpret_cast<double *>(p->rec_csr.get());
	a.err_b = reinterpret_cast<double *>(p->rec_csc.get());
	a.map = p->csr2csc;
	mf::SliceArgs ra;
	ra.K = p->K;
	ra.wg = p->res_wg;
	for (int side = 0; side < 2; ++side) {
		const SideOperands &x = side == 0 ? items : users;
		ra.ptr[side] = x.ptr;
		ra.side[side] = mf::StreamSide{x.rec, x.X_old, x.Y_old, x.X_new};
		ra.yrows[side] = x.yrows;
		ra.ldx[side] = x.ldx;
		ra.ldy[side] = x.ldy;
		const SideUpdate u = side_update(p, side, 1);
		ra.d[side] = u.d;
		ra.frozen[side] = u.frozen;
		ra.beta[side] = u.beta;
		ra.box[side] = u.box;
	}
	const bool momentum = ra.beta[0] != 0.0 || ra.beta[1] != 0.0;
	if (momentum) {
		MF_TRY(leave_rest(p, 0));
		MF_TRY(leave_rest(p, 1));
	}
	TimedLaunch t0{}, t1{};
	if (p->timing) {
		MF_HIP(hipEventCreate(&t0.t0));
		MF_HIP(hipEventCreate(&t0.t1));
		MF_HIP(hipEventCreate(&t1.t1));
		t0.kind = 0;
		t1.kind = 1;
		MF_HIP(hipEventRecord(t0.t0, p->stream));
	}
	void *eargs[] = {&a};
	MF_HIP(hipLaunchKernel((const void *) p->sweep.errs[p->weighted], dim3(p->es_nseg), dim3(mf::kWave), eargs, p->es_lds_errors,
	                       p->stream));
	if (p->timing) MF_HIP(hipEventRecord(t0.t1, p->stream));
	{
		void *rargs[] = {&ra};
		MF_HIP(hipLaunchKernel(stream_resident_fn(p->res_sw, momentum), dim3(p->res_nwg), dim3(mf::kResidentThreads), rargs, p->res_lds, p->stream));
	}
	if (p->timing) {
		MF_HIP(hipEventRecord(t1.t1, p->stream));
		t1.t0 = t0.t1;
		t1.shared_start = true;
		p->timed.push_back(t0);
		p->timed.push_back(t1);
	}
	return MF_OK;
}

// ---- alternating least squares (mf_als.hip.h)

// The form of an ALS solve at this K: one wave per row while a row's triangle is a few blocks per lane (K <= 16), one
// workgroup per row above.  MF_ALS_FORM forces a form where it has this K; every form gives the same bits.
AlsFormId als_form(int K, int forced)
{
	if (forced == kAlsWg) return kAlsWg;
	if (forced == kAlsWave && K <= kAlsForm[kAlsWave].max_k) return kAlsWave;
	return K <= 16 ? kAlsWave : kAlsWg;
}

// The form of a conjugate-gradient solve at this K and its entries per chunk: the pure rules of mf_schedule.h, fed with
// MF_ALS_CG_FORM and the tile geometry of mf_als_cg.hip.h.
mf_sched::AlsCgFormId als_cg_form(int K, int forced) { return mf_sched::als_cg_form(K, forced); }
int als_cg_chunk(int K) { return mf_sched::als_cg_chunk(2 * (size_t) mf::als_cg_vec_bytes(K), (size_t) mf::als_cg_row_stride(K), kLdsPerCu); }

// ---- the Gram of a whole side (mf_gram.hip.h)

int gram_blocks(int rows) { return (rows + mf::kLossBlock - 1) / mf::kLossBlock; }
int gram_rows(const mf_plan *p, int side) { return side == 0 ? p->items : p->uc; }

// the two triangles [items | users] and the partials of the longer side, allocated together on first use
int gram_buffers(mf_plan *p)
{
	if (p->gram) return MF_OK;
	const size_t tri = (size_t) mf::als_triangle(p->K);
	const size_t blocks = (size_t) std::max(1, std::max(gram_blocks(p->items), gram_blocks(p->uc)));
	int rc = p->gram_partial.alloc(blocks * tri);
	if (rc == MF_OK) rc = p->gram.alloc(2 * tri);
	if (rc == MF_OK) rc = p->gram_square.alloc((size_t) p->K * mf::als_icg_ld(p->K));   // what the implicit conjugate-gradient solve reads S from
	if (rc != MF_OK) p->gram_partial.reset(), p->gram.reset();
	return rc;
}

// S of `side` in its current (0) or next (1) buffer into the side's triangle, on the plan's stream: one workgroup per block
// of kLossBlock rows, then the sum over the blocks.  The buffers exist (gram_buffers).
int launch_gram(mf_plan *p, int side, int generation)
{
	const int rows = gram_rows(p, side), tri = mf::als_triangle(p->K), blocks = gram_blocks(rows);
	double *S = p->gram.get() + (size_t) side * tri;
	if (blocks > 0) {
		mf::GramArgs a;
		a.rows = rows;
		a.K = p->K;
		const SideOperands x = side_operands(p, side);
		a.ld = x.ldx;
		a.X = generation ? x.X_new : x.X_old;
		a.partial = p->gram_partial;
		const int nb = (mf::als_blocks(p->K, mf::kGramBS) + mf::kGramThreads - 1) / mf::kGramThreads;
		const size_t lds = (size_t) mf::kGramChunk * mf::als_padded_k(p->K, mf::kGramBS) * sizeof(double);
		hipLaunchKernelGGL(kGramFn[nb - 1], dim3(blocks), dim3(mf::kGramThreads), lds, p->stream, a);
		MF_HIP(hipGetLastError());
	}
	hipLaunchKernelGGL(mf::gram_sum_kernel, dim3((tri + mf::kGramThreads - 1) / mf::kGramThreads), dim3(mf::kGramThreads), 0, p->stream,
	                   (const double *) p->gram_partial.get(), blocks, tri, S);
	MF_HIP(hipGetLastError());
	return MF_OK;
}

// which solve the plan's next launch runs: the rule of mf_schedule.h on the plan's four fields, read at every launch
mf_sched::AlsSolver als_solver(const mf_plan *p) { return mf_sched::als_solver(p->als_kind, p->als_cg, p->implicit_cg, p->als_box); }

// the arguments every row solve of a side takes, but the row list (walk_row_lists' caller fills it per launch)
mf::AlsArgs als_args(const mf_plan *p, int side, int other_generation, unsigned long long *counts)
{
	const SideUpdate u = side_update(p, side, 1);
	const SideOperands x = side_operands(p, side);
	mf::AlsArgs a;
	a.K = p->K;
	a.ldx = x.ldx;
	a.ldy = x.ldy;
	a.frozen = u.frozen;   // -1 under the implicit kind: the caller has refused a frozen column
	a.count_scaled = p->als_kind == MF_ALS_RIDGE_COUNT;
	a.lambda = p->rule[side].lambda;
	a.ptr = x.ptr;
	a.idx = x.idx;
	a.val = x.val;
	a.wgt = x.wgt;
	a.X_old = x.X_old;
	a.X_new = x.X_new;
	a.Y = other_generation ? side_operands(p, side ^ 1).X_new : x.Y_old;   // the other side's next buffer, or its current one
	a.counts = counts;
	a.box = u.box;
	return a;
}

// The row lists of a side in its dispatch order, launch(rowlist, nrows) for each that has rows: the extreme rows of a split
// side first, they are its longest, then the others; a side without extreme rows in one launch, over its LPT list or none.
template <class Launch>
int walk_row_lists(const SweepSide &sd, Launch launch)
{
	if (sd.n_long > 0) {
		if (int rc = launch(sd.long_rows.get(), sd.n_long); rc != MF_OK) return rc;
		return sd.n_short > 0 ? launch(sd.short_rows.get(), sd.n_short) : MF_OK;
	}
	return sd.nrows > 0 ? launch(sd.lpt ? sd.short_rows.get() : nullptr, sd.nrows) : MF_OK;
}

// One solve of a side (0: items, 1: users) against the other side's current (0) or next (1) buffer, into the side's next
// buffer; the only function that launches a row solve.  The rule (als_solver), the steps and the side's update rule are read
// here, at every launch.  Under the implicit kind the Gram of the other side in that generation is enqueued first (the caller
// has refused a frozen column): the direct solve reads it as the packed triangle, the conjugate-gradient one as the plan's
// square, copied in front of it.  Then the counters zeroed and one launch per row list of the side.
int launch_als(mf_plan *p, int side, int other_generation)
{
	const SweepSide &sd = p->side[side];
	const mf_sched::AlsSolver s = als_solver(p);
	if (s.implicit) MF_TRY(launch_gram(p, side ^ 1, other_generation));
	unsigned long long *counts = p->als_counts.get() + 3 * side;
	MF_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned long long), p->stream));
	if (sd.nrows <= 0) return MF_OK;
	mf::AlsImplicit im{s.implicit ? p->gram.get() + (size_t) (side ^ 1) * mf::als_triangle(p->K) : nullptr, p->confidence};
	if (s.implicit && s.cg) {
		const int ld = mf::als_icg_ld(p->K), cells = p->K * ld;
		hipLaunchKernelGGL(mf::gram_square_kernel, dim3((cells + mf::kGramThreads - 1) / mf::kGramThreads), dim3(mf::kGramThreads), 0, p->stream,
		                   im.S, p->K, ld, p->gram_square.get());
		MF_HIP(hipGetLastError());
		im.S = p->gram_square.get();
	}
	mf::AlsArgs a = als_args(p, side, other_generation, counts);

	// the instance, the rows of a workgroup, its threads and LDS request, and the arguments behind `a` in the kernel's order
	const void *fn;
	int rows_per_wg, threads, steps = s.steps, nch = 0, sweeps = s.box_sweeps;
	size_t lds;
	if (s.cg) {
		const int form = als_cg_form(p->K, p->cfg.als_cg_form);
		fn = s.implicit ? als_cg_fn<mf::AlsImplicit>(form, p->K) : als_cg_fn<>(form, p->K);
		nch = als_cg_chunk(p->K);
		rows_per_wg = 1, threads = mf::kWave, lds = mf::als_cg_lds_bytes(p->K, nch);
	} else {
		const AlsForm &form = kAlsForm[als_form(p->K, p->cfg.als_form)];
		const int nb = (mf::als_blocks(p->K, form.bs) + form.threads - 1) / form.threads;
		if (sweeps > 0) {   // the box-constrained solve: the same form, geometry and LDS request
			const AlsBoxForm &box = kAlsBoxForm[als_form(p->K, p->cfg.als_form)];
			fn = s.implicit ? (const void *) box.implicit[nb - 1] : (const void *) box.fn[nb - 1];
		} else {
			fn = s.implicit ? (const void *) form.implicit[nb - 1] : (const void *) form.fn[nb - 1];
		}
		rows_per_wg = mf::kAlsThreads / form.threads, threads = mf::kAlsThreads;
		lds = (size_t) rows_per_wg * mf::als_group_doubles(p->K, form.bs, form.nch, s.implicit || p->weighted) * sizeof(double);
	}
	if (!fn) return MF_ERR_UNSUPPORTED;   // a missing instance is an error, never another kernel
	MF_HIP(raise_lds_limit(fn, lds));
	void *args[4] = {&a};
	int nargs = 1;
	if (sweeps > 0) args[nargs++] = &sweeps;
	if (s.implicit) args[nargs++] = &im;
	if (s.cg) args[nargs++] = &steps, args[nargs++] = &nch;

	return walk_row_lists(sd, [&](const int *rowlist, int nrows) {
		a.rowlist = rowlist;
		a.nrows = nrows;
		MF_HIP(hipLaunchKernel(fn, dim3((nrows + rows_per_wg - 1) / rows_per_wg), dim3(threads), args, lds, p->stream));
		return MF_OK;
	});
}

// The solve cut at the normal equations (mf_als_normal.hip.h), the only function that launches either half.  solve == false:
// the side's normal records over the plan's own entries against the other side in `other_generation`, and record `rows` --
// under the implicit kind launch_gram of that side and generation first, copied on the device; +0.0 otherwise.
// solve == true: every row solved from the records into the side's next buffer, the counters zeroed first.  The forms, the
// row lists and the arguments are launch_als's; the caller has checked the buffer, the pitch and the refusals.
int launch_als_normal(mf_plan *p, int side, int other_generation, double *N, long long pitch, bool solve)
{
	const SweepSide &sd = p->side[side];
	const mf_sched::AlsSolver s = als_solver(p);
	const int np = mf::als_normal_pitch(p->K);
	unsigned long long *counts = p->als_counts.get() + 3 * side;
	mf::AlsNormal nr{N, pitch, sd.nrows, s.implicit ? 1 : 0};
	mf::AlsImplicit im{nullptr, p->confidence};
	if (solve) {
		MF_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned long long), p->stream));
	} else {
		const double *S = nullptr;
		if (s.implicit) {
			MF_TRY(launch_gram(p, side ^ 1, other_generation));
			S = p->gram.get() + (size_t) (side ^ 1) * mf::als_triangle(p->K);
		}
		hipLaunchKernelGGL(mf::als_normal_gram_kernel, dim3((np + mf::kAlsThreads - 1) / mf::kAlsThreads), dim3(mf::kAlsThreads), 0, p->stream, S,
		                   mf::als_triangle(p->K), np, N + (size_t) sd.nrows * (size_t) pitch);
		MF_HIP(hipGetLastError());
	}
	if (sd.nrows <= 0) return MF_OK;
	mf::AlsArgs a = als_args(p, side, other_generation, counts);

	const AlsNormalForm &form = kAlsNormalForm[als_form(p->K, p->cfg.als_form)];
	const int nb = (mf::als_blocks(p->K, form.bs) + form.threads - 1) / form.threads;
	const int rows_per_wg = mf::kAlsThreads / form.threads;
	const void *fn = nullptr;
	if (p->K <= form.max_k && nb >= 1 && nb <= 3)
		fn = solve ? (s.box_sweeps > 0 ? (const void *) kAlsBoxNormalForm[als_form(p->K, p->cfg.als_form)] : (const void *) form.solve)
		           : s.implicit ? (const void *) form.implicit[nb - 1] : (const void *) form.fn[nb - 1];
	if (!fn) return MF_ERR_UNSUPPORTED;   // a missing instance is an error, never another kernel
	const size_t lds = (size_t) rows_per_wg * sizeof(double) *
	                   (solve ? mf::als_solve_normal_doubles(p->K) : mf::als_group_doubles(p->K, form.bs, form.nch, s.implicit || p->weighted));
	MF_HIP(raise_lds_limit(fn, lds));
	int sweeps = s.box_sweeps;
	void *args[3] = {&a, &nr};
	int nargs = 2;
	if (solve && sweeps > 0) args[nargs++] = &sweeps;   // the box-constrained solve of the records (mf_als_box.hip.h)
	if (!solve && s.implicit) args[nargs++] = &im;

	return walk_row_lists(sd, [&](const int *rowlist, int nrows) {
		a.rowlist = rowlist;
		a.nrows = nrows;
		MF_HIP(hipLaunchKernel(fn, dim3((nrows + rows_per_wg - 1) / rows_per_wg), dim3(mf::kAlsThreads), args, lds, p->stream));
		return MF_OK;
	});
}

// ---- the loops of mf_plan_iterate, one per mf_sched::Loop (iterate_path, mf_schedule.h, picks; mf_plan_iterate dispatches)

// what the rule reads of a plan and a call
mf_sched::IterateInput iterate_input(const mf_plan *p, int iters)
{
	mf_sched::IterateInput in;
	in.als = p->als_kind != MF_ALS_OFF;
	in.whole = p->u0 == 0 && p->uc == p->users_total;
	in.rows = (long long) p->uc + p->items;
	in.toy_bytes = mf_sched::toy_lds_bytes(p->uc, p->items, p->K, p->nnz);
	in.nnz = p->nnz;
	in.K = p->K;
	in.iters = iters;
	in.timing = p->timing;
	in.adaptive = adaptive_any(p);
	in.es_mode = p->es_mode;
	in.extreme = p->side[0].n_long > 0 || p->side[1].n_long > 0;
	in.resident = p->cfg.resident;
	in.graph = p->cfg.graph;
	in.graph_max = p->cfg.graph_max;
	return in;
}

// ALS: the users against the current R, the items against the NEW L (Gauss-Seidel), the flip
int iterate_als(mf_plan *p, int iters)
{
	for (int it = 0; it < iters; ++it) {
		MF_TRY(launch_als(p, 1, 0));
		MF_TRY(launch_als(p, 0, 1));
		p->cur ^= 1;
	}
	return MF_OK;
}

// The toy loop: ONE launch of one workgroup runs all `iters` iterations (sweep_resident_kernel), thread t owning factor row t.
int launch_toy_loop(mf_plan *p, int iters)
{
	const SideOperands items = side_operands(p, 0), users = side_operands(p, 1);
	const SideUpdate ui = side_update(p, 0, 1), uu = side_update(p, 1, 1);
	// the result lands where `iters` flips of the two generations would have left it
	const int fin = (iters & 1) ? (p->cur ^ 1) : p->cur;
	mf::ResidentArgs ra;
	ra.users = p->uc;
	ra.items = p->items;
	ra.K = p->K;
	ra.ldl = p->ldl;
	ra.ldr = p->ldr;
	ra.iters = iters;
	ra.c2 = p->alpha * 2;
	ra.d_users = uu.d;
	ra.d_items = ui.d;
	ra.frozen_users = uu.frozen;
	ra.frozen_items = ui.frozen;
	ra.box_users = uu.box;
	ra.box_items = ui.box;
	ra.csr_ptr = users.ptr;
	ra.csr_idx = users.idx;
	ra.csr_val = users.val;
	ra.csr_wgt = users.wgt;
	ra.csc_ptr = items.ptr;
	ra.csc_idx = items.idx;
	ra.csc_val = items.val;
	ra.csc_wgt = items.wgt;
	ra.L_in = users.X_old;
	ra.R_in = items.X_old;
	ra.L_out = p->Lbuf[fin];
	ra.R_out = p->Rbuf[fin];
	ra.nnz = (int) p->nnz;
	// momentum: the next-generation buffers carry the history in; the generation before the final one goes out to
	// the buffers the final one does not take
	ra.beta_users = uu.beta;
	ra.beta_items = ui.beta;
	ra.L_hist = users.X_new;
	ra.R_hist = items.X_new;
	ra.L_prev = p->Lbuf[fin ^ 1];
	ra.R_prev = p->Rbuf[fin ^ 1];
	const bool momentum = ui.beta != 0.0 || uu.beta != 0.0;
	const int threads = ((p->uc + p->items + 63) / 64) * 64;
	const int kmax = mf_sched::toy_kmax(p->K, threads);
	const ResidentFn rfn = kResidentFn[kmax == 4 ? 0 : kmax == 16 ? 1 : kmax == 32 ? 2 : 3][momentum][p->weighted];
	const size_t need = mf_sched::toy_lds_bytes(p->uc, p->items, p->K, p->nnz, p->weighted);   // with the weights, where the plan has them
	MF_HIP(raise_lds_limit((const void *) rfn, need));
	hipLaunchKernelGGL(rfn, dim3(1), dim3(threads), need, p->stream, ra);
	MF_HIP(hipGetLastError());
	p->cur = fin;
	return MF_OK;
}

// `iters` iterations of kLoopEs or kLoopSweeps, launched one by one on the plan's stream
int iterate_eager(mf_plan *p, mf_sched::Loop loop, int iters)
{
	for (int it = 0; it < iters; ++it) {
		if (loop == mf_sched::kLoopEs) {
			MF_TRY(launch_es_iteration(p));
		} else {
			// Both sweeps read only the frozen generation (matFact.c:38-39), so the ordered sums of the item sweep's
			// extreme rows may run on the side stream UNDER the whole user sweep; they are joined before the flip.
			// Not when the user sweep has extreme rows of its own: it would reuse the scratch buffer.
			MF_TRY(launch_sweep(p, 0, 1, /*defer_join=*/p->side[1].n_long == 0));
			MF_TRY(launch_sweep(p, 1, 1));
			if (p->join_pending) {
				MF_HIP(hipStreamWaitEvent(p->stream, p->ev_join, 0));
				p->join_pending = false;
			}
		}
		p->cur ^= 1;
	}
	return MF_OK;
}

// `replays` replays of kGraphIters iterations of `loop`, captured once from iterate_eager on the plan's stream.  The
// capture only records, and kGraphIters is even, so every replay starts from the generation the call started in.
int replay_graph(mf_plan *p, mf_sched::Loop loop, int replays)
{
	hipGraph_t graph = nullptr;
	hipGraphExec_t exec = nullptr;
	const int cur0 = p->cur;
	int rc = MF_OK;
	hipError_t e = hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal);
	if (e == hipSuccess) {
		rc = iterate_eager(p, loop, mf_sched::kGraphIters);
		e = hipStreamEndCapture(p->stream, &graph);
	}
	if (e == hipSuccess && rc == MF_OK) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
	if (e == hipSuccess && rc == MF_OK) {
		p->cur = cur0;
		for (int g = 0; g < replays && e == hipSuccess; ++g) e = hipGraphLaunch(exec, p->stream);
	}
	if (exec) (void) hipGraphExecDestroy(exec);
	if (graph) (void) hipGraphDestroy(graph);
	if (rc != MF_OK) return rc;
	if (e != hipSuccess) {
		g_last_hip_error = std::string("hip graph path: ") + hipGetErrorString(e);
		return MF_ERR_HIP;
	}
	return MF_OK;
}

int drain_timing(mf_plan *p)
{
	for (auto &t : p->timed) {
		MF_HIP(hipEventSynchronize(t.t1));
		float ms = 0.f;
		MF_HIP(hipEventElapsedTime(&ms, t.t0, t.t1));
		p->acc_launch[t.kind]++;
		p->acc_ms[t.kind] += ms;
		if (!t.shared_start) (void) hipEventDestroy(t.t0);
	}
	for (auto &t : p->timed) (void) hipEventDestroy(t.t1);
	p->timed.clear();
	return MF_OK;
}

}  // namespace
