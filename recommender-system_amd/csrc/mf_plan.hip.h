// mf_plan.hip.h -- kernel variant tables, the buffers and operands of a top-N pass and the resident plan (struct mf_plan).
// The plan owns its device memory through dev_buf members (mf_device.hip.h): deleting the plan frees it.
#pragma once
#include "mf_schedule.h"

namespace {

using SweepFn = void (*)(mf::SweepArgs);
using LossFn = void (*)(mf::LossArgs);
using AlsFn = void (*)(mf::AlsArgs);
using AlsImplicitFn = void (*)(mf::AlsArgs, mf::AlsImplicit);
using GramFn = void (*)(mf::GramArgs);

// hipFuncAttributeMaxDynamicSharedMemorySize is per FUNCTION, not per plan: two live plans that share a kernel
// instance (the run-time-K forms) but need different tile sizes must never lower each other's limit.
inline hipError_t raise_lds_limit(const void *fn, size_t bytes)
{
	static std::mutex mu;
	static std::map<std::pair<int, const void *>, size_t> limit;   // the attribute is kept per device
	std::lock_guard<std::mutex> lock(mu);
	int dev = 0;
	(void) hipGetDevice(&dev);
	size_t &cur = limit[std::make_pair(dev, fn)];
	if (bytes <= cur) return hipSuccess;
	const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
	if (e == hipSuccess) cur = bytes;
	return e;
}

using mf_sched::Form, mf_sched::kPlain, mf_sched::kPipelined, mf_sched::kPair, mf_sched::kDb, mf_sched::kCoop, mf_sched::kForms;
using mf_sched::Flavour, mf_sched::kAccumulate, mf_sched::kDecay, mf_sched::kMomentum, mf_sched::kDecayW, mf_sched::kMomentumW, mf_sched::kFlavours;

// One K's kernels: the grid of the main launch's instances, form by flavour (mf_schedule.h), and the kernels beside it.
// A cell a K does not have stays null and launch_sweep refuses it.
struct SweepVariant {
	// kPlain: the single-wave form (the register-staged sweep_kernel, or the LDS-DMA sweep_dma_kernel); kPipelined: the
	// LDS-DMA form with the LDS reads of phases A / B kept in flight (compile-time K); kPair: the wave-pair form (loader +
	// compute) for launches that end on long rows (64 <= K <= 128, compile-time K); kDb: the intra-wave double-buffered form
	// for launches of few rows (all DMA variants); kCoop: the row-cooperative form for tiny sweeps (compile-time-K DMA
	// variants).  The weighted flavours are what a plan created with per-entry weights runs: kDecayW also at lambda = 0,
	// beta = 0, where d = 1.0.
	SweepFn fn[kForms][kFlavours] = {};
	int kt = 0;         // compile-time K, 0 = runtime K
	int kpmax = 0;      // 64-column groups held in registers (register-staged form) / DMA passes per row (run-time-K DMA form)
	int dma = 0;        // 1: LDS-DMA form
	int row_bytes = 0;  // LDS tile row stride in bytes (DMA form)
	int xs_bytes = 0;   // LDS bytes in front of the tile (DMA form)
	// beside the grid, each [weighted] (all DMA variants): the products form for segments of extreme rows; the errors form,
	// e_n per entry of a segment (mf_stream.hip.h); the row sums of mf_plan_loss in the same geometry (the others use
	// loss_reg_kernel)
	SweepFn prod[2] = {}, errs[2] = {};
	LossFn loss[2] = {};
	// the band launches of the user sweep (mf_schedule.h: band_count), [pipelined]: the resume instance of the plain and of
	// the pipelined single-wave form.  Compile-time-K DMA variants only; a K without them runs no bands.
	SweepFn resume[2] = {};
	constexpr bool has(Form form) const { return fn[form][kAccumulate] != nullptr; }
};

// A form whose one instance always multiplies the seed by d, keeps the frozen column and clamps (the register-staged, db,
// pair and coop forms): the accumulate and the decay cell are that instance -- x * 1.0 is x bit for bit.
constexpr void seeded_row(SweepFn *row, SweepFn plain, SweepFn mom, SweepFn wd, SweepFn wm)
{
	row[kAccumulate] = row[kDecay] = plain;
	row[kMomentum] = mom;
	row[kDecayW] = wd;
	row[kMomentumW] = wm;
}

// The LDS-DMA single-wave form multiplies the seed, keeps a frozen column and clamps only in the instances behind its
// accumulate one: one per flavour, at prefetch depth PF (0: plain, 8: pipelined).
template <int KT, int NP, int PF>
constexpr void dma_row(SweepFn *row)
{
	row[kDecay] = mf::sweep_dma_kernel<KT, NP, mf::kSweepDecay, PF>;
	row[kMomentum] = mf::sweep_dma_kernel<KT, NP, mf::kSweepMomentum, PF>;
	row[kDecayW] = mf::sweep_dma_kernel<KT, NP, mf::kSweepDecayW, PF>;
	row[kMomentumW] = mf::sweep_dma_kernel<KT, NP, mf::kSweepMomentumW, PF>;
}

// what all LDS-DMA variants have: the products, errors and loss kernels and the double-buffered form
template <int KT, int NP>
constexpr void dma_common(SweepVariant &v)
{
	v.dma = 1;
	v.fn[kPlain][kAccumulate] = mf::sweep_dma_kernel<KT, NP>;
	seeded_row(v.fn[kDb], mf::sweep_db_kernel<KT, NP>, mf::sweep_db_kernel<KT, NP, true>, mf::sweep_db_kernel<KT, NP, false, true>,
	           mf::sweep_db_kernel<KT, NP, true, true>);
	v.prod[0] = mf::sweep_dma_kernel<KT, NP, mf::kSweepProducts>, v.prod[1] = mf::sweep_dma_kernel<KT, NP, mf::kSweepProductsW>;
	v.errs[0] = mf::sweep_dma_kernel<KT, NP, mf::kSweepErrors>, v.errs[1] = mf::sweep_dma_kernel<KT, NP, mf::kSweepErrorsW>;
	v.loss[0] = mf::loss_dma_kernel<KT, NP>, v.loss[1] = mf::loss_dma_w_kernel<KT, NP>;
}

template <int KT, int KP>
constexpr SweepVariant variant()
{
	SweepVariant v;
	seeded_row(v.fn[kPlain], mf::sweep_kernel<KT, KP>, mf::sweep_kernel<KT, KP, true>, mf::sweep_kernel<KT, KP, false, true>,
	           mf::sweep_kernel<KT, KP, true, true>);
	v.kt = KT;
	v.kpmax = KP;
	return v;
}

template <int KT>
constexpr SweepVariant dma_variant()
{
	constexpr int NP = mf::DmaGeom<KT>::kPasses;
	SweepVariant v;
	dma_common<KT, NP>(v);
	v.kt = KT;
	v.row_bytes = mf::DmaGeom<KT>::kStride;
	v.xs_bytes = mf::DmaGeom<KT>::kXsBytes;
	// two-pass rows (K = 256) take the pipelined form at every size (single_wave_pipelined): no plain instance but the
	// accumulate one
	if constexpr (KT <= 128) dma_row<KT, NP, 0>(v.fn[kPlain]);
	v.fn[kPipelined][kAccumulate] = mf::sweep_dma_kernel<KT, NP, mf::kSweepAccumulate, 8>;
	dma_row<KT, NP, 8>(v.fn[kPipelined]);
	if constexpr (KT <= 128) v.resume[0] = mf::sweep_dma_kernel<KT, NP, mf::kSweepResume, 0>;
	v.resume[1] = mf::sweep_dma_kernel<KT, NP, mf::kSweepResume, 8>;
	if constexpr (mf::DmaGeom<KT>::kOnePassWide)
		seeded_row(v.fn[kPair], mf::sweep_pair_kernel<KT, 1>, mf::sweep_pair_kernel<KT, 1, true>, mf::sweep_pair_kernel<KT, 1, false, true>,
		           mf::sweep_pair_kernel<KT, 1, true, true>);
	seeded_row(v.fn[kCoop], mf::sweep_coop_kernel<KT>, mf::sweep_coop_kernel<KT, true>, mf::sweep_coop_kernel<KT, false, true>,
	           mf::sweep_coop_kernel<KT, true, true>);
	return v;
}

// run-time even K <= 128 * NPASS through the LDS-DMA kernel (row_bytes / xs_bytes filled in per plan)
template <int NPASS>
constexpr SweepVariant dma_generic_variant()
{
	SweepVariant v;
	dma_common<0, NPASS>(v);
	v.kpmax = NPASS;
	dma_row<0, NPASS, 0>(v.fn[kPlain]);
	return v;
}

// The geometry of a launch: entries per chunk, LDS request and workgroup size; and a launchable form, a geometry with its kernel.
struct LaunchGeometry {
	int nch = 0;
	size_t lds = 0;
	int block = mf::kWave;
};
struct SweepForm : LaunchGeometry {
	SweepFn fn = nullptr;
};

// K-specialised instances for the K of the bundled samples and of the BASELINE configs, then generic ones.
const SweepVariant kSpecialised[] = {
    variant<10, 1>(), variant<20, 1>(), variant<30, 1>(), variant<50, 1>(),
    variant<100, 2>(), variant<128, 2>(), variant<256, 4>(),
};
// LDS-DMA form: the production kernel for these (even) K
const SweepVariant kDma[] = {
    dma_variant<10>(), dma_variant<20>(), dma_variant<30>(), dma_variant<50>(),
    dma_variant<100>(), dma_variant<128>(), dma_variant<256>(),
};
const SweepVariant kDmaGeneric[] = {
    dma_generic_variant<1>(), dma_generic_variant<2>(), dma_generic_variant<4>(), dma_generic_variant<8>(),
};
const SweepVariant kGeneric[] = {
    variant<0, 1>(), variant<0, 2>(), variant<0, 4>(), variant<0, 8>(),
    variant<0, 16>(), variant<0, 32>(), variant<0, 64>(),
};

constexpr int kLargestK = 64 * mf::kWave;   // the widest row of kGeneric: choose_sweep refuses a larger K

constexpr size_t kLdsPerCu = 160 * 1024;
constexpr size_t kChipL2Bytes = (size_t) 32 << 20;   // 8 XCDs x 4 MiB

// One side of an iteration (0 = items / CSC, 1 = users / CSR): its rows and what plan_row_schedule decided for its sweep by
// the rules of mf_schedule.h.
struct SweepSide {
	int nrows = 0;           // items / the shard's users
	bool use_db = false;     // the sweep's main launch takes the double-buffered form
	bool use_pair = false;   // ... or the wave-pair form
	bool coop_all = false;   // ... or is ONE cooperative launch over all rows (tiny sweeps)
	int max_row_len = 0;     // longest column (item sweep) / longest user row (user sweep)
	int prio_len = 0;        // rows at least this long run at raised wave priority in the single-wave launch (0: none)
	// skew-aware split of a sweep with many rows: rows whose serial walk would dominate the launch go to the extreme-row
	// path on a side stream (products over their segments -> ordered sums), the others stay on the main launch
	dev_buf<int> long_rows, short_rows;
	bool lpt = false;        // short_rows = ALL rows in dispatch order: a sweep without extreme rows
	int n_long = 0, n_short = 0;
	int long_len = 0;        // a row at least this long is on the extreme-row path (when n_long > 0)
	int n_seg = 0;
	dev_buf<int> seg_row, seg_beg, seg_end;
	dev_buf<long long> seg_out, lr_sbeg;
	dev_buf<int> lr_cnt;
	// item bands of the user sweep (mf_schedule.h: band_count; 0 on the item side): the count and the entry offsets
	// [bands + 1][nrows], offset [b][r] = the first entry of row r whose item id is at least band b's first item
	int bands = 0;
	dev_buf<int> band_off;
	bool last_unseeded = false;   // the side's last sweep was launched unseeded, so in one launch: mf_plan_describe tells no bands
};

struct TimedLaunch {
	hipEvent_t t0, t1;
	int kind;            // 0 item sweep / errors launch, 1 user sweep / streams launch
	bool shared_start;   // t0 is the previous record's t1 (not owned)
};

// What a top-N pass (launch_topn_core, mf_certified.hip.h) writes and reports: the output rows (rows x n), the per-split lists of
// an item split, and the last call's exact-pass count and form.  All device buffers are allocated on first use and grown
// on demand; one instance per entry point, so the report of one is not disturbed by a call of the other.
struct topn_buffers {
	dev_buf<int> items;              // items / scores share a capacity, part_v / part_i another
	dev_buf<double> scores;
	dev_buf<double> part_v;
	dev_buf<int> part_i, part_bad;
	int64_t last_uncertain = -1;     // rows of the last call that went through the exact pass (-1: exact form ran)
	int form = -1;                   // form of the last call (mf_plan_recommend_topn_info)
};

// The operands of a top-N pass: `rows` rows of L (pitch ldl) are ranked against the `items` rows of R (pitch ldr), row i
// choosing among the items its mask (a CSR over the rows: item ids ascending within a row) leaves open.
struct topn_operands {
	int rows = 0, items = 0;
	const double *L = nullptr, *R = nullptr;
	int ldl = 0, ldr = 0;
	const int *mask_ptr = nullptr, *mask_idx = nullptr;
	double *lnorm = nullptr;                    // scratch: the norm of every row of L (rows doubles)
	unsigned long long *rmax_bits = nullptr;    // scratch: the largest norm of a row of R
	int *ulist = nullptr, *ucount = nullptr;    // scratch: the rows that need the exact pass (rows ints) and their number
	topn_buffers *out = nullptr;
};

// How one side's rows are updated: what the setters of the C API write and the getters read.
struct SideRule {
	double lambda = 0.0;   // L2 regularisation, mf_plan_set_regularization
	double beta = 0.0;     // heavy-ball momentum, mf_plan_set_momentum
	int frozen = -1;       // frozen column or -1, mf_plan_set_frozen_columns
	// box constraint, mf_plan_set_bounds: columns k < columns (-1: all K) of a finished row are projected onto [lo, hi]
	double lo = -INFINITY, hi = INFINITY;
	int columns = -1;
	// a side at rest has no history: X_prev = X_old by definition.  Set by mf_plan_upload_factors and by a change of the
	// side's beta from 0; cleared by its first seeded momentum sweep (leave_rest copies current -> next) and by
	// mf_plan_upload_previous
	bool at_rest = true;
	// adaptive step size, mf_plan_set_adaptive: kind NONE is the plain step.  A side never has beta != 0 and a kind
	mf_adaptive opt = {MF_OPT_NONE, 0.0, 0.0, 0.0, 0.0};
};

// The accumulators of an adaptive side (mf_adaptive.hip.h), allocated when first needed: m (ADAM only) and v, rows x the
// side's pitch, and the step record.  `rest`: the state is at rest by definition -- zeros, 1.0, 0 steps -- whatever the
// buffers hold; adaptive_ready (mf_launch.hip.h) makes them say so in front of the side's next adaptive launch.
struct AdaptiveState {
	dev_buf<double> m, v;
	dev_buf<mf::AdaptiveStep> step;
	bool rest = true;
};

// The forms of the ALS solve (mf_als.hip.h): how many threads own a row, the side of a register block, the entries of a
// gather chunk, the widest K, and the instances by blocks per thread (NB = 1, 2, 3).  als_form (mf_launch.hip.h) picks one.
enum AlsFormId { kAlsWg = 0, kAlsWave = 1, kAlsForms = 2 };
struct AlsForm {
	const char *name;
	int threads, bs, nch, max_k;
	AlsFn fn[3];
	AlsImplicitFn implicit[3];   // the instances of MF_ALS_IMPLICIT: the same forms, S and conf beside the arguments
};
const AlsForm kAlsForm[kAlsForms] = {
    {"wg", mf::kAlsThreads, 4, mf::kAlsChunkWg, mf::kAlsMaxK,
     {mf::als_kernel<mf::kAlsThreads, 4, 1>, mf::als_kernel<mf::kAlsThreads, 4, 2>, mf::als_kernel<mf::kAlsThreads, 4, 3>},
     {mf::als_kernel<mf::kAlsThreads, 4, 1, mf::AlsImplicit>, mf::als_kernel<mf::kAlsThreads, 4, 2, mf::AlsImplicit>, mf::als_kernel<mf::kAlsThreads, 4, 3, mf::AlsImplicit>}},
    {"wave", mf::kWave, 2, mf::kAlsChunkWave, mf::kAlsWaveMaxK,
     {mf::als_kernel<mf::kWave, 2, 1>, mf::als_kernel<mf::kWave, 2, 2>, mf::als_kernel<mf::kWave, 2, 3>},
     {mf::als_kernel<mf::kWave, 2, 1, mf::AlsImplicit>, mf::als_kernel<mf::kWave, 2, 2, mf::AlsImplicit>, mf::als_kernel<mf::kWave, 2, 3, mf::AlsImplicit>}},
};
// The same forms of the solve cut at the normal equations (mf_als_normal.hip.h), in the order of AlsFormId: the instances
// that write a side's normal records by blocks per thread, explicit and implicit, and the one that solves from them.
using AlsNormalFn = void (*)(mf::AlsArgs, mf::AlsNormal);
using AlsNormalImplicitFn = void (*)(mf::AlsArgs, mf::AlsNormal, mf::AlsImplicit);
struct AlsNormalForm {
	const char *name;
	int threads, bs, nch, max_k;
	AlsNormalFn fn[3];
	AlsNormalImplicitFn implicit[3];
	AlsNormalFn solve;
};
const AlsNormalForm kAlsNormalForm[kAlsForms] = {
    {"wg", mf::kAlsThreads, 4, mf::kAlsChunkWg, mf::kAlsMaxK,
     {mf::als_normal_kernel<mf::kAlsThreads, 4, 1>, mf::als_normal_kernel<mf::kAlsThreads, 4, 2>, mf::als_normal_kernel<mf::kAlsThreads, 4, 3>},
     {mf::als_normal_kernel<mf::kAlsThreads, 4, 1, mf::AlsImplicit>, mf::als_normal_kernel<mf::kAlsThreads, 4, 2, mf::AlsImplicit>, mf::als_normal_kernel<mf::kAlsThreads, 4, 3, mf::AlsImplicit>},
     mf::als_solve_normal_kernel<mf::kAlsThreads>},
    {"wave", mf::kWave, 2, mf::kAlsChunkWave, mf::kAlsWaveMaxK,
     {mf::als_normal_kernel<mf::kWave, 2, 1>, mf::als_normal_kernel<mf::kWave, 2, 2>, mf::als_normal_kernel<mf::kWave, 2, 3>},
     {mf::als_normal_kernel<mf::kWave, 2, 1, mf::AlsImplicit>, mf::als_normal_kernel<mf::kWave, 2, 2, mf::AlsImplicit>, mf::als_normal_kernel<mf::kWave, 2, 3, mf::AlsImplicit>},
     mf::als_solve_normal_kernel<mf::kWave>},
};
// The box-constrained solve (mf_als_box.hip.h) in the same forms, in the order of AlsFormId and by blocks per thread: the
// instances launch_als and launch_als_normal(solve) take where the rule (als_solver) names box sweeps; the geometry and the LDS
// request of a form are kAlsForm's / kAlsNormalForm's.
using AlsBoxFn = void (*)(mf::AlsArgs, int);
using AlsBoxImplicitFn = void (*)(mf::AlsArgs, int, mf::AlsImplicit);
using AlsBoxNormalFn = void (*)(mf::AlsArgs, mf::AlsNormal, int);
struct AlsBoxForm {
	AlsBoxFn fn[3];
	AlsBoxImplicitFn implicit[3];
};
const AlsBoxForm kAlsBoxForm[kAlsForms] = {
    {{mf::als_box_kernel<mf::kAlsThreads, 4, 1>, mf::als_box_kernel<mf::kAlsThreads, 4, 2>, mf::als_box_kernel<mf::kAlsThreads, 4, 3>},
     {mf::als_box_kernel<mf::kAlsThreads, 4, 1, mf::AlsImplicit>, mf::als_box_kernel<mf::kAlsThreads, 4, 2, mf::AlsImplicit>, mf::als_box_kernel<mf::kAlsThreads, 4, 3, mf::AlsImplicit>}},
    {{mf::als_box_kernel<mf::kWave, 2, 1>, mf::als_box_kernel<mf::kWave, 2, 2>, mf::als_box_kernel<mf::kWave, 2, 3>},
     {mf::als_box_kernel<mf::kWave, 2, 1, mf::AlsImplicit>, mf::als_box_kernel<mf::kWave, 2, 2, mf::AlsImplicit>, mf::als_box_kernel<mf::kWave, 2, 3, mf::AlsImplicit>}},
};
const AlsBoxNormalFn kAlsBoxNormalForm[kAlsForms] = {mf::als_box_solve_normal_kernel<mf::kAlsThreads>, mf::als_box_solve_normal_kernel<mf::kWave>};
// The forms of the conjugate-gradient solve in the order of mf_sched::AlsCgFormId; als_cg_form (mf_launch.hip.h) picks one,
// als_cg_fn<>(form, K) its explicit instance (als_cg_kernel, mf_als_cg.hip.h), als_cg_fn<mf::AlsImplicit>(form, K) its
// implicit one (als_icg_kernel, mf_als_icg.hip.h): null where the form does not take the K, and for the implicit kind above
// K = 128 -- it has one piece per lane, so none of the two-pass instances.
const char *const kAlsCgFormName[mf_sched::kAlsCgForms] = {"fixed", "dma", "general"};
static_assert(mf_sched::kAlsImplicitKind == MF_ALS_IMPLICIT && mf_sched::kAlsDirectMaxK == mf::kAlsMaxK, "als_solver (mf_schedule.h) restates both");
template <int KT, int NP, bool DMA, class... IM>
inline const void *als_cg_instance()
{
	if constexpr (sizeof...(IM) == 0)
		return (const void *) mf::als_cg_kernel<KT, NP, DMA>;
	else if constexpr (NP == 1)
		return (const void *) mf::als_icg_kernel<KT, NP, DMA>;
	else
		return nullptr;
}
template <class... IM>
inline const void *als_cg_fn(int form, int K)
{
	if (!mf_sched::als_cg_takes(form, K) || (sizeof...(IM) == 1 && K > mf::kAlsMaxK)) return nullptr;
	if (form == mf_sched::kAlsCgFixed) {
		switch (K) {
		case 10: return als_cg_instance<10, 1, true, IM...>();
		case 20: return als_cg_instance<20, 1, true, IM...>();
		case 30: return als_cg_instance<30, 1, true, IM...>();
		case 50: return als_cg_instance<50, 1, true, IM...>();
		case 100: return als_cg_instance<100, 1, true, IM...>();
		case 128: return als_cg_instance<128, 1, true, IM...>();
		case 256: return als_cg_instance<256, 2, true, IM...>();
		}
		return nullptr;
	}
	const bool two = mf::als_cg_passes(K) == 2;
	if (form == mf_sched::kAlsCgDma) return two ? als_cg_instance<0, 2, true, IM...>() : als_cg_instance<0, 1, true, IM...>();
	return two ? als_cg_instance<0, 2, false, IM...>() : als_cg_instance<0, 1, false, IM...>();
}
// the Gram of a whole side (mf_gram.hip.h) by blocks of the triangle per thread, as the workgroup form above
const GramFn kGramFn[3] = {mf::gram_block_kernel<1>, mf::gram_block_kernel<2>, mf::gram_block_kernel<3>};

// the toy loop (sweep_resident_kernel, mf_sweep.hip.h) by [register-row class][momentum][weighted]; the classes are the
// values of mf_sched::toy_kmax: 4, 16, 32 and, last, 0
using ResidentFn = void (*)(mf::ResidentArgs);
#define MF_TOY_ROW(KMAX) \
	{{mf::sweep_resident_kernel<KMAX, false, false>, mf::sweep_resident_kernel<KMAX, false, true>}, \
	 {mf::sweep_resident_kernel<KMAX, true, false>, mf::sweep_resident_kernel<KMAX, true, true>}}
const ResidentFn kResidentFn[4][2][2] = {MF_TOY_ROW(4), MF_TOY_ROW(16), MF_TOY_ROW(32), MF_TOY_ROW(0)};
#undef MF_TOY_ROW
// the resident streams launch (mf_resident.hip.h) by [slice width 8, 4, 2][momentum]
using StreamResidentFn = void (*)(mf::SliceArgs);
const StreamResidentFn kStreamResidentFn[3][2] = {{mf::stream_resident_kernel<8>, mf::stream_resident_kernel<8, true>},
                                                  {mf::stream_resident_kernel<4>, mf::stream_resident_kernel<4, true>},
                                                  {mf::stream_resident_kernel<2>, mf::stream_resident_kernel<2, true>}};

}  // namespace

struct mf_plan {
	mf_config cfg;   // the environment switches, read once at creation (mf_config.hip.h)
	int device = 0;
	int users_total = 0, items = 0, K = 0;
	int u0 = 0, uc = 0;
	int64_t nnz = 0;
	double alpha = 0.0;
	SideRule rule[2];   // the update rule per side (0 = items, 1 = users); side_update (mf_launch.hip.h) reads it at every launch
	AdaptiveState opt[2];   // the accumulators of a side whose rule has an adaptive kind
	// alternating least squares (mf_als.hip.h): the kind (mf_plan_set_als; OFF: the plan of every other section) and the
	// three row counts of each side's last solve, [side][solved, kept_empty, kept_not_pd], allocated on first use
	int als_kind = MF_ALS_OFF;
	int als_cg = 0;   // conjugate-gradient steps per row (mf_plan_set_als_cg; 0: the direct solve), read at every launch
	int als_box = 0;  // coordinate-descent sweeps per row (mf_plan_set_als_box; 0: Cholesky, then the clamp), read at every launch
	dev_buf<unsigned long long> als_counts;
	// implicit feedback: the confidence scale (mf_plan_set_confidence, read at every launch) and the Gram matrices of the two
	// sides (mf_plan_gram): [items | users], each a packed lower triangle, and the per-block partials they are summed from
	// (as many blocks as the longer side has), allocated together on first use
	double confidence = 1.0;
	dev_buf<double> gram, gram_partial;
	// conjugate-gradient steps per row under MF_ALS_IMPLICIT (mf_plan_set_implicit_cg; 0: the direct solve), read at every
	// launch, and the square its kernel reads the other side's Gram from (K rows of an even stride), allocated with the above
	int implicit_cg = 0;
	dev_buf<double> gram_square;
	int flags = 0;

	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr;

	// CSR over the shard's users (idx = item id) and CSC over items (idx = LOCAL user id)
	dev_buf<int> csr_ptr, csr_idx;
	dev_buf<double> csr_val;
	dev_buf<int> csc_ptr, csc_idx;
	dev_buf<double> csc_val;
	// per-entry confidence weights (mf_plan_create_weighted), in CSR and in CSC order beside the values; a plan created
	// without weights allocates neither and launches the unweighted kernels
	bool weighted = false;
	dev_buf<double> csr_wgt, csc_wgt;
	dev_buf<int> mask_idx;   // item ids ascending inside every user's row, only when the file order is not (recommend mask)
	// errors + streams iteration (mf_stream.hip.h): CSR position -> CSC position, the {idx, e_n} records in both orders, the segment table
	// of the errors launch and the task list (both factors' rows, longest first) of the streams launch
	bool want_map = false, es_mode = false;
	dev_buf<int> csr2csc;
	dev_buf<mf::StreamRec> rec_csr, rec_csc;
	int es_nseg = 0, es_nch = 0;
	size_t es_lds_errors = 0;
	dev_buf<int> es_seg_row, es_seg_beg, es_seg_end;
	// streams launch with a column slice of Y resident in LDS (mf_resident.hip.h): small factor matrices only
	int res_sw = 0, res_nwg = 0;
	size_t res_lds = 0;
	dev_buf<mf::SliceWg> res_wg;

	double *Lbuf[2] = {nullptr, nullptr};   // the two generations: the plan's own buffers or the caller's
	double *Rbuf[2] = {nullptr, nullptr};
	dev_buf<double> Lown[2], Rown[2];       // the plan's own, empty when l_external / r_external
	int ldl = 0, ldr = 0;   // row pitch of the L and R buffers in doubles (K, or K padded to whole 128-byte lines)
	bool r_external = false;
	bool l_external = false;
	bool join_pending = false;          // ordered sums of the last item sweep still run on the side stream
	dev_buf<mf_candidate> cand_dev;     // recommend_scored output, allocated on first use
	dev_buf<mf_candidate> cand_pack;    // the listed users' records in list order (recommend_scored_users)
	dev_buf<mf_filter> filt_dev;        // recommend_filter output, allocated on first use
	dev_buf<mf_filter> part_dev;        // per-split reports of a small recommendation (nsplit x users), grown on demand
	bool rec_half_used = false;   // the last MFMA pass ran as 64-user workgroups, two per CU (recommend_mfma2_kernel)
	int cur = 0;            // generation index of the current factors
	bool have_factors = false;
	dev_buf<int> best_dev;
	// MFMA recommend scratch
	dev_buf<double> lnorm;
	dev_buf<unsigned long long> rmax_bits;
	dev_buf<int> ulist, ucount;
	int64_t last_uncertain = -1;   // users re-scored by the exact pass in the last recommend (-1: exact form ran)
	// top-N (mf_plan_recommend_topn) and similar items (mf_plan_similar_items): each its own output rows, per-split lists
	// and report of the last call
	topn_buffers topn, sim;
	// similar items, allocated on first use and grown on demand: Q (the rows of R divided by their norms, R's pitch), the
	// gathered rows of a listed query with the device copy of the list, the self mask, and the pass's scratch by query row
	dev_buf<double> sim_q, sim_block, sim_lnorm;
	dev_buf<int> sim_query, sim_ptr, sim_idx, sim_ulist;

	// loss (mf_plan_loss, mf_loss.hip.h): row sums, block sums and total, allocated on first use; the held-out set as a
	// second CSR over the shard's users (entries of a user in the caller's order)
	LossFn loss_fn[2] = {nullptr, nullptr};   // [1]: the weighted twin (the training loss of a weighted plan)
	int loss_nch[2] = {0, 0};        // chunk size of the row-sum launch: [0] ordinary, [1] fewer rows than fill the chip
	size_t loss_lds[2] = {0, 0};     // its LDS request (the L row + ONE tile)
	dev_buf<double> row_sse, loss_blocks, loss_total;
	// penalty (mf_plan_penalty), allocated on first use: the row sums of squares [users | items], their block sums
	// [user blocks | item blocks] and the two totals
	dev_buf<double> pen_rows, pen_blocks, pen_total;
	// the three counts of mf_plan_bounds_active (at_lo, at_hi, inside), allocated on first use
	dev_buf<unsigned long long> box_counts;
	dev_buf<int> ho_ptr, ho_idx;
	dev_buf<double> ho_val;
	int64_t ho_nnz = 0;
	bool have_heldout = false;
	// ranks of the held-out entries (mf_plan_rank_heldout, mf_rank.hip.h): the local user of every bucketed entry, the
	// bucketed position of every entry the caller gave (host), and the pass's six buffers, which share a capacity and grow
	// on demand
	dev_buf<int> ho_user;
	std::vector<int> ho_pos;
	dev_buf<double> rank_score;
	dev_buf<int> rank_state, rank_out, rank_above, rank_band, rank_list;
	int64_t last_rank_uncertain = -1;   // entries of the last rank call that went through the exact pass (-1: exact form ran)
	int rank_form = -1;                 // form of the last rank call (mf_plan_rank_heldout_info)

	SweepVariant sweep{};
	int stride = 0;             // register-staged form: LDS row stride in doubles
	// the geometries of a sweep's main launch (launch_sweep: main_form adds the instance from the grid)
	LaunchGeometry single;      // single-wave form at the chunk size of choose_sweep
	LaunchGeometry few;         // ... at the chunk size for a sweep of too few rows to fill the chip
	LaunchGeometry db;          // double-buffered form (two tiles)
	LaunchGeometry pair;        // wave-pair form (two tiles, two waves per row)
	LaunchGeometry coop;           // tiny sweeps (a few us of data): ONE cooperative launch over all rows; a fork/join costs more than it saves
	SweepForm prod;             // products launch over the segments of the extreme rows
	SweepSide side[2];          // 0 = items / CSC, 1 = users / CSR
	// extreme rows: 64-entry segments -> scaled rows in `scratch` -> ordered sum
	dev_buf<double> scratch;
	size_t scratch_entries = 0;
	size_t lds_bytes_osum = 0;  // LDS request of ordered_sum_kernel (ring + padding that bounds the waves per CU)
	hipStream_t side_stream = nullptr;
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;

	bool timing = false;
	std::vector<TimedLaunch> timed;
	int64_t acc_launch[2] = {0, 0};
	double acc_ms[2] = {0.0, 0.0};
};

