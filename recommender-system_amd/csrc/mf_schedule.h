// mf_schedule.h -- how the two sweeps of a plan run, decided on the host from the row lengths alone: which rows count as
// extreme, whether a tiny sweep is ONE cooperative launch, the segment tables of the extreme-row path, the wave
// priority, the form of the main launch and the dispatch order, and the tables of the errors +
// streams iteration (5.6); the choice made at every launch, the form, flavour and geometry of a main launch (5.8k); and the
// choice made at every mf_plan_iterate, the loop an iteration runs in and its graph replays (5.8k2).
// Pure functions of (row pointers, K, switches, limits): no HIP type, no kernel header, so they compile with any C++17
// compiler and tests/test_schedule.py, tests/test_launch_choice.py and tests/test_iterate_path.py pin them on a CPU.
// mf_build.hip.h fills the inputs, calls sweep_schedule / es_errors / es_workgroups, and allocates and uploads what they
// return; mf_launch.hip.h makes the launch-time choice and fills the rule's input for mf_plan_iterate.
#pragma once
#include <algorithm>
#include <cstddef>
#include <functional>
#include <vector>

namespace mf_sched {

// the environment switches the rules read (mf_config.hip.h)
struct Switches {
	bool skew = true;              // MF_SWEEP_SKEW=0: no split of long rows
	int sweep_nch = 0;             // MF_SWEEP_NCH
	bool sweep_long_set = false;   // MF_SWEEP_LONG
	double sweep_long = 0.0;
	int sweep_pair = -1;           // MF_SWEEP_PAIR
	int sweep_db = -1;             // MF_SWEEP_DB
};

// what the chosen kernel variant can do and the kernel constants, filled by the caller
struct Caps {
	bool prod = false, pf = false, pair = false, coop = false, db = false;   // the forms the variant has
	int row_bytes = 0, xs_bytes = 0;   // LDS tile row stride and the bytes in front of the tile
	int single_nch = 0;                // entries per chunk of the single-wave form
	int coop_producers = 0, coop_waves = 0, slice_cols = 0, block_entries = 0, wave = 0;
	size_t lds_per_cu = 0;
};

struct Problem {
	int K = 0;
	long long nnz = 0;
	// free device memory in bytes; asked only where the scratch cap is consulted (rare), because the query is not free:
	// a process's first one costs about 10 ms on the MI355X (profiles/sweep_schedule/README.md)
	std::function<size_t()> free_bytes;
};

// one side's rows: row r holds the entries [ptr[r], ptr[r + 1])
struct Rows {
	const int *ptr = nullptr;
	int nrows = 0;
	int len(int r) const { return ptr[(size_t) r + 1] - ptr[r]; }
	int longest() const
	{
		int m = 0;
		for (int r = 0; r < nrows; ++r) m = std::max(m, len(r));
		return m;
	}
};

// estimated bandwidth time of one sweep in us: nnz * 8K bytes at ~6 TB/s
inline double sweep_us(const Problem &pb) { return (double) pb.nnz * 8.0 * pb.K / 6e12 * 1e6; }
// column slices of the extreme-row scratch
inline size_t slice_count(int K, int slice_cols) { return (size_t) ((K + slice_cols - 1) / slice_cols); }

// Does the single-wave launch of this sweep take the wave-pair form (mf_sweep.hip.h: loader + compute wave per row)?  Where
// the kernel exists (64 <= K <= 128, compile-time K) and the side is
//   made of long rows: 512 entries per row or more on average, skewed or not -- a wave spends its life inside rows, where
//          the pair overlaps the gather of chunk c+1 with the arithmetic of chunk c (cfg4's 1e5 items of 1000 entries:
//          11.77 vs 12.19 ms, three alternating runs on one box).  On a skewed side of that kind (the Netflix shape's 17770
//          items of 3770 entries, cfg4-Zipf's) the extreme-row threshold moves up 2.7x with the pairs (long_threshold),
//          the scratch round trip shrinks and the side stream no longer eats into the other sweep: Netflix shape 19.7 ->
//          17.1 ms, cfg4-Zipf 35.5 -> 31.2 (profiles/r03/pair_long_rows_ab.txt; at the single-wave threshold the pairs LOSE
//          there, 20.0 vs 19.7); or
//   small and skewed: at most 65536 rows and ~2 ms of bytes, the longest row at least four times the mean -- such a launch
//          ENDS on its long rows, which a pair walks 2.4x faster than one wave (cfg3 power-law).
// Short equally long rows stay on the single-wave form (cfg3 uniform, 253 / 166 entries per row: 0.207 vs 0.222 ms), and so
// does a large side of short rows (users of the Netflix shape 8.2 vs 6.8 ms, of cfg4 12.9 vs 11.4).  MF_SWEEP_PAIR=0|1 overrides.
inline bool pair_long_rows(const Problem &pb, int nrows) { return nrows >= 512 && pb.nnz / nrows >= 512; }
inline bool pair_wanted(const Problem &pb, const Caps &caps, const Switches &sw, int nrows, int longest)
{
	if (!caps.pair || sw.sweep_pair == 0) return false;
	if (sw.sweep_pair == 1) return true;
	if (nrows < 512 || pb.nnz <= 0) return false;
	if (pair_long_rows(pb, nrows)) return true;
	if ((long long) longest < 4 * std::max<long long>(pb.nnz / nrows, 1)) return false;
	return nrows <= 65536 && sweep_us(pb) <= 2000.0;
}

// The long threshold of one side.  A row is "long" when its serial walk would exceed a good part of the bandwidth time
// of the whole sweep (nnz * 8K bytes at ~7 TB/s): len > 4e-6 (6e-6) * nnz * K, and never below 128 entries.  cfg4
// has none; a power-law instance a few.
// (6e-6 where the accumulate form with the pipelined phases exists: its lone wave walks 0.13 us per entry at K=100
// instead of 0.17, so fewer rows need the scratch round trip -- Netflix shape 21.05 -> 19.68 ms at 40000 instead of
// 26800 entries, cfg4-Zipf 34.5 -> 33.9; round 2's 4e-6 otherwise)
// ... and only rows well above the average count as long: when every row is equally long (the cfg4
// twin: 1000 items x 1000 entries) there is no skew to fix and the single-wave kernel is the faster one
// (a side of long rows walked by wave pairs -- 0.055 us per entry instead of 0.13 --: 16e-6 nnz K.  Netflix shape,
// pairs on the item side: 18.5 / 17.9 / 17.1 / 18.6 ms at 60 / 80 / 100 / 160 thousand entries, the rule gives 107 000;
// cfg4-Zipf 32.6 / 31.2 / 31.2 / 39.9 at 120 / 160 / 220 / 400 thousand, the rule gives 160 000)
inline int long_threshold(const Problem &pb, const Caps &caps, const Switches &sw, int nrows, bool pairs)
{
	auto entries = [&](double per_nnz_k) { return std::max(128, (int) std::min(per_nnz_k * (double) pb.nnz * (double) pb.K, 2e9)); };
	if (sw.sweep_long_set) return std::max(128, (int) std::min(sw.sweep_long, 2e9));
	const bool pairs_long = pairs && pair_long_rows(pb, nrows) && sw.sweep_pair != 1;
	const int t_side = pairs_long ? entries(16e-6) : entries(caps.pf ? 6e-6 : 4e-6);
	const long long mean4 = std::min<long long>(4 * (long long) (pb.nnz / std::max(nrows, 1)), 2000000000ll);
	return std::max(t_side, (int) mean4);
}

// With the wave-pair form a long row is walked at ~0.055 us per entry at K=100 (a lone single wave: 0.13): when
// even the longest row's walk fits the sweep's bandwidth time the split buys nothing and costs the scratch
// round trip and a fork/join (cfg3 power-law users, longest row 2324: 0.160 -> 0.139 ms without the split).
inline bool longest_walk_fits(const Problem &pb, const Switches &sw, bool pairs, int longest)
{
	const double est_us = sweep_us(pb);
	return pairs && !sw.sweep_long_set && est_us >= 50.0 && (double) longest * 0.055 * pb.K / 100.0 <= 1.3 * est_us;
}

// The tiny sweep: below ~50 us of estimated bandwidth time the two-stream fork/join (tens of us on the 6000
// launches of ML100k) costs more than the split saves: one cooperative launch for all rows there.
inline bool tiny_sweep(const Problem &pb, const Switches &sw, int nrows)
{
	return sweep_us(pb) < 50.0 && nrows < 4096 && !sw.sweep_long_set;
}
// ... its entries per chunk and LDS request (nch = 0: the variant has no cooperative form, or fewer than 8 entries fit)
struct CoopForm {
	int nch = 0;
	size_t lds = 0;
};
inline CoopForm coop_form(const Caps &caps, const Switches &sw)
{
	const size_t per_entry = 2 * (size_t) caps.coop_producers * (size_t) caps.row_bytes, head = (size_t) caps.xs_bytes;
	int nl = (int) std::min<size_t>(32, (caps.lds_per_cu - 4096 - head) / per_entry);
	if (const int v = sw.sweep_nch; v >= 1 && head + (size_t) v * per_entry <= caps.lds_per_cu) nl = v;
	const int nc = (int) std::min<size_t>(32, (48 * 1024) / per_entry);
	if (!caps.coop || !(nc >= 8 || sw.sweep_nch)) return CoopForm{};
	const int n = sw.sweep_nch ? nl : nc;
	return CoopForm{n, head + (size_t) n * per_entry};
}

// The scratch cap: the scratch buffer holds K doubles per entry of every extreme row: keep it under a quarter of the free
// memory by raising the threshold (on Netflix-like data most entries sit in long columns)
inline int scratch_cap(const Problem &pb, const Caps &caps, const Rows &rows, int threshold)
{
	const size_t nsl = slice_count(pb.K, caps.slice_cols);
	const size_t cap_entries = std::max<size_t>(pb.free_bytes() / 4 / (nsl * caps.slice_cols * 8), 1);
	int t_eff = threshold;
	for (;;) {
		size_t ent = 0;
		for (int r = 0; r < rows.nrows; ++r)
			if (rows.len(r) >= t_eff) ent += (size_t) rows.len(r);
		if (ent <= cap_entries || t_eff > (1 << 29)) break;
		t_eff *= 2;
	}
	return t_eff;
}

// longest first, rows of equal length in index order
inline void sort_longest_first(const Rows &rows, std::vector<int> &list)
{
	std::stable_sort(list.begin(), list.end(), [&](int x, int y) { return rows.len(x) > rows.len(y); });
}

// Everything the plan keeps of one side's schedule, as host vectors and scalars.
struct Side {
	int max_row_len = 0;   // longest column (item sweep) / longest user row (user sweep)
	bool pair = false;     // pair_wanted of this side
	bool coop_all = false, lpt = false, use_db = false, use_pair = false;
	int long_len = 0;      // a row at least this long is on the extreme-row path (when long_rows is not empty)
	int prio_len = 0;
	std::vector<int> long_rows;    // the extreme rows, longest first
	std::vector<int> short_rows;   // beside extreme rows: the other rows, longest first; lpt: ALL rows in dispatch order
	std::vector<int> seg_row, seg_beg, seg_end, lr_cnt;
	std::vector<long long> seg_out, lr_sbeg;
	long long long_entries = 0;   // entries of the extreme rows = the side's scratch need
};

// The 64-entry segments of the extreme rows; scratch offsets in entry units, rows back to back.
// Entries per segment of the products launch: one wave walks a segment chunk by chunk (~2.5 us per 16 entries
// of exposed latency), so short segments finish sooner and there are more of them to overlap
// (cfg3 power-law: 256 -> 64 entries 0.452 -> 0.421 ms per iteration; Netflix-shaped 21.6 -> 21.4 ms)
inline void cut_segments(const Rows &rows, Side &s)
{
	constexpr int kSeg = 64;
	long long off = 0;
	for (int r : s.long_rows) {
		const int b = rows.ptr[r], e = rows.ptr[(size_t) r + 1];
		s.lr_sbeg.push_back(off);
		s.lr_cnt.push_back(e - b);
		for (int c = b; c < e; c += kSeg) {
			s.seg_row.push_back(r);
			s.seg_beg.push_back(c);
			s.seg_end.push_back(std::min(e, c + kSeg));
			s.seg_out.push_back(off + (c - b));
		}
		off += e - b;
	}
	s.long_entries = off;
}

// The skew-aware split of one side: rows whose serial walk would dominate the launch go to the extreme-row path
// (products launch + ordered sums on a side stream), the others stay on the main launch; or the whole tiny sweep is
// one cooperative launch; or, most often, nothing.
inline void split_side(const Problem &pb, const Caps &caps, const Switches &sw, const Rows &rows, const CoopForm &coop, Side &s)
{
	const int threshold = long_threshold(pb, caps, sw, rows.nrows, s.pair);
	if (s.max_row_len < threshold) return;
	if (longest_walk_fits(pb, sw, s.pair, s.max_row_len)) return;
	if (tiny_sweep(pb, sw, rows.nrows)) {
		s.coop_all = coop.nch > 0;
		return;
	}
	const int t_eff = scratch_cap(pb, caps, rows, threshold);
	if (s.max_row_len < t_eff) return;
	for (int r = 0; r < rows.nrows; ++r) (rows.len(r) >= t_eff ? s.long_rows : s.short_rows).push_back(r);
	// longest first: workgroups are dispatched in list order as slots free up, so the long walks start
	// at once and the short rows fill in behind them (longest-processing-time-first scheduling)
	sort_longest_first(rows, s.short_rows);
	sort_longest_first(rows, s.long_rows);
	s.long_len = t_eff;
	cut_segments(rows, s);
}

// Wave priority for the long rows of the main launch (what the launch ends on): when the launch is skewed
// (its longest row at least four times its mean), rows of at least twice the mean run at raised priority.
// The launch = the rows that are not on the extreme-row path.
inline int priority_length(const Rows &rows, const Side &s)
{
	const bool split = !s.long_rows.empty();
	const long long n = split ? (long long) s.short_rows.size() : rows.nrows;
	const long long ent = (long long) (rows.nrows ? rows.ptr[rows.nrows] - rows.ptr[0] : 0) - s.long_entries;
	const int longest = !split ? s.max_row_len : s.short_rows.empty() ? 0 : rows.len(s.short_rows[0]);
	const long long mean = n ? ent / n : 0;
	return n > 256 && longest >= 4 * std::max<long long>(mean, 1) ? (int) std::max<long long>(64, 2 * mean) : 0;
}

// The form of the main launch.  Double-buffered single-wave form for the WHOLE launch: measured slower than the
// single-buffered form whenever the launch has more rows than double-tile workgroups fit the chip (cfg3 uniform 0.222 ->
// 0.429 ms: the second tile halves the resident workgroups and the CU's gather rate is shared by fewer requests in
// flight), so it is off unless forced (MF_SWEEP_DB=1).  Else the wave-pair form where pair_wanted says so.
inline void main_launch_form(const Caps &caps, const Switches &sw, const Rows &rows, Side &s)
{
	const int launch_rows = !s.long_rows.empty() ? (int) s.short_rows.size() : rows.nrows;
	s.use_db = caps.db && !s.coop_all && launch_rows > 0 && sw.sweep_db == 1;
	s.use_pair = !s.coop_all && !s.use_db && launch_rows > 0 && s.pair;
}

// The dispatch order of a sweep without extreme rows.  A sweep of a few thousand rows is a handful of rounds of
// workgroups: in index order its tail is whatever long rows happen to start last.  Longest first (workgroups are
// dispatched in list order) the tail is made of the shortest rows.  cfg3 uniform (3952 / 6040 rows of 50..311 entries):
// see DESIGN 5.1.  Large sweeps keep the index order (the tail is a negligible part of them and neighbouring rows share
// lines of the entry arrays) except for rows several times longer than the average, which lead the list.
inline void dispatch_order(const Problem &pb, const Rows &rows, Side &s)
{
	const int nrows = rows.nrows;
	if (!s.long_rows.empty() || s.coop_all || nrows < 512) return;
	std::vector<int> &order = s.short_rows;
	order.reserve((size_t) nrows);
	if (nrows <= (1 << 15)) {   // a dozen rounds of workgroups at most: the tail matters, the order of the row reads does not
		for (int r = 0; r < nrows; ++r) order.push_back(r);
		sort_longest_first(rows, order);
	} else {
		// a large sweep with a few very long rows (power-law users): only those move to the front
		const long long mean = pb.nnz / nrows;
		if ((long long) s.max_row_len < 8 * std::max<long long>(mean, 1)) return;
		std::vector<int> head;
		for (int r = 0; r < nrows; ++r) (rows.len(r) >= 4 * mean ? head : order).push_back(r);
		sort_longest_first(rows, head);
		order.insert(order.begin(), head.begin(), head.end());
	}
	s.lpt = true;
}

// The schedule of both sweeps (side 0 = items / CSC, 1 = users / CSR).
struct Sweeps {
	Side side[2];
	CoopForm coop;                // the cooperative form, when a side is coop_all
	bool extreme = false;         // a side has extreme rows: the products form, the scratch and the side stream are needed
	int prod_nch = 0;             // the products launch: entries per chunk and LDS request
	size_t prod_lds = 0;
	size_t scratch_entries = 0;   // [slice][entry][slice_cols doubles]; one block of padding per slice: the last block of a row is read whole
	// Priority of the side stream.  Beside the single-wave form: high -- the ordered sums are few, latency-bound waves that
	// must get their slots ahead of the thousands of workgroups of the sweep they run under.  Beside the wave-pair form: LOW
	// -- there the launch ends on the pairs of the long rows, which must be dispatched at once, and the
	// side path has the whole other sweep to hide under (cfg3 power-law 0.304 -> 0.268 ms).
	bool side_low = false;
};

inline Sweeps sweep_schedule(const Problem &pb, const Caps &caps, const Switches &sw, const Rows rows[2])
{
	Sweeps out;
	const bool split = caps.prod && sw.skew;   // MF_SWEEP_SKEW=0 disables the split
	const CoopForm coop = split ? coop_form(caps, sw) : CoopForm{};
	for (int kind = 0; kind < 2; ++kind) {
		Side &s = out.side[kind];
		s.max_row_len = rows[kind].longest();
		s.pair = pair_wanted(pb, caps, sw, rows[kind].nrows, s.max_row_len);
		if (split) split_side(pb, caps, sw, rows[kind], coop, s);
		s.prio_len = priority_length(rows[kind], s);
		main_launch_form(caps, sw, rows[kind], s);
		dispatch_order(pb, rows[kind], s);
	}
	const Side &a = out.side[0], &b = out.side[1];
	if (a.coop_all || b.coop_all) out.coop = coop;
	out.extreme = !a.long_rows.empty() || !b.long_rows.empty();
	if (out.extreme) {
		out.prod_nch = caps.single_nch;
		out.prod_lds = (size_t) caps.xs_bytes + (size_t) caps.single_nch * caps.row_bytes;
		out.scratch_entries = (size_t) std::max(a.long_entries, b.long_entries) + caps.block_entries;
		out.side_low = a.pair || b.pair;
	}
	return out;
}

// ---- the choice of a sweep's main launch, made at every launch (launch_sweep, mf_launch.hip.h): a kernel instance is a
// cell of the variant's grid fn[form][flavour] (mf_plan.hip.h), launched in the geometry of its form
enum Form { kPlain, kPipelined, kPair, kDb, kCoop, kForms };
// What an instance does at the seed and the finished row: kAccumulate seeds with x as it is; kDecay multiplies the seed by d,
// keeps a frozen column and clamps; kMomentum adds the heavy-ball term; the W twins read per-entry weights, and come last.
enum Flavour { kAccumulate, kDecay, kMomentum, kDecayW, kMomentumW, kFlavours };
constexpr int kUnweightedFlavours = kDecayW;
// Where a launch takes its entries per chunk, LDS request and workgroup size from.
enum Geometry { kGeomSingle, kGeomFew, kGeomPair, kGeomDb, kGeomCoop, kGeomCoopSingleNch };

// Accumulate form of a single-wave launch: true for the form with the pipelined phases, false for the plain one.  Up to
// 262144 rows: the form whose phases keep their LDS reads in flight and whose gather issue is lean -- what a wave walking a
// long row alone is bound by (cfg3 uniform 0.224 -> 0.201 ms, power-law 0.367 -> 0.350, a lone 5993-entry row 1.02 -> 0.78
// ms).  Larger launches of one-pass rows (K <= 128) are never bound by one wave and keep round 2's form (cfg4 user sweep,
// 1e6 rows: 11.45 vs 11.60 ms).  Two-pass rows (K = 256) take it at every size: their phase A is a 256-deep chain per chunk
// that the six resident workgroups of a CU do not hide, and keeping its LDS reads in flight shortens it (cfg5: 346.6 ->
// 327.9 ms, 0.745 -> 0.787).
inline bool single_wave_pipelined(bool has_pipelined, int K, int n_short, int nrows)
{
	constexpr int kPfRows = 262144;
	return has_pipelined && (K > 128 || (n_short <= kPfRows && nrows <= kPfRows));
}

// The form: cooperative, double-buffered or wave-pair where the schedule chose one, else single-wave, pipelined or plain.
inline Form launch_form(bool coop_all, bool use_db, bool use_pair, bool pipelined)
{
	return coop_all ? kCoop : use_db ? kDb : use_pair ? kPair : pipelined ? kPipelined : kPlain;
}

// The flavour.  `momentum`: a seeded sweep of a side with beta != 0.  `decay`: d != 1.0, or the side has a frozen column or
// a box constraint (x * 1.0 is x: the rest runs the accumulate instance).  A weighted plan runs kDecayW at d = 1.0 too.
inline Flavour launch_flavour(bool weighted, bool momentum, bool decay)
{
	if (weighted) return momentum ? kMomentumW : kDecayW;
	return momentum ? kMomentum : decay ? kDecay : kAccumulate;
}

// The geometry: each form its own; the single-wave forms at the large chunk when `few_rows`.  A cooperative launch that is
// not one of few rows runs at the single-wave chunk size with the cooperative LDS request, as it always has.  Known and left
// for a change of its own: at K = 30 and K = 50 that request is sized for fewer rows (14 and 8) than the chunk's 16.
inline Geometry launch_geometry(Form form, bool few_rows)
{
	if (form == kCoop) return few_rows ? kGeomCoop : kGeomCoopSingleNch;
	return form == kDb ? kGeomDb : form == kPair ? kGeomPair : few_rows ? kGeomFew : kGeomSingle;
}

// ---- the user sweep in item bands (profiles/user_bands/README.md): every user's row is walked in `bands`
// consecutive item ranges, one launch per band, so the table a launch gathers from is 1/bands of Y and an XCD's L2 holds
// that much more of it.  Band b holds the items [band_first(b), band_first(b + 1)): equal ranges, empty ones where
// items < bands.  The partial row is handed from launch to launch through X_new; the chain of adds per element is the same
// chain in the same order, and an FP64 store and load between two adds is exact: the same bits as one launch.
constexpr int kBandsMax = 4096;                   // largest MF_SWEEP_BANDS
constexpr long long kBandTableBytes = 1ll << 30;  // ... and no band table above 1 GiB
constexpr int band_first(int b, int items, int bands) { return (int) ((long long) b * items / bands); }

// The offset cut: the first entry of [beg, end) -- item ids ascending -- whose id is at least first_item (end: none).
// Entry offsets of row r: off[b][r] = band_cut(idx, ptr[r], ptr[r + 1], band_first(b)), b = 0 .. bands.
constexpr int band_cut(const int *idx, int beg, int end, int first_item)
{
	while (beg < end) {
		const int mid = beg + ((end - beg) >> 1);
		if (idx[mid] < first_item)
			beg = mid + 1;
		else
			end = mid;
	}
	return beg;
}

// The band count the size rule picks (0: the rule is off).  Measured on cfg4 (1e6 x 1e5, K = 100, 100 entries per row, R 80
// MB; two runs each on one MI355X, profiles/user_bands/README.md), user sweep in ms by bands:
//   1 launch 11.61 | 2: 11.27 | 3: 11.44 | 4: 12.03 | 6: 13.56 | 8: 15.11 | 10: 16.81 | 12: 18.85 | 16: 23.37
// A band costs every row one more chain of dependent loads in front of its first gather and, on average, one more
// partly filled chunk -- about 0.85 ms per band on this shape --: two bands gain 0.34 ms, three 0.16, four and more lose.
// Against the parent commit, three alternating pairs: 23.32 .. 23.34 -> 23.10 .. 23.12 ms per iteration.
constexpr int kBandsRule = 2;
// ... and the fewest entries per row and band, on average, at which the rule runs them: two full 16-entry chunks, so that
// the chunk a band adds stays under a third of its work.  Reasoned from the table above, which still gains at 33 per band
// (three bands) and loses at 25 (four); no other row length was measured.
constexpr int kBandFloor = 32;
// ... and the largest Y, in L2 sizes, for which it does: what a band gains is the part of its table the caches hold, and
// the one table measured is 2.4 of them (80 MB against 32 MiB); a table many times larger would keep the cost and lose the gain.
constexpr int kBandYMaxL2 = 4;

struct BandInput {
	bool user_side = false;     // side 1, the CSR
	bool sorted = false;        // item ids ascending inside every row (the plan keeps no mask_idx)
	bool weighted = false;      // plan created with per-entry weights
	bool extreme = false;       // the side has extreme rows
	bool single_wave = false;   // the main launch is a single-wave one: not the pair, double-buffered or cooperative form
	bool fixed_k = false;       // K has a compile-time single-wave LDS-DMA instance
	int nrows = 0, items = 0;
	long long nnz = 0;
	int longest_column = 0;     // entries of the most rated item (the item side's longest row)
	size_t y_bytes = 0;         // items x pitch x 8
	size_t l2_bytes = 0;        // the chip's L2, all XCDs
	int forced = -1;            // MF_SWEEP_BANDS (-1: unset)
};

// Are the gathers spread evenly over Y?  The longest column under four times the mean one (the skew test of priority_length).
// Where a few items take most entries their rows of Y are served from L2 as it is, and the bands only cost: cfg4 with Zipf
// columns, user sweep 9.95 ms in one launch, 10.75 in two bands.
inline bool band_columns_even(const BandInput &in)
{
	return (long long) in.longest_column < 4 * std::max<long long>(in.nnz / std::max(in.items, 1), 1);
}

// Bands of a side, decided when the plan is created: 0, or the count whose offset table the plan builds.  The form must
// allow them; then MF_SWEEP_BANDS=n sets the count, and unset the size rule does: Y larger than the chip's L2 but no more than
// kBandYMaxL2 of them, gathered evenly, and rows long enough.
inline int band_count(const BandInput &in)
{
	if (!in.user_side || !in.sorted || in.weighted || in.extreme || !in.single_wave || !in.fixed_k) return 0;
	if (in.nrows <= 0 || in.items <= 0 || in.nnz <= 0) return 0;
	int bands = kBandsRule;
	if (in.forced >= 0)
		bands = std::min(in.forced, kBandsMax);
	else if (bands < 1 || in.y_bytes <= in.l2_bytes || in.y_bytes > kBandYMaxL2 * in.l2_bytes || !band_columns_even(in) || in.nnz / in.nrows / bands < kBandFloor)
		bands = 0;
	if ((long long) (bands + 1) * in.nrows * (long long) sizeof(int) > kBandTableBytes) bands = 0;
	return bands;
}

// ... and at every launch of the side: the bands run only for a seeded sweep of the plain flavour -- no decay, frozen column
// or bounds (kDecay), no momentum, no weights -- that is not the unseeded launch of an adaptive side.  An unseeded sweep (the
// non-root contribution of a sharded driver) keeps its one launch.
constexpr bool bands_at_launch(int bands, int seed, Flavour flavour, bool adaptive)
{
	return bands > 0 && seed == 1 && flavour == kAccumulate && !adaptive;
}

// ---- how an iteration runs (mf_plan_iterate, mf_hip.hip): one rule picks the loop and how much of it is replayed from a
// captured graph; mf_plan_iterate only dispatches on the result (tests/test_iterate_path.py)

// LDS bytes of the toy loop (sweep_resident_kernel, mf_sweep.hip.h): both generations of L and R, the entries in CSR and in
// CSC order -- value and index, 12 bytes, with the weight 20 --, the two row-pointer arrays and 64 bytes of slack.
constexpr size_t toy_lds_bytes(int users, int items, int K, long long nnz, bool weighted = false)
{
	return (size_t) 2 * (size_t) (users + items) * K * 8 + (size_t) nnz * 2 * (weighted ? 20 : 12) + (size_t) (users + items + 2) * 4 + 64;
}

// Register-row class of sweep_resident_kernel for this K in a workgroup of `threads`: 4, 16 or 32 (K <= class, the owner keeps
// its row in registers), 0 for the generic instance.  The K <= 32 instance is bounded to 256 threads by its
// __launch_bounds__, hence the guard.  No toy instance reaches it: more than 256 threads are users + items >= 257, which
// with K >= 17 need at least 16 * 257 * 17 = 69 904 bytes, over the 60 KiB bound of iterate_path (the test enumerates it).
constexpr int toy_kmax(int K, int threads) { return K <= 4 ? 4 : K <= 16 ? 16 : K <= 32 && threads <= 256 ? 32 : 0; }

enum Loop { kLoopAls, kLoopToy, kLoopEs, kLoopSweeps };
// `replays` replays of a captured body of kGraphIters iterations of `loop`, then `eager` iterations launched one by one.
// An even body, so the ping-pong parity of the generations returns to where it started and every replay starts alike.
constexpr int kGraphIters = 32;
struct IteratePath {
	Loop loop;
	int replays, eager;
};

struct IterateInput {
	bool als = false;          // an ALS kind is set
	bool whole = false;        // whole-instance plan: u0 == 0 && uc == users_total
	long long rows = 0;        // uc + items
	size_t toy_bytes = 0;      // toy_lds_bytes of the plan, unweighted
	long long nnz = 0;
	int K = 0, iters = 0;
	bool timing = false;       // per-launch timing is on
	bool adaptive = false;     // a side has an adaptive step size
	bool es_mode = false;      // the plan holds the errors + streams tables
	bool extreme = false;      // a side has extreme rows (n_long > 0)
	bool resident = true, graph = true;   // MF_RESIDENT, MF_GRAPH
	double graph_max = 2e6;               // MF_GRAPH_MAX
};

inline IteratePath iterate_path(const IterateInput &in)
{
	// ALS: eager launches, no graph
	if (in.als) return {kLoopAls, 0, in.iters};
	const double work = (double) in.nnz * in.K;   // multiply-adds of a sweep
	// Toy regime (inst0/1/2: a dozen entries, 1e5 iterations): the whole instance fits the LDS of one workgroup -> one launch
	// runs all the iterations with a workgroup barrier in between.
	const bool toy = in.whole &&                            // thread t owns factor row t: every row of both sides
	                 in.rows > 0 && in.rows <= 1024 &&      // ... one thread each
	                 // The unweighted footprint: weights do not alter which loop a plan takes.  The request of a weighted plan
	                 // holds 16 bytes more per entry, at most 2 KiB where the footprint is near its bound, since nnz * K <= 512:
	                 // never above 64 KiB.
	                 in.toy_bytes <= 60 * 1024 &&
	                 // Only while an iteration is a few hundred multiply-adds: measured through the CLI, inst1 0.70 -> 0.33 s and
	                 // inst2 0.47 -> 0.21 s, but inst30-40 (170 entries x K=10) 0.32 -> 0.39 s -- one workgroup on an otherwise
	                 // idle chip runs slowly, and two graph-replayed launches per iteration win again.
	                 work <= 512.0 &&
	                 !in.timing &&                          // one launch has no per-sweep times
	                 in.iters >= 8 && in.resident &&
	                 !in.adaptive;                          // the toy loop seeds unconditionally; an adaptive side's sweep is the unseeded one
	if (toy) return {kLoopToy, 0, in.iters};
	// errors + streams seeds unconditionally too: the two sweeps while a side is adaptive, whatever the plan's tables say
	const Loop loop = in.es_mode && !in.adaptive ? kLoopEs : kLoopSweeps;
	// Launch-bound regime (inst1: 100000 iterations of a 13-entry instance, ~4 us per launch): capture kGraphIters
	// iterations into a HIP graph and replay it.  Only for small sweeps -- a large one is not launch-bound and a graph would
	// pin its arguments for nothing --, never with per-launch timing (its events are host calls), nor beside extreme rows.
	const bool replay = work < in.graph_max && !in.timing && !in.extreme && in.iters >= 4 * kGraphIters && in.graph;
	if (!replay) return {loop, 0, in.iters};
	return {loop, in.iters / kGraphIters, in.iters % kGraphIters};
}

// ---- errors + streams iteration (mf_stream.hip.h, mf_resident.hip.h)

// The errors launch: the CSR rows cut into segments of at most nch entries, one wave each; nch = what a third of a
// CU's LDS holds, 64 at the most (nch = 0: not even one row fits, no tables).
struct EsErrors {
	int nch = 0;
	size_t lds = 0;
	std::vector<int> seg_row, seg_beg, seg_end;
};
inline EsErrors es_errors(const Caps &caps, const Rows &users)
{
	EsErrors e;
	const size_t row_bytes = (size_t) caps.row_bytes, head = (size_t) caps.xs_bytes;
	const int nch = (int) std::min<size_t>(64, (caps.lds_per_cu / 3 - head) / row_bytes);
	if (nch < 1) return e;
	e.nch = nch;
	e.lds = head + (size_t) nch * row_bytes;
	for (int u = 0; u < users.nrows; ++u)
		for (int c = users.ptr[u]; c < users.ptr[(size_t) u + 1]; c += nch) {
			e.seg_row.push_back(u);
			e.seg_beg.push_back(c);
			e.seg_end.push_back(std::min(users.ptr[(size_t) u + 1], c + nch));
		}
	return e;
}

// Run boundaries of one side of the streams launch: greedy on cost = entries + 16 per row; a run never splits a row and
// never holds more than max_rows rows (its row pointers live in one register), so a side of many short rows gets more
// workgroups than one per CU and slice.  The number of runs is a multiple of `waves` (empty runs at the end).
inline std::vector<int> es_run_cuts(const Rows &rows, int target_runs, int max_rows, int waves)
{
	std::vector<int> cut(1, 0);
	const int nrows = rows.nrows;
	constexpr double row_cost = 16.0;   // entries a row end is worth
	const double total_cost = (double) rows.ptr[(size_t) nrows] + row_cost * nrows;
	double acc_cost = 0, done = 0;
	int in_run = 0;
	for (int r = 0; r < nrows; ++r) {
		acc_cost += rows.len(r) + row_cost;
		++in_run;
		const int left = target_runs - (int) cut.size();
		const bool share = left > 0 && acc_cost >= (total_cost - done) / (left + 1);
		if (r + 1 < nrows && (share || in_run == max_rows)) {
			cut.push_back(r + 1);
			done += acc_cost;
			acc_cost = 0;
			in_run = 0;
		}
	}
	cut.push_back(nrows);
	while (((int) cut.size() - 1) % waves != 0) cut.push_back(nrows);
	return cut;
}

// The workgroup table of the LDS-resident streams launch: ~one workgroup per CU; every (side, slice) gets `per`
// workgroups of kWaves waves, and the side's rows are cut into per * kWaves runs of consecutive rows balanced by cost.
// Wg = the kernel's record {side, slice, row_beg[kWaves + 1], ent_beg[kWaves + 1]}.
template <class Wg, int kWaves>
std::vector<Wg> es_workgroups(const Rows rows[2], int K, int slice_width, int ncu, int max_rows)
{
	const int nsl = (K + slice_width - 1) / slice_width;
	const int per = std::max(1, ncu / (2 * nsl));
	std::vector<Wg> wgs;
	for (int side = 0; side < 2; ++side) {
		const std::vector<int> cut = es_run_cuts(rows[side], per * kWaves, max_rows, kWaves);   // every wave of a workgroup owns rows
		const int nwg_side = ((int) cut.size() - 1) / kWaves;
		for (int sl = 0; sl < nsl; ++sl)
			for (int w = 0; w < nwg_side; ++w) {
				Wg g;
				g.side = side;
				g.slice = sl;
				for (int i = 0; i <= kWaves; ++i) {
					g.row_beg[i] = cut[(size_t) (w * kWaves + i)];
					g.ent_beg[i] = rows[side].ptr[(size_t) g.row_beg[i]];
				}
				if (g.row_beg[kWaves] > g.row_beg[0]) wgs.push_back(g);
			}
	}
	return wgs;
}

// LDS request of that launch: the slice of the larger factor plus every wave's buffers
inline size_t es_resident_lds(int yrows_max, int slice_width, int waves, int wave_lds)
{
	return (size_t) yrows_max * slice_width * 8 + (size_t) waves * wave_lds;
}

// ---- the form of a conjugate-gradient ALS solve (mf_als_cg.hip.h), chosen at every launch.  Every form gives the same bits.
//   fixed    compile-time K, LDS-DMA gather: the K the sweeps have instances for;
//   dma      run-time even K, LDS-DMA gather;
//   general  any K from 1 to 256, the only form of an odd K: the gathered rows go through registers.
// The values are the indices of kAlsCgForm (mf_plan.hip.h) and what MF_ALS_CG_FORM=fixed|dma|general stores.
enum AlsCgFormId { kAlsCgFixed = 0, kAlsCgDma = 1, kAlsCgGeneral = 2, kAlsCgForms = 3 };
constexpr int kAlsCgMaxK = 256;
constexpr bool als_cg_fixed_k(int K) { return K == 10 || K == 20 || K == 30 || K == 50 || K == 100 || K == 128 || K == 256; }
// does `form` take this K?
constexpr bool als_cg_takes(int form, int K)
{
	if (K < 1 || K > kAlsCgMaxK) return false;
	return form == kAlsCgFixed ? als_cg_fixed_k(K) : form == kAlsCgDma ? (K & 1) == 0 : form == kAlsCgGeneral;
}
// The forced form where it takes the K; otherwise the most special form that does: LDS-DMA moves a gathered row without a
// register or an LDS store, and a compile-time K unrolls phase A with its reads in flight.
constexpr AlsCgFormId als_cg_form(int K, int forced)
{
	if (forced >= 0 && forced < kAlsCgForms && als_cg_takes(forced, K)) return (AlsCgFormId) forced;
	return als_cg_takes(kAlsCgFixed, K) ? kAlsCgFixed : als_cg_takes(kAlsCgDma, K) ? kAlsCgDma : kAlsCgGeneral;
}
// Entries per chunk: the sweeps' rule (chunk_rule, mf_launch.hip.h) -- 16, or what a sixth of a CU's LDS holds behind `head`
// bytes but at least 12 -- because a wave here alternates "gather a chunk" and "compute on it" exactly as a sweep's does, and
// the bytes in flight per CU come from the other resident workgroups.
constexpr int als_cg_chunk(size_t head, size_t row_bytes, size_t lds_per_cu)
{
	const size_t budget = lds_per_cu / 6;
	if (head + 16 * row_bytes <= budget) return 16;
	const size_t fit = budget > head ? (budget - head) / row_bytes : 0;
	return fit > 12 ? (int) fit : 12;
}

// ---- which ALS solve a launch runs: the one rule over the plan's kind (mf_plan_set_als; kAlsImplicitKind is the header's
// MF_ALS_IMPLICIT, mf_plan.hip.h asserts it), the steps of mf_plan_set_als_cg, those of mf_plan_set_implicit_cg and the sweeps
// of mf_plan_set_als_box.  The steps of the explicit kinds come first and make the solve theirs; the implicit steps count under
// the implicit kind alone; the box sweeps count where no steps are in force (the setters refuse the two together) and turn the
// direct solve's Cholesky into coordinate descent (mf_als_box.hip.h).  The launch, mf_plan_describe and the setters all read it:
// a setter refuses the state whose solve does not take the plan's K, and the implicit kind where the solve would not be an
// implicit one.
constexpr int kAlsImplicitKind = 4;
constexpr int kAlsDirectMaxK = 128;   // the direct solve keeps a row's triangle in LDS (mf_als.hip.h: kAlsMaxK)
struct AlsSolver {
	bool cg;         // conjugate gradient (mf_als_cg.hip.h); otherwise the direct solve (mf_als.hip.h)
	bool implicit;   // S and the confidence beside the arguments
	int steps;       // conjugate-gradient steps per row, 0 for the direct solve
	int max_k;       // the widest K it takes
	int box_sweeps;  // coordinate-descent sweeps per row of the direct solve (mf_als_box.hip.h), 0 for every other solve
};
constexpr AlsSolver als_solver(int als_kind, int als_cg, int implicit_cg, int als_box = 0)
{
	if (als_cg > 0) return {true, false, als_cg, kAlsCgMaxK, 0};
	const bool implicit = als_kind == kAlsImplicitKind;
	if (implicit && implicit_cg > 0) return {true, true, implicit_cg, kAlsDirectMaxK, 0};
	return {false, implicit, 0, kAlsDirectMaxK, als_box > 0 ? als_box : 0};
}

}  // namespace mf_sched
