// schedule_main -- the schedule decisions of csrc/mf_schedule.h on one instance, printed in full (tests/test_schedule.py).
// Input file: K nnz items users, the capability values (Caps), the switches, free bytes, the inputs of the errors +
// streams tables, then the items' and the users' row pointers.  Output: one "name values..." line per record and list.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../recommender-system_amd/csrc/mf_schedule.h"

namespace {

constexpr int kWaves = 8;   // waves of a workgroup of the resident streams launch
struct Wg {
	int side, slice;
	int row_beg[kWaves + 1], ent_beg[kWaves + 1];
};

template <class T>
void list(const std::string &name, const std::vector<T> &v)
{
	printf("%s %zu", name.c_str(), v.size());
	for (const T &x : v) printf(" %lld", (long long) x);
	printf("\n");
}

bool read(FILE *f, long long &v) { return fscanf(f, "%lld", &v) == 1; }

}  // namespace

int main(int argc, char **argv)
{
	FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
	if (!f) return fprintf(stderr, "usage: schedule_main <input file>\n"), 2;
	long long h[18], t[6];
	double sweep_long = 0.0;
	for (int i = 0; i < 18; ++i)
		if (!read(f, h[i])) return 2;
	long long skew, nch, long_set, pair, db;
	if (!read(f, skew) || !read(f, nch) || !read(f, long_set) || fscanf(f, "%lf", &sweep_long) != 1 || !read(f, pair) || !read(f, db)) return 2;
	for (int i = 0; i < 6; ++i)
		if (!read(f, t[i])) return 2;
	mf_sched::Problem pb;
	pb.K = (int) h[0];
	pb.nnz = h[1];
	const int items = (int) h[2], users = (int) h[3];
	mf_sched::Caps caps;
	caps.prod = h[4], caps.pf = h[5], caps.pair = h[6], caps.coop = h[7], caps.db = h[8];
	caps.row_bytes = (int) h[9], caps.xs_bytes = (int) h[10], caps.single_nch = (int) h[11];
	caps.coop_producers = (int) h[12], caps.coop_waves = (int) h[13], caps.slice_cols = (int) h[14];
	caps.block_entries = (int) h[15], caps.wave = (int) h[16], caps.lds_per_cu = (size_t) h[17];
	mf_sched::Switches sw;
	sw.skew = skew, sw.sweep_nch = (int) nch, sw.sweep_long_set = long_set, sw.sweep_long = sweep_long;
	sw.sweep_pair = (int) pair, sw.sweep_db = (int) db;
	pb.free_bytes = [&t] { return (size_t) t[0]; };
	const bool es_enabled = t[1];
	const int res_sw = (int) t[2], ncu = (int) t[3], res_rows = (int) t[4], res_wave_lds = (int) t[5];
	std::vector<int> ptr[2];
	for (int kind = 0; kind < 2; ++kind) {
		ptr[kind].resize((size_t) (kind == 0 ? items : users) + 1);
		for (int &v : ptr[kind]) {
			long long x;
			if (!read(f, x)) return 2;
			v = (int) x;
		}
	}
	fclose(f);
	const mf_sched::Rows rows[2] = {{ptr[0].data(), items}, {ptr[1].data(), users}};

	printf("plan %d %lld %d %d\n", pb.K, pb.nnz, items, users);
	const mf_sched::Sweeps s = mf_sched::sweep_schedule(pb, caps, sw, rows);
	for (int kind = 0; kind < 2; ++kind) {
		const mf_sched::Side &d = s.side[kind];
		const std::string pre = "s" + std::to_string(kind) + ".";
		const bool split = !d.long_rows.empty();
		if (split) list(pre + "long_rows", d.long_rows);
		if (split || d.lpt) list(pre + "short_rows", d.short_rows);
		if (split) {
			list(pre + "seg_row", d.seg_row);
			list(pre + "seg_beg", d.seg_beg);
			list(pre + "seg_end", d.seg_end);
			list(pre + "seg_out", d.seg_out);
			list(pre + "lr_sbeg", d.lr_sbeg);
			list(pre + "lr_cnt", d.lr_cnt);
		}
		printf("side %d %d %d %d %d %zu %zu %d %zu %d %d %d\n", kind, rows[kind].nrows, d.max_row_len, d.prio_len, (int) d.lpt,
		       d.long_rows.size(), split ? d.short_rows.size() : (size_t) 0, d.long_len, d.seg_row.size(), (int) d.coop_all,
		       (int) d.use_db, (int) d.use_pair);
	}
	if (s.extreme) printf("side_low %d\n", (int) s.side_low);
	printf("sched %d %zu %d %zu %d %zu\n", s.coop.nch, s.coop.lds, s.coop.nch ? caps.coop_waves * caps.wave : 0, s.scratch_entries,
	       s.prod_nch, s.prod_lds);

	// errors + streams tables, with the early ends of plan_es_schedule
	int es_mode = 0, res_nwg = 0;
	size_t res_lds = 0;
	mf_sched::EsErrors e;
	if (es_enabled) e = mf_sched::es_errors(caps, rows[1]);
	if (e.nch >= 1) {
		list("es.seg_row", e.seg_row);
		list("es.seg_beg", e.seg_beg);
		list("es.seg_end", e.seg_end);
		if (!e.seg_row.empty() && res_sw > 0) {
			const std::vector<Wg> wgs = mf_sched::es_workgroups<Wg, kWaves>(rows, pb.K, res_sw, ncu, res_rows);
			std::vector<int> flat;
			for (const Wg &g : wgs) {
				flat.push_back(g.side);
				flat.push_back(g.slice);
				flat.insert(flat.end(), g.row_beg, g.row_beg + kWaves + 1);
				flat.insert(flat.end(), g.ent_beg, g.ent_beg + kWaves + 1);
			}
			list("es.wg", flat);
			res_nwg = (int) wgs.size();
			res_lds = mf_sched::es_resident_lds(std::max(users, items), res_sw, kWaves, res_wave_lds);
			es_mode = 1;
		}
	}
	printf("es %d %d %zu %zu %d %d %zu\n", es_mode, e.nch, e.lds, e.seg_row.size(), res_sw, res_nwg, res_lds);
	return 0;
}
