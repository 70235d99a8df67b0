"""The same temporary dump as apply_dump_parent.py, for the tree WITH mf_schedule.h: the fields mapped one to one, printed
from the plan's per-side records and from the host vectors the rules returned, just before their upload.
usage: python apply_dump_new.py <checkout>/recommender-system_amd/csrc/mf_build.hip.h"""
import sys

path = sys.argv[1]
src = open(path).read()


def once(old, new):
    global src
    assert src.count(old) == 1, old
    src = src.replace(old, new)


once("// Schedule of the two sweeps from the row lengths, by the rules", '''#include <sys/syscall.h>
#include <unistd.h>
// ---- TEMPORARY schedule dump (MF_SCHED_DUMP=<file>, appended)
// MF_SCHED_DUMP_SPLIT=1: one file per process and thread (plans created from several threads or processes at once)
static FILE *sd_open()
{
	const char *f = getenv("MF_SCHED_DUMP");
	if (!f || !*f) return nullptr;
	std::string name = f;
	if (getenv("MF_SCHED_DUMP_SPLIT")) name += "." + std::to_string((long) getpid()) + "." + std::to_string((long) syscall(SYS_gettid));
	return fopen(name.c_str(), "a");
}
template <class T> static void sd_list(FILE *f, const std::string &name, const std::vector<T> &v)
{
	if (!f) return;
	fprintf(f, "%s %zu", name.c_str(), v.size());
	for (const T &x : v) fprintf(f, " %lld", (long long) x);
	fprintf(f, "\\n");
}

// Schedule of the two sweeps from the row lengths, by the rules''')
once('''	// ---- its tables on the device
''', '''	if (FILE *sd = sd_open()) {
		fprintf(sd, "plan %d %lld %d %d\\n", p->K, (long long) p->nnz, p->items, p->uc);
		fprintf(sd, "caps %d %d %d %d %d %d %d %d\\n", (int) caps.prod, (int) caps.pf, (int) caps.pair, (int) caps.coop, (int) caps.db,
		        caps.row_bytes, caps.xs_bytes, caps.single_nch);
		fprintf(sd, "consts %d %d %d %d %d %zu\\n", caps.coop_producers, caps.coop_waves, caps.slice_cols, caps.block_entries, caps.wave, caps.lds_per_cu);
		fprintf(sd, "switches %d %d %d %.17g %d %d\\n", (int) sw.skew, sw.sweep_nch, (int) sw.sweep_long_set, sw.sweep_long, sw.sweep_pair, sw.sweep_db);
		for (int kind = 0; kind < 2; ++kind) {
			const mf_sched::Side &h = s.side[kind];
			const std::string pre = "s" + std::to_string(kind) + ".";
			if (!h.long_rows.empty()) {
				sd_list(sd, pre + "long_rows", h.long_rows);
				sd_list(sd, pre + "seg_row", h.seg_row);
				sd_list(sd, pre + "seg_beg", h.seg_beg);
				sd_list(sd, pre + "seg_end", h.seg_end);
				sd_list(sd, pre + "seg_out", h.seg_out);
				sd_list(sd, pre + "lr_sbeg", h.lr_sbeg);
				sd_list(sd, pre + "lr_cnt", h.lr_cnt);
			}
			if (!h.long_rows.empty() || h.lpt) sd_list(sd, pre + "short_rows", h.short_rows);
			fprintf(sd, "side %d %d %d %d %d %zu %zu %d %zu %d %d %d\\n", kind, p->side[kind].nrows, h.max_row_len, h.prio_len, (int) h.lpt,
			        h.long_rows.size(), h.long_rows.empty() ? (size_t) 0 : h.short_rows.size(), h.long_len, h.seg_row.size(), (int) h.coop_all,
			        (int) h.use_db, (int) h.use_pair);
		}
		if (s.extreme) fprintf(sd, "side_low %d\\n", (int) s.side_low);
		fprintf(sd, "sched %d %zu %d %zu %d %zu\\n", s.coop.nch, s.coop.lds, s.coop.nch ? mf::kCoopWaves * mf::kWave : 0, s.scratch_entries,
		        s.prod_nch, s.prod_lds);
		fclose(sd);
	}
	// ---- its tables on the device
''')
# errors + streams: one closing line at every return, as in the parent's dump
once('''	p->es_mode = false;
	if (!p->want_map || !p->csr2csc) return MF_OK;''', '''	p->es_mode = false;
	FILE *sd = sd_open();
	auto sd_done = [&]() {
		if (!sd) return;
		fprintf(sd, "es %d %d %zu %d %d %d %zu\\n", (int) p->es_mode, p->es_nch, p->es_lds_errors, p->es_nseg, p->res_sw, p->res_nwg, p->res_lds);
		fclose(sd);
		sd = nullptr;
	};
	if (sd) fprintf(sd, "es_in %d %d\\n", (int) (p->want_map && p->csr2csc), p->res_sw);
	if (!p->want_map || !p->csr2csc) return sd_done(), MF_OK;''')
once("	if (e.nch < 1) return MF_OK;", "	if (e.nch < 1) return sd_done(), MF_OK;")
once("	if (p->es_nseg == 0 || p->res_sw <= 0) return MF_OK;", '''	sd_list(sd, "es.seg_row", e.seg_row);
	sd_list(sd, "es.seg_beg", e.seg_beg);
	sd_list(sd, "es.seg_end", e.seg_end);
	if (p->es_nseg == 0 || p->res_sw <= 0) return sd_done(), MF_OK;''')
once("	p->res_nwg = (int) wgs.size();", '''	if (sd) {
		fprintf(sd, "ncu %d\\n", ncu);
		std::vector<int> flat;
		for (const mf::SliceWg &g : wgs) {
			flat.push_back(g.side);
			flat.push_back(g.slice);
			for (int i = 0; i <= mf::kResidentWaves; ++i) flat.push_back(g.row_beg[i]);
			for (int i = 0; i <= mf::kResidentWaves; ++i) flat.push_back(g.ent_beg[i]);
		}
		sd_list(sd, "es.wg", flat);
	}
	p->res_nwg = (int) wgs.size();''')
once('''	p->es_mode = true;
	return MF_OK;''', '''	p->es_mode = true;
	sd_done();
	return MF_OK;''')
open(path, "w").write(src)
