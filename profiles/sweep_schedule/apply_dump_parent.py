"""Temporary schedule dump for the library BEFORE mf_schedule.h existed: patches csrc/mf_build.hip.h of a checkout of that
commit (never committed there).  With MF_SCHED_DUMP=<file> set, plan_row_schedule and plan_es_schedule append the per-side
fields, the capability values, the free bytes they saw and every host vector just before its upload.
usage: python apply_dump_parent.py <checkout>/recommender-system_amd/csrc/mf_build.hip.h"""
import sys

path = sys.argv[1]
lines = open(path).read().split("\n")


def at(content, nth=0):
    hits = [i for i, l in enumerate(lines) if l.strip() == content]
    assert len(hits) > nth, content
    return hits[nth]


def insert(content, new, after=False, nth=0):
    i = at(content, nth)
    ind = lines[i][:len(lines[i]) - len(lines[i].lstrip("\t"))]
    lines[i + 1 if after else i:i + 1 if after else i] = [ind + n for n in new]


def replace(content, new):
    i = at(content)
    ind = lines[i][:len(lines[i]) - len(lines[i].lstrip("\t"))]
    lines[i:i + 1] = [ind + n for n in new]


def lists(*names):
    return ['sd_list(sd, sd_name(kind, "%s").c_str(), %s);' % (n, v) for n, v in names]


i = [k for k, l in enumerate(lines) if l.startswith("// Schedule of the two sweeps from the row lengths")][0]
lines[i:i] = '''#include <sys/syscall.h>
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
template <class T> static void sd_list(FILE *f, const char *name, const std::vector<T> &v)
{
	if (!f) return;
	fprintf(f, "%s %zu", name, v.size());
	for (auto x : v) fprintf(f, " %lld", (long long) x);
	fprintf(f, "\\n");
}
static std::string sd_name(int kind, const char *n) { return "s" + std::to_string(kind) + "." + n; }
'''.split("\n")
insert("for (int u = 0; u < p->uc; ++u) p->max_row_len[1] = std::max(p->max_row_len[1], rptr[(size_t) u + 1] - rptr[u]);", [
    'FILE *sd = sd_open();',
    'if (sd) {',
    '\tfprintf(sd, "plan %d %lld %d %d\\n", p->K, (long long) p->nnz, p->items, p->uc);',
    '\tfprintf(sd, "caps %d %d %d %d %d %d %d %d\\n", p->sweep.prod != nullptr, p->sweep.pf != nullptr, p->sweep.pair != nullptr,',
    '\t        p->sweep.coop != nullptr, p->sweep.db != nullptr, p->sweep.row_bytes, p->sweep.xs_bytes, p->single.nch);',
    '\tfprintf(sd, "consts %d %d %d %d %d %zu\\n", mf::kCoopProducers, mf::kCoopWaves, mf::kSliceCols, mf::kBlockEntries, mf::kWave, kLdsPerCu);',
    '\tfprintf(sd, "switches %d %d %d %.17g %d %d\\n", (int) p->cfg.skew, p->cfg.sweep_nch, (int) p->cfg.sweep_long_set, p->cfg.sweep_long,',
    '\t        p->cfg.sweep_pair, p->cfg.sweep_db);',
    '}'])
insert("(void) hipMemGetInfo(&free_b, &total_b);", ['if (sd) fprintf(sd, "free %d %zu\\n", kind, free_b);'], after=True)
insert("MF_TRY(p->long_rows[kind].alloc(lg.size()));", lists(("long_rows", "lg"), ("short_rows", "sh")))
insert("MF_TRY(p->seg_row[kind].alloc(srow.size()));", lists(("seg_row", "srow"), ("seg_beg", "sbeg"), ("seg_end", "send"), ("seg_out", "sout"),
                                                            ("lr_sbeg", "lbeg"), ("lr_cnt", "lcnt")))
insert("const bool side_low = pair_wanted(p, 0) || pair_wanted(p, 1);", ['if (sd) fprintf(sd, "side_low %d\\n", (int) side_low);'], after=True)
insert("MF_TRY(p->short_rows[kind].alloc(order.size()));", lists(("short_rows", "order")))
i = at("p->lpt[kind] = true;")
assert lines[i + 2].strip() == "return MF_OK;"
lines[i + 2:i + 2] = ["\t" + n for n in [
    'if (sd) {',
    '\tfor (int kind = 0; kind < 2; ++kind)',
    '\t\tfprintf(sd, "side %d %d %d %d %d %d %d %d %d %d %d %d\\n", kind, kind == 0 ? p->items : p->uc, p->max_row_len[kind], p->prio_len[kind],',
    '\t\t        (int) p->lpt[kind], p->n_long[kind], p->n_short[kind], p->long_len[kind], p->n_seg[kind], (int) p->coop_all[kind],',
    '\t\t        (int) p->use_db[kind], (int) p->use_pair[kind]);',
    '\tfprintf(sd, "sched %d %zu %d %zu %d %zu\\n", p->coop.nch, p->coop.lds, p->coop.fn ? p->coop.block : 0, p->scratch_entries, p->prod.nch, p->prod.lds);',
    '\tfclose(sd);',
    '}']]
# errors + streams
insert("p->es_mode = false;", [
    'FILE *sd = sd_open();',
    'auto sd_done = [&]() {',
    '\tif (!sd) return;',
    '\tfprintf(sd, "es %d %d %zu %d %d %d %zu\\n", (int) p->es_mode, p->es_nch, p->es_lds_errors, p->es_nseg, p->res_sw, p->res_nwg, p->res_lds);',
    '\tfclose(sd);',
    '\tsd = nullptr;',
    '};',
    'if (sd) fprintf(sd, "es_in %d %d\\n", (int) (p->want_map && p->csr2csc), p->res_sw);'], after=True)
replace("if (!p->want_map || !p->csr2csc) return MF_OK;", ["if (!p->want_map || !p->csr2csc) return sd_done(), MF_OK;"])
replace("if (nch < 1) return MF_OK;", ["if (nch < 1) return sd_done(), MF_OK;"])
replace("if (p->es_nseg == 0 || p->res_sw <= 0) return MF_OK;", [
    'if (sd) fprintf(sd, "ncu %d\\n", ncu);',
    'sd_list(sd, "es.seg_row", srow);',
    'sd_list(sd, "es.seg_beg", sbeg);',
    'sd_list(sd, "es.seg_end", send);',
    'if (p->es_nseg == 0 || p->res_sw <= 0) return sd_done(), MF_OK;'])
insert("p->res_nwg = (int) wgs.size();", [
    'if (sd) {',
    '\tstd::vector<int> flat;',
    '\tfor (const mf::SliceWg &g : wgs) {',
    '\t\tflat.push_back(g.side);',
    '\t\tflat.push_back(g.slice);',
    '\t\tfor (int i = 0; i <= mf::kResidentWaves; ++i) flat.push_back(g.row_beg[i]);',
    '\t\tfor (int i = 0; i <= mf::kResidentWaves; ++i) flat.push_back(g.ent_beg[i]);',
    '\t}',
    '\tsd_list(sd, "es.wg", flat);',
    '}'])
insert("p->es_mode = true;", ["sd_done();"], after=True)
open(path, "w").write("\n".join(lines))
