// mf_config.hip.h -- every environment switch of the library, read ONCE per plan (mf_plan_create / the level-1 calls /
// mf_backend_run_multi) into a struct the plan keeps.  Nothing reads the environment per launch or per iteration, so a
// plan's behaviour is fixed at its creation and mf_plan_describe prints the switches that differ from their defaults.
//
// Every switch is documented and selects between forms the library SHIPS: the
// tests force each form through them and bench.py --check uses them for its reference run.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

namespace {

struct mf_config {
	enum IterMode { kIterAuto, kIterSweeps, kIterEs };
	IterMode iter_mode = kIterAuto;   // MF_ITER_MODE=auto|sweeps|es: two sweeps or errors + resident streams
	bool sweep_reg = false;           // MF_SWEEP_IMPL=reg: register-staged sweep only
	bool skew = true;                 // MF_SWEEP_SKEW=0: no split of long rows
	bool sweep_long_set = false;      // MF_SWEEP_LONG=<entries>: a row at least this long takes the extreme-row path
	double sweep_long = 0.0;
	int sweep_nch = 0;                // MF_SWEEP_NCH=<1..64>: entries per chunk (0: the rule of choose_sweep)
	int sweep_db = -1;                // MF_SWEEP_DB=0|1: intra-wave double-buffered sweep off / forced (-1: by occupancy)
	int sweep_pair = -1;              // MF_SWEEP_PAIR=0|1: wave-pair sweep (loader + compute wave per row) off / forced (-1: by the plan)
	int sweep_bands = -1;             // MF_SWEEP_BANDS=<n>: the user sweep in n item bands, 0 off (-1: the rule of mf_schedule.h)
	int es_sw = 0;                    // MF_ES_SW=8|4|2: slice width of the resident streams launch to try first
	bool row_pitch = true;            // MF_ROW_PITCH=0: dense device rows
	bool resident = true;             // MF_RESIDENT=0: no single-launch loop for toy instances
	bool graph = true;                // MF_GRAPH=0: no HIP-graph replay of small iterations
	double graph_max = 2e6;           // MF_GRAPH_MAX: nnz*K below which iterations are replayed from a graph
	bool rec_exact = false;           // MF_RECOMMEND_IMPL=exact: the exact recommendation kernel only
	bool rec_ares = true;             // MF_RECOMMEND_ARES=0: no LDS-resident L image in the MFMA pass
	bool rec_bdma = true;             // MF_RECOMMEND_BDMA=0: R chunks staged through registers
	int rec_half = 1;                 // MF_RECOMMEND_HALF=0: no 64-user workgroups (two per CU) in the MFMA pass; all: also for
	                                  // K that is no multiple of 20 (the general form of that kernel: slower than the 128-user one)
	int rec_split = -1;               // MF_RECOMMEND_SPLIT=0|n: item split of small recommendations off / n splits (-1: rule)
	bool build_host = false;          // MF_BUILD=host: CSR/CSC bucketed on the host
	bool os_dpp = true;               // MF_OS_DPP=0: ordered sums by plain v_add_f64 (no DPP broadcast)
	int als_form = -1;                // MF_ALS_FORM=wg|wave: the ALS solve as one workgroup / one wave per row (-1: by K)
	int als_cg_form = -1;             // MF_ALS_CG_FORM=fixed|dma|general: the form of the conjugate-gradient ALS solve (-1: by K)
	bool multi_force = false;         // MF_MULTI_FORCE=1: sharded path even with one shard
	bool multi_rccl = false;          // MF_MULTI_REDUCE=rccl|peer
	bool multi_threads = true;        // MF_MULTI_THREADS=0: all shards enqueued from the calling thread

	static bool is0(const char *v) { return v && v[0] == '0'; }
	static bool eq(const char *v, const char *s) { return v && strcmp(v, s) == 0; }

	static mf_config from_env()
	{
		mf_config c;
		const char *v;
		if ((v = getenv("MF_ITER_MODE"))) c.iter_mode = eq(v, "sweeps") ? kIterSweeps : eq(v, "es") ? kIterEs : kIterAuto;
		c.sweep_reg = eq(getenv("MF_SWEEP_IMPL"), "reg");
		c.skew = !is0(getenv("MF_SWEEP_SKEW"));
		if ((v = getenv("MF_SWEEP_LONG"))) {
			c.sweep_long_set = true;
			c.sweep_long = atof(v);
		}
		if ((v = getenv("MF_SWEEP_NCH"))) {
			const int n = atoi(v);
			if (n >= 1 && n <= 64) c.sweep_nch = n;
		}
		if ((v = getenv("MF_SWEEP_DB"))) c.sweep_db = is0(v) ? 0 : 1;
		if ((v = getenv("MF_SWEEP_PAIR"))) c.sweep_pair = is0(v) ? 0 : 1;
		if ((v = getenv("MF_SWEEP_BANDS"))) c.sweep_bands = atoi(v) > 0 ? atoi(v) : 0;
		if ((v = getenv("MF_ES_SW"))) c.es_sw = atoi(v);
		c.row_pitch = !is0(getenv("MF_ROW_PITCH"));
		c.resident = !is0(getenv("MF_RESIDENT"));
		c.graph = !is0(getenv("MF_GRAPH"));
		if ((v = getenv("MF_GRAPH_MAX"))) c.graph_max = atof(v);
		c.rec_exact = eq(getenv("MF_RECOMMEND_IMPL"), "exact");
		c.rec_ares = !is0(getenv("MF_RECOMMEND_ARES"));
		c.rec_bdma = !is0(getenv("MF_RECOMMEND_BDMA"));
		if ((v = getenv("MF_RECOMMEND_HALF"))) c.rec_half = is0(v) ? 0 : eq(v, "all") ? 2 : 1;
		if ((v = getenv("MF_RECOMMEND_SPLIT"))) c.rec_split = atoi(v);
		c.build_host = eq(getenv("MF_BUILD"), "host");
		c.os_dpp = !is0(getenv("MF_OS_DPP"));
		if ((v = getenv("MF_ALS_FORM"))) c.als_form = eq(v, "wg") ? 0 : eq(v, "wave") ? 1 : -1;
		if ((v = getenv("MF_ALS_CG_FORM"))) c.als_cg_form = eq(v, "fixed") ? 0 : eq(v, "dma") ? 1 : eq(v, "general") ? 2 : -1;
		c.multi_force = eq(getenv("MF_MULTI_FORCE"), "1");
		c.multi_rccl = eq(getenv("MF_MULTI_REDUCE"), "rccl");
		c.multi_threads = !is0(getenv("MF_MULTI_THREADS"));
		return c;
	}

	// the switches that differ from their defaults, for mf_plan_describe ("" when none does)
	std::string describe() const
	{
		const mf_config d;
		std::string s;
		auto add = [&](const char *name, const std::string &val) { s += std::string(s.empty() ? "" : ",") + name + "=" + val; };
		if (iter_mode != d.iter_mode) add("MF_ITER_MODE", iter_mode == kIterSweeps ? "sweeps" : "es");
		if (sweep_reg) add("MF_SWEEP_IMPL", "reg");
		if (!skew) add("MF_SWEEP_SKEW", "0");
		if (sweep_long_set) add("MF_SWEEP_LONG", std::to_string(sweep_long));
		if (sweep_nch) add("MF_SWEEP_NCH", std::to_string(sweep_nch));
		if (sweep_db >= 0) add("MF_SWEEP_DB", std::to_string(sweep_db));
		if (sweep_pair >= 0) add("MF_SWEEP_PAIR", std::to_string(sweep_pair));
		if (sweep_bands >= 0) add("MF_SWEEP_BANDS", std::to_string(sweep_bands));
		if (es_sw) add("MF_ES_SW", std::to_string(es_sw));
		if (!row_pitch) add("MF_ROW_PITCH", "0");
		if (!resident) add("MF_RESIDENT", "0");
		if (!graph) add("MF_GRAPH", "0");
		if (graph_max != d.graph_max) add("MF_GRAPH_MAX", std::to_string(graph_max));
		if (rec_exact) add("MF_RECOMMEND_IMPL", "exact");
		if (!rec_ares) add("MF_RECOMMEND_ARES", "0");
		if (!rec_bdma) add("MF_RECOMMEND_BDMA", "0");
		if (rec_half != 1) add("MF_RECOMMEND_HALF", rec_half ? "all" : "0");
		if (rec_split >= 0) add("MF_RECOMMEND_SPLIT", std::to_string(rec_split));
		if (build_host) add("MF_BUILD", "host");
		if (!os_dpp) add("MF_OS_DPP", "0");
		if (als_form >= 0) add("MF_ALS_FORM", als_form ? "wave" : "wg");
		if (als_cg_form >= 0) add("MF_ALS_CG_FORM", als_cg_form == 0 ? "fixed" : als_cg_form == 1 ? "dma" : "general");
		if (multi_force) add("MF_MULTI_FORCE", "1");
		if (multi_rccl) add("MF_MULTI_REDUCE", "rccl");
		if (!multi_threads) add("MF_MULTI_THREADS", "0");
		return s;
	}
};

}  // namespace
