#!/bin/bash
# Round 3, final sources: everything under profiles/r03 that depends on the kernel sources, in one call on the GPU box.
# cfg4 kernel stats + the two PMC passes + bench line (tools/refresh_profiles.sh), cfg5 PMC, the traffic file staged in
# the box's copy so that the bench lines that follow carry `roofline.traffic`, the other configurations, the recommend
# kernel alone (kernel-trace stats, PMC), the power-law timeline.  Raw outputs under gpurun_out/; the caller copies.
R=$GRAFT_REPO_ROOT; cd $R; O=$R/gpurun_out/final3; rm -rf $O; mkdir -p $O
bash tools/refresh_profiles.sh > $O/refresh.txt 2>&1 || { tail -5 $O/refresh.txt; exit 1; }; tail -4 $O/refresh.txt | cut -c1-400
bash tools/pmc_traffic.sh cfg5_n1 --config cfg5 --no-recommend > $O/cfg5_pmc.txt 2>&1 || { tail -5 $O/cfg5_pmc.txt; exit 1; }
python3 - <<'PY'
import json, os, sys
R = os.environ["GRAFT_REPO_ROOT"]; sys.path.insert(0, R)
import recommender_system_amd as rs
t = json.load(open(R + "/profiles/pmc_traffic.json"))
t.update(json.load(open(R + "/gpurun_out/refresh/pmc_traffic_entry.json")))
s = json.load(open(R + "/gpurun_out/pmc_cfg5_n1/summary.json"))
sw = [v["hbm_bytes_per_launch"] for k, v in s["kernels"].items() if "sweep_dma_kernel" in k]
t["cfg5_n1"] = {"hbm_bytes_per_launch": sum(sw) / len(sw), "algorithmic_bytes_per_launch": s["algorithmic_bytes_per_launch"],
                "kernel_source_hash": rs.capi.kernel_source_hash(),
                "csvs": ["profiles/r03/cfg5_n1_pmc_FETCH_SIZE.csv", "profiles/r03/cfg5_n1_pmc_WRITE_SIZE.csv"],
                "method": "tools/pmc_traffic.sh cfg5_n1 --config cfg5: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes; "
                          "bytes = (2*FETCH_SIZE + WRITE_SIZE)*1024 per launch of the sweep kernel (MI355X_MICROARCH.md)"}
json.dump(t, open(R + "/profiles/pmc_traffic.json", "w"), indent=1)
json.dump(t, open(R + "/gpurun_out/final3/pmc_traffic.json", "w"), indent=1)
print("cfg5 PMC bytes per launch %.4g over algorithmic %.4g = %.3f" % (t["cfg5_n1"]["hbm_bytes_per_launch"], t["cfg5_n1"]["algorithmic_bytes_per_launch"],
                                                                         t["cfg5_n1"]["hbm_bytes_per_launch"] / t["cfg5_n1"]["algorithmic_bytes_per_launch"]))
PY
python3 bench.py --full > $O/cfg4_n1_bench.json 2> $O/cfg4_n1_bench.err || exit 1
python3 - $O/cfg4_n1_bench.json <<'PY'
import json,sys
d=json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1]); r=d["roofline"]; c=d["cpu_baseline"]
print("default line: ms", d["ms_per_step"], "value %.4g"%d["value"], "frac", r["frac"], "traffic", r["traffic"], "rec", d["recommend"]["tflops"], d["recommend"]["seconds"], "cpu %.3g cores %d x%.0f"%(c["value"], c["cores"], c["gpu_over_cpu"]))
PY
bash tools/config_benches.sh 2>&1 | tail -12
export TMPDIR=/tmp; cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/rec_stats -- python3 $R/tools/rec_bench.py --reps 3 > $O/rec_bench.txt 2>&1 || exit 1
python3 - <<PY
import csv, glob
f = glob.glob("$O/rec_stats/*/*kernel_stats.csv")[0]
rows = [r for r in csv.DictReader(open(f)) if "recommend" in r["Name"] or "row_norm" in r["Name"] or "merge" in r["Name"] or "pack" in r["Name"]]
with open("$O/recommend_kernel_stats.csv", "w") as g:
    w = csv.DictWriter(g, fieldnames=rows[0].keys()); w.writeheader(); w.writerows(rows)
for r in rows: print(r["Name"][:60], r["Calls"], "avg_ns", r["AverageNs"])
PY
cd $R; bash tools/rec_pmc.sh > $O/recommend_pmc.txt 2>&1; cat $O/recommend_pmc.txt | head -8
bash tools/rec_quick.sh > $O/recommend_k_sweep.txt 2>&1; cat $O/recommend_k_sweep.txt
TRACE_OUT=$O/cfg3_powerlaw_timeline.txt bash tools/trace_skew.sh > /dev/null 2>&1; cat $O/cfg3_powerlaw_timeline.txt
