#!/bin/bash
R=${GRAFT_REPO_ROOT:-.}; O=$R/gpurun_out/r3n; mkdir -p $O; cd $R
python3 bench.py --full > $O/cfg4_n1_bench.json 2> $O/cfg4_n1_bench.err; python3 - $O/cfg4_n1_bench.json <<'PY'
import json,sys
d=json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1]); r=d["roofline"]; c=d["cpu_baseline"]
print("default line: ms", d["ms_per_step"], "value %.4g"%d["value"], "frac", r["frac"], "traffic", r["traffic"], "rec", d["recommend"]["tflops"], "cpu %.3g cores %d x%.0f"%(c["value"], c["cores"], c["gpu_over_cpu"]))
PY
python3 bench.py --columns zipf --steps 20 --warmup 3 --full --no-cpu-baseline --check > $O/cfg4_zipf_bench.json 2> $O/cfg4_zipf.err; python3 - $O/cfg4_zipf_bench.json <<'PY'
import json,sys
d=json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1]); r=d["roofline"]
print("zipf: ms", d["ms_per_step"], "frac", r["frac"], "item", r["item_sweep_ms"], "user", r["user_sweep_ms"], d["check"], r["kernel"].split("long_rows")[1][:30], "rec", d["recommend"]["tflops"])
PY
bash tools/pmc_traffic.sh cfg5_n1 --config cfg5 --no-recommend > $O/cfg5_pmc.txt 2>&1; tail -12 $O/cfg5_pmc.txt
TRACE_OUT=$O/trace_skew.txt bash tools/trace_skew.sh > /dev/null 2>&1; cat $O/trace_skew.txt
bash tools/run_samples.sh $O/cli_all_samples.txt > /dev/null 2>&1; cat $O/cli_all_samples.txt
