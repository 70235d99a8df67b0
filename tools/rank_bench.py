#!/usr/bin/env python3
"""Times mf_plan_recommend and mf_plan_rank_heldout (one and --per held-out entries per user) in the same process on a
synthetic shard (--config cfg4: 1e6 x 1e5, K = 100; nflx: the Netflix-shaped power-law instance of bench.py; cfg5s: cfg5's
K = 256 and row lengths at 2e5 x 2e5), after two iterations from the reference's initial factors and a warm-up call of
each, --reps repetitions each.  Prints one line per call and a JSON summary (seconds, TFLOP/s at 2 rows I K flop,
exact-pass entries, form, the ratios t_rank1 / t_top1 and t_rankN / t_rank1, the metrics at cutoff 10, the kernel-source
hash); for rocprofv3 runs of the rank kernels as well."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg5s"])
ap.add_argument("--per", type=int, default=10, help="entries per user of the second measurement (0: skip it)")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
c = rs.capi
if a.config == "nflx":
    cfg = bench.CONFIGS["nflx"]
    row, col, val = bench.power_law_large(cfg["seed"], cfg["users"], cfg["items"], cfg["power_law_nnz"])
else:
    cfg = dict(bench.CONFIGS["cfg4" if a.config == "cfg4" else "cfg5"])
    if a.config == "cfg5s":
        cfg.update(users=200_000, items=200_000, nnz=100_000_000)
    row, col, val = c.synth_block(cfg["seed"], cfg["users"], cfg["items"], cfg["min_row"], cfg["max_row"],
                                  **bench.synth_args(cfg, "uniform"))
a.users, a.items, a.feats = cfg["users"], cfg["items"], cfg["feats"]
L, R = c.init_factors(a.users, a.items, a.feats)
plan = c.Plan(a.users, a.items, a.feats, cfg["alpha"], row, col, val)
plan.upload(L, R)
rng = np.random.default_rng(0)
plan.iterate(2)
out = {"config": a.config, "users": a.users, "items": a.items, "feats": a.feats, "reps": a.reps,
       "kernel_source_hash": c.kernel_source_hash(), "top1": [], "rank": {}}
flop1 = 2.0 * a.users * a.items * a.feats
plan.recommend()   # warm-up
for r in range(a.reps):
    t = time.perf_counter()
    plan.recommend()
    dt = time.perf_counter() - t
    out["top1"].append(dt)
    print("recommend          %.4f s  %.2f TFLOP/s  exact-pass users %d" % (dt, flop1 / dt / 1e12, plan.recommend_info()), flush=True)
for per in [1] + ([a.per] if a.per > 1 else []):
    # uniformly drawn items; the few draws that hit a training pair come back as MF_RANK_MASKED and are counted below
    hrow = np.repeat(np.arange(a.users, dtype=np.int32), per)
    hcol = rng.integers(0, a.items, hrow.shape[0]).astype(np.int32)
    plan.set_heldout(hrow, hcol, np.ones(hrow.shape[0]))
    rank = plan.rank_heldout()   # warm-up
    ts = []
    for r in range(a.reps):
        t = time.perf_counter()
        rank = plan.rank_heldout()
        dt = time.perf_counter() - t
        ts.append(dt)
        ex, form = plan.rank_heldout_info()
        print("rank_heldout x%-3d  %.4f s  %.2f TFLOP/s  exact-pass entries %d  form %d"
              % (per, dt, per * flop1 / dt / 1e12, ex, form), flush=True)
    m = c.rank_metrics(rank, hrow, 10)
    out["rank"][per] = {"s": ts, "exact_pass_entries": ex, "form": form, "evaluated": m.evaluated, "masked": m.masked,
                        "nan": m.nan, "hit_rate_at_10": m.hit_rate, "mrr": m.mrr, "ndcg_at_10": m.ndcg}
out["t_rank1_over_t_top1"] = min(out["rank"][1]["s"]) / min(out["top1"])
if a.per > 1:
    out["t_rankN_over_t_rank1"] = min(out["rank"][a.per]["s"]) / min(out["rank"][1]["s"])
print(json.dumps(out))
