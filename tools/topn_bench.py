#!/usr/bin/env python3
"""Times mf_plan_recommend and mf_plan_recommend_topn(N) in the same process on a synthetic shard (default: the cfg4 shape,
1e6 x 1e5, K = 100), after a warm-up call of each, --reps repetitions each.  Prints one line per call and a JSON summary
(seconds, TFLOP/s at 2 U I K flop, exact-pass users, form); for rocprofv3 runs of the top-N kernels as well."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recommender_system_amd as rs

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--feats", type=int, default=100)
ap.add_argument("--ns", default="1,10,16,32")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
c = rs.capi
row, col, val = c.synth_block(0xC0FFEE + 4, a.users, a.items, 50, 150)
rng = np.random.default_rng(0)
L = rng.random((a.users, a.feats)) / a.feats
R = rng.random((a.items, a.feats)) / a.feats
plan = c.Plan(a.users, a.items, a.feats, 1e-4, row, col, val)
plan.upload(L, R)
plan.iterate(2)
flop = 2.0 * a.users * a.items * a.feats
out = {"users": a.users, "items": a.items, "feats": a.feats, "reps": a.reps, "top1": [], "topn": {}}
best = plan.recommend()   # warm-up
for r in range(a.reps):
    t = time.perf_counter()
    best = plan.recommend()
    dt = time.perf_counter() - t
    out["top1"].append(dt)
    print("recommend        %.4f s  %.2f TFLOP/s  exact-pass users %d" % (dt, flop / dt / 1e12, plan.recommend_info()), flush=True)
for n in [int(x) for x in a.ns.split(",")]:
    items = plan.recommend_topn(n, scores=False)   # warm-up
    assert np.array_equal(items[:, 0], best), "column 0 differs from recommend()"
    ts = []
    for r in range(a.reps):
        t = time.perf_counter()
        items = plan.recommend_topn(n, scores=False)
        dt = time.perf_counter() - t
        ts.append(dt)
        ex, form = plan.recommend_topn_info()
        print("recommend_topn %2d %.4f s  %.2f TFLOP/s  exact-pass users %d  form %d" % (n, dt, flop / dt / 1e12, ex, form), flush=True)
    out["topn"][n] = {"s": ts, "exact_pass_users": ex, "form": form, "ratio_to_top1": min(ts) / min(out["top1"])}
print(json.dumps(out))
