#!/usr/bin/env python3
"""Times mf_plan_similar_items on plans that hold nothing but R: the cfg4 item shape (1e5 items, K = 100), the Netflix item
shape (17 770 items, K = 100) and K = 256 at 2e5 items.  Per shape: all items at n = 10 and n = 32 (both metrics: the
difference is similar_normalize_kernel) and listed queries of 1, 1 000 and 100 000 items at n = 10, after a warm-up call of
each, --reps repetitions each.  Prints one line per call (seconds, TFLOP/s at 2 nq items K flop, form, exact-pass queries)
and a JSON summary."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recommender_system_amd as rs

SHAPES = {"cfg4": (100_000, 100), "nflx": (17_770, 100), "k256": (200_000, 256)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="cfg4,nflx,k256")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
c = rs.capi
out = {}
for name in a.shapes.split(","):
    items, K = SHAPES[name]
    rng = np.random.default_rng(0)
    R = rng.random((items, K)) / K          # the factors' initial range (topn_bench.py)
    e = np.zeros(0, np.int32)
    plan = c.Plan(1, items, K, 1e-4, e, e, np.zeros(0))
    plan.upload(np.zeros((1, K)), R)
    calls = [("all", None, n, metric) for n in (10, 32) for metric in ("cosine", "dot")]
    calls += [("listed", rng.integers(0, items, nq).astype(np.int32), 10, "cosine") for nq in (1, 1_000, 100_000)]
    res = out[name] = {"items": items, "feats": K, "calls": []}
    for kind, query, n, metric in calls:
        nq = items if query is None else len(query)
        plan.similar_items(n, metric, query=query, scores=False)   # warm-up
        ts = []
        for r in range(a.reps):
            t = time.perf_counter()
            plan.similar_items(n, metric, query=query, scores=False)
            ts.append(time.perf_counter() - t)
        ex, form = plan.similar_items_info()
        best = min(ts)
        tf = 2.0 * nq * items * K / best / 1e12
        print("%-5s %-6s nq %6d n %2d %-6s  %.5f s  %6.2f TFLOP/s  form %d  exact-pass queries %d" %
              (name, kind, nq, n, metric, best, tf, form, ex), flush=True)
        res["calls"].append({"kind": kind, "nq": nq, "n": n, "metric": metric, "s": ts, "tflops": tf, "form": form,
                             "exact_pass_queries": ex})
    plan.close()
print(json.dumps(out))
