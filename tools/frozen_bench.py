#!/usr/bin/env python3
"""Times one plan's iteration with and without frozen columns, in one process.  After a warm-up, --reps rounds of four
interleaved settings, each from freshly uploaded factors: lambda = 0 unfrozen (the plain instances), lambda = 0 frozen (the
decay instances at d = 1.0), lambda > 0 unfrozen, lambda > 0 frozen; the frozen columns are the bias convention, users' K-1
and items' K-2.  An iteration is timed by the plan's own events (mf_plan_timing_read: item_ms + user_ms).  Shapes as in
tools/reg_bench.py: cfg4, nflx, cfg4z (Zipf columns: extreme rows and ordered sums), ml100k (errors + streams); and toy, the
bundled inst0 sample, whose --toy-iters iterations run inside ONE launch that a timed plan never takes: there the host
clock goes around iterate() and a synchronise.  Prints one line per round and a JSON summary with median, minimum, maximum
and spread per series, the ratios of medians and of minima, and the kernel-source hash."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k", "toy"])
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--lambda-users", type=float, default=0.05)
ap.add_argument("--lambda-items", type=float, default=0.3)
ap.add_argument("--toy-iters", type=int, default=5000)
a = ap.parse_args()
c = rs.capi
toy = a.config == "toy"
if a.config in ("ml100k", "toy"):
    path = bench.CONFIGS["ml100k"]["file"] if a.config == "ml100k" else os.path.join(ROOT, "tests", "golden", "inst0.in")
    inst = c.parse_file(path)
    U, I, K, alpha, row, col, val = inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val
elif a.config == "nflx":
    cfg = bench.CONFIGS["nflx"]
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = bench.power_law_large(cfg["seed"], U, I, cfg["power_law_nnz"])
else:
    cfg = dict(bench.CONFIGS["cfg4"])
    columns = "zipf" if a.config == "cfg4z" else "uniform"
    if columns == "zipf":
        cfg["alpha"] = cfg["alpha"] * 0.5 * (cfg["min_row"] + cfg["max_row"]) / cfg["users"]
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = c.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, columns))
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.upload(L0, R0)
print(plan.describe(), flush=True)
SETTINGS = [("plain", (0.0, 0.0), (-1, -1)), ("frozen", (0.0, 0.0), (K - 1, K - 2)),
            ("reg", (a.lambda_users, a.lambda_items), (-1, -1)), ("reg_frozen", (a.lambda_users, a.lambda_items), (K - 1, K - 2))]


def one(lam, frozen):
    plan.set_regularization(*lam)
    plan.set_frozen_columns(*frozen)
    plan.upload(L0, R0)
    if toy:
        plan.synchronize()
        t0 = time.perf_counter()
        plan.iterate(a.toy_iters)
        plan.synchronize()
        return (time.perf_counter() - t0) * 1e3
    plan.iterate(1)
    t = plan.timing_read()
    return t["item_ms"] + t["user_ms"]


if not toy:
    plan.timing(True)
for _, lam, frozen in SETTINGS:   # warm-up: every instance any setting launches
    one(lam, frozen)
    one(lam, frozen)
series = {name: [] for name, _, _ in SETTINGS}
for r in range(a.reps):
    for name, lam, frozen in SETTINGS:
        series[name].append(one(lam, frozen))
    print("round %2d  " % r + "  ".join("%s %9.4f ms" % (name, series[name][-1]) for name, _, _ in SETTINGS), flush=True)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x)), "raw": x}


def ratio(x, y):
    return {"medians": float(np.median(series[x]) / np.median(series[y])), "minima": min(series[x]) / min(series[y])}


print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": int(len(row)), "reps": a.reps,
                  "lambda": [a.lambda_users, a.lambda_items], "frozen": [K - 1, K - 2], "unit": "ms per %d iteration(s)" % (a.toy_iters if toy else 1),
                  "kernel_source_hash": c.kernel_source_hash(), "series": {k: stats(v) for k, v in series.items()},
                  "frozen_over_plain": ratio("frozen", "plain"), "reg_over_plain": ratio("reg", "plain"),
                  "reg_frozen_over_reg": ratio("reg_frozen", "reg")}))
