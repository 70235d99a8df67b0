#!/usr/bin/env python3
"""Times one plan's box-constrained ALS iteration (mf_plan_set_als_box) beside its direct ALS iteration -- sweeps 0, which under
a box is project-after-solve -- alternating in one process.  After a warm-up of every leg, --reps rounds of: per entry of
0,--sweeps the factors uploaded afresh and one iteration, then the user solve and the item solve apart, each by the host clock
around the call and a synchronise.  Shapes as in tools/als_bench.py: cfg4, nflx, cfg4z, ml100k.  --kind ridge | ridge-count |
implicit (--conf).  The box is [--lo, --hi] on all columns of both sides (default [0, inf)).  Prints one line per round and a
JSON summary with median, minimum, maximum and spread per series, every box leg as a ratio of medians and of minima to the
direct leg, the row counters, and the kernel-source hash.

--quality (ml100k): a 90 / 10 split of the entries by --seed; from the reference's initialisation, for sweeps 0 and every entry
of --sweeps, after each of --iters iterations the training objective (the loss plus lambda times the squares; under the
implicit kind mf_plan_implicit_objective's), the held-out RMSE and the share of exact zeros in L and R."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k"])
ap.add_argument("--kind", default="ridge", choices=["ridge", "ridge-count", "implicit"])
ap.add_argument("--lam", type=float, default=0.05)
ap.add_argument("--conf", type=float, default=40.0)
ap.add_argument("--lo", type=float, default=0.0)
ap.add_argument("--hi", type=float, default=float("inf"))
ap.add_argument("--sweeps", default="1,2,4")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quality", action="store_true")
ap.add_argument("--iters", type=int, default=12)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()
c = rs.capi
sweeps = [int(s) for s in a.sweeps.split(",")]
if a.config == "ml100k":
    inst = c.parse_file(bench.CONFIGS["ml100k"]["file"])
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
held = None
if a.quality:
    pick = np.random.default_rng(a.seed).random(len(row)) < 0.1
    held = (row[pick], col[pick], val[pick])
    row, col, val = row[~pick], col[~pick], val[~pick]
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.set_regularization(a.lam)
plan.set_bounds("users", a.lo, a.hi)
plan.set_bounds("items", a.lo, a.hi)
if a.kind == "implicit":
    plan.set_confidence(a.conf)
plan.upload(L0, R0)
nnz = int(len(row))


def leg(s):
    plan.set_als("off")
    plan.set_als_box(s)
    plan.set_als(a.kind)


def timed(call):
    plan.synchronize()
    t0 = time.perf_counter()
    call()
    plan.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


if a.quality:
    plan.set_heldout(*held)
    out = {"config": a.config, "users": U, "items": I, "feats": K, "train": nnz, "heldout": int(len(held[0])), "kind": a.kind, "lambda": a.lam,
           "box": [a.lo, a.hi], "legs": {}, "kernel_source_hash": c.kernel_source_hash()}
    for s in [0] + sweeps:
        leg(s)
        print(plan.describe(), flush=True)
        plan.upload(L0, R0)
        curve = []
        for it in range(a.iters):
            plan.iterate(1)
            lu, li = plan.penalty()
            if a.kind == "implicit":
                all_sq, observed, _ = plan.implicit_objective()
                obj = all_sq + observed + a.lam * lu + a.lam * li
            else:
                obj = plan.loss("train").sse + a.lam * lu + a.lam * li      # ridge; under ridge-count the squares are not count-scaled here
            h = plan.loss("heldout")
            L, R = plan.download()
            curve.append({"iteration": it + 1, "objective": float(obj), "heldout_rmse": float(np.sqrt(h.sse / float(h.count))),
                          "zeros": float(((L == 0.0).sum() + (R == 0.0).sum()) / float(L.size + R.size))})
        out["legs"]["sweeps %d" % s] = curve
    print(json.dumps(out))
    sys.exit(0)

legs = [0] + sweeps
for s in legs:   # warm-up of every leg
    leg(s)
    print(plan.describe(), flush=True)
    plan.iterate(1)
series, users, items = ({s: [] for s in legs} for _ in range(3))
for k in range(a.reps):
    for s in legs:
        leg(s)
        plan.upload(L0, R0)
        series[s].append(timed(lambda: plan.iterate(1)))
    for s in legs:
        leg(s)
        plan.upload(L0, R0)
        users[s].append(timed(lambda: plan.als_solve("users", "current")))
        items[s].append(timed(lambda: plan.als_solve("items", "next")))
    print("round %2d" % k + "".join("  box%d %10.4f ms (users %10.4f, items %10.4f)" % (s, series[s][-1], users[s][-1], items[s][-1]) for s in legs),
          flush=True)
counts = {}
for s in legs:
    leg(s)
    plan.upload(L0, R0)
    plan.iterate(1)
    counts[s] = {"users": plan.als_info("users"), "items": plan.als_info("items")}


def ratio(x, s, f):
    return f(x[s]) / f(x[0])


print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "kind": a.kind, "lambda": a.lam, "box": [a.lo, a.hi],
                  "reps": a.reps, "unit": "ms, host clock", "kernel_source_hash": c.kernel_source_hash(),
                  "legs": {"sweeps %d" % s: {"iteration_ms": stats(series[s]), "user_solve_ms": stats(users[s]), "item_solve_ms": stats(items[s]),
                                             "to_direct_by_medians": {"iteration": ratio(series, s, np.median), "users": ratio(users, s, np.median),
                                                                      "items": ratio(items, s, np.median)},
                                             "to_direct_by_minima": {"iteration": ratio(series, s, min), "users": ratio(users, s, min),
                                                                     "items": ratio(items, s, min)},
                                             "rows_solved_empty_not_pd": counts[s]} for s in legs}}))
