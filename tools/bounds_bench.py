#!/usr/bin/env python3
"""Times one plan's regularised iteration without and with a box constraint, in one process.  After a warm-up of both
settings, --reps rounds of: factors uploaded afresh, one timed iteration at the default bounds (the decay instances, the
clamp's columns = 0), then the same at [--lo, --hi] on both sides, the order of the two alternating from round to round.  An
iteration is timed by the plan's own events (mf_plan_timing_read: item_ms + user_ms).  Shapes as in tools/frozen_bench.py:
cfg4, nflx, cfg4z (Zipf columns: extreme rows and ordered sums), ml100k (errors + streams); and toy, the bundled inst0
sample, whose --toy-iters iterations run inside ONE launch that a timed plan never takes: there the host clock goes around
iterate() and a synchronise.  Prints one line per round and a JSON summary with median, minimum, maximum and spread per
series, the ratios of medians and of minima, and the kernel-source hash.

--costs: one mf_plan_project call and one mf_plan_bounds_active call on the users' side, host clock around the call and a
synchronise, beside the user sweep of the same plan (the plan's events).
--nmf (ml100k): record only -- held-out RMSE of a 90/10 split, bounds [0, inf) against unconstrained at equal iterations, and
the share of exact zeros in the NMF factors."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k", "toy"])
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--lambda-users", type=float, default=0.05)
ap.add_argument("--lambda-items", type=float, default=0.3)
ap.add_argument("--lo", type=float, default=0.0)
ap.add_argument("--hi", type=float, default=0.5)
ap.add_argument("--toy-iters", type=int, default=5000)
ap.add_argument("--costs", action="store_true")
ap.add_argument("--nmf", action="store_true")
ap.add_argument("--nmf-iters", type=int, default=200)
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
lam = (a.lambda_users, a.lambda_items)
INF = float("inf")


def rmse(lo):
    return float(np.sqrt(lo.sse / float(lo.count)))


if a.nmf:
    rng = np.random.default_rng(1)
    held = rng.random(len(row)) < 0.1
    out = {}
    for name, box in (("unconstrained", (-INF, INF)), ("nmf", (0.0, INF))):
        plan = c.Plan(U, I, K, alpha, row[~held], col[~held], val[~held])
        plan.set_heldout(row[held], col[held], val[held])
        plan.set_bounds("users", *box)
        plan.set_bounds("items", *box)
        plan.upload(L0, R0)
        plan.iterate(a.nmf_iters)
        L, R = plan.download()
        out[name] = {"train_rmse": rmse(plan.loss("train")), "heldout_rmse": rmse(plan.loss("heldout")),
                     "zeros_users": float((L == 0.0).mean()), "zeros_items": float((R == 0.0).mean()),
                     "bounds_active_users": plan.bounds_active("users"), "bounds_active_items": plan.bounds_active("items")}
        plan.close()
    print(json.dumps({"config": a.config, "iterations": a.nmf_iters, "heldout_entries": int(held.sum()), "results": out,
                      "kernel_source_hash": c.kernel_source_hash()}))
    sys.exit(0)

plan = c.Plan(U, I, K, alpha, row, col, val)
plan.set_regularization(*lam)
plan.upload(L0, R0)
print(plan.describe(), flush=True)
SETTINGS = {"unbounded": (-INF, INF), "bounded": (a.lo, a.hi)}


def one(box):
    plan.set_bounds("users", *box)
    plan.set_bounds("items", *box)
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


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x)), "raw": x}


if a.costs:
    plan.timing(True)
    plan.set_bounds("users", a.lo, a.hi)
    sweep, project, active = [], [], []
    for r in range(a.reps + 1):
        plan.upload(L0, R0)
        plan.iterate(1)
        t = plan.timing_read()
        plan.synchronize()
        t0 = time.perf_counter()
        plan.project("users")
        plan.synchronize()
        t1 = time.perf_counter()
        got = plan.bounds_active("users")
        t2 = time.perf_counter()
        if r:   # round 0 is the warm-up
            sweep.append(t["user_ms"])
            project.append((t1 - t0) * 1e3)
            active.append((t2 - t1) * 1e3)
    print(json.dumps({"config": a.config, "users": U, "feats": K, "bounds": [a.lo, a.hi], "bounds_active_users": got, "unit": "ms",
                      "user_sweep": stats(sweep), "project": stats(project), "bounds_active": stats(active),
                      "project_over_user_sweep": float(np.median(project) / np.median(sweep)),
                      "bounds_active_over_user_sweep": float(np.median(active) / np.median(sweep)),
                      "kernel_source_hash": c.kernel_source_hash()}))
    sys.exit(0)

if not toy:
    plan.timing(True)
for box in SETTINGS.values():   # warm-up of both settings
    one(box)
    one(box)
series = {name: [] for name in SETTINGS}
for r in range(a.reps):
    for name in (list(SETTINGS) if r % 2 == 0 else list(SETTINGS)[::-1]):
        series[name].append(one(SETTINGS[name]))
    print("round %2d  " % r + "  ".join("%s %9.4f ms" % (name, series[name][-1]) for name in SETTINGS), flush=True)
print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": int(len(row)), "reps": a.reps, "lambda": list(lam),
                  "bounds": [a.lo, a.hi], "unit": "ms per %d iteration(s)" % (a.toy_iters if toy else 1),
                  "kernel_source_hash": c.kernel_source_hash(), "series": {k: stats(v) for k, v in series.items()},
                  "bounded_over_unbounded": {"medians": float(np.median(series["bounded"]) / np.median(series["unbounded"])),
                                             "minima": min(series["bounded"]) / min(series["unbounded"])}}))
