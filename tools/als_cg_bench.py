#!/usr/bin/env python3
"""Times one plan's conjugate-gradient ALS iteration (mf_plan_set_als_cg) beside its direct ALS iteration and its gradient
iteration, in one process.  After a warm-up of every leg, --reps rounds of: factors uploaded afresh, one gradient iteration,
one direct ALS iteration (steps 0; skipped above K = 128, where the direct solve does not exist, and with --no-direct), then
one CG iteration per entry of --steps, each by the host clock around iterate(1) and a synchronise; then the two solves of every
CG leg apart.  Shapes as in tools/als_bench.py -- cfg4, nflx, cfg4z, ml100k -- and cfg5s: cfg5's K = 256 and row lengths at
2e5 x 2e5, 1e8 entries.  Prints one line per round and a JSON summary with median, minimum, maximum and spread per series,
each CG iteration as a multiple of the plan's gradient iteration next to the count steps + 1 of passes per side, the row
counters, and the kernel-source hash.

--quality (ml100k): from the reference's initialisation, the training RMSE after each of --iters iterations at every entry of
--steps and at steps 0, and per leg the iterations and wall time (a loss after every iteration) to the plain run's final
training RMSE."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k", "cfg5s"])
ap.add_argument("--kind", default="ridge", choices=["ridge", "ridge-count"])
ap.add_argument("--lam", type=float, default=0.05)
ap.add_argument("--steps", default="1,3,10")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-direct", action="store_true")
ap.add_argument("--quality", action="store_true")
ap.add_argument("--iters", type=int, default=8)
ap.add_argument("--max-iters", type=int, default=50)
a = ap.parse_args()
c = rs.capi
steps = [int(s) for s in a.steps.split(",")]
iters_of_file = 0
if a.config == "ml100k":
    inst = c.parse_file(bench.CONFIGS["ml100k"]["file"])
    U, I, K, alpha, row, col, val = inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val
    iters_of_file = inst.iters
elif a.config == "nflx":
    cfg = bench.CONFIGS["nflx"]
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = bench.power_law_large(cfg["seed"], U, I, cfg["power_law_nnz"])
else:
    cfg = dict(bench.CONFIGS["cfg5" if a.config == "cfg5s" else "cfg4"])
    columns = "zipf" if a.config == "cfg4z" else "uniform"
    if a.config == "cfg5s":
        cfg.update(users=200_000, items=200_000, nnz=100_000_000)
    if columns == "zipf":
        cfg["alpha"] = cfg["alpha"] * 0.5 * (cfg["min_row"] + cfg["max_row"]) / cfg["users"]
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = c.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, columns))
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.upload(L0, R0)
nnz = int(len(row))
longest = (int(np.bincount(row, minlength=U).max()), int(np.bincount(col, minlength=I).max()))
direct = K <= 128 and not a.no_direct


def rmse(lo):
    return float(np.sqrt(lo.sse / float(lo.count)))


def leg(s):
    """s: None the gradient iteration, 0 the direct solve, > 0 that many CG steps"""
    if s is None:
        plan.set_als("off")
        plan.set_als_cg(0)
        plan.set_regularization(0.0)
    else:
        plan.set_als("off")
        plan.set_als_cg(s)
        plan.set_als(a.kind)
        plan.set_regularization(a.lam)


def timed(call):
    plan.synchronize()
    t0 = time.perf_counter()
    call()
    plan.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


if a.quality:
    n = iters_of_file or 1000
    leg(None)
    plan.iterate(2)   # warm-up
    plan.upload(L0, R0)
    plain_ms = timed(lambda: plan.iterate(n))
    goal = rmse(plan.loss("train"))
    out = {"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "kind": a.kind, "lambda": a.lam,
           "plain": {"iterations": n, "train_rmse": goal, "wall_ms": plain_ms}, "legs": {}, "kernel_source_hash": c.kernel_source_hash()}
    for s in [0] + steps:
        leg(s)
        print(plan.describe(), flush=True)
        plan.upload(L0, R0)
        plan.iterate(1)   # warm-up of the launches
        plan.upload(L0, R0)
        plan.synchronize()
        t0 = time.perf_counter()
        done, at, curve, reached = 0, rmse(plan.loss("train")), [], None
        while done < a.max_iters and (done < a.iters or reached is None):
            plan.iterate(1)
            done += 1
            at = rmse(plan.loss("train"))
            curve.append(at)
            if reached is None and at <= goal:
                reached = {"iterations": done, "train_rmse": at, "wall_ms_with_a_loss_every_iteration": (time.perf_counter() - t0) * 1e3}
        out["legs"]["steps %d" % s] = {"train_rmse_after_%d" % a.iters: curve[a.iters - 1], "to_the_plain_rmse": reached,
                                       "train_rmse_by_iteration": curve}
    print(json.dumps(out))
    sys.exit(0)

legs = [None] + ([0] if direct else []) + steps
for s in legs:   # warm-up of every leg
    leg(s)
    if s:
        print(plan.describe(), flush=True)
    plan.iterate(1)
series = {s: [] for s in legs}
users, items = {s: [] for s in steps}, {s: [] for s in steps}
for k in range(a.reps):
    for s in legs:
        leg(s)
        plan.upload(L0, R0)
        series[s].append(timed(lambda: plan.iterate(1)))
    for s in steps:
        leg(s)
        plan.upload(L0, R0)
        users[s].append(timed(lambda: plan.als_solve("users", "current")))
        items[s].append(timed(lambda: plan.als_solve("items", "next")))
    print("round %2d  gradient %10.4f ms" % (k, series[None][-1]) + ("  direct %10.4f ms" % series[0][-1] if direct else "") +
          "".join("  cg%d %10.4f ms (users %10.4f, items %10.4f)" % (s, series[s][-1], users[s][-1], items[s][-1]) for s in steps), flush=True)
counts = {}
for s in steps:
    leg(s)
    plan.upload(L0, R0)
    plan.iterate(1)
    counts[s] = {"users": plan.als_info("users"), "items": plan.als_info("items")}
grad = float(np.median(series[None]))
print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "longest_row_users_items": longest,
                  "kind": a.kind, "lambda": a.lam, "reps": a.reps, "unit": "ms per iteration, host clock",
                  "kernel_source_hash": c.kernel_source_hash(), "iteration_gradient_ms": stats(series[None]),
                  "iteration_direct_ms": stats(series[0]) if direct else None,
                  "cg": {"steps %d" % s: {"iteration_ms": stats(series[s]), "user_solve_ms": stats(users[s]), "item_solve_ms": stats(items[s]),
                                          "gradient_iterations": float(np.median(series[s])) / grad, "passes_per_side": s + 1,
                                          "rows_solved_empty_not_pd": counts[s]} for s in steps}}))
