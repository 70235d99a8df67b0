#!/usr/bin/env python3
"""Times one plan's ALS iteration (mf_plan_set_als: the user solve against R, the item solve against the new L, the flip)
beside its gradient iteration, in one process.  After a warm-up of both, --reps rounds of: factors uploaded afresh, one
gradient iteration, then one ALS iteration, each by the host clock around iterate(1) and a synchronise (an ALS iteration is
two launches of tens of milliseconds and more; the plan's own events cover the sweeps only).  Shapes as in
tools/adaptive_bench.py: cfg4, nflx, cfg4z (Zipf columns: a few very long item rows, each one workgroup's serial chain),
ml100k.  Prints one line per round and a JSON summary with median, minimum, maximum and spread per series, the two solves
timed apart (--split: als_solve(users), synchronise, als_solve(items), synchronise), the row counters of the last
iteration, the ALU bound -- nnz * K (K + 1) / 2 * 2 lane operations per side over 256 CUs x 4 SIMDs x 16 FP64 lanes per clock
at --clock-ghz -- with the achieved fraction of it, and the kernel-source hash.

--target (ml100k): ALS iterations and wall time to the plain run's final training RMSE.  The plain run makes the instance
file's own iterations; the ALS run from the same start is monitored after every iteration and stops at the first point at or
below that RMSE."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k"])
ap.add_argument("--kind", default="ridge", choices=["ridge", "ridge-count"])
ap.add_argument("--lam", type=float, default=0.05)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--clock-ghz", type=float, default=2.4)
ap.add_argument("--target", action="store_true")
ap.add_argument("--max-iters", type=int, default=50)
a = ap.parse_args()
c = rs.capi
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
    cfg = dict(bench.CONFIGS["cfg4"])
    columns = "zipf" if a.config == "cfg4z" else "uniform"
    if columns == "zipf":
        cfg["alpha"] = cfg["alpha"] * 0.5 * (cfg["min_row"] + cfg["max_row"]) / cfg["users"]
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = c.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, columns))
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.upload(L0, R0)
nnz = int(len(row))
longest = (int(np.bincount(row, minlength=U).max()), int(np.bincount(col, minlength=I).max()))


def rmse(lo):
    return float(np.sqrt(lo.sse / float(lo.count)))


def als(on):
    plan.set_als(a.kind if on else "off")
    plan.set_regularization(a.lam if on else 0.0)


def timed(call):
    plan.synchronize()
    t0 = time.perf_counter()
    call()
    plan.synchronize()
    return (time.perf_counter() - t0) * 1e3


if a.target:
    n = iters_of_file or 1000
    plan.iterate(2)   # warm-up
    plan.upload(L0, R0)
    plain_ms = timed(lambda: plan.iterate(n))
    goal = rmse(plan.loss("train"))
    als(True)
    print(plan.describe(), flush=True)
    plan.upload(L0, R0)
    plan.iterate(1)   # warm-up of the ALS launches
    plan.upload(L0, R0)
    plan.synchronize()
    t0 = time.perf_counter()
    done, at, curve = 0, rmse(plan.loss("train")), []
    while at > goal and done < a.max_iters:
        plan.iterate(1)
        done += 1
        at = rmse(plan.loss("train"))
        curve.append(at)
    als_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "kind": a.kind, "lambda": a.lam,
                      "plain": {"iterations": n, "train_rmse": goal, "wall_ms": plain_ms},
                      "als": {"iterations": done, "train_rmse": at, "wall_ms_with_a_loss_every_iteration": als_ms,
                              "reached": bool(at <= goal), "train_rmse_by_iteration": curve},
                      "kernel_source_hash": c.kernel_source_hash()}))
    sys.exit(0)

als(True)
print(plan.describe(), flush=True)
for on in (False, True):   # warm-up of both
    als(on)
    plan.iterate(1)
plain, full, users, items = [], [], [], []
for k in range(a.reps):
    als(False)
    plan.upload(L0, R0)
    plain.append(timed(lambda: plan.iterate(1)))
    als(True)
    plan.upload(L0, R0)
    full.append(timed(lambda: plan.iterate(1)))
    plan.upload(L0, R0)
    users.append(timed(lambda: plan.als_solve("users", "current")))
    items.append(timed(lambda: plan.als_solve("items", "next")))
    print("round %2d  gradient %10.4f ms  als %10.4f ms  (user solve %10.4f, item solve %10.4f)" % (k, plain[-1], full[-1], users[-1], items[-1]),
          flush=True)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


lane_ops = 2.0 * nnz * (K * (K + 1) / 2) * 2.0   # both sides: a multiply and an add per element of the triangle and entry
bound_ms = lane_ops / (256 * 4 * 16 * a.clock_ghz * 1e9) * 1e3
print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "longest_row_users_items": longest,
                  "kind": a.kind, "lambda": a.lam, "reps": a.reps, "unit": "ms per iteration, host clock",
                  "kernel_source_hash": c.kernel_source_hash(), "iteration_gradient_ms": stats(plain), "iteration_als_ms": stats(full),
                  "user_solve_ms": stats(users), "item_solve_ms": stats(items),
                  "rows_solved_empty_not_pd": {"users": plan.als_info("users"), "items": plan.als_info("items")},
                  "alu_bound_ms": bound_ms, "clock_ghz": a.clock_ghz, "achieved_fraction_of_alu_bound": bound_ms / float(np.median(full))}))
