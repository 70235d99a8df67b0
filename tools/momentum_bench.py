#!/usr/bin/env python3
"""Times one plan's iteration without and with heavy-ball momentum, in one process.  After a warm-up of both settings,
--reps rounds of: factors uploaded afresh, one untimed iteration (with momentum it takes the side out of rest: the copy
current -> next is not part of a steady-state iteration), then one timed iteration -- at beta = 0, then at beta > 0.  An
iteration is timed by the plan's own events (mf_plan_timing_read: item_ms + user_ms).  Shapes as in tools/reg_bench.py: cfg4,
nflx, cfg4z (Zipf columns: extreme rows, the preparation launch and the ordered sums), ml100k (errors + streams); and toy,
the bundled inst0 sample, whose --toy-iters iterations run inside ONE launch that a timed plan never takes: there the host
clock goes around iterate() and a synchronise.  Prints one line per round and a JSON summary with median, minimum, maximum
and spread per series, the ratios of medians and of minima, and the kernel-source hash.

--target (ml100k, cfg3): iterations and wall time to the plain run's final training RMSE instead.  The plain run makes
--plain-iters iterations (the instance file's own count at ml100k); the momentum run is monitored every --every iterations
and stops at the first point at or below that RMSE."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k", "toy", "cfg3"])
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--beta-users", type=float, default=0.9)
ap.add_argument("--beta-items", type=float, default=0.9)
ap.add_argument("--toy-iters", type=int, default=5000)
ap.add_argument("--target", action="store_true")
ap.add_argument("--plain-iters", type=int, default=0)
ap.add_argument("--every", type=int, default=10)
a = ap.parse_args()
c = rs.capi
toy = a.config == "toy"
iters_of_file = 0
if a.config in ("ml100k", "toy"):
    path = bench.CONFIGS["ml100k"]["file"] if a.config == "ml100k" else os.path.join(ROOT, "tests", "golden", "inst0.in")
    inst = c.parse_file(path)
    U, I, K, alpha, row, col, val = inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val
    iters_of_file = inst.iters
elif a.config == "nflx":
    cfg = bench.CONFIGS["nflx"]
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = bench.power_law_large(cfg["seed"], U, I, cfg["power_law_nnz"])
else:
    cfg = dict(bench.CONFIGS["cfg3" if a.config == "cfg3" else "cfg4"])
    columns = "zipf" if a.config == "cfg4z" else "uniform"
    if columns == "zipf":
        cfg["alpha"] = cfg["alpha"] * 0.5 * (cfg["min_row"] + cfg["max_row"]) / cfg["users"]
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = c.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, columns))
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.upload(L0, R0)
print(plan.describe(), flush=True)
beta = (a.beta_users, a.beta_items)


def rmse(lo):
    return float(np.sqrt(lo.sse / float(lo.count)))


if a.target:
    n = a.plain_iters or iters_of_file or 1000
    plan.iterate(2)   # warm-up
    plan.upload(L0, R0)
    plan.synchronize()
    t0 = time.perf_counter()
    plan.iterate(n)
    plan.synchronize()
    plain_s = time.perf_counter() - t0
    goal = rmse(plan.loss("train"))
    plan.set_momentum(*beta)
    plan.upload(L0, R0)
    plan.synchronize()
    t0 = time.perf_counter()
    done, at = 0, rmse(plan.loss("train"))
    while at > goal and done < n:
        plan.iterate(a.every)
        done += a.every
        at = rmse(plan.loss("train"))
    mom_s = time.perf_counter() - t0
    print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": int(len(row)), "alpha": alpha, "beta": list(beta),
                      "plain": {"iterations": n, "train_rmse": goal, "wall_s": plain_s},
                      "momentum": {"iterations": done, "train_rmse": at, "wall_s_with_a_loss_every_%d" % a.every: mom_s,
                                   "reached": bool(at <= goal)},
                      "kernel_source_hash": c.kernel_source_hash()}))
    sys.exit(0)


def one(b):
    plan.set_momentum(*b)
    plan.upload(L0, R0)
    if toy:
        plan.iterate(8)   # out of rest, inside the single-launch loop
        plan.synchronize()
        t0 = time.perf_counter()
        plan.iterate(a.toy_iters)
        plan.synchronize()
        return (time.perf_counter() - t0) * 1e3
    plan.iterate(1)
    plan.timing_read()
    plan.iterate(1)
    t = plan.timing_read()
    return t["item_ms"] + t["user_ms"]


if not toy:
    plan.timing(True)
for b in ((0.0, 0.0), beta):   # warm-up of both settings
    one(b)
off, on = [], []
for r in range(a.reps):
    off.append(one((0.0, 0.0)))
    on.append(one(beta))
    print("round %2d  beta=0 %9.4f ms  beta>0 %9.4f ms" % (r, off[-1], on[-1]), flush=True)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": int(len(row)), "reps": a.reps, "beta": list(beta),
                  "unit": "ms per %d iteration(s)" % (a.toy_iters if toy else 1), "kernel_source_hash": c.kernel_source_hash(),
                  "iteration_plain_ms": stats(off), "iteration_momentum_ms": stats(on),
                  "momentum_over_plain": {"medians": float(np.median(on) / np.median(off)), "minima": min(on) / min(off)}}))
