#!/usr/bin/env python3
"""Times one plan's iteration without and with L2 regularisation, and mf_plan_penalty against the user sweep of the same
plan, in one process.  After a warm-up, --reps rounds of: one iteration at lambda = 0, one at lambda > 0 (both timed by the
plan's own events, mf_plan_timing_read: item_ms + user_ms), one penalty call (host clock around the call, which ends
synchronised).  The factors are uploaded again before every round, so both settings time the same values' neighbourhood and
nothing drifts.  Shapes: cfg4 (1e6 x 1e5, K = 100, 1e8 entries), nflx (the Netflix-shaped power-law instance of bench.py),
cfg4z (cfg4 with Zipf columns: extreme rows and ordered sums; alpha scaled as bench.py scales it), ml100k (the bundled
MovieLens-100k sample in its errors + streams mode).  Prints one line per round and a JSON summary with the ratios of the
medians and of the minima, the spread of every series and the kernel-source hash."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k"])
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--lambda-users", type=float, default=0.05)
ap.add_argument("--lambda-items", type=float, default=0.3)
a = ap.parse_args()
c = rs.capi
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
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.upload(L0, R0)
print(plan.describe(), flush=True)
plan.timing(True)
plan.iterate(2)       # warm-up of the sweeps
plan.penalty()        # warm-up of the penalty launches
plan.timing_read()
plain, reg, user, pen = [], [], [], []


def one_iteration(lam_u, lam_i):
    plan.set_regularization(lam_u, lam_i)
    plan.iterate(1)
    t = plan.timing_read()
    return t["item_ms"] + t["user_ms"], t["user_ms"] / max(t["user_launches"], 1)


for r in range(a.reps):
    plan.upload(L0, R0)
    ms, u = one_iteration(0.0, 0.0)
    plain.append(ms)
    user.append(u)
    plan.upload(L0, R0)
    reg.append(one_iteration(a.lambda_users, a.lambda_items)[0])
    t0 = time.perf_counter()
    usq, isq = plan.penalty()
    pen.append((time.perf_counter() - t0) * 1e3)
    print("round %2d  iteration lambda=0 %9.4f ms  lambda>0 %9.4f ms  user sweep %9.4f ms  penalty %9.4f ms  (|L|^2 %.6g |R|^2 %.6g)"
          % (r, plain[-1], reg[-1], user[-1], pen[-1], usq, isq), flush=True)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": int(len(row)), "reps": a.reps,
                  "lambda": [a.lambda_users, a.lambda_items], "kernel_source_hash": c.kernel_source_hash(),
                  "iteration_plain_ms": stats(plain), "iteration_regularised_ms": stats(reg), "user_sweep_ms": stats(user),
                  "penalty_ms": stats(pen),
                  "regularised_over_plain": {"medians": float(np.median(reg) / np.median(plain)), "minima": min(reg) / min(plain)},
                  "penalty_over_user_sweep": {"medians": float(np.median(pen) / np.median(user)), "minima": min(pen) / min(user)}}))
