#!/usr/bin/env python3
"""Times one plan's iteration with the plain step and with an adaptive one (AdaGrad, RMSProp or Adam on both sides), in one
process.  After a warm-up of both settings, --reps rounds of: factors uploaded afresh, one untimed iteration (an adaptive side
leaves rest there: its accumulators are zeroed in front of it, which is not part of a steady-state iteration), then one timed
iteration -- with kind none, then with --kind.  An iteration is timed by the plan's own events (mf_plan_timing_read: item_ms +
user_ms; a sweep's finishing kernels lie inside its pair of events).  Shapes as in tools/momentum_bench.py: cfg4, nflx, cfg4z
(Zipf columns: extreme rows, their finish on the side stream), ml100k (the plain plan takes errors + streams there, the
adaptive one the two sweeps: the ratio holds the cost of losing that form); and toy, the bundled inst0 sample, whose
--toy-iters iterations the plain plan runs inside ONE launch and the adaptive one as replayed graphs of two sweeps: there the
host clock goes around iterate() and a synchronise.  Prints one line per round and a JSON summary with median, minimum,
maximum and spread per series, the ratios of medians and of minima, the predicted ratio -- (rows_users + rows_items) * K * 8 * S
bytes added to bench.algorithmic_bytes of the two sweeps, S = 5 streams (7 with ADAM's m) -- and the kernel-source hash.

--target (ml100k, cfg3): iterations and wall time to the plain run's final training RMSE instead.  The plain run makes
--plain-iters iterations (the instance file's own count at ml100k); the adaptive run is monitored every --every iterations
and stops at the first point at or below that RMSE."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

DEFAULT_ETA = {"adam": 0.03, "rmsprop": 0.01, "adagrad": 0.1}
ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k", "toy", "cfg3"])
ap.add_argument("--kind", default="adam", choices=["adam", "rmsprop", "adagrad"])
ap.add_argument("--eta", type=float, default=0.0, help="0: 0.03 (adam), 0.01 (rmsprop), 0.1 (adagrad)")
ap.add_argument("--beta1", type=float, default=0.9)
ap.add_argument("--beta2", type=float, default=0.999)
ap.add_argument("--eps", type=float, default=1e-8)
ap.add_argument("--reps", type=int, default=8)
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
rule = (a.kind, a.eta or DEFAULT_ETA[a.kind], a.beta1, a.beta2, a.eps)
nnz = int(len(row))
streams = 7 if a.kind == "adam" else 5
algorithmic = bench.algorithmic_bytes(nnz, K, I) + bench.algorithmic_bytes(nnz, K, U)
predicted = 1.0 + (U + I) * K * 8.0 * streams / algorithmic


def set_rule(r):
    for side in ("users", "items"):
        if r is None:
            plan.set_adaptive(side, None)
        else:
            plan.set_adaptive(side, *r)


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
    set_rule(rule)
    plan.upload(L0, R0)
    plan.iterate(2)   # warm-up of the adaptive launches
    plan.upload(L0, R0)
    plan.synchronize()
    t0 = time.perf_counter()
    done, at = 0, rmse(plan.loss("train"))
    while at > goal and done < n:
        plan.iterate(a.every)
        done += a.every
        at = rmse(plan.loss("train"))
    ad_s = time.perf_counter() - t0
    print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "alpha": alpha, "rule": list(rule),
                      "plain": {"iterations": n, "train_rmse": goal, "wall_s": plain_s},
                      "adaptive": {"iterations": done, "train_rmse": at, "wall_s_with_a_loss_every_%d" % a.every: ad_s,
                                   "reached": bool(at <= goal)},
                      "kernel_source_hash": c.kernel_source_hash()}))
    sys.exit(0)


def one(r):
    set_rule(r)
    plan.upload(L0, R0)
    if toy:
        plan.iterate(8)   # out of rest
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
for r in (None, rule):   # warm-up of both settings
    one(r)
off, on = [], []
for k in range(a.reps):
    off.append(one(None))
    on.append(one(rule))
    print("round %2d  plain %9.4f ms  %s %9.4f ms" % (k, off[-1], a.kind, on[-1]), flush=True)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "reps": a.reps, "rule": list(rule),
                  "unit": "ms per %d iteration(s)" % (a.toy_iters if toy else 1), "kernel_source_hash": c.kernel_source_hash(),
                  "iteration_plain_ms": stats(off), "iteration_adaptive_ms": stats(on),
                  "adaptive_over_plain": {"medians": float(np.median(on) / np.median(off)), "minima": min(on) / min(off)},
                  "predicted_by_bytes": predicted}))
