#!/usr/bin/env python3
"""Times one plan's implicit-feedback iteration (mf_plan_set_als "implicit": Gram of R, user solve, Gram of the new L, item
solve, flip) beside its explicit ridge iteration, in one process.  After a warm-up of both, --reps rounds of: factors uploaded
afresh, one explicit iteration, factors uploaded afresh, one implicit iteration -- the two series alternate --, each by the
host clock around iterate(1) and a synchronise; then the two Gram launches of an iteration alone (mf_plan_gram without a host
pointer, items then users) and the objective.  Shapes as in tools/als_bench.py: cfg4, nflx, ml100k.  Prints one line per
round and a JSON summary: median, minimum, maximum and spread per series, the ratio of medians and of minima, the Grams'
share of the implicit iteration, the row counters of the last iteration and the kernel-source hash.

--rank (ml100k): a record, not a benchmark.  A 90 / 10 split of the entries (seeded), the training ratings as preferences of
1.0 with w = the rating, --iters implicit iterations from the reference's initialisation; beside it an explicit ridge run on
the ratings themselves.  Hit rate and NDCG at 10 of the held-out entries from mf_plan_rank_heldout."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "ml100k"])
ap.add_argument("--lam", type=float, default=0.05)
ap.add_argument("--conf", type=float, default=40.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rank", action="store_true")
ap.add_argument("--iters", type=int, default=15)
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
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = c.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, "uniform"))
L0, R0 = c.init_factors(U, I, K)
nnz = int(len(row))

if a.rank:
    held = np.zeros(nnz, bool)
    held[np.random.default_rng(90).choice(nnz, nnz // 10, replace=False)] = True
    tr = ~held
    out = {"config": a.config, "users": U, "items": I, "feats": K, "train": int(tr.sum()), "heldout": int(held.sum()),
           "iters": a.iters, "lambda": a.lam, "conf": a.conf, "cutoff": 10, "kernel_source_hash": c.kernel_source_hash()}
    for name, values, weight, kind in (("implicit", np.ones(int(tr.sum())), val[tr], "implicit"), ("explicit_ridge", val[tr], None, "ridge")):
        plan = c.Plan(U, I, K, alpha, row[tr], col[tr], values, weight=weight)
        plan.set_regularization(a.lam)
        plan.set_confidence(a.conf)
        plan.set_als(kind)
        plan.set_heldout(row[held], col[held], val[held])
        plan.upload(L0, R0)
        plan.iterate(a.iters)
        m = c.rank_metrics(plan.rank_heldout(), row[held], 10)
        out[name] = {"hit_rate": m.hit_rate, "ndcg": m.ndcg, "mrr": m.mrr, "evaluated": m.evaluated, "users": m.users,
                     "rows_solved_empty_not_pd": {"users": plan.als_info("users"), "items": plan.als_info("items")}}
        if kind == "implicit":
            all_sq, observed, _ = plan.implicit_objective()
            us, its = plan.penalty()
            out[name]["objective"] = all_sq + observed + a.lam * (us + its)
        plan.close()
    print(json.dumps(out))
    sys.exit(0)

plan = c.Plan(U, I, K, alpha, row, col, val)
plan.set_regularization(a.lam)
plan.set_confidence(a.conf)
plan.upload(L0, R0)


def timed(call):
    plan.synchronize()
    t0 = time.perf_counter()
    call()
    plan.synchronize()
    return (time.perf_counter() - t0) * 1e3


def grams():
    plan.gram("items", "current", download=False)
    plan.gram("users", "current", download=False)


plan.set_als("implicit")
print(plan.describe(), flush=True)
for kind in ("ridge", "implicit"):   # warm-up of both
    plan.set_als(kind)
    plan.iterate(1)
grams()
explicit, implicit, gram = [], [], []
for k in range(a.reps):
    plan.set_als("ridge")
    plan.upload(L0, R0)
    explicit.append(timed(lambda: plan.iterate(1)))
    plan.set_als("implicit")
    plan.upload(L0, R0)
    implicit.append(timed(lambda: plan.iterate(1)))
    gram.append(timed(grams))
    print("round %2d  explicit %10.4f ms  implicit %10.4f ms  (the two Grams alone %10.4f)" % (k, explicit[-1], implicit[-1], gram[-1]), flush=True)
objective_ms = timed(plan.implicit_objective)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


se, si, sg = stats(explicit), stats(implicit), stats(gram)
print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "lambda": a.lam, "conf": a.conf, "reps": a.reps,
                  "unit": "ms per iteration, host clock", "kernel_source_hash": c.kernel_source_hash(),
                  "iteration_explicit_ridge_ms": se, "iteration_implicit_ms": si, "two_grams_ms": sg,
                  "implicit_over_explicit": {"medians": si["median"] / se["median"], "minima": si["min"] / se["min"]},
                  "grams_share_of_implicit_iteration": sg["median"] / si["median"], "objective_ms": objective_ms,
                  "rows_solved_empty_not_pd": {"users": plan.als_info("users"), "items": plan.als_info("items")}}))
