#!/usr/bin/env python3
"""Times one plan's implicit-feedback iteration by conjugate gradient (mf_plan_set_implicit_cg) beside its direct implicit
iteration, in one process.  After a warm-up of every leg, --reps rounds of: factors uploaded afresh, one direct implicit
iteration (steps 0), then one CG iteration per entry of --steps -- the series alternate --, each by the host clock around
iterate(1) and a synchronise; then the two solves of every leg apart (each with its Gram and, under CG, the copy into the
square).  Shapes as in tools/als_cg_bench.py: cfg4, nflx, cfg4z, ml100k.  Prints one line per round and a JSON summary with
median, minimum, maximum and spread per series, every CG iteration over the direct one (medians and minima), the row counters
and the kernel-source hash.

--rank (ml100k): a record, not a benchmark.  tools/implicit_bench.py's 90 / 10 split (seeded), the training ratings as
preferences of 1.0 with w = the rating, --iters iterations from the reference's initialisation at every entry of --steps and
at steps 0.  Hit rate, NDCG and MRR at 10 of the held-out entries from mf_plan_rank_heldout, and the objective."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k"])
ap.add_argument("--lam", type=float, default=0.05)
ap.add_argument("--conf", type=float, default=40.0)
ap.add_argument("--steps", default="1,3,10")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rank", action="store_true")
ap.add_argument("--iters", type=int, default=15)
a = ap.parse_args()
c = rs.capi
steps = [int(s) for s in a.steps.split(",")]
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
nnz = int(len(row))

if a.rank:
    held = np.zeros(nnz, bool)
    held[np.random.default_rng(90).choice(nnz, nnz // 10, replace=False)] = True
    tr = ~held
    out = {"config": a.config, "users": U, "items": I, "feats": K, "train": int(tr.sum()), "heldout": int(held.sum()),
           "iters": a.iters, "lambda": a.lam, "conf": a.conf, "cutoff": 10, "kernel_source_hash": c.kernel_source_hash()}
    plan = c.Plan(U, I, K, alpha, row[tr], col[tr], np.ones(int(tr.sum())), weight=val[tr])
    plan.set_regularization(a.lam)
    plan.set_confidence(a.conf)
    plan.set_als("implicit")
    plan.set_heldout(row[held], col[held], val[held])
    for s in [0] + steps:
        plan.set_implicit_cg(s)
        plan.upload(L0, R0)
        plan.iterate(a.iters)
        m = c.rank_metrics(plan.rank_heldout(), row[held], 10)
        all_sq, observed, _ = plan.implicit_objective()
        us, its = plan.penalty()
        out["steps %d" % s] = {"hit_rate": m.hit_rate, "ndcg": m.ndcg, "mrr": m.mrr, "evaluated": m.evaluated, "users": m.users,
                               "objective": all_sq + observed + a.lam * (us + its),
                               "rows_solved_empty_not_pd": {"users": plan.als_info("users"), "items": plan.als_info("items")}}
    plan.close()
    print(json.dumps(out))
    sys.exit(0)

plan = c.Plan(U, I, K, alpha, row, col, val)
plan.set_regularization(a.lam)
plan.set_confidence(a.conf)
plan.set_als("implicit")
plan.upload(L0, R0)
longest = (int(np.bincount(row, minlength=U).max()), int(np.bincount(col, minlength=I).max()))


def timed(call):
    plan.synchronize()
    t0 = time.perf_counter()
    call()
    plan.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


legs = [0] + steps
for s in legs:   # warm-up of every leg
    plan.set_implicit_cg(s)
    print(plan.describe(), flush=True)
    plan.iterate(1)
series, users, items = {s: [] for s in legs}, {s: [] for s in legs}, {s: [] for s in legs}
for k in range(a.reps):
    for s in legs:
        plan.set_implicit_cg(s)
        plan.upload(L0, R0)
        series[s].append(timed(lambda: plan.iterate(1)))
    for s in legs:
        plan.set_implicit_cg(s)
        plan.upload(L0, R0)
        users[s].append(timed(lambda: plan.als_solve("users", "current")))
        items[s].append(timed(lambda: plan.als_solve("items", "next")))
    print("round %2d  direct %10.4f ms (users %10.4f, items %10.4f)" % (k, series[0][-1], users[0][-1], items[0][-1]) +
          "".join("  cg%d %10.4f ms (users %10.4f, items %10.4f)" % (s, series[s][-1], users[s][-1], items[s][-1]) for s in steps), flush=True)
counts = {}
for s in legs:
    plan.set_implicit_cg(s)
    plan.upload(L0, R0)
    plan.iterate(1)
    counts[s] = {"users": plan.als_info("users"), "items": plan.als_info("items")}
d = stats(series[0])
print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "longest_row_users_items": longest,
                  "lambda": a.lam, "conf": a.conf, "reps": a.reps, "unit": "ms per iteration, host clock",
                  "kernel_source_hash": c.kernel_source_hash(),
                  "direct": {"iteration_ms": d, "user_solve_ms": stats(users[0]), "item_solve_ms": stats(items[0]),
                             "rows_solved_empty_not_pd": counts[0]},
                  "cg": {"steps %d" % s: {"iteration_ms": stats(series[s]), "user_solve_ms": stats(users[s]), "item_solve_ms": stats(items[s]),
                                          "over_direct": {"medians": float(np.median(series[s])) / d["median"], "minima": min(series[s]) / d["min"]},
                                          "passes_per_side": s + 1, "rows_solved_empty_not_pd": counts[s]} for s in steps}}))
