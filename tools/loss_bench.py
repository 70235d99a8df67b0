#!/usr/bin/env python3
"""Times mf_plan_loss against the user sweep of the same plan, in one process: after a warm-up of each, --reps rounds of
one iteration (its user sweep timed by the plan's own events, mf_plan_timing_read's user_ms / user_launches) alternating
with one loss call (host clock around the call, which ends synchronised).  Shapes: cfg4 (1e6 x 1e5, K = 100, 1e8 entries),
nflx (the Netflix-shaped power-law instance of bench.py), cfg5s (cfg5's K = 256 and row lengths at 2e5 x 2e5, 1e8 entries),
ml100k (the bundled MovieLens-100k sample; latency-bound).  Prints one line per round and a JSON summary with the ratio of
the medians, the ratio of the minima and the spread of both series; for rocprofv3 runs of the loss kernels as well."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recommender_system_amd as rs
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg5s", "ml100k"])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--heldout", type=float, default=0.0, help="also time a held-out set of this share of the entries")
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
    cfg = dict(bench.CONFIGS["cfg4" if a.config == "cfg4" else "cfg5"])
    if a.config == "cfg5s":
        cfg.update(users=200_000, items=200_000, nnz=100_000_000)
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = c.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, "uniform"))
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.upload(L0, R0)
print(plan.describe(), flush=True)
if a.heldout > 0:
    sel = np.sort(np.random.default_rng(1).choice(len(row), int(len(row) * a.heldout), replace=False))
    plan.set_heldout(row[sel], col[sel], val[sel])
plan.timing(True)
plan.iterate(2)      # warm-up of the sweeps
first = plan.loss()  # warm-up of the loss launch
plan.timing_read()
sweep, item, loss, held = [], [], [], []
for r in range(a.reps):
    plan.iterate(1)
    t = plan.timing_read()
    sweep.append(t["user_ms"] / t["user_launches"])
    item.append(t["item_ms"] / max(t["item_launches"], 1))
    t0 = time.perf_counter()
    out = plan.loss()
    loss.append((time.perf_counter() - t0) * 1e3)
    line = "round %2d  user sweep %9.4f ms  item sweep %9.4f ms  loss %9.4f ms  train rmse %.6f" % (r, sweep[-1], item[-1], loss[-1], out.rmse)
    if a.heldout > 0:
        t0 = time.perf_counter()
        h = plan.loss("heldout")
        held.append((time.perf_counter() - t0) * 1e3)
        line += "  held-out loss %9.4f ms rmse %.6f" % (held[-1], h.rmse)
    print(line, flush=True)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x)}


res = {"config": a.config, "users": U, "items": I, "feats": K, "nnz": int(len(row)), "reps": a.reps, "user_sweep_ms": stats(sweep),
       "item_sweep_ms": stats(item), "loss_ms": stats(loss), "ratio_of_medians": float(np.median(loss) / np.median(sweep)),
       "ratio_of_minima": min(loss) / min(sweep),
       "spread": {"user_sweep": (max(sweep) - min(sweep)) / float(np.median(sweep)), "loss": (max(loss) - min(loss)) / float(np.median(loss))}}
if held:
    res["heldout_loss_ms"] = stats(held)
print(json.dumps(res))
