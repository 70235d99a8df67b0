#!/usr/bin/env python3
"""Times the item solve cut at the normal equations (mf_plan_als_normal + mf_plan_als_solve_normal: what a user shard runs
around its all-reduce) beside the single plan's mf_plan_als_solve(items), on ONE plan that holds all users, alternating in one
process.  After a warm-up of both, --reps rounds of: als_solve(items, next); als_normal + als_solve_normal(items); the two
new launches apart -- each by the host clock around the calls and a synchronise (launches of milliseconds and more).  The
user solve runs once, before the rounds: every series solves the items against the same new L.  Shapes as in
tools/als_bench.py: cfg4, nflx, cfg4z (Zipf columns), ml100k.  The records live in one torch tensor of (items + 1) x pitch
doubles (4.1 GB at cfg4).

Prints one line per round and a JSON summary: median, minimum, maximum and spread per series, the ratio pair / als_solve of
the medians and of the minima, the bytes of the records' round trip with its time at --copy-tbs, whether the pair's factors
equal als_solve's bit for bit (explicit kinds: they must), and registers, LDS request and the workgroups per CU that
registers and LDS allow for the instances this K launches (tools/isa.py; left out where the LLVM tools are missing)."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import recommender_system_amd as rs
import bench
import isa

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="cfg4", choices=["cfg4", "nflx", "cfg4z", "ml100k"])
ap.add_argument("--kind", default="ridge", choices=["ridge", "ridge-count", "implicit"])
ap.add_argument("--lam", type=float, default=0.05)
ap.add_argument("--conf", type=float, default=40.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--copy-tbs", type=float, default=6.3)
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
    U, I, K, alpha = cfg["users"], cfg["items"], cfg["feats"], cfg["alpha"]
    row, col, val = c.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, columns))
L0, R0 = c.init_factors(U, I, K)
plan = c.Plan(U, I, K, alpha, row, col, val)
plan.set_regularization(a.lam)
if a.kind == "implicit":
    plan.set_confidence(a.conf)
plan.set_als(a.kind)
plan.upload(L0, R0)
print(plan.describe(), flush=True)
nnz = int(len(row))
pitch = c.als_normal_pitch(K)
normal = torch.empty((I + 1, pitch), dtype=torch.float64, device=torch.device("cuda", 0))
torch.cuda.synchronize()
ptr = int(normal.data_ptr())


def timed(call):
    plan.synchronize()
    t0 = time.perf_counter()
    call()
    plan.synchronize()
    return (time.perf_counter() - t0) * 1e3


def pair():
    plan.als_normal("items", "next", ptr, pitch)
    plan.als_solve_normal("items", ptr, pitch)


def items_next():
    """the items' next generation: flip, download, flip back (the flip is host only)"""
    plan.flip()
    R = plan.download(want_l=False)[1]
    plan.flip()
    return R


plan.als_solve("users", "current")
plan.als_solve("items", "next")   # warm-up of both
ref, ref_info = items_next(), plan.als_info("items")
pair()
cut, cut_info = items_next(), plan.als_info("items")
same = bool(np.array_equal(ref.view(np.uint64), cut.view(np.uint64))) and ref_info == cut_info
single, both, first, second = [], [], [], []
for k in range(a.reps):
    single.append(timed(lambda: plan.als_solve("items", "next")))
    both.append(timed(pair))
    first.append(timed(lambda: plan.als_normal("items", "next", ptr, pitch)))
    second.append(timed(lambda: plan.als_solve_normal("items", ptr, pitch)))
    print("round %2d  als_solve(items) %10.4f ms  normal + solve_normal %10.4f ms  (als_normal %10.4f, als_solve_normal %10.4f)"
          % (k, single[-1], both[-1], first[-1], second[-1]), flush=True)


def stats(x):
    return {"min": min(x), "median": float(np.median(x)), "max": max(x), "spread": (max(x) - min(x)) / float(np.median(x))}


def instances():
    """registers, LDS request and workgroups per CU of the instances this K launches"""
    if not isa.have_tools():
        return None
    form = "wave" if " als_form=wave(" in plan.describe() else "wg"
    threads, bs, nch = (64, 2, 8) if form == "wave" else (256, 4, 16)
    kb = (K + bs - 1) // bs
    nb = (kb * (kb + 1) // 2 + threads - 1) // threads
    groups = 256 // threads
    tri, kp = K * (K + 1) // 2, kb * bs
    tiles = 2 if (a.kind == "implicit" or plan.weighted) else 1
    lds = {"als_kernel": groups * 8 * (tiles * nch * kp + 2 * nch + (nch + 1) // 2 + tri + 3 * K),
           "als_solve_normal_kernel": groups * 8 * (tri + 3 * K)}
    lds["als_normal_kernel"] = lds["als_kernel"]
    im = ", mf::AlsImplicit" if a.kind == "implicit" else ""
    names = {"als_kernel": "void mf::als_kernel<%d, %d, %d%s>" % (threads, bs, nb, im),
             "als_normal_kernel": "void mf::als_normal_kernel<%d, %d, %d%s>" % (threads, bs, nb, im),
             "als_solve_normal_kernel": "void mf::als_solve_normal_kernel<%d>" % threads}
    meta, out = isa.metadata(), {"form": form}
    for key, head in names.items():
        (m,) = [v for n, v in meta.items() if n.startswith(head + "(")]
        alloc = (m[".vgpr_count"] + 7) // 8 * 8
        by_regs = min(8, 512 // alloc) * 4 // 4          # waves per SIMD x 4 SIMDs over 4 waves per workgroup
        by_lds = (160 * 1024) // max(lds[key], 1)
        out[key] = {"vgpr": m[".vgpr_count"], "sgpr": m[".sgpr_count"], "scratch_bytes": m[".private_segment_fixed_size"],
                    "spilled": m[".vgpr_spill_count"] + m[".sgpr_spill_count"], "lds_request_bytes": lds[key],
                    "workgroups_per_cu_by_registers": by_regs, "workgroups_per_cu_by_lds": min(by_lds, 8),
                    "workgroups_per_cu": min(by_regs, by_lds, 8)}
    return out


round_trip = 2.0 * I * pitch * 8
print(json.dumps({"config": a.config, "users": U, "items": I, "feats": K, "nnz": nnz, "kind": a.kind, "lambda": a.lam, "reps": a.reps,
                  "unit": "ms, host clock", "kernel_source_hash": c.kernel_source_hash(), "record_pitch_doubles": pitch,
                  "als_solve_items_ms": stats(single), "normal_plus_solve_normal_ms": stats(both), "als_normal_ms": stats(first),
                  "als_solve_normal_ms": stats(second),
                  "ratio_of_medians": float(np.median(both)) / float(np.median(single)), "ratio_of_minima": min(both) / min(single),
                  "records_round_trip_bytes": round_trip, "records_round_trip_ms_at_copy_rate": round_trip / (a.copy_tbs * 1e12) * 1e3,
                  "copy_rate_tbs": a.copy_tbs, "pair_equals_als_solve_bit_for_bit": same,
                  "rows_solved_empty_not_pd": {"als_solve": ref_info, "pair": cut_info}, "instances": instances()}))
plan.close()
