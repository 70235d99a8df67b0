#!/usr/bin/env python3
"""Wall time of the level-1 drop-in call mf_backend_run (host buffers in, host buffers out: CSR/CSC build,
H2D, iterations, recommend, D2H) -- the PCIe-inclusive figure DESIGN.md quotes beside bench.py's value.
--instance FILE times a bundled instance instead of the synthetic one (--iters then replaces the file's count): on the
small ones an iteration is tens of microseconds, so the host's share of a launch shows (MF_GRAPH=0: every launch eager)."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recommender_system_amd as rs
ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--feats", type=int, default=100)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--instance", default=None, help="an instance file (tests/golden/*.in[.gz]) instead of the synthetic block")
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
c = rs.capi
if a.instance:
    f = c.parse_file(a.instance)
    inst = c.Instance(a.iters, f.alpha, f.feats, f.users, f.items, f.row, f.col, f.val)
    a.users = f.users
else:
    row, col, val = c.synth_block(0xC0FFEE + 4, a.users, a.items, 50, 150)
    inst = c.Instance(a.iters, 1e-4, a.feats, a.users, a.items, row, col, val)
L, R = c.init_factors(inst.users, inst.items, inst.feats)
c.device_count()
p, keep = c._problem(inst)
best = np.empty(a.users, np.int32)
for rep in range(a.reps):
    t = time.perf_counter()
    rc = c.hip().mf_backend_run(p, L, R, best, 0)
    dt = time.perf_counter() - t
    assert rc == 0
    print("mf_backend_run: %.3f s wall for %d iterations of %d entries + recommend -> %.3e nnz-updates/s "
          "(host buffers, PCIe and CSR/CSC build included)" % (dt, a.iters, inst.nnz, a.iters * inst.nnz / dt), flush=True)
