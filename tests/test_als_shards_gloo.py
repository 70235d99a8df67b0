"""AlsShardedFactorization (recommender-system_amd/sharded.py) with world_size 2 on CPU over gloo.  The arithmetic of each shard
is the numpy model of tests/test_als_shards.py behind capi.Plan's surface; what is under test is the host logic: the order of
the five steps, one all-reduce of one buffer (the implicit kind's Gram record rides in it), the flip.  A two-operand sum is
commutative, so the collective's order cannot matter: the factors equal the model of the procedure bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from test_als import als_solve as single_als_solve
from test_als_shards import CONF, normal_records, pitch_of, sharded_iteration, shards_of, solve_records
from test_implicit import gram, implicit_solve
from test_regularised import LAM_I, LAM_U, _small
from test_sharded_gloo import _free_port
from test_sweep_edges import assert_same_bits
from test_weighted import plain_weights

LAM = (LAM_U, LAM_I)
USERS, ITEMS, K, ITERS = 21, 37, 6, 3


def inputs():
    pat, L0, R0, val, _ = _small(users=USERS, items=ITEMS, nnz=200, K=K, seed=23)
    return pat, L0, R0, val, plain_weights(3, pat.nnz)


class ModelPlan:
    """capi.Plan's surface for one user shard, computed by the model into numpy generations and the caller's CPU tensor"""

    def __init__(self, shard, items, L_block, R, kind, normal):
        self.sh, self.items, self.feats, self.kind, self.normal = shard, items, R.shape[1], kind, normal
        self.L, self.R, self.cur = [L_block.copy(), L_block.copy()], [R.copy(), R.copy()], 0
        self.calls = []

    def _check(self, ptr, pitch):
        assert ptr == self.normal.data_ptr() and pitch == self.normal.shape[1] >= pitch_of(self.feats) and pitch % 2 == 0

    def als_solve(self, side, other="current"):
        assert (side, other) == ("users", "current")
        sh = self.sh
        if self.kind == "implicit":
            self.L[self.cur ^ 1] = implicit_solve(sh.side[1], sh.val, sh.wgt, self.L[self.cur], self.R[self.cur], LAM_U, CONF)[0]
        else:
            self.L[self.cur ^ 1] = single_als_solve(sh.side[1], sh.val, sh.wgt, self.L[self.cur], self.R[self.cur], LAM_U, self.kind)[0]
        self.calls.append("solve-users")

    def als_normal(self, side, other, ptr, pitch):
        assert (side, other) == ("items", "next")
        self._check(ptr, pitch)
        Lb, T = self.L[self.cur ^ 1], self.feats * (self.feats + 1) // 2
        N = normal_records(self.sh.side[0], self.sh.val, self.sh.wgt, self.R[self.cur], Lb, -1, CONF if self.kind == "implicit" else None)
        out = np.zeros((self.items + 1, pitch))
        out[:self.items, :N.shape[1]] = N
        if self.kind == "implicit":
            out[self.items, :T] = gram(Lb)
        self.normal.copy_(torch.from_numpy(out))
        self.calls.append("normal")

    def als_solve_normal(self, side, ptr, pitch):
        assert side == "items"
        self._check(ptr, pitch)
        N, T = self.normal.numpy().copy(), self.feats * (self.feats + 1) // 2
        self.R[self.cur ^ 1] = solve_records(N[:self.items, :T + self.feats + 1], N[self.items, :T], self.R[self.cur], LAM_I, self.kind)[0]
        self.calls.append("solve-normal")

    def flip(self):
        self.cur ^= 1
        self.calls.append("flip")

    def iterate(self, iters):
        raise AssertionError("world 2 never takes the single-plan path")


def _worker(rank, world, port, kind, cut, out_path):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import importlib
    sharded = importlib.import_module("recommender_system_amd.sharded")
    pat, L0, R0, val, w = inputs()
    shard = shards_of(pat, val, w, (0, cut, pat.users))[rank]
    normal = torch.full((ITEMS + 1, pitch_of(K)), float("nan"), dtype=torch.float64)
    plan = ModelPlan(shard, ITEMS, L0[shard.begin:shard.begin + shard.count], R0, kind, normal)
    run = sharded.AlsShardedFactorization(plan, normal, rank, world)
    run.run(ITERS)
    assert plan.calls == ["solve-users", "normal", "solve-normal", "flip"] * ITERS
    parts = [None] * world
    dist.all_gather_object(parts, (plan.L[plan.cur], plan.R[plan.cur]))
    if rank == 0:
        np.savez(out_path, L=np.concatenate([p[0] for p in parts]), R0=parts[0][1], R1=parts[1][1])
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["ridge", "implicit"])
def test_als_sharded_run_equals_the_model_of_the_procedure(tmp_path, kind):
    pat, L0, R0, val, w = inputs()
    cut = 9
    shards = shards_of(pat, val, w, (0, cut, pat.users))
    L, R = L0, R0
    for _ in range(ITERS):
        blocks, R, _, _ = sharded_iteration(shards, L, R, LAM, kind, CONF)
        L = np.concatenate(blocks)
    out = str(tmp_path / "res.npz")
    mp.spawn(_worker, args=(2, _free_port(), kind, cut, out), nprocs=2, join=True)
    got = np.load(out)
    assert_same_bits(got["L"], L, kind + ": L after %d iterations" % ITERS)
    assert_same_bits(got["R0"], R, kind + ": rank 0's R")
    assert_same_bits(got["R1"], R, kind + ": rank 1's R")
    assert (L.view(np.uint64) != L0.view(np.uint64)).mean() > 0.9


def test_als_sharded_world_one_calls_iterate_and_checks_its_buffer():
    import importlib
    sharded = importlib.import_module("recommender_system_amd.sharded")

    class One:
        items, feats, n = ITEMS, K, 0

        def iterate(self, iters):
            self.n += iters
    plan = One()
    normal = torch.zeros((ITEMS + 1, pitch_of(K)), dtype=torch.float64)
    sharded.AlsShardedFactorization(plan, normal, 0, 1).run(4)
    assert plan.n == 4
    for bad in (torch.zeros((ITEMS, pitch_of(K)), dtype=torch.float64), torch.zeros((ITEMS + 1, pitch_of(K) + 1), dtype=torch.float64),
                torch.zeros((ITEMS + 1, pitch_of(K)), dtype=torch.float32)):
        with pytest.raises(ValueError):
            sharded.AlsShardedFactorization(plan, bad, 0, 1)
