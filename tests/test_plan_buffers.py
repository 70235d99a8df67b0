"""A long-lived plan whose on-demand buffers grow, shrink and are replaced between calls (dev_buf, mf_device.hip.h).

One plan per K answers a sequence of calls that makes every grow-on-demand buffer of the plan change size at least once,
in both directions: the top-N rows and per-split lists (n = 1, 32, 5), the similar-items operands (all items, 3 listed, 250
listed with repeats, all again; both metrics), the held-out set and the six rank buffers (50, 500, 10 entries), the
candidate records (3 users, 150), the loss sums, the temporary of predict.  Every answer has to equal the answer of a
fresh plan created for that call alone: indices with array_equal, scores and sums bit for bit through a uint64 view, the
_info reports as well.  No tolerance: both sides run the same kernels on the same inputs, and the passes are deterministic.

200 users x 300 items, about 2000 entries: 300 items are three 128-item tiles, so the item split is taken and the per-split
buffers exist.  K = 20 is a four-wave matrix-core form, K = 128 the eight-wave form of top-N and ranks (four-wave for
top-1), K = 30 has no matrix-core form and takes the exact pass.

The second test creates and closes 50 plans that each used every entry point once: the destructor path.
"""
import functools

import numpy as np
import pytest

from conftest import random_instance

pytestmark = pytest.mark.gpu

USERS, ITEMS = 200, 300
KS = (20, 128, 30)


@functools.lru_cache(maxsize=None)
def instance(K):
    import recommender_system_amd as rs
    d = random_instance(4242, USERS, ITEMS, K, density=2000.0 / (USERS * ITEMS))
    L, R = rs.capi.init_factors(USERS, ITEMS, K)
    return d, L, R


@functools.lru_cache(maxsize=None)
def heldout(n):
    rng = np.random.default_rng(1000 + n)
    return (rng.integers(0, USERS, n).astype(np.int32), rng.integers(0, ITEMS, n).astype(np.int32),
            rng.integers(1, 6, n).astype(np.float64))


def new_plan(capi, K):
    d, L, R = instance(K)
    p = capi.Plan(USERS, ITEMS, K, d["alpha"], d["row"], d["col"], d["val"])
    p.upload(L, R)
    return p


# ---- the calls: name -> f(plan) -> tuple of arrays (the answer and the _info report)
def topn(n):
    def f(p):
        items, scores = p.recommend_topn(n)
        return items, scores, np.array(p.recommend_topn_info())
    return f


def similar(metric, query):
    def f(p):
        items, scores = p.similar_items(10, metric=metric, query=query)
        return items, scores, np.array(p.similar_items_info())
    return f


def rank(n):
    def f(p):
        p.set_heldout(*heldout(n))
        r = p.rank_heldout()
        held = p.loss("heldout")
        return r, np.array(p.rank_heldout_info()), np.array([held.sse]), np.array([held.count])
    return f


def scored_users(n):
    users = np.random.default_rng(77 + n).permutation(USERS)[:n].astype(np.int32)
    return lambda p: (p.recommend_scored_users(users),)


def train_loss(p):
    loss, rows = p.loss("train", rows=True)
    return np.array([loss.sse]), np.array([loss.count]), rows


QUERY_3 = np.array([299, 0, 128], np.int32)
QUERY_250 = np.random.default_rng(5).integers(0, ITEMS, 250).astype(np.int32)   # with repeats

CALLS = [("topn 1", topn(1)), ("topn 32", topn(32)), ("topn 5", topn(5))]
for _m in ("dot", "cosine"):
    CALLS += [("similar %s all" % _m, similar(_m, None)), ("similar %s 3" % _m, similar(_m, QUERY_3)),
              ("similar %s 250" % _m, similar(_m, QUERY_250)), ("similar %s all again" % _m, similar(_m, None))]
CALLS += [("rank 50", rank(50)), ("rank 500", rank(500)), ("rank 10", rank(10)),
          ("scored_users 3", scored_users(3)), ("scored_users 150", scored_users(150)),
          ("recommend", lambda p: (p.recommend(), np.array([p.recommend_info()]))),
          ("loss train", train_loss),
          ("predict", lambda p: (p.predict(),)),
          ("topn 32 again", topn(32))]


def assert_same(got, want, where):
    assert len(got) == len(want), where
    for t, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (where, t, a.shape, b.shape)
        if a.dtype == np.float64:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (where, t, "bits differ")
        elif a.dtype.fields:   # candidate records: every field, bit for bit
            assert a.tobytes() == b.tobytes(), (where, t)
        else:
            assert np.array_equal(a, b), (where, t, np.argwhere(a != b)[:5])


@pytest.mark.parametrize("K", KS)
def test_long_lived_plan_equals_fresh_plans(capi, K):
    long_lived = new_plan(capi, K)
    try:
        for name, call in CALLS:
            got = call(long_lived)
            fresh = new_plan(capi, K)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert_same(got, want, "K=%d %s" % (K, name))
    finally:
        long_lived.close()
    # what the K were chosen for: 30 takes the exact form (0), the others a matrix-core form
    assert (got[2][1] == 0) == (K == 30), ("top-N form", K, got[2])


def test_fifty_plans_created_and_closed(capi):
    K = KS[0]
    first = None
    for _ in range(50):
        p = new_plan(capi, K)
        try:
            last = [call(p) for _, call in CALLS]   # a call that returns an error status raises
        finally:
            p.close()
        if first is None:
            first = last
    for (name, _), got, want in zip(CALLS, last, first):
        assert_same(got, want, "plan 50 vs plan 1: " + name)
