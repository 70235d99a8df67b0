"""Ranks of the held-out entries (mf_plan_rank_heldout, mf_plan_rank_heldout_info, mf_backend_rank_metrics).

The contract (include/matfact_hip.h): for held-out entry n = (i, j), C_i = the items user i has not rated in the training
entries, B = the exact scores (oracle.predict_row: sequential k, unfused, mat2d.c:100-113):
    j rated -> -1;  B[i][j] NaN -> -2;  else #{ j' in C_i, j' != j : B[i][j'] > B[i][j] or (== and j' < j) },
IEEE comparisons, reported in the caller's order.  The model below states that rule in numpy; every comparison with it is
np.array_equal on int32 over ALL entries.

CPU tests: declarations, argument checks before any HIP call, mf_backend_rank_metrics against a numpy restatement, the
model against test_topn.py's model_row, the ISA of the new kernels, the CLI's refusals.  GPU tests (-m gpu): every
matrix-core shape and the exact form against the model and against recommend_topn, certification, replaced sets and
repeated calls, user shards, the golden ML100k factors, the CLI, the cfg4 shape.
"""
import math
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa  # noqa: E402
from test_topn import _cli_input, _plan, _rated_sets, model_row, planted_instance  # noqa: E402


# ------------------------------------------------------------------------------------------------ the model
def rank_of(b, rated, items, j):
    """The definition over one exact B row."""
    if j in rated:
        return -1
    if np.isnan(b[j]):
        return -2
    alive = np.ones(items, bool)
    if len(rated):
        alive[np.fromiter(rated, np.int64, len(rated))] = False
    alive[j] = False
    idx = np.arange(items)
    with np.errstate(invalid="ignore"):
        ahead = (b > b[j]) | ((b == b[j]) & (idx < j))     # IEEE: a NaN score is neither greater nor equal
    return int(np.count_nonzero(alive & ahead))


def model_ranks(orc, users, items, row, col, L, R, hrow, hcol, user_begin=0):
    """row / hrow: global user ids; L: the rows of users [user_begin, user_begin + users)."""
    rated = [set(x) for x in _rated_sets(users, np.asarray(row) - user_begin, col)]
    rows = {}
    out = np.empty(len(hrow), np.int32)
    for n, (i, j) in enumerate(zip((np.asarray(hrow) - user_begin).tolist(), np.asarray(hcol).tolist())):
        if i not in rows:
            rows[i] = orc.predict_row(np.ascontiguousarray(L[i]), R)
        out[n] = rank_of(rows[i], rated[i], items, j)
    return out


TIED = [3, 11, 7, 40, 100, 101, 200, 13]      # planted_instance's duplicated R rows


def heldout_for(seed, users, items, row, col, most=12, user_begin=0):
    """For every user 0 .. `most` entries in shuffled caller order: training pairs, the tied items, repeats, random items."""
    rng = np.random.default_rng(1000 + seed)
    rated = _rated_sets(users, np.asarray(row) - user_begin, col)
    hr, hc = [], []
    for u in range(users):
        picks = []
        for _ in range(int(rng.integers(0, most + 1))):
            x = rng.random()
            if x < 0.15 and rated[u]:
                picks.append(int(rng.choice(rated[u])))
            elif x < 0.35:
                picks.append(int(rng.choice([t for t in TIED if t < items])))
            elif x < 0.45 and picks:
                picks.append(picks[int(rng.integers(len(picks)))])
            else:
                picks.append(int(rng.integers(items)))
        hr += [u + user_begin] * len(picks)
        hc += picks
    perm = rng.permutation(len(hr))
    hr, hc = np.asarray(hr, np.int32)[perm], np.asarray(hc, np.int32)[perm]
    return hr, hc, rng.integers(1, 6, hr.shape[0]).astype(np.float64)


def np_metrics(rank, row, cutoff):
    """mf_backend_rank_metrics restated: python floats are IEEE doubles, sums run in the stated order."""
    rank, row = np.asarray(rank).tolist(), np.asarray(row).tolist()
    ev = [(r, u) for r, u in zip(rank, row) if r >= 0]
    out = dict(evaluated=len(ev), masked=rank.count(-1), nan=rank.count(-2), users=len({u for _, u in ev}),
               hits=sum(1 for r, _ in ev if r < cutoff), terms=0)
    if not ev:
        out.update(hit_rate=math.nan, mrr=math.nan, ndcg=math.nan)
        return out
    out["hit_rate"] = float(np.float64(out["hits"]) / np.float64(len(ev)))
    s = 0.0
    for r, _ in ev:
        s = s + 1.0 / float(r + 1)
    out["mrr"] = s / float(len(ev))
    total = 0.0
    for u in sorted({u for _, u in ev}):
        mine = [r for r, v in ev if v == u]
        dcg = 0.0
        for r in mine:
            if r < cutoff:
                dcg = dcg + 1.0 / float(np.log2(np.float64(r + 2)))
                out["terms"] += 1
        idcg = 0.0
        for r in range(min(len(mine), cutoff)):
            idcg = idcg + 1.0 / float(np.log2(np.float64(r + 2)))
            out["terms"] += 1
        total = total + dcg / idcg
    out["ndcg"] = total / float(out["users"])
    return out


def assert_metrics(m, ref):
    for k in ("evaluated", "masked", "nan", "users", "hits"):
        assert getattr(m, k) == ref[k], k
    if ref["evaluated"] == 0:
        assert math.isnan(m.hit_rate) and math.isnan(m.mrr) and math.isnan(m.ndcg)
        return
    assert np.float64(m.hit_rate).view(np.int64) == np.float64(ref["hit_rate"]).view(np.int64)
    assert np.float64(m.mrr).view(np.int64) == np.float64(ref["mrr"]).view(np.int64)
    # all terms positive; per term only log2 (<= 1 ulp in both libraries) and one division differ
    assert abs(m.ndcg - ref["ndcg"]) <= (ref["terms"] + 8) * 2.0 ** -52 * abs(ref["ndcg"]), (m.ndcg, ref["ndcg"])


# ------------------------------------------------------------------------------------------------ CPU
def test_rank_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    assert re.search(r"#define MF_RANK_MASKED \(-1\)", hdr) and capi.MF_RANK_MASKED == -1
    assert re.search(r"#define MF_RANK_NAN +\(-2\)", hdr) and capi.MF_RANK_NAN == -2
    assert "typedef struct mf_rank_metrics" in hdr
    for s in ("mf_plan_rank_heldout", "mf_plan_rank_heldout_info", "mf_backend_rank_metrics"):
        assert s + "(" in hdr and s in capi.HIP_SYMBOLS
        assert hasattr(capi.hip(), s)
    assert capi.hip().mf_backend_abi_version() == 5
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr)


def test_rank_argument_errors_come_before_any_hip_call(capi):
    import ctypes as C
    lib = capi.hip()
    out = np.zeros(4, np.int32)
    assert lib.mf_plan_rank_heldout(None, out.ctypes.data) == capi.MF_ERR_ARGUMENT
    assert lib.mf_plan_rank_heldout(None, None) == capi.MF_ERR_ARGUMENT
    assert lib.mf_plan_rank_heldout_info(None, None, None) == capi.MF_ERR_ARGUMENT
    rank = np.array([0, 3, -1, -2], np.int32)
    row = np.array([0, 1, 1, 0], np.int32)
    m = capi.RankMetrics()
    fn = lib.mf_backend_rank_metrics
    assert fn(rank.ctypes.data, row.ctypes.data, 4, 10, C.byref(m)) == capi.MF_OK
    assert fn(rank.ctypes.data, row.ctypes.data, 4, 0, C.byref(m)) == capi.MF_ERR_ARGUMENT
    assert fn(rank.ctypes.data, row.ctypes.data, 4, -1, C.byref(m)) == capi.MF_ERR_ARGUMENT
    assert fn(rank.ctypes.data, row.ctypes.data, -1, 10, C.byref(m)) == capi.MF_ERR_ARGUMENT
    assert fn(rank.ctypes.data, row.ctypes.data, 4, 10, None) == capi.MF_ERR_ARGUMENT
    assert fn(None, row.ctypes.data, 4, 10, C.byref(m)) == capi.MF_ERR_ARGUMENT
    assert fn(rank.ctypes.data, None, 4, 10, C.byref(m)) == capi.MF_ERR_ARGUMENT
    bad = np.array([0, -3, 1, 2], np.int32)
    assert fn(bad.ctypes.data, row.ctypes.data, 4, 10, C.byref(m)) == capi.MF_ERR_ARGUMENT
    assert fn(None, None, 0, 10, C.byref(m)) == capi.MF_OK and m.evaluated == 0 and math.isnan(m.ndcg)


def test_rank_plan_state_errors_need_no_gpu_work(capi):
    """no held-out set / no factors -> MF_ERR_STATE, rank == NULL -> MF_ERR_ARGUMENT (on a machine with a GPU; a plan cannot
    exist without one, which the NULL-plan checks above cover)"""
    if capi.device_count() < 1:
        assert capi.hip().mf_plan_rank_heldout(None, None) == capi.MF_ERR_ARGUMENT
        return
    inst = capi.parse_file(golden_in("inst0"))
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    out = np.zeros(8, np.int32)
    assert capi.hip().mf_plan_rank_heldout(plan._h, out.ctypes.data) == capi.MF_ERR_STATE      # no factors
    plan.upload(*capi.init_factors(inst.users, inst.items, inst.feats))
    assert capi.hip().mf_plan_rank_heldout(plan._h, out.ctypes.data) == capi.MF_ERR_STATE      # no held-out set
    assert capi.hip().mf_plan_rank_heldout(plan._h, None) == capi.MF_ERR_ARGUMENT
    assert plan.rank_heldout_info() == (-1, -1)
    plan.close()


@pytest.mark.parametrize("cutoff", [1, 10, 1000])
def test_rank_metrics_equal_the_numpy_restatement(capi, cutoff):
    rng = np.random.default_rng(cutoff)
    for n, nusers, top in [(1, 1, 3), (40, 7, 30), (3000, 200, 5000), (3000, 3, 100000)]:
        rank = rng.integers(0, top, n).astype(np.int32)
        rank[rng.random(n) < 0.1] = -1
        rank[rng.random(n) < 0.1] = -2
        row = (rng.integers(0, nusers, n) * 13 + 5).astype(np.int32)      # interleaved, any ids
        assert_metrics(capi.rank_metrics(rank, row, cutoff), np_metrics(rank, row, cutoff))
    # hand-made: user 9 has ranks 0 and 4, user 2 has rank 1 and a masked entry, user 5 only a NaN entry
    rank = np.array([4, 1, -2, 0, -1], np.int32)
    row = np.array([9, 2, 5, 9, 2], np.int32)
    m = capi.rank_metrics(rank, row, cutoff)
    assert (m.evaluated, m.masked, m.nan, m.users) == (3, 1, 1, 2)
    assert m.hits == {1: 1, 10: 3, 1000: 3}[cutoff]
    assert m.mrr == ((0.0 + 1.0 / 5.0) + 1.0 / 2.0 + 1.0 / 1.0) / 3.0
    assert_metrics(m, np_metrics(rank, row, cutoff))
    # nothing evaluated, and nothing at all
    assert_metrics(capi.rank_metrics(np.array([-1, -2], np.int32), np.array([0, 0], np.int32), cutoff),
                   np_metrics([-1, -2], [0, 0], cutoff))
    assert_metrics(capi.rank_metrics(np.zeros(0, np.int32), np.zeros(0, np.int32), cutoff), np_metrics([], [], cutoff))
    with pytest.raises(capi.HipBackendError):
        capi.rank_metrics(np.array([-3], np.int32), np.array([0], np.int32), cutoff)
    with pytest.raises(capi.HipBackendError):
        capi.rank_metrics(np.array([1], np.int32), np.array([0], np.int32), 0)


def test_model_rank_is_the_position_in_the_topn_model(orc):
    """rank = r < N  <=>  the top-N model has item j at position r, for users without a NaN candidate score; 60 users x 300
    items with duplicated R rows, a zero L row and +-inf entries"""
    users, items, K = 60, 300, 9
    row, col, val, L, R = planted_instance(3, users, items, K)
    L[3, :] = np.random.default_rng(5).standard_normal(K)     # no NaN user here: every user is comparable ...
    L[10, :] = 0.0                                            # every score +0.0 or -0.0: all ties
    R[60:64, 0] = -np.inf                                     # +-inf scores (NaN where L[i][0] is 0 or the other inf meets them)
    R[70, 1] = np.inf
    rated = _rated_sets(users, row, col)
    rated[10] = sorted(set(rated[10]) | {60, 61, 62, 63, 70})  # the zero row keeps no 0 * inf among its candidates
    rng = np.random.default_rng(9)
    compared = 0
    for i in range(users):
        b = orc.predict_row(np.ascontiguousarray(L[i]), R)
        open_ = np.setdiff1d(np.arange(items), rated[i])
        mi, _ = model_row(b, rated[i], items, 32)
        nan_candidate = bool(np.isnan(b[open_]).any())
        cand = list(mi[mi >= 0][:6]) + [int(x) for x in rng.integers(0, items, 4)]
        for j in cand[:10]:
            r = rank_of(b, set(rated[i]), items, int(j))
            if j in rated[i]:
                assert r == -1
                continue
            if np.isnan(b[j]):
                assert r == -2
                continue
            assert 0 <= r < open_.size
            if nan_candidate:
                continue                                      # ... except the users the inf entries give NaN scores
            compared += 1
            for N in (1, 5, 32):
                assert (r < N) == bool((mi[:N] == j).any())
                if r < N:
                    assert mi[r] == j
    assert compared >= 300


def test_rank_kernels_isa(capi):
    if not isa.have_tools() or not os.path.exists(isa.DEFAULT_LIB):
        pytest.skip("needs llvm-objdump/llvm-readelf/c++filt and the built library")
    kernels = isa.disassemble()
    meta = isa.metadata()
    mfma = [n for n in kernels if "mf::rank_mfma_kernel" in n]
    assert len(mfma) == 14, mfma      # K = 20 c (5), 16 c (6), 112, 128, 256
    for n in mfma:
        assert any(i.startswith("v_mfma_f64_16x16x4_f64") for i in kernels[n]), n
    small = [n for n in kernels if "mf::rank_threshold_kernel" in n or "mf::rank_exact_kernel" in n]
    assert len(small) == 2
    for n in small:
        ops = {isa.split(i)[0].replace("_e32", "").replace("_e64", "") for i in kernels[n]}
        assert {"v_mul_f64", "v_add_f64"} <= ops, n
    ours = [n for n in kernels if "mf::rank_" in n]
    assert len(ours) == 14 + 3        # + rank_finish_kernel
    for n in ours:
        assert not [i for i in kernels[n] if re.match(r"v_(fma|fmac|mad|pk_fma)\w*_f64", i)], n
        assert not [i for i in kernels[n] if i.startswith("scratch_")], n
        m = meta[n]
        assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0 and m[".sgpr_spill_count"] == 0, (n, m)
        assert "topn_" not in n and "loss_" not in n and "recommend_mfma_kernel" not in n


@pytest.mark.parametrize("env", [dict(MATFACT_RANK="0"), dict(MATFACT_RANK="-2"), dict(MATFACT_RANK="ten"),
                                 dict(MATFACT_RANK="3x"), dict(MATFACT_RANK=""), dict(MATFACT_RANK="10"),
                                 dict(MATFACT_RANK="10", MATFACT_LOSS="5")])
def test_cli_rank_bad_values_die_with_empty_stdout(capi, env, tmp_path):
    if "MATFACT_RANK" in env and env["MATFACT_RANK"] in ("0", "-2", "ten", "3x", ""):
        env = dict(env, MATFACT_LOSS="5", MATFACT_HELDOUT=golden_in("inst0"))
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(os.environ, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_RANK" in r.stderr, r
    if "MATFACT_HELDOUT" not in env:
        assert b"MATFACT_RANK needs MATFACT_HELDOUT=<file.in>." in r.stderr


# ------------------------------------------------------------------------------------------------ GPU
EXACT_KS = [8, 30, 301, 1024]      # no matrix-core shape: the exact pass for every entry; 301 and 1024 lie above every shape
KS = [8, 20, 30, 64, 100, 112, 128, 256, 301, 1024]


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


def _check_against_topn(plan, hrow, hcol, ranks, skip_users, where):
    """rank = r < 32  <=>  recommend_topn(32).items[i][r] == j (users with a NaN candidate score excepted)"""
    it = plan.recommend_topn(32, scores=False)
    n = 0
    for i, j, r in zip(hrow.tolist(), hcol.tolist(), ranks.tolist()):
        i -= plan.user_begin
        if i in skip_users or r < 0:
            continue
        n += 1
        if r < 32:
            assert it[i, r] == j, (where, i, j, r)
        else:
            assert not (it[i] == j).any(), (where, i, j, r)
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("impl,split", [("mfma", "rule"), ("mfma", "0"), ("exact", "rule")])
@pytest.mark.parametrize("K", KS)
def test_rank_every_k_equals_the_model(gpu, orc, K, impl, split, monkeypatch):
    """150 x 700 with exact ties, a NaN user (3), an inf entry (user 4), a full and an empty row, nearly full rows; a few
    hundred entries are a handful of row blocks, so the rule splits the items.  The entries of the NaN and the inf user
    that are not training pairs (those are decided by the masked test alone) must have gone through the exact pass."""
    capi = gpu
    if impl == "exact":
        monkeypatch.setenv("MF_RECOMMEND_IMPL", "exact")
    if split != "rule":
        monkeypatch.setenv("MF_RECOMMEND_SPLIT", split)
    users, items = 150, 700
    row, col, val, L, R = planted_instance(K, users, items, K)
    hrow, hcol, hval = heldout_for(K, users, items, row, col)
    # the NaN and the inf user get entries whatever the draw gave them
    hrow = np.concatenate([hrow, np.array([3, 3, 4, 4, 4], np.int32)])
    hcol = np.concatenate([hcol, np.array([0, 699, 5, 350, 698], np.int32)])
    hval = np.concatenate([hval, np.ones(5)])
    want = model_ranks(orc, users, items, row, col, L, R, hrow, hcol)
    assert (want == -1).any() and (want == -2).any() and (want >= 0).sum() > 300
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    plan.set_heldout(hrow, hcol, hval)
    got = plan.rank_heldout()
    assert got.dtype == np.int32 and np.array_equal(got, want), (K, impl, split, np.flatnonzero(got != want)[:8])
    exact_entries, form = plan.rank_heldout_info()
    if impl == "exact" or K in EXACT_KS:
        assert exact_entries == -1 and form == 0
    else:
        special = int(np.count_nonzero(((hrow == 3) | (hrow == 4)) & (want != -1)))
        assert special >= 2 and form in (1, 2) and exact_entries >= special, (exact_entries, special, form)
    # the same ranks against recommend_topn(32) of the same plan
    nan_users = {i for i in range(users)
                 if np.isnan(orc.predict_row(np.ascontiguousarray(L[i]), R)[np.setdiff1d(np.arange(items), col[row == i])]).any()}
    assert _check_against_topn(plan, hrow, hcol, got, nan_users, (K, impl, split)) > 300
    plan.close()


@pytest.mark.gpu
def test_rank_certification_near_ties_and_separated(gpu, orc):
    capi = gpu
    users, items, K = 130, 256, 64
    rng = np.random.default_rng(7)
    L = rng.standard_normal((users, K))
    R = rng.standard_normal((items, K))
    R[1::2] = R[0::2] * (1.0 + 2.0 ** -52)        # every item has an ulp-scaled twin (test_topn.py's near-tie instance)
    row = np.repeat(np.arange(users, dtype=np.int32), 2)
    col = (np.arange(2 * users, dtype=np.int32) * 7) % items
    val = np.ones(row.shape[0])
    hrow = np.repeat(np.arange(users, dtype=np.int32), 2)
    hcol = np.stack([(np.arange(users) * 2 + 10) % items, (np.arange(users) * 2 + 11) % items], 1).reshape(-1).astype(np.int32)
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    plan.set_heldout(hrow, hcol, np.ones(hrow.shape[0]))
    want = model_ranks(orc, users, items, row, col, L, R, hrow, hcol)
    assert np.array_equal(plan.rank_heldout(), want), "near ties"
    assert plan.rank_heldout_info()[0] > 0
    plan.close()
    R = rng.standard_normal((items, K))
    hrow = np.arange(users, dtype=np.int32)
    hcol = ((np.arange(users) * 5 + 1) % items).astype(np.int32)
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    plan.set_heldout(hrow, hcol, np.ones(users))
    want = model_ranks(orc, users, items, row, col, L, R, hrow, hcol)
    assert np.array_equal(plan.rank_heldout(), want), "separated"
    # the band is ~1e-11 wide where neighbouring scores are ~0.1 apart: the expected number is 0 (test_topn.py's bound)
    assert 0 <= plan.rank_heldout_info()[0] <= 2
    plan.close()


@pytest.mark.gpu
def test_rank_new_set_repeated_calls_and_current_factors(gpu, orc):
    capi = gpu
    users, items, K = 200, 900, 100
    row, col, val, L, R = planted_instance(5, users, items, K)
    L[3] = np.random.default_rng(1).standard_normal(K)      # finite factors: the plan iterates below
    L[4, 0] = 0.5
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    s1 = heldout_for(1, users, items, row, col)
    s2 = heldout_for(2, users, items, row, col, most=3)
    plan.set_heldout(*s1)
    w1 = model_ranks(orc, users, items, row, col, L, R, s1[0], s1[1])
    assert np.array_equal(plan.rank_heldout(), w1)
    best = plan.recommend()
    assert np.array_equal(plan.rank_heldout(), w1)
    plan.recommend_topn(10)
    assert np.array_equal(plan.rank_heldout(), w1)
    assert np.array_equal(plan.recommend(), best)
    plan.set_heldout(*s2)                                   # a new set replaces the old one
    w2 = model_ranks(orc, users, items, row, col, L, R, s2[0], s2[1])
    assert np.array_equal(plan.rank_heldout(), w2)
    plan.set_heldout(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))      # n = 0 removes it
    assert capi.hip().mf_plan_rank_heldout(plan._h, np.zeros(1, np.int32).ctypes.data) == capi.MF_ERR_STATE
    plan.set_heldout(*s1)
    plan.iterate(2)
    L2, R2 = plan.download()
    w3 = model_ranks(orc, users, items, row, col, L2, R2, s1[0], s1[1])
    assert not np.array_equal(w3, w1)
    assert np.array_equal(plan.rank_heldout(), w3)          # the ranks of the then-current factors
    plan.recommend()
    assert np.array_equal(plan.rank_heldout(), w3)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [20, 100])
def test_rank_user_shards_concatenate(gpu, orc, K):
    capi = gpu
    users, items = 160, 600
    row, col, val, L, R = planted_instance(40 + K, users, items, K)
    hrow, hcol, hval = heldout_for(K, users, items, row, col)
    whole = _plan(capi, users, items, K, row, col, val, L, R)
    whole.set_heldout(hrow, hcol, hval)
    want = whole.rank_heldout()
    assert np.array_equal(want, model_ranks(orc, users, items, row, col, L, R, hrow, hcol))
    whole.close()
    got = np.full(hrow.shape[0], -99, np.int32)
    for u0, uc in ((0, users // 2), (users // 2, users - users // 2)):
        m = (row >= u0) & (row < u0 + uc)
        h = (hrow >= u0) & (hrow < u0 + uc)
        p = capi.Plan(users, items, K, 0.01, row[m], col[m], val[m], user_begin=u0, user_count=uc)
        p.upload(L[u0:u0 + uc], R)
        p.set_heldout(hrow[h], hcol[h], hval[h])
        got[h] = p.rank_heldout()                           # the caller's order within the shard
        p.close()
    assert np.array_equal(got, want)
    mw, mg = capi.rank_metrics(want, hrow, 10), capi.rank_metrics(got, hrow, 10)
    assert (mw.hits, mw.evaluated, mw.mrr, mw.ndcg) == (mg.hits, mg.evaluated, mg.mrr, mg.ndcg)


@pytest.mark.gpu
def test_rank_golden_ml100k_factors(gpu, orc):
    capi = gpu
    inst = capi.parse_file(golden_in("instML100k"))
    z = np.load(os.path.join(GOLDEN, "instML100k.factors.npz"))
    L, R = np.ascontiguousarray(z["L_full"]), np.ascontiguousarray(z["R_full"])
    held = np.zeros(inst.row.shape[0], bool)
    held[::10] = True                                       # every 10th training entry is held out
    row, col, val = inst.row[~held], inst.col[~held], inst.val[~held]
    plan = _plan(capi, inst.users, inst.items, inst.feats, row, col, val, L, R)
    plan.set_heldout(inst.row[held], inst.col[held], inst.val[held])
    got = plan.rank_heldout()
    want = model_ranks(orc, inst.users, inst.items, row, col, L, R, inst.row[held], inst.col[held])
    assert np.array_equal(got, want) and (want >= 0).all()
    m = capi.rank_metrics(got, inst.row[held], 10)
    assert_metrics(m, np_metrics(got, inst.row[held], 10))
    print("\nML100k golden factors: %d held-out entries, hit_rate@10 %.4f mrr %.4f ndcg@10 %.4f, exact-pass entries %d, form %d"
          % (m.evaluated, m.hit_rate, m.mrr, m.ndcg, *plan.rank_heldout_info()))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "instML100k"])
def test_cli_rank(gpu, name, tmp_path):
    capi = gpu
    path = _cli_input(name, tmp_path)
    inst = capi.parse_file(path)
    rng = np.random.default_rng(3)
    n = min(2000, 5 * inst.users)
    hrow = rng.integers(0, inst.users, n).astype(np.int32)
    hcol = rng.integers(0, inst.items, n).astype(np.int32)
    hpath = str(tmp_path / "held.in")
    with open(hpath, "w") as f:
        f.write("%d\n%r\n%d\n%d %d %d\n" % (inst.iters, float(inst.alpha), inst.feats, inst.users, inst.items, n))
        f.writelines("%d %d %d\n" % (r, c, 1 + (r + c) % 5) for r, c in zip(hrow.tolist(), hcol.tolist()))
    env = dict(os.environ, MATFACT_LOSS="5", MATFACT_HELDOUT=hpath)
    base = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=env)
    assert base.returncode == 0, base.stderr
    assert base.stdout == open(os.path.join(GOLDEN, name + ".out"), "rb").read()
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(env, MATFACT_RANK="10"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == base.stdout
    err = r.stderr.decode().splitlines()
    mine = [ln for ln in err if ln.startswith("heldout_rank ")]
    assert len(mine) == 1
    iters = [ln for ln in err if ln.startswith("iter ")]
    assert iters == [ln for ln in base.stderr.decode().splitlines() if ln.startswith("iter ")]
    assert err.index(mine[0]) > err.index(iters[-1])
    w = mine[0].split()
    assert w[1::2] == ["cutoff", "evaluated", "masked", "nan", "users", "hits", "hit_rate", "mrr", "ndcg"]
    # the same factors through the plan
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    plan.upload(*capi.init_factors(inst.users, inst.items, inst.feats))
    plan.iterate(inst.iters)
    plan.set_heldout(hrow, hcol, np.ones(n))
    m = capi.rank_metrics(plan.rank_heldout(), hrow, 10)
    plan.close()
    assert [int(x) for x in w[2:12:2]] == [10, m.evaluated, m.masked, m.nan, m.users]
    assert int(w[12]) == m.hits and m.evaluated + m.masked + m.nan == n
    assert (float(w[14]), float(w[16]), float(w[18])) == (m.hit_rate, m.mrr, m.ndcg)


@pytest.mark.gpu
def test_rank_cfg4_shape(gpu, orc):
    """1e6 x 1e5, K = 100 (the bench workload's shape): one held-out entry per user on a uniformly drawn unrated item; the
    ranks of 256 sampled users equal the model; the times are printed."""
    capi = gpu
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.CONFIGS["cfg4"]
    U, I, K = cfg["users"], cfg["items"], cfg["feats"]
    row, col, val = capi.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, "uniform"))
    L0, R0 = capi.init_factors(U, I, K)
    plan = capi.Plan(U, I, K, cfg["alpha"], row, col, val)
    plan.upload(L0, R0)
    # a uniformly drawn unrated item per user: redraw the (few) draws that hit a rated pair
    rng = np.random.default_rng(44)
    hcol = rng.integers(0, I, U).astype(np.int64)
    key = row.astype(np.int64) * I + col
    if not (key[1:] > key[:-1]).all():
        key.sort()
    for _ in range(50):
        q = np.arange(U, dtype=np.int64) * I + hcol
        hit = key[np.minimum(np.searchsorted(key, q), key.shape[0] - 1)] == q
        if not hit.any():
            break
        hcol[hit] = rng.integers(0, I, int(hit.sum()))
    assert not hit.any()
    hrow = np.arange(U, dtype=np.int32)
    plan.set_heldout(hrow, hcol.astype(np.int32), np.ones(U))
    plan.recommend()
    t0 = time.perf_counter()
    plan.recommend()
    t1 = time.perf_counter()
    got = plan.rank_heldout()
    t2 = time.perf_counter()
    got2 = plan.rank_heldout()
    t3 = time.perf_counter()
    info = plan.rank_heldout_info()
    print("\ncfg4 top-1 %.3f s, rank (one entry per user) %.3f s first call, %.3f s second, exact-pass entries %d, form %d"
          % (t1 - t0, t2 - t1, t3 - t2, *info))
    assert np.array_equal(got, got2) and (got >= 0).all() and (got < I).all()
    users = np.sort(np.random.default_rng(4).choice(U, 256, replace=False))
    ptr = np.searchsorted(row, np.arange(U + 1))
    sub_row = np.concatenate([np.full(ptr[u + 1] - ptr[u], t, np.int32) for t, u in enumerate(users)])
    sub_col = np.concatenate([col[ptr[u]:ptr[u + 1]] for u in users])
    want = model_ranks(orc, len(users), I, sub_row, sub_col, L0[users], R0, np.arange(len(users)), hcol[users])
    assert np.array_equal(got[users], want)
    plan.close()
