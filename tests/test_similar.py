"""Similar items: the top-N neighbours of an item's row of R among the other items (mf_plan_similar_items and friends).

The contract (include/matfact_hip.h): Q = R (dot) or R with every row divided by its norm (cosine: the squares added in
ascending k from 0.0, unfused; sqrt and division correctly rounded; nothing special-cased); S[j][j'] = dot(Q[j], Q[j']) as
mat2d_prod forms it; row t is the repeated print_output rule of mf_plan_recommend_topn over S[query[t]][.] with the query item
itself masked.  The model below builds Q in numpy, takes the scores from oracle.predict_row and applies test_topn's model_row
with rated = [j].  Items are compared exactly and scores bit for bit; a NaN score has to be a NaN, which sign and payload it
carries is the hardware's choice (IEEE 754 leaves it open, and 0/0 differs between the CPU and the GPU).

CPU tests: declarations, argument checks before any HIP call, the CLI's messages, the numpy recipe, the model.  GPU tests
(-m gpu): every matrix-core shape and the exact form at the edges of the 64-row workgroup, the 128-item tile and the item
split; certification; special values; listed queries; the composition with recommend_topn; trained factors; the CLI; one
shape at size.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in
from test_topn import model_row

METRICS = ("dot", "cosine")


# ------------------------------------------------------------------------------------------------ the model
def cosine_q(R):
    """Q of MF_SIMILAR_COSINE: two array operations per k (multiply, then add), hence unfused"""
    with np.errstate(all="ignore"):
        s = np.zeros(R.shape[0])
        for k in range(R.shape[1]):
            s = s + R[:, k] * R[:, k]
        n = np.sqrt(s)
        return np.ascontiguousarray(R / n[:, None])


def operand(R, metric):
    return cosine_q(R) if metric == "cosine" else np.ascontiguousarray(R)


def model_similar(orc, R, metric, n, only=None):
    Q = operand(R, metric)
    items = Q.shape[0]
    sel = range(items) if only is None else only
    oi = np.full((len(sel), n), -1, np.int32)
    os_ = np.full((len(sel), n), np.nan)
    for t, j in enumerate(sel):
        oi[t], os_[t] = model_row(orc.predict_row(np.ascontiguousarray(Q[j]), Q), [j], items, n)
    return oi, os_


def _bits(s):
    s = np.array(s, np.float64)
    s[np.isnan(s)] = np.nan   # one NaN for all: sign and payload are not part of the contract
    return s.view(np.int64)


def assert_same(items, scores, mi, ms, where=""):
    assert items.shape == mi.shape, (where, items.shape, mi.shape)
    assert np.array_equal(items, mi), (where, np.argwhere(items != mi)[:5])
    if scores is None:
        return
    live = mi >= 0
    assert np.array_equal(_bits(scores[live]), _bits(ms[live])), where
    assert np.isnan(scores[~live]).all(), (where, "NaN where the item is -1")


PAIRS_EQUAL = [(3, 11), (100, 101)]     # R[b] = R[a]: ties under both metrics
PAIRS_TWICE = [(7, 40), (200, 13)]      # R[b] = 2 R[a]: ties under cosine only


@functools.lru_cache(maxsize=None)
def instance_a(items, K):
    rng = np.random.default_rng(977 * K + items)
    R = rng.standard_normal((items, K))
    for a, b in PAIRS_EQUAL:
        if max(a, b) < items:
            R[b] = R[a]
    for a, b in PAIRS_TWICE:
        if max(a, b) < items:
            R[b] = 2.0 * R[a]
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def instance_b(K):
    items = 200
    R = np.random.default_rng(31 + K).standard_normal((items, K))
    R[5, :] = np.nan          # NaN row
    R[17, 3] = np.inf         # one +inf: an infinite norm
    R[64, :] = 0.0            # all-zero row: 0/0
    R[130, :] = 1e-200        # the sum of squares underflows to 0
    R[199, :] = 1e200         # the sum of squares overflows
    R.setflags(write=False)
    return R


_MODELS = {}


def model_of(orc, key, R, metric, n):
    """the model rows of all items at 33 entries, computed once per instance and metric; their first n columns"""
    k = (key, metric)
    if k not in _MODELS:
        _MODELS[k] = model_similar(orc, R, metric, 33)
    mi, ms = _MODELS[k]
    return mi[:, :n], ms[:, :n]


def _plan(capi, R):
    """a plan that holds nothing but R: one user without entries"""
    R = np.ascontiguousarray(R)
    e = np.zeros(0, np.int32)
    p = capi.Plan(1, R.shape[0], R.shape[1], 0.01, e, e, np.zeros(0))
    p.upload(np.zeros((1, R.shape[1])), R)
    return p


# ------------------------------------------------------------------------------------------------ CPU
def test_similar_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    assert re.search(r"#define MF_SIMILAR_DOT\s+0\b", hdr) and re.search(r"#define MF_SIMILAR_COSINE\s+1\b", hdr)
    assert (capi.MF_SIMILAR_DOT, capi.MF_SIMILAR_COSINE) == (0, 1)
    for s in ("mf_plan_similar_items", "mf_plan_similar_items_info", "mf_backend_similar_items"):
        assert s + "(" in hdr and s in capi.HIP_SYMBOLS
        assert hasattr(capi.hip(), s)
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr) and capi.hip().mf_backend_abi_version() == 5


def _raw(capi, R, metric, query, nq, n, items=True):
    out = np.empty((max(nq, 1), max(n, 1)), np.int32)
    q = None if query is None else np.ascontiguousarray(query, np.int32)
    return capi.hip().mf_backend_similar_items(R.ctypes.data, R.shape[0], R.shape[1], metric, None if q is None else q.ctypes.data,
                                               nq, n, out.ctypes.data if items else None, None, 0)


def test_similar_argument_errors_come_before_any_hip_call(capi):
    R = np.ascontiguousarray(instance_a(5, 10))
    A, U = capi.MF_ERR_ARGUMENT, capi.MF_ERR_UNSUPPORTED
    assert _raw(capi, R, 1, None, 5, 3, items=False) == A          # NULL items
    assert _raw(capi, R, 1, None, 5, 0) == A and _raw(capi, R, 0, None, 5, -2) == A
    assert _raw(capi, R, 2, None, 5, 3) == A and _raw(capi, R, -1, None, 5, 3) == A      # unknown metric
    assert _raw(capi, R, 1, [0, 1], -1, 3) == A                    # nq < 0
    assert _raw(capi, R, 1, [0, 5], 2, 3) == A and _raw(capi, R, 0, [-1, 2, 2], 3, 3) == A   # a query id out of range
    assert _raw(capi, R, 1, None, 4, 3) == A and _raw(capi, R, 1, None, 0, 3) == A       # all items, but nq != items
    assert _raw(capi, R, 1, None, 5, 33) == U and _raw(capi, R, 0, [4, 4, 0], 3, 33) == U
    assert _raw(capi, R, 1, [0, 5], 2, 33) == A                    # the argument rules come first
    assert capi.hip().mf_backend_similar_items(None, 5, 10, 1, None, 5, 3, np.empty(15, np.int32).ctypes.data, None, 0) == A
    assert capi.hip().mf_backend_similar_items(R.ctypes.data, 5, 0, 1, None, 5, 3, np.empty(15, np.int32).ctypes.data, None, 0) == A
    out = np.empty(15, np.int32)
    assert capi.hip().mf_plan_similar_items(None, 1, None, 5, 3, out.ctypes.data, None) == A
    assert capi.hip().mf_plan_similar_items_info(None, None, None) == A
    with pytest.raises(capi.HipBackendError) as e:
        capi.backend_similar_items(R, 40)
    assert e.value.status == U
    with pytest.raises(capi.HipBackendError) as e:
        capi.backend_similar_items(R, 3, query=[1, 7])
    assert e.value.status == A


def test_similar_without_a_gpu_fails_loudly(capi):
    """valid arguments reach the device: without one the call says so (there is no CPU path)"""
    want = capi.MF_OK if capi.device_count() > 0 else capi.MF_ERR_NO_DEVICE
    R = np.ascontiguousarray(instance_a(5, 10))
    for metric in (0, 1):
        assert _raw(capi, R, metric, None, 5, 3) == want
        assert _raw(capi, R, metric, [4, 0, 4], 3, 32) == want


@pytest.mark.parametrize("env", [dict(MATFACT_SIMILAR="0"), dict(MATFACT_SIMILAR="33"), dict(MATFACT_SIMILAR="ten"),
                                 dict(MATFACT_SIMILAR="3x"), dict(MATFACT_SIMILAR=""), dict(MATFACT_SIMILAR="3,"),
                                 dict(MATFACT_SIMILAR="3,euclid"), dict(MATFACT_SIMILAR="3,cosine,dot"),
                                 dict(MATFACT_SIMILAR="3"), dict(MATFACT_SIMILAR="3,dot", MATFACT_SIMILAR_OUT=""),
                                 dict(MATFACT_SIMILAR_OUT="s.txt"),
                                 dict(MATFACT_SIMILAR="3", MATFACT_DEVICES="0"), dict(MATFACT_SIMILAR="3", MATFACT_MATS="/dev/null"),
                                 dict(MATFACT_SIMILAR="3", MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_SIMILAR="3", MATFACT_RESUME="x.ck"),
                                 dict(MATFACT_SIMILAR="3", MATFACT_TOPN="3"), dict(MATFACT_SIMILAR="3", MATFACT_LOSS="1")])
def test_cli_similar_bad_values_die_with_empty_stdout(capi, env, tmp_path):
    env = dict(env)
    if set(env) - {"MATFACT_SIMILAR", "MATFACT_SIMILAR_OUT"}:
        env["MATFACT_SIMILAR_OUT"] = "s.txt"     # the exclusivity rules, not the missing path
    base = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(base, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_SIMILAR" in r.stderr, r
    assert not (tmp_path / "s.txt").exists()
    if list(env) == ["MATFACT_SIMILAR"] and env["MATFACT_SIMILAR"] == "3":
        assert b"MATFACT_SIMILAR needs MATFACT_SIMILAR_OUT=<path>." in r.stderr
    if env.get("MATFACT_SIMILAR") in ("0", "33", "ten", "3x", "", "3,", "3,euclid", "3,cosine,dot"):
        assert b"MATFACT_SIMILAR: expected N[,dot|cosine]" in r.stderr


def test_numpy_q_of_a_row_and_of_twice_that_row_are_the_same_bits():
    """scaling by 2 is exact through the square, the sum, the root and the division: what plants exact cosine ties"""
    rng = np.random.default_rng(3)
    for K in (1, 10, 100, 256):
        R = rng.standard_normal((6, K))
        R[1] = 2.0 * R[0]
        R[3] = 0.5 * R[2]
        R[5] = 2.0 ** 40 * R[4]
        Q = cosine_q(R)
        for a, b in ((0, 1), (2, 3), (4, 5)):
            assert np.array_equal(Q[a].view(np.int64), Q[b].view(np.int64)), (K, a, b)
    s = np.float64(0.0)
    r = R[0]
    for k in range(r.shape[0]):
        s = s + r[k] * r[k]       # the scalar recipe of the header: the array form is the same sum
    assert np.array_equal((r / np.sqrt(s)).view(np.int64), Q[0].view(np.int64))


def test_model_masks_the_query_itself_and_pads_the_tail(orc):
    R = np.array(instance_a(5, 10))
    R[4] = R[1]
    for metric in METRICS:
        mi, ms = model_similar(orc, R, metric, 6)
        for j in range(5):
            assert sorted(mi[j, :4].tolist()) == sorted(set(range(5)) - {j})
            assert (mi[j, 4:] == -1).all() and np.isnan(ms[j, 4:]).all()
        assert mi[0].tolist().index(1) < mi[0].tolist().index(4)          # an exact tie: the lower index first
        Q = operand(R, metric)
        assert ms[2, 0] == orc.predict_row(np.ascontiguousarray(Q[2]), Q)[mi[2, 0]]
    assert model_similar(orc, R, "cosine", 1)[0][1, 0] == 4 and model_similar(orc, R, "cosine", 1)[0][4, 0] == 1
    mi, ms = model_similar(orc, R[:1], "dot", 3)                          # one item: no candidate at all
    assert (mi == -1).all() and np.isnan(ms).all()
    R[0, :] = np.nan
    mi, ms = model_similar(orc, R, "dot", 3, only=[2])
    assert mi[0, 0] == 0 and np.isnan(ms[0, 0]) and mi[0, 1] in (1, 3, 4)   # the first candidate's score is NaN: it is the pick


# ------------------------------------------------------------------------------------------------ GPU
MATRIX_KS = [20, 100, 48, 96, 112, 128, 256]
EXACT_KS = [30, 10, 301, 1024]     # 301 and 1024: above every matrix-core shape, the normalisation chunked over K
ITEM_COUNTS = [1, 2, 5, 63, 64, 65, 127, 128, 129, 300]
NS = [1, 10, 32]
SHAPES = [(300, K) for K in MATRIX_KS + EXACT_KS] + [(i, K) for K in (100, 48) for i in ITEM_COUNTS if i != 300]


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.mark.gpu
@pytest.mark.parametrize("items,K", SHAPES)
def test_similar_all_items_equals_the_model(gpu, orc, items, K):
    """instance A at every K form (items = 300: five row blocks of 64, three item tiles of 128, the item split by the rule)
    and at every edge of the row block and the item tile (K = 100 and 48); with n >= items - 1 the tail is -1 / NaN"""
    capi = gpu
    R = instance_a(items, K)
    plan = _plan(capi, R)
    assert plan.similar_items_info() == (-1, -1)
    for metric in METRICS:
        for n in NS:
            mi, ms = model_of(orc, ("A", items, K), R, metric, n)
            it, sc = plan.similar_items(n, metric)
            assert_same(it, sc, mi, ms, (items, K, metric, n))
            if n >= items - 1:
                assert (it[:, max(items - 1, 0):] == -1).all()
            cnt, form = plan.similar_items_info()
            if K in EXACT_KS:
                assert (cnt, form) == (-1, 0)
            else:
                assert form in (1, 2) and 0 <= cnt <= items
            assert np.array_equal(plan.similar_items(n, metric, scores=False), it)
    plan.close()


def _uncertain_bound(capi, R, K, metric, n, ms33):
    """#{ j : exact gap between the n-th and the (n+1)-th model score <= 2 thr_j }: every approximate score is within
    thr_j / 2 of the exact one (and so is every order statistic of a row), hence an exact gap above 2 thr_j certifies"""
    Q = operand(R, metric)
    norm = np.sqrt((Q * Q).sum(axis=1)) * (1.0 + 1e-12)     # covers row_norm_kernel's rounding up
    thr = capi.recommend_margin(K) * norm * norm.max() + 1e-300
    gap = ms33[:, n - 1] - ms33[:, n]
    return int(np.count_nonzero(gap <= 2.0 * thr))


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import recommender_system_amd as rs
c = rs.capi
z = np.load(sys.argv[2])
out = {}
e = np.zeros(0, np.int32)
for key in z.files:
    if not key.startswith("R"):
        continue
    R = np.ascontiguousarray(z[key])
    p = c.Plan(1, R.shape[0], R.shape[1], 0.01, e, e, np.zeros(0))
    p.upload(np.zeros((1, R.shape[1])), R)
    for metric in ("dot", "cosine"):
        for n in (1, 10, 32):
            it, sc = p.similar_items(n, metric)
            tag = "%s_%s_%d" % (key, metric, n)
            out["i_" + tag], out["s_" + tag] = it, sc
            out["f_" + tag] = np.array(p.similar_items_info(), np.int64)
            if "query" in z.files:
                qi, qs = p.similar_items(n, metric, query=z["query"])
                out["qi_" + tag], out["qs_" + tag] = qi, qs
    p.close()
np.savez(sys.argv[3], **out)
"""


def _child(tmp_path, arrays, **env):
    """similar_items of every R* array (all items; the listed `query` too when given) at every n and metric in a fresh
    process with `env` set: the environment switches are read when a plan is created"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, src, dst], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(dst)


@pytest.mark.gpu
def test_similar_is_decided_on_the_matrix_cores(gpu, orc, tmp_path):
    capi = gpu
    items = 300
    got = {}
    for K in MATRIX_KS:
        R = instance_a(items, K)
        plan = _plan(capi, R)
        for metric in METRICS:
            _, ms33 = model_of(orc, ("A", items, K), R, metric, 33)
            for n in NS:
                bound = _uncertain_bound(capi, R, K, metric, n, ms33)
                assert bound < items // 10, (K, metric, n, bound)       # the exact kernel alone cannot pass for this
                got[K, metric, n] = plan.similar_items(n, metric)
                cnt, form = plan.similar_items_info()
                print("K=%d %s n=%d: exact-pass queries %d (bound %d), form %d" % (K, metric, n, cnt, bound, form))
                assert form in (1, 2), (K, metric, n)
                assert 0 <= cnt <= bound, (K, metric, n, cnt, bound)
        plan.close()
    z = _child(tmp_path, {"R%d" % K: instance_a(items, K) for K in MATRIX_KS}, MF_RECOMMEND_IMPL="exact")
    for (K, metric, n), (it, sc) in got.items():
        tag = "R%d_%s_%d" % (K, metric, n)
        assert z["f_" + tag].tolist() == [-1, 0], tag
        assert np.array_equal(z["i_" + tag], it) and np.array_equal(_bits(z["s_" + tag]), _bits(sc)), tag


@pytest.mark.gpu
@pytest.mark.parametrize("K", [100, 30])
def test_similar_special_values(gpu, orc, K):
    """a NaN row, an infinite norm, a zero row (0/0), a sum of squares that underflows (x/0) and one that overflows (x/inf)"""
    capi = gpu
    R = instance_b(K)
    plan = _plan(capi, R)
    for metric in METRICS:
        for n in NS:
            mi, ms = model_of(orc, ("B", K), R, metric, n)
            it, sc = plan.similar_items(n, metric)
            assert_same(it, sc, mi, ms, (K, metric, n))
            cnt, form = plan.similar_items_info()
            if K == 30:
                assert (cnt, form) == (-1, 0)
            elif metric == "cosine":
                assert form in (1, 2) and cnt == R.shape[0]     # every query sees a non-finite candidate
    bi, bs = capi.backend_similar_items(R, 10, "cosine")
    assert_same(bi, bs, *model_of(orc, ("B", K), R, "cosine", 10), where="level 1")
    plan.close()


def _queries(items):
    rng = np.random.default_rng(items)
    edges = [128, 0, items - 1, 64, 63, 127, 64, 0]
    out = [np.array([128], np.int32)]
    for length in (63, 64, 65, 700):
        q = np.concatenate([edges, rng.integers(0, items, length - len(edges))]).astype(np.int32)
        out.append(q[rng.permutation(length)])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("K", [100, 256])
def test_similar_listed_queries(gpu, orc, K, tmp_path):
    """row t of a listed query is row query[t] of the all-items result, on a plan with users and ratings of its own whose
    recommend_topn and its report are not disturbed; the same under a forced item split"""
    capi = gpu
    items, users = 300, 70
    R = instance_a(items, K)
    rng = np.random.default_rng(K)
    L = rng.standard_normal((users, K))
    mask = rng.random((users, items)) < 0.1
    row, col = (x.astype(np.int32) for x in np.nonzero(mask))
    plan = capi.Plan(users, items, K, 0.01, row, col, np.ones(row.shape[0]))
    plan.upload(L, R)
    top, top_s = plan.recommend_topn(7)
    top_info = plan.recommend_topn_info()
    assert top_info[1] in (1, 2)
    full = {}
    for metric in METRICS:
        for n in NS:
            full[metric, n] = plan.similar_items(n, metric)
            assert_same(*full[metric, n], *model_of(orc, ("A", items, K), R, metric, n), where=(K, metric, n))
    assert plan.recommend_topn_info() == top_info
    for q in _queries(items):
        for n, metric in ((10, "cosine"), (32, "dot"), (1, "cosine"), (10, "dot"), (32, "cosine"), (1, "dot")):
            it, sc = plan.similar_items(n, metric, query=q)
            fi, fs = full[metric, n]
            assert it.shape == (len(q), n)
            assert np.array_equal(it, fi[q]) and np.array_equal(_bits(sc), _bits(fs[q])), (K, len(q), metric, n)
            cnt, form = plan.similar_items_info()
            assert form in (1, 2) and 0 <= cnt <= len(q)
        assert plan.recommend_topn_info() == top_info
        t2, s2 = plan.recommend_topn(7)
        assert np.array_equal(t2, top) and np.array_equal(_bits(s2), _bits(top_s))
        assert np.array_equal(plan.similar_items(10, "cosine", scores=False), full["cosine", 10][0])
    it, sc = plan.similar_items(5, "dot", query=np.zeros(0, np.int32))
    assert it.shape == (0, 5) and plan.similar_items_info() == (0, 0)
    plan.close()
    q = _queries(items)[-1]
    z = _child(tmp_path, {"R": R, "query": q}, MF_RECOMMEND_SPLIT="2")
    for (metric, n), (fi, fs) in full.items():
        tag = "R_%s_%d" % (metric, n)
        assert np.array_equal(z["i_" + tag], fi) and np.array_equal(_bits(z["s_" + tag]), _bits(fs)), tag
        assert np.array_equal(z["qi_" + tag], fi[q]) and np.array_equal(_bits(z["qs_" + tag]), _bits(fs[q])), tag


@pytest.mark.gpu
@pytest.mark.parametrize("K", [100, 112, 30])
def test_similar_is_recommend_topn_on_a_diagonal_plan(gpu, K):
    """the hard way of the same query: users = items, every user rated exactly itself, L = R = Q uploaded from the host --
    Q from numpy for the cosine, which checks the device's square root and division against the host's bit for bit"""
    capi = gpu
    items = 300
    R = instance_a(items, K)
    diag = np.arange(items, dtype=np.int32)
    plan = _plan(capi, R)
    for metric in METRICS:
        Q = operand(R, metric)
        twin = capi.Plan(items, items, K, 0.01, diag, diag, np.ones(items))
        twin.upload(Q, Q)
        for n in NS:
            ti, ts = twin.recommend_topn(n)
            it, sc = plan.similar_items(n, metric)
            assert np.array_equal(it, ti) and np.array_equal(_bits(sc), _bits(ts)), (K, metric, n)
        twin.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "instML100k"])
def test_similar_after_training_uses_the_current_r(gpu, orc, name):
    capi = gpu
    inst = capi.parse_file(golden_in(name))
    z = np.load(os.path.join(GOLDEN, name + ".factors.npz"))
    if "L_full" in z.files:
        L, R = np.ascontiguousarray(z["L_full"]), np.ascontiguousarray(z["R_full"])
    else:
        L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    plan.upload(L, R)
    before = plan.similar_items(5, "dot")
    plan.iterate(3)
    Rt = plan.download()[1]
    assert not np.array_equal(Rt, R)
    for metric in METRICS:
        it, sc = plan.similar_items(5, metric)
        bi, bs = capi.backend_similar_items(Rt, 5, metric)
        assert np.array_equal(it, bi) and np.array_equal(_bits(sc), _bits(bs)), (name, metric)
        sel = np.arange(inst.items) if inst.items <= 64 else np.random.default_rng(1).choice(inst.items, 64, replace=False)
        mi, ms = model_similar(orc, Rt, metric, 5, only=sel)
        assert_same(it[sel], sc[sel], mi, ms, (name, metric))
        q = sel[::-1].astype(np.int32)
        qi, qs = capi.backend_similar_items(Rt, 5, metric, query=q)
        assert np.array_equal(qi, it[q]) and np.array_equal(_bits(qs), _bits(sc[q]))
    assert not np.array_equal(_bits(plan.similar_items(5, "dot")[1]), _bits(before[1]))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spec,metric", [("5", "cosine"), ("5,dot", "dot"), ("32,cosine", "cosine")])
def test_cli_similar(gpu, spec, metric, tmp_path):
    capi = gpu
    name = "inst30-40-10-2-10"
    path = golden_in(name)
    out = tmp_path / "similar.txt"
    base = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(base, MATFACT_SIMILAR=spec, MATFACT_SIMILAR_OUT=str(out)))
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(os.path.join(GOLDEN, name + ".out"), "rb").read()
    inst = capi.parse_file(path)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    plan.upload(L, R)
    plan.iterate(inst.iters)
    n = int(spec.split(",")[0])
    want = capi.write_topn(plan.similar_items(n, metric, scores=False))
    plan.close()
    text = out.read_bytes()
    assert text == want
    lines = text.decode().splitlines()
    assert len(lines) == inst.items and all(len(ln.split()) == min(n, inst.items - 1) for ln in lines)
    assert all(str(j) not in ln.split() for j, ln in enumerate(lines))


@pytest.mark.gpu
def test_similar_shape_at_size(gpu, orc):
    """20 000 items, K = 100, n = 10, cosine, all items: 313 row blocks and 157 item tiles without an item split; 256 sampled
    rows equal the model"""
    capi = gpu
    items, K = 20000, 100
    R = np.random.default_rng(20).standard_normal((items, K))
    plan = _plan(capi, R)
    it, sc = plan.similar_items(10, "cosine")
    cnt, form = plan.similar_items_info()
    print("\n%d items: exact-pass queries %d, form %d" % (items, cnt, form))
    assert form == 1 and 0 <= cnt <= items
    sel = np.sort(np.random.default_rng(4).choice(items, 256, replace=False))
    mi, ms = model_similar(orc, R, "cosine", 10, only=sel)
    assert_same(it[sel], sc[sel], mi, ms)
    assert (it != np.arange(items)[:, None]).all() and (it >= 0).all()
    plan.close()
