"""Top-N recommendations per user (mf_plan_recommend_topn and friends).

The contract: row i is print_output's rule (matFact.c:10-27) applied N times, each pick removed from the set of unrated
items -- S empty -> -1; first = min S; B[i][first] NaN -> first; otherwise the arg-max over the non-NaN scores, the lowest
index on ties -- and scores[i][r] = B[i][t_r] bit for bit (NaN where t_r = -1).  The model below states that rule over
exact B rows (oracle.predict_row: sequential k, unfused, mat2d.c:100-113) with the rated mask of every rated item.

CPU tests: declarations, argument checks before any HIP call, the `.out`-style writer, the model itself against the
oracle's top-1, and the ISA of the new kernels.  GPU tests (-m gpu): every matrix-core shape and the exact form against the
model, certification, the item split, unsorted input, repeated calls, the golden ML100k factors, the CLI, the cfg4 shape.
"""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa  # noqa: E402

QNAN_OK = "NaN where the item is -1"

# ------------------------------------------------------------------------------------------------ the model
def _rated_sets(users, row, col):
    rated = [[] for _ in range(users)]
    for r, c in zip(np.asarray(row).tolist(), np.asarray(col).tolist()):
        rated[r].append(c)
    return rated


def model_row(b, rated, items, n):
    """The repeated print_output rule over one exact B row; (items, scores) of length n."""
    alive = np.ones(items, bool)
    if len(rated):
        alive[np.asarray(rated, np.int64)] = False
    nan = np.isnan(b)
    out_i = np.full(n, -1, np.int32)
    out_s = np.full(n, np.nan)
    for r in range(n):
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        f = idx[0]
        if nan[f]:
            pick = f
        else:
            cand = idx[~nan[idx]]
            pick = cand[int(np.argmax(b[cand]))]   # first occurrence of the maximum: the lowest index on ties
        out_i[r] = pick
        out_s[r] = b[pick]
        alive[pick] = False
    return out_i, out_s


def model_topn(orc, users, items, row, col, L, R, n, only=None):
    rated = _rated_sets(users, row, col)
    sel = range(users) if only is None else only
    oi = np.full((len(sel), n), -1, np.int32)
    os_ = np.full((len(sel), n), np.nan)
    for t, i in enumerate(sel):
        b = orc.predict_row(np.ascontiguousarray(L[i]), R) if items else np.zeros(0)
        oi[t], os_[t] = model_row(b, rated[i], items, n)
    return oi, os_


def assert_same(items, scores, mi, ms, where=""):
    assert np.array_equal(items, mi), (where, np.argwhere(items != mi)[:5])
    if scores is None:
        return
    live = mi >= 0
    assert np.array_equal(scores[live].view(np.int64), ms[live].view(np.int64)), where
    assert np.isnan(scores[~live]).all(), (where, QNAN_OK)


def planted_instance(seed, users, items, K, n_few=4):
    """Random factors and ratings with planted exact ties (duplicated R rows), a NaN user, an inf entry, a full row, an
    empty row and users with fewer unrated items than most N."""
    rng = np.random.default_rng(seed)
    mask = rng.random((users, items)) < 0.15
    mask[1, :] = True                   # full row
    mask[2, :] = False                  # empty row
    for u in range(5, 5 + n_few):       # 1, 4, 9, 16 unrated items
        keep = rng.choice(items, size=min(items, (u - 4) ** 2), replace=False)
        mask[u, :] = True
        mask[u, keep] = False
    row, col = np.nonzero(mask)
    val = rng.integers(1, 6, row.shape[0]).astype(np.float64)
    L = rng.standard_normal((users, K))
    R = rng.standard_normal((items, K))
    for a, b in [(3, 11), (7, 40), (100, 101), (200, 13)]:
        if max(a, b) < items:
            R[b] = R[a]                 # exact ties for every user
    L[3, :] = np.nan                    # NaN user: every score NaN
    L[4, 0] = np.inf                    # inf entry: +-inf scores
    return row.astype(np.int32), col.astype(np.int32), val, L, R


def _plan(capi, users, items, K, row, col, val, L, R):
    p = capi.Plan(users, items, K, 0.01, row, col, val)
    p.upload(L, R)
    return p


# ------------------------------------------------------------------------------------------------ CPU
def test_topn_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    assert re.search(r"#define MF_TOPN_MAX 32\b", hdr) and capi.MF_TOPN_MAX == 32
    for s in ("mf_plan_recommend_topn", "mf_plan_recommend_topn_info", "mf_backend_recommend_topn", "mf_backend_run_topn"):
        assert s + "(" in hdr and s in capi.HIP_SYMBOLS
        assert hasattr(capi.hip(), s)
    assert "mf_host_write_topn(" in open(os.path.join(ROOT, "include", "matfact_host.h")).read()
    assert "mf_host_write_topn" in capi.HOST_SYMBOLS and hasattr(capi.host(), "mf_host_write_topn")
    assert capi.hip().mf_backend_abi_version() == 5


def _raw(capi, entry, inst, n, items=True):
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    it = np.empty((inst.users, max(n, 1)), np.int32)
    return getattr(capi.hip(), entry)(p, L.ctypes.data, R.ctypes.data, n, it.ctypes.data if items else None, None, 0)


@pytest.mark.parametrize("entry", ["mf_backend_recommend_topn", "mf_backend_run_topn"])
def test_topn_argument_errors_come_before_any_hip_call(capi, entry):
    inst = capi.parse_file(golden_in("inst0"))
    assert _raw(capi, entry, inst, 0) == capi.MF_ERR_ARGUMENT
    assert _raw(capi, entry, inst, -3) == capi.MF_ERR_ARGUMENT
    assert _raw(capi, entry, inst, 5, items=False) == capi.MF_ERR_ARGUMENT
    assert _raw(capi, entry, inst, 33) == capi.MF_ERR_UNSUPPORTED
    assert capi.hip().mf_plan_recommend_topn(None, 3, None, None) == capi.MF_ERR_ARGUMENT


@pytest.mark.parametrize("entry", ["mf_backend_recommend_topn", "mf_backend_run_topn"])
def test_topn_without_a_gpu_fails_loudly(capi, entry):
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    inst = capi.parse_file(golden_in("inst0"))
    for n in (1, 10, 32):
        assert _raw(capi, entry, inst, n) == capi.MF_ERR_NO_DEVICE


def _write_out(capi, best):
    """mf_host_write_out of best[], as bytes (the `.out` writer the reference's main calls)"""
    import ctypes as C
    import tempfile
    best = np.ascontiguousarray(best, np.int32)
    libc = C.CDLL(None)
    libc.fdopen.restype = C.c_void_p
    libc.fdopen.argtypes = [C.c_int, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    fn = capi.host().mf_host_write_out
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    with tempfile.TemporaryFile() as tf:
        f = libc.fdopen(os.dup(tf.fileno()), b"w")
        assert fn(f, best.ctypes.data, best.shape[0]) == 0
        libc.fclose(f)
        tf.seek(0)
        return tf.read()


@pytest.mark.parametrize("name", ["inst0", "inst1", "inst2", "inst30-40-10-2-10", "instML100k"])
def test_write_topn_with_one_item_is_the_out_writer(capi, name):
    text = open(os.path.join(GOLDEN, name + ".out"), "rb").read()
    got = np.array([int(x) for x in text.split()], np.int32)
    best = np.full(2 * got.shape[0] + 1, -1, np.int32)   # users without a line (every item rated) in between
    best[1::2] = got
    assert _write_out(capi, best) == text
    assert capi.write_topn(best.reshape(-1, 1)) == text


def test_write_topn_skips_empty_slots_and_users(capi):
    items = np.array([[4, 2, -1], [-1, -1, -1], [7, -1, -1], [0, 1, 2]], np.int32)
    assert capi.write_topn(items) == b"4 2\n7\n0 1 2\n"
    assert capi.write_topn(np.zeros((0, 3), np.int32)) == b""
    assert capi.write_topn(np.array([[5], [-1], [3]], np.int32)) == b"5\n3\n"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_with_one_item_is_the_oracle_recommend(orc, seed):
    users, items, K = 24, 150, 9
    row, col, val, L, R = planted_instance(seed, users, items, K)
    L[10, :] = 0.0                      # every score +0.0 or -0.0: all ties
    R[60:64] = -np.inf if seed == 1 else R[60:64]
    inst = orc.Instance(1, 0.01, K, users, items, row, col, val)
    best = orc.recommend(inst, L, R)
    mi, _ = model_topn(orc, users, items, row, col, L, R, 1)
    assert np.array_equal(mi[:, 0], best)
    # t_1 .. t_N are prefixes of each other and the finite case is the sorted order
    m5, s5 = model_topn(orc, users, items, row, col, L, R, 5)
    assert np.array_equal(m5[:, :1], mi)
    u = 0
    b = orc.predict_row(np.ascontiguousarray(L[u]), R)
    open_ = np.setdiff1d(np.arange(items), col[row == u])
    order = open_[np.lexsort((open_, -b[open_]))][:5]
    assert np.array_equal(m5[u], order)


def test_topn_kernels_isa(capi):
    if not isa.have_tools() or not os.path.exists(isa.DEFAULT_LIB):
        pytest.skip("needs llvm-objdump/llvm-readelf/c++filt and the built library")
    kernels = isa.disassemble()
    meta = isa.metadata()
    mfma = [n for n in kernels if "mf::topn_mfma_kernel" in n]
    assert len(mfma) == 14, mfma
    for n in mfma:
        assert any(i.startswith("v_mfma_f64_16x16x4_f64") for i in kernels[n]), n
    exact = [n for n in kernels if "mf::topn_exact_kernel" in n or "mf::topn_merge_kernel" in n]
    assert len(exact) == 2
    for n in exact + mfma:   # the re-scoring of the members lives in topn_mfma_kernel and topn_merge_kernel
        body = kernels[n]
        assert not [i for i in body if re.match(r"v_(fma|fmac|mad|pk_fma)\w*_f64", i)], n
        ops = {isa.split(i)[0] for i in body}
        assert {"v_mul_f64", "v_add_f64"} <= {o.replace("_e32", "").replace("_e64", "") for o in ops}, n
    for n in exact + mfma:
        assert not [i for i in kernels[n] if i.startswith("scratch_")], n
        m = meta[n]
        assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0, (n, m)
    assert not [n for n in kernels if "topn" in n and "recommend_mfma_kernel" in n]


# ------------------------------------------------------------------------------------------------ GPU
EXACT_KS = [8, 30, 301, 1024]      # no matrix-core shape: the exact pass for everybody; 301 and 1024 lie above every shape
KS = [8, 20, 30, 64, 100, 128, 256, 301, 1024]
NS = [1, 3, 10, 16, 17, 32]


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.mark.gpu
@pytest.mark.parametrize("impl,split", [("mfma", "rule"), ("mfma", "0"), ("exact", "rule")])
@pytest.mark.parametrize("K", KS)
def test_topn_every_k_and_n_equals_the_model(gpu, orc, K, impl, split, monkeypatch):
    """150 users are three user blocks: the rule splits the items (topn_merge_kernel certifies); MF_RECOMMEND_SPLIT=0 keeps
    the certification and re-scoring inside topn_mfma_kernel"""
    capi = gpu
    if impl == "exact":
        monkeypatch.setenv("MF_RECOMMEND_IMPL", "exact")
    if split != "rule":
        monkeypatch.setenv("MF_RECOMMEND_SPLIT", split)
    users, items = 150, 700
    row, col, val, L, R = planted_instance(K, users, items, K)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 32)
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    best = plan.recommend()
    for n in NS:
        it, sc = plan.recommend_topn(n)
        assert_same(it, sc, mi[:, :n], ms[:, :n], (K, n, impl))
        assert np.array_equal(it[:, 0], best), (K, n, impl)
        exact_users, form = plan.recommend_topn_info()
        if impl == "exact" or K in EXACT_KS:
            assert exact_users == -1 and form == 0
        else:
            assert form in (1, 2) and exact_users >= 2     # the NaN and the inf user at least
    inst = capi.Instance(1, 0.01, K, users, items, row, col, val)
    i1, s1 = capi.backend_recommend_topn(inst, L, R, 1)
    assert np.array_equal(i1[:, 0], capi.backend_recommend(inst, L, R))
    assert_same(i1, s1, mi[:, :1], ms[:, :1])
    plan.close()


@pytest.mark.gpu
def test_topn_certification_near_ties_and_separated(gpu, orc):
    capi = gpu
    users, items, K = 130, 256, 64
    rng = np.random.default_rng(7)
    L = rng.standard_normal((users, K))
    R = rng.standard_normal((items, K))
    R[1::2] = R[0::2] * (1.0 + 2.0 ** -52)        # every item has an ulp-scaled twin: near ties at every odd rank
    row = np.repeat(np.arange(users, dtype=np.int32), 2)
    col = (np.arange(2 * users, dtype=np.int32) * 7) % items
    val = np.ones(row.shape[0])
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 3)
    it, sc = plan.recommend_topn(3)
    assert_same(it, sc, mi, ms, "near ties")
    assert plan.recommend_topn_info()[0] > 0
    plan.close()
    R = rng.standard_normal((items, K))
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 10)
    it, sc = plan.recommend_topn(10)
    assert_same(it, sc, mi, ms, "separated")
    assert 0 <= plan.recommend_topn_info()[0] <= 2
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [20, 64, 256])
def test_topn_item_split_and_unsorted_input(gpu, orc, K, monkeypatch):
    capi = gpu
    users, items = 100, 1000
    row, col, val, L, R = planted_instance(11 + K, users, items, K)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 17)
    got = {}
    for split in ("0", None, "3"):
        if split is None:
            monkeypatch.delenv("MF_RECOMMEND_SPLIT", raising=False)
        else:
            monkeypatch.setenv("MF_RECOMMEND_SPLIT", split)
        plan = _plan(capi, users, items, K, row, col, val, L, R)
        got[split] = plan.recommend_topn(17)
        assert_same(*got[split], mi, ms, (K, split))
        plan.close()
    monkeypatch.delenv("MF_RECOMMEND_SPLIT", raising=False)
    perm = np.random.default_rng(K).permutation(row.shape[0])     # file order not (row, col)-sorted
    plan = _plan(capi, users, items, K, row[perm], col[perm], val[perm], L, R)
    it, sc = plan.recommend_topn(17)
    assert_same(it, sc, mi, ms, (K, "unsorted"))
    plan.close()


@pytest.mark.gpu
def test_topn_repeated_calls_interleaved_with_recommend(gpu, orc):
    capi = gpu
    users, items, K = 200, 900, 100
    row, col, val, L, R = planted_instance(5, users, items, K)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 32)
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    best = plan.recommend()
    for n in (32, 1, 10, 17, 3, 32, 16):
        it, sc = plan.recommend_topn(n)
        assert_same(it, sc, mi[:, :n], ms[:, :n], n)
        assert np.array_equal(plan.recommend(), best)
        assert np.array_equal(plan.recommend_topn(n, scores=False), it)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [100, 64, 256])
def test_topn_first_then_recommend_then_topn_on_a_split_plan(gpu, orc, K):
    """Top-N before the plan's first recommend(), on a plan both passes split the items of: each call leaves the other's
    buffers alone"""
    capi = gpu
    users, items = 200, 900
    row, col, val, L, R = planted_instance(21 + K, users, items, K)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 17)
    best_o = orc.recommend(orc.Instance(1, 0.01, K, users, items, row, col, val), L, R)
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    it, sc = plan.recommend_topn(17)
    assert_same(it, sc, mi, ms, "first")
    assert np.array_equal(plan.recommend(), best_o)
    for n in (17, 10, 17):
        it, sc = plan.recommend_topn(n)
        assert_same(it, sc, mi[:, :n], ms[:, :n], n)
        assert np.array_equal(plan.recommend(), best_o)
    plan.close()


@pytest.mark.gpu
def test_topn_golden_ml100k_factors(gpu, orc):
    capi = gpu
    inst = capi.parse_file(golden_in("instML100k"))
    z = np.load(os.path.join(GOLDEN, "instML100k.factors.npz"))
    L, R = np.ascontiguousarray(z["L_full"]), np.ascontiguousarray(z["R_full"])
    mi, ms = model_topn(orc, inst.users, inst.items, inst.row, inst.col, L, R, 10)
    it, sc = capi.backend_recommend_topn(inst, L, R, 10)
    assert_same(it, sc, mi, ms)
    assert np.array_equal(it[:, 0], capi.backend_recommend(inst, L, R))


def _cli_input(name, tmp_path):
    path = golden_in(name)
    if path.endswith(".gz"):
        import gzip
        raw = gzip.open(path, "rb").read()
        path = str(tmp_path / (name + ".in"))
        open(path, "wb").write(raw)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inst0", "inst1", "inst2", "inst30-40-10-2-10", "instML100k"])
def test_cli_topn(gpu, name, tmp_path):
    capi = gpu
    path = _cli_input(name, tmp_path)
    out = open(os.path.join(GOLDEN, name + ".out"), "rb").read()
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(os.environ, MATFACT_TOPN="1"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == out
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(os.environ, MATFACT_TOPN="5"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().splitlines()
    assert [ln.split()[0] for ln in lines] == out.decode().split()
    assert all(1 <= len(ln.split()) <= 5 and len(set(ln.split())) == len(ln.split()) for ln in lines)


@pytest.mark.parametrize("env", [dict(MATFACT_TOPN="0"), dict(MATFACT_TOPN="33"), dict(MATFACT_TOPN="ten"),
                                 dict(MATFACT_TOPN="3x"), dict(MATFACT_TOPN=""),
                                 dict(MATFACT_TOPN="3", MATFACT_DEVICES="0"), dict(MATFACT_TOPN="3", MATFACT_MATS="/dev/null"),
                                 dict(MATFACT_TOPN="3", MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_TOPN="3", MATFACT_RESUME="x.ck")])
def test_cli_topn_bad_values_die_with_empty_stdout(capi, env, tmp_path):
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(os.environ, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_TOPN" in r.stderr, r


@pytest.mark.gpu
def test_topn_cfg4_shape(gpu, orc):
    """1e6 x 1e5, K = 100, N = 10 (the bench workload's shape): column 0 is recommend() for every user, 256 sampled users
    equal the model; the times are printed."""
    capi = gpu
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.CONFIGS["cfg4"]
    U, I, K = cfg["users"], cfg["items"], cfg["feats"]
    row, col, val = capi.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], **bench.synth_args(cfg, "uniform"))
    L0, R0 = capi.init_factors(U, I, K)
    plan = capi.Plan(U, I, K, cfg["alpha"], row, col, val)
    plan.upload(L0, R0)
    best = plan.recommend()
    t0 = time.perf_counter()
    best = plan.recommend()
    t1 = time.perf_counter()
    it, sc = plan.recommend_topn(10)
    t2 = time.perf_counter()
    info = plan.recommend_topn_info()
    print("\ncfg4 top-1 %.3f s, top-10 %.3f s (first call), exact-pass users %d, form %d" % (t1 - t0, t2 - t1, *info))
    assert np.array_equal(it[:, 0], best)
    users = np.sort(np.random.default_rng(4).choice(U, 256, replace=False))
    ptr = np.searchsorted(row, np.arange(U + 1))
    sub_row = np.concatenate([np.full(ptr[u + 1] - ptr[u], t, np.int32) for t, u in enumerate(users)])
    sub_col = np.concatenate([col[ptr[u]:ptr[u + 1]] for u in users])
    mi, ms = model_topn(orc, len(users), I, sub_row, sub_col, L0[users], R0, 10)
    assert_same(it[users], sc[users], mi, ms)
    plan.close()
