"""Training and held-out loss (mf_plan_loss and friends), the monitored iteration loop and MATFACT_LOSS.

The contract (include/matfact_hip.h): p_n = dot(L[i_n], R[j_n]) sequential in k from 0.0 and unfused; q_n = (a_n - p_n)^2
formed as d * d; the row sum of a user adds its q_n from 0.0 in the order the caller gave the entries; users are cut into
blocks of 1024 counted from global user 0, a block sum adds its row sums in ascending order from 0.0, and SSE adds the block
sums in ascending order from 0.0.  The model below states that in numpy with np.cumsum (sequential; np.sum is pairwise).
Every comparison is on the int64 view of the doubles: equal bits, no tolerance anywhere.

CPU tests: declarations, argument checks before any HIP call, mf_backend_loss_total against the model, the model's dot
against the oracle, the ISA of the new kernels and of the untouched sweeps, the CLI's refusals.  GPU tests (-m gpu): every
kernel form against the model, unsorted input, held-out sets, NaN / inf, interleaving with iterate / recommend, the monitored
loop, shards, the golden ML100k factors, the CLI, the cfg4 shape.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in, random_instance

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa  # noqa: E402

BLOCK = 1024


# ------------------------------------------------------------------------------------------------ the model
def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def seq_sum(x):
    """(((0.0 + x0) + x1) + ...): np.cumsum is sequential."""
    return np.cumsum(np.concatenate([np.zeros(1), np.asarray(x, np.float64)]))[-1]


def model_p(L, R, row, col):
    """dot(L[row], R[col]) per entry: k ascending from 0.0, multiply and add as separate elementwise operations."""
    p = np.zeros(len(row))
    Lt, Rt = np.ascontiguousarray(L.T), np.ascontiguousarray(R.T)   # column k contiguous: the same values, gathered faster
    for k in range(L.shape[1]):
        p = p + Lt[k][row] * Rt[k][col]
    return p


def model_rows(L, R, row, col, val, users, user_begin=0):
    """s_i of the users [user_begin, user_begin + users): entries of a user in the order given (L holds these users' rows)."""
    row = np.asarray(row, np.int64) - user_begin
    col = np.asarray(col, np.int64)
    d = np.asarray(val, np.float64) - model_p(L, R, row, col)
    q = d * d
    order = np.argsort(row, kind="stable")
    ptr = np.searchsorted(row[order], np.arange(users + 1))
    q = q[order]
    return np.array([seq_sum(q[ptr[i]:ptr[i + 1]]) for i in range(users)], np.float64).reshape(users)


def model_total(s, user_begin=0):
    """Step 4: block sums over blocks cut at global multiples of 1024, then the sum of the block sums."""
    s = np.asarray(s, np.float64)
    T, i = [], 0
    while i < len(s):
        stop = min(len(s), ((user_begin + i) // BLOCK + 1) * BLOCK - user_begin)
        T.append(seq_sum(s[i:stop]))
        i = stop
    return seq_sum(T)


def assert_bits(a, b, where=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (where, a.shape, b.shape)
    bad = np.flatnonzero(bits(a).reshape(-1) != bits(b).reshape(-1))
    assert bad.size == 0, (where, bad[:5], a.reshape(-1)[bad[:5]], b.reshape(-1)[bad[:5]],
                           [hex(v) for v in bits(a).reshape(-1)[bad[:5]].view(np.uint64)], [hex(v) for v in bits(b).reshape(-1)[bad[:5]].view(np.uint64)])


def check_loss(plan, L, R, row, col, val, which="train", where=""):
    """plan.loss(which, rows=True) against the model over (row, col, val); returns the model's row sums."""
    out, rs = plan.loss(which, rows=True)
    ms = model_rows(L, R, row, col, val, plan.user_count, plan.user_begin)
    assert out.count == len(row), (where, out.count, len(row))
    assert_bits(rs, ms, where + " row_sse")
    assert_bits(out.sse, model_total(ms, plan.user_begin), where + " sse")
    return ms


def instance(seed, users, items, K, density=0.05, full=(3,), empty=(0, 5)):
    d = random_instance(seed, users, items, K, density=density, empty_rows=empty, full_rows=full, float_ratings=True)
    rng = np.random.default_rng(seed + 1000)
    L = rng.standard_normal((users, K)) * rng.choice([1e-3, 1.0, 30.0], (users, 1))
    R = rng.standard_normal((items, K))
    return d["row"], d["col"], d["val"], L, R


def _plan(capi, users, items, K, row, col, val, L, R, **kw):
    p = capi.Plan(users, items, K, 0.01, row, col, val, **kw)
    p.upload(L, R)
    return p


# ------------------------------------------------------------------------------------------------ CPU
LOSS_SYMBOLS = ("mf_plan_set_heldout", "mf_plan_loss", "mf_backend_loss_total", "mf_plan_iterate_monitored", "mf_backend_loss")


def test_loss_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    assert re.search(r"#define MF_LOSS_BLOCK 1024\b", hdr) and capi.MF_LOSS_BLOCK == 1024
    assert re.search(r"#define MF_LOSS_TRAIN 0\b", hdr) and re.search(r"#define MF_LOSS_HELDOUT 1\b", hdr)
    assert "typedef struct mf_loss {" in hdr and "typedef struct mf_loss_point {" in hdr
    for s in LOSS_SYMBOLS:
        assert s + "(" in hdr and s in capi.HIP_SYMBOLS
        assert hasattr(capi.hip(), s)
    assert C.sizeof(capi.Loss) == 16 and C.sizeof(capi.LossPoint) == 40
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr)
    assert capi.hip().mf_backend_abi_version() == 5


def test_loss_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    out = capi.Loss()
    one = np.zeros(1)
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    assert h.mf_plan_loss(None, 0, C.byref(out), None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_loss(fake, 0, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_loss(fake, 2, C.byref(out), None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_loss(fake, -1, C.byref(out), None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_set_heldout(None, 0, None, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_set_heldout(fake, -1, None, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_set_heldout(fake, 3, None, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_iterate_monitored(None, 1, 1, 0.0, None, 0, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_iterate_monitored(fake, -1, 1, 0.0, None, 0, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_iterate_monitored(fake, 5, 0, 0.0, None, 0, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_iterate_monitored(fake, 5, -2, 0.0, None, 0, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_iterate_monitored(fake, 5, 1, 0.0, None, 4, None, None) == capi.MF_ERR_ARGUMENT
    sse = C.c_double()
    assert h.mf_backend_loss_total(one.ctypes.data, 0, 1, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_loss_total(None, 0, 1, C.byref(sse)) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_loss_total(one.ctypes.data, -1, 1, C.byref(sse)) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_loss_total(one.ctypes.data, 0, -1, C.byref(sse)) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    assert h.mf_backend_loss(None, L.ctypes.data, R.ctypes.data, C.byref(out), None, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_loss(C.byref(p), None, R.ctypes.data, C.byref(out), None, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_loss(C.byref(p), L.ctypes.data, None, C.byref(out), None, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_loss(C.byref(p), L.ctypes.data, R.ctypes.data, None, None, 0) == capi.MF_ERR_ARGUMENT


def test_loss_without_a_gpu_fails_loudly(capi):
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    inst = capi.parse_file(golden_in("inst0"))
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    with pytest.raises(capi.HipBackendError) as e:
        capi.backend_loss(inst, L, R)
    assert e.value.status == capi.MF_ERR_NO_DEVICE


def _row_sums(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n) * 10.0 ** rng.integers(-8, 9, n)   # mixed magnitudes: the order of the additions shows in the bits


@pytest.mark.parametrize("user_begin", [0, 1, 1000, 1024])
@pytest.mark.parametrize("users", [0, 1, 1023, 1024, 1025, 5000])
def test_loss_total_equals_the_model(capi, users, user_begin):
    s = _row_sums(users, users + 7 * user_begin)
    assert_bits(capi.loss_total(s, user_begin), model_total(s, user_begin))
    if users >= 2:
        for bad in (np.nan, np.inf):
            t = s.copy()
            t[users // 2] = bad
            got = capi.loss_total(t, user_begin)
            assert_bits(got, model_total(t, user_begin))
            assert np.isnan(got) if np.isnan(bad) else np.isinf(got)
        t = s.copy()
        t[0], t[-1] = np.inf, np.nan
        assert_bits(capi.loss_total(t, user_begin), model_total(t, user_begin))


def test_loss_total_is_sequential_and_blocked(capi):
    """pins the model: np.cumsum equals a Python loop bit for bit; the blocked total differs from one plain chain over all
    users on this data, so a total without the blocks cannot pass"""
    s = _row_sums(5000, 3)
    acc = 0.0
    for x in s[:1024]:
        acc = acc + x
    assert_bits(seq_sum(s[:1024]), acc)
    total = capi.loss_total(s)
    assert bits(total) != bits(seq_sum(s))


def test_shard_totals_do_not_add_but_row_sums_concatenate(capi):
    s = _row_sums(5000, 11)
    single = capi.loss_total(s)
    assert_bits(single, model_total(s))
    rng = np.random.default_rng(5)
    differs = 0
    for trial in range(8):
        cuts = np.sort(rng.choice(np.arange(1, 5000), 3, replace=False))
        parts = np.split(s, cuts)
        begins = np.concatenate([[0], cuts])
        totals = [capi.loss_total(part, int(b)) for part, b in zip(parts, begins)]
        for part, b, t in zip(parts, begins, totals):
            assert_bits(t, model_total(part, int(b)))
        differs += bits(seq_sum(totals)) != bits(single)
        assert_bits(capi.loss_total(np.concatenate(parts)), single)
    assert differs > 0, "adding shard totals happened to reproduce the single total on every cut: the test cannot tell"


@pytest.mark.parametrize("seed,K", [(0, 7), (1, 20), (2, 64)])
def test_model_dot_is_the_oracle_prediction(orc, seed, K):
    row, col, val, L, R = instance(seed, 40, 60, K, density=0.2)
    p = model_p(L, R, row.astype(np.int64), col.astype(np.int64))
    for u in range(40):
        b = orc.predict_row(np.ascontiguousarray(L[u]), R)
        sel = row == u
        assert_bits(p[sel], b[col[sel]])


ACC = re.compile(r"mf::sweep_dma_kernel<\d+, \d+, 0, \d+>")


def test_loss_kernels_isa(capi):
    if not isa.have_tools() or not os.path.exists(isa.DEFAULT_LIB):
        pytest.skip("needs llvm-objdump/llvm-readelf/c++filt and the built library")
    kernels = isa.disassemble()
    meta = isa.metadata()
    dma = [n for n in kernels if "mf::loss_dma_kernel<" in n]
    assert len(dma) == 11, dma   # K = 10, 20, 30, 50, 100, 128, 256 and the run-time-K forms of 1, 2, 4, 8 passes
    rest = [n for n in kernels if re.search(r"mf::loss_(reg|block|total)_kernel", n)]
    assert len(rest) == 3, rest
    for n in dma:
        assert any(i.startswith("global_load_lds_dwordx4") for i in kernels[n]), n
    for n in dma + rest:
        body = kernels[n]
        fused = [i for i in body if re.match(r"v_(fma|fmac|mad|pk_fma)\w*_f64", i) and "_dpp" not in isa.split(i)[0]]
        assert not fused, (n, fused[:3])
        assert not [i for i in body if i.startswith("scratch_")], n
        m = meta[n]
        assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0 and m[".sgpr_spill_count"] == 0, (n, m)
        stores = [i for i in body if re.match(r"(global|flat|buffer)_store|s_\w*store", i)]
        assert stores and all(i.startswith("global_store_dwordx2") for i in stores), (n, stores)
        assert any(isa.split(i)[0].startswith("v_readlane_b32") for i in body), n   # the ordered chain
    # the sweeps' accumulate instances keep the instruction counts recorded for them (re-recorded when the kernel was
    # assembled from shared pieces: scalar compare / branch / ALU counts and the compiler's s_nop padding moved; every vector,
    # LDS, memory and wait count stayed, but for two more v_readlane / v_writelane pairs in <0, 8, 0, 0>)
    want = json.load(open(os.path.join(GOLDEN, "sweep_dma_accumulate_census.json")))
    acc = {n: isa.census(b) for n, b in kernels.items() if ACC.search(n)}
    assert sorted(acc) == sorted(want), sorted(set(acc) ^ set(want))
    for n in acc:
        assert acc[n] == want[n], (n, {k: (acc[n].get(k), want[n].get(k)) for k in set(acc[n]) | set(want[n])
                                       if acc[n].get(k) != want[n].get(k)})


@pytest.mark.parametrize("env", [dict(MATFACT_LOSS="0"), dict(MATFACT_LOSS="-3"), dict(MATFACT_LOSS="five"), dict(MATFACT_LOSS=""),
                                 dict(MATFACT_LOSS="5x"), dict(MATFACT_LOSS="5,"), dict(MATFACT_LOSS="5,abc"),
                                 dict(MATFACT_LOSS="5", MATFACT_DEVICES="0"), dict(MATFACT_LOSS="5", MATFACT_RESUME="x.ck"),
                                 dict(MATFACT_LOSS="5", MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_LOSS="5", MATFACT_TOPN="3"),
                                 dict(MATFACT_LOSS="5", MATFACT_MATS="/dev/null")])
def test_cli_loss_refusals_die_with_empty_stdout(capi, env, tmp_path):
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(os.environ, **env))
    assert r.returncode == 255 and r.stdout == b"" and (b"MATFACT_LOSS" in r.stderr or b"MATFACT_TOPN" in r.stderr), r


def test_cli_heldout_needs_loss_and_a_matching_header(capi, tmp_path):
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path,
                       env=dict(os.environ, MATFACT_HELDOUT=golden_in("inst0")))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_HELDOUT needs MATFACT_LOSS" in r.stderr, r
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path,
                       env=dict(os.environ, MATFACT_LOSS="5", MATFACT_HELDOUT=golden_in("inst30-40-10-2-10")))
    assert r.returncode == 255 and r.stdout == b"" and b"Error in multiple int argument." in r.stderr, r
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path,
                       env=dict(os.environ, MATFACT_LOSS="5", MATFACT_HELDOUT=str(tmp_path / "missing.in")))
    assert r.returncode == 255 and r.stdout == b"" and b"Unable to open input file." in r.stderr, r


# ------------------------------------------------------------------------------------------------ GPU
KS = [1, 2, 7, 10, 20, 30, 50, 62, 64, 100, 128, 130, 256, 300, 511, 513, 1024, 1026, 4095]


def loss_shape(K):
    """users x items of the every-K instance: 1100 x 260, and 100 x 100 where a factor row is 32 KiB"""
    return (1100, 260) if K <= 2048 else (100, 100)


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.mark.gpu
@pytest.mark.parametrize("impl", ["dma", "reg"])
@pytest.mark.parametrize("K", KS)
def test_loss_every_k_equals_the_model(gpu, K, impl, monkeypatch):
    """1100 users (not a multiple of 1024) x 260 items: users 0 and 5 empty, user 3 rated everything (260 entries: more
    than 64 * 3, so the chain crosses chunks at every chunk size).  Above K = 300: the last odd and the first odd K of two
    register counts (511, 513), the eight full passes of the run-time-K LDS-DMA row sums (1024), the first even K past them
    (1026) and the plan at the edge of a CU's LDS (4095, on 100 x 100: user 3 has 100 entries, 20 chunks of five)."""
    capi = gpu
    if impl == "reg":
        monkeypatch.setenv("MF_SWEEP_IMPL", "reg")
    U, I = loss_shape(K)
    row, col, val, L, R = instance(K, U, I, K)
    plan = _plan(capi, U, I, K, row, col, val, L, R)
    desc = plan.describe()
    assert ("loss=loss_dma_kernel(" if impl == "dma" and K % 2 == 0 and K <= 1024 else "loss=loss_reg_kernel(") in desc, desc
    if K > 300:
        assert desc.startswith("sweep_dma_kernel<KT=0,NPASS=8> " if "loss=loss_dma_kernel(" in desc else
                               "sweep_kernel<KT=0,KPMAX=%d> " % next(kp for kp in (8, 16, 32, 64) if K <= 64 * kp)), desc
    ms = check_loss(plan, L, R, row, col, val, where="K=%d %s" % (K, impl))
    assert ms[0] == 0.0 and ms[5] == 0.0 and bits(ms[0]) == 0
    out = capi.backend_loss(capi.Instance(1, 0.01, K, U, I, row, col, val), L, R)
    assert_bits(out.sse, model_total(ms))
    assert out.count == len(row)
    assert out.rmse == float(np.sqrt(out.sse / out.count))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nch", ["1", "5", "64"])
@pytest.mark.parametrize("K", [7, 30, 100])
def test_loss_is_the_same_bits_at_every_chunk_size(gpu, K, nch, monkeypatch):
    capi = gpu
    monkeypatch.setenv("MF_SWEEP_NCH", nch)
    row, col, val, L, R = instance(50 + K, 300, 200, K, density=0.1)
    plan = _plan(capi, 300, 200, K, row, col, val, L, R)
    assert "(nch=%s/%s " % (nch, nch) in plan.describe(), plan.describe()
    check_loss(plan, L, R, row, col, val, where="K=%d nch=%s" % (K, nch))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("users", [2500, 40000])
def test_loss_many_users_and_launch_orders(gpu, users):
    """more users than one block of the total and than the few-rows chunk rule (2048); 40000 users with one long row
    take the longest-first order of the row list"""
    capi = gpu
    K = 20
    row, col, val, L, R = instance(users, users, 300, K, density=0.02, full=(7, users - 1))
    plan = _plan(capi, users, 300, K, row, col, val, L, R)
    check_loss(plan, L, R, row, col, val, where="users=%d" % users)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [7, 20, 100])
def test_loss_row_sum_follows_the_file_order(gpu, K):
    capi = gpu
    row, col, val, L, R = instance(77 + K, 200, 300, K, density=0.2)
    rng = np.random.default_rng(9)
    perm = rng.permutation(len(row))          # entries of every user shuffled, and the users interleaved
    urow, ucol, uval = row[perm], col[perm], val[perm]
    plan = _plan(capi, 200, 300, K, urow, ucol, uval, L, R)
    ms = check_loss(plan, L, R, urow, ucol, uval, where="unsorted")
    sorted_ms = model_rows(L, R, row, col, val, 200)
    assert (bits(ms) != bits(sorted_ms)).any(), "the shuffled order gives the sorted order's bits: the test cannot tell"
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [7, 30, 100, 513, 1024])
def test_heldout_sets(gpu, K):
    capi = gpu
    U, I = 1500, 240
    row, col, val, L, R = instance(300 + K, U, I, K, density=0.1)
    plan = _plan(capi, U, I, K, row, col, val, L, R)
    with pytest.raises(capi.HipBackendError) as e:
        plan.loss("heldout")
    assert e.value.status == capi.MF_ERR_STATE
    rng = np.random.default_rng(K)
    rated = np.zeros((U, I), bool)
    rated[row, col] = True
    # disjoint from the training set, sorted; users 0..9 and every user from 1200 on have no held-out entry
    hr, hc = np.nonzero(~rated & (rng.random((U, I)) < 0.03))
    keep = (hr >= 10) & (hr < 1200)
    hr, hc = hr[keep].astype(np.int32), hc[keep].astype(np.int32)
    hv = rng.random(len(hr)) * 5
    plan.set_heldout(hr, hc, hv)
    hs = check_loss(plan, L, R, hr, hc, hv, "heldout", "disjoint")
    assert (hs[:10] == 0.0).all() and (hs[1200:] == 0.0).all()
    check_loss(plan, L, R, row, col, val, "train", "train beside a held-out set")
    # replaced by a second set: unsorted, overlapping the training pairs, with repeated pairs, one user with 400 entries
    sel = rng.choice(len(row), 3000, replace=False)
    r2 = np.concatenate([row[sel], hr[:500], hr[:500], np.full(400, 33, np.int32)])
    c2 = np.concatenate([col[sel], hc[:500], hc[:500], rng.integers(0, I, 400).astype(np.int32)])
    v2 = rng.random(len(r2)) * 5
    perm = rng.permutation(len(r2))
    r2, c2, v2 = r2[perm], c2[perm], v2[perm]
    plan.set_heldout(r2, c2, v2)
    check_loss(plan, L, R, r2, c2, v2, "heldout", "replaced, unsorted, overlapping")
    # a bad triple changes nothing
    for br, bc in ((U, 0), (-1, 0), (0, I), (0, -1)):
        with pytest.raises(capi.HipBackendError) as e:
            plan.set_heldout(np.array([1, br], np.int32), np.array([1, bc], np.int32), np.ones(2))
        assert e.value.status == capi.MF_ERR_ARGUMENT
    check_loss(plan, L, R, r2, c2, v2, "heldout", "after refused sets")
    plan.set_heldout(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(capi.HipBackendError) as e:
        plan.loss("heldout")
    assert e.value.status == capi.MF_ERR_STATE
    check_loss(plan, L, R, row, col, val, "train", "train after removal")
    plan.close()


@pytest.mark.gpu
def test_loss_before_upload_is_a_state_error(gpu):
    capi = gpu
    row, col, val, L, R = instance(1, 50, 40, 10, density=0.2)
    plan = capi.Plan(50, 40, 10, 0.01, row, col, val)
    with pytest.raises(capi.HipBackendError) as e:
        plan.loss()
    assert e.value.status == capi.MF_ERR_STATE
    with pytest.raises(capi.HipBackendError) as e:
        plan.iterate_monitored(3)
    assert e.value.status == capi.MF_ERR_STATE
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [7, 20, 100])
def test_loss_nan_and_inf_propagate(gpu, K):
    capi = gpu
    U, I = 2100, 150
    row, col, val, L, R = instance(500 + K, U, I, K, density=0.05, full=(), empty=())
    L = L.copy()
    R = R.copy()
    L[40, K // 2] = np.nan      # user 40's row sum is NaN
    L[1500, 0] = np.inf         # user 1500's is inf or NaN by the rules
    R[I - 1, K - 1] = -np.inf   # every user who rated the last item
    plan = _plan(capi, U, I, K, row, col, val, L, R)
    ms = check_loss(plan, L, R, row, col, val, where="non-finite")
    touched = np.zeros(U, bool)
    touched[[40, 1500]] = True
    touched[row[col == I - 1]] = True
    assert not np.isfinite(ms[touched & (np.bincount(row, minlength=U) > 0)]).any()
    assert np.isfinite(ms[~touched]).all()
    assert not np.isfinite(plan.loss().sse)
    plan.close()


def _ml100k(capi):
    inst = capi.parse_file(golden_in("instML100k"))
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    return inst, L0, R0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sweeps", "es"])
def test_loss_does_not_disturb_the_run(gpu, mode, monkeypatch):
    capi = gpu
    monkeypatch.setenv("MF_ITER_MODE", mode)
    inst, L0, R0 = _ml100k(capi)
    a, b = 7, 6
    ref = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    ref.upload(L0, R0)
    assert ("iterate=errors" in ref.describe()) == (mode == "es"), ref.describe()
    ref.iterate(a + b)
    Lr, Rr = ref.download()
    best = ref.recommend()
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    plan.upload(L0, R0)
    plan.iterate(a)
    La, Ra = plan.download()
    check_loss(plan, La, Ra, inst.row, inst.col, inst.val, where="after %d iterations" % a)
    plan.iterate(b)
    L, R = plan.download()
    assert_bits(L, Lr, "L")
    assert_bits(R, Rr, "R")
    assert np.array_equal(plan.recommend(), best)
    plan.loss()
    assert np.array_equal(plan.recommend(), best)
    L, R = plan.download()
    assert_bits(L, Lr, "L after loss")
    assert_bits(R, Rr, "R after loss")
    ref.close()
    plan.close()


@pytest.mark.gpu
def test_iterate_monitored(gpu):
    capi = gpu
    inst, L0, R0 = _ml100k(capi)
    rng = np.random.default_rng(1)
    hsel = rng.choice(inst.nnz, 5000, replace=False)
    tmask = np.ones(inst.nnz, bool)
    tmask[hsel] = False
    tr = (inst.row[tmask], inst.col[tmask], inst.val[tmask])
    ho = (inst.row[hsel], inst.col[hsel], inst.val[hsel])

    def fresh(heldout):
        p = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, *tr)
        p.upload(L0, R0)
        if heldout:
            p.set_heldout(*ho)
        return p

    # every = 3, iters = 10: points at 0, 3, 6, 9, 10, each equal to a separate loss() at that iteration
    plan = fresh(True)
    done, pts = plan.iterate_monitored(10, every=3, tol=0.0)
    assert done == 10 and [p.iter for p in pts] == [0, 3, 6, 9, 10]
    Lm, Rm = plan.download()
    other = fresh(True)
    at = 0
    for p in pts:
        other.iterate(p.iter - at)
        at = p.iter
        t, h = other.loss("train"), other.loss("heldout")
        assert_bits([p.train.sse, p.heldout.sse], [t.sse, h.sse], "point %d" % p.iter)
        assert (p.train.count, p.heldout.count) == (t.count, h.count) == (len(tr[0]), 5000)
    Lo, Ro = other.download()
    assert_bits(Lm, Lo)
    assert_bits(Rm, Ro)
    La, Ra = other.download()
    check_loss(other, La, Ra, *tr, "train", "last point, training")
    check_loss(other, La, Ra, *ho, "heldout", "last point, held-out")
    other.close()
    plan.close()

    # without a held-out set the points carry {0.0, 0} and the rule looks at the training RMSE
    for heldout in (False, True):
        plan = fresh(heldout)
        done, pts = plan.iterate_monitored(24, every=2, tol=0.0)
        assert done == 24 and [p.iter for p in pts] == list(range(0, 25, 2))   # tol = 0: nothing stops the loop
        if not heldout:
            assert all(p.heldout.sse == 0.0 and p.heldout.count == 0 for p in pts)
        rm = [(p.heldout if heldout else p.train).rmse for p in pts]
        print("\nmonitored rmse (heldout=%s):" % heldout, " ".join("%.6f" % r for r in rm))
        rel = [(rm[i - 1] - rm[i]) / rm[i - 1] for i in range(1, len(rm))]
        # a tol between two neighbouring relative improvements, so that the rule fires at a known point: the first i with
        # rm[i-1] - rm[i] <= tol * rm[i-1], evaluated with the library's own expression
        order = np.argsort(rel)
        tol = 0.5 * (rel[order[len(rel) // 2]] + rel[order[len(rel) // 2 + 1]])
        fire = next(i for i in range(1, len(rm)) if rm[i - 1] - rm[i] <= tol * rm[i - 1])
        plan.close()
        plan = fresh(heldout)
        done, pts2 = plan.iterate_monitored(24, every=2, tol=tol)
        assert done == 2 * fire and [p.iter for p in pts2] == list(range(0, 2 * fire + 1, 2)), (done, fire, tol, rel)
        for p, q in zip(pts2, pts):
            assert_bits([p.train.sse, p.heldout.sse], [q.train.sse, q.heldout.sse])
        L, R = plan.download()
        plan.close()
        plan = fresh(heldout)
        plan.iterate(done)
        L2, R2 = plan.download()
        assert_bits(L, L2)
        assert_bits(R, R2)
        # iters = 0: the single point at 0; a tol that any first step satisfies stops at the second point
        assert plan.iterate_monitored(0, every=5, tol=0.5)[0] == 0
        d, pp = plan.iterate_monitored(9, every=4, tol=1e9)
        assert d == 4 and len(pp) == 2
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, 700, 1024, 1500, 2999])
def test_two_shards_combine_through_the_row_sums(gpu, cut):
    capi = gpu
    U, I, K = 3000, 200, 30
    row, col, val, L, R = instance(cut, U, I, K, density=0.05)
    single = _plan(capi, U, I, K, row, col, val, L, R)
    want, ws = single.loss(rows=True)
    lo = row < cut
    a = _plan(capi, U, I, K, row[lo], col[lo], val[lo], L[:cut], R, user_begin=0, user_count=cut)
    b = _plan(capi, U, I, K, row[~lo], col[~lo], val[~lo], L[cut:], R, user_begin=cut, user_count=U - cut)
    la, sa = a.loss(rows=True)
    lb, sb = b.loss(rows=True)
    assert_bits(np.concatenate([sa, sb]), ws)
    assert_bits(capi.loss_total(np.concatenate([sa, sb])), want.sse)
    assert la.count + lb.count == want.count
    # a shard's own total is step 4 over its users, blocks cut at global multiples of 1024
    assert_bits(la.sse, model_total(sa, 0))
    assert_bits(lb.sse, model_total(sb, cut))
    assert_bits(lb.sse, capi.loss_total(sb, cut))
    for p in (single, a, b):
        p.close()


@pytest.mark.gpu
def test_loss_golden_ml100k(gpu):
    capi = gpu
    inst, L0, R0 = _ml100k(capi)
    z = np.load(os.path.join(GOLDEN, "instML100k.factors.npz"))
    Lg, Rg = np.ascontiguousarray(z["L_full"]), np.ascontiguousarray(z["R_full"])
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    plan.upload(L0, R0)
    done, pts = plan.iterate_monitored(inst.iters, every=max(inst.iters // 4, 1))
    assert done == inst.iters
    L, R = plan.download()
    assert_bits(L, Lg)
    assert_bits(R, Rg)
    ms = model_rows(Lg, Rg, inst.row, inst.col, inst.val, inst.users)
    assert_bits(pts[-1].train.sse, model_total(ms))
    assert pts[-1].train.count == inst.nnz
    out = capi.backend_loss(inst, Lg, Rg)
    assert_bits(out.sse, model_total(ms))
    print("\nML100k training rmse: %.6f -> %.6f after %d iterations" % (pts[0].train.rmse, pts[-1].train.rmse, done))
    assert pts[-1].train.rmse < pts[0].train.rmse   # a sanity line, not a bound
    plan.close()


def _cli_input(name, tmp_path):
    path = golden_in(name)
    if path.endswith(".gz"):
        import gzip
        raw = gzip.open(path, "rb").read()
        path = str(tmp_path / (name + ".in"))
        open(path, "wb").write(raw)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "instML100k"])
def test_cli_loss(gpu, name, tmp_path):
    capi = gpu
    path = _cli_input(name, tmp_path)
    inst = capi.parse_file(path)
    plain = subprocess.run([capi.CLI_PATH, path], capture_output=True)
    assert plain.returncode == 0 and plain.stdout == open(os.path.join(GOLDEN, name + ".out"), "rb").read()
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(os.environ, MATFACT_LOSS="5"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout
    lines = [ln.split() for ln in r.stderr.decode().splitlines() if ln.startswith("iter ")]
    want_iters = sorted(set(list(range(0, inst.iters + 1, 5)) + [inst.iters]))
    assert [int(ln[1]) for ln in lines] == want_iters
    assert all(len(ln) == 4 and ln[2] == "train_rmse" for ln in lines)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    plan.upload(L0, R0)
    at = 0
    for ln in lines[:4] + lines[-1:]:
        plan.iterate(int(ln[1]) - at)
        at = int(ln[1])
        L, R = plan.download()
        sse = model_total(model_rows(L, R, inst.row, inst.col, inst.val, inst.users))
        assert_bits(float(ln[3]), np.sqrt(sse / inst.nnz), "stderr line of iteration %d" % at)
    plan.close()
    # a held-out file (the instance itself: overlapping pairs are allowed) adds the third column; tol stops early
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(os.environ, MATFACT_LOSS="5", MATFACT_HELDOUT=path))
    assert r.returncode == 0 and r.stdout == plain.stdout
    l2 = [ln.split() for ln in r.stderr.decode().splitlines() if ln.startswith("iter ")]
    assert len(l2) == len(lines) and all(len(ln) == 6 and ln[4] == "heldout_rmse" and ln[5] == ln[3] for ln in l2)
    assert [ln[:4] for ln in l2] == lines
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(os.environ, MATFACT_LOSS="5,1e9"))
    assert r.returncode == 0
    assert [ln.split()[1] for ln in r.stderr.decode().splitlines() if ln.startswith("iter ")] == ["0", "5"]
    best = capi.backend_run(inst, *capi.init_factors(inst.users, inst.items, inst.feats), iters=5)
    assert r.stdout == "".join("%d\n" % b for b in best if b >= 0).encode()


def _synthetic(capi, scale):
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.CONFIGS["cfg4"]
    U, I, K = cfg["users"] // scale, cfg["items"] // scale, cfg["feats"]
    row, col, val = capi.synth_block(cfg["seed"], U, I, cfg["min_row"], cfg["max_row"], columns="uniform",
                                     target_nnz=cfg["nnz"] // scale)
    assert len(row) == cfg["nnz"] // scale
    L0, R0 = capi.init_factors(U, I, K)
    plan = capi.Plan(U, I, K, cfg["alpha"], row, col, val)
    plan.upload(L0, R0)
    plan.iterate(1)
    return plan, U, I, K, row, col, val


@pytest.mark.gpu
def test_loss_tenth_of_the_cfg4_shape_in_full(gpu):
    """1e5 x 1e4, K = 100, 1e7 entries (cfg4 at a tenth of every dimension): every row sum and the total against the model."""
    capi = gpu
    plan, U, I, K, row, col, val = _synthetic(capi, 10)
    L, R = plan.download()
    t0 = time.perf_counter()
    check_loss(plan, L, R, row, col, val, where="tenth of cfg4")
    print("\ntenth-size model and comparison: %.1f s for %d entries" % (time.perf_counter() - t0, len(row)))
    plan.close()


@pytest.mark.gpu
def test_loss_cfg4_shape(gpu):
    """1e6 x 1e5, K = 100, 1e8 entries (the bench workload's shape), after one iteration: all 1e6 row sums and the total
    against the numpy model (2e10 gathered elements; measured: 34 s of host time, printed by the test), and the device
    SSE against mf_backend_loss_total over the downloaded row sums.
    Backstop on time (a condition, not a target): the loss call takes at most twice the user sweep of the same plan, both
    measured here."""
    capi = gpu
    plan, U, I, K, row, col, val = _synthetic(capi, 1)
    L, R = plan.download()
    out, rs = plan.loss(rows=True)
    assert out.count == len(row) == 100_000_000
    assert_bits(out.sse, capi.loss_total(rs))
    t0 = time.perf_counter()
    ms = model_rows(L, R, row, col, val, U)
    print("\ncfg4: numpy model of %d entries, %d users: %.1f s" % (len(row), U, time.perf_counter() - t0))
    assert_bits(rs, ms, "all row sums")
    assert_bits(out.sse, model_total(ms))
    del L, ms
    # time: the user sweep by the plan's own events, the loss call by the host clock around it (it ends synchronised)
    plan.timing(True)
    plan.iterate(1)
    plan.loss()
    plan.timing_read()
    loss_ms, sweep_ms = [], []
    for rep in range(5):
        plan.iterate(1)
        t = plan.timing_read()
        sweep_ms.append(t["user_ms"] / t["user_launches"])
        t0 = time.perf_counter()
        plan.loss()
        loss_ms.append((time.perf_counter() - t0) * 1e3)
    print("cfg4: loss %s ms, user sweep %s ms, ratio of the minima %.3f" % (
        " ".join("%.2f" % x for x in loss_ms), " ".join("%.2f" % x for x in sweep_ms), min(loss_ms) / min(sweep_ms)))
    assert min(loss_ms) <= 2.0 * min(sweep_ms), (loss_ms, sweep_ms)
    plan.close()
