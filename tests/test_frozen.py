"""Frozen factor columns (mf_plan_set_frozen_columns) in every sweep form, and the biased model on top of them
(mf_backend_bias_mean / _pack / _unpack, mf_backend_run_biased, MATFACT_BIAS).

The definition is the library's own (include/matfact_hip.h): each side has one frozen column f or -1; after a sweep of side
X, X_new[r][f] = X_old[r][f] when the sweep is seeded and 0.0 when it is not, for every row, whatever e_n, Y and the decay
are; every other column is what it is without a frozen column.  The numpy model is the one of test_regularised.py plus that
one line (freeze below).  Every GPU comparison is bit for bit (assert_same_bits of test_sweep_edges.py).

The biased model a ~ mu + b_user + b_item + l.r is the K = F + 2 product of L' = [L | b_user | 1.0] (users' column F+1
frozen) and R' = [R | 1.0 | b_item] (items' column F frozen); test_explicit_bias_model_is_the_packed_frozen_model is the
evidence, on the CPU, that the two are the same numbers.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in
from test_loss import check_loss, model_rows, model_total
from test_rank import heldout_for, model_ranks
from test_regularised import (CASES, LAM_I, LAM_U, LARGE, ZERO_FORMS, Model, Side, _case_id, _pick, _single_wave, _small, _step, _toy,
                              decay, differs, expected, fast_dot, model_sweep)
from test_sweep_edges import CLASSES, FORMS, SWITCHES, assert_same_bits, cls_signed, pattern, seq_dot, signed_inputs
from test_topn import assert_same, model_topn

gpu = pytest.mark.gpu

FROZEN_SYMBOLS = ("mf_plan_set_frozen_columns", "mf_plan_get_frozen_columns", "mf_backend_bias_mean", "mf_backend_bias_pack",
                  "mf_backend_bias_unpack", "mf_backend_run_biased")


# ------------------------------------------------------------------------------------------------ the model
def freeze(new, old, f, seeded):
    """the one line on top of model_sweep: column f is X_old's when seeded and 0.0 otherwise"""
    if f < 0:
        return new
    new = new.copy()
    new[:, f] = old[:, f] if seeded else 0.0
    return new


def fstep(m, L, R, lam_u, lam_i, fu, fi, seed_u=True, seed_i=True, dot=seq_dot):
    Ln, Rn = m.step(L, R, lam_u, lam_i, seed_u, seed_i, dot)
    return freeze(Ln, L, fu, seed_u), freeze(Rn, R, fi, seed_i)


def fiterate(m, L, R, iters, lam_u, lam_i, fu, fi):
    for _ in range(iters):
        L, R = fstep(m, L, R, lam_u, lam_i, fu, fi, dot=fast_dot)
    return L, R


def ordered_sum(start, e, side):
    """((start_r + e_0) + e_1) + ... over the entries of every row in the side's order"""
    if side.maxlen == 0:
        return start
    run = np.cumsum(np.concatenate([start[:, None], e[side.pad]], axis=1), axis=1)
    return np.ascontiguousarray(run[side.rows, side.lens])


class BiasModel:
    """The biased model with its biases as vectors of their own: p = (dot_F + bu) + bi, e = c2 * (val - p), the latent
    columns by the regularised rule and b_new = b * d + sum e_n in entry order.  Nothing is multiplied by 1.0."""

    def __init__(self, users, items, row, col, val, alpha):
        self.row, self.col = np.asarray(row, np.int64), np.asarray(col, np.int64)
        self.val, self.alpha = np.asarray(val, np.float64), float(alpha)
        self.us, self.its = Side(self.row, users), Side(self.col, items)

    def step(self, L, R, bu, bi, lam_u, lam_i, dot=seq_dot):
        with np.errstate(all="ignore"):
            c2 = self.alpha * 2
            p = (dot(L, R, self.row, self.col) + bu[self.row]) + bi[self.col]
            e = c2 * (self.val - p)
            du, di = decay(self.alpha, lam_u), decay(self.alpha, lam_i)
            Ln = model_sweep(L, R, e, self.us, self.col, du, True)
            Rn = model_sweep(R, L, e, self.its, self.row, di, True)
            return Ln, Rn, ordered_sum(bu * du, e, self.us), ordered_sum(bi * di, e, self.its)

    def iterate(self, L, R, bu, bi, iters, lam_u, lam_i):
        for _ in range(iters):
            L, R, bu, bi = self.step(L, R, bu, bi, lam_u, lam_i, dot=fast_dot)
        return L, R, bu, bi


def seq_mean(val):
    """s = ((0.0 + v_0) + v_1) + ..., mu = s / n; 0.0 for nothing"""
    val = np.asarray(val, np.float64)
    if len(val) == 0:
        return 0.0
    return float(np.cumsum(np.concatenate([np.zeros(1), val]))[-1] / float(len(val)))


def pack(X, b, side):
    """users (side 1): [X | b | 1.0]; items (side 0): [X | 1.0 | b]"""
    one = np.ones((X.shape[0], 1))
    return np.ascontiguousarray(np.concatenate([X, b[:, None], one] if side == 1 else [X, one, b[:, None]], axis=1))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def fexpected(pat_name, cls, K, lam_u, lam_i, fu, fi):
    """The inputs and the free model's results of test_regularised.expected, and the frozen model's on the same inputs;
    computed once and shared.  The guards keep the inputs doing their job."""
    base = expected(pat_name, cls, K, lam_u, lam_i)
    x = type("FrozenExpected", (), {})()
    x.base, x.pat, x.K, x.L0, x.R0, x.val, x.alpha, x.model = base, base.pat, K, base.L0, base.R0, base.val, base.alpha, base.model
    x.seeded = (freeze(base.seeded[0], x.L0, fu, True), freeze(base.seeded[1], x.R0, fi, True))
    x.unseeded = (freeze(base.unseeded[0], x.L0, fu, False), freeze(base.unseeded[1], x.R0, fi, False))
    x.two = fstep(x.model, *x.seeded, lam_u, lam_i, fu, fi)
    for new, free, old, f in ((x.seeded[0], base.seeded[0], x.L0, fu), (x.seeded[1], base.seeded[1], x.R0, fi)):
        if f < 0:
            continue
        assert same_bits(new[:, f], old[:, f])
        if cls == "signed":
            # the free model changes the frozen column in more than half of its rows: a kernel that ignores the index fails
            changed = (free[:, f].view(np.uint64) != old[:, f].view(np.uint64)).mean()
            assert changed > 0.5, (pat_name, K, f, changed)
        if cls == "nonfinite":
            # at least one row takes a non-finite e_n, all its free columns are NaN and the frozen one is finite: zeroing
            # Y or e_n instead of selecting the result (NaN * 0) fails
            rest = np.delete(new, f, axis=1)
            hit = np.isnan(rest).all(axis=1) & np.isfinite(old[:, f])
            assert hit.any() and np.isnan(free[hit, f]).all(), (pat_name, K, f)
    if cls == "nonfinite":
        with np.errstate(all="ignore"):
            e = (x.alpha * 2) * (x.val - seq_dot(x.L0, x.R0, x.pat.row, x.pat.col))
        assert (~np.isfinite(e)).any()
    return x


# ------------------------------------------------------------------------------------------------ CPU
def test_frozen_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in FROZEN_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr) and capi.hip().mf_backend_abi_version() == 5
    for name in ("set_frozen_columns", "frozen_columns"):
        assert callable(getattr(capi.Plan, name))
    for name in ("bias_mean", "bias_pack", "bias_unpack", "backend_run_biased"):
        assert callable(getattr(capi, name))


def test_frozen_argument_errors_come_before_any_hip_call(capi):
    """A column below -1, NULL pointers, bad lambdas and an F too wide are refused without a device.  A column >= K can only
    be told with a plan, which needs a device: test_frozen_column_out_of_range_is_refused."""
    h = capi.hip()
    a, b = C.c_int32(), C.c_int32()
    fake = C.c_void_p(1)   # never dereferenced: a column below -1 is refused before the plan is looked at
    assert h.mf_plan_set_frozen_columns(None, 0, 0) == capi.MF_ERR_ARGUMENT
    for bad in (-2, -3, -(2 ** 31)):
        assert h.mf_plan_set_frozen_columns(fake, bad, 0) == capi.MF_ERR_ARGUMENT, bad
        assert h.mf_plan_set_frozen_columns(fake, 0, bad) == capi.MF_ERR_ARGUMENT, bad
    assert h.mf_plan_get_frozen_columns(None, C.byref(a), C.byref(b)) == capi.MF_ERR_ARGUMENT
    mu = C.c_double()
    v = np.ones(3)
    out = np.zeros((3, 3))
    assert h.mf_backend_bias_mean(v.ctypes.data, 3, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_mean(None, 3, C.byref(mu)) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_mean(v.ctypes.data, -1, C.byref(mu)) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_pack(None, None, 3, 1, 1, out.ctypes.data) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_pack(v.ctypes.data, None, 3, 1, 1, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_pack(v.ctypes.data, None, 3, 0, 1, out.ctypes.data) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_pack(v.ctypes.data, None, 3, 1, 2, out.ctypes.data) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_unpack(None, 3, 1, 1, v.ctypes.data, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_bias_unpack(out.ctypes.data, 3, 1, -1, v.ctypes.data, None) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    bu, bi = np.zeros(inst.users), np.zeros(inst.items)
    assert h.mf_backend_run_biased(None, L, R, bu, bi, C.byref(mu), None, 0.1, 0.1, 0) == capi.MF_ERR_ARGUMENT
    run = C.CDLL(h._name).mf_backend_run_biased   # a handle of its own: NULL factors, which the declared ndpointer would refuse itself
    run.argtypes = [C.c_void_p] * 7 + [C.c_double, C.c_double, C.c_int]
    ptr = [C.addressof(p), L.ctypes.data, R.ctypes.data, bu.ctypes.data, bi.ctypes.data, C.addressof(mu)]
    for null in range(1, 6):
        args = list(ptr)
        args[null] = None
        assert run(*args, None, 0.1, 0.1, 0) == capi.MF_ERR_ARGUMENT, null
    for bad in (-0.5, float("nan"), float("inf")):
        assert run(*ptr, None, bad, 0.1, 0) == capi.MF_ERR_ARGUMENT
        assert run(*ptr, None, 0.1, bad, 0) == capi.MF_ERR_ARGUMENT
    wide = capi.Instance(1, inst.alpha, 4095, inst.users, inst.items, inst.row, inst.col, inst.val)   # F + 2 = 4097
    pw, keepw = capi._problem(wide)
    Lw, Rw = np.zeros((inst.users, 4095)), np.zeros((inst.items, 4095))
    assert run(C.addressof(pw), Lw.ctypes.data, Rw.ctypes.data, *ptr[3:], None, 0.1, 0.1, 0) == capi.MF_ERR_UNSUPPORTED
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2) and not bu.any() and not bi.any()   # a refused call touches nothing


@gpu
def test_frozen_column_out_of_range_is_refused(device):
    """column -2 and column = K on a live plan: MF_ERR_ARGUMENT and nothing changes"""
    capi = device
    pat, L0, R0, val, alpha = _small()
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        assert plan.frozen_columns() == (-1, -1) and "frozen=" not in plan.describe()
        plan.set_frozen_columns(9, 8)          # legal before the upload
        for bad in (-2, 10, 11, -(2 ** 31)):
            for args in ((bad, 0), (0, bad)):
                with pytest.raises(capi.HipBackendError) as err:
                    plan.set_frozen_columns(*args)
                assert err.value.status == capi.MF_ERR_ARGUMENT and plan.frozen_columns() == (9, 8)
        assert " frozen=9/8" in plan.describe()
        plan.set_frozen_columns(-1, 3)
        assert plan.frozen_columns() == (-1, 3) and " frozen=-1/3" in plan.describe()
        got = C.c_int32(77)
        assert capi.hip().mf_plan_get_frozen_columns(plan._h, None, C.byref(got)) == 0 and got.value == 3
        assert capi.hip().mf_plan_get_frozen_columns(plan._h, C.byref(got), None) == 0 and got.value == -1
    finally:
        plan.close()


def test_bias_host_functions_agree_with_numpy(capi):
    rng = np.random.default_rng(5)
    assert capi.bias_mean(np.zeros(0)) == 0.0
    for n in (1, 2, 7, 1000, 4097):
        v = rng.uniform(-5, 5, n) * 10.0 ** rng.integers(-8, 9, n)
        assert_same_bits(np.array([capi.bias_mean(v)]), np.array([seq_mean(v)]), "mean of %d" % n)
    v = np.array([1e16, 1.0, -1e16, 1.0])       # order matters: ((1e16 + 1) - 1e16) + 1 = 1, not 2
    assert capi.bias_mean(v) == seq_mean(v) == 0.25
    for F in (1, 2, 8, 98):
        for side in (0, 1):
            X = rng.standard_normal((13, F))
            X[0, 0] = -0.0
            b = rng.standard_normal(13)
            b[1] = -0.0
            got = capi.bias_pack(X, b, side)
            assert got.shape == (13, F + 2)
            assert_same_bits(got, pack(X, b, side), "pack F=%d side=%d" % (F, side))
            assert (got[:, F + 1 if side == 1 else F] == 1.0).all()
            assert_same_bits(capi.bias_pack(X, None, side), pack(X, np.zeros(13), side), "pack without biases")
            X2, b2 = capi.bias_unpack(got, side)
            assert_same_bits(X2, X, "round trip X")
            assert_same_bits(b2, b, "round trip bias")
            # either output may be NULL
            only_b = np.full(13, 9.0)
            assert capi.hip().mf_backend_bias_unpack(got.ctypes.data, 13, F, side, None, only_b.ctypes.data) == 0
            assert_same_bits(only_b, b, "bias alone")
            only_x = np.empty((13, F))
            assert capi.hip().mf_backend_bias_unpack(got.ctypes.data, 13, F, side, only_x.ctypes.data, None) == 0
            assert_same_bits(only_x, X, "X alone")
    assert capi.bias_pack(np.zeros((0, 3)), None, 1).shape == (0, 5)


@pytest.mark.parametrize("F", [1, 8, 98])
@pytest.mark.parametrize("pat_name", ["pair", "skewed"])
def test_explicit_bias_model_is_the_packed_frozen_model(pat_name, F):
    """Two iterations of the model with biases of their own equal the K = F + 2 frozen-column model bit for bit: the dot
    ((dot_F + bu*1.0) + 1.0*bi) and the update b*d + sum e_n*1.0 multiply by 1.0 exactly."""
    pat = pattern(pat_name)
    K = F + 2
    L0, R0, val, alpha = cls_signed(6000 + F, pat, F)
    rng = np.random.default_rng(F)
    bu, bi = rng.uniform(-1, 1, pat.users), rng.uniform(-1, 1, pat.items)
    mu = seq_mean(val)
    cen = val - mu
    explicit = BiasModel(pat.users, pat.items, pat.row, pat.col, cen, alpha)
    packed = Model(pat.users, pat.items, pat.row, pat.col, cen, alpha)
    L, R, Lp, Rp = L0, R0, pack(L0, bu, 1), pack(R0, bi, 0)
    for it in range(2):
        L, R, bu, bi = explicit.step(L, R, bu, bi, LAM_U, LAM_I)
        Lp, Rp = fstep(packed, Lp, Rp, LAM_U, LAM_I, K - 1, K - 2)
        assert_same_bits(Lp, pack(L, bu, 1), "%s F=%d iteration %d: users" % (pat_name, F, it))
        assert_same_bits(Rp, pack(R, bi, 0), "%s F=%d iteration %d: items" % (pat_name, F, it))
    assert differs(bu, np.zeros_like(bu)) > 0.5 and (Lp[:, K - 1] == 1.0).all() and (Rp[:, K - 2] == 1.0).all()
    # the free model would have moved the constant columns
    free = packed.step(pack(L0, bu, 1), pack(R0, bi, 0), LAM_U, LAM_I)
    assert (free[0][:, K - 1] != 1.0).mean() > 0.5 and (free[1][:, K - 2] != 1.0).mean() > 0.5


@pytest.mark.parametrize("cls", ["signed", "nonfinite"])
def test_guards_of_the_shared_expectation(cls):
    """fexpected asserts its guards when it is built; a model that ignores the index, or one that zeroes instead of
    selecting, is told apart by these inputs."""
    x = fexpected("pair", cls, 10, LAM_U, LAM_I, 9, 8)
    assert not same_bits(x.base.seeded[0][:, 9], x.seeded[0][:, 9]) and not same_bits(x.base.seeded[1][:, 8], x.seeded[1][:, 8])
    assert (x.unseeded[0][:, 9] == 0.0).all() and not np.signbit(x.unseeded[0][:, 9]).any()
    keep = np.ones(10, bool)
    keep[9] = False
    assert_same_bits(x.seeded[0][:, keep], x.base.seeded[0][:, keep], "every other column is the free model's")


BAD_BIAS = ["", "0", "2", "yes", "1 ", "11", "-1", "true"]
FORBIDDEN = [dict(MATFACT_DEVICES="0"), dict(MATFACT_MATS="/dev/null"), dict(MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_RESUME="x.ck"),
             dict(MATFACT_TOPN="3"), dict(MATFACT_SIMILAR="3", MATFACT_SIMILAR_OUT="sim.out")]


@pytest.mark.parametrize("env", [dict(MATFACT_BIAS=v) for v in BAD_BIAS] + [dict(e, MATFACT_BIAS="1") for e in FORBIDDEN],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_bias_refusals_die_with_empty_stdout(capi, env, tmp_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(clean, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_BIAS" in r.stderr, r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def device(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.fixture
def switches(monkeypatch):
    """No sweep switch from the caller's environment; the test sets its own."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_all(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_all


def run_form(capi, switches, case, x, lam, fu, fi, one_iteration=None):
    """One plan in the form of `case`: describe(), a seeded and an unseeded step where the form has steps, two iterate(1)."""
    K, pat = case["K"], x.pat
    switches(case["env"])
    if case.get("nch"):
        switches({"MF_SWEEP_NCH": case["nch"]})
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        assert plan.frozen_columns() == (-1, -1) and "frozen=" not in plan.describe()
        plan.set_regularization(*lam)
        plan.set_frozen_columns(fu, fi)
        desc = plan.describe()
        assert case["check"](desc, K), desc
        assert plan.frozen_columns() == (fu, fi) and " frozen=%d/%d" % (fu, fi) in desc, desc
        where = "%s-K%d-nch%s frozen=%d/%d lambda=%s [%s]" % (case["name"], K, case.get("nch") or "rule", fu, fi, lam, desc.split(" loss=")[0])
        if case["steps"]:
            L, R = _step(plan, x.L0, x.R0, True, True)
            assert_same_bits(R, x.seeded[1], where + ": seeded item sweep")
            assert_same_bits(L, x.seeded[0], where + ": seeded user sweep")
            L, R = _step(plan, x.L0, x.R0, False, False)
            assert_same_bits(R, x.unseeded[1], where + ": item sweep from zero")
            assert_same_bits(L, x.unseeded[0], where + ": user sweep from zero")
        plan.upload(x.L0, x.R0)
        plan.iterate(1)
        if one_iteration:
            one_iteration(*plan.download())
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.two[0], where + ": L after two iterations")
        assert_same_bits(R, x.two[1], where + ": R after two iterations")
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("lam", [(LAM_U, LAM_I), (0.0, 0.0)], ids=["lambda", "lambda0"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_frozen_columns_through_every_form(device, switches, case, lam):
    """The bias convention (users' column K-1, items' column K-2) through every sweep form at the rule's chunk size and at
    5, regularised and -- the decay instances at d = 1.0 -- with lambda = 0."""
    K = case["K"]
    run_form(device, switches, case, fexpected(case["pat"], "signed", K, lam[0], lam[1], K - 1, K - 2), lam, K - 1, K - 2)


POSITIONS = [("dma-ct", 256, 128, 255),   # the first piece of the second pass; the last column
             ("dma-ct", 100, 0, 99),
             ("dma-rt", 130, 129, 64),    # an odd column, the .y of the last piece; lane 0 of the second pass
             ("reg", 129, 128, 128),      # lane 0 of the third register
             ("reg", 65, 64, 64),         # lane 0 of the second register
             ("es-sw2", 6, 5, 4),         # the last slice
             ("es-sw8", 10, 9, 8),        # the last, partly filled slice
             ("coop", 30, 0, 0),
             ("long", 30, 0, 29),         # the extreme rows are items: their last piece's .y, in the partly filled slice
             # the wide rows (the table of every form has the bias layout: 4094 / 4093 are lanes 62 and 61 of register 63)
             ("reg-wide", 4095, 4032, 0),       # lane 0 of register 63; lane 0 of register 0
             ("reg-wide", 4095, 0, 4032),
             ("reg-wide", 513, 512, 511),       # the lone lane of the ninth register; lane 63 of the eighth
             ("dma-rt", 1024, 1023, 512),       # the .y of the last piece of the eighth pass; the first piece of the fifth
             ("dma-rt", 1024, 0, 1023)]


@gpu
@pytest.mark.parametrize("name,K,fu,fi", POSITIONS, ids=lambda v: str(v))
def test_frozen_column_positions(device, switches, name, K, fu, fi):
    case = _pick(name, K)
    run_form(device, switches, case, fexpected(case["pat"], "signed", K, LAM_U, LAM_I, fu, fi), (LAM_U, LAM_I), fu, fi)


@gpu
@pytest.mark.parametrize("cls", ["zeros", "subnormal-users", "nonfinite"])
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("long", 30), ("es-sw4", 10)], ids=lambda v: str(v))
def test_special_values_do_not_reach_the_frozen_column(device, switches, name, K, cls):
    """The frozen column has X_old's bits (signed zeros, subnormals) or 0.0, also in the rows whose every other element is
    NaN (fexpected's guard finds such rows)."""
    case = _pick(name, K)
    run_form(device, switches, case, fexpected(case["pat"], cls, K, LAM_U, LAM_I, K - 1, K - 2), (LAM_U, LAM_I), K - 1, K - 2)


@gpu
@pytest.mark.parametrize("users_frozen", [True, False], ids=["users", "items"])
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("es-sw4", 10)], ids=lambda v: str(v))
def test_one_side_only(device, switches, name, K, users_frozen):
    """After one iteration the unfrozen side has the bits of the free model."""
    case = _pick(name, K)
    fu, fi = (K - 1, -1) if users_frozen else (-1, K - 2)
    x = fexpected(case["pat"], "signed", K, LAM_U, LAM_I, fu, fi)

    def one(L, R):
        assert_same_bits(L, x.seeded[0], "L after one")
        assert_same_bits(R, x.seeded[1], "R after one")
        free = x.base.seeded[0 if not users_frozen else 1]
        assert_same_bits(R if users_frozen else L, free, "the unfrozen side is the free model's")
    run_form(device, switches, case, x, (LAM_U, LAM_I), fu, fi, one_iteration=one)


@gpu
@pytest.mark.parametrize("name,K", ZERO_FORMS, ids=lambda v: str(v))
def test_unfreezing_gives_the_plain_library(device, orc, switches, name, K):
    """set_frozen_columns(-1, -1) after a freeze: the oracle's bits and no frozen= in describe()."""
    capi = device
    case = _pick(name, K)
    pat = pattern(case["pat"])
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    with np.errstate(all="ignore"):
        seeded = orc.tile_step(0, pat.users, 0, pat.items, K, pat.row, pat.col, val, alpha, L0, R0, True, True)
        L2, R2 = L0.copy(), R0.copy()
        orc.factorize(orc.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, val), L2, R2)
    switches(case["env"])
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    try:
        plan.set_frozen_columns(K - 1, K - 2)
        assert " frozen=" in plan.describe()
        plan.set_frozen_columns(-1, -1)
        desc = plan.describe()
        assert case["check"](desc, K) and "frozen=" not in desc, desc
        if case["steps"]:
            L, R = _step(plan, L0, R0, True, True)
            assert_same_bits(L, seeded[0], name + " L")
            assert_same_bits(R, seeded[1], name + " R")
        plan.upload(L0, R0)
        plan.iterate(2)
        L, R = plan.download()
        assert_same_bits(L, L2, name + " L after two")
        assert_same_bits(R, R2, name + " R after two")
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("K", [3, 10, 30, 40])
def test_toy_single_launch_loop(device, switches, K):
    """iterate(9) of a toy instance inside one launch (sweep_resident_kernel: K <= 4, <= 16, <= 32 and the generic form) and
    by two launches per iteration (MF_RESIDENT=0); K = 3 is the smallest biased model, F = 1."""
    capi = device
    pat, L0, R0, val, alpha = _toy(K)
    m = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    for lam in ((LAM_U, LAM_I), (0.0, 0.0)):
        want = fiterate(m, L0, R0, 9, lam[0], lam[1], K - 1, K - 2)
        free = m.iterate(L0, R0, 9, *lam)
        assert not same_bits(want[0][:, K - 1], free[0][:, K - 1]) and same_bits(want[0][:, K - 1], L0[:, K - 1])
        for mode in (None, "0"):
            switches({} if mode is None else {"MF_RESIDENT": mode})
            plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
            try:
                plan.set_regularization(*lam)
                plan.set_frozen_columns(K - 1, K - 2)
                plan.upload(L0, R0)
                plan.iterate(9)
                L, R = plan.download()
                where = "K=%d MF_RESIDENT=%s lambda=%s" % (K, mode, lam)
                assert_same_bits(L, want[0], where + " L")
                assert_same_bits(R, want[1], where + " R")
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("graph", [None, "0"])
def test_graph_replay_and_a_change_of_the_frozen_columns(device, switches, graph):
    """iterate(130) = four replays of a captured 32-iteration graph plus two eager iterations; the graph is captured per
    call, so the columns set between two calls are the ones the second call runs with."""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({"MF_ITER_MODE": "sweeps"})
    if graph:
        switches({"MF_GRAPH": graph})
    m = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    mid = fiterate(m, L0, R0, 130, LAM_U, LAM_I, 9, 8)
    end = fiterate(m, *mid, 130, LAM_U, LAM_I, 2, -1)
    assert same_bits(mid[0][:, 9], L0[:, 9]) and not same_bits(end[0][:, 9], L0[:, 9]) and same_bits(end[0][:, 2], mid[0][:, 2])
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        assert ("MF_GRAPH=0" in plan.describe()) == (graph == "0"), plan.describe()
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_frozen_columns(9, 8)
        plan.upload(L0, R0)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, mid[0], "L after 130")
        assert_same_bits(R, mid[1], "R after 130")
        plan.set_frozen_columns(2, -1)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, end[0], "L after 260, columns switched at 130")
        assert_same_bits(R, end[1], "R after 260, columns switched at 130")
    finally:
        plan.close()


@gpu
def test_two_user_shards_on_one_gpu(device, switches):
    """Shard 0 seeds R and shard 1 does not: its frozen column is 0.0, so the host sum of the two items_next gives the
    frozen column of the single plan back, bit for bit (1.0 and other non-zero numbers); the user blocks are the single
    plan's."""
    capi = device
    K, cut = 30, 333
    base = expected("pair", "signed", K)
    pat, alpha, val = base.pat, base.alpha, base.val
    fu, fi = K - 1, K - 2
    L0, R0 = base.L0.copy(), base.R0.copy()
    L0[:, fu] = 1.0
    R0[::2, fi] = 1.0
    assert (R0[:, fi] != 0.0).all()
    switches({"MF_ITER_MODE": "sweeps"})
    whole = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    want = fstep(whole, L0, R0, LAM_U, LAM_I, fu, fi)
    single = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    single.set_regularization(LAM_U, LAM_I)
    single.set_frozen_columns(fu, fi)
    Ls, Rs = _step(single, L0, R0, True, True)
    single.close()
    assert_same_bits(Ls, want[0], "single plan, L")
    assert_same_bits(Rs, want[1], "single plan, R")
    lo = pat.row < cut
    parts = []
    for sel, begin, count, seeded in ((lo, 0, cut, True), (~lo, cut, pat.users - cut, False)):
        row, col, v = pat.row[sel], pat.col[sel], val[sel]
        plan = capi.Plan(pat.users, pat.items, K, alpha, row, col, v, user_begin=begin, user_count=count)
        try:
            plan.set_regularization(LAM_U, LAM_I)
            plan.set_frozen_columns(fu, fi)
            Lb, Rn = _step(plan, L0[begin:begin + count], R0, seeded, True)
        finally:
            plan.close()
        m = Model(count, pat.items, row - begin, col, v, alpha)
        Lm, Rm = fstep(m, L0[begin:begin + count], R0, LAM_U, LAM_I, fu, fi, True, seeded)
        assert_same_bits(Rn, Rm, "shard at %d: items_next" % begin)
        assert_same_bits(Lb, Lm, "shard at %d: user block against the model" % begin)
        assert_same_bits(Lb, Ls[begin:begin + count], "shard at %d: user block against the single plan" % begin)
        parts.append(Rn)
    assert (parts[1][:, fi] == 0.0).all() and not np.signbit(parts[1][:, fi]).any()
    assert_same_bits((parts[0] + parts[1])[:, fi], Rs[:, fi], "host sum of the frozen column")
    assert_same_bits(Rs[:, fi], R0[:, fi], "the single plan's frozen column")


@gpu
def test_plain_decay_instance_above_262144_rows(device, switches):
    """Both sides just above 262144 rows launch sweep_dma_kernel<10, 1, decay> without the pipelined phases, at d = 1.0
    here: one seeded and one unseeded step with frozen columns, every row of both factors."""
    capi = device
    K, env, make, form = LARGE["both-K10"]
    switches(env)
    pat = make()
    L0, R0, val = signed_inputs(7000 + K, pat, K)
    alpha = 1e-3
    m = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    try:
        plan.set_frozen_columns(K - 1, K - 2)
        desc = plan.describe()
        assert form in desc and _single_wave(desc, K, K) and " frozen=9/8" in desc and "lambda=" not in desc, desc
        for seed in (True, False):
            free = m.step(L0, R0, 0.0, 0.0, seed, seed)
            want = (freeze(free[0], L0, K - 1, seed), freeze(free[1], R0, K - 2, seed))
            assert (free[0][:, K - 1] != want[0][:, K - 1]).mean() > 0.5
            L, R = _step(plan, L0, R0, seed, seed)
            assert_same_bits(R, want[1], "item sweep, seed=%s" % seed)
            assert_same_bits(L, want[0], "user sweep, seed=%s" % seed)
    finally:
        plan.close()


@gpu
def test_downstream_passes_on_a_packed_plan(device, orc, switches):
    """pair, F = 18 (K = 20, a matrix-core K): after two biased iterations recommend, top-N, the loss and the held-out ranks
    are the numpy models of test_topn.py, test_loss.py and test_rank.py applied to the packed factors."""
    capi = device
    F, K = 18, 20
    pat = pattern("pair")
    L0, R0, val, alpha = cls_signed(6000 + F, pat, F)
    rng = np.random.default_rng(18)
    bu, bi = rng.uniform(-1, 1, pat.users), rng.uniform(-1, 1, pat.items)
    cen = val - seq_mean(val)
    Lp0, Rp0 = pack(L0, bu, 1), pack(R0, bi, 0)
    switches({})
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, cen)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_frozen_columns(K - 1, K - 2)
        plan.upload(Lp0, Rp0)
        plan.iterate(2)
        Lp, Rp = plan.download()
        want = fiterate(Model(pat.users, pat.items, pat.row, pat.col, cen, alpha), Lp0, Rp0, 2, LAM_U, LAM_I, K - 1, K - 2)
        assert_same_bits(Lp, want[0], "packed L")
        assert_same_bits(Rp, want[1], "packed R")
        best = plan.recommend()
        assert np.array_equal(best, orc.recommend(orc.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, cen), Lp, Rp))
        mi, ms = model_topn(orc, pat.users, pat.items, pat.row, pat.col, Lp, Rp, 5)
        it, sc = plan.recommend_topn(5)
        assert_same(it, sc, mi, ms, "top-5 on the packed plan")
        assert np.array_equal(it[:, 0], best)
        assert plan.recommend_topn_info()[1] in (1, 2)
        check_loss(plan, Lp, Rp, pat.row, pat.col, cen, "train", "packed plan")
        hrow, hcol, hval = heldout_for(18, pat.users, pat.items, pat.row, pat.col, most=3)
        plan.set_heldout(hrow, hcol, hval)
        assert np.array_equal(plan.rank_heldout(), model_ranks(orc, pat.users, pat.items, pat.row, pat.col, Lp, Rp, hrow, hcol))
    finally:
        plan.close()


RUN_ITERS = 300   # the toy single-launch loop for inst0, graph replays for inst30-40


@functools.lru_cache(maxsize=None)
def biased_reference(name, lam_u, lam_i, iters):
    """The explicit-bias model on a fixture from the reference's initialisation and zero biases: (mu, L, R, bu, bi)."""
    from recommender_system_amd import capi
    inst = capi.parse_file(golden_in(name))
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    mu = seq_mean(inst.val)
    m = BiasModel(inst.users, inst.items, inst.row, inst.col, inst.val - mu, inst.alpha)
    return (mu,) + m.iterate(L0, R0, np.zeros(inst.users), np.zeros(inst.items), iters, lam_u, lam_i)


def model_best(orc, inst, L, R, bu, bi):
    """the arg-max rule of print_output on the packed factors"""
    K = inst.feats + 2
    return orc.recommend(orc.Instance(1, inst.alpha, K, inst.users, inst.items, inst.row, inst.col, inst.val), pack(L, bu, 1), pack(R, bi, 0))


@gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "inst0"])
def test_backend_run_biased(device, orc, name):
    """L, R, bu, bi and mu against the explicit-bias model, best against the arg-max rule; and the documented sequence by
    hand -- a K = F + 2 plan over the centred values, the packed factors, set_regularization, set_frozen_columns(F+1, F) --
    gives the same bits."""
    capi = device
    inst = capi.parse_file(golden_in(name))
    F = inst.feats
    mu, Lm, Rm, bum, bim = biased_reference(name, LAM_U, LAM_I, RUN_ITERS)
    L, R = capi.init_factors(inst.users, inst.items, F)
    L0, R0 = L.copy(), R.copy()
    bu, bi = np.zeros(inst.users), np.zeros(inst.items)
    got_mu, best = capi.backend_run_biased(inst, L, R, bu, bi, LAM_U, LAM_I, iters=RUN_ITERS)
    assert_same_bits(np.array([got_mu]), np.array([mu]), "mu")
    assert_same_bits(L, Lm, "L")
    assert_same_bits(R, Rm, "R")
    assert_same_bits(bu, bum, "user biases")
    assert_same_bits(bi, bim, "item biases")
    assert bu.any() and bi.any() and not same_bits(L, L0)
    assert np.array_equal(best, model_best(orc, inst, Lm, Rm, bum, bim))
    L2, R2, bu2, bi2 = L0.copy(), R0.copy(), np.zeros(inst.users), np.zeros(inst.items)
    assert capi.backend_run_biased(inst, L2, R2, bu2, bi2, LAM_U, LAM_I, iters=RUN_ITERS, recommend=False)[1] is None
    assert_same_bits(L2, L, "L without a recommendation")
    plan = capi.Plan(inst.users, inst.items, F + 2, inst.alpha, inst.row, inst.col, inst.val - mu)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_frozen_columns(F + 1, F)
        plan.upload(capi.bias_pack(L0, None, 1), capi.bias_pack(R0, None, 0))
        plan.iterate(RUN_ITERS)
        Lp, Rp = plan.download()
        assert np.array_equal(plan.recommend(), best)
    finally:
        plan.close()
    assert_same_bits(Lp, pack(L, bu, 1), "by hand: packed L")
    assert_same_bits(Rp, pack(R, bi, 0), "by hand: packed R")


def _cli(capi, path, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(clean, **env))


@functools.lru_cache(maxsize=None)
def packed_trace(name, lam_u, lam_i, points):
    """The packed frozen-column model (the explicit-bias model, by test_explicit_bias_model_is_the_packed_frozen_model) over
    all the iterations of a fixture in one pass: (mu, {iteration: (L', R')} for the listed iterations and the last)."""
    from recommender_system_amd import capi
    inst = capi.parse_file(golden_in(name))
    F = inst.feats
    L0, R0 = capi.init_factors(inst.users, inst.items, F)
    mu = seq_mean(inst.val)
    m = Model(inst.users, inst.items, inst.row, inst.col, inst.val - mu, inst.alpha)
    L, R = pack(L0, np.zeros(inst.users), 1), pack(R0, np.zeros(inst.items), 0)
    out = {}
    for it in range(inst.iters + 1):
        if it in points or it == inst.iters:
            out[it] = (L, R)
        if it < inst.iters:
            L, R = fstep(m, L, R, lam_u, lam_i, F + 1, F, dot=fast_dot)
    return mu, out


@gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "inst0"])
def test_cli_bias(device, orc, name):
    """MATFACT_BIAS=1 alone and with MATFACT_LAMBDA: stdout is the .out of the model's best; with MATFACT_LOSS=1 there is a
    stderr line per iteration whose RMSE parses back to the bits of the model's loss (the first three, the middle and the
    last are compared), and one more line carries mu."""
    capi = device
    path = golden_in(name)
    inst = capi.parse_file(path)
    K = inst.feats + 2
    oi = orc.Instance(1, inst.alpha, K, inst.users, inst.items, inst.row, inst.col, inst.val)
    points = (0, 1, 2, inst.iters // 2, inst.iters)
    for lam, env in (((0.0, 0.0), {}), ((LAM_U, LAM_I), dict(MATFACT_LAMBDA="0.05,0.3"))):
        mu, trace = packed_trace(name, lam[0], lam[1], points)
        want = orc.format_out(orc.recommend(oi, *trace[inst.iters])).encode()
        r = _cli(capi, path, MATFACT_BIAS="1", **env)
        assert r.returncode == 0 and r.stdout == want, (lam, r.returncode, r.stdout[:80], r.stderr[:200])
    r = _cli(capi, path, MATFACT_BIAS="1", MATFACT_LAMBDA="0.05,0.3", MATFACT_LOSS="1")
    assert r.returncode == 0 and r.stdout == want, (r.returncode, r.stdout[:80], r.stderr[:200])
    lines = r.stderr.decode().splitlines()
    its = [ln.split() for ln in lines if ln.startswith("iter ")]
    assert [int(t[1]) for t in its] == list(range(inst.iters + 1)) and all(t[2] == "train_rmse" for t in its)
    assert lines[inst.iters + 1].startswith("bias mu ") and sum(ln.startswith("bias mu ") for ln in lines) == 1, lines[-3:]
    assert_same_bits(np.array([float(lines[inst.iters + 1].split()[2])]), np.array([mu]), "mu on stderr")
    assert lines[inst.iters + 2].startswith("penalty lambda ")
    cen = inst.val - mu
    for it in points:
        sse = model_total(model_rows(*trace[it], inst.row, inst.col, cen, inst.users))
        assert_same_bits(np.array([float(its[it][3])]), np.array([np.sqrt(sse / float(inst.nnz))]), "train_rmse at iteration %d" % it)
