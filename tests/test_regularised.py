"""L2-regularised sweeps (mf_plan_set_regularization, mf_plan_penalty, mf_backend_run_reg, MATFACT_LAMBDA).

The definition is the library's own (include/matfact_hip.h): on the host c2 = alpha * 2 and d = 1.0 - c2 * lambda (two
roundings); a seeded row starts from X_old[r] * d -- one rounded multiply, unfused with the add that follows --, an unseeded
one from 0.0; e_n = c2 * (val_n - dot_n) sees the unshrunk factors.  The model below is numpy on the CPU and follows that
text; every GPU comparison is bit for bit (assert_same_bits of test_sweep_edges.py: NaN as a class, everything else by its
bits).  lambda_users = 0.05 and lambda_items = 0.3 at alpha = 1e-3 give two inexact, different d: a swapped side, a fused
multiply-add or x - t * x all show.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in
from test_iterate_path import path_of_plan
from test_loss import model_total
from test_sweep_edges import (CLASSES, FORMS, GRID_CAP, PF_ROWS, SINGLE, SWEEPS, SWITCHES, Pattern, _single_wave, assert_same_bits,
                              cls_signed, pattern, pattern_both_large, pattern_one_large, seq_dot, signed_inputs)

gpu = pytest.mark.gpu

LAM_U, LAM_I = 0.05, 0.3


# ------------------------------------------------------------------------------------------------ the model
def decay(alpha, lam):
    """d = 1.0 - (alpha * 2) * lambda: the product is rounded, then the subtraction"""
    c2 = alpha * 2
    t = c2 * lam
    return 1.0 - t


class Side:
    """The entries of one side's rows, padded to the longest row: pad[r, j] = the j-th entry of row r in the side's order
    (CSR order for users; stable by item for items), 0 past the row's end (never used: the sums are read at lens[r])."""

    def __init__(self, own, nrows):
        order = np.argsort(own, kind="stable")
        self.lens = np.bincount(own, minlength=nrows)
        first = np.concatenate([[0], np.cumsum(self.lens)[:-1]])
        self.maxlen = int(self.lens.max()) if len(own) else 0
        j = np.arange(self.maxlen)
        inside = j[None, :] < self.lens[:, None]
        pos = np.where(inside, first[:, None] + j[None, :], 0)
        self.pad = order[pos] if len(own) else np.zeros((nrows, 0), np.int64)
        self.rows = np.arange(nrows)


def fast_dot(L, R, row, col):
    """seq_dot by one cumulative sum per entry: ((0.0 + x0*y0) + x1*y1) + ... (np.cumsum is sequential)"""
    prod = L[row] * R[col]
    return np.cumsum(np.concatenate([np.zeros((len(row), 1)), prod], axis=1), axis=1)[:, -1]


def model_sweep(X_old, Y_old, e, side, other, d, seeded):
    """acc = X_old[r] * d (0.0 unseeded); for the row's entries in order: acc = acc + e_n * Y_old[other_n]"""
    start = X_old * d if seeded else np.zeros_like(X_old)
    if side.maxlen == 0:
        return start
    if side.pad.size * X_old.shape[1] > 20_000_000:
        # many rows, most of them short, or rows of a few thousand columns: entry j of every row that has one, j ascending
        # (the same sums, no padded array)
        acc = start
        for j in range(side.maxlen):
            has = np.flatnonzero(side.lens > j)
            n = side.pad[has, j]
            acc[has] = acc[has] + e[n][:, None] * Y_old[other[n]]
        return acc
    terms = e[side.pad][:, :, None] * Y_old[other[side.pad]]
    run = np.cumsum(np.concatenate([start[:, None, :], terms], axis=1), axis=1)
    return np.ascontiguousarray(run[side.rows, side.lens])


class Model:
    def __init__(self, users, items, row, col, val, alpha):
        self.row, self.col = np.asarray(row, np.int64), np.asarray(col, np.int64)
        self.val, self.alpha = np.asarray(val, np.float64), float(alpha)
        self.us, self.its = Side(self.row, users), Side(self.col, items)

    def step(self, L, R, lam_u, lam_i, seed_u=True, seed_i=True, dot=seq_dot):
        """(L_new, R_new) of one iteration from the frozen L, R"""
        with np.errstate(all="ignore"):
            c2 = self.alpha * 2
            e = c2 * (self.val - dot(L, R, self.row, self.col))
            Ln = model_sweep(L, R, e, self.us, self.col, decay(self.alpha, lam_u), seed_u)
            Rn = model_sweep(R, L, e, self.its, self.row, decay(self.alpha, lam_i), seed_i)
        return Ln, Rn

    def iterate(self, L, R, iters, lam_u, lam_i):
        for _ in range(iters):
            L, R = self.step(L, R, lam_u, lam_i, dot=fast_dot)
        return L, R


def row_squares(X):
    """s_r = ((0.0 + x0*x0) + x1*x1) + ..., k ascending"""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.cumsum(np.concatenate([np.zeros((X.shape[0], 1)), X * X], axis=1), axis=1)[:, -1])


def differs(a, b):
    return float((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).mean())


@functools.lru_cache(maxsize=None)
def expected(pat_name, cls, K, lam_u=LAM_U, lam_i=LAM_I):
    """Inputs of one (pattern, class, K) and the model's results on them, computed once and shared."""
    pat = pattern(pat_name)
    x = type("Expected", (), {})()
    x.pat, x.K = pat, K
    x.L0, x.R0, x.val, x.alpha = CLASSES[cls](4000 + K, pat, K)
    x.model = Model(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha)
    x.seeded = x.model.step(x.L0, x.R0, lam_u, lam_i)
    x.unseeded = x.model.step(x.L0, x.R0, lam_u, lam_i, False, False)
    x.plain = x.model.step(x.L0, x.R0, 0.0, 0.0)
    x.two = x.model.step(*x.seeded, lam_u, lam_i)
    if cls == "signed" and lam_u > 0.0 and lam_i > 0.0:
        # the guard: the decay shows in more than half of the elements of each factor, and the two d are inexact and different
        assert differs(x.seeded[0], x.plain[0]) > 0.5 and differs(x.seeded[1], x.plain[1]) > 0.5, (pat_name, K)
        du, di = decay(x.alpha, lam_u), decay(x.alpha, lam_i)
        assert du != di and du != 1.0 and di != 1.0 and 1.0 - du != x.alpha * 2 * lam_u
    return x


# ------------------------------------------------------------------------------------------------ CPU
REG_SYMBOLS = ("mf_plan_set_regularization", "mf_plan_get_regularization", "mf_plan_penalty", "mf_backend_run_reg")


@pytest.mark.parametrize("K", [3, 6, 100])
@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed"])
def test_model_at_d_one_is_the_oracle(orc, pat_name, K):
    """This tests the model: at lambda = 0 it is the oracle's shard_step, seeded and (r_is_root=False) unseeded; the fast
    dot of the many-iteration model is seq_dot; and x * 1.0 is x."""
    pat = pattern(pat_name)
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    assert decay(alpha, 0.0) == 1.0
    m = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    assert_same_bits(fast_dot(L0, R0, m.row, m.col), seq_dot(L0, R0, pat.row, pat.col), "fast_dot")
    for root in (True, False):
        Lo, Ro = orc.shard_step(0, pat.users, pat.items, K, pat.row, pat.col, val, alpha, L0, R0, root)
        Lm, Rm = m.step(L0, R0, 0.0, 0.0, True, root)
        assert_same_bits(Lm, Lo, "%s K=%d root=%s L" % (pat_name, K, root))
        assert_same_bits(Rm, Ro, "%s K=%d root=%s R" % (pat_name, K, root))
    Lf, Rf = m.step(L0, R0, 0.0, 0.0, dot=fast_dot)
    assert_same_bits(Lf, m.step(L0, R0, 0.0, 0.0)[0], "fast dot, L")
    Lr, Rr = m.step(L0, R0, LAM_U, LAM_I)
    assert differs(Lr, Lf) > 0.5 and differs(Rr, Rf) > 0.5


def test_regularisation_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in REG_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr)
    assert capi.hip().mf_backend_abi_version() == 5
    for name in ("set_regularization", "regularization", "penalty"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_reg)


def test_regularisation_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    a, b = C.c_double(), C.c_double()
    assert h.mf_plan_set_regularization(None, 0.0, 0.0) == capi.MF_ERR_ARGUMENT
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert h.mf_plan_set_regularization(fake, bad, 0.1) == capi.MF_ERR_ARGUMENT, bad
        assert h.mf_plan_set_regularization(fake, 0.1, bad) == capi.MF_ERR_ARGUMENT, bad
    assert h.mf_plan_get_regularization(None, C.byref(a), C.byref(b)) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_penalty(None, C.byref(a), C.byref(b), None, None) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    assert h.mf_backend_run_reg(None, L, R, None, 0.1, 0.1, 0) == capi.MF_ERR_ARGUMENT
    for bad in (-0.5, float("nan"), float("inf")):
        assert h.mf_backend_run_reg(C.byref(p), L, R, None, bad, 0.1, 0) == capi.MF_ERR_ARGUMENT
        assert h.mf_backend_run_reg(C.byref(p), L, R, None, 0.1, bad, 0) == capi.MF_ERR_ARGUMENT
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


@pytest.mark.parametrize("users", [1, 1023, 1025, 3000])
def test_host_total_of_row_squares_equals_the_blocked_model(capi, users):
    """mf_backend_loss_total is the host twin of the penalty's total: blocks cut at global multiples of 1024, user_begin
    inside a block."""
    rng = np.random.default_rng(users)
    X = rng.standard_normal((users, 7)) * 10.0 ** rng.integers(-6, 7, (users, 1))
    s = row_squares(X)
    acc = 0.0
    for v in X[0]:
        acc = acc + v * v
    assert_same_bits(np.array([s[0]]), np.array([acc]), "row sum of squares is sequential")
    for begin in (700, 0):
        assert_same_bits(np.array([capi.loss_total(s, begin)]), np.array([model_total(s, begin)]), "begin %d" % begin)


BAD_LAMBDA = ["", "abc", "-1", "-0.5,0.1", "0.1,-2", "nan", "inf", "1e999", "0.1,", "0.1,x", "0.1x", "0.1,0.2,0.3", ",0.1"]
FORBIDDEN = [dict(MATFACT_DEVICES="0"), dict(MATFACT_MATS="/dev/null"), dict(MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_RESUME="x.ck"),
             dict(MATFACT_TOPN="3"), dict(MATFACT_SIMILAR="3", MATFACT_SIMILAR_OUT="sim.out")]


@pytest.mark.parametrize("env", [dict(MATFACT_LAMBDA=v) for v in BAD_LAMBDA] + [dict(e, MATFACT_LAMBDA="0.1") for e in FORBIDDEN],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_lambda_refusals_die_with_empty_stdout(capi, env, tmp_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(clean, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_LAMBDA" in r.stderr, r
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


def _ends(forms):
    """the smallest and the largest K of every row of the table (its rows of wide K apart: WIDE below picks among those)"""
    forms = [f for f in forms if not f.get("wide")]
    ks = {}
    for f in forms:
        ks.setdefault(f["name"], []).append(f["K"])
    return [f for f in forms if f["K"] in (min(ks[f["name"]]), max(ks[f["name"]]))]


def _pick(name, K):
    return next(f for f in FORMS if f["name"] == name and f["K"] == K)


# The extensions at wide K, on the "wide" pattern: the register-staged form with lane 0 of its ninth register alone (513)
# and with all 64 registers at the edge of a CU's LDS (4095), and the eight full passes of the run-time-K LDS-DMA form.
WIDE = [("reg-wide", 513), ("reg-wide", 4095), ("dma-rt", 1024)]
CASES = [dict(f, nch=nch) for f in _ends(FORMS) + [_pick(*w) for w in WIDE] for nch in (None, "5")]


def _case_id(c):
    return "%s-K%d-nch%s" % (c["name"], c["K"], c["nch"] or "rule")


def test_every_form_is_in_the_table():
    names = {c["name"] for c in CASES}
    assert names == {"reg", "reg-wide", "dma-ct", "dma-rt", "db", "pair", "long", "long-nodpp", "coop", "es-sw8", "es-sw4", "es-sw2"}
    assert len(CASES) == 2 * 2 * (len(names) - 1) + 2 * len(WIDE)
    assert {(c["name"], c["K"]) for c in CASES if c["pat"] == "wide"} == set(WIDE)


def _step(plan, L0, R0, seed_items, seed_users):
    plan.upload(L0, R0)
    plan.sweep_items(seed_from_old=seed_items)
    plan.sweep_users(seed_from_old=seed_users)
    plan.flip()
    return plan.download()


@gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_regularised_sweeps_through_every_form(device, switches, case):
    """sweep_items(1) / sweep_users() carry the decay of their side, sweep_items(0) / sweep_users_seeded(0) are the plain
    unseeded bits, two iterate(1) are two model iterations -- in every sweep form, at the rule's chunk size and at 5."""
    capi = device
    K = case["K"]
    x = expected(case["pat"], "signed", K)
    pat = x.pat
    switches(case["env"])
    if case["nch"]:
        switches({"MF_SWEEP_NCH": case["nch"]})
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        assert plan.regularization() == (0.0, 0.0) and "lambda=" not in plan.describe()
        plan.set_regularization(LAM_U, LAM_I)
        desc = plan.describe()
        assert case["check"](desc, K), desc
        assert ("MF_SWEEP_NCH=5" in desc) == (case["nch"] == "5"), desc
        assert plan.regularization() == (LAM_U, LAM_I) and " lambda=0.05/0.3" in desc, desc
        where = "%s [%s]" % (_case_id(case), desc.split(" loss=")[0])
        if case["steps"]:
            L, R = _step(plan, x.L0, x.R0, True, True)
            assert_same_bits(R, x.seeded[1], where + ": seeded item sweep")
            assert_same_bits(L, x.seeded[0], where + ": seeded user sweep")
            L, R = _step(plan, x.L0, x.R0, False, False)
            assert_same_bits(R, x.unseeded[1], where + ": item sweep from zero")
            assert_same_bits(L, x.unseeded[0], where + ": user sweep from zero")
            plain = expected(case["pat"], "signed", K, 0.0, 0.0)
            assert_same_bits(x.unseeded[0], plain.unseeded[0], "an unseeded sweep takes no decay")
            assert_same_bits(x.unseeded[1], plain.unseeded[1], "an unseeded sweep takes no decay")
        plan.upload(x.L0, x.R0)
        plan.iterate(1)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.two[0], where + ": L after two iterations")
        assert_same_bits(R, x.two[1], where + ": R after two iterations")
    finally:
        plan.close()


LARGE = {
    # both sides just above 262144 rows: both sweeps leave the pipelined form for the plain one
    "both-K10": (10, SWEEPS, lambda: pattern_both_large(), " accumulate=plain/plain "),
    "both-K100": (100, SWEEPS, lambda: pattern_both_large(), " accumulate=plain/plain "),
    # 2^20 + 130 users: the launch is capped at 2^20 workgroups, 130 of them walk a second row
    "users-2^20-K10": (10, SINGLE, lambda: pattern_one_large(True), " accumulate=pf/plain "),
}


@gpu
@pytest.mark.parametrize("name", list(LARGE))
def test_plain_decay_instances_above_262144_rows(device, switches, name):
    """sweep_dma_kernel<K, 1, decay> without the pipelined phases is what a regularised sweep of more than 262144 rows
    launches (cfg4's user sweep); no smaller launch reaches it.  One seeded and one unseeded step against the model, every
    row of both factors."""
    capi = device
    K, env, make, form = LARGE[name]
    switches(env)
    pat = make()
    assert max(pat.users, pat.items) > PF_ROWS and (name != "users-2^20-K10" or pat.users > GRID_CAP)
    L0, R0, val = signed_inputs(7000 + K, pat, K)
    alpha = 1e-3
    m = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        desc = plan.describe()
        assert form in desc and _single_wave(desc, K, K) and " lambda=0.05/0.3" in desc, desc
        plain = m.step(L0, R0, 0.0, 0.0)
        for seed in (True, False):
            want = m.step(L0, R0, LAM_U, LAM_I, seed, seed)
            if seed:
                assert differs(want[0], plain[0]) > 0.5 and differs(want[1], plain[1]) > 0.5
            L, R = _step(plan, L0, R0, seed, seed)
            assert_same_bits(R, want[1], "%s: item sweep, seed=%s" % (name, seed))
            assert_same_bits(L, want[0], "%s: user sweep, seed=%s" % (name, seed))
    finally:
        plan.close()


ZERO_FORMS = [("reg", 3), ("dma-ct", 100), ("dma-rt", 6), ("db", 64), ("pair", 100), ("long", 30), ("long-nodpp", 30), ("coop", 10),
              ("es-sw4", 10)] + WIDE


@gpu
@pytest.mark.parametrize("name,K", ZERO_FORMS, ids=lambda v: str(v))
def test_lambda_zero_is_the_plain_library(device, orc, switches, name, K):
    """set_regularization(0, 0), and a plan never told anything, give the oracle's bits."""
    capi = device
    case = _pick(name, K)
    pat = pattern(case["pat"])
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    with np.errstate(all="ignore"):
        seeded = orc.tile_step(0, pat.users, 0, pat.items, K, pat.row, pat.col, val, alpha, L0, R0, True, True)
        L2, R2 = L0.copy(), R0.copy()
        orc.factorize(orc.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, val), L2, R2)
    switches(case["env"])
    for told in (False, True):
        plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
        try:
            if told:
                plan.set_regularization(LAM_U, LAM_I)
                plan.set_regularization(0.0, 0.0)
            desc = plan.describe()
            assert case["check"](desc, K) and "lambda=" not in desc, desc
            if case["steps"]:
                L, R = _step(plan, L0, R0, True, True)
                assert_same_bits(L, seeded[0], "%s told=%s L" % (name, told))
                assert_same_bits(R, seeded[1], "%s told=%s R" % (name, told))
            plan.upload(L0, R0)
            plan.iterate(2)
            L, R = plan.download()
            assert_same_bits(L, L2, "%s told=%s L after two" % (name, told))
            assert_same_bits(R, R2, "%s told=%s R after two" % (name, told))
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("cls", ["zeros", "subnormal-users", "nonfinite"])
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("long", 30), ("es-sw4", 10)], ids=lambda v: str(v))
def test_special_values_survive_the_multiply(device, switches, name, K, cls):
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], cls, K)
    pat = x.pat
    assert decay(x.alpha, LAM_U) != 1.0 and decay(x.alpha, LAM_I) != decay(x.alpha, LAM_U)
    switches(case["env"])
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        assert case["check"](plan.describe(), K), plan.describe()
        where = "%s K=%d %s" % (name, K, cls)
        if case["steps"]:
            for seed, want in ((True, x.seeded), (False, x.unseeded)):
                L, R = _step(plan, x.L0, x.R0, seed, seed)
                assert_same_bits(R, want[1], "%s: item sweep, seed=%s" % (where, seed))
                assert_same_bits(L, want[0], "%s: user sweep, seed=%s" % (where, seed))
        plan.upload(x.L0, x.R0)
        plan.iterate(2)
        L, R = plan.download()
        assert_same_bits(L, x.two[0], where + ": L after two iterations")
        assert_same_bits(R, x.two[1], where + ": R after two iterations")
    finally:
        plan.close()


def _toy(K):
    """6 users x 5 items, 12 entries: the whole instance fits one workgroup's LDS"""
    rng = np.random.default_rng(40 + K)
    cells = np.sort(rng.choice(30, 12, replace=False))
    row, col = (cells // 5).astype(np.int32), (cells % 5).astype(np.int32)
    pat = Pattern("toy", 6, 5, row, col)
    L0, R0, val, alpha = cls_signed(50 + K, pat, K)
    return pat, L0, R0, val, alpha


@gpu
@pytest.mark.parametrize("K", [3, 10, 30, 40])
def test_toy_single_launch_loop(device, orc, switches, K):
    """iterate(9) of a toy instance runs inside one launch (sweep_resident_kernel: K <= 4, <= 16, <= 32 and the generic
    form): the model's bits, the bits of the two-launch path (MF_RESIDENT=0, and a timed plan, which never takes the toy
    path and counts nine launches per side), and at lambda = 0 the oracle's."""
    capi = device
    pat, L0, R0, val, alpha = _toy(K)
    m = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    want = m.iterate(L0, R0, 9, LAM_U, LAM_I)
    assert differs(want[0], m.iterate(L0, R0, 9, 0.0, 0.0)[0]) > 0.5
    Lo, Ro = L0.copy(), R0.copy()
    orc.factorize(orc.Instance(9, alpha, K, pat.users, pat.items, pat.row, pat.col, val), Lo, Ro)
    for mode, timed in ((None, False), ("0", False), (None, True)):
        env = {} if mode is None else {"MF_RESIDENT": mode}
        switches(env)
        for lam, (wl, wr) in (((LAM_U, LAM_I), want), ((0.0, 0.0), (Lo, Ro))):
            plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
            try:
                plan.set_regularization(*lam)
                plan.timing(timed)
                loop = path_of_plan(plan.describe(), pat, K, 9, env, timing=timed)[0]
                assert loop == ("toy" if mode is None and not timed else "sweeps"), (loop, mode, timed)
                plan.upload(L0, R0)
                plan.iterate(9)
                L, R = plan.download()
                where = "K=%d MF_RESIDENT=%s timed=%s lambda=%s" % (K, mode, timed, lam)
                assert_same_bits(L, wl, where + " L")
                assert_same_bits(R, wr, where + " R")
                if timed:
                    t = plan.timing_read()
                    assert t["item_launches"] == 9 and t["user_launches"] == 9, t
            finally:
                plan.close()


@functools.lru_cache(maxsize=None)
def _small(users=60, items=30, nnz=400, K=10, seed=7):
    rng = np.random.default_rng(seed)
    cells = np.sort(rng.choice(users * items, nnz, replace=False))
    pat = Pattern("small", users, items, cells // items, cells % items)
    L0, R0, val, alpha = cls_signed(seed + 1, pat, K)
    return pat, L0, R0, val, alpha


@gpu
@pytest.mark.parametrize("graph", [None, "0"])
def test_graph_replay_and_a_change_of_lambda(device, switches, graph):
    """iterate(130) = four replays of a captured 32-iteration graph plus two eager iterations; the graph is captured per
    call, so the lambda set between two calls is the one the second call runs with."""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({"MF_ITER_MODE": "sweeps"})
    if graph:
        switches({"MF_GRAPH": graph})
    m = Model(pat.users, pat.items, pat.row, pat.col, val, alpha)
    mid = m.iterate(L0, R0, 130, LAM_U, LAM_I)
    end = m.iterate(*mid, 130, 0.2, 0.0)
    assert differs(end[0], m.iterate(*mid, 130, LAM_U, LAM_I)[0]) > 0.5
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        assert ("MF_GRAPH=0" in plan.describe()) == (graph == "0"), plan.describe()
        plan.set_regularization(LAM_U, LAM_I)
        plan.upload(L0, R0)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, mid[0], "L after 130")
        assert_same_bits(R, mid[1], "R after 130")
        for bad in (float("nan"), -1.0, float("inf")):   # a refused value changes nothing on a live plan
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_regularization(bad, 0.1)
            assert err.value.status == capi.MF_ERR_ARGUMENT and plan.regularization() == (LAM_U, LAM_I)
            with pytest.raises(capi.HipBackendError):
                plan.set_regularization(0.1, bad)
            assert plan.regularization() == (LAM_U, LAM_I) and " lambda=0.05/0.3" in plan.describe()
        plan.set_regularization(0.2, 0.0)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, end[0], "L after 260, lambda switched at 130")
        assert_same_bits(R, end[1], "R after 260, lambda switched at 130")
    finally:
        plan.close()


@gpu
def test_two_user_shards_on_one_gpu(device, switches):
    """The item sweep is seeded on shard 0 only: that shard's items_next carries the whole decay, the other's none; the
    user blocks are the single plan's."""
    capi = device
    K, cut = 30, 333
    x = expected("pair", "signed", K)
    pat = x.pat
    assert cut % 1024 and 0 < cut < pat.users
    switches({"MF_ITER_MODE": "sweeps"})
    single = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    single.set_regularization(LAM_U, LAM_I)
    Ls, _ = _step(single, x.L0, x.R0, True, True)
    single.close()
    assert_same_bits(Ls, x.seeded[0], "single plan, L")
    lo = pat.row < cut
    for sel, begin, count, seeded in ((lo, 0, cut, True), (~lo, cut, pat.users - cut, False)):
        row, col, val = pat.row[sel], pat.col[sel], x.val[sel]
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, row, col, val, user_begin=begin, user_count=count)
        try:
            plan.set_regularization(LAM_U, LAM_I)
            Lb, Rn = _step(plan, x.L0[begin:begin + count], x.R0, seeded, True)
        finally:
            plan.close()
        m = Model(count, pat.items, row - begin, col, val, x.alpha)
        Lm, Rm = m.step(x.L0[begin:begin + count], x.R0, LAM_U, LAM_I, True, seeded)
        assert_same_bits(Rn, Rm, "shard at %d: items_next" % begin)
        assert_same_bits(Lb, Lm, "shard at %d: user block against the model" % begin)
        assert_same_bits(Lb, Ls[begin:begin + count], "shard at %d: user block against the single plan" % begin)


@gpu
@pytest.mark.parametrize("users", [1, 1025, 3000])
@pytest.mark.parametrize("K", [3, 20, 100, 256])
def test_penalty(device, K, users):
    capi = device
    begin, items = 700, 1500
    rng = np.random.default_rng(K + users)
    n = min(users * items, 4000)
    cells = np.sort(rng.choice(users * items, n, replace=False))
    row, col = (cells // items + begin).astype(np.int32), (cells % items).astype(np.int32)
    val = rng.integers(-10, 11, n) / 2.0
    L = rng.uniform(-1, 1, (users, K)) * 10.0 ** rng.integers(-4, 5, (users, 1))
    R = rng.uniform(-1, 1, (items, K)) * 10.0 ** rng.integers(-4, 5, (items, 1))
    plan = capi.Plan(begin + users + 5, items, K, 1e-3, row, col, val, user_begin=begin, user_count=users)
    try:
        empty = C.c_double()
        assert capi.hip().mf_plan_penalty(plan._h, C.byref(empty), None, None, None) == capi.MF_ERR_STATE   # no factors yet

        def check(Lx, Rx, where):
            usq, isq, ur, ir = plan.penalty(rows=True)
            assert_same_bits(ur, row_squares(Lx), where + ": user rows")
            assert_same_bits(ir, row_squares(Rx), where + ": item rows")
            assert_same_bits(np.array([usq, isq]), np.array([model_total(ur, begin), model_total(ir, 0)]), where + ": totals")
            assert_same_bits(np.array([usq, isq]), np.array([capi.loss_total(ur, begin), capi.loss_total(ir, 0)]), where + ": host twin")
            assert plan.penalty() == (usq, isq) or np.isnan(usq) or np.isnan(isq)
            return usq, isq
        plan.upload(L, R)
        check(L, R, "uploaded")
        plan.set_regularization(LAM_U, LAM_I)
        plan.iterate(1)
        L1, R1 = plan.download()
        assert differs(L1, L) > 0.5
        check(L1, R1, "after an iterate")
        Ln, Rn = L.copy(), R.copy()
        Ln[users // 2, K // 2] = np.nan
        Rn[1030, 0] = np.inf
        plan.upload(Ln, Rn)
        usq, isq = check(Ln, Rn, "NaN and inf")
        assert np.isnan(usq) and np.isinf(isq)
    finally:
        plan.close()


@gpu
def test_monitored_loop_runs_regularised(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})

    def fresh():
        p = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
        p.set_regularization(LAM_U, LAM_I)
        p.upload(L0, R0)
        return p
    plan, other = fresh(), fresh()
    try:
        done, pts = plan.iterate_monitored(10, every=3, tol=0.0)
        assert done == 10 and [p.iter for p in pts] == [0, 3, 6, 9, 10]
        at = 0
        for p in pts:
            other.iterate(p.iter - at)
            at = p.iter
            assert_same_bits(np.array([p.train.sse]), np.array([other.loss("train").sse]), "point %d" % p.iter)
        Lm, Rm = plan.download()
        Lo, Ro = other.download()
        assert_same_bits(Lm, Lo, "L of the monitored loop")
        assert_same_bits(Rm, Ro, "R of the monitored loop")
        want = Model(pat.users, pat.items, pat.row, pat.col, val, alpha).iterate(L0, R0, 10, LAM_U, LAM_I)
        assert_same_bits(Lm, want[0], "L against the model")
        assert_same_bits(Rm, want[1], "R against the model")
    finally:
        plan.close()
        other.close()


def _cli(capi, path, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(clean, **env))


@gpu
@pytest.mark.parametrize("name", ["inst0", "inst30-40-10-2-10"])
def test_cli_lambda(device, orc, name):
    capi = device
    path = golden_in(name)
    inst = capi.parse_file(path)
    r = _cli(capi, path, MATFACT_LAMBDA="0")
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLDEN, name + ".out"), "rb").read(), r
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    m = Model(inst.users, inst.items, inst.row, inst.col, inst.val, inst.alpha)
    Lm, Rm = m.iterate(L0, R0, inst.iters, LAM_U, LAM_I)
    oi = orc.parse_in(path)
    want = orc.format_out(orc.recommend(oi, Lm, Rm)).encode()
    r = _cli(capi, path, MATFACT_LAMBDA="0.05,0.3")
    assert r.returncode == 0 and r.stdout == want, r
    both = m.iterate(L0, R0, inst.iters, 0.05, 0.05)
    r = _cli(capi, path, MATFACT_LAMBDA="0.05")
    assert r.returncode == 0 and r.stdout == orc.format_out(orc.recommend(oi, *both)).encode(), r
    # with MATFACT_LOSS the loop is the monitored one, and one more stderr line carries penalty()'s values
    r = _cli(capi, path, MATFACT_LAMBDA="0.05,0.3", MATFACT_LOSS="10")
    assert r.returncode == 0 and r.stdout == want, r
    lines = r.stderr.decode().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("penalty ")]
    assert len(at) == 1 and at[0] == max(i for i, ln in enumerate(lines) if ln.startswith("iter ")) + 1, lines
    pen = [lines[at[0]].split()]
    assert len(pen[0]) == 10, pen
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_regularization(0.05, 0.3)
        plan.upload(L0, R0)
        plan.iterate_monitored(inst.iters, every=10)
        usq, isq = plan.penalty()
        sse = plan.loss("train").sse
    finally:
        plan.close()
    got = dict(zip(pen[0][4::2], pen[0][5::2]))
    assert pen[0][1] == "lambda" and (float(pen[0][2]), float(pen[0][3])) == (0.05, 0.3), pen
    assert_same_bits(np.array([float(got["users_sq"]), float(got["items_sq"])]), np.array([usq, isq]), "stderr penalty line")
    assert_same_bits(np.array([float(got["objective"])]), np.array([(sse + 0.05 * usq) + 0.3 * isq]), "stderr objective")
    assert_same_bits(np.array([usq, isq]), np.array([model_total(row_squares(Lm)), model_total(row_squares(Rm))]), "penalty of the model's factors")


@gpu
def test_backend_run_reg(device):
    capi = device
    pat, L0, R0, val, alpha = _small()
    inst = capi.Instance(40, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.upload(L0, R0)
        plan.set_regularization(LAM_U, LAM_I)
        plan.iterate(40)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    L, R = L0.copy(), R0.copy()
    best = capi.backend_run_reg(inst, L, R, LAM_U, LAM_I)
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    want = Model(pat.users, pat.items, pat.row, pat.col, val, alpha).iterate(L0, R0, 40, LAM_U, LAM_I)
    assert_same_bits(L, want[0], "L against the model")
    assert_same_bits(R, want[1], "R against the model")
    L2, R2 = L0.copy(), R0.copy()
    assert capi.backend_run_reg(inst, L2, R2, LAM_U, LAM_I, recommend=False) is None
    assert_same_bits(L2, Lp, "L without a recommendation")
    La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
    b0 = capi.backend_run_reg(inst, La, Ra, 0.0)
    b1 = capi.backend_run(inst, Lb, Rb)
    assert_same_bits(La, Lb, "lambda 0: L of mf_backend_run")
    assert_same_bits(Ra, Rb, "lambda 0: R of mf_backend_run")
    assert np.array_equal(b0, b1)
