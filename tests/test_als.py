"""Alternating least squares (mf_plan_set_als, mf_plan_als_solve, mf_plan_als_info, mf_backend_run_als, MATFACT_SOLVER).

The definition is include/matfact_hip.h's, operation by operation; the model below performs its steps 1-10 with elementwise
numpy operations -- products formed as arrays of their own, serial sums through ufunc.accumulate, which applies its
operation element after element -- so that nothing fuses and nothing is re-ordered.  Every GPU result is compared with it bit
for bit (assert_same_bits: NaN as a class, everything else as uint64), the three row counters included.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import time
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in, random_instance
from test_stream_order import gate  # noqa: F401  (the calibrated gate of the stream-order tests, once for this module)
from test_regularised import LAM_I, LAM_U, ZERO_FORMS, _pick, _small, differs
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits, cls_signed, pattern
from test_weighted import plain_weights

gpu = pytest.mark.gpu

KINDS = ("ridge", "ridge-count")
LAM = (LAM_U, LAM_I)
NO_BOX = (-np.inf, np.inf, 0)
FORMS = {"wg": dict(chunk=16, max_k=128), "wave": dict(chunk=8, max_k=32)}   # MF_ALS_FORM, its gather chunk, its widest K
ALL_K = (1, 2, 3, 10, 16, 17, 30, 64, 100, 127, 128)
ALS_SYMBOLS = ("mf_plan_set_als", "mf_plan_get_als", "mf_plan_als_solve", "mf_plan_als_info", "mf_backend_run_als")


# ------------------------------------------------------------------------------------------------ the model
class Rows:
    """One side's rows as the plan walks them: ptr / idx / the position of every entry in the file order"""

    def __init__(self, nrows, own, other, order):
        own = np.asarray(own)[order]
        self.nrows = int(nrows)
        self.ptr = np.concatenate([[0], np.cumsum(np.bincount(own, minlength=nrows))]).astype(np.int64)
        self.idx = np.asarray(other)[order].astype(np.int64)
        self.pos = np.asarray(order)
        self.cnt = np.diff(self.ptr)


def sides(users, items, row, col):
    """(item rows in CSC order, user rows in CSR order), indexed as the library counts sides"""
    row, col = np.asarray(row), np.asarray(col)
    return (Rows(items, col, row, np.argsort(col, kind="stable")), Rows(users, row, col, np.argsort(row, kind="stable")))


def serial_sum(terms):
    """0.0 + terms[0] + terms[1] + ... along axis 0, one rounded addition after the other"""
    return np.add.accumulate(np.concatenate([np.zeros((1,) + terms.shape[1:]), terms]), axis=0)[-1]


@functools.lru_cache(maxsize=None)
def triangle(K):
    """(p, q) of the lower triangle, p >= q, row by row"""
    return np.tril_indices(K)


def plain_products(y, yw, out):
    """out[n] = y_n[p] * yw_n[q] over the lower triangle"""
    at = 0
    for p in range(y.shape[1]):   # row p of the triangle: q = 0 .. p
        np.multiply(y[:, p:p + 1], yw[:, :p + 1], out=out[:, at:at + p + 1])
        at += p + 1


def gram_rhs(rows, r, val, wgt, Y, xf, frozen, products=plain_products):
    """steps 1-4 of one row: (G, b), G as its lower triangle row by row"""
    K = Y.shape[1]
    G, b = np.zeros(K * (K + 1) // 2), np.zeros(K)
    for c0 in range(int(rows.ptr[r]), int(rows.ptr[r + 1]), 128):
        e = np.arange(c0, min(c0 + 128, int(rows.ptr[r + 1])))
        y, a = Y[rows.idx[e]], val[rows.pos[e]]
        if frozen >= 0:
            t = xf * y[:, frozen]
            a = a - t
        yw = y * wgt[rows.pos[e]][:, None] if wgt is not None else y
        chain = np.empty((len(e) + 1, len(G)))      # G, then the products: the serial sum is the running one
        chain[0] = G
        products(y, yw, chain[1:])
        G = np.add.accumulate(chain, axis=0, out=chain)[-1]
        b = np.add.accumulate(np.concatenate([b[None], a[:, None] * yw]), axis=0)[-1]
    return G, b


def cholesky_solve(G, b, observer=None):
    """steps 7-9 for a batch: G (B, K, K), b (B, K) -> x (B, K), positive definite (B,).  `observer`: called as
    observer("pivot", j, s, ok) with the values handed to sqrt at column j and observer("divisor", j, d, ok) with the divisors
    of that column, ok = the rows still positive definite there (a row that is not has left the solve); it only looks"""
    B, K = b.shape
    Ct = np.zeros((K, B, K))   # Ct[t][:, i] = C[i][t] of every row of the batch: column t of the factors, contiguous
    ok = np.ones(B, bool)
    for j in range(K):
        chain = np.empty((j + 1, B, K - j))   # s, then the products of t = 0 .. j-1: the chain is the running difference
        chain[0] = G[:, j:, j]
        if j:   # s = s - (C[i][t] * C[j][t]), t ascending
            np.multiply(Ct[:j, :, j:], Ct[:j, :, j][:, :, None], out=chain[1:])
            np.subtract.accumulate(chain, axis=0, out=chain)
        s = chain[-1]
        ok &= s[:, 0] > 0.0
        d = np.sqrt(s[:, 0])
        if observer is not None:
            observer("pivot", j, s[:, 0].copy(), ok.copy())
            observer("divisor", j, d.copy(), ok.copy())
        Ct[j, :, j] = d
        Ct[j, :, j + 1:] = s[:, 1:] / d[:, None]
    bb, z = b.copy(), np.empty_like(b)
    for j in range(K):
        z[:, j] = bb[:, j] / Ct[j, :, j]
        t = Ct[j, :, j + 1:] * z[:, j][:, None]
        bb[:, j + 1:] = bb[:, j + 1:] - t
    zz, x = z.copy(), np.empty_like(b)
    for j in range(K - 1, -1, -1):
        x[:, j] = zz[:, j] / Ct[j, :, j]
        t = Ct[:j, :, j].T * x[:, j][:, None]
        zz[:, :j] = zz[:, :j] - t
    return x, ok


def als_solve(rows, val, wgt, X_old, Y, lam, kind, frozen=-1, box=NO_BOX, products=plain_products, grams=None, observer=None):
    """steps 1-10 for every row of a side -> (X_new, (solved, kept_empty, kept_not_pd)).  `grams`: a dict that keeps steps 1-4
    of every row for a second solve of the same inputs (the other kind differs from step 5 on).  `observer`: cholesky_solve's,
    told observer("gram", batch, G, b) first -- the rows of the batch, their matrices with the ridge and right-hand sides"""
    K = X_old.shape[1]
    tp, tq = triangle(K)
    X_new = X_old.copy()
    todo = np.flatnonzero(rows.cnt > 0)
    kept_empty, kept_not_pd = rows.nrows - len(todo), 0
    lo, hi, ncols = box
    with np.errstate(all="ignore"):
        for b0 in range(0, len(todo), max(1, (1 << 21) // (K * K))):
            batch = todo[b0:b0 + max(1, (1 << 21) // (K * K))]
            G, b = np.empty((len(batch), K, K)), np.empty((len(batch), K))
            G[:] = 0.0
            for i, r in enumerate(batch):
                if grams is None or r not in grams:
                    g = gram_rhs(rows, r, val, wgt, Y, X_old[r, frozen] if frozen >= 0 else 0.0, frozen, products)
                    if grams is not None:
                        grams[r] = g
                G[i][tp, tq], b[i] = g if grams is None else grams[r]
            ridge = lam * rows.cnt[batch].astype(np.float64) if kind == "ridge-count" else np.full(len(batch), float(lam))
            d = np.arange(K)
            G[:, d, d] = G[:, d, d] + ridge[:, None]
            if frozen >= 0:
                G[:, frozen, :frozen] = 0.0
                G[:, frozen + 1:, frozen] = 0.0
                G[:, frozen, frozen] = 1.0
                b[:, frozen] = X_old[batch, frozen]
            if observer is not None:
                observer("gram", batch.copy(), G.copy(), b.copy())
            x, ok = cholesky_solve(G, b, observer)
            head = x[:, :ncols]
            head = np.where(head < lo, lo, head)
            head = np.where(head > hi, hi, head)
            x = np.concatenate([head, x[:, ncols:]], axis=1)
            if frozen >= 0:
                x[:, frozen] = X_old[batch, frozen]
            X_new[batch[ok]] = x[ok]
            kept_not_pd += int((~ok).sum())
    return X_new, (len(todo) - kept_not_pd, kept_empty, kept_not_pd)


class AlsModel:
    def __init__(self, users, items, row, col, val, weight=None):
        self.side = sides(users, items, row, col)
        self.val = np.asarray(val, np.float64)
        self.wgt = None if weight is None else np.asarray(weight, np.float64)

    def solve(self, side, X_old, Y, lam, kind, frozen=-1, box=NO_BOX, products=plain_products, grams=None, observer=None):
        return als_solve(self.side[side], self.val, self.wgt, X_old, Y, lam, kind, frozen, box, products, grams, observer)

    def iteration(self, L, R, lam, kind, frozen=(-1, -1), box=(NO_BOX, NO_BOX)):
        """users against R, items against the NEW L: (L', R', users' counts, items' counts); lam, frozen, box as (users, items)"""
        L1, cu = self.solve(1, L, R, lam[0], kind, frozen[0], box[0])
        R1, ci = self.solve(0, R, L1, lam[1], kind, frozen[1], box[1])
        return L1, R1, cu, ci


def fused_products_sum(y, yw, n=None):
    """the (first n) elements of the triangle, row by row, as fused multiply-adds, exactly: the rational
    y_n[p] * yw_n[q] + G rounded once per entry"""
    out = []
    for p, q in list(zip(*triangle(y.shape[1])))[:n]:
        g = 0.0
        for e in range(y.shape[0]):
            g = float(Fraction(float(y[e, p])) * Fraction(float(yw[e, q])) + Fraction(g))
        out.append(g)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def expected(pat_name, K, kind):
    """Inputs of one (pattern, K) -- the signed class of the sweep tests -- and one model iteration of `kind` at lambda
    0.05 / 0.3, computed once and shared by the forms."""
    pat = pattern(pat_name)
    x = type("Expected", (), {})()
    x.pat, x.K, x.kind = pat, K, kind
    x.L0, x.R0, x.val, x.alpha = cls_signed(4000 + K, pat, K)
    x.model = AlsModel(pat.users, pat.items, pat.row, pat.col, x.val)
    gu = _user_grams(pat_name, K)   # the users' steps 1-4 do not depend on the kind
    x.L1, x.cu = x.model.solve(1, x.L0, x.R0, LAM_U, kind, grams=gu)
    x.R1, x.ci = x.model.solve(0, x.R0, x.L1, LAM_I, kind)
    return x


@functools.lru_cache(maxsize=None)
def _user_grams(pat_name, K):
    return {}


def planted(K, seed=0):
    """Y upper triangular, small integers, positive diagonal; three integer x*; a = Y x*: every root and quotient of the
    solve is exact, so x* comes back exactly"""
    rng = np.random.default_rng(300 + K + seed)
    Y = np.triu(rng.integers(-2, 3, (K, K))).astype(np.float64)
    Y[np.arange(K), np.arange(K)] = rng.integers(1, 4, K)
    xs = rng.integers(-3, 4, (3, K)).astype(np.float64)
    return Y, xs, xs @ Y.T


def planted_instance(K):
    """three users who rated all K items, R = Y: the user solve at lambda 0 returns x*"""
    Y, xs, a = planted(K)
    row, col = np.repeat(np.arange(3), K), np.tile(np.arange(K), 3)
    return Pattern("planted", 3, K, row, col), Y, xs, a.ravel()


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("K", [1, 2, 3, 7, 16, 32])
def test_planted_integers_come_back_exactly(K):
    pat, Y, xs, a = planted_instance(K)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, a)
    rng = np.random.default_rng(K)
    for kind in KINDS:   # lambda = 0: both kinds add 0.0
        got, counts = m.solve(1, rng.uniform(-1, 1, (3, K)), Y, 0.0, kind)
        assert_same_bits(got, xs, "K=%d %s" % (K, kind))
        assert counts == (3, 0, 0)
    # checked here: the factor is Y^T, all integers, so every root and quotient was exact
    G, b = gram_rhs(m.side[1], 0, m.val, None, Y, 0.0, -1)
    assert_same_bits(G, (Y.T @ Y)[triangle(K)], "Gram matrix")
    assert (G == np.round(G)).all() and (b == np.round(b)).all()


@pytest.mark.parametrize("f", [0, 2, 4])
def test_frozen_column_gives_the_bits_of_the_reduced_system(f):
    pat, L0, R0, val, _ = _small(K=5)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    keep = [k for k in range(5) if k != f]
    for kind in KINDS:
        full, counts = m.solve(1, L0, R0, LAM_U, kind, frozen=f)
        shifted = AlsModel(pat.users, pat.items, pat.row, pat.col, val - (L0[pat.row, f] * R0[pat.col, f]))
        reduced, rcounts = shifted.solve(1, L0[:, keep], np.ascontiguousarray(R0[:, keep]), LAM_U, kind)
        assert counts == rcounts and counts[0] > 50
        assert_same_bits(full[:, keep], reduced, "frozen %d %s: the other columns" % (f, kind))
        assert_same_bits(full[:, f], L0[:, f], "frozen %d %s: the frozen column" % (f, kind))
        free, _ = m.solve(1, L0, R0, LAM_U, kind)
        assert differs(free[:, keep], full[:, keep]) > 0.5


@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed", "wide"])
def test_model_guards_against_silent_contraction(pat_name):
    """a Gram accumulation through fused multiply-adds differs from the definition on every pattern the GPU tests use (rows
    of at least two entries: the first product is added to 0.0), and the difference reaches the solved row"""
    K = 10
    pat = pattern(pat_name)
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    for side, Y in ((1, R0), (0, L0)):
        rows = m.side[side]
        seen = 0
        for r in [r for r in np.argsort(rows.cnt, kind="stable") if rows.cnt[r] >= 2][:6]:   # the six shortest rows of two entries or more
            e = np.arange(rows.ptr[r], rows.ptr[r + 1])
            y = Y[rows.idx[e]]
            G, _ = gram_rhs(rows, r, val, None, Y, 0.0, -1)
            seen += differs(G, fused_products_sum(y, y)) > 0.0
        assert seen >= 3, (pat_name, side, seen)

    def fused_chunk(y, yw, out):   # a mutant of the whole model, one ulp in the first product of every chunk: it reaches the rows
        plain_products(y, yw, out)
        out[0] = out[0] * (1.0 + 2.0 ** -52)
    mutant, _ = m.solve(1, L0, R0, LAM_U, "ridge", products=fused_chunk)
    assert differs(mutant, m.solve(1, L0, R0, LAM_U, "ridge")[0]) > 0.3


def test_fused_products_sum_is_a_fused_multiply_add():
    p = 0.1 * 0.1
    y = np.array([[1.0], [0.1]])      # -p first: the second entry's product meets it
    yw = np.array([[-p], [0.1]])
    assert fused_products_sum(y, yw, 1)[0] == float(Fraction(0.1) * Fraction(0.1) - Fraction(p)) != 0.0
    assert gram_rhs(Rows(1, [0, 0], [0, 1], [0, 1]), 0, np.zeros(2), None, y, 0.0, -1)[0][0] == 0.1 * 0.1 + 1.0   # sanity of the helper
    prods = np.empty((2, 1))
    plain_products(y, yw, prods)
    assert serial_sum(prods)[0] == 0.0


def test_als_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in ALS_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr)
    assert capi.hip().mf_backend_abi_version() == 5
    for name, value in (("MF_ALS_OFF", 0), ("MF_ALS_RIDGE", 1), ("MF_ALS_RIDGE_COUNT", 2)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr) and getattr(capi, name) == value
    for name in ("set_als", "als", "als_solve", "als_info"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_als) and callable(capi.run_als)
    contract = hdr[hdr.index("The plan's stream"):hdr.index("int mf_plan_set_stream")]
    assert "mf_plan_als_solve" in contract.split("Host only")[0] and "mf_plan_als_info" in contract.split("COMPLETE ON RETURN")[1]


def test_als_argument_and_state_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    k = C.c_int()
    assert h.mf_plan_set_als(None, 1) == capi.MF_ERR_ARGUMENT and h.mf_plan_get_als(None, C.byref(k)) == capi.MF_ERR_ARGUMENT
    for kind in (-1, 3, 7):
        assert h.mf_plan_set_als(fake, kind) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_als_solve(None, 0, 0) == capi.MF_ERR_ARGUMENT and h.mf_plan_als_info(None, 0, None, None, None) == capi.MF_ERR_ARGUMENT
    for side in (-1, 2):
        assert h.mf_plan_als_solve(fake, side, 0) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_als_info(fake, side, None, None, None) == capi.MF_ERR_ARGUMENT
    for gen in (-1, 2):
        assert h.mf_plan_als_solve(fake, 0, gen) == capi.MF_ERR_ARGUMENT
    # level 1
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    run = h.mf_backend_run_als
    assert run(None, None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, 1, 0) == capi.MF_ERR_ARGUMENT
    assert run(C.byref(p), None, None, R.ctypes.data, None, 0.1, 0.1, None, None, 1, 0) == capi.MF_ERR_ARGUMENT
    assert run(C.byref(p), None, L.ctypes.data, None, None, 0.1, 0.1, None, None, 1, 0) == capi.MF_ERR_ARGUMENT
    for lam in ((-0.5, 0.1), (0.1, float("nan"))):
        assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, *lam, None, None, 1, 0) == capi.MF_ERR_ARGUMENT
    badbox = capi.Bounds(1.0, 0.0, -1)
    assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, C.byref(badbox), None, 1, 0) == capi.MF_ERR_ARGUMENT
    for kind in (-1, 3):
        assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, kind, 0) == capi.MF_ERR_ARGUMENT
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


BAD_SOLVER = ["", "als,", "ALS", "als,count,1", "als,count,", "sgd", "als,cnt", "count", ",count", "als count", "1"]
FORBIDDEN = [dict(MATFACT_DEVICES="0"), dict(MATFACT_MATS="/dev/null"), dict(MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_RESUME="x.ck"),
             dict(MATFACT_SIMILAR="3", MATFACT_SIMILAR_OUT="sim.out"), dict(MATFACT_MOMENTUM="0.9"), dict(MATFACT_OPTIMIZER="adam,0.03")]


@pytest.mark.parametrize("env", [dict(MATFACT_SOLVER=v) for v in BAD_SOLVER] + [dict(e, MATFACT_SOLVER=s) for e in FORBIDDEN for s in ("als", "als,count")],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_solver_refusals_die_with_empty_stdout(capi, env, tmp_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(clean, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_SOLVER" in r.stderr, r
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
    """No switch from the caller's environment; the test sets its own."""
    for k in SWITCHES + ("MF_ALS_FORM",):
        monkeypatch.delenv(k, raising=False)

    def set_all(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_all


def forms_of(K):
    return [f for f in FORMS if K <= FORMS[f]["max_k"]]


def als_plan(capi, pat, K, val, kind, lam=LAM, weight=None, **kw):
    plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val, weight=weight, **kw)
    try:
        plan.set_regularization(*lam)
        plan.set_als(kind)
    except BaseException:
        plan.close()
        raise
    return plan


def check_form(plan, form, kind):
    desc = plan.describe()
    assert " als=%s als_form=%s(chunk=%d)" % (kind, form, FORMS[form]["chunk"]) in desc and "MF_ALS_FORM=%s" % form in desc, desc
    return desc


def hand_iteration(plan, where, want=None):
    """als_solve(users, current), als_solve(items, next), flip; the counters against the model's when `want` is given"""
    plan.als_solve("users", "current")
    cu = plan.als_info("users")
    plan.als_solve("items", "next")
    ci = plan.als_info("items")
    plan.flip()
    if want is not None:
        assert (cu, ci) == want, (where, cu, ci, want)
    return cu, ci


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", ALL_K)
@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed"])
def test_both_sides_in_every_form(device, switches, pat_name, K, kind):
    capi = device
    x = expected(pat_name, K, kind)
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        plan = als_plan(capi, x.pat, K, x.val, kind)
        try:
            where = "%s K=%d %s [%s]" % (pat_name, K, kind, form)
            check_form(plan, form, kind)
            assert plan.als() == kind and plan.als_info("users") == (0, 0, 0)
            plan.upload(x.L0, x.R0)
            hand_iteration(plan, where, (x.cu, x.ci))
            L, R = plan.download()
            assert_same_bits(L, x.L1, where + ": L")
            assert_same_bits(R, x.R1, where + ": R")
            assert x.cu[2] == 0 and x.ci[2] == 0 and x.cu[1] == int((x.pat.ulen == 0).sum()) and x.ci[1] == int((x.pat.ilen == 0).sum())
        finally:
            plan.close()


@gpu
def test_default_form_is_by_k(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    for K, form in ((1, "wave"), (16, "wave"), (17, "wg"), (128, "wg")):
        plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
        try:
            assert " als" not in plan.describe()
            plan.set_als("ridge")
            assert " als=ridge als_form=%s(" % form in plan.describe() and "MF_ALS_FORM" not in plan.describe()
        finally:
            plan.close()
    switches({"MF_ALS_FORM": "wave"})   # a form the K does not have: the rule's
    plan = capi.Plan(pat.users, pat.items, 33, alpha, pat.row, pat.col, val)
    try:
        plan.set_als("ridge-count")
        assert " als=ridge-count als_form=wg(" in plan.describe()
    finally:
        plan.close()


@gpu
def test_k_129_is_unsupported_and_changes_nothing(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small(K=129)
    switches({})
    plan = capi.Plan(pat.users, pat.items, 129, alpha, pat.row, pat.col, val)
    try:
        before = plan.describe()
        for kind in KINDS:
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_als(kind)
            assert err.value.status == capi.MF_ERR_UNSUPPORTED
        assert plan.als() == "off" and plan.describe() == before
        plan.set_als("off")
        plan.upload(L0, R0)
        with pytest.raises(capi.HipBackendError) as err:
            plan.als_solve("users")
        assert err.value.status == capi.MF_ERR_STATE   # the kind is OFF
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("lam", [LAM, (0.0, 0.0)], ids=["lambda", "lambda0"])
@pytest.mark.parametrize("K", [10, 30])
def test_row_lengths(device, switches, K, lam):
    """the `wide` pattern has users and items of 0 .. 34, 63, 64 and 65 entries: 0, 1, K - 1, K, K + 1, each form's gather
    chunk (8, 16) minus one, exactly and plus one, and 33 and 65 = several chunks plus one.  At lambda 0 the rows shorter than
    K are not positive definite in exact arithmetic: kept or solved as the model decides."""
    capi = device
    pat = pattern("wide")
    assert {0, 1, K - 1, K, K + 1, 7, 8, 9, 15, 16, 17, 33, 65} <= set(pat.ulen[:38]) and pat.ulen[:38].tolist() == pat.ilen[65:103].tolist()
    L0, R0, val, _ = cls_signed(4100 + K, pat, K)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    for kind in KINDS:
        L1, R1, cu, ci = m.iteration(L0, R0, lam, kind)
        if lam == LAM:
            assert cu[2] == 0 and ci[2] == 0
        elif kind == "ridge":
            # a row of K entries or more has a Gram matrix of full rank (random factors) and solves: WIDE_LENS has eight such
            # at K = 30; the shorter ones are kept, or solved on rounding noise
            assert cu[2] >= 5 and ci[2] >= 5 and cu[0] >= int((pat.ulen >= K).sum()) >= 8 and ci[0] >= 8
        for form in forms_of(K):
            switches({"MF_ALS_FORM": form})
            plan = als_plan(capi, pat, K, val, kind, lam)
            try:
                where = "wide K=%d %s [%s] lambda %s" % (K, kind, form, lam)
                plan.upload(L0, R0)
                hand_iteration(plan, where, (cu, ci))
                L, R = plan.download()
                assert_same_bits(L, L1, where + ": L")
                assert_same_bits(R, R1, where + ": R")
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("K", [1, 2, 3, 7, 16, 32])
def test_planted_integers_on_the_gpu(device, switches, K):
    capi = device
    pat, Y, xs, a = planted_instance(K)
    L0 = np.random.default_rng(K).uniform(-1, 1, (3, K))
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        plan = als_plan(capi, pat, K, a, "ridge", (0.0, 0.0))
        try:
            plan.upload(L0, Y)
            plan.als_solve("users")
            assert plan.als_info("users") == (3, 0, 0)
            plan.flip()
            assert_same_bits(plan.download()[0], xs, "K=%d [%s]" % (K, form))
        finally:
            plan.close()


def _not_pd_inputs(K):
    """the `wide` pattern with, among the items' rows, zero rows, a NaN and an infinity, and a NaN and an infinity among the
    values"""
    pat = pattern("wide")
    L0, R0, val, _ = cls_signed(4200 + K, pat, K)
    R0, val = R0.copy(), val.copy()
    R0[[2, 3, 5, 8, 13]] = 0.0
    R0[20, K // 2], R0[31, 0] = np.nan, np.inf
    special = np.zeros(pat.nnz, bool)
    for r in (12, 20, 70):
        e = np.flatnonzero(pat.row == r)[:1]
        val[e] = np.nan if r != 20 else -np.inf
        special[e] = True
    return pat, L0, R0, val, special


@gpu
@pytest.mark.parametrize("K", [10, 30])
def test_rows_that_are_not_positive_definite(device, switches, K):
    capi = device
    pat, L0, R0, val, special = _not_pd_inputs(K)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    touched_users = np.zeros(pat.users, bool)
    touched_users[pat.row[special | np.isin(pat.col, [20, 31])]] = True
    for lam in ((0.0, 0.0), LAM):
        for kind in KINDS:
            L1, R1, cu, ci = m.iteration(L0, R0, lam, kind)
            if lam == LAM:   # the same inputs solve: every row but the ones that met a NaN or an infinity
                clean = ~touched_users & (pat.ulen > 0)
                assert cu[0] >= int(clean.sum()) and cu[2] >= 1 and np.isfinite(L1[clean]).all() and differs(L1[clean], L0[clean]) > 0.9
            else:
                assert cu[2] >= 8 and ci[2] >= 8
            kept = np.flatnonzero((L1.view(np.uint64) == L0.view(np.uint64)).all(axis=1))
            assert len(kept) >= cu[1] + cu[2]
            for form in forms_of(K):
                switches({"MF_ALS_FORM": form})
                plan = als_plan(capi, pat, K, val, kind, lam)
                try:
                    where = "K=%d %s [%s] lambda %s" % (K, kind, form, lam)
                    plan.upload(L0, R0)
                    hand_iteration(plan, where, (cu, ci))
                    L, R = plan.download()
                    assert_same_bits(L, L1, where + ": L")
                    assert_same_bits(R, R1, where + ": R")
                    assert_same_bits(L[kept], L0[kept], where + ": a kept row holds X_old's bits")
                finally:
                    plan.close()


@gpu
@pytest.mark.parametrize("pat_name,K", [("small", 10), ("pair", 17), ("pair", 64)])
def test_weights_frozen_box_and_lambda_all_at_once(device, switches, pat_name, K):
    capi = device
    if pat_name == "small":
        pat, L0, R0, val, _ = _small()
    else:
        pat = pattern(pat_name)
        L0, R0, val, _ = cls_signed(4300 + K, pat, K)
    w = plain_weights(77, pat.nnz)
    frozen, box = (K - 1, 0), ((-1.0, 1.0, -1 if K == 10 else K - 1), (-1.5, 0.75, max(K // 2, 1)))
    mbox = tuple((lo, hi, K if c < 0 else c) for lo, hi, c in box)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val, w)
    plain = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    for kind in KINDS:
        L1, R1, cu, ci = m.iteration(L0, R0, LAM, kind, frozen, mbox)
        Lp, Rp, cpu, cpi = plain.iteration(L0, R0, LAM, kind, frozen, mbox)
        # the inputs do their job: the box cuts some elements and leaves others, and the weights show in those it leaves
        assert 0.002 < (np.abs(L1[:, :K - 1]) == 1.0).mean() < 0.9 and differs(L1, Lp) > 0.1 and differs(R1, Rp) > 0.1
        for form in forms_of(K):
            switches({"MF_ALS_FORM": form})
            for weight, want in ((w, (L1, R1, cu, ci)), (np.ones(pat.nnz), (Lp, Rp, cpu, cpi)), (None, (Lp, Rp, cpu, cpi))):
                plan = als_plan(capi, pat, K, val, kind, weight=weight)
                try:
                    where = "%s K=%d %s [%s] %s" % (pat_name, K, kind, form, "unweighted" if weight is None else "w[0]=%g" % weight[0])
                    plan.set_frozen_columns(*frozen)
                    plan.set_bounds("users", *box[0])
                    plan.set_bounds("items", *box[1])
                    assert (" weighted=1" in plan.describe()) == (weight is not None)
                    plan.upload(L0, R0)
                    hand_iteration(plan, where, want[2:])
                    L, R = plan.download()
                    assert_same_bits(L, want[0], where + ": L")
                    assert_same_bits(R, want[1], where + ": R")
                finally:
                    plan.close()


@gpu
def test_the_biased_layout(device, switches):
    """users' column K - 1 and items' column K - 2 frozen at 1.0: the other side's column there is its bias"""
    capi = device
    K = 12
    pat, L0, R0, val, _ = _small(K=K)
    L0, R0 = L0.copy(), R0.copy()
    L0[:, K - 1], R0[:, K - 2] = 1.0, 1.0
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    L1, R1, cu, ci = m.iteration(L0, R0, LAM, "ridge", (K - 1, K - 2))
    assert (L1[:, K - 1] == 1.0).all() and (R1[:, K - 2] == 1.0).all() and differs(L1[:, K - 2], L0[:, K - 2]) > 0.9
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        plan = als_plan(capi, pat, K, val, "ridge")
        try:
            plan.set_frozen_columns(K - 1, K - 2)
            plan.upload(L0, R0)
            hand_iteration(plan, form, (cu, ci))
            L, R = plan.download()
            assert_same_bits(L, L1, form + ": L")
            assert_same_bits(R, R1, form + ": R")
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_iterate_is_the_hand_driven_sequence(device, switches, kind):
    capi = device
    pat, L0, R0, val, alpha = _small()
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    gens = [(L0, R0)]
    for _ in range(3):
        gens.append(m.iteration(*gens[-1], LAM, kind)[:2])
    jacobi = m.solve(0, R0, L0, LAM_I, kind)[0]   # the item solve from the OLD L
    assert differs(jacobi, gens[1][1]) > 0.9
    switches({})
    plan, hand = als_plan(capi, pat, 10, val, kind), als_plan(capi, pat, 10, val, kind)
    try:
        plan.upload(L0, R0)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, gens[1][0], "iterate(1): L")
        assert_same_bits(R, gens[1][1], "iterate(1): R, solved against the new L")
        plan.iterate(2)
        hand.upload(L0, R0)
        for _ in range(3):
            hand_iteration(hand, "hand-driven")
        for got, name in ((plan.download(), "iterate"), (hand.download(), "hand-driven")):
            assert_same_bits(got[0], gens[3][0], name + ": L after three")
            assert_same_bits(got[1], gens[3][1], name + ": R after three")
        assert plan.als_info("users") == hand.als_info("users") and plan.als_info("items") == hand.als_info("items")
        # the sweep entry points stay gradient sweeps
        plain = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
        try:
            plain.set_regularization(*LAM)
            for p in (plan, plain):
                p.upload(L0, R0)
                p.sweep_items()
                p.sweep_users()
                p.flip()
            assert_same_bits(plan.download()[0], plain.download()[0], "sweep_users under ALS")
            assert_same_bits(plan.download()[1], plain.download()[1], "sweep_items under ALS")
        finally:
            plain.close()
    finally:
        plan.close()
        hand.close()


@gpu
def test_monitored_loop(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    plan, hand = als_plan(capi, pat, 10, val, "ridge"), als_plan(capi, pat, 10, val, "ridge")
    try:
        plan.upload(L0, R0)
        hand.upload(L0, R0)
        done, trace = plan.iterate_monitored(6, every=2)
        assert done == 6 and [t.iter for t in trace] == [0, 2, 4, 6]
        for t in trace:
            want = hand.loss()
            assert t.train.count == want.count == pat.nnz
            assert_same_bits(np.array([t.train.sse]), np.array([want.sse]), "trace at %d" % t.iter)
            hand_iteration(hand, "monitored")
            hand_iteration(hand, "monitored")
        assert trace[-1].train.sse < trace[0].train.sse
    finally:
        plan.close()
        hand.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lam", [0.05, 1.0])
def test_objective_decreases(device, switches, lam, kind):
    """30 x 40, K = 10, about a quarter dense, integer ratings: loss + lambda * squares (the rows' squares times their counts
    under ridge-count) after each of the 16 half-steps of 8 iterations strictly decreases and no row is kept"""
    capi = device
    d = random_instance(11, 30, 40, 10, density=0.25)
    ulen, ilen = np.bincount(d["row"], minlength=30), np.bincount(d["col"], minlength=40)
    assert ulen.min() > 0 and ilen.min() > 0
    rng = np.random.default_rng(12)
    L, R = rng.uniform(0, 1, (30, 10)), rng.uniform(0, 1, (40, 10))
    switches({})
    plan = capi.Plan(30, 40, 10, d["alpha"], d["row"], d["col"], d["val"])
    try:
        plan.set_regularization(lam)
        plan.set_als(kind)

        def objective():
            _, _, ur, ir = plan.penalty(rows=True)
            if kind == "ridge-count":
                ur, ir = ur * ulen, ir * ilen
            return plan.loss().sse + lam * (ur.sum() + ir.sum())
        plan.upload(L, R)
        obj = [objective()]
        for _ in range(8):
            for side in ("users", "items"):
                plan.als_solve(side, "current")
                info = plan.als_info(side)
                assert info[1] == 0 and info[2] == 0, info
                plan.flip()
                if side == "users":
                    L = plan.download(want_r=False)[0]
                else:
                    R = plan.download(want_l=False)[1]
                plan.upload(L, R)
                obj.append(objective())
        print("objective:", " ".join("%.6g" % o for o in obj))
        assert len(obj) == 17 and all(b < a for a, b in zip(obj, obj[1:])), obj
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("name,K", ZERO_FORMS, ids=lambda v: str(v))
def test_als_off_is_the_plain_library(device, orc, switches, name, K):
    """a plan that ran an ALS iteration and then turned it off gives the oracle's bits and the description of a plan never
    told anything; above K = 128 it was never on"""
    capi = device
    case = _pick(name, K)
    pat = pattern(case["pat"])
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    with np.errstate(all="ignore"):
        L2, R2 = L0.copy(), R0.copy()
        orc.factorize(orc.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, val), L2, R2)
    switches(case["env"])
    untold = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    try:
        if K > 128:
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_als("ridge")
            assert err.value.status == capi.MF_ERR_UNSUPPORTED
        else:
            plan.set_als("ridge")
            assert " als=ridge " in plan.describe()
            plan.upload(L0, R0)
            plan.iterate(1)   # an ALS iteration in between: what it leaves must not show afterwards
            plan.set_als("off")
        desc = plan.describe()
        assert plan.als() == "off" and case["check"](desc, K) and " als" not in desc and desc == untold.describe(), desc
        plan.upload(L0, R0)
        plan.iterate(2)
        L, R = plan.download()
        assert_same_bits(L, L2, "%s L after two" % name)
        assert_same_bits(R, R2, "%s R after two" % name)
    finally:
        plan.close()
        untold.close()


@gpu
def test_als_excludes_momentum_and_adaptive_sides(device, switches):
    """in every order the second setter returns MF_ERR_UNSUPPORTED and changes nothing"""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.set_als("ridge")
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_momentum(0.9, 0.0)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.momentum() == (0.0, 0.0) and plan.als() == "ridge"
        plan.set_momentum(0.0, 0.0)   # no momentum is no momentum
        for side in ("users", "items"):
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_adaptive(side, "adam", 0.03)
            assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.adaptive(side)[0] == "none"
        plan.set_adaptive("users", "none")
        plan.set_als("off")
        plan.set_momentum(0.0, 0.5)
        for kind in KINDS:
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_als(kind)
            assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.als() == "off" and plan.momentum() == (0.0, 0.5)
        plan.set_momentum(0.0, 0.0)
        plan.set_adaptive("items", "adagrad", 0.1)
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_als("ridge-count")
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.als() == "off" and plan.adaptive("items")[0] == "adagrad"
        assert " als" not in plan.describe()
        plan.set_adaptive("items", None)
        plan.set_als("ridge-count")
        assert plan.als() == "ridge-count"
        # without factors
        with pytest.raises(capi.HipBackendError) as err:
            plan.als_solve("users")
        assert err.value.status == capi.MF_ERR_STATE
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_two_user_shards_on_one_gpu(device, switches, kind):
    """rows of L are private: each shard's user solve gives the single plan's rows; an item's Gram matrix is a sum over all
    users, so the item solve of a shard (and its iterate) is refused"""
    capi = device
    K, cut = 30, 333
    x = expected("pair", K, kind)
    pat = x.pat
    switches({})
    lo = pat.row < cut
    for sel, begin, count in ((lo, 0, cut), (~lo, cut, pat.users - cut)):
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row[sel], pat.col[sel], x.val[sel], user_begin=begin, user_count=count)
        try:
            plan.set_regularization(*LAM)
            plan.set_als(kind)
            plan.upload(x.L0[begin:begin + count], x.R0)
            plan.als_solve("users", "current")
            empty = int((pat.ulen[begin:begin + count] == 0).sum())
            assert plan.als_info("users") == (count - empty, empty, 0)
            for call in (lambda: plan.als_solve("items", "next"), lambda: plan.als_solve("items", "current"), lambda: plan.iterate(1)):
                with pytest.raises(capi.HipBackendError) as err:
                    call()
                assert err.value.status == capi.MF_ERR_UNSUPPORTED
            plan.iterate(0)
            plan.flip()
            assert_same_bits(plan.download(want_r=False)[0], x.L1[begin:begin + count], "shard at %d" % begin)
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_backend_run_als_equals_the_plan_session(device, switches, kind):
    capi = device
    pat, L0, R0, val, alpha = _small()
    inst = capi.Instance(5, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
    w = plain_weights(5, pat.nnz)
    box = (-0.4, 0.4)
    switches({})
    plan = als_plan(capi, pat, 10, val, kind, weight=w)
    try:
        plan.set_bounds("users", *box)
        plan.upload(L0, R0)
        plan.iterate(5)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    L, R = L0.copy(), R0.copy()
    best = capi.backend_run_als(inst, L, R, kind, bounds_users=box, weight=w, lambda_users=LAM_U, lambda_items=LAM_I)
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val, w)
    want = (L0, R0)
    for _ in range(5):
        want = m.iteration(*want, LAM, kind, box=((box[0], box[1], 10), NO_BOX))[:2]
    assert_same_bits(L, want[0], "L against the model")
    assert_same_bits(R, want[1], "R against the model")
    # kind OFF: mf_backend_run_bounded without momentum
    La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
    b0 = capi.backend_run_als(inst, La, Ra, "off", lambda_users=LAM_U, lambda_items=LAM_I)
    b1 = capi.backend_run_reg(inst, Lb, Rb, LAM_U, LAM_I)
    assert_same_bits(La, Lb, "kind off: L of mf_backend_run_reg")
    assert_same_bits(Ra, Rb, "kind off: R of mf_backend_run_reg")
    assert np.array_equal(b0, b1)


def _cli(capi, path, cwd=None, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, cwd=cwd, env=dict(clean, **env))


@gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "inst0"])
def test_cli_solver(device, orc, switches, name, tmp_path):
    """MATFACT_SOLVER=als[,count], alone and with MATFACT_LAMBDA, MATFACT_BOUNDS, MATFACT_WEIGHTS and MATFACT_TOPN: stdout is
    the plan session's recommendation after the file's iterations from the reference's initialisation, byte for byte"""
    capi = device
    path = golden_in(name)
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    w = np.round(plain_weights(9, inst.nnz), 3)
    wpath = os.path.join(tmp_path, "weights.in")
    with open(wpath, "w") as f:
        f.write("%d\n%r\n%d\n%d %d %d\n" % (inst.iters, float(inst.alpha), inst.feats, inst.users, inst.items, inst.nnz))
        f.write("".join("%d %d %r\n" % (r, c, float(v)) for r, c, v in zip(inst.row, inst.col, w)))
    switches({})

    def session(kind, lam=None, box=None, weight=None):
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val, weight=weight)
        try:
            if lam:
                plan.set_regularization(*lam)
            if box:
                plan.set_bounds("users", box[0], box[1], inst.feats)
                plan.set_bounds("items", box[0], box[1], inst.feats)
            plan.set_als(kind)
            plan.upload(L0, R0)
            plan.iterate(inst.iters)
            return orc.format_out(plan.recommend()).encode()
        finally:
            plan.close()
    outs = []
    for env, args in ((dict(MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05,0.3"), dict(kind="ridge", lam=LAM)),
                      (dict(MATFACT_SOLVER="als,count", MATFACT_LAMBDA="0.1", MATFACT_BOUNDS="0,0.9"), dict(kind="ridge-count", lam=(0.1, 0.1), box=(0.0, 0.9))),
                      (dict(MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05", MATFACT_WEIGHTS=wpath), dict(kind="ridge", lam=(0.05, 0.05), weight=w))):
        r = _cli(capi, path, **env)
        outs.append(session(**args))
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == outs[-1], (env, r)
    r = _cli(capi, path, MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05,0.3", MATFACT_LOSS="%d" % inst.iters)
    assert r.returncode == 0 and r.stdout == outs[0] and r.stderr.count(b"train_rmse") == 2, r
    if name != "inst0":
        assert outs[0] != open(os.path.join(GOLDEN, name + ".out"), "rb").read()


@gpu
def test_cli_solver_with_topn_and_bias(device, switches, tmp_path):
    capi = device
    path = golden_in("inst30-40-10-2-10")
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    switches({})
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_als("ridge")
        plan.upload(L0, R0)
        plan.iterate(inst.iters)
        items = plan.recommend_topn(3, scores=False)
    finally:
        plan.close()
    r = _cli(capi, path, MATFACT_SOLVER="als", MATFACT_TOPN="3")
    lines = r.stdout.decode().splitlines()
    assert r.returncode == 0 and r.stderr == b"" and len(lines) == inst.users, r
    for u, line in enumerate(lines):
        assert [int(t) for t in line.split()] == [int(i) for i in items[u] if i >= 0], (u, line)
    # the biased model: frozen columns F + 1 (users) and F (items), the values centred; it runs and recommends
    r = _cli(capi, path, MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05", MATFACT_BIAS="1", MATFACT_LOSS="%d" % inst.iters)
    assert r.returncode == 0 and len(r.stdout.decode().splitlines()) > 0 and b"bias mu" in r.stderr, r
    rmse = [float(l.split()[3]) for l in r.stderr.decode().splitlines() if l.startswith("iter ")]
    assert len(rmse) == 2 and rmse[1] < rmse[0], r.stderr


@gpu
def test_als_behind_a_closed_gate(device, switches, gate):
    """mf_plan_als_solve and an ALS mf_plan_iterate on a busy caller-owned stream return before the gate opens and give the
    model's bits afterwards: caller-owned NaN buffers, the inputs written by torch on the stream behind the gate, the results
    cloned by torch on the stream (tests/test_stream_order.py has the instruments)"""
    import torch
    from test_stream_order import behind_gate, padded, poisoned_plan
    capi = device
    K = 30
    x = expected("pair", K, "ridge")
    pat = x.pat
    L2, R2 = x.model.iteration(x.L1, x.R1, LAM, "ridge")[:2]
    switches({})
    plan, bufs = poisoned_plan(capi, pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_als("ridge")
        plan.set_stream(gate.s.cuda_stream)

        def solves(plan, bufs):
            plan.als_solve("users", "current")
            plan.als_solve("items", "next")
            plan.flip()
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, solves, "als_solve x 2")
        assert_same_bits(got[0], padded(x.L1, bufs.ld), "als_solve: L")
        assert_same_bits(got[1], padded(x.R1, bufs.ld), "als_solve: R")
        assert plan.als_info("users") == x.cu and plan.als_info("items") == x.ci
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, lambda plan, bufs: plan.iterate(2), "iterate(2) under ALS")
        assert_same_bits(got[0], padded(L2, bufs.ld), "iterate(2): L")
        assert_same_bits(got[1], padded(R2, bufs.ld), "iterate(2): R")
        assert_same_bits(got[2], padded(x.L1, bufs.ld), "iterate(2): L of the generation before")
        assert_same_bits(got[3], padded(x.R1, bufs.ld), "iterate(2): R of the generation before")
    finally:
        plan.set_stream(None)
        plan.close()
