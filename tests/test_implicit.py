"""Implicit-feedback ALS (mf_plan_gram, mf_plan_set_confidence, MF_ALS_IMPLICIT, mf_plan_implicit_objective,
mf_backend_gram_dot, mf_backend_run_implicit, MATFACT_IMPLICIT).

The definition is include/matfact_hip.h's, operation by operation.  The model below performs it with elementwise numpy
operations -- products as arrays of their own, serial sums through ufunc.accumulate -- and borrows the Cholesky chain of
tests/test_als.py.  Every GPU result is compared with it bit for bit (NaN as a class), the row counters included; there are no
tolerances on the GPU side.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_in
from test_stream_order import gate  # noqa: F401  (the calibrated gate of the stream-order tests, once for this module)
from test_als import ALL_K, FORMS, NO_BOX, cholesky_solve, forms_of, plain_products, serial_sum, sides, triangle
from test_regularised import LAM_I, LAM_U, _small, differs, fast_dot
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits, cls_signed, pattern
from test_weighted import plain_weights

gpu = pytest.mark.gpu

LAM = (LAM_U, LAM_I)
BLOCK = 1024   # MF_LOSS_BLOCK
IMPLICIT_SYMBOLS = ("mf_plan_gram", "mf_plan_set_confidence", "mf_plan_get_confidence", "mf_plan_implicit_objective", "mf_backend_gram_dot",
                    "mf_backend_run_implicit")
GRAM_ROWS = (1, 1023, 1024, 1025, 2049, 3072)
GRAM_K = (1, 2, 3, 16, 17, 100, 127, 128)
CONFS = (0.0, 1.0, 40.0)


# ------------------------------------------------------------------------------------------------ the model
def gram(X):
    """S = X^T X as the packed lower triangle: per block of 1024 rows T = ((0.0 + x_0[p] x_0[q]) + x_1[p] x_1[q]) + ...,
    then S = ((0.0 + T_0) + T_1) + ..."""
    K = X.shape[1]
    tp, tq = triangle(K)
    totals = []
    with np.errstate(all="ignore"):
        for b0 in range(0, X.shape[0], BLOCK):
            blk = X[b0:b0 + BLOCK]
            chain = np.empty((len(blk) + 1, len(tp)))
            chain[0] = 0.0
            np.multiply(blk[:, tp], blk[:, tq], out=chain[1:])
            totals.append(np.add.accumulate(chain, axis=0, out=chain)[-1].copy())
        return serial_sum(np.array(totals)) if totals else np.zeros(len(tp))


def full(tri, K):
    """the symmetric K x K matrix of a packed lower triangle"""
    M = np.zeros((K, K))
    M[triangle(K)] = tri
    return np.where(np.tri(K, dtype=bool), M, M.T)


def gram_dot(SL, SR, K):
    """t = t + (SL[p][q] * SR[p][q]) over the full matrices, p ascending then q ascending, from 0.0"""
    with np.errstate(all="ignore"):
        return float(serial_sum((full(SL, K) * full(SR, K)).ravel()))


def implicit_solve(rows, val, wgt, X_old, Y, lam, conf, box=NO_BOX, S=None):
    """the implicit solve of every row of a side -> (X_new, (solved, 0, kept_not_pd))"""
    K = X_old.shape[1]
    tp, tq = triangle(K)
    S = gram(Y) if S is None else S
    X_new = X_old.copy()
    lo, hi, ncols = box
    not_pd = 0
    step = max(1, (1 << 21) // (K * K))
    with np.errstate(all="ignore"):
        for b0 in range(0, rows.nrows, step):
            batch = np.arange(b0, min(b0 + step, rows.nrows))
            G, b = np.zeros((len(batch), K, K)), np.zeros((len(batch), K))
            for i, r in enumerate(batch):
                g, bb = S, np.zeros(K)
                for c0 in range(int(rows.ptr[r]), int(rows.ptr[r + 1]), 128):
                    e = np.arange(c0, min(c0 + 128, int(rows.ptr[r + 1])))
                    y, a = Y[rows.idx[e]], val[rows.pos[e]]
                    en = conf * wgt[rows.pos[e]] if wgt is not None else np.full(len(e), float(conf))
                    cn = 1.0 + en
                    ye = y * en[:, None]
                    ac = a * cn
                    chain = np.empty((len(e) + 1, len(tp)))
                    chain[0] = g
                    plain_products(y, ye, chain[1:])
                    g = np.add.accumulate(chain, axis=0, out=chain)[-1]
                    bb = np.add.accumulate(np.concatenate([bb[None], ac[:, None] * y]), axis=0)[-1]
                G[i][tp, tq], b[i] = g, bb
            d = np.arange(K)
            G[:, d, d] = G[:, d, d] + float(lam)
            x, ok = cholesky_solve(G, b)
            head = x[:, :ncols]
            head = np.where(head < lo, lo, head)
            head = np.where(head > hi, hi, head)
            x = np.concatenate([head, x[:, ncols:]], axis=1)
            X_new[batch[ok]] = x[ok]
            not_pd += int((~ok).sum())
    return X_new, (rows.nrows - not_pd, 0, not_pd)


class ImplicitModel:
    def __init__(self, users, items, row, col, val, weight=None):
        self.users, self.items = users, items
        self.row, self.col = np.asarray(row), np.asarray(col)
        self.side = sides(users, items, row, col)
        self.val = np.asarray(val, np.float64)
        self.wgt = None if weight is None else np.asarray(weight, np.float64)

    def solve(self, side, X_old, Y, lam, conf, box=NO_BOX):
        return implicit_solve(self.side[side], self.val, self.wgt, X_old, Y, lam, conf, box)

    def iteration(self, L, R, lam, conf, box=(NO_BOX, NO_BOX)):
        """gram(R), users against R, gram(new L), items against the new L: (L', R', users' counts, items' counts)"""
        L1, cu = self.solve(1, L, R, lam[0], conf, box[0])
        R1, ci = self.solve(0, R, L1, lam[1], conf, box[1])
        return L1, R1, cu, ci

    def objective_parts(self, L, R, conf):
        """(all_sq, observed) of mf_plan_implicit_objective"""
        K = L.shape[1]
        with np.errstate(all="ignore"):
            all_sq = gram_dot(gram(L), gram(R), K)
            p = fast_dot(L, R, self.row, self.col)
            d = self.val - p
            en = conf * self.wgt if self.wgt is not None else np.full(len(p), float(conf))
            cn = 1.0 + en
            dd = d * d
            cd = cn * dd
            pp = p * p
            q = cd - pp
            rows = self.side[1]
            s = np.array([serial_sum(q[rows.pos[rows.ptr[r]:rows.ptr[r + 1]]]) for r in range(self.users)])
            blocks = np.array([serial_sum(s[b0:b0 + BLOCK]) for b0 in range(0, self.users, BLOCK)])
            return all_sq, float(serial_sum(blocks))

    def objective(self, L, R, lam, conf):
        a, o = self.objective_parts(L, R, conf)
        return a + o + lam[0] * float((L * L).sum()) + lam[1] * float((R * R).sum())


@functools.lru_cache(maxsize=None)
def expected(pat_name, K, conf, weighted):
    """Inputs of one (pattern, K) -- the signed class of the sweep tests -- and one model iteration, computed once and shared
    by the forms."""
    pat = pattern(pat_name)
    x = type("Expected", (), {})()
    x.pat, x.K, x.conf = pat, K, conf
    x.L0, x.R0, x.val, x.alpha = cls_signed(4000 + K, pat, K)
    x.w = plain_weights(31 + K, pat.nnz) if weighted else None
    x.model = ImplicitModel(pat.users, pat.items, pat.row, pat.col, x.val, x.w)
    x.L1, x.R1, x.cu, x.ci = x.model.iteration(x.L0, x.R0, LAM, conf)
    return x


# ------------------------------------------------------------------------------------------------ CPU
def test_implicit_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in IMPLICIT_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"\bMF_ALS_IMPLICIT = %d\b" % capi.MF_ALS_IMPLICIT, hdr) and capi.ALS_KINDS["implicit"] == capi.MF_ALS_IMPLICIT
    assert capi.MF_ALS_IMPLICIT not in (capi.MF_ALS_OFF, capi.MF_ALS_RIDGE, capi.MF_ALS_RIDGE_COUNT)
    assert re.search(r"typedef struct mf_implicit_objective \{\s*double all_sq, observed;\s*int64_t count;\s*\} mf_implicit_objective;", hdr)
    assert C.sizeof(capi.ImplicitObjective) == 24
    for name in ("gram", "set_confidence", "confidence", "implicit_objective"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_implicit) and callable(capi.run_implicit) and callable(capi.gram_dot)
    contract = hdr[hdr.index("The plan's stream"):hdr.index("int mf_plan_set_stream")]
    assert "mf_plan_gram" in contract.split("Host only")[0] and "mf_plan_implicit_objective" in contract.split("COMPLETE ON RETURN")[1]


def test_implicit_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    d = C.c_double()
    assert h.mf_plan_gram(None, 0, 0, None) == capi.MF_ERR_ARGUMENT
    for side in (-1, 2):
        assert h.mf_plan_gram(fake, side, 0, None) == capi.MF_ERR_ARGUMENT
    for gen in (-1, 2):
        assert h.mf_plan_gram(fake, 0, gen, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_set_confidence(None, 1.0) == capi.MF_ERR_ARGUMENT and h.mf_plan_get_confidence(None, C.byref(d)) == capi.MF_ERR_ARGUMENT
    for conf in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert h.mf_plan_set_confidence(fake, conf) == capi.MF_ERR_ARGUMENT, conf
    o = capi.ImplicitObjective()
    assert h.mf_plan_implicit_objective(None, C.byref(o)) == capi.MF_ERR_ARGUMENT and h.mf_plan_implicit_objective(fake, None) == capi.MF_ERR_ARGUMENT
    t = np.ones(3)
    assert h.mf_backend_gram_dot(None, t.ctypes.data, 2, C.byref(d)) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_gram_dot(t.ctypes.data, None, 2, C.byref(d)) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_gram_dot(t.ctypes.data, t.ctypes.data, 0, C.byref(d)) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_gram_dot(t.ctypes.data, t.ctypes.data, 2, None) == capi.MF_ERR_ARGUMENT
    # level 1
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    run = h.mf_backend_run_implicit
    assert run(None, None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, 1.0, 0) == capi.MF_ERR_ARGUMENT
    assert run(C.byref(p), None, None, R.ctypes.data, None, 0.1, 0.1, None, None, 1.0, 0) == capi.MF_ERR_ARGUMENT
    assert run(C.byref(p), None, L.ctypes.data, None, None, 0.1, 0.1, None, None, 1.0, 0) == capi.MF_ERR_ARGUMENT
    for lam in ((-0.5, 0.1), (0.1, float("nan"))):
        assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, *lam, None, None, 1.0, 0) == capi.MF_ERR_ARGUMENT
    badbox = capi.Bounds(1.0, 0.0, -1)
    assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, C.byref(badbox), None, 1.0, 0) == capi.MF_ERR_ARGUMENT
    for conf in (-1.0, float("nan"), float("inf")):
        assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, conf, 0) == capi.MF_ERR_ARGUMENT
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


def test_gram_dot_host_twin_gives_the_models_bits(capi):
    rng = np.random.default_rng(5)
    for K in (1, 2, 3, 17, 128):
        A, B = rng.uniform(-1, 1, (50, K)), rng.uniform(-1, 1, (70, K))
        SA, SB = gram(A), gram(B)
        assert_same_bits(np.array([capi.gram_dot(SA, SB)]), np.array([gram_dot(SA, SB, K)]), "K=%d" % K)
    SA[0] = np.nan
    assert np.isnan(capi.gram_dot(SA, SB))


def test_gram_model_cuts_blocks_at_1024_rows():
    """the block cut shows in the bits: one chain over 2000 rows is not the sum of two block totals"""
    X = np.random.default_rng(9).uniform(-1, 1, (2000, 3))
    tp, tq = triangle(3)
    one_chain = serial_sum(X[:, tp] * X[:, tq])
    assert differs(gram(X), one_chain) > 0.0
    assert_same_bits(gram(X[:1024]), serial_sum(X[:1024, tp] * X[:1024, tq]), "one block")
    assert_same_bits(gram(X), (0.0 + gram(X[:1024])) + serial_sum(X[1024:, tp] * X[1024:, tq]), "two blocks")


def test_the_definition_against_the_mathematics():
    """6 x 7, K = 4: the model's rows solve the dense normal equations A = Y^T C^u Y + lambda I, b = Y^T C^u p over ALL 7 items
    within the backward-error bound of a Cholesky solve (a small multiple of K 2^-53; 1e-10 leaves about six orders), and
    all_sq is the dense sum over all pairs to the same relative bound."""
    rng = np.random.default_rng(21)
    U, I, K, lam, conf = 6, 7, 4, 0.3, 40.0
    mask = rng.random((U, I)) < 0.4
    mask[2] = False   # a user without entries
    row, col = np.nonzero(mask)
    val, w = rng.uniform(0.5, 1.5, len(row)), rng.uniform(0.5, 3.0, len(row))
    L0, R0 = rng.uniform(-1, 1, (U, K)), rng.uniform(-1, 1, (I, K))
    for wgt in (None, w):
        m = ImplicitModel(U, I, row, col, val, wgt)
        L1, counts = m.solve(1, L0, R0, lam, conf)
        assert counts == (U, 0, 0)
        Cd, Pd = np.ones((U, I)), np.zeros((U, I))
        Cd[row, col] = 1.0 + conf * (wgt if wgt is not None else 1.0)
        Pd[row, col] = val
        for u in range(U):
            A = R0.T @ (Cd[u][:, None] * R0) + lam * np.eye(K)
            b = R0.T @ (Cd[u] * Pd[u])
            x = L1[u]
            resid = np.abs(A @ x - b).max()
            bound = 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())
            assert resid <= bound, (u, resid, bound)
        assert (L1[2].view(np.uint64) == 0).all()   # the cold row: +0.0 in every column
        dense = float((((L1 @ R0.T) ** 2)).sum())
        all_sq, observed = m.objective_parts(L1, R0, conf)
        assert abs(all_sq - dense) <= 1e-10 * dense
        # and the whole objective is the dense one
        want = float((Cd * (Pd - L1 @ R0.T) ** 2).sum())
        assert abs((all_sq + observed) - want) <= 1e-10 * (abs(all_sq) + abs(observed))


@functools.lru_cache(maxsize=None)
def inst30_objectives():
    """inst30-40-10-2-10 from the reference initialisation, lambda 0.05 / 0.3, conf 40: the generations and the objective's parts
    before and after each of 5 iterations"""
    import recommender_system_amd as rs
    capi = rs.capi
    inst = capi.parse_file(golden_in("inst30-40-10-2-10"))
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    m = ImplicitModel(inst.users, inst.items, inst.row, inst.col, inst.val)
    gens, parts = [(L, R)], [m.objective_parts(L, R, 40.0)]
    for _ in range(5):
        L, R = m.iteration(L, R, LAM, 40.0)[:2]
        gens.append((L, R))
        parts.append(m.objective_parts(L, R, 40.0))
    return inst, m, gens, parts


def test_the_models_objective_decreases_on_inst30():
    inst, m, gens, parts = inst30_objectives()
    obj = [m.objective(L, R, LAM, 40.0) for L, R in gens]
    print("objective:", " ".join("%.17g" % o for o in obj))
    assert len(obj) == 6 and all(b < a for a, b in zip(obj, obj[1:])), obj


BAD_IMPLICIT = ["", "x", "-1", "nan", "inf", "1,2", "40 "]


def _cli(capi, path, cwd=None, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, cwd=cwd, env=dict(clean, **env))


@pytest.mark.parametrize("env,word", [(dict(MATFACT_IMPLICIT=v, MATFACT_SOLVER="als"), b"MATFACT_IMPLICIT: expected") for v in BAD_IMPLICIT] + [
    (dict(MATFACT_IMPLICIT="40"), b"MATFACT_IMPLICIT needs MATFACT_SOLVER=als."),
    (dict(MATFACT_IMPLICIT="40", MATFACT_SOLVER="als,count"), b"MATFACT_IMPLICIT cannot be combined with MATFACT_SOLVER=als,count."),
    (dict(MATFACT_IMPLICIT="40", MATFACT_SOLVER="als", MATFACT_BIAS="1"), b"MATFACT_IMPLICIT cannot be combined with MATFACT_BIAS"),
    (dict(MATFACT_IMPLICIT="40", MATFACT_SOLVER="sgd"), b"MATFACT_SOLVER: expected als or als,count."),
    (dict(MATFACT_IMPLICIT="40", MATFACT_SOLVER="als", MATFACT_MOMENTUM="0.9"), b"MATFACT_SOLVER works on the single-GPU path only"),
], ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())) if isinstance(e, dict) else None)
def test_cli_implicit_refusals_die_with_empty_stdout(capi, env, word, tmp_path):
    r = _cli(capi, os.path.join(tmp_path, "no-such-file.in"), cwd=tmp_path, **env)
    assert r.returncode == 255 and r.stdout == b"" and word in r.stderr, r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    assert not os.listdir(tmp_path)


def test_cli_implicit_accepts_its_value_and_then_reads_the_input(capi, tmp_path):
    for v in ("0", "40", "1e-3", "2.5"):
        r = _cli(capi, os.path.join(tmp_path, "no-such-file.in"), cwd=tmp_path, MATFACT_IMPLICIT=v, MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05")
        assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_" not in r.stderr, r   # the parser's message: the options passed


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


def implicit_plan(capi, pat, K, val, conf, lam=LAM, weight=None, **kw):
    plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val, weight=weight, **kw)
    try:
        plan.set_regularization(*lam)
        plan.set_confidence(conf)
        plan.set_als("implicit")
    except BaseException:
        plan.close()
        raise
    return plan


def check_form(plan, form, conf):
    desc = plan.describe()
    assert " als=implicit conf=%.17g als_form=%s(chunk=%d)" % (conf, form, FORMS[form]["chunk"]) in desc and "MF_ALS_FORM=%s" % form in desc, desc


def hand_iteration(plan, where, want=None):
    plan.als_solve("users", "current")
    cu = plan.als_info("users")
    plan.als_solve("items", "next")
    ci = plan.als_info("items")
    plan.flip()
    if want is not None:
        assert (cu, ci) == want, (where, cu, ci, want)
    return cu, ci


def sparse_entries(users, items, seed):
    """a handful of entries: most rows of both sides have none"""
    rng = np.random.default_rng(seed)
    n = min(users * items, 40)
    cells = np.sort(rng.choice(users * items, n, replace=False))
    return Pattern("sparse", users, items, cells // items, cells % items)


def four_grams(plan, users, items, K, rng):
    """both generations of both sides hold factors of their own; returns what was uploaded as (next, current)"""
    nxt = rng.uniform(-1, 1, (users, K)), rng.uniform(-1, 1, (items, K))
    cur = rng.uniform(-1, 1, (users, K)), rng.uniform(-1, 1, (items, K))
    plan.upload(*nxt)
    plan.flip()
    plan.upload(*cur)
    return nxt, cur


@gpu
@pytest.mark.parametrize("K", GRAM_K)
@pytest.mark.parametrize("i", range(len(GRAM_ROWS)), ids=lambda i: "rows%d" % GRAM_ROWS[i])
def test_gram_of_both_sides_in_both_generations(device, switches, i, K):
    """users = one row count of the list, items = the next one: over the parametrisation every count sits on both sides"""
    capi = device
    users, items = GRAM_ROWS[i], GRAM_ROWS[(i + 1) % len(GRAM_ROWS)]
    pat = sparse_entries(users, items, 70 + i)
    assert (pat.ulen == 0).any() or users == 1
    switches({})
    plan = capi.Plan(users, items, K, 1e-3, pat.row, pat.col, np.ones(pat.nnz))
    try:
        nxt, cur = four_grams(plan, users, items, K, np.random.default_rng(100 * i + K))
        for gen, (L, R) in (("current", cur), ("next", nxt)):
            assert_same_bits(plan.gram("users", gen), gram(L), "users %d x %d %s" % (users, K, gen))
            assert_same_bits(plan.gram("items", gen), gram(R), "items %d x %d %s" % (items, K, gen))
        # enqueue only, then the same buffer through a second call
        assert plan.gram("users", "current", download=False) is None
        plan.synchronize()
        assert_same_bits(plan.gram("users", "current"), gram(cur[0]), "again")
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("rows,K", [(1025, 17), (2049, 100), (3, 2)])
def test_gram_special_values(device, switches, rows, K):
    capi = device
    pat = sparse_entries(rows, 5, 3)
    rng = np.random.default_rng(rows + K)
    L, R = rng.uniform(-1, 1, (rows, K)), rng.uniform(-1, 1, (5, K))
    L[rows // 2, K - 1] = np.nan
    L[rows - 1, 0] = np.inf
    L[0, K // 2] = -0.0
    if rows > 3:
        L[rows // 3] = -0.0
    R[:] = -0.0     # every product is (-0.0) * (-0.0) = +0.0 ...
    R[2, 0] = 0.0   # ... or (+0.0) * (-0.0) = -0.0, added to a +0.0
    switches({})
    plan = capi.Plan(rows, 5, K, 1e-3, pat.row, pat.col, np.ones(pat.nnz))
    try:
        plan.upload(L, R)
        S = gram(L)
        assert np.isnan(S).any() and (np.isinf(S).any() or K == 1) and (K < 3 or np.isfinite(S).any())
        assert_same_bits(plan.gram("users"), S, "users")
        assert_same_bits(plan.gram("items"), gram(R), "items of zeros")
        assert (gram(R).view(np.uint64) == 0).all()   # (+0.0) + anything of zeros stays +0.0
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("K", [10, 30, 62])
def test_gram_never_reads_the_padding_of_a_row(device, switches, K):
    """caller-owned buffers at the library's pitch (whole 128-byte lines for these even K: wider than K), NaN in every padding
    element"""
    from test_stream_order import poisoned_plan
    capi = device
    users, items = 1500, 300
    pat = sparse_entries(users, items, 8)
    switches({})
    plan, bufs = poisoned_plan(capi, users, items, K, 1e-3, pat.row, pat.col, np.ones(pat.nnz))
    try:
        assert bufs.ld > K
        nxt, cur = four_grams(plan, users, items, K, np.random.default_rng(K))
        for gen, (L, R) in (("current", cur), ("next", nxt)):
            got = plan.gram("users", gen), plan.gram("items", gen)
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
            assert_same_bits(got[0], gram(L), "users " + gen)
            assert_same_bits(got[1], gram(R), "items " + gen)
        import torch
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t[:, K:]).all()) for t in bufs.l + bufs.r)   # and never written
    finally:
        plan.close()


@gpu
def test_gram_errors(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small(K=129)
    switches({})
    plan = capi.Plan(pat.users, pat.items, 129, alpha, pat.row, pat.col, val)
    small = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        for call in (lambda: small.gram("users"), small.implicit_objective):
            with pytest.raises(capi.HipBackendError) as err:
                call()
            assert err.value.status == capi.MF_ERR_STATE   # no factors
        plan.upload(L0, R0)
        for call in (lambda: plan.gram("users"), plan.implicit_objective, lambda: plan.set_als("implicit")):
            with pytest.raises(capi.HipBackendError) as err:
                call()
            assert err.value.status == capi.MF_ERR_UNSUPPORTED
        assert plan.als() == "off"
    finally:
        plan.close()
        small.close()


def _variant(pat_name, K):
    """the confidence and the weights of one (pattern, K) of the wide test: every conf and both kinds of plan over the list"""
    n = ALL_K.index(K) + ("pair", "skewed", "long-items").index(pat_name)
    return CONFS[n % 3], bool(n % 2)


@gpu
@pytest.mark.parametrize("pat_name,K", [(p, K) for p in ("pair", "skewed") for K in ALL_K] + [("long-items", K) for K in (1, 3, 10, 17, 30)])
def test_both_sides_in_every_form(device, switches, pat_name, K):
    capi = device
    conf, weighted = _variant(pat_name, K)
    x = expected(pat_name, K, conf, weighted)
    empty_u, empty_i = x.pat.ulen == 0, x.pat.ilen == 0
    assert x.cu[1] == 0 and x.ci[1] == 0 and x.cu[2] == 0 and x.ci[2] == 0 and x.cu[0] == x.pat.users and x.ci[0] == x.pat.items
    assert (x.L1[empty_u].view(np.uint64) == 0).all() and (x.R1[empty_i].view(np.uint64) == 0).all() and (empty_u.any() or pat_name != "pair")
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        plan = implicit_plan(capi, x.pat, K, x.val, conf, weight=x.w)
        try:
            where = "%s K=%d conf=%g %s [%s]" % (pat_name, K, conf, "weighted" if weighted else "unweighted", form)
            check_form(plan, form, conf)
            assert plan.als() == "implicit" and plan.confidence() == conf and plan.als_info("users") == (0, 0, 0)
            plan.upload(x.L0, x.R0)
            hand_iteration(plan, where, (x.cu, x.ci))
            L, R = plan.download()
            assert_same_bits(L, x.L1, where + ": L")
            assert_same_bits(R, x.R1, where + ": R")
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("conf", CONFS)
@pytest.mark.parametrize("K", [10, 30])
def test_every_confidence_weighted_and_not(device, switches, K, conf, weighted):
    capi = device
    x = expected("pair", K, conf, weighted)
    if conf == 0.0:   # c = 1 everywhere: the weights drop out, and so does every entry's share of G
        other = expected("pair", K, conf, not weighted)
        assert_same_bits(x.L1, other.L1, "conf 0: the weights play no part")
    else:
        assert differs(x.L1, expected("pair", K, 0.0, weighted).L1) > 0.5
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        plan = implicit_plan(capi, x.pat, K, x.val, conf, weight=x.w)
        try:
            where = "K=%d conf=%g weighted=%d [%s]" % (K, conf, weighted, form)
            plan.upload(x.L0, x.R0)
            hand_iteration(plan, where, (x.cu, x.ci))
            L, R = plan.download()
            assert_same_bits(L, x.L1, where + ": L")
            assert_same_bits(R, x.R1, where + ": R")
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("lo", [0.0, 0.125])
@pytest.mark.parametrize("K", [10, 17])
def test_with_a_box(device, switches, K, lo):
    """[lo, 0.5] on all columns of both sides: a row without entries comes out +0.0, or lo under a positive lo"""
    capi = device
    pat = pattern("pair")
    L0, R0, val, _ = cls_signed(4400 + K, pat, K)
    w = plain_weights(3, pat.nnz)
    m = ImplicitModel(pat.users, pat.items, pat.row, pat.col, val, w)
    box = (lo, 0.5, K)
    L1, R1, cu, ci = m.iteration(L0, R0, LAM, 40.0, (box, box))
    empty = pat.ulen == 0
    assert empty.sum() >= 3 and cu[1] == 0
    assert_same_bits(L1[empty], np.full((int(empty.sum()), K), lo), "cold rows")
    assert 0.01 < (L1 == 0.5).mean() < 0.9 and 0.01 < (L1 == lo).mean() < 0.9
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        plan = implicit_plan(capi, pat, K, val, 40.0, weight=w)
        try:
            plan.set_bounds("users", lo, 0.5)
            plan.set_bounds("items", lo, 0.5, K)
            plan.upload(L0, R0)
            hand_iteration(plan, form, (cu, ci))
            L, R = plan.download()
            assert_same_bits(L, L1, form + ": L")
            assert_same_bits(R, R1, form + ": R")
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("K", [10, 30])
def test_a_nan_in_y_keeps_every_row(device, switches, K):
    capi = device
    x = expected("pair", K, 40.0, False)
    R0 = x.R0.copy()
    R0[7, 0] = np.nan     # column 0 of S is NaN: the first pivot of every row
    L1, cu = x.model.solve(1, x.L0, R0, LAM_U, 40.0)
    assert cu == (0, 0, x.pat.users)
    assert_same_bits(L1, x.L0, "the model keeps X_old")
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        plan = implicit_plan(capi, x.pat, K, x.val, 40.0)
        try:
            plan.upload(x.L0, R0)
            plan.als_solve("users", "current")
            assert plan.als_info("users") == cu
            plan.flip()
            assert_same_bits(plan.download(want_r=False)[0], x.L0, form)
        finally:
            plan.close()


@gpu
def test_frozen_columns_and_momentum_are_refused(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    plan = implicit_plan(capi, pat, 10, val, 40.0)
    try:
        plan.upload(L0, R0)
        plan.set_frozen_columns(3, -1)
        for call in (lambda: plan.als_solve("users"), lambda: plan.iterate(1), lambda: plan.iterate_monitored(2)):
            with pytest.raises(capi.HipBackendError) as err:
                call()
            assert err.value.status == capi.MF_ERR_UNSUPPORTED
        plan.iterate(0)
        assert plan.als_info("users") == (0, 0, 0) and plan.als_info("items") == (0, 0, 0)   # nothing was enqueued
        L, R = plan.download()
        assert_same_bits(L, L0, "L untouched")
        assert_same_bits(R, R0, "R untouched")
        plan.als_solve("items", "current")     # the items' side has no frozen column
        assert plan.als_info("items") == (pat.items, 0, 0)
        plan.set_frozen_columns(-1, 0)
        with pytest.raises(capi.HipBackendError) as err:
            plan.als_solve("items")
        assert err.value.status == capi.MF_ERR_UNSUPPORTED
        plan.als_solve("users")
        plan.set_frozen_columns(-1, -1)
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_momentum(0.9, 0.0)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.momentum() == (0.0, 0.0) and plan.als() == "implicit"
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_adaptive("items", "adam", 0.03)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED
        plan.set_als("off")
        plan.set_momentum(0.5, 0.0)
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_als("implicit")
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.als() == "off" and " als" not in plan.describe()
        for conf in (-1.0, float("nan"), float("inf")):
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_confidence(conf)
            assert err.value.status == capi.MF_ERR_ARGUMENT and plan.confidence() == 40.0
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_iterate_is_the_gauss_seidel_order(device, switches, weighted):
    capi = device
    pat, L0, R0, val, alpha = _small()
    w = plain_weights(17, pat.nnz) if weighted else None
    m = ImplicitModel(pat.users, pat.items, pat.row, pat.col, val, w)
    gens = [(L0, R0)]
    for _ in range(3):
        gens.append(m.iteration(*gens[-1], LAM, 40.0)[:2])
    jacobi = m.solve(0, R0, L0, LAM_I, 40.0)[0]   # the item solve from the OLD L
    assert differs(jacobi, gens[1][1]) > 0.9
    switches({})
    plan, hand = implicit_plan(capi, pat, 10, val, 40.0, weight=w), implicit_plan(capi, pat, 10, val, 40.0, weight=w)
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
        # the confidence is read at every launch
        plan.set_confidence(1.0)
        plan.iterate(1)
        want = m.iteration(*gens[3], LAM, 1.0)[:2]
        assert_same_bits(plan.download()[0], want[0], "conf changed between two calls")
        # level 1
        inst = capi.Instance(3, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
        L, R = L0.copy(), R0.copy()
        best = capi.backend_run_implicit(inst, L, R, 40.0, weight=w, lambda_users=LAM_U, lambda_items=LAM_I)
        assert_same_bits(L, gens[3][0], "mf_backend_run_implicit: L")
        assert_same_bits(R, gens[3][1], "mf_backend_run_implicit: R")
        assert np.array_equal(best, hand.recommend())
    finally:
        plan.close()
        hand.close()


@gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("pat_name,K", [("pair", 10), ("pair", 17), ("skewed", 30), ("long-items", 100)])
def test_objective_parts_equal_the_model(device, switches, pat_name, K, weighted):
    capi = device
    x = expected(pat_name, K, 40.0, weighted) if pat_name != "long-items" else None
    if x is None:   # no model iteration at K = 100 on 2600 rows: the objective of the inputs alone
        pat = pattern(pat_name)
        L0, R0, val, _ = cls_signed(4000 + K, pat, K)
        w = plain_weights(31 + K, pat.nnz) if weighted else None
        m = ImplicitModel(pat.users, pat.items, pat.row, pat.col, val, w)
        states = [(L0, R0)]
    else:
        pat, val, w, m = x.pat, x.val, x.w, x.model
        states = [(x.L0, x.R0), (x.L1, x.R1)]
    switches({})
    plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val, weight=w)   # any kind: here none
    try:
        for conf in (40.0, 0.0):
            plan.set_confidence(conf)
            for n, (L, R) in enumerate(states):
                plan.upload(L, R)
                all_sq, observed, count = plan.implicit_objective()
                want = m.objective_parts(L, R, conf)
                assert count == pat.nnz
                assert_same_bits(np.array([all_sq, observed]), np.array(want), "%s K=%d conf=%g state %d" % (pat_name, K, conf, n))
    finally:
        plan.close()


@gpu
def test_objective_decreases_on_inst30_and_equals_the_model(device, switches):
    capi = device
    inst, m, gens, parts = inst30_objectives()
    switches({})
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_confidence(40.0)
        plan.set_als("implicit")
        plan.upload(*gens[0])
        obj = []
        for it in range(6):
            if it:
                plan.iterate(1)
            L, R = plan.download()
            assert_same_bits(L, gens[it][0], "L after %d" % it)
            assert_same_bits(R, gens[it][1], "R after %d" % it)
            all_sq, observed, count = plan.implicit_objective()
            assert_same_bits(np.array([all_sq, observed]), np.array(parts[it]), "objective after %d" % it)
            us, its = plan.penalty()
            obj.append(all_sq + observed + LAM_U * us + LAM_I * its)
            assert plan.als_info("users")[2] == 0 and plan.als_info("items")[2] == 0
        print("objective:", " ".join("%.17g" % o for o in obj))
        assert all(b < a for a, b in zip(obj, obj[1:])), obj
    finally:
        plan.close()


@gpu
def test_user_solve_on_a_shard_and_item_solve_refused(device, switches):
    capi = device
    K, cut = 30, 333
    x = expected("pair", K, 40.0, False)
    pat = x.pat
    switches({})
    lo = pat.row < cut
    for sel, begin, count in ((lo, 0, cut), (~lo, cut, pat.users - cut)):
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row[sel], pat.col[sel], x.val[sel], user_begin=begin, user_count=count)
        try:
            plan.set_regularization(*LAM)
            plan.set_confidence(40.0)
            plan.set_als("implicit")
            plan.upload(x.L0[begin:begin + count], x.R0)
            plan.als_solve("users", "current")
            assert plan.als_info("users") == (count, 0, 0)
            for call in (lambda: plan.als_solve("items", "next"), lambda: plan.iterate(1)):
                with pytest.raises(capi.HipBackendError) as err:
                    call()
                assert err.value.status == capi.MF_ERR_UNSUPPORTED
            plan.flip()
            assert_same_bits(plan.download(want_r=False)[0], x.L1[begin:begin + count], "shard at %d" % begin)
        finally:
            plan.close()


@gpu
def test_cli_implicit(device, orc, switches, tmp_path):
    """MATFACT_IMPLICIT=40 next to MATFACT_SOLVER=als and MATFACT_LAMBDA: stdout is the plan session's recommendation after the
    file's iterations, stderr the one objective line in %.17g"""
    capi = device
    path = golden_in("inst30-40-10-2-10")
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    switches({})
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_confidence(40.0)
        plan.set_als("implicit")
        plan.upload(L0, R0)
        plan.iterate(inst.iters)
        best = plan.recommend()
        all_sq, observed, _ = plan.implicit_objective()
        us, its = plan.penalty()
    finally:
        plan.close()
    r = _cli(capi, path, MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05,0.3", MATFACT_IMPLICIT="40")
    assert r.returncode == 0 and r.stdout == orc.format_out(best).encode(), r
    lines = r.stderr.decode().strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("implicit conf 40 "), r.stderr
    words = lines[0].split()
    got = {words[i]: float(words[i + 1]) for i in range(1, len(words), 2)}
    assert got == dict(conf=40.0, all_sq=all_sq, observed=observed, users_sq=us, items_sq=its,
                       objective=((all_sq + observed) + LAM_U * us) + LAM_I * its), (got, all_sq, observed)


@gpu
def test_implicit_behind_a_closed_gate(device, switches, gate):
    """mf_plan_als_solve under the implicit kind (its Gram launches included), mf_plan_gram without a host pointer and an
    implicit mf_plan_iterate on a busy caller-owned stream return before the gate opens and give the model's bits afterwards"""
    from test_stream_order import behind_gate, padded, poisoned_plan
    capi = device
    K = 30
    x = expected("pair", K, 40.0, False)
    pat = x.pat
    L2, R2 = x.model.iteration(x.L1, x.R1, LAM, 40.0)[:2]
    switches({})
    plan, bufs = poisoned_plan(capi, pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_confidence(40.0)
        plan.set_als("implicit")
        plan.set_stream(gate.s.cuda_stream)

        def solves(plan, bufs):
            plan.gram("items", "current", download=False)
            plan.als_solve("users", "current")
            plan.als_solve("items", "next")
            plan.flip()
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, solves, "implicit als_solve x 2")
        assert_same_bits(got[0], padded(x.L1, bufs.ld), "als_solve: L")
        assert_same_bits(got[1], padded(x.R1, bufs.ld), "als_solve: R")
        assert plan.als_info("users") == x.cu and plan.als_info("items") == x.ci
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, lambda plan, bufs: plan.iterate(2), "iterate(2) under the implicit kind")
        assert_same_bits(got[0], padded(L2, bufs.ld), "iterate(2): L")
        assert_same_bits(got[1], padded(R2, bufs.ld), "iterate(2): R")
        assert_same_bits(got[2], padded(x.L1, bufs.ld), "iterate(2): L of the generation before")
        assert_same_bits(got[3], padded(x.R1, bufs.ld), "iterate(2): R of the generation before")
    finally:
        plan.set_stream(None)
        plan.close()
