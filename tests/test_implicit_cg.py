"""Implicit-feedback ALS by conjugate gradient (mf_plan_set_implicit_cg, mf_plan_get_implicit_cg, mf_backend_run_implicit_cg,
MATFACT_IMPLICIT_CG).

The definition is include/matfact_hip.h's steps J0-J5.  The model below performs them literally with elementwise numpy
operations -- products formed as arrays of their own, serial sums through ufunc.accumulate -- in the style of
tests/test_als_cg.py, whose dot and serial_last it uses, with tests/test_implicit.py's Gram.  Rows of equal length are taken
together.  Every GPU result is compared with it bit for bit (assert_same_bits: NaN as a class), the three row counters
included; there are no tolerances on the GPU side.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, golden_in
from test_stream_order import gate, long_rows  # noqa: F401  (the calibrated gate of the stream-order tests, once for this module)
from test_als import NO_BOX, sides
from test_als_cg import BAD_STEPS, chunk_of, dot, forms_of, serial_last
from test_implicit import ImplicitModel, full, gram
from test_regularised import LAM_I, LAM_U, _small, differs
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits, cls_signed, pattern
from test_weighted import plain_weights

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa  # noqa: E402

gpu = pytest.mark.gpu

LAM = (LAM_U, LAM_I)
CONFS = (0.0, 1.0, 40.0)
FIXED_K = (10, 20, 30, 50, 100, 128)
# every compile-time K of als_cg_fn<mf::AlsImplicit> and both ends of the range of K of its run-time instances (2 .. 128 under
# the LDS-DMA gather, 1 .. 127 through registers; 128 runs there too, forced): tests/test_als_edges.py checks this list against
# the table
ALL_K = (1, 2, 3, 10, 16, 17, 20, 30, 50, 64, 100, 127, 128)
ICG_SYMBOLS = ("mf_plan_set_implicit_cg", "mf_plan_get_implicit_cg", "mf_backend_run_implicit_cg")


# ------------------------------------------------------------------------------------------------ the model
def s_times(Sf, v):
    """sx[k] = ((0.0 + S(k, 0) * v[0]) + S(k, 1) * v[1]) + ..., j ascending: Sf (K, K) symmetric, v (B, K) -> (B, K)"""
    return serial_last(Sf[None, :, :] * v[:, None, :], -1)


def entry_pass(y, a, e, v, residual):
    """sum_n f_n * y_n, n ascending, with t_n = dot(y_n, v) and f_n = (a_n * (1.0 + e_n)) - (e_n * t_n) (residual: J1, J2) or
    t_n * e_n (J4b, c).  y (B, c, K), a / e (B, c), v (B, K) -> (B, K); a row without entries has the empty sum, 0.0"""
    if y.shape[1] == 0:
        return np.zeros_like(v)
    t = dot(y, v[:, None, :])
    if residual:
        cn = 1.0 + e
        ac = a * cn
        f = ac - (e * t)
    else:
        f = t * e
    return serial_last(f[:, :, None] * y, 1)


def icg_side(rows, val, wgt, X_old, Y, lam, conf, steps, box=NO_BOX, S=None, sv=s_times, passes=entry_pass):
    """J0-J5 for every row of a side.  `steps`: a number, or a tuple of numbers -- then {steps: result}.
    result = (X_new, (solved, 0, kept_not_pd))"""
    wanted = (steps,) if isinstance(steps, int) else tuple(steps)
    K = X_old.shape[1]
    lo, hi, ncols = box
    out = {s: [X_old.copy(), 0] for s in wanted}
    ridge = float(lam)

    def finish(s, R, x, notpd):
        head = x[:, :ncols]
        head = np.where(head < lo, lo, head)
        head = np.where(head > hi, hi, head)
        xx = np.concatenate([head, x[:, ncols:]], axis=1)
        out[s][0][R[~notpd]] = xx[~notpd]
        out[s][1] += int(notpd.sum())

    with np.errstate(all="ignore"):
        Sf = full(gram(Y) if S is None else S, K)
        for c in np.unique(rows.cnt):
            group = np.flatnonzero(rows.cnt == c)
            per = max(1, (1 << 21) // (max(int(c), K) * K))
            for b0 in range(0, len(group), per):
                R = group[b0:b0 + per]
                e = rows.ptr[R][:, None] + np.arange(int(c))[None, :]
                y, a = Y[rows.idx[e]], val[rows.pos[e]]
                en = conf * wgt[rows.pos[e]] if wgt is not None else np.full(a.shape, float(conf))
                x = X_old[R].copy()                                                  # J0
                g = passes(y, a, en, x, True)                                        # J1, J2
                sx = sv(Sf, x)
                r = (g - sx) - (ridge * x)
                p, rs = r.copy(), dot(r, r)                                          # J3
                active, notpd = np.ones(len(R), bool), np.zeros(len(R), bool)
                for s in range(1, max(wanted) + 1):                                  # J4
                    active &= ~(rs == 0.0)                                           # a: a NaN is not equal and goes on
                    i = np.flatnonzero(active)
                    if len(i):
                        q = passes(y[i], None, en[i], p[i], False)                   # b, c
                        sp = sv(Sf, p[i])
                        q = (q + sp) + (ridge * p[i])
                        pq = dot(p[i], q)                                            # d
                        bad = ~(pq > 0.0)
                        notpd[i[bad]], active[i[bad]] = True, False
                        i, q, pq = i[~bad], q[~bad], pq[~bad]
                        alpha = (rs[i] / pq)[:, None]                                # e
                        x[i] = x[i] + (alpha * p[i])
                        r[i] = r[i] - (alpha * q)
                        rn = dot(r[i], r[i])                                         # f
                        beta = (rn / rs[i])[:, None]
                        p[i] = r[i] + (beta * p[i])
                        rs[i] = rn
                    if s in out:
                        finish(s, R, x, notpd)
    res = {s: (X, (rows.nrows - bad, 0, bad)) for s, (X, bad) in out.items()}
    return res[steps] if isinstance(steps, int) else res


class IcgModel:
    def __init__(self, users, items, row, col, val, weight=None):
        self.side = sides(users, items, row, col)
        self.val = np.asarray(val, np.float64)
        self.wgt = None if weight is None else np.asarray(weight, np.float64)

    def solve(self, side, X_old, Y, lam, conf, steps, box=NO_BOX, **kw):
        return icg_side(self.side[side], self.val, self.wgt, X_old, Y, lam, conf, steps, box, **kw)

    def iteration(self, L, R, lam, conf, steps, box=(NO_BOX, NO_BOX)):
        """gram(R), users against R, gram(new L), items against the new L: (L', R', users' counts, items' counts)"""
        L1, cu = self.solve(1, L, R, lam[0], conf, steps, box[0])
        R1, ci = self.solve(0, R, L1, lam[1], conf, steps, box[1])
        return L1, R1, cu, ci


def _variant(pat_name, K):
    """the confidence and the weights of one (pattern, K) of the wide test: every conf and both kinds of plan over the list"""
    n = ALL_K.index(K) + ("pair", "skewed", "long-items").index(pat_name)
    return CONFS[n % 3], bool(n % 2)


@functools.lru_cache(maxsize=None)
def expected(pat_name, K, conf, weighted, steps):
    """Inputs of one (pattern, K) -- the signed class of the sweep tests -- and one model iteration, computed once and shared
    by the forms."""
    pat = pattern(pat_name)
    x = type("Expected", (), {})()
    x.pat, x.K, x.conf, x.steps = pat, K, conf, steps
    x.L0, x.R0, x.val, x.alpha = cls_signed(4000 + K, pat, K)
    x.w = plain_weights(31 + K, pat.nnz) if weighted else None
    x.model = IcgModel(pat.users, pat.items, pat.row, pat.col, x.val, x.w)
    x.L1, x.cu = _user_solves(pat_name, K, conf, weighted)[steps]
    x.R1, x.ci = x.model.solve(0, x.R0, x.L1, LAM_I, conf, steps)
    return x


@functools.lru_cache(maxsize=None)
def _user_solves(pat_name, K, conf, weighted):
    """the users after 1 and after 3 steps from one run of the model"""
    pat = pattern(pat_name)
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    w = plain_weights(31 + K, pat.nnz) if weighted else None
    return IcgModel(pat.users, pat.items, pat.row, pat.col, val, w).solve(1, L0, R0, LAM_U, conf, (1, 3))


# ------------------------------------------------------------------------------------------------ CPU
def test_icg_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in ICG_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION +5\b", hdr)   # the change only adds symbols
    for name in ("set_implicit_cg", "implicit_cg"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_implicit_cg) and callable(capi.run_implicit_cg)
    section = hdr[hdr.index("Implicit-feedback ALS by conjugate gradient"):]
    for step in ("J0.", "J1.", "J2.", "J3.", "J4.", "J5."):
        assert step in section, step
    assert hdr.index("ALS by conjugate gradient: a fixed") < hdr.index("Implicit-feedback ALS by conjugate gradient")


def test_icg_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    s = C.c_int()
    assert h.mf_plan_set_implicit_cg(None, 1) == capi.MF_ERR_ARGUMENT and h.mf_plan_get_implicit_cg(None, C.byref(s)) == capi.MF_ERR_ARGUMENT
    for steps in (-1, 257, -2 ** 31, 2 ** 31 - 1):
        assert h.mf_plan_set_implicit_cg(fake, steps) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    run = h.mf_backend_run_implicit_cg
    ok = (C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, 40.0, 3, 0)

    def with_(at, v):
        return ok[:at] + (v,) + ok[at + 1:]
    badbox = capi.Bounds(1.0, 0.0, -1)
    for args in (with_(0, None), with_(2, None), with_(3, None), with_(5, -0.5), with_(6, float("nan")), with_(7, C.byref(badbox)),
                 with_(9, -1.0), with_(9, float("inf")), with_(10, -1), with_(10, 257)):
        assert run(*args) == capi.MF_ERR_ARGUMENT, args
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


def _cli(capi, path, cwd=None, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, cwd=cwd, env=dict(clean, **env))


@pytest.mark.parametrize("env,word", [(dict(MATFACT_SOLVER="als", MATFACT_IMPLICIT="40", MATFACT_IMPLICIT_CG=v),
                                       b"MATFACT_IMPLICIT_CG: expected a whole number from 1 to 256.") for v in BAD_STEPS] + [
    (dict(MATFACT_IMPLICIT_CG="3"), b"MATFACT_IMPLICIT_CG needs MATFACT_IMPLICIT."),
    (dict(MATFACT_IMPLICIT_CG="3", MATFACT_SOLVER="als", MATFACT_LAMBDA="0.1"), b"MATFACT_IMPLICIT_CG needs MATFACT_IMPLICIT."),
    (dict(MATFACT_IMPLICIT_CG="3", MATFACT_SOLVER="als,count"), b"MATFACT_IMPLICIT_CG needs MATFACT_IMPLICIT."),
    # what was refused before stays refused, with its message
    (dict(MATFACT_IMPLICIT_CG="3", MATFACT_SOLVER="als", MATFACT_IMPLICIT="40", MATFACT_ALS_CG="3"),
     b"MATFACT_ALS_CG cannot be combined with MATFACT_IMPLICIT: the implicit solve is the direct one."),
    (dict(MATFACT_IMPLICIT_CG="3", MATFACT_SOLVER="als", MATFACT_IMPLICIT="1,2"), b"MATFACT_IMPLICIT: expected conf, a number >= 0."),
], ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())) if isinstance(e, dict) else None)
def test_cli_icg_refusals_die_with_empty_stdout(capi, env, word, tmp_path):
    r = _cli(capi, os.path.join(tmp_path, "no-such-file.in"), cwd=tmp_path, **env)
    assert r.returncode == 255 and r.stdout == b"" and r.stderr.strip().endswith(word), r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    assert not os.listdir(tmp_path)


def test_cli_icg_accepts_its_value_and_then_reads_the_input(capi, tmp_path):
    for v in ("1", "3", "256", "+7", " 12"):
        r = _cli(capi, os.path.join(tmp_path, "no-such-file.in"), cwd=tmp_path, MATFACT_IMPLICIT="40", MATFACT_SOLVER="als",
                 MATFACT_LAMBDA="0.05", MATFACT_IMPLICIT_CG=v)
        assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_" not in r.stderr, r   # the parser's message: the options passed


# ---- the definition is the mathematics: J0-J5 in exact rational arithmetic
def exact_icg(y, a, e, S, ridge, x0, steps):
    """J0-J4 of one row in fractions.Fraction: the x after 0, 1, .. steps steps (a row that left at J4a repeats its x)"""
    K = len(x0)

    def A_times(v):
        t = [sum(yn[k] * v[k] for k in range(K)) for yn in y]
        return [sum(e[n] * t[n] * y[n][k] for n in range(len(y))) + sum(S[k][j] * v[j] for j in range(K)) + ridge * v[k] for k in range(K)]
    x = list(x0)
    t = [sum(yn[k] * x[k] for k in range(K)) for yn in y]
    d = [a[n] * (1 + e[n]) - e[n] * t[n] for n in range(len(y))]
    r = [sum(d[n] * y[n][k] for n in range(len(y))) - sum(S[k][j] * x[j] for j in range(K)) - ridge * x[k] for k in range(K)]
    p, rs = list(r), sum(v * v for v in r)
    xs = [list(x)]
    for _ in range(steps):
        if rs != 0:
            q = A_times(p)
            pq = sum(u * v for u, v in zip(p, q))
            assert pq > 0
            alpha = rs / pq
            x = [u + alpha * v for u, v in zip(x, p)]
            r = [u - alpha * v for u, v in zip(r, q)]
            rn = sum(v * v for v in r)
            p = [u + (rn / rs) * v for u, v in zip(r, p)]
            rs = rn
        xs.append(list(x))
    return xs


def exact_solve(A, b):
    """Gaussian elimination in Fractions (A positive definite: no pivoting needed)"""
    n = len(b)
    M = [list(A[i]) + [b[i]] for i in range(n)]
    for j in range(n):
        for i in range(j + 1, n):
            f = M[i][j] / M[j][j]
            M[i] = [u - f * v for u, v in zip(M[i], M[j])]
    x = [Fraction(0)] * n
    for i in reversed(range(n)):
        x[i] = (M[i][n] - sum(M[i][j] * x[j] for j in range(i + 1, n))) / M[i][i]
    return x


def twin_instance(K, weighted):
    """5 users x 6 items of small whole numbers and halves, user 2 without entries"""
    rng = np.random.default_rng(60 + K)
    U, I = 5, 6
    mask = rng.random((U, I)) < 0.5
    mask[2] = False
    mask[0, :2] = True
    row, col = np.nonzero(mask)
    Y, X0 = rng.integers(-2, 3, (I, K)).astype(np.float64), rng.integers(-3, 4, (U, K)) / 2.0
    X0[2, 0] = 1.5
    val = rng.integers(1, 6, len(row)).astype(np.float64)
    w = rng.integers(1, 4, len(row)) / 2.0 if weighted else None
    return U, I, row, col, val, w, Y, X0


def twin_row(inst, u, conf, ridge, steps):
    """row u of the instance in exact arithmetic: (the x after 0 .. steps steps, A, b of the dense system over ALL items --
    c = 1 + e on the observed pairs and 1 elsewhere, the preference a there and 0 elsewhere)"""
    F = Fraction
    U, I, row, col, val, w, Y, X0 = inst
    K = Y.shape[1]
    Yf = [[F(float(v)) for v in r] for r in Y]
    S = [[sum(Yf[i][k] * Yf[i][j] for i in range(I)) for j in range(K)] for k in range(K)]
    at = np.flatnonzero(row == u)
    items = [int(col[n]) for n in at]
    a = [F(float(val[n])) for n in at]
    e = [conf * (F(float(w[n])) if w is not None else 1) for n in at]
    xs = exact_icg([Yf[i] for i in items], a, e, S, ridge, [F(float(v)) for v in X0[u]], steps)
    c = {i: 1 + e[n] for n, i in enumerate(items)}
    A = [[sum(c.get(i, F(1)) * Yf[i][k] * Yf[i][j] for i in range(I)) + (ridge if k == j else 0) for j in range(K)] for k in range(K)]
    b = [sum(c[i] * a[n] * Yf[i][k] for n, i in enumerate(items)) for k in range(K)]
    return xs, A, b


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("K", [3, 4])
def test_exact_arithmetic_twin_reaches_the_all_pairs_solution(K, weighted):
    """after K steps J0-J5 in exact arithmetic give the exact solution of (S + sum_n e_n y_n y_n^T + ridge I) x = sum_n ac_n y_n
    over ALL pairs -- the dense normal equations of Hu, Koren and Volinsky --, the cold row exactly 0, and the row's quadratic
    x^T A x / 2 - b^T x never increases from step to step.  The numpy model, the same steps in float64, lands within 1e-9 of
    it (whole numbers, a condition number of a few tens: about six orders above its rounding)"""
    inst = twin_instance(K, weighted)
    U, I, row, col, val, w, Y, X0 = inst
    conf, ridge = Fraction(3), Fraction(1, 2)
    model, counts = IcgModel(U, I, row, col, val, w).solve(1, X0, Y, float(ridge), float(conf), K)
    assert counts == (U, 0, 0)
    moved = 0
    for u in range(U):
        xs, A, b = twin_row(inst, u, conf, ridge, K)
        exact = exact_solve(A, b)
        assert xs[K] == exact, u
        if not (row == u).any():
            assert all(v == 0 for v in xs[K]) and any(v != 0 for v in xs[0])

        def quad(x):
            return sum(x[k] * sum(A[k][j] * x[j] for j in range(K)) for k in range(K)) / 2 - sum(b[k] * x[k] for k in range(K))
        f = [quad(x) for x in xs]
        assert all(n <= m for m, n in zip(f, f[1:])), (u, [float(v) for v in f])
        moved += f[K] < f[0]
        assert np.abs(model[u] - np.array([float(v) for v in exact])).max() <= 1e-9 * max(1.0, max(abs(float(v)) for v in exact)), u
    assert moved == U


@functools.lru_cache(maxsize=None)
def inst30_runs():
    """inst30-40-10-2-10 from the reference initialisation, lambda 0.05 / 0.3, conf 40: the generations of 5 iterations at
    steps 1, 3 and 10, and the direct solve's"""
    import recommender_system_amd as rs
    capi = rs.capi
    inst = capi.parse_file(golden_in("inst30-40-10-2-10"))
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    m = IcgModel(inst.users, inst.items, inst.row, inst.col, inst.val)
    direct = ImplicitModel(inst.users, inst.items, inst.row, inst.col, inst.val)
    gens = {}
    for steps in (1, 3, 10, "direct"):
        g = [(L0, R0)]
        for _ in range(5):
            g.append(direct.iteration(*g[-1], LAM, 40.0)[:2] if steps == "direct" else m.iteration(*g[-1], LAM, 40.0, steps)[:2])
        gens[steps] = g
    return inst, direct, gens


@pytest.mark.parametrize("steps", [1, 3, 10])
def test_the_models_objective_decreases_on_inst30(steps):
    """ImplicitModel.objective -- the all-pairs objective both solves minimise row by row -- decreases strictly over 5
    iterations.  At 10 = K steps every row is, in exact arithmetic, the direct solve's: the two series agree to about 1e-4
    relative (1e-3 asserted: CG's rounding on systems whose condition conf = 40 sets, not the solve's backward error)"""
    inst, direct, gens = inst30_runs()
    obj = [direct.objective(L, R, LAM, 40.0) for L, R in gens[steps]]
    print("objective at steps %d:" % steps, " ".join("%.17g" % o for o in obj))
    assert len(obj) == 6 and all(b < a for a, b in zip(obj, obj[1:])), obj
    if steps == 10:
        want = [direct.objective(L, R, LAM, 40.0) for L, R in gens["direct"]]
        rel = [abs(a - b) / b for a, b in zip(obj, want)]
        print("relative to the direct solve:", " ".join("%.3g" % v for v in rel))
        assert max(rel) <= 1e-3, rel


def fused_s_times(Sf, v):
    """S v as fused multiply-adds: the rational S(k, j) * v[j] + sx[k] rounded once per j"""
    out = np.empty_like(v)
    for b in range(v.shape[0]):
        for k in range(v.shape[1]):
            s = 0.0
            for j in range(v.shape[1]):
                s = float(Fraction(float(Sf[k, j])) * Fraction(float(v[b, j])) + Fraction(s))
            out[b, k] = s
    return out


def test_model_guards_against_silent_contraction():
    """a fused sum in the S v chain changes sx on every pattern the GPU tests use, and the change reaches the stored rows (at
    conf = 40 the entry sums are some hundred times sx and the subtraction rounds most of it away: a few elements per row)"""
    K = 10
    reached = {}
    for pat_name in ("pair", "skewed", "wide"):
        pat = pattern(pat_name)
        L0, R0, val, _ = cls_signed(4000 + K, pat, K)
        Sf = full(gram(R0), K)
        assert_same_bits(s_times(Sf, L0[:1]), np.array([[sum_serial(Sf[k] * L0[0]) for k in range(K)]]), "the helper")
        assert differs(s_times(Sf, L0[:6]), fused_s_times(Sf, L0[:6])) > 0.2, pat_name
        # six rows through the whole solve, their lengths kept: one without entries and the first five of two or more
        rows = sides(pat.users, pat.items, pat.row, pat.col)[1]
        pick = np.concatenate([np.flatnonzero(rows.cnt == 0)[:1], np.flatnonzero(rows.cnt >= 2)[:5]])
        sel = np.isin(pat.row, pick)
        sub = IcgModel(pat.users, pat.items, pat.row[sel], pat.col[sel], val[sel])
        for conf in (1.0, 40.0):
            plain = sub.solve(1, L0, R0, LAM_U, conf, 3)[0]
            fused = sub.solve(1, L0, R0, LAM_U, conf, 3, sv=lambda S, v: fused_s_times(S, v) if len(v) <= 8 else s_times(S, v))[0]
            reached[(pat_name, conf)] = differs(plain[pick], fused[pick])
    print("stored elements a fused S v changes:", reached)
    # (the picked rows of `skewed` have some 630 entries each: at conf 40 their entry sums drown sx entirely)
    assert all(v > 0.3 for (_, conf), v in reached.items() if conf == 1.0) and reached[("pair", 40.0)] > 0.0, reached


def sum_serial(terms):
    s = 0.0
    for t in terms:
        s = s + float(t)
    return s


# ---- ISA
needs_isa = pytest.mark.skipif(not isa.have_tools() or not os.path.exists(isa.DEFAULT_LIB),
                               reason="needs llvm-objdump/llvm-readelf/c++filt and the built library")


@needs_isa
def test_isa_of_the_icg_instances():
    kernels = {n: b for n, b in isa.disassemble().items() if "mf::als_icg_kernel<" in n}
    meta = {n: m for n, m in isa.metadata().items() if "mf::als_icg_kernel<" in n}
    want = ["<%d, 1, true>" % K for K in FIXED_K] + ["<0, 1, true>", "<0, 1, false>"]
    assert len(kernels) == len(want) == len(meta) and all(any(w in n for n in kernels) for w in want), sorted(kernels)
    for name, body in kernels.items():
        ops = set(isa.split(i)[0] for i in body)
        assert "v_mul_f64" in ops and "v_add_f64" in ops, name
        assert not [i for i in body if i.startswith("v_mfma")], name
        # The correctly rounded `/` of alpha and of beta is the one place with fused operations: hipcc expands it to
        # v_rcp_f64, five Newton steps (v_fma_f64 x 3, v_fmac_f64 x 2), v_div_fmas_f64, v_div_fixup_f64.  Outside these two
        # expansions there is no fused multiply-add, and inside them no more than the five.
        outside, windows, inside = [], [], None
        for i in body:
            op = isa.split(i)[0]
            if op.startswith("v_rcp_f64"):
                assert inside is None, name
                inside = []
            elif re.match(r"v_(fma|fmac|mad|pk_fma)_f64", op):
                (outside if inside is None else inside).append(op)
            elif op == "v_div_fixup_f64":
                windows.append(inside)
                inside = None
        assert not outside and inside is None, (name, outside[:3])
        assert [sorted(w) for w in windows] == [["v_fma_f64"] * 3 + ["v_fmac_f64_e32"] * 2] * 2, (name, windows)
        dma = [i for i in body if i.startswith("global_load_lds_dwordx4")]
        assert bool(dma) == (", true>" in name), (name, len(dma))
        assert any(i.startswith("global_load_dwordx4") for i in body), name     # S: one 16-byte load per row and lane
    for name, m in meta.items():
        assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0 and m[".sgpr_spill_count"] == 0, (name, m)
    square = [n for n in isa.metadata() if "mf::gram_square_kernel" in n]
    assert len(square) == 1
    body = isa.disassemble()[square[0]]
    assert not [i for i in body if re.match(r"v_(add|mul|fma|fmac)_f64", i)], "the copy has no arithmetic"


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def device(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.fixture
def switches(monkeypatch):
    """No switch from the caller's environment; the test sets its own."""
    for k in SWITCHES + ("MF_ALS_FORM", "MF_ALS_CG_FORM"):
        monkeypatch.delenv(k, raising=False)

    def set_all(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_all


def icg_plan(capi, pat, K, val, conf, steps, lam=LAM, weight=None, **kw):
    plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val, weight=weight, **kw)
    try:
        plan.set_regularization(*lam)
        plan.set_confidence(conf)
        plan.set_implicit_cg(steps)
        plan.set_als("implicit")
    except BaseException:
        plan.close()
        raise
    return plan


def check_form(plan, form, conf, steps, K, forced=True):
    desc = plan.describe()
    assert " als=implicit conf=%.17g implicit_cg=%d als_cg_form=%s(chunk=%d)" % (conf, steps, form, chunk_of(K)) in desc, desc
    assert " als_form=" not in desc and " als_cg=" not in desc, desc
    assert ("MF_ALS_CG_FORM=%s" % form in desc) == forced, desc


def hand_iteration(plan, where, want=None):
    plan.als_solve("users", "current")
    cu = plan.als_info("users")
    plan.als_solve("items", "next")
    ci = plan.als_info("items")
    plan.flip()
    if want is not None:
        assert (cu, ci) == tuple(want), (where, cu, ci, want)
    return cu, ci


def check_against(plan, where, want):
    """one hand-driven iteration of `plan` (factors uploaded) against (L1, R1, cu, ci)"""
    hand_iteration(plan, where, want[2:])
    L, R = plan.download()
    assert_same_bits(L, want[0], where + ": L")
    assert_same_bits(R, want[1], where + ": R")
    return L, R


@gpu
@pytest.mark.parametrize("pat_name,K", [(p, K) for p in ("pair", "skewed") for K in ALL_K] + [("long-items", K) for K in (1, 3, 10, 17, 30)])
def test_both_sides_in_every_form(device, switches, pat_name, K):
    capi = device
    conf, weighted = _variant(pat_name, K)
    for steps in (1, 3):
        x = expected(pat_name, K, conf, weighted, steps)
        assert x.cu == (x.pat.users, 0, 0) and x.ci == (x.pat.items, 0, 0)
        for form in forms_of(K):
            switches({"MF_ALS_CG_FORM": form})
            plan = icg_plan(capi, x.pat, K, x.val, conf, steps, weight=x.w)
            try:
                where = "%s K=%d conf=%g %s steps=%d [%s]" % (pat_name, K, conf, "weighted" if weighted else "unweighted", steps, form)
                check_form(plan, form, conf, steps, K)
                assert plan.als() == "implicit" and plan.implicit_cg() == steps and plan.als_cg() == 0 and plan.als_info("users") == (0, 0, 0)
                plan.upload(x.L0, x.R0)
                check_against(plan, where, (x.L1, x.R1, x.cu, x.ci))
            finally:
                plan.close()
    assert differs(expected(pat_name, K, conf, weighted, 1).L1, expected(pat_name, K, conf, weighted, 3).L1) > 0.2 or K == 1


@gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("conf", CONFS)
@pytest.mark.parametrize("K", [10, 17])
def test_every_confidence_weighted_and_not(device, switches, K, conf, weighted):
    capi = device
    x = expected("pair", K, conf, weighted, 3)
    if conf == 0.0:   # e = 0 everywhere: the weights drop out
        assert_same_bits(x.L1, expected("pair", K, conf, not weighted, 3).L1, "conf 0: the weights play no part")
    else:
        assert differs(x.L1, expected("pair", K, 0.0, weighted, 3).L1) > 0.5
        assert differs(x.L1, expected("pair", K, conf, not weighted, 3).L1) > 0.5
    for form in forms_of(K):
        switches({"MF_ALS_CG_FORM": form})
        plan = icg_plan(capi, x.pat, K, x.val, conf, 3, weight=x.w)
        try:
            plan.upload(x.L0, x.R0)
            check_against(plan, "K=%d conf=%g weighted=%d [%s]" % (K, conf, weighted, form), (x.L1, x.R1, x.cu, x.ci))
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("K", [10, 16, 17])
def test_row_lengths(device, switches, K):
    """one fixed, one even and one odd K on the `wide` pattern, whose users and items have 0 .. 34, 63, 64 and 65 entries: 0, 1,
    chunk - 1, chunk, chunk + 1 and 2 chunk + 1 of the one chunk these K have, 16.  The row of 0 entries is solved and counted
    as solved; kept_empty is 0"""
    capi = device
    pat = pattern("wide")
    chunk = chunk_of(K)
    assert chunk == 16 and {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1} <= set(pat.ulen[:38]) and pat.ulen[:38].tolist() == pat.ilen[65:103].tolist()
    L0, R0, val, _ = cls_signed(4100 + K, pat, K)
    m = IcgModel(pat.users, pat.items, pat.row, pat.col, val)
    for steps in (1, 3):
        want = m.iteration(L0, R0, LAM, 40.0, steps)
        assert want[2] == (pat.users, 0, 0) and want[3] == (pat.items, 0, 0)
        assert differs(want[0][pat.ulen == 0], L0[pat.ulen == 0]) == 1.0      # a cold row moves: towards 0
        for form in forms_of(K):
            switches({"MF_ALS_CG_FORM": form})
            plan = icg_plan(capi, pat, K, val, 40.0, steps)
            try:
                plan.upload(L0, R0)
                check_against(plan, "wide K=%d steps=%d [%s]" % (K, steps, form), want)
            finally:
                plan.close()


def planted_instance(K, users=3):
    """every user rated all K items, R = 2 I, conf = 1, lambda = 0: S = 4 I, the row's matrix is S + 4 I = 8 I and its right-hand
    side 2 * 2 a = 4 a; with a = 2 x* the solution is x* in whole numbers, and every operation on the way is exact"""
    rng = np.random.default_rng(700 + K)
    xs = rng.integers(-3, 4, (users, K)).astype(np.float64)
    xs[:, 0] = np.arange(1, users + 1)
    row, col = np.repeat(np.arange(users), K), np.tile(np.arange(K), users)
    return Pattern("planted", users, K, row, col), 2.0 * np.eye(K), xs, (2.0 * xs).ravel()


@pytest.mark.parametrize("K", [1, 2, 3, 7, 16])
def test_planted_integers_come_back_after_one_step(K):
    pat, Y, xs, a = planted_instance(K)
    m = IcgModel(pat.users, pat.items, pat.row, pat.col, a)
    calls = []

    def counting(y, a, e, v, residual):
        calls.append(residual)
        return entry_pass(y, a, e, v, residual)
    got = m.solve(1, np.zeros((3, K)), Y, 0.0, 1.0, (1, 2, 5), passes=counting)
    for s in (1, 2, 5):
        assert_same_bits(got[s][0], xs, "K=%d steps=%d" % (K, s))
        assert got[s][1] == (3, 0, 0)
    assert calls == [True, False]                        # the residual and step 1: steps 2 .. 5 leave at rs == 0.0
    calls.clear()
    m.solve(1, xs, Y, 0.0, 1.0, 5, passes=counting)       # planted at the solution: the residual alone
    assert calls == [True]


@gpu
@pytest.mark.parametrize("K", [1, 2, 3, 7, 16])
def test_planted_integers_and_the_exit_at_a_zero_residual(device, switches, K):
    """x0 = 0: one step returns the planted whole numbers and steps 2 .. 5 leave at J4a; x0 = the solution: step 1 leaves there
    and the row stored is x0, projected"""
    capi = device
    pat, Y, xs, a = planted_instance(K)
    m = IcgModel(pat.users, pat.items, pat.row, pat.col, a)
    box = (-2.0, 2.0, K)
    clamped, counts = m.solve(1, xs, Y, 0.0, 1.0, 3, box=box)
    assert_same_bits(clamped, np.clip(xs, -2.0, 2.0), "the model stores x0 projected")
    assert counts == (3, 0, 0) and differs(clamped, xs) > 0
    for form in forms_of(K):
        switches({"MF_ALS_CG_FORM": form})
        for steps in (1, 2, 5):
            plan = icg_plan(capi, pat, K, a, 1.0, steps, (0.0, 0.0))
            try:
                plan.upload(np.zeros((3, K)), Y)
                plan.als_solve("users")
                assert plan.als_info("users") == (3, 0, 0)
                plan.flip()
                assert_same_bits(plan.download()[0], xs, "K=%d steps=%d [%s]" % (K, steps, form))
                plan.set_bounds("users", *box)
                plan.upload(xs, Y)
                plan.als_solve("users")
                assert plan.als_info("users") == (3, 0, 0)
                plan.flip()
                assert_same_bits(plan.download()[0], clamped, "K=%d steps=%d [%s]: x0 projected" % (K, steps, form))
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("K", [10, 17])
def test_rows_that_are_not_positive_definite(device, switches, K):
    """Y and X_old scaled by 2^-500 at lambda 0: the products of S and of pq underflow, pq == 0.0 while rs != 0.0, every row
    with entries keeps its bits and is counted.  And a NaN in Y: every row keeps its bits"""
    capi = device
    x = expected("pair", K, 40.0, False, 3)
    pat = x.pat
    tiny = 2.0 ** -500
    Ls, Rs = x.L0 * tiny, x.R0 * tiny
    lam = (0.0, 0.0)
    Rn = x.R0.copy()
    Rn[7, 0] = np.nan
    for steps in (1, 3):
        L1, cu = x.model.solve(1, Ls, Rs, 0.0, 40.0, steps)
        # a row whose ratings are all zero, or that has none, has g = 0 and so rs == 0.0: it leaves at J4a and stores x0
        busy = np.bincount(pat.row, weights=(x.val != 0), minlength=pat.users) > 0
        assert cu == (pat.users - int(busy.sum()), 0, int(busy.sum())) and busy.sum() > 600
        assert_same_bits(L1, Ls, "the model keeps X_old's bits")
        Ln, cn = x.model.solve(1, x.L0, Rn, LAM_U, 40.0, steps)
        assert cn == (0, 0, pat.users)
        assert_same_bits(Ln, x.L0, "the model keeps X_old under a NaN")
        for form in forms_of(K):
            switches({"MF_ALS_CG_FORM": form})
            plan = icg_plan(capi, pat, K, x.val, 40.0, steps, lam)
            try:
                where = "K=%d steps=%d [%s]" % (K, steps, form)
                plan.upload(Ls, Rs)
                plan.als_solve("users", "current")
                assert plan.als_info("users") == cu, where
                plan.flip()
                assert_same_bits(plan.download(want_r=False)[0], L1, where + ": underflow")
                plan.set_regularization(*LAM)
                plan.upload(x.L0, Rn)
                plan.als_solve("users", "current")
                assert plan.als_info("users") == cn, where
                plan.flip()
                assert_same_bits(plan.download(want_r=False)[0], x.L0, where + ": NaN in Y")
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("lo", [0.0, 0.125])
@pytest.mark.parametrize("K", [10, 17])
def test_with_a_box(device, switches, K, lo):
    """lo = 0 and [lo, 0.5] on a weighted plan: all columns of the users, the first K - 1 of the items"""
    capi = device
    pat = pattern("pair")
    L0, R0, val, _ = cls_signed(4400 + K, pat, K)
    w = plain_weights(3, pat.nnz)
    m = IcgModel(pat.users, pat.items, pat.row, pat.col, val, w)
    boxes = ((lo, np.inf if lo == 0.0 else 0.5, K), (lo, 0.5, K - 1))
    want = m.iteration(L0, R0, LAM, 40.0, 3, boxes)
    L1 = want[0]
    assert 0.01 < (L1 == lo).mean() < 0.9 and (L1 >= lo).all() and (want[1][:, K - 1] < lo).any()
    for form in forms_of(K):
        switches({"MF_ALS_CG_FORM": form})
        plan = icg_plan(capi, pat, K, val, 40.0, 3, weight=w)
        try:
            plan.set_bounds("users", boxes[0][0], boxes[0][1])
            plan.set_bounds("items", lo, 0.5, K - 1)
            plan.upload(L0, R0)
            check_against(plan, "box lo=%g K=%d [%s]" % (lo, K, form), want)
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("K", [10, 30, 17])
def test_the_padding_of_a_row_is_never_read_or_written(device, switches, K):
    """caller-owned buffers at the library's pitch, NaN in every padding element: a padding element read would reach every
    sum it touches, one written would show"""
    from test_stream_order import padded, poisoned_plan
    import torch
    capi = device
    conf, weighted = _variant("pair", K)
    x = expected("pair", K, conf, weighted, 3)
    pat = x.pat
    for form in forms_of(K):
        switches({"MF_ALS_CG_FORM": form})
        plan, bufs = poisoned_plan(capi, pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val, weight=x.w)
        try:
            assert bufs.ld > K or K % 2
            plan.set_regularization(*LAM)
            plan.set_confidence(conf)
            plan.set_implicit_cg(3)
            plan.set_als("implicit")
            plan.upload(x.L0, x.R0)
            hand_iteration(plan, form, (x.cu, x.ci))
            plan.synchronize()
            torch.cuda.synchronize()
            cur = [t.cpu().numpy() for t in bufs.cur(plan)]
            assert_same_bits(cur[0], padded(x.L1, bufs.ld), form + ": L and its padding")
            assert_same_bits(cur[1], padded(x.R1, bufs.ld), form + ": R and its padding")
            assert all(bool(torch.isnan(t[:, K:]).all()) for t in bufs.l + bufs.r)
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("K", [10, 64, 17])
def test_split_side_launches_twice(device, switches, K):
    """MF_SWEEP_LONG=128 on `skewed`: both sides of an even K have extreme rows, so launch_als launches twice into the same
    three counters; the expected bits are the model's, which knows no split"""
    capi = device
    conf, weighted = _variant("skewed", K)
    x = expected("skewed", K, conf, weighted, 3)
    pat = x.pat
    switches({"MF_SWEEP_LONG": "128"})
    plan = icg_plan(capi, pat, K, x.val, conf, 3, weight=x.w)
    try:
        n = long_rows(plan.describe())
        if K % 2 == 0:
            assert n == (int((pat.ilen >= 128).sum()), int((pat.ulen >= 128).sum())) and 0 < n[0] < pat.items and 0 < n[1] < pat.users, plan.describe()
        else:
            assert n is None, plan.describe()      # an odd K has no split
        plan.upload(x.L0, x.R0)
        check_against(plan, "split K=%d, hand-driven" % K, (x.L1, x.R1, x.cu, x.ci))
        plan.upload(x.L0, x.R0)
        plan.iterate(1)
        assert (plan.als_info("users"), plan.als_info("items")) == (x.cu, x.ci)
        L, R = plan.download()
        assert_same_bits(L, x.L1, "split K=%d, iterate: L" % K)
        assert_same_bits(R, x.R1, "split K=%d, iterate: R" % K)
    finally:
        plan.close()


@gpu
def test_setter_states(device, switches):
    """steps 0 is the library of before; the steps under kind off or ridge change nothing there; the refusals of the implicit
    kind stay with the steps on, and those of mf_plan_set_als_cg stay as they are"""
    from test_als import expected as direct_expected
    from test_implicit import expected as implicit_expected, implicit_plan
    capi = device
    K = 30
    x = implicit_expected("pair", K, 40.0, False)
    switches({})

    def refused(call, status=None):
        with pytest.raises(capi.HipBackendError) as err:
            call()
        assert err.value.status == (capi.MF_ERR_UNSUPPORTED if status is None else status)
    untold = implicit_plan(capi, x.pat, K, x.val, 40.0)
    plan = icg_plan(capi, x.pat, K, x.val, 40.0, 3)
    try:
        assert "implicit_cg=3" in plan.describe() and untold.implicit_cg() == 0
        plan.upload(x.L0, x.R0)
        plan.iterate(1)                      # a CG iteration in between: what it leaves must not show afterwards
        plan.set_implicit_cg(0)
        assert plan.implicit_cg() == 0 and plan.describe() == untold.describe() and " als_form=wg(chunk=16)" in plan.describe()
        assert "implicit_cg" not in plan.describe()
        plan.upload(x.L0, x.R0)
        check_against(plan, "steps 0", (x.L1, x.R1, x.cu, x.ci))
        assert differs(expected("pair", K, 40.0, False, 3).L1, x.L1) > 0.5
        # argument errors change nothing
        plan.set_implicit_cg(5)
        for steps in (-1, 257):
            refused(lambda: plan.set_implicit_cg(steps), capi.MF_ERR_ARGUMENT)
        assert plan.implicit_cg() == 5
        # mf_plan_set_als_cg with the implicit kind stays refused, in both orders
        refused(lambda: plan.set_als_cg(3))
        assert plan.als_cg() == 0 and plan.als() == "implicit"
        plan.set_als("off")
        assert " als" not in plan.describe()                    # the kind is off: nothing to describe
        plan.set_als_cg(3)
        refused(lambda: plan.set_als("implicit"))
        plan.set_als_cg(0)
        # under ridge the steps are not read: bits and text of the direct ridge solve
        d = direct_expected("pair", K, "ridge")
        plan.set_als("ridge")
        told = plan.describe()
        plan.set_implicit_cg(0)
        assert plan.describe() == told and "implicit_cg" not in told and " als=ridge als_form=" in told
        plan.set_implicit_cg(7)
        assert plan.describe() == told
        plan.upload(d.L0, d.R0)
        check_against(plan, "ridge with the steps set", (d.L1, d.R1, d.cu, d.ci))
        # the refusals of the implicit kind, the steps on
        plan.set_als("implicit")
        plan.set_implicit_cg(3)
        plan.upload(x.L0, x.R0)
        plan.set_frozen_columns(3, -1)
        for call in (lambda: plan.als_solve("users"), lambda: plan.iterate(1), lambda: plan.iterate_monitored(2)):
            refused(call)
        plan.set_frozen_columns(-1, -1)
        refused(lambda: plan.set_momentum(0.9, 0.0))
        refused(lambda: plan.set_adaptive("items", "adam", 0.03))
        plan.set_als("off")
        plan.set_momentum(0.5, 0.0)
        refused(lambda: plan.set_als("implicit"))
        assert plan.als() == "off" and plan.implicit_cg() == 3
    finally:
        plan.close()
        untold.close()
    pat, L0, R0, val, alpha = _small(K=129)
    plan = capi.Plan(pat.users, pat.items, 129, alpha, pat.row, pat.col, val)
    try:
        plan.set_implicit_cg(3)              # accepted under any kind at any K: it is read under the implicit kind alone
        refused(lambda: plan.set_als("implicit"))
        assert plan.als() == "off"
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_iterate_is_the_hand_driven_sequence(device, switches, weighted):
    capi = device
    pat, L0, R0, val, alpha = _small()
    w = plain_weights(17, pat.nnz) if weighted else None
    m = IcgModel(pat.users, pat.items, pat.row, pat.col, val, w)
    gens = [(L0, R0)]
    for _ in range(3):
        gens.append(m.iteration(*gens[-1], LAM, 40.0, 3)[:2])
    jacobi = m.solve(0, R0, L0, LAM_I, 40.0, 3)[0]   # the item solve from the OLD L
    assert differs(jacobi, gens[1][1]) > 0.9
    switches({})
    plan, hand = icg_plan(capi, pat, 10, val, 40.0, 3, weight=w), icg_plan(capi, pat, 10, val, 40.0, 3, weight=w)
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
        # the steps are read at every launch
        plan.set_implicit_cg(1)
        plan.upload(L0, R0)
        plan.iterate(1)
        want = m.iteration(L0, R0, LAM, 40.0, 1)
        assert_same_bits(plan.download()[0], want[0], "steps changed between two calls: L")
        assert_same_bits(plan.download()[1], want[1], "steps changed between two calls: R")
        # level 1
        inst = capi.Instance(3, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
        L, R = L0.copy(), R0.copy()
        best = capi.backend_run_implicit_cg(inst, L, R, 3, 40.0, weight=w, lambda_users=LAM_U, lambda_items=LAM_I)
        assert_same_bits(L, gens[3][0], "mf_backend_run_implicit_cg: L")
        assert_same_bits(R, gens[3][1], "mf_backend_run_implicit_cg: R")
        assert np.array_equal(best, hand.recommend())
        # ... and with steps 0 it is mf_backend_run_implicit
        La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
        b0 = capi.backend_run_implicit_cg(inst, La, Ra, 0, 40.0, weight=w, lambda_users=LAM_U, lambda_items=LAM_I)
        b1 = capi.backend_run_implicit(inst, Lb, Rb, 40.0, weight=w, lambda_users=LAM_U, lambda_items=LAM_I)
        assert_same_bits(La, Lb, "steps 0: L of mf_backend_run_implicit")
        assert_same_bits(Ra, Rb, "steps 0: R of mf_backend_run_implicit")
        assert np.array_equal(b0, b1) and differs(La, L) > 0.5
    finally:
        plan.close()
        hand.close()


@gpu
def test_monitored_loop(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    plan, hand = icg_plan(capi, pat, 10, val, 40.0, 3), icg_plan(capi, pat, 10, val, 40.0, 3)
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
    finally:
        plan.close()
        hand.close()


@gpu
def test_cli_implicit_cg(device, orc, switches):
    """MATFACT_SOLVER=als MATFACT_IMPLICIT=40 MATFACT_IMPLICIT_CG=3 MATFACT_LAMBDA: stdout is the plan session's recommendation
    after the file's iterations, stderr the one objective line"""
    capi = device
    path = golden_in("inst30-40-10-2-10")
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    switches({})
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_confidence(40.0)
        plan.set_implicit_cg(3)
        plan.set_als("implicit")
        plan.upload(L0, R0)
        plan.iterate(inst.iters)
        best = plan.recommend()
        all_sq, observed, _ = plan.implicit_objective()
        us, its = plan.penalty()
    finally:
        plan.close()
    r = _cli(capi, path, MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05,0.3", MATFACT_IMPLICIT="40", MATFACT_IMPLICIT_CG="3")
    assert r.returncode == 0 and r.stdout == orc.format_out(best).encode(), r
    lines = r.stderr.decode().strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("implicit conf 40 "), r.stderr
    words = lines[0].split()
    got = {words[i]: float(words[i + 1]) for i in range(1, len(words), 2)}
    assert got == dict(conf=40.0, all_sq=all_sq, observed=observed, users_sq=us, items_sq=its,
                       objective=((all_sq + observed) + LAM_U * us) + LAM_I * its), (got, all_sq, observed)
    direct = _cli(capi, path, MATFACT_SOLVER="als", MATFACT_LAMBDA="0.05,0.3", MATFACT_IMPLICIT="40")
    assert direct.returncode == 0 and direct.stderr != r.stderr      # another solve: another objective


@gpu
def test_user_solve_on_a_shard_and_item_solve_refused(device, switches):
    capi = device
    K, cut = 30, 333
    x = expected("pair", K, 40.0, False, 3)
    pat = x.pat
    switches({})
    lo = pat.row < cut
    for sel, begin, count in ((lo, 0, cut), (~lo, cut, pat.users - cut)):
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row[sel], pat.col[sel], x.val[sel], user_begin=begin, user_count=count)
        try:
            plan.set_regularization(*LAM)
            plan.set_confidence(40.0)
            plan.set_implicit_cg(3)
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
def test_implicit_cg_behind_a_closed_gate(device, switches, gate):
    """mf_plan_als_solve under the implicit kind with the steps on -- its Gram launches, the copy into the square and the solve --
    and such an mf_plan_iterate on a busy caller-owned stream return before the gate opens and give the model's bits
    afterwards: nothing of them ran ahead of the gate, or it would have read the poison"""
    from test_stream_order import behind_gate, padded, poisoned_plan
    capi = device
    K = 30
    x = expected("pair", K, 40.0, False, 3)
    pat = x.pat
    L2, R2 = x.model.iteration(x.L1, x.R1, LAM, 40.0, 3)[:2]
    switches({})
    plan, bufs = poisoned_plan(capi, pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_confidence(40.0)
        plan.set_implicit_cg(3)
        plan.set_als("implicit")
        plan.set_stream(gate.s.cuda_stream)

        def solves(plan, bufs):
            plan.als_solve("users", "current")
            plan.als_solve("items", "next")
            plan.flip()
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, solves, "implicit als_solve x 2 under CG")
        assert_same_bits(got[0], padded(x.L1, bufs.ld), "als_solve: L")
        assert_same_bits(got[1], padded(x.R1, bufs.ld), "als_solve: R")
        assert plan.als_info("users") == x.cu and plan.als_info("items") == x.ci
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, lambda plan, bufs: plan.iterate(2), "iterate(2) under the implicit kind with CG")
        assert_same_bits(got[0], padded(L2, bufs.ld), "iterate(2): L")
        assert_same_bits(got[1], padded(R2, bufs.ld), "iterate(2): R")
        assert_same_bits(got[2], padded(x.L1, bufs.ld), "iterate(2): L of the generation before")
        assert_same_bits(got[3], padded(x.R1, bufs.ld), "iterate(2): R of the generation before")
    finally:
        plan.set_stream(None)
        plan.close()


@gpu
@pytest.mark.parametrize("steps", [1, 3, 10])
def test_objective_decreases_on_inst30_and_equals_the_model(device, switches, steps):
    capi = device
    inst, direct, gens = inst30_runs()
    switches({})
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_confidence(40.0)
        plan.set_implicit_cg(steps)
        plan.set_als("implicit")
        plan.upload(*gens[steps][0])
        obj = []
        for it in range(6):
            if it:
                plan.iterate(1)
            L, R = plan.download()
            assert_same_bits(L, gens[steps][it][0], "L after %d" % it)
            assert_same_bits(R, gens[steps][it][1], "R after %d" % it)
            all_sq, observed, count = plan.implicit_objective()
            assert_same_bits(np.array([all_sq, observed]), np.array(direct.objective_parts(L, R, 40.0)), "objective after %d" % it)
            us, its = plan.penalty()
            obj.append(all_sq + observed + LAM_U * us + LAM_I * its)
            assert plan.als_info("users")[1:] == (0, 0) and plan.als_info("items")[1:] == (0, 0)
        print("objective at steps %d:" % steps, " ".join("%.17g" % o for o in obj))
        assert all(b < a for a, b in zip(obj, obj[1:])), obj
    finally:
        plan.close()
