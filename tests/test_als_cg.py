"""ALS by conjugate gradient (mf_plan_set_als_cg, mf_plan_get_als_cg, mf_backend_run_als_cg, MATFACT_ALS_CG).

The definition is include/matfact_hip.h's steps C0-C5; the model below performs them literally with elementwise numpy
operations -- products formed as arrays of their own, serial sums through ufunc.accumulate, which applies its operation element
after element -- so that nothing fuses and nothing is re-ordered.  Rows of equal length are taken together (the operations of a
row do not depend on its neighbours).  Every GPU result is compared with it bit for bit (assert_same_bits), the three row
counters included.
"""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, golden_in, random_instance
from test_stream_order import gate  # noqa: F401  (the calibrated gate of the stream-order tests, once for this module)
from test_als import (KINDS, LAM, NO_BOX, AlsModel, _cli, als_plan, hand_iteration, sides)
from test_als import expected as direct_expected
from test_regularised import LAM_I, LAM_U, _small, differs
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits, cls_signed, pattern
from test_weighted import plain_weights

gpu = pytest.mark.gpu

MAX_STEPS, MAX_K = 256, 256
FIXED_K = (10, 20, 30, 50, 100, 128, 256)          # the compile-time K of the sweeps
FORMS = ("fixed", "dma", "general")                # MF_ALS_CG_FORM, in the order of the rule's enum
# every compile-time K of als_cg_fn and both ends of the range of K of its run-time instances (2 .. 128 and 130 .. 256 under the
# LDS-DMA gather, 1 .. 128 and 129 .. 256 through registers): tests/test_als_edges.py checks this list against the table
ALL_K = (1, 2, 3, 10, 16, 17, 20, 30, 50, 64, 100, 127, 128, 129, 130, 200, 255, 256)
CG_SYMBOLS = ("mf_plan_set_als_cg", "mf_plan_get_als_cg", "mf_backend_run_als_cg")
LDS_PER_CU = 160 * 1024


def takes(form, K):
    return 1 <= K <= MAX_K and (K in FIXED_K if form == "fixed" else K % 2 == 0 if form == "dma" else True)


def forms_of(K):
    return [f for f in FORMS if takes(f, K)]


def chunk_of(K):
    """entries per gather chunk: 16, or what a sixth of a CU's LDS holds behind the two vectors, at least 12"""
    pieces = (K + 1) // 2
    row, head = 16 * (pieces | 1), 2 * ((2 * pieces * 8 + 255) // 256 * 256)
    return rule_chunk(head, row)


def rule_chunk(head, row):
    budget = LDS_PER_CU // 6
    if head + 16 * row <= budget:
        return 16
    return max(12, (budget - head) // row if budget > head else 0)


# ------------------------------------------------------------------------------------------------ the model
def serial_last(terms, axis):
    """0.0 + t[0] + t[1] + ... along `axis`, one rounded addition after the other"""
    zero = np.zeros_like(np.take(terms, [0], axis=axis))
    return np.take(np.add.accumulate(np.concatenate([zero, terms], axis=axis), axis=axis), -1, axis=axis)


def dot(u, v):
    """dot(u, v) of the definition along the last axis: the products are an array of their own"""
    return serial_last(u * v, -1)


def row_product(y, a, w, v, residual):
    """one pass: sum_n e_n * y_n, n ascending, e_n = a_n - dot(y_n, v) (residual) or dot(y_n, v), times w_n when weighted.
    y (B, c, K), a / w (B, c), v (B, K) -> (B, K)"""
    t = dot(y, v[:, None, :])
    e = a - t if residual else t
    if w is not None:
        e = e * w
    return serial_last(e[:, :, None] * y, 1)


def cg_side(rows, val, wgt, X_old, Y, lam, kind, steps, frozen=-1, box=NO_BOX, pass_fn=row_product, observer=None):
    """C0-C5 for every row of a side.  `steps`: a number, or a tuple of numbers -- then {steps: result}: the row after s steps
    is an intermediate of every longer run.  result = (X_new, (solved, kept_empty, kept_not_pd)).  `observer`: called as
    observer("pq", s, rows, pq) with the divisors of C4e and observer("rs", s, rows, rs) with those of C4f at step s, for the
    rows that divide there; it only looks"""
    wanted = (steps,) if isinstance(steps, int) else tuple(steps)
    K = X_old.shape[1]
    lo, hi, ncols = box
    out = {s: [X_old.copy(), 0] for s in wanted}   # X_new, kept_not_pd
    todo = np.flatnonzero(rows.cnt > 0)

    def finish(s, R, x, notpd):
        head = x[:, :ncols]
        head = np.where(head < lo, lo, head)
        head = np.where(head > hi, hi, head)
        xx = np.concatenate([head, x[:, ncols:]], axis=1)
        if frozen >= 0:
            xx[:, frozen] = X_old[R, frozen]
        out[s][0][R[~notpd]] = xx[~notpd]
        out[s][1] += int(notpd.sum())

    with np.errstate(all="ignore"):
        for c in np.unique(rows.cnt[todo]):
            group = todo[rows.cnt[todo] == c]
            per = max(1, (1 << 21) // (int(c) * K))
            for b0 in range(0, len(group), per):
                R = group[b0:b0 + per]
                e = rows.ptr[R][:, None] + np.arange(int(c))[None, :]
                y, a = Y[rows.idx[e]], val[rows.pos[e]]
                w = None if wgt is None else wgt[rows.pos[e]]
                ridge = (lam * rows.cnt[R].astype(np.float64) if kind == "ridge-count" else np.full(len(R), float(lam)))[:, None]
                x = X_old[R].copy()                                                  # C0
                g = pass_fn(y, a, w, x, True)                                        # C1, C2
                r = g - (ridge * x)
                if frozen >= 0:
                    r[:, frozen] = 0.0
                p, rs = r.copy(), dot(r, r)                                          # C3
                active, notpd = np.ones(len(R), bool), np.zeros(len(R), bool)
                for s in range(1, max(wanted) + 1):                                  # C4
                    active &= ~(rs == 0.0)                                           # a: a NaN is not equal and goes on
                    i = np.flatnonzero(active)
                    if len(i):
                        q = pass_fn(y[i], None, None if w is None else w[i], p[i], False)   # b, c
                        q = q + (ridge[i] * p[i])
                        if frozen >= 0:
                            q[:, frozen] = 0.0
                        pq = dot(p[i], q)                                            # d
                        bad = ~(pq > 0.0)
                        notpd[i[bad]], active[i[bad]] = True, False
                        i, q, pq = i[~bad], q[~bad], pq[~bad]
                        if observer is not None:
                            observer("pq", s, R[i].copy(), pq.copy())
                            observer("rs", s, R[i].copy(), rs[i].copy())
                        alpha = (rs[i] / pq)[:, None]                                # e
                        x[i] = x[i] + (alpha * p[i])
                        r[i] = r[i] - (alpha * q)
                        rn = dot(r[i], r[i])                                         # f
                        beta = (rn / rs[i])[:, None]
                        p[i] = r[i] + (beta * p[i])
                        rs[i] = rn
                    if s in out:
                        finish(s, R, x, notpd)
    res = {s: (X, (len(todo) - bad, rows.nrows - len(todo), bad)) for s, (X, bad) in out.items()}
    return res[steps] if isinstance(steps, int) else res


class CgModel:
    def __init__(self, users, items, row, col, val, weight=None):
        self.side = sides(users, items, row, col)
        self.val = np.asarray(val, np.float64)
        self.wgt = None if weight is None else np.asarray(weight, np.float64)

    def solve(self, side, X_old, Y, lam, kind, steps, frozen=-1, box=NO_BOX, pass_fn=row_product, observer=None):
        return cg_side(self.side[side], self.val, self.wgt, X_old, Y, lam, kind, steps, frozen, box, pass_fn, observer)

    def iteration(self, L, R, lam, kind, steps, frozen=(-1, -1), box=(NO_BOX, NO_BOX)):
        """users against R, items against the NEW L: (L', R', users' counts, items' counts); lam, frozen, box as (users, items)"""
        L1, cu = self.solve(1, L, R, lam[0], kind, steps, frozen[0], box[0])
        R1, ci = self.solve(0, R, L1, lam[1], kind, steps, frozen[1], box[1])
        return L1, R1, cu, ci


@functools.lru_cache(maxsize=None)
def expected(pat_name, K, kind, steps):
    """Inputs of one (pattern, K) -- the signed class of the sweep tests -- and one model iteration at lambda 0.05 / 0.3,
    computed once and shared by the forms."""
    pat = pattern(pat_name)
    x = type("Expected", (), {})()
    x.pat, x.K, x.kind, x.steps = pat, K, kind, steps
    x.L0, x.R0, x.val, x.alpha = cls_signed(4000 + K, pat, K)
    x.model = CgModel(pat.users, pat.items, pat.row, pat.col, x.val)
    x.L1, x.cu = _user_solves(pat_name, K, kind)[steps]
    x.R1, x.ci = x.model.solve(0, x.R0, x.L1, LAM_I, kind, steps)
    return x


@functools.lru_cache(maxsize=None)
def _user_solves(pat_name, K, kind):
    """the users after 1 and after 3 steps from one run of the model"""
    pat = pattern(pat_name)
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    return CgModel(pat.users, pat.items, pat.row, pat.col, val).solve(1, L0, R0, LAM_U, kind, (1, 3))


def planted_instance(K, users=3):
    """every user rated all K items, R = 2 I: A = 4 I at lambda 0, b = 2 a holds multiples of 4, x* = a / 2 whole numbers"""
    rng = np.random.default_rng(700 + K)
    xs = rng.integers(-3, 4, (users, K)).astype(np.float64)
    xs[:, 0] = np.arange(1, users + 1)                  # no row is all zero: rs != 0.0 at x0 = 0
    row, col = np.repeat(np.arange(users), K), np.tile(np.arange(K), users)
    return Pattern("planted", users, K, row, col), 2.0 * np.eye(K), xs, (2.0 * xs).ravel()


def row_objective(y, a, w, ridge, x):
    """sum_n w_n (a_n - y_n . x)^2 + ridge |x|^2 of one row, exactly"""
    F = Fraction
    xs = [F(float(v)) for v in x]
    total = F(ridge) * sum(v * v for v in xs)
    for n in range(len(a)):
        d = F(float(a[n])) - sum(F(float(y[n, k])) * xs[k] for k in range(len(xs)))
        total += (F(float(w[n])) if w is not None else 1) * d * d
    return total


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("K", [1, 2, 3, 7, 16, 32])
def test_planted_integers_come_back_after_one_step(K):
    pat, Y, xs, a = planted_instance(K)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, a)
    x0 = np.zeros((3, K))
    for kind in KINDS:   # lambda = 0: both kinds add 0.0
        got = m.solve(1, x0, Y, 0.0, kind, (1, 2, 5))
        for s in (1, 2, 5):
            assert_same_bits(got[s][0], xs, "K=%d %s steps=%d" % (K, kind, s))
            assert got[s][1] == (3, 0, 0)
    # step 2 leaves at rs == 0.0: one step from the solution the residual is exactly zero, and so the model takes no pass
    calls = []

    def counting(y, a, w, v, residual):
        calls.append(len(y))
        return row_product(y, a, w, v, residual)
    m.solve(1, x0, Y, 0.0, "ridge", 5, pass_fn=counting)
    assert calls == [3, 3]                               # the residual and step 1, nothing for steps 2 .. 5
    calls.clear()
    m.solve(1, xs, Y, 0.0, "ridge", 5, pass_fn=counting)   # planted at the solution: the residual alone
    assert calls == [3]


def test_exact_rational_objective_never_increases():
    """K = 6, rows of 9 .. 20 entries with small half-integer factors: the exact objective of the model's x after 0, 1, 2, 3
    steps is non-increasing on every row of both sides, weighted and not, under both kinds -- checked here, the model alone"""
    rng = np.random.default_rng(41)
    users, items, K = 12, 9, 6
    mask = rng.random((users, items)) < 0.85
    mask[:, 0] = mask[0, :] = True
    row, col = np.nonzero(mask)
    pat = Pattern("dense", users, items, row, col)
    L0, R0 = rng.integers(-4, 5, (users, K)) / 4.0, rng.integers(-4, 5, (items, K)) / 4.0 + np.eye(items, K)
    val = rng.integers(-6, 7, pat.nnz) / 2.0
    for w in (None, rng.integers(1, 5, pat.nnz) / 2.0):
        m = CgModel(users, items, pat.row, pat.col, val, w)
        for kind in KINDS:
            for side, X, Y, lam in ((1, L0, R0, LAM_U), (0, R0, L0, LAM_I)):
                rows = m.side[side]
                xs = m.solve(side, X, Y, lam, kind, (1, 2, 3))
                xs[0] = (X, None)
                assert xs[3][1] == (rows.nrows, 0, 0)
                strictly = 0
                for r in range(rows.nrows):
                    e = np.arange(rows.ptr[r], rows.ptr[r + 1])
                    ridge = lam * float(len(e)) if kind == "ridge-count" else lam
                    obj = [row_objective(Y[rows.idx[e]], val[rows.pos[e]], None if w is None else w[rows.pos[e]], ridge, xs[s][0][r])
                           for s in range(4)]
                    assert all(b <= a for a, b in zip(obj, obj[1:])), (kind, side, r, [float(o) for o in obj])
                    strictly += obj[3] < obj[0]
                assert strictly == rows.nrows


@pytest.mark.parametrize("f", [0, 2, 4])
def test_frozen_column_gives_the_bits_of_the_reduced_system(f):
    """small whole numbers: a_n - xf * y_n[f] and the products of C1 are exact, and behind C1 the frozen column of p is 0.0"""
    pat = _small(K=5)[0]
    rng = np.random.default_rng(50 + f)
    L0, R0 = rng.integers(-3, 4, (pat.users, 5)).astype(np.float64), rng.integers(-3, 4, (pat.items, 5)).astype(np.float64)
    val = rng.integers(-9, 10, pat.nnz).astype(np.float64)
    keep = [k for k in range(5) if k != f]
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    shifted = CgModel(pat.users, pat.items, pat.row, pat.col, val - (L0[pat.row, f] * R0[pat.col, f]))
    for kind in KINDS:
        for steps in (1, 3):
            full, counts = m.solve(1, L0, R0, LAM_U, kind, steps, frozen=f)
            reduced, rcounts = shifted.solve(1, L0[:, keep], np.ascontiguousarray(R0[:, keep]), LAM_U, kind, steps)
            assert counts == rcounts and counts[0] > 50
            assert_same_bits(full[:, keep], reduced, "frozen %d %s: the other columns" % (f, kind))
            assert_same_bits(full[:, f], L0[:, f], "frozen %d %s: the frozen column" % (f, kind))
            free, _ = m.solve(1, L0, R0, LAM_U, kind, steps)
            assert differs(free[:, keep], full[:, keep]) > 0.5


def fused_sum(e, y):
    """sum_n e_n * y_n[k] as fused multiply-adds: the rational e_n * y_n[k] + g rounded once per entry"""
    out = []
    for k in range(y.shape[1]):
        g = 0.0
        for n in range(y.shape[0]):
            g = float(Fraction(float(e[n])) * Fraction(float(y[n, k])) + Fraction(g))
        out.append(g)
    return np.array(out)


@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed", "wide"])
def test_model_guards_against_silent_contraction(pat_name):
    """the residual's sum through fused multiply-adds differs from the definition on every pattern the GPU tests use (rows of
    at least two entries: the first product is added to 0.0), and a one-ulp change of a product reaches the stored rows"""
    K = 10
    pat = pattern(pat_name)
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    for side, X, Y in ((1, L0, R0), (0, R0, L0)):
        rows = m.side[side]
        seen = 0
        for r in [r for r in np.argsort(rows.cnt, kind="stable") if rows.cnt[r] >= 2][:6]:   # the six shortest rows of two entries or more
            e = np.arange(rows.ptr[r], rows.ptr[r + 1])
            y, a = Y[rows.idx[e]], val[rows.pos[e]]
            d = a - dot(y, X[r][None, :])
            g = row_product(y[None], a[None], None, X[r][None], True)[0]
            assert_same_bits(g, serial_last(d[:, None] * y, 0), "the helper")
            seen += differs(g, fused_sum(d, y)) > 0.0
        assert seen >= 3, (pat_name, side, seen)

    def mutant(y, a, w, v, residual):   # one ulp in the sum of every pass
        return row_product(y, a, w, v, residual) * (1.0 + 2.0 ** -52)
    for steps in (1, 3):
        assert differs(m.solve(1, L0, R0, LAM_U, "ridge", steps, pass_fn=mutant)[0], m.solve(1, L0, R0, LAM_U, "ridge", steps)[0]) > 0.3


def test_cg_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in CG_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MF_ALS_CG_MAX_STEPS 256\b", hdr) and re.search(r"#define MF_ALS_CG_MAX_K +256\b", hdr)
    for name in ("set_als_cg", "als_cg"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_als_cg) and callable(capi.run_als_cg)
    for step in ("C0.", "C1.", "C2.", "C3.", "C4.", "C5."):
        assert step in hdr[hdr.index("ALS by conjugate gradient"):], step


def test_cg_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    s = C.c_int()
    assert h.mf_plan_set_als_cg(None, 1) == capi.MF_ERR_ARGUMENT and h.mf_plan_get_als_cg(None, C.byref(s)) == capi.MF_ERR_ARGUMENT
    for steps in (-1, 257, -2 ** 31, 2 ** 31 - 1):
        assert h.mf_plan_set_als_cg(fake, steps) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    run = h.mf_backend_run_als_cg
    ok = (C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, 1, 3, 0)

    def with_(at, v):
        return ok[:at] + (v,) + ok[at + 1:]
    badbox = capi.Bounds(1.0, 0.0, -1)
    for args in (with_(0, None), with_(2, None), with_(3, None), with_(5, -0.5), with_(6, float("nan")), with_(7, C.byref(badbox)),
                 with_(9, -1), with_(9, 3), with_(9, 4), with_(10, -1), with_(10, 257)):
        assert run(*args) == capi.MF_ERR_ARGUMENT, args
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


BAD_STEPS = ["", "0", "-1", "257", "3,", "3.5", "three", " 3x", "1e2", "0x10"]


@pytest.mark.parametrize("env", [dict(MATFACT_SOLVER="als", MATFACT_ALS_CG=v) for v in BAD_STEPS] +
                         [dict(MATFACT_ALS_CG="3"), dict(MATFACT_ALS_CG="3", MATFACT_LAMBDA="0.1"),
                          dict(MATFACT_SOLVER="als", MATFACT_IMPLICIT="2", MATFACT_ALS_CG="3")],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_cg_refusals_die_with_empty_stdout(capi, env, tmp_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(clean, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_ALS_CG" in r.stderr, r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    if "MATFACT_SOLVER" not in env:
        assert b"needs MATFACT_SOLVER" in r.stderr
    elif "MATFACT_IMPLICIT" in env:
        assert b"cannot be combined with MATFACT_IMPLICIT" in r.stderr
    else:
        assert b"expected a whole number from 1 to 256" in r.stderr
    assert not os.listdir(tmp_path)


@pytest.fixture(scope="module")
def form_choices(tmp_path_factory):
    """what tests/als_cg_form_main.cpp prints: {(K, forced): form}, {(head, row): chunk} and {(kind, als_cg, implicit_cg): solver}"""
    exe = str(tmp_path_factory.mktemp("als_cg_form") / "als_cg_form_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "als_cg_form_main.cpp")])
    forms, chunks, solvers = {}, {}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        t = line.split()
        if t[0] == "form":
            forms[(int(t[1]), int(t[2]))] = (int(t[3]), [int(v) for v in t[4:]])
        elif t[0] == "chunk":
            chunks[(int(t[1]), int(t[2]))] = int(t[3])
        else:
            assert t[0] == "solver", line
            solvers[tuple(int(v) for v in t[1:4])] = tuple(int(v) for v in t[4:])
    return forms, chunks, solvers


def test_form_choice(form_choices):
    """the rule against its truth table, written out here: the forced form where it takes the K, otherwise the first of fixed,
    dma, general that does; and the chunk rule on a grid of geometries, the kernel's among them"""
    forms, chunks, _ = form_choices
    assert len(forms) == 258 * 6
    for (K, forced), (form, taken) in forms.items():
        assert taken == [int(takes(f, K)) for f in FORMS], K
        if 0 <= forced < 3 and takes(FORMS[forced], K):
            want = forced
        else:
            want = 0 if takes("fixed", K) else 1 if takes("dma", K) else 2      # no form takes K = 0 or 257: the setters refuse those
        assert form == want, (K, forced, form)
        assert not (1 <= K <= MAX_K) or takes(FORMS[form], K)
    seen = set()
    for (head, row), chunk in chunks.items():
        assert chunk == rule_chunk(head, row), (head, row)
        seen.add(chunk)
    assert {12, 13, 14, 15, 16} <= seen
    for K in range(1, MAX_K + 1):
        pieces = (K + 1) // 2
        assert (2 * ((16 * pieces + 255) // 256 * 256), 16 * (pieces | 1)) in chunks, K
    assert [chunk_of(K) for K in (1, 10, 30, 128, 129, 200, 255, 256)] == [16, 16, 16, 16, 16, 14, 12, 12]


def solver_of(kind, als_cg, implicit_cg):
    """which solve a launch runs, as (conjugate gradient?, implicit?, steps, widest K): the steps of mf_plan_set_als_cg come
    first and make it the explicit CG solve, K to 256; those of mf_plan_set_implicit_cg count under the implicit kind alone;
    otherwise the direct solve of the kind, K to 128"""
    if als_cg > 0:
        return (1, 0, als_cg, MAX_K)
    if kind == 4 and implicit_cg > 0:
        return (1, 1, implicit_cg, 128)
    return (0, int(kind == 4), 0, 128)


def test_solver_rule(form_choices, capi):
    """mf_sched::als_solver on every kind x als_cg x implicit_cg against the restatement above, and what the 16 lines come to"""
    solvers = form_choices[2]
    kinds = (capi.ALS_KINDS["off"], capi.ALS_KINDS["ridge"], capi.ALS_KINDS["ridge-count"], capi.ALS_KINDS["implicit"])
    assert kinds == (0, 1, 2, 4)
    assert sorted(solvers) == sorted((k, a, i) for k in kinds for a in (0, 3) for i in (0, 3)) and len(solvers) == 16
    for (kind, als_cg, implicit_cg), got in solvers.items():
        assert got == solver_of(kind, als_cg, implicit_cg), (kind, als_cg, implicit_cg)
    # the explicit kinds never read the implicit steps; the implicit kind without explicit steps does
    assert all(solvers[(k, 0, 3)] == solvers[(k, 0, 0)] == (0, 0, 0, 128) for k in (0, 1, 2))
    assert all(solvers[(k, 3, i)] == (1, 0, 3, 256) for k in kinds for i in (0, 3))
    assert solvers[(4, 0, 0)] == (0, 1, 0, 128) and solvers[(4, 0, 3)] == (1, 1, 3, 128)


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


def cg_plan(capi, pat, K, val, kind, steps, lam=LAM, weight=None, **kw):
    """the steps first: K may lie in 129 .. 256"""
    plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val, weight=weight, **kw)
    try:
        plan.set_regularization(*lam)
        plan.set_als_cg(steps)
        plan.set_als(kind)
    except BaseException:
        plan.close()
        raise
    return plan


def check_form(plan, form, kind, steps, K, forced=True):
    desc = plan.describe()
    assert " als=%s als_cg=%d als_cg_form=%s(chunk=%d)" % (kind, steps, form, chunk_of(K)) in desc and " als_form=" not in desc, desc
    assert ("MF_ALS_CG_FORM=%s" % form in desc) == forced, desc
    return desc


def check_against(plan, where, want):
    """one hand-driven iteration of `plan` (factors uploaded) against (L1, R1, cu, ci)"""
    hand_iteration(plan, where, want[2:])
    L, R = plan.download()
    assert_same_bits(L, want[0], where + ": L")
    assert_same_bits(R, want[1], where + ": R")
    return L, R


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", ALL_K)
@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed"])
def test_both_sides_in_every_form(device, switches, pat_name, K, kind):
    capi = device
    for steps in (1, 3):
        x = expected(pat_name, K, kind, steps)
        assert x.cu[1] == int((x.pat.ulen == 0).sum()) and x.ci[1] == int((x.pat.ilen == 0).sum()) and x.cu[2] == 0 and x.ci[2] == 0
        for form in forms_of(K):
            switches({"MF_ALS_CG_FORM": form})
            plan = cg_plan(capi, x.pat, K, x.val, kind, steps)
            try:
                where = "%s K=%d %s steps=%d [%s]" % (pat_name, K, kind, steps, form)
                check_form(plan, form, kind, steps, K)
                assert plan.als() == kind and plan.als_cg() == steps and plan.als_info("users") == (0, 0, 0)
                plan.upload(x.L0, x.R0)
                check_against(plan, where, (x.L1, x.R1, x.cu, x.ci))
            finally:
                plan.close()
    assert differs(expected(pat_name, K, kind, 1).L1, expected(pat_name, K, kind, 3).L1) > 0.2 or K == 1


@gpu
def test_default_form_is_by_k_and_a_form_without_the_k_is_the_rule_s(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    for K, form in ((1, "general"), (2, "dma"), (10, "fixed"), (17, "general"), (64, "dma"), (100, "fixed"), (255, "general"), (256, "fixed")):
        plan = cg_plan(capi, pat, K, val, "ridge", 2)
        try:
            check_form(plan, form, "ridge", 2, K, forced=False)
        finally:
            plan.close()
    for forced, K, form in (("fixed", 12, "dma"), ("dma", 11, "general"), ("fixed", 11, "general"), ("nonsense", 10, "fixed")):
        switches({"MF_ALS_CG_FORM": forced})
        plan = cg_plan(capi, pat, K, val, "ridge-count", 2)
        try:
            assert " als=ridge-count als_cg=2 als_cg_form=%s(" % form in plan.describe()
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("lam", [LAM, (0.0, 0.0)], ids=["lambda", "lambda0"])
@pytest.mark.parametrize("K", [10, 30])
def test_row_lengths(device, switches, K, lam):
    """the `wide` pattern has users and items of 0 .. 34, 63, 64 and 65 entries: 0, 1, chunk - 1, chunk, chunk + 1 and
    2 chunk + 1 of the one chunk size these K have in every form, 16.  At lambda 0 the rows shorter than K are singular: kept or
    solved as the model decides"""
    capi = device
    pat = pattern("wide")
    chunk = chunk_of(K)
    assert chunk == 16 and {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1} <= set(pat.ulen[:38]) and pat.ulen[:38].tolist() == pat.ilen[65:103].tolist()
    L0, R0, val, _ = cls_signed(4100 + K, pat, K)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    for kind in KINDS:
        for steps in (1, 3):
            want = m.iteration(L0, R0, lam, kind, steps)
            # with the ridge pq > 0 on every row; at lambda 0 a row shorter than K has converged after as many steps as it has
            # entries, p is rounding noise from then on and the sign of pq is the model's to say
            assert want[2][1] > 0 and (lam != LAM or (want[2][2] == 0 and want[3][2] == 0))
            for form in forms_of(K):
                switches({"MF_ALS_CG_FORM": form})
                plan = cg_plan(capi, pat, K, val, kind, steps, lam)
                try:
                    plan.upload(L0, R0)
                    check_against(plan, "wide K=%d %s steps=%d [%s] lambda %s" % (K, kind, steps, form, lam), want)
                finally:
                    plan.close()


@gpu
@pytest.mark.parametrize("K", [1, 2, 3, 7, 16, 32])
def test_planted_integers_and_the_exit_at_a_zero_residual(device, switches, K):
    """x0 = 0: one step returns the planted whole numbers and steps 2 .. 5 leave at rs == 0.0; x0 = the solution: step 1 leaves
    there and the row stored is x0, projected"""
    capi = device
    pat, Y, xs, a = planted_instance(K)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, a)
    box = (-2.0, 2.0, K)
    clamped, counts = m.solve(1, xs, Y, 0.0, "ridge", 3, box=box)
    assert_same_bits(clamped, np.clip(xs, -2.0, 2.0), "the model stores x0 projected")
    assert counts == (3, 0, 0) and differs(clamped, xs) > 0
    for form in forms_of(K):
        switches({"MF_ALS_CG_FORM": form})
        for steps in (1, 2, 5):
            plan = cg_plan(capi, pat, K, a, "ridge", steps, (0.0, 0.0))
            try:
                plan.upload(np.zeros((3, K)), Y)
                plan.als_solve("users")
                assert plan.als_info("users") == (3, 0, 0)
                plan.flip()
                assert_same_bits(plan.download()[0], xs, "K=%d steps=%d [%s]" % (K, steps, form))
                plan.set_bounds("users", *box)      # planted at the solution, under a box
                plan.upload(xs, Y)
                plan.als_solve("users")
                assert plan.als_info("users") == (3, 0, 0)
                plan.flip()
                assert_same_bits(plan.download()[0], clamped, "K=%d steps=%d [%s]: x0 projected" % (K, steps, form))
            finally:
                plan.close()


def _not_pd_inputs(K):
    """the `wide` pattern at lambda 0 with negative weights on some users' entries (pq < 0), a NaN planted in one item's row
    (rs and pq are NaN) and zero rows among the items: a user who rated only those has A = 0 and so pq = 0, but also r = 0 --
    by the definition the row leaves at C4a before pq is looked at, stores x0 and counts as solved; the model decides"""
    pat = pattern("wide")
    L0, R0, val, _ = cls_signed(4200 + K, pat, K)
    R0 = R0.copy()
    zero_items = np.flatnonzero(np.isin(np.arange(pat.items), pat.col[np.isin(pat.row, [1, 2, 3])]))   # all items of users 1 .. 3
    R0[zero_items] = 0.0
    R0[40, K // 2] = np.nan
    w = plain_weights(4200, pat.nnz)
    w[np.isin(pat.row, [20, 25, 30])] = -1.5
    return pat, L0, R0, val, w


@gpu
@pytest.mark.parametrize("K", [10, 30])
def test_rows_that_are_not_positive_definite(device, switches, K):
    capi = device
    pat, L0, R0, val, w = _not_pd_inputs(K)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val, w)
    lam = (0.0, 0.0)
    for kind in KINDS:
        for steps in (1, 3):
            want = m.iteration(L0, R0, lam, kind, steps)
            L1, cu = want[0], want[2]
            nan_users = np.unique(pat.row[pat.col == 40])
            bad = np.unique(np.concatenate([[1, 2, 3, 20, 25, 30], nan_users]))
            assert len(nan_users) > 0 and cu[2] >= 3 + len(set(nan_users) - {20, 25, 30}) and cu[1] > 0 and want[3][2] > 0
            assert_same_bits(L1[bad], L0[bad], "the model keeps X_old's bits")
            assert sum(cu) == pat.users and sum(want[3]) == pat.items
            for form in forms_of(K):
                switches({"MF_ALS_CG_FORM": form})
                plan = cg_plan(capi, pat, K, val, kind, steps, lam, weight=w)
                try:
                    where = "K=%d %s steps=%d [%s]" % (K, kind, steps, form)
                    plan.upload(L0, R0)
                    L, R = check_against(plan, where, want)
                    assert_same_bits(L[bad], L0[bad], where + ": a kept row holds X_old's bits")
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
    frozen, box = (K - 1, 0), ((-0.5, 0.5, -1 if K == 10 else K - 1), (-0.75, 0.4, max(K // 2, 1)))
    mbox = tuple((lo, hi, K if c < 0 else c) for lo, hi, c in box)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val, w)
    plain = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    steps = 3
    for kind in KINDS:
        want = m.iteration(L0, R0, LAM, kind, steps, frozen, mbox)
        wantp = plain.iteration(L0, R0, LAM, kind, steps, frozen, mbox)
        # the inputs do their job: the box cuts some elements and leaves others, and the weights show in those it leaves
        assert 0.002 < (np.abs(want[0][:, :K - 1]) == 0.5).mean() < 0.9 and differs(want[0], wantp[0]) > 0.1 and differs(want[1], wantp[1]) > 0.1
        assert_same_bits(want[0][:, K - 1], L0[:, K - 1], "frozen users' column")
        assert_same_bits(want[1][:, 0], R0[:, 0], "frozen items' column")
        for form in forms_of(K):
            switches({"MF_ALS_CG_FORM": form})
            for weight, exp in ((w, want), (np.ones(pat.nnz), wantp), (None, wantp)):
                plan = cg_plan(capi, pat, K, val, kind, steps, weight=weight)
                try:
                    where = "%s K=%d %s [%s] %s" % (pat_name, K, kind, form, "unweighted" if weight is None else "w[0]=%g" % weight[0])
                    plan.set_frozen_columns(*frozen)
                    plan.set_bounds("users", *box[0])
                    plan.set_bounds("items", *box[1])
                    plan.upload(L0, R0)
                    check_against(plan, where, exp)
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
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    want = m.iteration(L0, R0, LAM, "ridge", 3, (K - 1, K - 2))
    assert (want[0][:, K - 1] == 1.0).all() and (want[1][:, K - 2] == 1.0).all() and differs(want[0][:, K - 2], L0[:, K - 2]) > 0.9
    for form in forms_of(K):
        switches({"MF_ALS_CG_FORM": form})
        plan = cg_plan(capi, pat, K, val, "ridge", 3)
        try:
            plan.set_frozen_columns(K - 1, K - 2)
            plan.upload(L0, R0)
            check_against(plan, form, want)
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_steps_zero_is_the_library_of_before(device, switches, kind):
    """set_als_cg(3) then set_als_cg(0): the bits of test_als's expected values, its description, and K = 129 refused"""
    capi = device
    K = 30
    x = direct_expected("pair", K, kind)
    switches({})
    untold = als_plan(capi, x.pat, K, x.val, kind)
    plan = cg_plan(capi, x.pat, K, x.val, kind, 3)
    try:
        plan.upload(x.L0, x.R0)
        plan.iterate(1)                      # a CG iteration in between: what it leaves must not show afterwards
        plan.set_als_cg(0)
        assert plan.als_cg() == 0 and untold.als_cg() == 0 and plan.describe() == untold.describe() and " als_form=wg(chunk=16)" in plan.describe()
        assert "als_cg" not in plan.describe()
        plan.upload(x.L0, x.R0)
        check_against(plan, "steps 0 %s" % kind, (x.L1, x.R1, x.cu, x.ci))
        assert differs(expected("pair", K, kind, 3).L1, x.L1) > 0.5
    finally:
        plan.close()
        untold.close()
    pat, L0, R0, val, alpha = _small(K=129)
    plan = capi.Plan(pat.users, pat.items, 129, alpha, pat.row, pat.col, val)
    try:
        before = plan.describe()
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_als(kind)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.als() == "off" and plan.describe() == before
    finally:
        plan.close()


@gpu
def test_state_errors_and_refusals(device, switches):
    """the refusals that need a live plan, and so a GPU: no factors, kind off, the implicit kind with CG in both orders, K = 257,
    steps = 0 while a kind is on at K = 200 -- each with nothing changed.  (Steps -1 and 257 are refused on a CPU above.)"""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})

    def refused(call, status=None):
        with pytest.raises(capi.HipBackendError) as err:
            call()
        assert err.value.status == (capi.MF_ERR_UNSUPPORTED if status is None else status)
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        assert plan.als_cg() == 0
        for steps in (-1, 257):
            refused(lambda: plan.set_als_cg(steps), capi.MF_ERR_ARGUMENT)
        plan.set_als_cg(256)
        assert plan.als_cg() == 256 and " als" not in plan.describe()      # the kind is off: nothing to describe
        plan.upload(L0, R0)
        refused(lambda: plan.als_solve("users"), capi.MF_ERR_STATE)         # kind off
        plan.set_als_cg(3)
        refused(lambda: plan.set_als("implicit"))                           # implicit second
        assert plan.als() == "off" and plan.als_cg() == 3
        plan.set_als_cg(0)
        plan.set_als("implicit")
        refused(lambda: plan.set_als_cg(3))                                 # CG second
        assert plan.als() == "implicit" and plan.als_cg() == 0 and "als_cg" not in plan.describe()
        plan.set_als_cg(0)
        plan.set_als("off")
        plan.set_als_cg(3)
        plan.set_momentum(0.0, 0.5)                                         # momentum and adaptive sides stay refused
        refused(lambda: plan.set_als("ridge"))
        plan.set_momentum(0.0, 0.0)
        plan.set_als("ridge")
        refused(lambda: plan.set_adaptive("users", "adam", 0.03))
    finally:
        plan.close()
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.set_als_cg(2)
        plan.set_als("ridge")
        refused(lambda: plan.als_solve("users"), capi.MF_ERR_STATE)         # no factors
    finally:
        plan.close()
    L257, R257 = np.zeros((pat.users, 257)), np.zeros((pat.items, 257))
    plan = capi.Plan(pat.users, pat.items, 257, alpha, pat.row, pat.col, val)
    try:
        refused(lambda: plan.set_als_cg(1))                                  # K = 257
        plan.set_als_cg(0)
        assert plan.als_cg() == 0
        refused(lambda: plan.set_als("ridge"))
        del L257, R257
    finally:
        plan.close()
    plan = capi.Plan(pat.users, pat.items, 200, alpha, pat.row, pat.col, val)
    try:
        refused(lambda: plan.set_als("ridge"))                              # a caller at K in 129 .. 256 sets the steps first
        plan.set_als_cg(4)
        plan.set_als("ridge")
        refused(lambda: plan.set_als_cg(0))                                 # steps = 0 while a kind is on at K = 200
        assert plan.als_cg() == 4 and plan.als() == "ridge"
        plan.set_als("off")
        plan.set_als_cg(0)
        assert plan.als_cg() == 0
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_iterate_is_the_hand_driven_sequence(device, switches, kind):
    capi = device
    pat, L0, R0, val, alpha = _small()
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    gens = [(L0, R0)]
    for _ in range(3):
        gens.append(m.iteration(*gens[-1], LAM, kind, 3)[:2])
    switches({})
    plan, hand = cg_plan(capi, pat, 10, val, kind, 3), cg_plan(capi, pat, 10, val, kind, 3)
    try:
        plan.upload(L0, R0)
        plan.iterate(3)
        hand.upload(L0, R0)
        for _ in range(3):
            hand_iteration(hand, "hand-driven")
        for got, name in ((plan.download(), "iterate"), (hand.download(), "hand-driven")):
            assert_same_bits(got[0], gens[3][0], name + ": L after three")
            assert_same_bits(got[1], gens[3][1], name + ": R after three")
        assert plan.als_info("users") == hand.als_info("users") and plan.als_info("items") == hand.als_info("items")
        # the steps are read at every launch
        plan.set_als_cg(1)
        plan.upload(L0, R0)
        plan.iterate(1)
        want = m.iteration(L0, R0, LAM, kind, 1)
        assert_same_bits(plan.download()[0], want[0], "steps changed between two calls: L")
        assert_same_bits(plan.download()[1], want[1], "steps changed between two calls: R")
    finally:
        plan.close()
        hand.close()


@gpu
def test_monitored_loop(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    plan, hand = cg_plan(capi, pat, 10, val, "ridge", 3), cg_plan(capi, pat, 10, val, "ridge", 3)
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
def test_backend_run_als_cg_equals_the_plan_session(device, switches, kind):
    capi = device
    pat, L0, R0, val, alpha = _small()
    inst = capi.Instance(5, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
    w = plain_weights(5, pat.nnz)
    box = (-0.4, 0.4)
    switches({})
    plan = cg_plan(capi, pat, 10, val, kind, 2, weight=w)
    try:
        plan.set_bounds("users", *box)
        plan.upload(L0, R0)
        plan.iterate(5)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    L, R = L0.copy(), R0.copy()
    best = capi.backend_run_als_cg(inst, L, R, 2, kind, bounds_users=box, weight=w, lambda_users=LAM_U, lambda_items=LAM_I)
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val, w)
    want = (L0, R0)
    for _ in range(5):
        want = m.iteration(*want, LAM, kind, 2, box=((box[0], box[1], 10), NO_BOX))[:2]
    assert_same_bits(L, want[0], "L against the model")
    assert_same_bits(R, want[1], "R against the model")
    # steps 0: mf_backend_run_als
    La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
    b0 = capi.backend_run_als_cg(inst, La, Ra, 0, kind, lambda_users=LAM_U, lambda_items=LAM_I)
    b1 = capi.backend_run_als(inst, Lb, Rb, kind, lambda_users=LAM_U, lambda_items=LAM_I)
    assert_same_bits(La, Lb, "steps 0: L of mf_backend_run_als")
    assert_same_bits(Ra, Rb, "steps 0: R of mf_backend_run_als")
    assert np.array_equal(b0, b1) and differs(La, L) > 0.5


@gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "inst0"])
def test_cli_solver_with_cg(device, orc, switches, name):
    """MATFACT_SOLVER=als[,count] MATFACT_ALS_CG=3: stdout is the plan session's recommendation after the file's iterations from
    the reference's initialisation, byte for byte"""
    capi = device
    path = golden_in(name)
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    switches({})

    def session(kind, steps, lam):
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
        try:
            plan.set_regularization(*lam)
            plan.set_als_cg(steps)
            plan.set_als(kind)
            plan.upload(L0, R0)
            plan.iterate(inst.iters)
            return orc.format_out(plan.recommend()).encode(), plan.download()
        finally:
            plan.close()
    for env, args in ((dict(MATFACT_SOLVER="als", MATFACT_ALS_CG="3", MATFACT_LAMBDA="0.05,0.3"), ("ridge", 3, LAM)),
                      (dict(MATFACT_SOLVER="als,count", MATFACT_ALS_CG="1", MATFACT_LAMBDA="0.1"), ("ridge-count", 1, (0.1, 0.1)))):
        r = _cli(capi, path, **env)
        out, (L, R) = session(*args)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == out, (env, r)
        m = CgModel(inst.users, inst.items, inst.row, inst.col, inst.val)
        want = (L0, R0)
        for _ in range(min(inst.iters, 4)):
            want = m.iteration(*want, args[2], args[0], args[1])[:2]
        if inst.iters <= 4:
            assert_same_bits(L, want[0], "the session against the model: L")
            assert_same_bits(R, want[1], "the session against the model: R")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_two_user_shards_on_one_gpu(device, switches, kind):
    """rows of L are private: each shard's user solve gives the single plan's rows; the item solve of a shard is refused"""
    capi = device
    K, cut = 30, 333
    x = expected("pair", K, kind, 3)
    pat = x.pat
    switches({})
    lo = pat.row < cut
    for sel, begin, count in ((lo, 0, cut), (~lo, cut, pat.users - cut)):
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row[sel], pat.col[sel], x.val[sel], user_begin=begin, user_count=count)
        try:
            plan.set_regularization(*LAM)
            plan.set_als_cg(3)
            plan.set_als(kind)
            plan.upload(x.L0[begin:begin + count], x.R0)
            plan.als_solve("users", "current")
            empty = int((pat.ulen[begin:begin + count] == 0).sum())
            assert plan.als_info("users") == (count - empty, empty, 0)
            for call in (lambda: plan.als_solve("items", "next"), lambda: plan.als_solve("items", "current"), lambda: plan.iterate(1)):
                with pytest.raises(capi.HipBackendError) as err:
                    call()
                assert err.value.status == capi.MF_ERR_UNSUPPORTED
            plan.flip()
            assert_same_bits(plan.download(want_r=False)[0], x.L1[begin:begin + count], "shard at %d" % begin)
        finally:
            plan.close()


@gpu
def test_cg_behind_a_closed_gate(device, switches, gate):
    """mf_plan_als_solve under CG and a CG mf_plan_iterate on a busy caller-owned stream return before the gate opens and give
    the model's bits afterwards (tests/test_stream_order.py has the instruments)"""
    from test_stream_order import behind_gate, padded, poisoned_plan
    capi = device
    K = 30
    x = expected("pair", K, "ridge", 3)
    pat = x.pat
    L2, R2 = x.model.iteration(x.L1, x.R1, LAM, "ridge", 3)[:2]
    switches({})
    plan, bufs = poisoned_plan(capi, pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_als_cg(3)
        plan.set_als("ridge")
        plan.set_stream(gate.s.cuda_stream)

        def solves(plan, bufs):
            plan.als_solve("users", "current")
            plan.als_solve("items", "next")
            plan.flip()
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, solves, "als_solve x 2 under CG")
        assert_same_bits(got[0], padded(x.L1, bufs.ld), "als_solve: L")
        assert_same_bits(got[1], padded(x.R1, bufs.ld), "als_solve: R")
        assert plan.als_info("users") == x.cu and plan.als_info("items") == x.ci
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, lambda plan, bufs: plan.iterate(2), "iterate(2) under CG")
        assert_same_bits(got[0], padded(L2, bufs.ld), "iterate(2): L")
        assert_same_bits(got[1], padded(R2, bufs.ld), "iterate(2): R")
        assert_same_bits(got[2], padded(x.L1, bufs.ld), "iterate(2): L of the generation before")
        assert_same_bits(got[3], padded(x.R1, bufs.ld), "iterate(2): R of the generation before")
    finally:
        plan.set_stream(None)
        plan.close()


def _objective_inputs():
    d = random_instance(11, 30, 40, 10, density=0.25)
    rng = np.random.default_rng(12)
    return d, rng.uniform(0, 1, (30, 10)), rng.uniform(0, 1, (40, 10))


def _objective(d, L, R, lam, kind):
    """loss + lambda * squares (the rows' squares times their counts under ridge-count) of these factors, in plain float64:
    the decrease per half-step is many orders above its rounding"""
    ulen, ilen = np.bincount(d["row"], minlength=30), np.bincount(d["col"], minlength=40)
    res = d["val"] - (L[d["row"]] * R[d["col"]]).sum(axis=1)
    ur, ir = (L * L).sum(axis=1), (R * R).sum(axis=1)
    if kind == "ridge-count":
        ur, ir = ur * ulen, ir * ilen
    return float((res * res).sum() + lam * (ur.sum() + ir.sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lam", [0.05, 1.0])
def test_the_model_s_objective_does_not_increase(lam, kind):
    """the inputs of the device test below: the model passes the same assertion on the CPU"""
    d, L, R = _objective_inputs()
    m = CgModel(30, 40, d["row"], d["col"], d["val"])
    obj = [_objective(d, L, R, lam, kind)]
    for _ in range(3):
        L, R = m.iteration(L, R, (lam, lam), kind, 3)[:2]
        obj.append(_objective(d, L, R, lam, kind))
    assert all(b <= a for a, b in zip(obj, obj[1:])) and obj[3] < 0.9 * obj[0], obj


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lam", [0.05, 1.0])
def test_objective_does_not_increase_on_the_device(device, switches, lam, kind):
    """30 x 40, K = 10, about a quarter dense: loss + lambda * penalty from the device's factors over three iterations at
    steps 3"""
    capi = device
    d, L, R = _objective_inputs()
    ulen, ilen = np.bincount(d["row"], minlength=30), np.bincount(d["col"], minlength=40)
    switches({})
    plan = capi.Plan(30, 40, 10, d["alpha"], d["row"], d["col"], d["val"])
    try:
        plan.set_regularization(lam)
        plan.set_als_cg(3)
        plan.set_als(kind)

        def objective():
            _, _, ur, ir = plan.penalty(rows=True)
            if kind == "ridge-count":
                ur, ir = ur * ulen, ir * ilen
            return plan.loss().sse + lam * (ur.sum() + ir.sum())
        plan.upload(L, R)
        obj = [objective()]
        for _ in range(3):
            plan.iterate(1)
            assert plan.als_info("users")[1:] == (0, 0) and plan.als_info("items")[1:] == (0, 0)
            obj.append(objective())
        print("objective:", " ".join("%.6g" % o for o in obj))
        assert len(obj) == 4 and all(b <= a for a, b in zip(obj, obj[1:])), obj
    finally:
        plan.close()
