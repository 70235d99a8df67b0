"""Box-constrained ALS (mf_plan_set_als_box, mf_plan_get_als_box, mf_backend_run_als_box, MATFACT_ALS_BOX; include/matfact_hip.h,
"Box-constrained ALS").

The model restates the definition operation by operation: steps 1-4 of a row are gram_rhs of tests/test_als.py (under the
implicit kind the chain from S, restated below), steps 5-6 and B0-B4 are box_rows below -- elementwise numpy operations over a
batch of rows, every product an array of its own, so nothing fuses and nothing is re-ordered.  Every comparison is bit for bit
(assert_same_bits: NaN as a class, everything else as uint64), the three row counters included.  No tolerance appears.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_in
from test_als import FORMS, KINDS, LAM, NO_BOX, AlsModel, forms_of, gram_rhs, plain_products, sides, triangle
from test_als_shards import normal_records, pitch_of
from test_implicit import ImplicitModel, gram
from test_regularised import LAM_I, LAM_U, _small, differs
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits
from test_weighted import plain_weights

import sys
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa  # noqa: E402

gpu = pytest.mark.gpu

BOX_SYMBOLS = ("mf_plan_set_als_box", "mf_plan_get_als_box", "mf_backend_run_als_box")
ALL_KINDS = KINDS + ("implicit",)
CONF = 3.0
SWEEPS = (1, 2, 7)
# by als_blocks: the first and the last K of every instance of the workgroup form (NB = 1, 2, 3), 64 / 65 where a lane takes its
# second element; of the one-wave form likewise
FORM_K = {"wg": (17, 64, 65, 88, 89, 124, 125, 128), "wave": (1, 2, 20, 21, 30, 31, 32)}
NONNEG = (0.0, np.inf)


# ------------------------------------------------------------------------------------------------ the model
def box_rows(tri, b, cntd, xold, lam, kind, sweeps, frozen=-1, box=NO_BOX, seen=None):
    """steps 5-6 and B0-B4 for a batch: tri (B, T) the packed lower triangles, b (B, K), cntd (B,) the entry counts as doubles,
    xold (B, K) -> x (B, K), passed the diagonal test (B,).  `seen`: called with every step's dl; it only looks"""
    B, K = b.shape
    tp, tq = triangle(K)
    d = np.arange(K)
    lo, hi, ncols = box

    def clamp(y):
        y = np.where(y < lo, lo, y)
        return np.where(y > hi, hi, y)
    G = np.zeros((B, K, K))
    G[:, tp, tq] = tri
    ridge = lam * cntd if kind == "ridge-count" else np.full(B, float(lam))
    G[:, d, d] = G[:, d, d] + ridge[:, None]
    b = b.copy()
    if frozen >= 0:
        G[:, frozen, :frozen] = 0.0
        G[:, frozen + 1:, frozen] = 0.0
        G[:, frozen, frozen] = 1.0
        b[:, frozen] = xold[:, frozen]
    Gs = np.where(np.tri(K, dtype=bool), G, G.transpose(0, 2, 1))    # Gs[p][t] = G[max(p,t)][min(p,t)]
    diag = G[:, d, d].copy()
    ok = (diag > 0.0).all(axis=1)                                    # B0
    x = xold.copy()                                                  # B1
    x[:, :ncols] = clamp(x[:, :ncols])
    if frozen >= 0:
        x[:, frozen] = xold[:, frozen]
    res = b.copy()                                                   # B2
    for t in range(K):
        m = Gs[:, :, t] * x[:, t:t + 1]
        res = res - m
    for _ in range(sweeps):                                          # B3
        for j in range(K):
            if j == frozen:
                continue
            dd = res[:, j] / diag[:, j]
            y = x[:, j] + dd
            if j < ncols:
                y = clamp(y)
            dl = y - x[:, j]
            if seen is not None:
                seen(dl[ok])
            x[:, j] = y
            m = Gs[:, :, j] * dl[:, None]
            res = res - m
    if frozen >= 0:                                                  # B4
        x[:, frozen] = xold[:, frozen]
    return x, ok


def implicit_gram_rhs(rows, r, val, wgt, Y, conf, S):
    """the implicit kind's steps 1-4 of one row: the triangle from S, b against y_n"""
    g, bb = S, np.zeros(Y.shape[1])
    e = np.arange(int(rows.ptr[r]), int(rows.ptr[r + 1]))
    if len(e):
        y, a = Y[rows.idx[e]], val[rows.pos[e]]
        en = conf * wgt[rows.pos[e]] if wgt is not None else np.full(len(e), float(conf))
        cn = 1.0 + en
        ye = y * en[:, None]
        ac = a * cn
        chain = np.empty((len(e) + 1, len(S)))
        chain[0] = g
        plain_products(y, ye, chain[1:])
        g = np.add.accumulate(chain, axis=0, out=chain)[-1]
        bb = np.add.accumulate(np.concatenate([bb[None], ac[:, None] * y]), axis=0)[-1]
    return g, bb


def box_solve(rows, val, wgt, X_old, Y, lam, kind, sweeps, frozen=-1, box=NO_BOX, conf=CONF, seen=None):
    """mf_plan_als_solve with box sweeps for every row of a side -> (X_new, (solved, kept_empty, kept_not_pd))"""
    K = X_old.shape[1]
    X_new = X_old.copy()
    with np.errstate(all="ignore"):
        if kind == "implicit":
            todo, S = np.arange(rows.nrows), gram(Y)
            parts = [implicit_gram_rhs(rows, r, val, wgt, Y, conf, S) for r in todo]
        else:
            todo = np.flatnonzero(rows.cnt > 0)
            parts = [gram_rhs(rows, r, val, wgt, Y, X_old[r, frozen] if frozen >= 0 else 0.0, frozen) for r in todo]
        if not len(todo):
            return X_new, (0, rows.nrows, 0)
        tri, b = np.array([p[0] for p in parts]), np.array([p[1] for p in parts])
        x, ok = box_rows(tri, b, rows.cnt[todo].astype(np.float64), X_old[todo], lam, kind, sweeps, frozen, box, seen)
    X_new[todo[ok]] = x[ok]
    return X_new, (int(ok.sum()), rows.nrows - len(todo), int((~ok).sum()))


def box_solve_records(N, S, X_old, lam, kind, sweeps, frozen=-1, box=NO_BOX):
    """mf_plan_als_solve_normal with box sweeps on the (summed) records of tests/test_als_shards.py"""
    K = X_old.shape[1]
    T = K * (K + 1) // 2
    cntd = N[:, T + K]
    X_new = X_old.copy()
    with np.errstate(all="ignore"):
        todo = np.arange(len(N)) if kind == "implicit" else np.flatnonzero(cntd > 0.0)
        if not len(todo):
            return X_new, (0, len(N), 0)
        tri = S[None, :] + N[todo, :T] if kind == "implicit" else N[todo, :T]
        x, ok = box_rows(tri, N[todo, T:T + K], cntd[todo], X_old[todo], lam, kind, sweeps, frozen, box)
    X_new[todo[ok]] = x[ok]
    return X_new, (int(ok.sum()), len(N) - len(todo), int((~ok).sum()))


class BoxModel:
    def __init__(self, pat, val, weight=None):
        self.side = sides(pat.users, pat.items, pat.row, pat.col)
        self.val = np.asarray(val, np.float64)
        self.wgt = None if weight is None else np.asarray(weight, np.float64)

    def solve(self, side, X_old, Y, lam, kind, sweeps, frozen=-1, box=NO_BOX, conf=CONF, seen=None):
        return box_solve(self.side[side], self.val, self.wgt, X_old, Y, lam, kind, sweeps, frozen, box, conf, seen)

    def iteration(self, L, R, lam, kind, sweeps, frozen=(-1, -1), box=(NO_BOX, NO_BOX), conf=CONF):
        """users against R, items against the NEW L; lam, frozen, box as (users, items)"""
        L1, cu = self.solve(1, L, R, lam[0], kind, sweeps, frozen[0], box[0], conf)
        R1, ci = self.solve(0, R, L1, lam[1], kind, sweeps, frozen[1], box[1], conf)
        return L1, R1, cu, ci


def resolved(box, K):
    """(lo, hi, columns) as the launch reads a side's box: no column where both bounds are infinite, -1 means all K"""
    if box is None or (box[0] == -np.inf and box[1] == np.inf):
        return NO_BOX
    cols = box[2] if len(box) > 2 else -1
    return (box[0], box[1], K if cols < 0 else cols)


USER_LENS = (0, 1, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def toy():
    """40 users x 36 items: users of 0, 1, 15, 16, 17 and 33 entries (both gather chunks, 8 and 16, from below, exactly and from
    above), the others 2 .. 11; item 35 is rated by nobody"""
    rng = np.random.default_rng(4100)
    lens = np.concatenate([USER_LENS, rng.integers(2, 12, 40 - len(USER_LENS))])
    row = np.repeat(np.arange(40), lens)
    col = np.concatenate([np.sort(rng.choice(35, int(n), replace=False)) for n in lens if n])
    pat = Pattern("toy", 40, 36, row, col)
    assert tuple(pat.ulen[:6]) == USER_LENS and pat.ilen[35] == 0 and pat.ilen.max() >= 9
    return pat


def toy_inputs(K, seed=0):
    pat = toy()
    rng = np.random.default_rng(4200 + K + seed)
    return pat, rng.uniform(-1, 1, (pat.users, K)), rng.uniform(-1, 1, (pat.items, K)), rng.integers(-10, 11, pat.nnz) / 2.0


# ------------------------------------------------------------------------------------------------ CPU
def scalar_box_row(G, b, xold, f, box, sweeps):
    """B0-B4 of one row with Python floats, one operation per statement: the guard of the batched model"""
    K = len(b)
    lo, hi, ncols = box

    def clamp(y):
        y = lo if y < lo else y
        return hi if y > hi else y

    def gs(p, t):
        return float(G[max(p, t)][min(p, t)])
    if not all(G[j][j] > 0.0 for j in range(K)):
        return None
    x = [float(v) for v in xold]
    for p in range(min(ncols, K)):
        x[p] = clamp(x[p])
    if f >= 0:
        x[f] = float(xold[f])
    res = [float(v) for v in b]
    for p in range(K):
        for t in range(K):
            m = gs(p, t) * x[t]
            res[p] = res[p] - m
    for _ in range(sweeps):
        for j in range(K):
            if j == f:
                continue
            d = res[j] / float(G[j][j])
            y = x[j] + d
            if j < ncols:
                y = clamp(y)
            dl = y - x[j]
            x[j] = y
            for p in range(K):
                m = gs(p, j) * dl
                res[p] = res[p] - m
    return x


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_the_batched_model_is_the_scalar_restatement(kind):
    K = 5
    pat, L0, R0, val = toy_inputs(K)
    rows = sides(pat.users, pat.items, pat.row, pat.col)[1]
    for frozen, box, sweeps in ((-1, NO_BOX, 1), (-1, (0.0, np.inf, K), 3), (2, (0.0, 0.5, 3), 2)):
        if kind == "implicit" and frozen >= 0:
            continue
        got, counts = box_solve(rows, val, None, L0, R0, LAM_U, kind, sweeps, frozen, box)
        assert counts[2] == 0 and counts[0] >= pat.users - 1
        S = gram(R0)
        for r in range(pat.users):
            if kind == "implicit":
                tri, b = implicit_gram_rhs(rows, r, val, None, R0, CONF, S)
            elif rows.cnt[r] == 0:
                assert_same_bits(got[r], L0[r], "a row without entries")
                continue
            else:
                tri, b = gram_rhs(rows, r, val, None, R0, L0[r, frozen] if frozen >= 0 else 0.0, frozen)
            G = np.zeros((K, K))
            G[triangle(K)] = tri
            ridge = LAM_U * float(rows.cnt[r]) if kind == "ridge-count" else LAM_U
            for p in range(K):
                G[p][p] = G[p][p] + ridge
            b = b.copy()
            if frozen >= 0:
                G[frozen, :frozen] = 0.0
                G[frozen + 1:, frozen] = 0.0
                G[frozen, frozen] = 1.0
                b[frozen] = L0[r, frozen]
            want = scalar_box_row(G, b, L0[r], frozen, box, sweeps)
            assert_same_bits(got[r], np.array(want), "%s row %d" % (kind, r))
            if frozen >= 0:
                assert got[r, frozen] == L0[r, frozen]


def ridge_objective(pat, val, L, R, lam):
    e = val - np.einsum("ij,ij->i", L[pat.row], R[pat.col])
    return float(e @ e + lam[0] * (L * L).sum() + lam[1] * (R * R).sum())


def test_the_constrained_solve_beats_project_after_solve():
    """the motivation, on the model: non-negative ALS from one start; after 12 iterations every sweep count is below clamping
    the unconstrained solution (the joint problem is not convex: more sweeps need not be lower still)"""
    K = 6
    pat, L0, R0, val = toy_inputs(K)
    L0, R0, val = np.abs(L0), np.abs(R0), np.abs(val)
    lam, box = (0.5, 0.5), ((0.0, np.inf, K), (0.0, np.inf, K))
    m, direct = BoxModel(pat, val), AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    L, R = L0, R0
    for _ in range(12):
        L, R = direct.iteration(L, R, lam, "ridge", box=box)[:2]
    objs = [ridge_objective(pat, val, L, R, lam)]
    for sweeps in (1, 2, 4, 16):
        L, R = L0, R0
        for _ in range(12):
            L, R = m.iteration(L, R, lam, "ridge", sweeps, box=box)[:2]
        assert (L >= 0).all() and (R >= 0).all()
        objs.append(ridge_objective(pat, val, L, R, lam))
    assert max(objs[1:]) < objs[0] and min(objs[2:]) < objs[1], objs


def test_box_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in BOX_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr) and capi.hip().mf_backend_abi_version() == 5
    assert re.search(r"#define MF_ALS_BOX_MAX_SWEEPS 256\b", hdr)
    for name in ("set_als_box", "als_box"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_als_box) and callable(capi.run_als_box)
    section = hdr[hdr.index("---- Box-constrained ALS"):hdr.index("---- ALS by conjugate gradient")]
    assert hdr.index("---- ALS on user shards") < hdr.index("---- Box-constrained ALS")
    for step in ("B0.", "B1.", "B2.", "B3.", "B4.", "WEAKER than Cholesky's test", "DIFFERS from the direct implicit solve", "als_box=<sweeps>"):
        assert step in section, step
    import inspect
    from recommender_system_amd import sharded
    assert inspect.signature(sharded.AlsShardedFactorization.__init__).parameters["box_sweeps"].default == 0


def test_box_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    s = C.c_int()
    assert h.mf_plan_set_als_box(None, 1) == capi.MF_ERR_ARGUMENT and h.mf_plan_get_als_box(None, C.byref(s)) == capi.MF_ERR_ARGUMENT
    for sweeps in (-1, 257, -2 ** 31, 2 ** 31 - 1):
        assert h.mf_plan_set_als_box(fake, sweeps) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    run = h.mf_backend_run_als_box
    ok = (C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, 1, 1.0, 3, 0)

    def with_(at, v, conf=None):
        a = ok[:at] + (v,) + ok[at + 1:]
        return a if conf is None else a[:10] + (conf,) + a[11:]
    badbox = capi.Bounds(1.0, 0.0, -1)
    for args in (with_(0, None), with_(2, None), with_(3, None), with_(5, -0.5), with_(6, float("nan")), with_(7, C.byref(badbox)),
                 with_(8, C.byref(badbox)), with_(9, -1), with_(9, 3), with_(9, 5), with_(11, -1), with_(11, 257),
                 with_(9, 4, conf=-1.0), with_(9, 4, conf=float("nan")), with_(9, 4, conf=float("inf"))):
        assert run(*args) == capi.MF_ERR_ARGUMENT, args
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


@pytest.fixture(scope="module")
def rule_lines(tmp_path_factory):
    """what tests/als_box_rule_main.cpp prints: {(kind, als_cg, implicit_cg, als_box): solver} and {(kind, als_cg, implicit_cg): solver}"""
    exe = str(tmp_path_factory.mktemp("als_box_rule") / "als_box_rule_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "als_box_rule_main.cpp")])
    four, three = {}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        t = line.split()
        if t[0] == "solver":
            four[tuple(int(v) for v in t[1:5])] = tuple(int(v) for v in t[5:])
        else:
            assert t[0] == "three", line
            three[tuple(int(v) for v in t[1:4])] = tuple(int(v) for v in t[4:])
    return four, three


def test_solver_rule_with_box_sweeps(rule_lines, capi):
    """mf_sched::als_solver on every kind x als_cg x implicit_cg x als_box: (conjugate gradient?, implicit?, steps, widest K, box
    sweeps).  CG steps in force make the solve theirs and leave no sweeps; otherwise the direct solve of the kind carries them"""
    four, three = rule_lines
    kinds = (capi.ALS_KINDS["off"], capi.ALS_KINDS["ridge"], capi.ALS_KINDS["ridge-count"], capi.ALS_KINDS["implicit"])
    assert kinds == (0, 1, 2, 4)
    assert sorted(four) == sorted((k, a, i, b) for k in kinds for a in (0, 3) for i in (0, 3) for b in (0, 3)) and len(three) == 16
    for (kind, als_cg, implicit_cg, als_box), got in four.items():
        if als_cg > 0:
            want = (1, 0, als_cg, 256, 0)
        elif kind == 4 and implicit_cg > 0:
            want = (1, 1, implicit_cg, 128, 0)
        else:
            want = (0, int(kind == 4), 0, 128, als_box)
        assert got == want, (kind, als_cg, implicit_cg, als_box, got)
        if als_box == 0:   # the call of before the sweeps, field by field
            assert got == three[(kind, als_cg, implicit_cg)] and got[4] == 0


BAD_SWEEPS = ["", "0", "-1", "257", "3,", "3.5", "three", " 3x", "1e2", "0x10"]


def _cli(capi, path, cwd=None, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, cwd=cwd, env=dict(clean, **env))


@pytest.mark.parametrize("env,word", [(dict(MATFACT_SOLVER="als", MATFACT_ALS_BOX=v), b"MATFACT_ALS_BOX: expected a whole number from 1 to 256.") for v in BAD_SWEEPS] + [
    (dict(MATFACT_ALS_BOX="2"), b"MATFACT_ALS_BOX needs MATFACT_SOLVER=als or als,count."),
    (dict(MATFACT_ALS_BOX="2", MATFACT_BOUNDS="0,inf"), b"MATFACT_ALS_BOX needs MATFACT_SOLVER=als or als,count."),
    (dict(MATFACT_ALS_BOX="2", MATFACT_SOLVER="als,count", MATFACT_ALS_CG="3"), b"MATFACT_ALS_BOX cannot be combined with MATFACT_ALS_CG or MATFACT_IMPLICIT_CG"),
    (dict(MATFACT_ALS_BOX="2", MATFACT_SOLVER="als", MATFACT_IMPLICIT="2", MATFACT_IMPLICIT_CG="3"), b"MATFACT_ALS_BOX cannot be combined with MATFACT_ALS_CG or MATFACT_IMPLICIT_CG"),
    (dict(MATFACT_ALS_BOX="2", MATFACT_SOLVER="als", MATFACT_MOMENTUM="0.9"), b"MATFACT_SOLVER works on the single-GPU path only"),
], ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())) if isinstance(e, dict) else None)
def test_cli_box_refusals_die_with_empty_stdout(capi, env, word, tmp_path):
    r = _cli(capi, os.path.join(tmp_path, "no-such-file.in"), cwd=tmp_path, **env)
    assert r.returncode == 255 and r.stdout == b"" and word in r.stderr, r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    assert not os.listdir(tmp_path)


def test_cli_box_accepts_its_value_and_then_reads_the_input(capi, tmp_path):
    for env in (dict(MATFACT_SOLVER="als"), dict(MATFACT_SOLVER="als,count", MATFACT_BOUNDS="0,inf"), dict(MATFACT_SOLVER="als", MATFACT_IMPLICIT="2")):
        for v in ("1", "2", "256"):
            r = _cli(capi, os.path.join(tmp_path, "no-such-file.in"), cwd=tmp_path, MATFACT_ALS_BOX=v, **env)
            assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_" not in r.stderr, r   # the parser's message: the options passed


@pytest.mark.skipif(not isa.have_tools() or not os.path.exists(isa.DEFAULT_LIB), reason="needs the built library, llvm-objdump, llvm-readelf and c++filt")
def test_isa_of_the_box_instances():
    kernels = {n: b for n, b in isa.disassemble().items() if "mf::als_box_" in n}
    meta = {n: m for n, m in isa.metadata().items() if "mf::als_box_" in n}
    want = ["als_box_kernel<%s, %d, %d%s>(" % (t, bs, nb, im) for t, bs in (("256", 4), ("64", 2)) for nb in (1, 2, 3) for im in ("", ", mf::AlsImplicit")]
    want += ["als_box_solve_normal_kernel<256>(", "als_box_solve_normal_kernel<64>("]
    assert len(kernels) == len(want) == len(meta) == 14 and all(any(w in n for n in kernels) for w in want), sorted(kernels)
    parents = isa.metadata()
    for name, body in kernels.items():
        ops = set(isa.split(i)[0] for i in body)
        assert "v_mul_f64" in ops and "v_add_f64" in ops and "v_readlane_b32" in ops, name
        assert not [i for i in body if i.startswith("v_mfma")], name
        # The correctly rounded `/` of a coordinate step is the one place with fused operations: hipcc expands it to v_rcp_f64,
        # five Newton steps (v_fma_f64 x 3, v_fmac_f64 x 2), v_div_fmas_f64, v_div_fixup_f64 -- once per lane slot of the step
        # (two in the workgroup form, one in the one-wave form).  Outside these expansions no FP64 operation is fused.
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
        slots = 2 if "<256" in name else 1
        assert [sorted(w) for w in windows] == [["v_fma_f64"] * 3 + ["v_fmac_f64_e32"] * 2] * slots, (name, windows)
        assert not [i for i in body if i.startswith("scratch_")], name
    for name, m in meta.items():
        assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0 and m[".sgpr_spill_count"] == 0, (name, m)
        # the LDS request is the launch's (dynamic), the parent form's by construction; statically both ask for nothing
        twin = name.replace("als_box_solve_normal_kernel", "als_solve_normal_kernel").replace("als_box_kernel", "als_kernel")
        twin = twin.replace(", int)", ")").replace(", int, ", ", ")
        assert twin in parents and twin != name, twin
        assert m[".group_segment_fixed_size"] == parents[twin][".group_segment_fixed_size"] == 0, name
    launch = open(os.path.join(ROOT, "recommender-system_amd", "csrc", "mf_launch.hip.h")).read()
    body = launch[launch.index("int launch_als(mf_plan *p"):launch.index("int launch_als_normal(")]
    assert body.count("als_group_doubles(") == 1 and "kAlsBoxForm" in body      # one request for either solver


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


def box_plan(capi, pat, K, val, kind, sweeps, lam=LAM, weight=None, conf=CONF, **kw):
    plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val, weight=weight, **kw)
    try:
        plan.set_regularization(*lam)
        if kind == "implicit":
            plan.set_confidence(conf)
        plan.set_als_box(sweeps)
        plan.set_als(kind)
    except BaseException:
        plan.close()
        raise
    return plan


def hand_iteration(plan):
    plan.als_solve("users", "current")
    cu = plan.als_info("users")
    plan.als_solve("items", "next")
    ci = plan.als_info("items")
    plan.flip()
    return cu, ci


def set_boxes(plan, boxes):
    for side, box in zip(("users", "items"), boxes):
        if box is not None:
            plan.set_bounds(side, *box)


def check_iteration(capi, pat, K, val, L0, R0, kind, sweeps, where, weight=None, frozen=(-1, -1), boxes=(None, None), lam=LAM, model=None):
    """one hand iteration of a fresh plan against the model -> (L, R, counters)"""
    want = (model or BoxModel(pat, val, weight)).iteration(L0, R0, lam, kind, sweeps, frozen, tuple(resolved(b, K) for b in boxes))
    plan = box_plan(capi, pat, K, val, kind, sweeps, lam, weight)
    try:
        assert plan.als_box() == sweeps and " als_box=%d" % sweeps in plan.describe()
        set_boxes(plan, boxes)
        if frozen != (-1, -1):
            plan.set_frozen_columns(*frozen)
        plan.upload(L0, R0)
        got = hand_iteration(plan)
        L, R = plan.download()
    finally:
        plan.close()
    assert got == (want[2], want[3]), (where, got, want[2], want[3])
    assert_same_bits(L, want[0], where + ": L")
    assert_same_bits(R, want[1], where + ": R")
    return L, R, got


@gpu
@pytest.mark.parametrize("form,K", [(f, K) for f in FORM_K for K in FORM_K[f]])
def test_both_sides_under_every_kind_in_every_form(device, switches, form, K):
    """every instance of kAlsBoxForm at both ends of its range of K: users non-negative, items free"""
    capi = device
    pat, L0, R0, val = toy_inputs(K)
    switches({"MF_ALS_FORM": form})
    boxes = (NONNEG, None)
    for kind in ALL_KINDS:
        for sweeps in SWEEPS:
            where = "toy K=%d %s sweeps=%d [%s]" % (K, kind, sweeps, form)
            L, R, (cu, ci) = check_iteration(capi, pat, K, val, L0, R0, kind, sweeps, where, boxes=boxes)
            assert (L[pat.ulen > 0] >= 0.0).all() and differs(L, L0) > 0.9 and differs(R, R0) > 0.9
            if kind == "implicit":
                assert cu == (pat.users, 0, 0) and ci == (pat.items, 0, 0)
            else:
                assert cu == (pat.users - 1, 1, 0) and ci == (pat.items - 1, 1, 0)
                assert_same_bits(L[0], L0[0], where + ": the user without entries")
                assert_same_bits(R[35], R0[35], where + ": the item without entries")


BOXES = {
    "none": (None, None),
    "nonneg": (NONNEG, NONNEG),
    "zero-half": ((0.0, 0.5), (0.0, 0.5)),
    "constant": ((0.25, 0.25), (-0.75, -0.75)),
    "bias-free": ((0.0, np.inf, -2), (0.0, 0.5, -2)),     # columns = K - 2, filled in below
}


@gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("K", [20, 65])
def test_boxes(device, switches, K, name, weighted):
    capi = device
    pat, L0, R0, val = toy_inputs(K, seed=1)
    w = plain_weights(11 + K, pat.nnz) if weighted else None
    boxes = tuple(b if b is None or len(b) == 2 else (b[0], b[1], K + b[2]) for b in BOXES[name])
    if name != "none":     # the start lies outside the box
        assert (L0 < boxes[0][0]).any() and (L0 > boxes[0][1]).any() if boxes[0][1] < np.inf else (L0 < 0.0).any()
    model = BoxModel(pat, val, w)
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        for kind in ALL_KINDS:
            where = "toy K=%d %s box %s [%s]" % (K, kind, name, form)
            L, R, _ = check_iteration(capi, pat, K, val, L0, R0, kind, 2, where, weight=w, boxes=boxes, model=model)
            solved_u, solved_i = (pat.ulen > 0) | (kind == "implicit"), (pat.ilen > 0) | (kind == "implicit")
            if name == "constant":
                assert (L[solved_u] == 0.25).all() and (R[solved_i] == -0.75).all(), where
            if name == "zero-half":
                assert (L[solved_u] >= 0.0).all() and (L[solved_u] <= 0.5).all() and (L[solved_u] == 0.5).any() and (L[solved_u] == 0.0).any()
            if name == "bias-free":
                assert (L[solved_u][:, :K - 2] >= 0.0).all() and (L[solved_u][:, K - 2:] < 0.0).any(), where
                assert (R[solved_i][:, K - 2:] > 0.5).any() or (R[solved_i][:, K - 2:] < 0.0).any(), where


@gpu
@pytest.mark.parametrize("K", [20, 65])
def test_a_frozen_column_under_the_explicit_kinds(device, switches, K):
    capi = device
    pat, L0, R0, val = toy_inputs(K, seed=2)
    w = plain_weights(3, pat.nnz)
    frozen, boxes = (K - 1, 0), ((0.0, np.inf, K - 2), (-0.5, 0.5))      # the items' frozen column 0 lies inside their box
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        for kind in KINDS:
            where = "toy K=%d %s frozen [%s]" % (K, kind, form)
            L, R, _ = check_iteration(capi, pat, K, val, L0, R0, kind, 2, where, weight=w, frozen=frozen, boxes=boxes)
            assert_same_bits(L[:, K - 1], L0[:, K - 1], where + ": the users' frozen column")
            assert_same_bits(R[:, 0], R0[:, 0], where + ": the items' frozen column")
            assert (np.abs(R0[:, 0]) > 0.5).any()      # it is not clamped
            free = BoxModel(pat, val, w).iteration(L0, R0, LAM, kind, 2, box=tuple(resolved(b, K) for b in boxes))
            assert differs(free[0][:, :K - 1], L[:, :K - 1]) > 0.5


@gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_special_values(device, switches, kind):
    """a NaN and an infinity in Y, -0.0 in X_old under lo = 0, and -- under the box [-0.0, 0.5] from a start of +0.0 -- steps
    whose dl is -0.0"""
    capi = device
    K = 21
    pat, L0, R0, val = toy_inputs(K, seed=3)
    L0, R0 = L0.copy(), R0.copy()
    R0[3, 4] = np.nan
    R0[9, 0] = np.inf
    L0[5:9, ::2] = -0.0
    L0[9:12] = 0.0
    boxes = ((-0.0, 0.5), (0.0, np.inf))
    m = BoxModel(pat, val)
    L1, cu = m.solve(1, L0, R0, LAM_U, kind, 2, box=resolved(boxes[0], K))
    if kind == "implicit":
        assert cu == (0, 0, pat.users)       # the NaN is in S: no row passes the diagonal test
    else:
        assert cu[2] >= 1 and cu[0] >= 20 and np.isnan(L1).any()     # the rows that rated item 3 fail it; the infinity passes and spreads
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        L, R, got = check_iteration(capi, pat, K, val, L0, R0, kind, 2, "special %s [%s]" % (kind, form), boxes=boxes, model=m)
        kept = (L.view(np.uint64) == L0.view(np.uint64)).all(axis=1)
        assert kept.sum() >= got[0][1] + got[0][2]
    # clean factors: -0.0 in X_old of both sides, under lo = -0.0 (users) and lo = 0.0 (items: -0.0 < 0.0 is false, the start keeps
    # it), and users that start at +0.0: a step that is pushed below the box lands on -0.0 from +0.0, dl = -0.0
    pat, L0, R0, val = toy_inputs(K, seed=3)
    L0, R0 = L0.copy(), R0.copy()
    L0[5:9, ::2] = -0.0
    L0[9:16] = 0.0
    R0[2:6, ::3] = -0.0
    minus_zero = []
    m.solve(1, L0, R0, LAM_U, kind, 2, box=resolved(boxes[0], K), seen=lambda dl: minus_zero.append(int(((dl == 0.0) & np.signbit(dl)).sum())))
    assert sum(minus_zero) >= 3, "the model met no dl of -0.0"
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        L, R, _ = check_iteration(capi, pat, K, val, L0, R0, kind, 2, "signed zeros %s [%s]" % (kind, form), boxes=boxes, model=m)
        assert (np.signbit(L) & (L == 0.0)).any(), "a -0.0 reaches the stored row under lo = -0.0"


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_diagonal_test_is_weaker_than_choleskys(device, switches, kind):
    """lambda = 0.  A column of Y that is zero on a row's entries puts 0.0 on the row's diagonal: kept_not_pd, X_old's bits.  A
    row of fewer entries than K has a singular G with a positive diagonal: it is solved, where Cholesky refuses it"""
    capi = device
    K = 20
    pat, L0, R0, val = toy_inputs(K, seed=4)
    R0 = R0.copy()
    mine = pat.col[pat.row == 3]              # the 16 items of user 3
    R0[mine, 6] = 0.0
    lam = (0.0, 0.0)
    m = BoxModel(pat, val)
    L1, cu = m.solve(1, L0, R0, 0.0, kind, 2)
    others = [u for u in range(pat.users) if pat.ulen[u] and set(pat.col[pat.row == u]) <= set(mine)]
    assert 3 in others and cu == (pat.users - 1 - len(others), 1, len(others))
    short = np.flatnonzero((pat.ulen > 0) & (pat.ulen < K))
    short = np.array([u for u in short if u not in others])
    assert len(short) >= 20 and pat.ulen[short].min() <= 2 and differs(L1[short], L0[short]) > 0.9
    direct = AlsModel(pat.users, pat.items, pat.row, pat.col, val).solve(1, L0, R0, 0.0, kind)[1]
    assert direct[2] >= len(others) + 10          # Cholesky keeps most of the rank-deficient rows as well
    for form in forms_of(K):
        switches({"MF_ALS_FORM": form})
        L, R, got = check_iteration(capi, pat, K, val, L0, R0, kind, 2, "weak test %s [%s]" % (kind, form), lam=lam, model=m)
        assert got[0] == cu
        assert_same_bits(L[others], L0[others], "a row with a zero on its diagonal keeps its bits")


@gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_iterate_is_three_gauss_seidel_iterations(device, switches, kind):
    capi = device
    K = 20
    pat, L0, R0, val = toy_inputs(K, seed=5)
    boxes = (NONNEG, (0.0, 0.5))
    m = BoxModel(pat, val)
    want, counts = (L0, R0), None
    for _ in range(3):
        step = m.iteration(*want, LAM, kind, 2, box=tuple(resolved(b, K) for b in boxes))
        want, counts = step[:2], step[2:]
    switches({})
    plan = box_plan(capi, pat, K, val, kind, 2)
    try:
        set_boxes(plan, boxes)
        plan.upload(L0, R0)
        plan.iterate(3)
        L, R = plan.download()
        assert (plan.als_info("users"), plan.als_info("items")) == counts
    finally:
        plan.close()
    assert_same_bits(L, want[0], "iterate(3) %s: L" % kind)
    assert_same_bits(R, want[1], "iterate(3) %s: R" % kind)


def cuda():
    import torch
    return torch.device("cuda", 0)


def normal_buffer(rows, pitch):
    import torch
    buf = torch.full((rows + 1, pitch), float("nan"), dtype=torch.float64, device=cuda())
    torch.cuda.synchronize()
    return buf


def cut_solve(plan, side, other):
    pitch = pitch_of(plan.feats)
    buf = normal_buffer(plan.items if side == "items" else plan.user_count, pitch)
    plan.als_normal(side, other, buf.data_ptr(), pitch)
    plan.als_solve_normal(side, buf.data_ptr(), pitch)
    return plan.als_info(side)


@gpu
@pytest.mark.parametrize("form,K", [("wave", 21), ("wg", 30), ("wg", 65)])
def test_whole_plan_cut_solve_is_als_solve(device, switches, form, K):
    capi = device
    pat, L0, R0, val = toy_inputs(K, seed=6)
    w = plain_weights(8, pat.nnz)
    switches({"MF_ALS_FORM": form})
    for kind in KINDS:
        ref, cut = box_plan(capi, pat, K, val, kind, 2, weight=w), box_plan(capi, pat, K, val, kind, 2, weight=w)
        try:
            for p in (ref, cut):
                p.set_frozen_columns(K - 1, -1)
                set_boxes(p, ((0.0, np.inf, K - 1), (0.0, 0.5)))
                p.upload(L0, R0)
            want = hand_iteration(ref)
            got = (cut_solve(cut, "users", "current"), cut_solve(cut, "items", "next"))
            cut.flip()
            assert got == want and want[0][0] == pat.users - 1, (kind, got, want)
            (L, R), (L1, R1) = cut.download(), ref.download()
            assert_same_bits(L, L1, "cut %s K=%d: L" % (kind, K))
            assert_same_bits(R, R1, "cut %s K=%d: R" % (kind, K))
            assert differs(L1, L0) > 0.9 and (R1[pat.ilen > 0] <= 0.5).all()
        finally:
            ref.close()
            cut.close()


@gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_two_user_shards_on_one_gpu(device, switches, kind):
    """every shard's user solve and item records, the records summed in shard order by torch, every shard's solve of the sum"""
    capi = device
    import torch
    K, sweeps, cut = 30, 2, 17
    pat, L0, R0, val = toy_inputs(K, seed=7)
    w = plain_weights(61, pat.nnz) if kind != "ridge" else None
    boxes = (NONNEG, (0.0, 0.5))
    bu, bi = (resolved(b, K) for b in boxes)
    conf = CONF if kind == "implicit" else None
    # the model of the procedure
    blocks, shards, N, S = [], [], None, None
    with np.errstate(all="ignore"):
        for b, e in ((0, cut), (cut, pat.users)):
            sel = (pat.row >= b) & (pat.row < e)
            rows = sides(e - b, pat.items, pat.row[sel] - b, pat.col[sel])
            sw = None if w is None else w[sel]
            Lb, cu = box_solve(rows[1], val[sel], sw, L0[b:e], R0, LAM_U, kind, sweeps, box=bu)
            n, s = normal_records(rows[0], val[sel], sw, R0, Lb, -1, conf), gram(Lb)
            N, S = (n, s) if N is None else (N + n, S + s)
            blocks.append(Lb)
            shards.append((b, e, sel, cu))
    R1, ci = box_solve_records(N, S, R0, LAM_I, kind, sweeps, box=bi)
    assert (N[:, -1] == pat.ilen).all() and ci[0] >= pat.items - 1
    switches({})
    pitch = pitch_of(K)
    plans, bufs = [], []
    try:
        for b, e, sel, cu in shards:
            sub = Pattern("shard", pat.users, pat.items, pat.row[sel], pat.col[sel])
            plan = box_plan(capi, sub, K, val[sel], kind, sweeps, weight=None if w is None else w[sel], user_begin=b, user_count=e - b)
            plans.append(plan)
            set_boxes(plan, boxes)
            plan.upload(L0[b:e], R0)
            plan.als_solve("users", "current")
            assert plan.als_info("users") == cu
            bufs.append(normal_buffer(pat.items, pitch))
            plan.als_normal("items", "next", bufs[-1].data_ptr(), pitch)
        for plan in plans:
            plan.synchronize()
        total = bufs[0] + bufs[1]
        torch.cuda.synchronize()
        for g, plan in enumerate(plans):
            plan.als_solve_normal("items", total.data_ptr(), pitch)
            assert plan.als_info("items") == ci, (g, plan.als_info("items"), ci)
            plan.flip()
            L, R = plan.download()
            assert_same_bits(L, blocks[g], "%s shard %d: L block" % (kind, g))
            assert_same_bits(R, R1, "%s shard %d: R" % (kind, g))
    finally:
        for plan in plans:
            plan.close()
    single = BoxModel(pat, val, w).iteration(L0, R0, LAM, kind, sweeps, box=(bu, bi))
    assert_same_bits(np.concatenate(blocks), single[0], "the user blocks are the single plan's")
    assert differs(R1, single[1]) > 0.0        # the sum over shards is re-associated: the single plan's bits are not expected


@gpu
def test_normal_sum_and_solve_on_one_caller_stream_without_host_synchronisation(device, switches):
    capi = device
    import torch
    K, kind = 30, "ridge-count"
    pat, L0, R0, val = toy_inputs(K, seed=8)
    pitch = pitch_of(K)
    T = K * (K + 1) // 2
    switches({})
    rng = np.random.default_rng(5)
    extra_host = np.zeros((pat.items + 1, pitch))
    extra_host[:, :T + K] = rng.uniform(-0.01, 0.01, (pat.items + 1, T + K))
    extra_host[np.arange(0, pat.items, 5), T + K] = 1.0
    results = []
    for ordered in (False, True):
        plan = box_plan(capi, pat, K, val, kind, 2)
        try:
            plan.set_bounds("items", 0.0, 0.5)
            plan.upload(L0, R0)
            extra = torch.from_numpy(extra_host).to(cuda())
            buf = normal_buffer(pat.items, pitch)
            if ordered:
                s = torch.cuda.Stream(cuda())
                assert s.cuda_stream != 0
                plan.set_stream(s.cuda_stream)
                with torch.cuda.stream(s):
                    torch.cuda._sleep(50_000_000)          # the stream is busy while the host enqueues everything below
                    plan.als_normal("items", "current", buf.data_ptr(), pitch)
                    buf.add_(extra)
                    plan.als_solve_normal("items", buf.data_ptr(), pitch)
                    summed = buf.clone()
                s.synchronize()
            else:
                plan.als_normal("items", "current", buf.data_ptr(), pitch)
                plan.synchronize()
                buf.add_(extra)
                torch.cuda.synchronize()
                plan.als_solve_normal("items", buf.data_ptr(), pitch)
                plan.synchronize()
                summed = buf.clone()
                torch.cuda.synchronize()
            info = plan.als_info("items")
            plan.als_solve("users", "current")
            plan.flip()
            results.append((plan.download(want_l=False)[1], summed.cpu().numpy(), info))
        finally:
            plan.close()
    (R_sync, N_sync, i_sync), (R_ord, N_ord, i_ord) = results
    assert i_sync == i_ord and i_sync[0] >= pat.items - 1
    assert_same_bits(N_ord, N_sync, "the summed records")
    assert_same_bits(R_ord, R_sync, "R")
    want, ci = box_solve_records(N_sync[:pat.items, :T + K + 1], None, R0, LAM_I, kind, 2, box=(0.0, 0.5, K))
    assert_same_bits(R_sync, want, "R against the model of the summed records")
    assert ci == i_sync and differs(R_sync, R0) > 0.9


@gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_refusals_change_nothing_and_zero_sweeps_is_the_direct_solve(device, switches, kind):
    capi = device
    K = 20
    pat, L0, R0, val = toy_inputs(K, seed=9)
    U = capi.MF_ERR_UNSUPPORTED
    implicit = kind == "implicit"
    switches({})

    def refused(call, status=U):
        with pytest.raises(capi.HipBackendError) as err:
            call()
        assert err.value.status == status, (err.value.status, status)

    def fresh():
        plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val)
        plan.set_regularization(*LAM)
        plan.set_bounds("users", *NONNEG)
        if implicit:
            plan.set_confidence(CONF)
        return plan
    untold, plan = fresh(), fresh()
    try:
        untold.set_als(kind)
        assert plan.als_box() == 0 and " als_box" not in plan.describe()
        plan.set_als_box(3)                       # a kind is not needed, and nothing is told while there is none
        assert plan.als_box() == 3 and " als" not in plan.describe()
        plan.set_als(kind)
        told = plan.describe()
        assert told == untold.describe() + " als_box=3" or told.replace(" als_box=3", "") == untold.describe()
        assert re.search(r" als_form=\w+\(chunk=\d+\) als_box=3( |$)", told), told
        for bad in (-1, 257):
            refused(lambda: plan.set_als_box(bad), capi.MF_ERR_ARGUMENT)
        # conjugate-gradient steps second
        refused(lambda: plan.set_als_cg(2))
        if implicit:
            refused(lambda: plan.set_implicit_cg(2))
        else:
            plan.set_implicit_cg(2)               # not in force under an explicit kind
            refused(lambda: plan.set_als("implicit"))
            plan.set_implicit_cg(0)
        assert plan.als_box() == 3 and plan.als_cg() == 0 and plan.als() == kind and plan.describe() == told
        # box sweeps second
        plan.set_als_box(0)
        if implicit:
            plan.set_implicit_cg(2)
        else:
            plan.set_als_cg(2)
        before = plan.describe()
        refused(lambda: plan.set_als_box(3))
        assert plan.als_box() == 0 and plan.describe() == before
        plan.set_als_cg(0)
        plan.set_implicit_cg(0)
        # momentum stays refused under ALS, a frozen column under the implicit kind at launch
        refused(lambda: plan.set_momentum(0.5, 0.5))
        plan.set_als_box(2)
        plan.upload(L0, R0)
        if implicit:
            plan.set_frozen_columns(2, -1)
            refused(lambda: plan.als_solve("users", "current"))
            refused(lambda: plan.iterate(1))
            plan.set_frozen_columns(-1, -1)
            assert plan.als_info("users") == (0, 0, 0)
        # a nonzero value, then 0: the direct solve's bits and kernels again
        hand_iteration(plan)
        boxed = plan.download()
        plan.set_als_box(0)
        assert plan.describe() == untold.describe()
        plan.upload(L0, R0)
        untold.upload(L0, R0)
        assert hand_iteration(plan) == hand_iteration(untold)
        (L, R), (L1, R1) = plan.download(), untold.download()
        assert_same_bits(L, L1, "sweeps 0 after 2: L")
        assert_same_bits(R, R1, "sweeps 0 after 2: R")
        if implicit:
            want = ImplicitModel(pat.users, pat.items, pat.row, pat.col, val).iteration(L0, R0, LAM, CONF, box=((0.0, np.inf, K), NO_BOX))
        else:
            want = AlsModel(pat.users, pat.items, pat.row, pat.col, val).iteration(L0, R0, LAM, kind, box=((0.0, np.inf, K), NO_BOX))
        assert_same_bits(L, want[0], "sweeps 0: the direct model's L")
        assert_same_bits(R, want[1], "sweeps 0: the direct model's R")
        assert differs(boxed[0], L) > 0.5
    finally:
        plan.close()
        untold.close()


@gpu
def test_k_129_is_unsupported_with_a_kind_set(device, switches):
    capi = device
    pat, L0, R0, val, alpha = _small(K=129)
    switches({})
    plan = capi.Plan(pat.users, pat.items, 129, alpha, pat.row, pat.col, val)
    try:
        plan.set_als_box(2)                       # no kind: accepted, and the kind is then refused as ever
        for kind in ALL_KINDS:
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_als(kind)
            assert err.value.status == capi.MF_ERR_UNSUPPORTED
        plan.set_als_box(0)
        plan.set_als_cg(2)
        plan.set_als("ridge")                     # K = 129 under CG: a kind is set
        before = plan.describe()
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_als_box(2)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.als_box() == 0 and plan.describe() == before
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_backend_run_als_box_equals_the_plan_session(device, switches, kind):
    capi = device
    K = 10
    pat, L0, R0, val = toy_inputs(K, seed=10)
    inst = capi.Instance(3, 1e-3, K, pat.users, pat.items, pat.row, pat.col, val)
    w = plain_weights(5, pat.nnz)
    switches({})
    plan = box_plan(capi, pat, K, val, kind, 2, weight=w)
    try:
        plan.set_bounds("users", *NONNEG)
        plan.upload(L0, R0)
        plan.iterate(3)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    L, R = L0.copy(), R0.copy()
    best = capi.backend_run_als_box(inst, L, R, 2, kind, conf=CONF, bounds_users=NONNEG, weight=w, lambda_users=LAM_U, lambda_items=LAM_I)
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    m, want = BoxModel(pat, val, w), (L0, R0)
    for _ in range(3):
        want = m.iteration(*want, LAM, kind, 2, box=((0.0, np.inf, K), NO_BOX))[:2]
    assert_same_bits(L, want[0], "L against the model")
    assert_same_bits(R, want[1], "R against the model")
    if kind != "implicit":      # sweeps 0: mf_backend_run_als
        La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
        b0 = capi.backend_run_als_box(inst, La, Ra, 0, kind, lambda_users=LAM_U, lambda_items=LAM_I)
        b1 = capi.backend_run_als(inst, Lb, Rb, kind, lambda_users=LAM_U, lambda_items=LAM_I)
        assert_same_bits(La, Lb, "sweeps 0: L of mf_backend_run_als")
        assert_same_bits(Ra, Rb, "sweeps 0: R of mf_backend_run_als")
        assert np.array_equal(b0, b1)


@gpu
def test_cli_solver_with_box_sweeps(device, orc, switches):
    """MATFACT_SOLVER=als[,count] MATFACT_ALS_BOX=n on inst30-40-10-2-10: stdout is the plan session's recommendation after the
    file's iterations from the reference's initialisation, byte for byte"""
    capi = device
    path = golden_in("inst30-40-10-2-10")
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    switches({})

    def session(kind, sweeps, lam, box, conf):
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
        try:
            plan.set_regularization(*lam)
            if box:
                plan.set_bounds("users", *box)
                plan.set_bounds("items", *box)
            if conf is not None:
                plan.set_confidence(conf)
            plan.set_als_box(sweeps)
            plan.set_als(kind)
            assert " als_box=%d" % sweeps in plan.describe()
            plan.upload(L0, R0)
            plan.iterate(inst.iters)
            return orc.format_out(plan.recommend()).encode()
        finally:
            plan.close()
    for env, args in ((dict(MATFACT_SOLVER="als", MATFACT_ALS_BOX="2", MATFACT_LAMBDA="0.05,0.3", MATFACT_BOUNDS="0,inf"), ("ridge", 2, LAM, NONNEG, None)),
                      (dict(MATFACT_SOLVER="als,count", MATFACT_ALS_BOX="1", MATFACT_LAMBDA="0.1"), ("ridge-count", 1, (0.1, 0.1), None, None)),
                      (dict(MATFACT_SOLVER="als", MATFACT_IMPLICIT="2", MATFACT_ALS_BOX="3", MATFACT_LAMBDA="0.1", MATFACT_BOUNDS="0,0.5"),
                       ("implicit", 3, (0.1, 0.1), (0.0, 0.5), 2.0))):
        r = _cli(capi, path, **env)
        assert r.returncode == 0 and r.stdout == session(*args), (env, r)
        assert (r.stderr == b"") == ("MATFACT_IMPLICIT" not in env), (env, r.stderr)      # the implicit run's objective line
