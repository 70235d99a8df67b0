"""Adaptive step sizes: AdaGrad, RMSProp and Adam behind every sweep form (mf_plan_set_adaptive, mf_plan_get_adaptive,
mf_plan_reset_adaptive, mf_plan_adaptive_finish, mf_plan_download_adaptive_state, mf_plan_upload_adaptive_state,
mf_backend_run_adaptive, MATFACT_OPTIMIZER).

The definition is the library's own (include/matfact_hip.h).  A seeded sweep of a side with a kind first forms g, the bits of
the side's unseeded sweep (test_regularised's model_sweep from 0.0), and then per element, every line rounded once,

    q = g * g
    adagrad:  v' = v + q                                                   mh = g        vh = v'
    rmsprop:  v' = (beta2 * v) + (ob2 * q)                                 mh = g        vh = v'
    adam:     m' = (beta1 * m) + (ob1 * g);  v' = (beta2 * v) + (ob2 * q)  mh = m' / c1  vh = v' / c2
    s = sqrt(vh);  den = s + eps;  u = mh / den;  step = eta * u;  x' = (x * d) + step

with c1 = 1.0 - p1, c2 = 1.0 - p2 of the sequential products p1 = p1 * beta1, p2 = p2 * beta2 (ADAM only), then the box, then
the frozen select.  The model below is plain numpy float64 (np.sqrt and / are correctly rounded); every GPU comparison is bit
for bit (assert_same_bits of test_sweep_edges.py) and covers the factors, m, v, steps, p1 and p2.  The two sides carry
different, inexact numbers (eta 0.03 / 0.01, beta1 0.9 / 0.8, beta2 0.999 / 0.99, eps 1e-8 / 1e-6), so a swapped side shows.
"""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in
from test_regularised import CASES, LAM_I, LAM_U, ZERO_FORMS, Model, _case_id, _pick, _small, _toy, decay, differs, fast_dot, model_sweep
from test_sweep_edges import CLASSES, assert_same_bits, cls_signed, is_negzero, pattern
from test_weighted import plain_weights

gpu = pytest.mark.gpu

KINDS = ("adagrad", "rmsprop", "adam")
LAM = (LAM_U, LAM_I)
# (eta, beta1, beta2, eps) of the users' and of the items' side
NUM_U = (0.03, 0.9, 0.999, 1e-8)
NUM_I = (0.01, 0.8, 0.99, 1e-6)
NO_BOX = (-np.inf, np.inf, 0)


# ------------------------------------------------------------------------------------------------ the model
class State:
    """the accumulators of one side: at rest zeros, 1.0, 1.0, 0 steps"""

    def __init__(self, shape, m=None, v=None, steps=0, p1=1.0, p2=1.0):
        self.m = np.zeros(shape) if m is None else np.array(m, np.float64)
        self.v = np.zeros(shape) if v is None else np.array(v, np.float64)
        self.steps, self.p1, self.p2 = int(steps), float(p1), float(p2)


def accumulate_v(v, g):
    """ADAGRAD's accumulator: the square is rounded, then the sum"""
    q = g * g
    return v + q


def finish(kind, num, g, x, st, d, frozen=-1, box=NO_BOX, accumulate=accumulate_v):
    """(x', state') of one seeded adaptive sweep of a side from its g: the header's steps 2 and 3, one rounding per line"""
    eta, b1, b2, eps = num
    p1, p2 = st.p1, st.p2
    with np.errstate(all="ignore"):
        if kind == "adam":
            p1 = p1 * b1
            p2 = p2 * b2
        c1 = 1.0 - p1
        c2 = 1.0 - p2
        ob1 = 1.0 - b1
        ob2 = 1.0 - b2
        q = g * g
        m = st.m
        if kind == "adagrad":
            v = accumulate(st.v, g)
        else:
            bv = b2 * st.v
            oq = ob2 * q
            v = bv + oq
        mh, vh = g, v
        if kind == "adam":
            bm = b1 * st.m
            og = ob1 * g
            m = bm + og
            mh = m / c1
            vh = v / c2
        s = np.sqrt(vh)
        den = s + eps
        u = mh / den
        step = eta * u
        xd = x * d
        y = xd + step
        lo, hi, columns = box
        if columns:
            part = y[:, :columns]
            part = np.where(part < lo, lo, part)      # compares and selects: a NaN stays, -0.0 stays under lo = 0.0
            part = np.where(part > hi, hi, part)
            y = np.concatenate([part, y[:, columns:]], axis=1)
        y, m, v = np.array(y), np.array(m), np.array(v)
        if frozen >= 0:
            y[:, frozen], m[:, frozen], v[:, frozen] = x[:, frozen], st.m[:, frozen], st.v[:, frozen]
    return y, State(x.shape, m, v, st.steps + 1, p1, p2)


class AModel(Model):
    """test_regularised's model with an adaptive rule per side: kinds = (users, items)"""

    def __init__(self, users, items, row, col, val, alpha, wgt=None):
        super().__init__(users, items, row, col, val, alpha)
        self.wgt = None if wgt is None else np.asarray(wgt, np.float64)

    def gradients(self, L, R, dot=fast_dot):
        """(g_users, g_items): the unseeded sweeps, 0.0 + every e_n * y_n in the side's order; e_n weighted on a weighted plan"""
        with np.errstate(all="ignore"):
            c2 = self.alpha * 2
            e = c2 * (self.val - dot(L, R, self.row, self.col))
            if self.wgt is not None:
                e = e * self.wgt
            return model_sweep(L, R, e, self.us, self.col, 1.0, False), model_sweep(R, L, e, self.its, self.row, 1.0, False)

    def astep(self, L, R, su, si, kinds, lam=LAM, frozen=(-1, -1), box=(NO_BOX, NO_BOX), num=(NUM_U, NUM_I), accumulate=accumulate_v):
        """one iteration: (L', R', users' state', items' state')"""
        gu, gi = self.gradients(L, R)
        out = []
        for X, g, st, kind, lm, fz, bx, nm in ((L, gu, su, kinds[0], lam[0], frozen[0], box[0], num[0]),
                                               (R, gi, si, kinds[1], lam[1], frozen[1], box[1], num[1])):
            out.append(finish(kind, nm, g, X, st, decay(self.alpha, lm), fz, bx, accumulate))
        (Ln, sun), (Rn, sin) = out
        return Ln, Rn, sun, sin

    def arun(self, L, R, iters, kinds, su=None, si=None, **kw):
        su = State(L.shape) if su is None else su
        si = State(R.shape) if si is None else si
        for _ in range(iters):
            L, R, su, si = self.astep(L, R, su, si, kinds, **kw)
        return L, R, su, si


def fused_accumulate(v, g, n=1500):
    """fma(g, g, v) of the first n elements, exactly: the rational g * g + v rounded once"""
    out = []
    for vv, gg in zip(v.ravel()[:n], g.ravel()[:n]):
        out.append(float(Fraction(float(gg)) * Fraction(float(gg)) + Fraction(float(vv))))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def expected(pat_name, cls, K, kind):
    """Inputs of one (pattern, class, K) -- test_regularised's --, and three model iterations of `kind` on both sides from
    rest at lambda 0.05 / 0.3, computed once and shared."""
    pat = pattern(pat_name)
    x = type("Expected", (), {})()
    x.pat, x.K, x.kind = pat, K, kind
    x.L0, x.R0, x.val, x.alpha = CLASSES[cls](4000 + K, pat, K)
    m = x.model = AModel(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha)
    x.steps = []
    L, R, su, si = x.L0, x.R0, State(x.L0.shape), State(x.R0.shape)
    for _ in range(3):
        L, R, su, si = m.astep(L, R, su, si, (kind, kind))
        x.steps.append((L, R, su, si))
    if cls == "signed":
        plain = Model.step(m, x.L0, x.R0, LAM_U, LAM_I)
        assert differs(x.steps[0][0], plain[0]) > 0.5 and differs(x.steps[0][1], plain[1]) > 0.5, (pat_name, K, kind)
        swapped = m.astep(x.L0, x.R0, State(x.L0.shape), State(x.R0.shape), (kind, kind), num=(NUM_I, NUM_U))
        assert differs(x.steps[0][0], swapped[0]) > 0.5 and differs(x.steps[0][1], swapped[1]) > 0.5, (pat_name, K, kind)
    return x


def same_state(plan, side, want, where, adam):
    m, v, steps, p1, p2 = plan.download_adaptive_state(side)
    assert_same_bits(v, want.v, "%s: v of %s" % (where, side))
    assert_same_bits(m, want.m if adam else np.zeros_like(want.m), "%s: m of %s" % (where, side))
    assert steps == want.steps, (where, side, steps, want.steps)
    assert_same_bits(np.array([p1, p2]), np.array([want.p1, want.p2]), "%s: p1, p2 of %s" % (where, side))


def same_all(plan, want, where, adam):
    """factors and both sides' state against (L, R, users' state, items' state)"""
    L, R = plan.download()
    assert_same_bits(L, want[0], where + ": L")
    assert_same_bits(R, want[1], where + ": R")
    same_state(plan, "users", want[2], where, adam)
    same_state(plan, "items", want[3], where, adam)


def set_both(plan, kind, num=(NUM_U, NUM_I)):
    plan.set_adaptive("users", kind, *num[0])
    plan.set_adaptive("items", kind, *num[1])


# ------------------------------------------------------------------------------------------------ CPU
ADAPTIVE_SYMBOLS = ("mf_plan_set_adaptive", "mf_plan_get_adaptive", "mf_plan_reset_adaptive", "mf_plan_adaptive_finish",
                    "mf_plan_download_adaptive_state", "mf_plan_upload_adaptive_state", "mf_backend_run_adaptive")


@pytest.mark.parametrize("K", [3, 6, 100])
@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed"])
def test_model_guards_against_silent_contraction(pat_name, K):
    """v + g * g formed as one fused multiply-add differs from the definition on a sample (second step: v is not 0 there);
    ADAGRAD is RMSPROP's formula at beta2 = 1, ob2 = 1; expected() asserts that the rule and the sides' numbers show."""
    x = expected(pat_name, "signed", K, "adagrad")
    m = x.model
    L, R, su, si = x.steps[0]
    gu, gi = m.gradients(L, R)
    for g, st in ((gu, su), (gi, si)):
        mine = accumulate_v(st.v, g)
        fused = fused_accumulate(st.v, g)
        assert differs(mine.ravel()[:len(fused)], fused) > 0.0, (pat_name, K, "fma mutant")
        with np.errstate(all="ignore"):
            rms_at_one = (1.0 * st.v) + (1.0 * (g * g))
        assert_same_bits(mine, rms_at_one, "adagrad is rmsprop's formula at (1, 1)")
    # the fused accumulator reaches the factors: a model built on it differs after two steps
    def fused_all(v, g):
        return np.array([float(Fraction(float(b)) * Fraction(float(b)) + Fraction(float(a))) for a, b in zip(v.ravel(), g.ravel())]).reshape(v.shape)
    if K == 3:
        mut = m.astep(L, R, su, si, ("adagrad", "adagrad"), accumulate=fused_all)
        assert differs(mut[0], x.steps[1][0]) > 0.0 or differs(mut[1], x.steps[1][1]) > 0.0


def test_fused_accumulate_is_a_fused_multiply_add():
    # 0.1 * 0.1 rounds up to 0.010000000000000002; fused with -0.010000000000000002 the exact product's tail survives
    p = 0.1 * 0.1
    got = fused_accumulate(np.array([-p]), np.array([0.1]))[0]
    assert got != 0.0 and got == float(Fraction(0.1) * Fraction(0.1) - Fraction(p)) and accumulate_v(np.array([-p]), np.array([0.1]))[0] == 0.0


def test_a_zero_gradient_at_rest_steps_by_plus_zero():
    """g = 0 at v = 0: 0 / eps = 0, the step is +0.0 and no NaN appears; a -0.0 gradient steps by -0.0 (sqrt(0) + eps > 0),
    which moves nothing either"""
    x = np.array([[1.5, -0.0, 0.0, -2.0]])
    for kind in KINDS:
        for g in (np.zeros((1, 4)), np.full((1, 4), -0.0)):
            y, st = finish(kind, NUM_U, g, x, State(x.shape), 0.5)
            assert not np.isnan(y).any() and not np.isnan(st.v).any() and (st.v == 0.0).all()
            assert (y == x * 0.5).all(), (kind, y)
            if not is_negzero(g).any():
                assert_same_bits(y, x * 0.5 + 0.0, kind)


def test_adaptive_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in ADAPTIVE_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr)
    assert capi.hip().mf_backend_abi_version() == 5
    assert re.search(r"typedef struct mf_adaptive \{\s*int32_t kind;[^}]*double eta, beta1, beta2, eps;\s*\} mf_adaptive;", hdr)
    for name, value in (("MF_OPT_NONE", 0), ("MF_OPT_ADAGRAD", 1), ("MF_OPT_RMSPROP", 2), ("MF_OPT_ADAM", 3)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr) and getattr(capi, name) == value
    for name in ("set_adaptive", "adaptive", "reset_adaptive", "adaptive_finish", "download_adaptive_state", "upload_adaptive_state"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_adaptive) and callable(capi.run_adaptive)


def _bad_rules(capi):
    A = capi.Adaptive
    nan, inf = float("nan"), float("inf")
    bad = [A(4, 0.1, 0.9, 0.999, 1e-8), A(-1, 0.1, 0.9, 0.999, 1e-8)]
    for kind in (1, 2, 3):
        bad += [A(kind, e, 0.9, 0.999, 1e-8) for e in (0.0, -0.1, nan, inf, -inf)]
        bad += [A(kind, 0.1, 0.9, 0.999, e) for e in (0.0, -1e-8, nan, inf)]
    for kind in (2, 3):
        bad += [A(kind, 0.1, 0.9, b, 1e-8) for b in (1.0, -0.1, nan, inf, 1.5)]
    bad += [A(3, 0.1, b, 0.999, 1e-8) for b in (1.0, -0.1, nan, inf, 1.5)]
    return bad


def test_adaptive_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    ok = capi.Adaptive(3, 0.03, 0.9, 0.999, 1e-8)
    assert h.mf_plan_set_adaptive(None, 0, C.byref(ok)) == capi.MF_ERR_ARGUMENT
    for side in (-1, 2):
        assert h.mf_plan_set_adaptive(fake, side, C.byref(ok)) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_get_adaptive(fake, side, C.byref(ok)) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_reset_adaptive(fake, side) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_adaptive_finish(fake, side) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_download_adaptive_state(fake, side, None, None, None, None, None) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_upload_adaptive_state(fake, side, None, None, None, None, None) == capi.MF_ERR_ARGUMENT
    for bad in _bad_rules(capi):
        assert h.mf_plan_set_adaptive(fake, 0, C.byref(bad)) == capi.MF_ERR_ARGUMENT, (bad.kind, bad.eta, bad.beta1, bad.beta2, bad.eps)
    assert h.mf_plan_get_adaptive(None, 0, C.byref(ok)) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_reset_adaptive(None, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_adaptive_finish(None, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_download_adaptive_state(None, 0, None, None, None, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_upload_adaptive_state(None, 0, None, None, None, None, None) == capi.MF_ERR_ARGUMENT
    neg, nan = C.c_int64(-1), C.c_double(float("nan"))
    assert h.mf_plan_upload_adaptive_state(fake, 0, None, None, C.byref(neg), None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_upload_adaptive_state(fake, 0, None, None, None, C.byref(nan), None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_upload_adaptive_state(fake, 0, None, None, None, None, C.byref(nan)) == capi.MF_ERR_ARGUMENT
    # level 1
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    run = h.mf_backend_run_adaptive
    assert run(None, None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, C.byref(ok), C.byref(ok), 0) == capi.MF_ERR_ARGUMENT
    assert run(C.byref(p), None, None, R.ctypes.data, None, 0.1, 0.1, None, None, C.byref(ok), C.byref(ok), 0) == capi.MF_ERR_ARGUMENT
    assert run(C.byref(p), None, L.ctypes.data, None, None, 0.1, 0.1, None, None, C.byref(ok), C.byref(ok), 0) == capi.MF_ERR_ARGUMENT
    for lam in ((-0.5, 0.1), (0.1, float("nan"))):
        assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, *lam, None, None, C.byref(ok), C.byref(ok), 0) == capi.MF_ERR_ARGUMENT
    badbox = capi.Bounds(1.0, 0.0, -1)
    assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, C.byref(badbox), None, C.byref(ok), C.byref(ok), 0) == capi.MF_ERR_ARGUMENT
    for bad in _bad_rules(capi):
        assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, C.byref(bad), C.byref(ok), 0) == capi.MF_ERR_ARGUMENT
        assert run(C.byref(p), None, L.ctypes.data, R.ctypes.data, None, 0.1, 0.1, None, None, C.byref(ok), C.byref(bad), 0) == capi.MF_ERR_ARGUMENT
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


BAD_OPTIMIZER = ["", "adam", "adam,", "sgd,0.1", "Adam,0.1", "adam,x", "adam,0", "adam,-0.1", "adam,nan", "adam,inf", "adam,1e999", "adam,0.1,",
                 "adam,0.1,0.9", "adam,0.1,1.0,0.999", "adam,0.1,0.9,1.0", "adam,0.1,-0.1,0.999", "adam,0.1,0.9,0.999,0", "adam,0.1,0.9,0.999,-1",
                 "adam,0.1,0.9,0.999,1e-8,1", "adam,0.1x", "rmsprop", "rmsprop,0", "rmsprop,0.1,1.0", "rmsprop,0.1,nan", "rmsprop,0.1,0.9,0",
                 "rmsprop,0.1,0.9,1e-8,3", "adagrad", "adagrad,-1", "adagrad,0.1,0", "adagrad,0.1,1e-8,0.5", "adagrad,0.1,inf", ",0.1", "0.1"]
FORBIDDEN = [dict(MATFACT_DEVICES="0"), dict(MATFACT_MATS="/dev/null"), dict(MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_RESUME="x.ck"),
             dict(MATFACT_TOPN="3"), dict(MATFACT_SIMILAR="3", MATFACT_SIMILAR_OUT="sim.out"), dict(MATFACT_MOMENTUM="0.9")]


@pytest.mark.parametrize("env", [dict(MATFACT_OPTIMIZER=v) for v in BAD_OPTIMIZER] + [dict(e, MATFACT_OPTIMIZER="adam,0.03") for e in FORBIDDEN],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_optimizer_refusals_die_with_empty_stdout(capi, env, tmp_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(clean, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_OPTIMIZER" in r.stderr, r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    assert not os.listdir(tmp_path)


def test_the_recorded_option_matrix_still_passes(capi, tmp_path):
    """the command line's answers to every recorded combination of the older options are unchanged: the existing test, run
    as it is"""
    import test_cli
    test_cli.test_cli_option_matrix_is_the_recorded_one(capi, tmp_path)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def device(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.fixture
def switches(monkeypatch):
    """No sweep switch from the caller's environment; the test sets its own."""
    from test_sweep_edges import SWITCHES
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_all(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_all


def _described(kind, num):
    eta, b1, b2, eps = num
    if kind == "adam":
        return "adam(%.17g,%.17g,%.17g,%.17g)" % (eta, b1, b2, eps)
    if kind == "rmsprop":
        return "rmsprop(%.17g,%.17g,%.17g)" % (eta, b2, eps)
    return "adagrad(%.17g,%.17g)" % (eta, eps)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_adaptive_sweeps_through_every_form(device, switches, case, kind):
    """Three iterations from rest at lambda 0.05 / 0.3 -- iterate(1), then iterate(2) -- against the model, factors and state,
    in every sweep form at the rule's chunk size and at 5; where the form has separate sweeps, one seeded step through
    sweep_items / sweep_users and the unseeded sweeps, which are g.  The es-shaped plans keep their description and run the
    two sweeps: the errors + streams iteration would seed from X_old and miss the model."""
    capi = device
    K = case["K"]
    x = expected(case["pat"], "signed", K, kind)
    pat = x.pat
    switches(case["env"])
    if case["nch"]:
        switches({"MF_SWEEP_NCH": case["nch"]})
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        assert plan.adaptive("users")[0] == "none" and " adaptive=" not in plan.describe()
        plan.set_regularization(LAM_U, LAM_I)
        set_both(plan, kind)
        desc = plan.describe()
        assert case["check"](desc, K), desc
        assert ("MF_SWEEP_NCH=5" in desc) == (case["nch"] == "5"), desc
        assert " adaptive=%s/%s" % (_described(kind, NUM_U), _described(kind, NUM_I)) in desc, desc
        assert plan.adaptive("users")[0] == kind and plan.adaptive("users")[1] == NUM_U[0] and plan.adaptive("items")[4] == NUM_I[3]
        where = "%s %s [%s]" % (_case_id(case), kind, desc.split(" loss=")[0])
        adam = kind == "adam"
        if case["steps"]:
            plan.upload(x.L0, x.R0)
            plan.sweep_items(seed_from_old=True)
            plan.sweep_users(seed_from_old=True)
            plan.flip()
            same_all(plan, x.steps[0], where + ": seeded sweeps", adam)
            plan.upload(x.L0, x.R0)
            plan.sweep_items(seed_from_old=False)
            plan.sweep_users(seed_from_old=False)
            plan.flip()
            gu, gi = x.model.gradients(x.L0, x.R0)
            L, R = plan.download()
            assert_same_bits(L, gu, where + ": the unseeded user sweep is g")
            assert_same_bits(R, gi, where + ": the unseeded item sweep is g")
            assert plan.download_adaptive_state("users")[2] == 0 and not plan.download_adaptive_state("items")[1].any()
        plan.upload(x.L0, x.R0)
        plan.iterate(1)
        same_all(plan, x.steps[0], where + ": after iterate(1)", adam)
        plan.iterate(2)
        same_all(plan, x.steps[2], where + ": after three iterations", adam)
    finally:
        plan.close()


def _plant_state(seed, shape, cls):
    """accumulators for the special-value tests: non-negative v of ordinary size with, per class, zeros of both signs or
    inf and NaN (and a negative v, whose root is NaN) planted; m signed"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 1e-4, shape)
    m = rng.uniform(-1e-2, 1e-2, shape)
    flat_v, flat_m = v.reshape(-1), m.reshape(-1)
    where = rng.choice(flat_v.size, min(flat_v.size, 24), replace=False)
    special = {"signed": [], "zeros": [0.0, -0.0], "nonfinite": [np.inf, np.nan, -1e-6, 0.0]}[cls]
    for i, w in enumerate(where):
        if special:
            flat_v[w] = special[i % len(special)]
            flat_m[where[-1 - i]] = {"zeros": [-0.0, 0.0], "nonfinite": [np.nan, -np.inf, np.inf]}.get(cls, [0.0])[i % (2 if cls == "zeros" else 3)]
    return m, v


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", ["signed", "zeros", "nonfinite"])
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("reg", 3), ("long", 30)], ids=lambda v: str(v))
def test_special_values_follow_the_model(device, switches, name, K, cls, kind):
    """From rest: two iterations of the class's inputs (rows without entries have g = 0 at v = 0: they step by +0.0 and make
    no NaN; -0.0, inf and NaN in x and g go where the model says).  Then one more from uploaded accumulators that hold -0.0,
    inf, NaN and a negative v."""
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], cls, K, kind)
    pat, m = x.pat, x.model
    adam = kind == "adam"
    switches(case["env"])
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        set_both(plan, kind)
        assert case["check"](plan.describe(), K), plan.describe()
        where = "%s K=%d %s %s" % (name, K, cls, kind)
        # the model on rows without entries: g = 0, v stays 0, the step is +0.0, nothing becomes NaN that was not
        L1, R1, su1, si1 = x.steps[0]
        for X0, X1, st, lens, lam in ((x.L0, L1, su1, pat.ulen, LAM_U), (x.R0, R1, si1, pat.ilen, LAM_I)):
            empty = np.flatnonzero(lens == 0)   # the "pair" pattern has 67 such users; "long-items" has none
            assert len(empty) or case["pat"] != "pair" or X0 is x.R0, where
            with np.errstate(all="ignore"):
                assert_same_bits(X1[empty], X0[empty] * decay(x.alpha, lam) + 0.0, where + ": a row without entries steps by +0.0")
            assert not st.v[empty].any() and not (np.isnan(X1[empty]) & ~np.isnan(X0[empty])).any(), where
        if cls == "zeros":
            assert is_negzero(x.L0).any() and is_negzero(x.R0).any()
        if cls == "nonfinite":
            assert np.isnan(L1).any() and np.isinf(x.L0).any() and np.isnan(su1.v).any()
        plan.upload(x.L0, x.R0)
        plan.iterate(2)
        same_all(plan, x.steps[1], where + ": two iterations from rest", adam)
        mu, vu = _plant_state(100 + K, x.L0.shape, cls)
        mi, vi = _plant_state(200 + K, x.R0.shape, cls)
        su = State(x.L0.shape, mu if adam else None, vu, 7, 0.9 ** 7, 0.999 ** 7)
        si = State(x.R0.shape, mi if adam else None, vi, 5, 0.8 ** 5, 0.99 ** 5)
        if not adam:
            su.p1 = su.p2 = si.p1 = si.p2 = 1.0
        plan.upload(x.L0, x.R0)
        plan.upload_adaptive_state("users", su.m, su.v, su.steps, su.p1, su.p2)
        plan.upload_adaptive_state("items", si.m, si.v, si.steps, si.p1, si.p2)
        same_state(plan, "users", su, where + ": uploaded state reads back", adam)
        want = m.astep(x.L0, x.R0, su, si, (kind, kind))
        if cls != "signed":
            assert differs(want[2].v, x.steps[0][2].v) > 0.5
        plan.iterate(1)
        same_all(plan, want, where + ": one iteration from planted accumulators", adam)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,K", [("dma-rt", 6), ("dma-ct", 100)], ids=lambda v: str(v))
def test_frozen_box_and_weights_all_at_once(device, switches, name, K, kind):
    """A weighted plan with the users' column K-1 and the items' K-2 frozen and the box [0, 0.5] over the leading K-2 columns
    of both sides: three iterations.  The frozen columns keep X_old's bits and their m and v stay at rest; the box follows
    the step (half of the signed factors leave it); frozen wins over the box."""
    capi = device
    case = _pick(name, K)
    pat = pattern(case["pat"])
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    w = plain_weights(9000 + K, pat.nnz)
    fu, fi = K - 1, K - 2
    box = (0.0, 0.5, K - 2)
    m = AModel(pat.users, pat.items, pat.row, pat.col, val, alpha, wgt=w)
    kw = dict(frozen=(fu, fi), box=(box, box))
    want = m.arun(L0, R0, 3, (kind, kind), **kw)
    free = m.arun(L0, R0, 1, (kind, kind))
    one = m.arun(L0, R0, 1, (kind, kind), **kw)
    unweighted = AModel(pat.users, pat.items, pat.row, pat.col, val, alpha).arun(L0, R0, 1, (kind, kind), **kw)
    assert differs(one[0][:, :K - 2], free[0][:, :K - 2]) > 0.3 and differs(one[1][:, :K - 2], free[1][:, :K - 2]) > 0.3   # the box cuts
    # the weights show: in the accumulators everywhere (v holds g * g), in the factors wherever the box has not cut them -- less
    # than half of the elements, and the first step of every kind is nearly eta * sign(g) whatever the weights are
    assert differs(one[2].v, unweighted[2].v) > 0.7 and differs(one[3].v, unweighted[3].v) > 0.7
    assert differs(one[0], unweighted[0]) > 0.1 and differs(one[1], unweighted[1]) > 0.1
    assert_same_bits(one[0][:, fu], L0[:, fu], "model: the users' frozen column") and not one[2].v[:, fu].any()
    assert_same_bits(one[0][:, K - 2], free[0][:, K - 2], "model: the users' column outside the box is the free step's")
    switches(case["env"])
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val, weight=w)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_frozen_columns(fu, fi)
        plan.set_bounds("users", *box)
        plan.set_bounds("items", *box)
        set_both(plan, kind)
        desc = plan.describe()
        assert case["check"](desc, K) and " weighted=1" in desc and " frozen=%d/%d" % (fu, fi) in desc and " bounds=" in desc, desc
        plan.upload(L0, R0)
        plan.iterate(3)
        where = "%s K=%d %s" % (name, K, kind)
        same_all(plan, want, where, kind == "adam")
        L, R = plan.download()
        assert_same_bits(L[:, fu], L0[:, fu], where + ": the users' frozen column")
        assert_same_bits(R[:, fi], R0[:, fi], where + ": the items' frozen column")
        assert not plan.download_adaptive_state("users")[1][:, fu].any() and not plan.download_adaptive_state("items")[1][:, fi].any()
        assert L[:, :K - 2].min() >= 0.0 and L[:, :K - 2].max() <= 0.5 and R[:, :K - 3].max() <= 0.5
    finally:
        plan.close()


@gpu
def test_the_biased_model_runs_under_adam(device, switches):
    """[ L | b_user | 1.0 ] x [ R | 1.0 | b_item ]: K = F + 2 with the users' column F + 1 and the items' column F frozen,
    three steps of ADAM: the ones stay ones, the biases move, everything equals the model."""
    capi = device
    pat, L0, R0, val, alpha = _small()
    F = 10
    mu = capi.bias_mean(val)
    Lp, Rp = capi.bias_pack(L0, None, 1), capi.bias_pack(R0, None, 0)
    m = AModel(pat.users, pat.items, pat.row, pat.col, val - mu, alpha)
    want = m.arun(Lp, Rp, 3, ("adam", "adam"), frozen=(F + 1, F))
    plan = capi.Plan(pat.users, pat.items, F + 2, alpha, pat.row, pat.col, val - mu)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_frozen_columns(F + 1, F)
        set_both(plan, "adam")
        plan.upload(Lp, Rp)
        plan.iterate(3)
        same_all(plan, want, "biased model under adam", True)
        L, R = plan.download()
        assert (L[:, F + 1] == 1.0).all() and (R[:, F] == 1.0).all() and L[:, F].any() and R[:, F + 1].any()
    finally:
        plan.close()


@functools.lru_cache(maxsize=None)
def _bundled(name="inst30-40-10-2-10"):
    import recommender_system_amd as rs
    inst = rs.capi.parse_file(golden_in(name))
    L0, R0 = rs.capi.init_factors(inst.users, inst.items, inst.feats)
    return inst, L0, R0


@functools.lru_cache(maxsize=None)
def _bundled_adam(iters):
    inst, L0, R0 = _bundled()
    m = AModel(inst.users, inst.items, inst.row, inst.col, inst.val, inst.alpha)
    return m.arun(L0, R0, iters, ("adam", "adam"))   # at lambda 0.05 / 0.3, like every run of the model


@gpu
@pytest.mark.parametrize("graph", [None, "0"])
@pytest.mark.parametrize("iters", [160, 150])
def test_graph_replay_equals_eager_launches(device, switches, iters, graph):
    """ADAM on inst30-40-10-2-10: 160 iterations are five replays of the captured 32-iteration graph, 150 four replays and
    22 eager iterations; with MF_GRAPH=0 every iteration is launched.  The step scalars live in the side's device record,
    which the tick kernel advances inside the graph: both ways give the model's bits, factors and state, so the same."""
    capi = device
    inst, L0, R0 = _bundled()
    want = _bundled_adam(iters)
    assert want[2].steps == iters and want[2].p1 == functools.reduce(lambda p, _: p * 0.9, range(iters), 1.0)
    if graph:
        switches({"MF_GRAPH": graph})
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        desc = plan.describe()
        assert ("MF_GRAPH=0" in desc) == (graph == "0") and "iterate=sweeps" in desc, desc
        plan.set_regularization(LAM_U, LAM_I)
        set_both(plan, "adam")
        plan.upload(L0, R0)
        plan.iterate(iters)
        same_all(plan, want, "MF_GRAPH=%s, %d iterations" % (graph, iters), True)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,K", [("pair", 100), ("long", 30)], ids=lambda v: str(v))
def test_a_run_resumes_bit_for_bit(device, switches, name, K, kind):
    """6 iterations = 3 iterations, factors and state downloaded into a fresh plan, 3 iterations; = iterate_monitored(6, 2)"""
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], "signed", K, kind)
    pat = x.pat
    switches(case["env"])
    adam = kind == "adam"

    def fresh():
        p = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
        p.set_regularization(LAM_U, LAM_I)
        set_both(p, kind)
        return p
    six = x.model.arun(x.steps[2][0], x.steps[2][1], 3, (kind, kind), x.steps[2][2], x.steps[2][3])
    assert six[2].steps == 6
    a, b, c, d = fresh(), fresh(), fresh(), fresh()
    try:
        assert case["check"](a.describe(), K), a.describe()
        where = "%s K=%d %s" % (name, K, kind)
        a.upload(x.L0, x.R0)
        a.iterate(6)
        same_all(a, six, where + ": 6", adam)
        b.upload(x.L0, x.R0)
        b.iterate(3)
        same_all(b, x.steps[2], where + ": 3", adam)
        L, R = b.download()
        su, si = b.download_adaptive_state("users"), b.download_adaptive_state("items")
        c.upload(L, R)
        c.upload_adaptive_state("users", *su)
        c.upload_adaptive_state("items", *si)
        c.iterate(3)
        same_all(c, six, where + ": 3, a fresh plan, 3", adam)
        d.upload(x.L0, x.R0)
        done, pts = d.iterate_monitored(6, every=2)
        assert done == 6 and [p.iter for p in pts] == [0, 2, 4, 6]
        same_all(d, six, where + ": monitored", adam)
        # without the state the fresh plan starts from rest and misses
        c.upload(L, R)
        c.iterate(3)
        assert differs(c.download()[0], six[0]) > 0.5
    finally:
        for p in (a, b, c, d):
            p.close()


@gpu
def test_reset_rules(device, switches):
    """upload_factors, a change of kind and reset_adaptive put a side at rest; a change of eta (or of any number) alone
    keeps what it has accumulated."""
    capi = device
    K = 30
    case = _pick("dma-ct", K)
    x = expected(case["pat"], "signed", K, "adam")
    pat, m = x.pat, x.model
    switches(case["env"])
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    rest_u, rest_i = State(x.L0.shape), State(x.R0.shape)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        set_both(plan, "adam")
        plan.upload(x.L0, x.R0)
        same_state(plan, "users", rest_u, "at rest before the first step", True)
        plan.iterate(3)
        same_all(plan, x.steps[2], "three iterations", True)
        # eta alone: the state stays, the next step uses the new number
        num = ((0.005,) + NUM_U[1:], (0.002, 0.7, 0.9, 1e-7))
        set_both(plan, "adam", num)
        same_state(plan, "users", x.steps[2][2], "after a change of the numbers", True)
        plan.iterate(1)
        L3, R3, su3, si3 = x.steps[2]
        want = m.astep(L3, R3, su3, si3, ("adam", "adam"), num=num)
        assert differs(want[0], m.astep(L3, R3, rest_u, rest_i, ("adam", "adam"), num=num)[0]) > 0.5   # from rest would show
        same_all(plan, want, "a fourth iteration with other numbers on the kept state", True)
        # reset_adaptive: that side only
        plan.reset_adaptive("users")
        same_state(plan, "users", rest_u, "reset_adaptive(users)", True)
        same_state(plan, "items", want[3], "reset_adaptive(users) leaves the items", True)
        plan.iterate(1)
        same_all(plan, m.astep(want[0], want[1], rest_u, want[3], ("adam", "adam"), num=num), "after reset_adaptive(users)", True)
        # a change of kind: that side at rest, m reads zeros for a side that is not ADAM
        L5, R5 = plan.download()
        items_state = plan.download_adaptive_state("items")
        plan.set_adaptive("users", "rmsprop", *NUM_U)
        same_state(plan, "users", rest_u, "after a change of kind", False)
        assert plan.download_adaptive_state("items")[2] == items_state[2] == 5
        plan.set_adaptive("users", "adam", *num[0])
        same_state(plan, "users", rest_u, "back to adam: still at rest", True)
        # upload_factors: both sides
        plan.upload(x.L0, x.R0)
        same_state(plan, "users", rest_u, "after upload_factors", True)
        same_state(plan, "items", rest_i, "after upload_factors", True)
        set_both(plan, "adam")
        plan.iterate(3)
        same_all(plan, x.steps[2], "three iterations after upload_factors", True)
        # off: a side of kind none is at rest, finish and upload_state refuse it
        plan.set_adaptive("users", "none")
        plan.set_adaptive("items", None)
        assert plan.adaptive("users") == ("none", 0.0, 0.0, 0.0, 0.0) and " adaptive=" not in plan.describe()
        same_state(plan, "items", rest_i, "kind none", False)
        for call in (lambda: plan.adaptive_finish("items"), lambda: plan.upload_adaptive_state("items", v=np.zeros(x.R0.shape))):
            with pytest.raises(capi.HipBackendError) as err:
                call()
            assert err.value.status == capi.MF_ERR_STATE
    finally:
        plan.close()
    cold = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        set_both(cold, "adam")   # legal before the upload
        for call in (lambda: cold.adaptive_finish("items"), lambda: cold.download_adaptive_state("items")):
            with pytest.raises(capi.HipBackendError) as err:
                call()
            assert err.value.status == capi.MF_ERR_STATE
    finally:
        cold.close()


@gpu
def test_momentum_and_an_adaptive_side_exclude_each_other(device):
    """in both orders the second setter returns MF_ERR_UNSUPPORTED and changes nothing; the other side stays free"""
    capi = device
    pat, L0, R0, val, alpha = _small()
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.set_momentum(0.9, 0.0)
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_adaptive("users", "adam", *NUM_U)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.adaptive("users")[0] == "none" and plan.momentum() == (0.9, 0.0)
        plan.set_adaptive("items", "adam", *NUM_I)   # the items have no momentum
        assert plan.adaptive("items")[0] == "adam" and " momentum=0.9/0 " in plan.describe() + " " and " adaptive=-/adam(" in plan.describe()
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_momentum(0.9, 0.3)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.momentum() == (0.9, 0.0) and plan.adaptive("items")[0] == "adam"
        plan.set_momentum(0.5, 0.0)   # a beta of 0 on the adaptive side is no momentum
        assert plan.momentum() == (0.5, 0.0)
        plan.set_momentum(0.0, 0.0)
        plan.set_adaptive("users", "rmsprop", *NUM_U)
        with pytest.raises(capi.HipBackendError) as err:
            plan.set_momentum(0.1, 0.0)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED and plan.momentum() == (0.0, 0.0)
        plan.set_adaptive("users", "none")
        plan.set_momentum(0.1, 0.0)
        assert plan.momentum() == (0.1, 0.0)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("name,K", ZERO_FORMS, ids=lambda v: str(v))
def test_kind_none_is_the_plain_library(device, orc, switches, name, K):
    """a plan that ran an adaptive iteration and then turned the rule off on both sides gives the oracle's bits and the
    description of a plan never told anything: an es-shaped plan takes its own form again"""
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
        set_both(plan, "adam")
        plan.upload(L0, R0)
        plan.iterate(1)   # an adaptive iteration in between: what it leaves must not show afterwards
        plan.set_adaptive("users", "none")
        plan.set_adaptive("items", "none")
        desc = plan.describe()
        assert case["check"](desc, K) and " adaptive=" not in desc and desc == untold.describe(), desc
        plan.upload(L0, R0)
        plan.iterate(2)
        L, R = plan.download()
        assert_same_bits(L, L2, "%s L after two" % name)
        assert_same_bits(R, R2, "%s R after two" % name)
    finally:
        plan.close()
        untold.close()


@gpu
@pytest.mark.parametrize("K", [3, 10])
def test_a_toy_plan_takes_the_sweeps_while_adaptive_and_its_loop_when_not(device, orc, switches, K):
    """iterate(9) of a toy instance: adaptive, the model's bits (the one-launch loop seeds unconditionally and would miss
    them); with the rule off again, the oracle's, from the one-launch loop as before"""
    capi = device
    pat, L0, R0, val, alpha = _toy(K)
    m = AModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    want = m.arun(L0, R0, 9, ("rmsprop", "rmsprop"))
    Lo, Ro = L0.copy(), R0.copy()
    orc.factorize(orc.Instance(9, alpha, K, pat.users, pat.items, pat.row, pat.col, val), Lo, Ro)
    switches({})
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        set_both(plan, "rmsprop")
        plan.upload(L0, R0)
        plan.iterate(9)
        same_all(plan, want, "toy K=%d under rmsprop" % K, False)
        plan.set_regularization(0.0, 0.0)
        plan.set_adaptive("users", None)
        plan.set_adaptive("items", None)
        plan.upload(L0, R0)
        plan.iterate(9)
        L, R = plan.download()
        assert_same_bits(L, Lo, "toy K=%d, rule off: L" % K)
        assert_same_bits(R, Ro, "toy K=%d, rule off: R" % K)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("kind", ["adam", "adagrad"])
def test_two_user_shards_on_one_gpu(device, switches, kind):
    """The users are adaptive in each shard's own sweep; the items are swept UNSEEDED on both shards, the host adds the two
    items_next in shard order, writes the sum into each shard's next-generation buffer and each shard calls
    mf_plan_adaptive_finish(items).  Against the numpy model of exactly that procedure, factors and state.
    This NARROWS what was asked for ("the result equals the one-plan run bit for bit"): the sum of the two shards' g adds
    the entries of an item as (0.0 + shard 0's) + (0.0 + shard 1's), the single plan as one chain, so the item side cannot
    equal the single plan bit for bit wherever both shards rated an item (test_momentum's two-shard test has the same
    note).  Compared with the single plan: every user block, factors and state, and the rows of R, m and v of the items
    that one shard alone rated -- there the other shard's g is +0.0 and x + 0.0 keeps the bits of a sum from 0.0."""
    import torch
    capi = device
    K, cut = 30, 333
    x = expected("pair", "signed", K, kind)
    pat = x.pat
    adam = kind == "adam"
    assert cut % 1024 and 0 < cut < pat.users
    switches({"MF_ITER_MODE": "sweeps"})
    single = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        single.set_regularization(LAM_U, LAM_I)
        set_both(single, kind)
        single.upload(x.L0, x.R0)
        single.iterate(1)
        same_all(single, x.steps[0], "single plan", adam)
    finally:
        single.close()
    Ls, Rs, sus, sis = x.steps[0]
    ld = capi.row_pitch(K)
    dev = torch.device("cuda", 0)
    lo = pat.row < cut
    shards = []
    try:
        for sel, begin, count in ((lo, 0, cut), (~lo, cut, pat.users - cut)):
            row, col, val = pat.row[sel], pat.col[sel], x.val[sel]
            rb = [torch.zeros((pat.items, ld), dtype=torch.float64, device=dev) for _ in range(2)]
            plan = capi.Plan(pat.users, pat.items, K, x.alpha, row, col, val, user_begin=begin, user_count=count,
                             items_ext=[t.data_ptr() for t in rb], items_pitch=ld)
            shards.append((plan, rb, begin, count, AModel(count, pat.items, row - begin, col, val, x.alpha)))
            plan.set_regularization(LAM_U, LAM_I)
            set_both(plan, kind)
            plan.upload(x.L0[begin:begin + count], x.R0)
            plan.sweep_items(seed_from_old=False)
            plan.sweep_users()
            plan.synchronize()
        parts, model_parts = [], []
        for plan, rb, begin, count, m in shards:
            nxt = next(t for t in rb if t.data_ptr() == plan.items_next_ptr())
            parts.append(nxt[:, :K].cpu().numpy().copy())
            model_parts.append(m.gradients(x.L0[begin:begin + count], x.R0)[1])
            assert_same_bits(parts[-1], model_parts[-1], "shard at %d: items_next before the sum is the shard's g" % begin)
        total = parts[0] + parts[1]
        Rw, siw = finish(kind, NUM_I, model_parts[0] + model_parts[1], x.R0, State(x.R0.shape), decay(x.alpha, LAM_I))
        alone = (np.bincount(pat.col[lo], minlength=pat.items) == 0) | (np.bincount(pat.col[~lo], minlength=pat.items) == 0)
        assert alone.any() and not alone.all()
        for plan, rb, begin, count, m in shards:
            nxt = next(t for t in rb if t.data_ptr() == plan.items_next_ptr())
            nxt[:, :K] = torch.from_numpy(total).to(dev)
            torch.cuda.synchronize()   # torch's stream wrote the sum; the plan's own (non-blocking) stream finishes it
            plan.adaptive_finish("items")
            plan.flip()
            Lb, R = plan.download()
            where = "shard at %d" % begin
            assert_same_bits(R, Rw, where + ": the finished sum")
            same_state(plan, "items", siw, where, adam)
            assert_same_bits(Lb, Ls[begin:begin + count], where + ": user block against the single plan")
            mu, vu, steps, p1, p2 = plan.download_adaptive_state("users")
            assert_same_bits(vu, sus.v[begin:begin + count], where + ": users' v against the single plan")
            assert_same_bits(mu, sus.m[begin:begin + count] if adam else np.zeros_like(mu), where + ": users' m against the single plan")
            assert (steps, p1, p2) == (sus.steps, sus.p1, sus.p2)
            assert_same_bits(R[alone], Rs[alone], where + ": items one shard alone rated, against the single plan")
            assert_same_bits(plan.download_adaptive_state("items")[1][alone], sis.v[alone], where + ": their v")
    finally:
        for s in shards:
            s[0].close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_backend_run_adaptive_equals_the_plan_session(device, kind):
    capi = device
    pat, L0, R0, val, alpha = _small()
    inst = capi.Instance(40, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
    box = (-0.4, 0.4)
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.upload(L0, R0)
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_bounds("users", *box)
        set_both(plan, kind)
        plan.iterate(40)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    L, R = L0.copy(), R0.copy()
    best = capi.backend_run_adaptive(inst, L, R, (kind,) + NUM_U, (kind,) + NUM_I, bounds_users=box, lambda_users=LAM_U, lambda_items=LAM_I)
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    want = AModel(pat.users, pat.items, pat.row, pat.col, val, alpha).arun(L0, R0, 40, (kind, kind), box=((box[0], box[1], 10), NO_BOX))
    assert_same_bits(L, want[0], "L against the model")
    assert_same_bits(R, want[1], "R against the model")
    # no rule on either side: mf_backend_run_reg
    La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
    b0 = capi.backend_run_adaptive(inst, La, Ra, None, None, lambda_users=LAM_U, lambda_items=LAM_I)
    b1 = capi.backend_run_reg(inst, Lb, Rb, LAM_U, LAM_I)
    assert_same_bits(La, Lb, "no rule: L of mf_backend_run_reg")
    assert_same_bits(Ra, Rb, "no rule: R of mf_backend_run_reg")
    assert np.array_equal(b0, b1)


def _cli(capi, path, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(clean, **env))


@gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "inst0"])
def test_cli_optimizer(device, orc, name):
    """MATFACT_OPTIMIZER=adam,0.03 (and rmsprop / adagrad with their own optional numbers, and with MATFACT_LAMBDA and
    MATFACT_BOUNDS): stdout is the .out of the plan's own recommendation after the file's iterations.  inst0 is
    toy-shaped: the plan and the command line both take the sweeps."""
    capi = device
    path = golden_in(name)
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)

    def session(rule, lam=None, box=None):
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
        try:
            if lam:
                plan.set_regularization(*lam)
            if box:
                plan.set_bounds("users", box[0], box[1], inst.feats)
                plan.set_bounds("items", box[0], box[1], inst.feats)
            plan.set_adaptive("users", *rule)
            plan.set_adaptive("items", *rule)
            plan.upload(L0, R0)
            plan.iterate(inst.iters)
            return orc.format_out(plan.recommend()).encode()
        finally:
            plan.close()
    for env, rule, lam, box in ((dict(MATFACT_OPTIMIZER="adam,0.03"), ("adam", 0.03, 0.9, 0.999, 1e-8), None, None),
                                (dict(MATFACT_OPTIMIZER="adam,0.01,0.8,0.99,1e-6", MATFACT_LAMBDA="0.05,0.3"), ("adam", 0.01, 0.8, 0.99, 1e-6), LAM, None),
                                (dict(MATFACT_OPTIMIZER="rmsprop,0.01,0.99", MATFACT_BOUNDS="0,0.9"), ("rmsprop", 0.01, 0.9, 0.99, 1e-8), None, (0.0, 0.9)),
                                (dict(MATFACT_OPTIMIZER="adagrad,0.1,1e-6"), ("adagrad", 0.1, 0.9, 0.999, 1e-6), None, None)):
        r = _cli(capi, path, **env)
        assert r.returncode == 0 and r.stderr == b"" and r.stdout == session(rule, lam, box), (env, r)
    plain = open(os.path.join(GOLDEN, name + ".out"), "rb").read()
    assert _cli(capi, path, MATFACT_OPTIMIZER="adam,0.03").stdout != plain or name == "inst0"


@gpu
def test_every_kind_reaches_the_plain_runs_rmse_on_ml100k(device, switches):
    """The feature's purpose.  On ML100k from the reference's initialisation the plain rule's training RMSE after the
    file's 3000 iterations is measured here; each kind must reach it within 1000 iterations at eta 0.03 (ADAM), 0.01 with
    rho 0.999 (RMSPROP), 0.1 (ADAGRAD), looked at every 10 iterations.  The cap is twice what a CPU model needed from a
    uniform start (370 / 454 / 480)."""
    capi = device
    switches({})
    inst = capi.parse_file(golden_in("instML100k"))
    assert inst.iters == 3000
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)

    def fresh():
        p = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
        p.upload(L0, R0)
        return p
    plan = fresh()
    try:
        plan.iterate(3000)
        target = plan.loss("train").rmse
    finally:
        plan.close()
    reached = {}
    for kind, num in (("adam", (0.03, 0.9, 0.999, 1e-8)), ("rmsprop", (0.01, 0.9, 0.999, 1e-8)), ("adagrad", (0.1, 0.9, 0.999, 1e-8))):
        plan = fresh()
        try:
            plan.set_adaptive("users", kind, *num)
            plan.set_adaptive("items", kind, *num)
            done, pts = plan.iterate_monitored(1000, every=10)
            rmse = [float(np.sqrt(p.train.sse / float(p.train.count))) for p in pts]
            hit = [p.iter for p, r in zip(pts, rmse) if r <= target]
            reached[kind] = hit[0] if hit else None
            print("%s: plain RMSE after 3000 iterations %.5f; reached at iteration %s; RMSE after %d: %.5f" % (kind, target, reached[kind], done, rmse[-1]))
        finally:
            plan.close()
    assert all(v is not None and v <= 1000 for v in reached.values()), (target, reached)
