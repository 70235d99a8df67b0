"""Heavy-ball momentum (mf_plan_set_momentum, mf_plan_get_momentum, mf_plan_upload_previous, mf_plan_download_previous,
mf_backend_run_momentum, MATFACT_MOMENTUM).

The definition is the library's own (include/matfact_hip.h).  For a seeded sweep of a side with beta != 0 every element of
a row that is not in the side's frozen column starts from

    v = x - x_prev;  m = beta * v;  seed = (x * d) + m        three roundings beside the decay's, nothing fused

where x_prev is what the side's next-generation buffer holds at launch, or x itself for a side at rest.  The model below is
numpy on the CPU and follows that text on top of test_regularised's model; every GPU comparison is bit for bit
(assert_same_bits of test_sweep_edges.py).  beta_users = 0.9 and beta_items = 0.3 with lambda 0.05 / 0.3 at alpha = 1e-3:
both betas are inexact and different, so a swapped side or a fused multiply-add shows (0.5 would hide a fusion).
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
from test_iterate_path import path_of_plan
from test_regularised import CASES, LAM_I, LAM_U, WIDE, ZERO_FORMS, Model, Side, _case_id, _pick, _small, _toy, decay, differs, fast_dot, model_sweep
from test_sweep_edges import (CLASSES, FORMS, PF_ROWS, SWEEPS, SWITCHES, _single_wave, assert_same_bits, cls_signed, is_negzero, pattern,
                              pattern_both_large, seq_dot, signed_inputs)

gpu = pytest.mark.gpu

BETA_U, BETA_I = 0.9, 0.3
LAM = (LAM_U, LAM_I)
BETA = (BETA_U, BETA_I)


# ------------------------------------------------------------------------------------------------ the model
def seed_of(x, xp, d, beta):
    """the seed of every element: the decay's multiply, and with beta != 0 the momentum term added -- the term is absent,
    not + 0.0, at beta == 0"""
    start = x * d
    if beta != 0.0:
        v = x - xp
        m = beta * v
        start = start + m
    return start


def msweep(X, Xp, Y, e, side, other, d, beta, seeded, frozen=-1, seed=seed_of):
    """model_sweep from the momentum seed (x * 1.0 is x); an unseeded sweep starts from 0.0 and takes no momentum; the frozen
    column keeps X's bits (0.0 unseeded)"""
    if seeded:
        out = model_sweep(seed(X, Xp, d, beta), Y, e, side, other, 1.0, True)
    else:
        out = model_sweep(X, Y, e, side, other, d, False)
    out = np.array(out)
    if frozen >= 0:
        out[:, frozen] = X[:, frozen] if seeded else 0.0
    return out


class MModel(Model):
    def mstep(self, L, R, Lp, Rp, lam=LAM, beta=BETA, seed_u=True, seed_i=True, dot=seq_dot, frozen=(-1, -1), seed=seed_of):
        """(L_new, R_new) of one iteration from the frozen L, R with the histories Lp, Rp (None: the side is at rest);
        lam, beta and frozen are (users, items)"""
        with np.errstate(all="ignore"):
            c2 = self.alpha * 2
            e = c2 * (self.val - dot(L, R, self.row, self.col))
            Ln = msweep(L, L if Lp is None else Lp, R, e, self.us, self.col, decay(self.alpha, lam[0]), beta[0], seed_u, frozen[0], seed)
            Rn = msweep(R, R if Rp is None else Rp, L, e, self.its, self.row, decay(self.alpha, lam[1]), beta[1], seed_i, frozen[1], seed)
        return Ln, Rn

    def run(self, L, R, iters, lam=LAM, beta=BETA, prev=(None, None), frozen=(-1, -1)):
        """`iters` iterations; returns (L, R, L_prev, R_prev).  A side with beta == 0 keeps no history of its own: the
        entry of `prev` it returns is what the next-generation buffer holds, the generation before."""
        Lp, Rp = prev
        for _ in range(iters):
            Ln, Rn = self.mstep(L, R, Lp, Rp, lam, beta, dot=fast_dot, frozen=frozen)
            Lp, Rp, L, R = L, R, Ln, Rn
        return L, R, Lp, Rp


def fma_sample(beta, v, xd, n=1500):
    """fma(beta, v, xd) of the first n finite elements, exactly: the rational beta * v + xd rounded once"""
    b, out = Fraction(beta), []
    for vv, aa in zip(v.ravel()[:n], xd.ravel()[:n]):
        out.append(float(b * Fraction(float(vv)) + Fraction(float(aa))))
    return np.array(out)


def seed_mutant_reassociated(x, xp, d, beta):
    return (x * d + beta * x) - beta * xp


def random_prev(seed, X):
    """an independent previous generation: X plus a step of the size a few iterations make"""
    rng = np.random.default_rng(seed)
    return X + rng.uniform(-1, 1, X.shape) * 2.0 ** -6


@functools.lru_cache(maxsize=None)
def expected(pat_name, cls, K):
    """Inputs of one (pattern, class, K), an independent random X_prev, and the model's results, computed once and shared."""
    pat = pattern(pat_name)
    x = type("Expected", (), {})()
    x.pat, x.K = pat, K
    x.L0, x.R0, x.val, x.alpha = CLASSES[cls](4000 + K, pat, K)
    x.Lp, x.Rp = random_prev(5000 + K, x.L0), random_prev(6000 + K, x.R0)
    m = x.model = MModel(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha)
    x.seeded = m.mstep(x.L0, x.R0, x.Lp, x.Rp)                      # one step with the chosen history
    x.unseeded = m.mstep(x.L0, x.R0, x.Lp, x.Rp, seed_u=False, seed_i=False)
    x.plain_unseeded = m.step(x.L0, x.R0, 0.0, 0.0, False, False)
    x.nomom = m.step(x.L0, x.R0, LAM_U, LAM_I)                      # the regularised step without momentum
    x.rest1 = m.mstep(x.L0, x.R0, None, None)                       # from rest: one and two iterations
    x.rest2 = m.mstep(*x.rest1, x.L0, x.R0)
    if cls == "signed":
        # the guards: momentum shows in more than half of the elements of each factor, and the definition differs somewhere
        # in each factor from a fused multiply-add, from the reassociated form and from the other side's beta
        assert differs(x.seeded[0], x.nomom[0]) > 0.5 and differs(x.seeded[1], x.nomom[1]) > 0.5, (pat_name, K)
        for X, Xp, lam, beta in ((x.L0, x.Lp, LAM_U, BETA_U), (x.R0, x.Rp, LAM_I, BETA_I)):
            d = decay(x.alpha, lam)
            mine = seed_of(X, Xp, d, beta)
            fused = fma_sample(beta, X - Xp, X * d)
            assert differs(mine.ravel()[:len(fused)], fused) > 0.0, (pat_name, K, "fma mutant")
            assert differs(mine, seed_mutant_reassociated(X, Xp, d, beta)) > 0.0, (pat_name, K, "reassociated mutant")
        swapped = m.mstep(x.L0, x.R0, x.Lp, x.Rp, beta=(BETA_I, BETA_U))
        assert differs(x.seeded[0], swapped[0]) > 0.0 and differs(x.seeded[1], swapped[1]) > 0.0, (pat_name, K, "swapped betas")
        assert BETA_U != BETA_I and Fraction(BETA_U).denominator > 2 and Fraction(BETA_I).denominator > 2
    return x


# ------------------------------------------------------------------------------------------------ CPU
MOMENTUM_SYMBOLS = ("mf_plan_set_momentum", "mf_plan_get_momentum", "mf_plan_upload_previous", "mf_plan_download_previous",
                    "mf_backend_run_momentum")


@pytest.mark.parametrize("K", [3, 6, 100])
@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed"])
def test_model_guards_and_its_degenerate_cases(pat_name, K):
    """expected() asserts the guards; at beta = 0 the model is test_regularised's, whatever the history; from rest a step
    equals the step without momentum except where a -0.0 seed became +0.0."""
    x = expected(pat_name, "signed", K)
    off = x.model.mstep(x.L0, x.R0, x.Lp, x.Rp, beta=(0.0, 0.0))
    assert_same_bits(off[0], x.nomom[0], "beta 0, L")
    assert_same_bits(off[1], x.nomom[1], "beta 0, R")
    assert_same_bits(x.rest1[0], x.nomom[0], "from rest, L")
    assert_same_bits(x.rest1[1], x.nomom[1], "from rest, R")
    assert_same_bits(x.unseeded[0], x.plain_unseeded[0], "an unseeded sweep takes no momentum")
    z = np.array([-0.0, 0.0, 1.5])
    assert is_negzero(z * 0.5)[0] and not is_negzero(seed_of(z, z, 0.5, 0.9)).any()   # (-0.0 * d) + (+0.0) is +0.0


def test_fma_sample_is_a_fused_multiply_add():
    # 0.1 * 0.1 rounds up to 0.010000000000000002; fused with -0.010000000000000002 the exact product's tail survives
    p = 0.1 * 0.1
    got = fma_sample(0.1, np.array([0.1]), np.array([-p]))[0]
    assert got != 0.0 and got == float(Fraction(0.1) * Fraction(0.1) - Fraction(p)) and 0.1 * 0.1 + -p == 0.0


def test_momentum_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in MOMENTUM_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr)
    assert capi.hip().mf_backend_abi_version() == 5
    for name in ("set_momentum", "momentum", "upload_previous", "download_previous"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_momentum) and callable(capi.run_momentum)


def test_momentum_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    a, b = C.c_double(), C.c_double()
    assert h.mf_plan_set_momentum(None, 0.0, 0.0) == capi.MF_ERR_ARGUMENT
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert h.mf_plan_set_momentum(fake, bad, 0.1) == capi.MF_ERR_ARGUMENT, bad
        assert h.mf_plan_set_momentum(fake, 0.1, bad) == capi.MF_ERR_ARGUMENT, bad
    assert h.mf_plan_get_momentum(None, C.byref(a), C.byref(b)) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_upload_previous(None, None, None) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_download_previous(None, None, None) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    assert h.mf_backend_run_momentum(None, L, R, None, 0.1, 0.1, 0.5, 0.5, 0) == capi.MF_ERR_ARGUMENT
    for bad in (-0.5, float("nan"), float("inf")):
        for args in ((bad, 0.1, 0.5, 0.5), (0.1, bad, 0.5, 0.5), (0.1, 0.1, bad, 0.5), (0.1, 0.1, 0.5, bad)):
            assert h.mf_backend_run_momentum(C.byref(p), L, R, None, *args, 0) == capi.MF_ERR_ARGUMENT, args
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


BAD_MOMENTUM = ["", "abc", "-1", "-0.5,0.1", "0.1,-2", "nan", "inf", "1e999", "0.1,", "0.1,x", "0.1x", "0.1,0.2,0.3", ",0.1"]
FORBIDDEN = [dict(MATFACT_DEVICES="0"), dict(MATFACT_MATS="/dev/null"), dict(MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_RESUME="x.ck"),
             dict(MATFACT_TOPN="3"), dict(MATFACT_SIMILAR="3", MATFACT_SIMILAR_OUT="sim.out")]


@pytest.mark.parametrize("env", [dict(MATFACT_MOMENTUM=v) for v in BAD_MOMENTUM] + [dict(e, MATFACT_MOMENTUM="0.9") for e in FORBIDDEN],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_momentum_refusals_die_with_empty_stdout(capi, env, tmp_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(clean, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_MOMENTUM" in r.stderr, r
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
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_all(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_all


def test_every_form_is_in_the_table():
    names = {c["name"] for c in CASES}
    assert names == {"reg", "reg-wide", "dma-ct", "dma-rt", "db", "pair", "long", "long-nodpp", "coop", "es-sw8", "es-sw4", "es-sw2"}
    assert len(CASES) == 2 * 2 * (len(names) - 1) + 2 * len(WIDE)      # both ends of every narrow row, and the wide rows
    assert {(c["name"], c["K"]) for c in CASES if c["pat"] == "wide"} == {("reg-wide", 513), ("reg-wide", 4095), ("dma-rt", 1024)}


def _plan(capi, x, K, lam=LAM, beta=BETA):
    pat = x.pat
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    plan.set_regularization(*lam)
    plan.set_momentum(*beta)
    return plan


def _step(plan, L0, R0, prev, seed_items, seed_users):
    plan.upload(L0, R0)
    if prev is not None:
        plan.upload_previous(*prev)
    plan.sweep_items(seed_from_old=seed_items)
    plan.sweep_users(seed_from_old=seed_users)
    plan.flip()
    return plan.download()


@gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_momentum_sweeps_through_every_form(device, switches, case):
    """With a chosen X_prev (upload_previous): the seeded item and user sweeps and one iterate(1) against the model; the
    unseeded sweeps are the plain unseeded bits.  From rest: two iterate(1) are two model iterations and download_previous
    is the model's first iterate -- in every sweep form, at the rule's chunk size and at 5."""
    capi = device
    K = case["K"]
    x = expected(case["pat"], "signed", K)
    switches(case["env"])
    if case["nch"]:
        switches({"MF_SWEEP_NCH": case["nch"]})
    plan = capi.Plan(x.pat.users, x.pat.items, K, x.alpha, x.pat.row, x.pat.col, x.val)
    try:
        assert plan.momentum() == (0.0, 0.0) and "momentum=" not in plan.describe()
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_momentum(BETA_U, BETA_I)
        desc = plan.describe()
        assert case["check"](desc, K), desc
        assert ("MF_SWEEP_NCH=5" in desc) == (case["nch"] == "5"), desc
        assert plan.momentum() == (BETA_U, BETA_I) and " momentum=0.9/0.3" in desc, desc
        where = "%s [%s]" % (_case_id(case), desc.split(" loss=")[0])
        if case["steps"]:
            L, R = _step(plan, x.L0, x.R0, (x.Lp, x.Rp), True, True)
            assert_same_bits(R, x.seeded[1], where + ": seeded item sweep")
            assert_same_bits(L, x.seeded[0], where + ": seeded user sweep")
            L, R = _step(plan, x.L0, x.R0, (x.Lp, x.Rp), False, False)
            assert_same_bits(R, x.plain_unseeded[1], where + ": item sweep from zero")
            assert_same_bits(L, x.plain_unseeded[0], where + ": user sweep from zero")
        plan.upload(x.L0, x.R0)
        plan.upload_previous(x.Lp, x.Rp)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.seeded[0], where + ": L after iterate(1) with a chosen history")
        assert_same_bits(R, x.seeded[1], where + ": R after iterate(1) with a chosen history")
        Lq, Rq = plan.download_previous()
        assert_same_bits(Lq, x.L0, where + ": the history after one iteration is the start, L")
        assert_same_bits(Rq, x.R0, where + ": the history after one iteration is the start, R")
        plan.upload(x.L0, x.R0)   # at rest again
        Lq, Rq = plan.download_previous()
        assert_same_bits(Lq, x.L0, where + ": a side at rest returns its current factors, L")
        assert_same_bits(Rq, x.R0, where + ": a side at rest returns its current factors, R")
        plan.iterate(1)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.rest2[0], where + ": L after two iterations from rest")
        assert_same_bits(R, x.rest2[1], where + ": R after two iterations from rest")
        Lq, Rq = plan.download_previous()
        assert_same_bits(Lq, x.rest1[0], where + ": previous L after two iterations")
        assert_same_bits(Rq, x.rest1[1], where + ": previous R after two iterations")
    finally:
        plan.close()


@gpu
def test_plain_momentum_instance_above_262144_rows(device, switches):
    """sweep_dma_kernel<10, 1, momentum> without the pipelined phases is what a momentum sweep of more than 262144 rows
    launches; no smaller launch reaches it.  One seeded and one unseeded step against the model, every row of both factors."""
    capi = device
    K = 10
    switches(SWEEPS)
    pat = pattern_both_large()
    assert min(pat.users, pat.items) > PF_ROWS
    L0, R0, val = signed_inputs(7000 + K, pat, K)
    Lp, Rp = random_prev(7100, L0), random_prev(7200, R0)
    alpha = 1e-3
    m = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_momentum(BETA_U, BETA_I)
        desc = plan.describe()
        assert " accumulate=plain/plain " in desc and _single_wave(desc, K, K) and " momentum=0.9/0.3" in desc, desc
        nomom = m.step(L0, R0, LAM_U, LAM_I)
        for seed in (True, False):
            want = m.mstep(L0, R0, Lp, Rp, seed_u=seed, seed_i=seed)
            if seed:
                assert differs(want[0], nomom[0]) > 0.5 and differs(want[1], nomom[1]) > 0.5
            L, R = _step(plan, L0, R0, (Lp, Rp), seed, seed)
            assert_same_bits(R, want[1], "item sweep, seed=%s" % seed)
            assert_same_bits(L, want[0], "user sweep, seed=%s" % seed)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("cls", ["signed", "zeros", "nonfinite"])
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("long", 30), ("es-sw4", 10)], ids=lambda v: str(v))
def test_first_step_from_rest(device, switches, name, K, cls):
    """From rest v = x - x: on signed inputs the first step is the regularised step without momentum bit for bit; on
    "zeros" a -0.0 seed comes out +0.0, (-0.0 * d) + (+0.0), and nothing else changes; on "nonfinite" inf - inf is NaN and
    NaN stays NaN, as the model says.  Then a second step, which has a history."""
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], cls, K)
    switches(case["env"])
    plan = _plan(capi, x, K)
    try:
        assert case["check"](plan.describe(), K), plan.describe()
        where = "%s K=%d %s" % (name, K, cls)
        if cls == "signed":
            assert_same_bits(x.rest1[0], x.nomom[0], where + ": the model from rest is the step without momentum, L")
            assert_same_bits(x.rest1[1], x.nomom[1], where + ": the model from rest is the step without momentum, R")
        if cls == "zeros":
            for got, ref in zip(x.rest1, x.nomom):
                moved = got.view(np.uint64) != ref.view(np.uint64)
                assert moved.any() and is_negzero(ref[moved]).all() and (got[moved] == 0.0).all() and not is_negzero(got[moved]).any(), where
        if cls == "nonfinite":
            assert np.isinf(x.L0).any() and np.isnan(x.rest1[0][np.isinf(x.L0)]).all(), where   # inf - inf
            assert np.isinf(x.R0).any() and np.isnan(x.rest1[1][np.isinf(x.R0)]).all(), where
        if case["steps"]:
            L, R = _step(plan, x.L0, x.R0, None, True, True)
            assert_same_bits(R, x.rest1[1], where + ": item sweep from rest")
            assert_same_bits(L, x.rest1[0], where + ": user sweep from rest")
        plan.upload(x.L0, x.R0)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.rest1[0], where + ": L after the first iteration")
        assert_same_bits(R, x.rest1[1], where + ": R after the first iteration")
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.rest2[0], where + ": L after the second iteration")
        assert_same_bits(R, x.rest2[1], where + ": R after the second iteration")
    finally:
        plan.close()


HISTORY_FORMS = [("dma-ct", 30), ("long", 30), ("es-sw4", 10), ("coop", 10)]


@gpu
@pytest.mark.parametrize("name,K", HISTORY_FORMS, ids=lambda v: str(v))
def test_history_rules(device, switches, name, K):
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], "signed", K)
    m = x.model
    switches(case["env"])

    def fresh(beta=BETA):
        p = _plan(capi, x, K, beta=beta)
        p.upload(x.L0, x.R0)
        return p

    def same(plan, want, where, prev=True):
        L, R = plan.download()
        assert_same_bits(L, want[0], where + ": L")
        assert_same_bits(R, want[1], where + ": R")
        if prev:
            Lq, Rq = plan.download_previous()
            assert_same_bits(Lq, want[2], where + ": previous L")
            assert_same_bits(Rq, want[3], where + ": previous R")
    where = "%s K=%d" % (name, K)
    # beta 0 keeps no history: a side whose beta leaves 0 starts at rest, from X_2
    plan = fresh(beta=(0.0, 0.0))
    try:
        plan.iterate(2)
        two = m.run(x.L0, x.R0, 2, beta=(0.0, 0.0))
        same(plan, two, where + " two plain iterations", prev=False)
        plan.set_momentum(BETA_U, BETA_I)
        Lq, Rq = plan.download_previous()
        assert_same_bits(Lq, two[0], where + ": at rest after set_momentum, L")
        assert_same_bits(Rq, two[1], where + ": at rest after set_momentum, R")
        plan.iterate(1)
        want = m.run(two[0], two[1], 1)
        assert differs(want[0], m.run(two[0], two[1], 1, prev=(two[2], two[3]))[0]) > 0.5   # the plain run's history would show
        same(plan, want, where + " first momentum iteration after two plain ones")
    finally:
        plan.close()
    # a change between two non-zero betas keeps the history; upload_factors resets it
    plan = fresh()
    try:
        plan.iterate(3)
        three = m.run(x.L0, x.R0, 3)
        same(plan, three, where + " three iterations")
        plan.set_momentum(0.6, 0.7)
        assert plan.momentum() == (0.6, 0.7) and " momentum=0.6/0.7" in plan.describe()
        plan.iterate(3)
        want = m.run(three[0], three[1], 3, beta=(0.6, 0.7), prev=(three[2], three[3]))
        assert differs(want[0], m.run(three[0], three[1], 3, beta=(0.6, 0.7))[0]) > 0.5   # at rest would show
        same(plan, want, where + " betas changed at 3")
        plan.upload(x.L0, x.R0)
        plan.set_momentum(BETA_U, BETA_I)
        plan.iterate(3)
        same(plan, three, where + " upload_factors resets the history")
    finally:
        plan.close()
    # iterate(3) + iterate(3) = iterate(6) = iterate_monitored(6, every=2); resume from the two downloaded generations
    six = m.run(x.L0, x.R0, 6)
    a, b, c, d = fresh(), fresh(), fresh(), None
    try:
        a.iterate(3)
        mid = a.download() + a.download_previous()
        a.iterate(3)
        same(a, six, where + " 3 + 3")
        b.iterate(6)
        same(b, six, where + " 6")
        done, pts = c.iterate_monitored(6, every=2)
        assert done == 6 and [p.iter for p in pts] == [0, 2, 4, 6]
        same(c, six, where + " monitored")
        d = _plan(capi, x, K)
        d.upload(mid[0], mid[1])
        d.upload_previous(mid[2], mid[3])
        d.iterate(3)
        same(d, six, where + " resumed")
    finally:
        for p in (a, b, c, d):
            if p is not None:
                p.close()


@gpu
@pytest.mark.parametrize("K", [3, 10, 30, 40])
def test_toy_single_launch_loop(device, switches, K):
    """iterate(5) then iterate(4) of a toy instance: nine model iterations, download_previous the eighth, with momentum on
    both sides and on one only.  Both calls are below the eight iterations from which one launch runs the whole loop, so
    this is the two-launch path carrying its history across calls; test_toy_loop_inside_one_launch has the single launch."""
    capi = device
    pat, L0, R0, val, alpha = _toy(K)
    m = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    for beta in (BETA, (0.0, BETA_I)):
        want = m.run(L0, R0, 9, beta=beta)
        assert differs(want[0], m.run(L0, R0, 9, beta=(0.0, 0.0))[0]) > 0.5
        for mode in (None, "0"):
            env = {} if mode is None else {"MF_RESIDENT": mode}
            switches(env)
            plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
            try:
                plan.set_regularization(LAM_U, LAM_I)
                plan.set_momentum(*beta)
                # a toy instance -- eight iterations would be one launch -- whose calls of five and of four are the sweeps
                loops = [path_of_plan(plan.describe(), pat, K, n, env)[0] for n in (8, 5, 4)]
                assert loops == ["toy" if mode is None else "sweeps", "sweeps", "sweeps"], loops
                plan.upload(L0, R0)
                plan.iterate(5)
                plan.iterate(4)
                L, R = plan.download()
                where = "K=%d MF_RESIDENT=%s beta=%s" % (K, mode, beta)
                assert_same_bits(L, want[0], where + " L")
                assert_same_bits(R, want[1], where + " R")
                Lq, Rq = plan.download_previous()
                if beta[0] != 0.0:
                    assert_same_bits(Lq, want[2], where + " previous L")
                assert_same_bits(Rq, want[3], where + " previous R")
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("K", [3, 10, 30, 40])
def test_toy_loop_inside_one_launch(device, switches, K):
    """mf_plan_iterate runs a toy instance's loop inside ONE launch from eight iterations on (sweep_resident_kernel<4 | 16 |
    32 | 0, momentum>); the launch takes its history from the next-generation buffers and leaves both generations behind.
    An odd count flips the generations, so the launch after it reads its history from the other buffer: iterate(8) +
    iterate(9) are 17 model iterations and download_previous the 16th; a chosen X_prev then iterate(9); iterate(9) +
    iterate(9) = iterate(18) = iterate_monitored(18, every=9); momentum on one side only.  MF_RESIDENT=0 (two launches per
    iteration) gives the same bits."""
    capi = device
    pat, L0, R0, val, alpha = _toy(K)
    m = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    Lp, Rp = random_prev(80 + K, L0), random_prev(90 + K, R0)

    def same(plan, want, where, beta=BETA):
        L, R = plan.download()
        assert_same_bits(L, want[0], where + " L")
        assert_same_bits(R, want[1], where + " R")
        Lq, Rq = plan.download_previous()
        if beta[0] != 0.0:   # a side with beta == 0 stays at rest: it returns its current factors
            assert_same_bits(Lq, want[2], where + " previous L")
        assert_same_bits(Rq, want[3], where + " previous R")
    w8, w17, w18 = m.run(L0, R0, 8), m.run(L0, R0, 17), m.run(L0, R0, 18)
    chosen = m.run(L0, R0, 9, prev=(Lp, Rp))
    assert differs(chosen[0], m.run(L0, R0, 9)[0]) > 0.5 and differs(chosen[1], m.run(L0, R0, 9)[1]) > 0.5   # from rest would show
    # a launch that took the current generation for its history (v = x - x in its first iteration) would show
    lost = m.run(w8[0], w8[1], 9)
    assert differs(w17[0], lost[0]) > 0.5 and differs(w17[1], lost[1]) > 0.5
    one_side = (0.0, BETA_I)
    o17 = m.run(L0, R0, 17, beta=one_side)
    for mode in (None, "0"):
        env = {} if mode is None else {"MF_RESIDENT": mode}
        switches(env)
        where = "K=%d MF_RESIDENT=%s" % (K, mode)

        def fresh(beta=BETA):
            p = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
            p.set_regularization(LAM_U, LAM_I)
            p.set_momentum(*beta)
            p.upload(L0, R0)
            # every count this test calls with (iterate_monitored(18, every=9) calls with 9): one launch, or the sweeps
            loops = {path_of_plan(p.describe(), pat, K, n, env)[0] for n in (8, 9)}
            assert loops == ({"toy"} if mode is None else {"sweeps"}), (where, loops)
            return p
        a, b, c, d, e = fresh(), fresh(), fresh(), fresh(), fresh(one_side)
        try:
            a.iterate(8)
            same(a, w8, where + " 8:")
            a.iterate(9)
            same(a, w17, where + " 8 + 9:")
            b.upload_previous(Lp, Rp)
            b.iterate(9)
            same(b, chosen, where + " chosen history, 9:")
            c.iterate(9)
            c.iterate(9)
            same(c, w18, where + " 9 + 9:")
            done, pts = d.iterate_monitored(18, every=9)
            assert done == 18 and [p.iter for p in pts] == [0, 9, 18]
            same(d, w18, where + " monitored(18, every=9):")
            e.iterate(8)
            e.iterate(9)
            same(e, o17, where + " one side, 8 + 9:", one_side)
        finally:
            for p in (a, b, c, d, e):
                p.close()


@gpu
@pytest.mark.parametrize("graph", [None, "0"])
def test_graph_replay_and_a_change_of_beta(device, switches, graph):
    """iterate(130) = four replays of a captured 32-iteration graph plus two eager iterations; the graph is captured per
    call, so the beta set between two calls is the one the second call runs with, on the first call's history."""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({"MF_ITER_MODE": "sweeps"})
    if graph:
        switches({"MF_GRAPH": graph})
    m = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    mid = m.run(L0, R0, 130)
    end = m.run(mid[0], mid[1], 130, beta=(0.2, 0.8), prev=(mid[2], mid[3]))
    assert differs(end[0], m.run(mid[0], mid[1], 130, prev=(mid[2], mid[3]))[0]) > 0.5
    assert differs(mid[0], m.run(L0, R0, 130, beta=(0.0, 0.0))[0]) > 0.5
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        assert ("MF_GRAPH=0" in plan.describe()) == (graph == "0"), plan.describe()
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_momentum(BETA_U, BETA_I)
        plan.upload(L0, R0)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, mid[0], "L after 130")
        assert_same_bits(R, mid[1], "R after 130")
        for bad in (float("nan"), -1.0, float("inf")):   # a refused value changes nothing on a live plan
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_momentum(bad, 0.1)
            assert err.value.status == capi.MF_ERR_ARGUMENT and plan.momentum() == (BETA_U, BETA_I)
            with pytest.raises(capi.HipBackendError):
                plan.set_momentum(0.1, bad)
            assert plan.momentum() == (BETA_U, BETA_I) and " momentum=0.9/0.3" in plan.describe()
        plan.set_momentum(0.2, 0.8)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, end[0], "L after 260, beta switched at 130")
        assert_same_bits(R, end[1], "R after 260, beta switched at 130")
        Lq, Rq = plan.download_previous()
        assert_same_bits(Lq, end[2], "previous L after 260")
        assert_same_bits(Rq, end[3], "previous R after 260")
    finally:
        plan.close()


@gpu
def test_upload_previous_without_factors_is_a_state_error(device):
    capi = device
    pat, L0, R0, val, alpha = _small()
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.set_momentum(0.5)   # legal before the upload
        assert plan.momentum() == (0.5, 0.5)
        for call in (lambda: plan.upload_previous(L0, R0), plan.download_previous):
            with pytest.raises(capi.HipBackendError) as err:
                call()
            assert err.value.status == capi.MF_ERR_STATE
        # one side given: the other stays at rest
        plan.upload(L0, R0)
        Rp = random_prev(1, R0)
        plan.upload_previous(None, Rp)
        Lq, Rq = plan.download_previous()
        assert_same_bits(Lq, L0, "users at rest")
        assert_same_bits(Rq, Rp, "items' history")
        plan.iterate(1)
        want = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha).mstep(L0, R0, None, Rp, lam=(0.0, 0.0), beta=(0.5, 0.5))
        L, R = plan.download()
        assert_same_bits(L, want[0], "L")
        assert_same_bits(R, want[1], "R")
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("name,K", [("reg", 3), ("dma-ct", 100), ("db", 64), ("pair", 100), ("long", 30), ("long-nodpp", 30), ("coop", 10), ("es-sw4", 10)],
                         ids=lambda v: str(v))
def test_frozen_columns_keep_their_bits_under_momentum(device, switches, name, K):
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], "signed", K)
    fu, fi = K - 1, K - 2
    switches(case["env"])
    plan = _plan(capi, x, K)
    try:
        plan.set_frozen_columns(fu, fi)
        assert case["check"](plan.describe(), K), plan.describe()
        want = x.model.run(x.L0, x.R0, 2, prev=(x.Lp, x.Rp), frozen=(fu, fi))
        one = x.model.mstep(x.L0, x.R0, x.Lp, x.Rp, frozen=(fu, fi))
        free = [k for k in range(K) if k != fu]
        assert_same_bits(one[0][:, free], x.seeded[0][:, free], "the free columns are those of the unfrozen step")
        assert differs(one[0][:, fu], x.seeded[0][:, fu]) > 0.5
        where = "%s K=%d" % (name, K)
        if case["steps"]:
            L, R = _step(plan, x.L0, x.R0, (x.Lp, x.Rp), True, True)
            assert_same_bits(L, one[0], where + ": seeded user sweep")
            assert_same_bits(R, one[1], where + ": seeded item sweep")
            L, R = _step(plan, x.L0, x.R0, (x.Lp, x.Rp), False, False)
            assert not L[:, fu].any() and not R[:, fi].any() and not is_negzero(L[:, fu]).any() and not is_negzero(R[:, fi]).any()
        plan.upload(x.L0, x.R0)
        plan.upload_previous(x.Lp, x.Rp)
        plan.iterate(1)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L[:, fu], x.L0[:, fu], where + ": the users' frozen column")
        assert_same_bits(R[:, fi], x.R0[:, fi], where + ": the items' frozen column")
        assert_same_bits(L, want[0], where + ": L after two iterations")
        assert_same_bits(R, want[1], where + ": R after two iterations")
    finally:
        plan.close()


def _cli(capi, path, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(clean, **env))


@gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "inst0"])
def test_cli_momentum(device, orc, name):
    """MATFACT_MOMENTUM alone, with MATFACT_LAMBDA, and with MATFACT_BIAS + MATFACT_LAMBDA (+ MATFACT_LOSS): stdout is the
    .out of the plan's own recommendation, and with MATFACT_LOSS=1 every stderr RMSE parses back (%.17g) to the bits of the
    plan's monitored loop."""
    capi = device
    path = golden_in(name)
    inst = capi.parse_file(path)
    oi = orc.parse_in(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    r = _cli(capi, path, MATFACT_MOMENTUM="0")
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLDEN, name + ".out"), "rb").read(), r
    m = MModel(inst.users, inst.items, inst.row, inst.col, inst.val, inst.alpha)
    for env, lam, beta in ((dict(MATFACT_MOMENTUM="0.9,0.3"), (0.0, 0.0), BETA), (dict(MATFACT_MOMENTUM="0.5", MATFACT_LAMBDA="0.05,0.3"), LAM, (0.5, 0.5))):
        Lm, Rm = m.run(L0, R0, inst.iters, lam=lam, beta=beta)[:2]
        r = _cli(capi, path, **env)
        assert r.returncode == 0 and r.stdout == orc.format_out(orc.recommend(oi, Lm, Rm)).encode(), (env, r)
    # the biased model under momentum: the plan session, with and without the monitored loop
    F = inst.feats
    mu = capi.bias_mean(inst.val)
    plan = capi.Plan(inst.users, inst.items, F + 2, inst.alpha, inst.row, inst.col, inst.val - mu)
    try:
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_frozen_columns(F + 1, F)
        plan.set_momentum(BETA_U, BETA_I)
        plan.upload(capi.bias_pack(L0, None, 1), capi.bias_pack(R0, None, 0))
        done, pts = plan.iterate_monitored(inst.iters, every=1)
        want = orc.format_out(plan.recommend()).encode()
    finally:
        plan.close()
    env = dict(MATFACT_BIAS="1", MATFACT_MOMENTUM="0.9,0.3", MATFACT_LAMBDA="0.05,0.3")
    r = _cli(capi, path, **env)
    assert r.returncode == 0 and r.stdout == want and r.stderr == b"", r
    r = _cli(capi, path, MATFACT_LOSS="1", **env)
    assert r.returncode == 0 and r.stdout == want, r
    lines = r.stderr.decode().splitlines()
    its = [ln.split() for ln in lines if ln.startswith("iter ")]
    assert done == inst.iters and [int(t[1]) for t in its] == [p.iter for p in pts] == list(range(inst.iters + 1))
    got = np.array([float(t[3]) for t in its])
    assert_same_bits(got, np.array([np.sqrt(p.train.sse / float(p.train.count)) for p in pts]), "train_rmse on stderr")
    assert lines[inst.iters + 1].startswith("bias mu ") and lines[inst.iters + 2].startswith("penalty lambda ")


@gpu
def test_two_user_shards_on_one_gpu(device, switches):
    """The item sweep is seeded on shard 0 only: that shard's items_next carries the whole seed -- decay and momentum, once
    --, the other's neither; the user blocks are the single plan's.
    This NARROWS what was asked for ("the sum equals the single-plan bits apart from the -0.0 case"): the sum of the two
    items_next adds the entries in the sharded run's order, ((seed + root's entries) + (0.0 + the other's entries)), not in the
    single plan's, so it cannot equal the single plan bit for bit wherever both shards rated an item.  What is compared: each
    shard's items_next and user block with the model of that shard, the user blocks with the single plan, and the sum with
    the single plan on the items rated in the root shard alone (+ 0.0 turns the single plan's -0.0 into the sum's +0.0)."""
    capi = device
    K, cut = 30, 333
    x = expected("pair", "signed", K)
    pat = x.pat
    assert cut % 1024 and 0 < cut < pat.users
    switches({"MF_ITER_MODE": "sweeps"})
    single = _plan(capi, x, K)
    Ls, Rs = _step(single, x.L0, x.R0, (x.Lp, x.Rp), True, True)
    single.close()
    assert_same_bits(Ls, x.seeded[0], "single plan, L")
    assert_same_bits(Rs, x.seeded[1], "single plan, R")
    lo = pat.row < cut
    parts = []
    for sel, begin, count, seeded in ((lo, 0, cut, True), (~lo, cut, pat.users - cut, False)):
        row, col, val = pat.row[sel], pat.col[sel], x.val[sel]
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, row, col, val, user_begin=begin, user_count=count)
        try:
            plan.set_regularization(LAM_U, LAM_I)
            plan.set_momentum(BETA_U, BETA_I)
            Lb, Rn = _step(plan, x.L0[begin:begin + count], x.R0, (x.Lp[begin:begin + count], x.Rp), seeded, True)
        finally:
            plan.close()
        m = MModel(count, pat.items, row - begin, col, val, x.alpha)
        Lm, Rm = m.mstep(x.L0[begin:begin + count], x.R0, x.Lp[begin:begin + count], x.Rp, seed_i=seeded)
        assert_same_bits(Rn, Rm, "shard at %d: items_next" % begin)
        assert_same_bits(Lb, Lm, "shard at %d: user block against the model" % begin)
        assert_same_bits(Lb, Ls[begin:begin + count], "shard at %d: user block against the single plan" % begin)
        parts.append(Rn)
    # the root's seed is the single plan's: items nobody in the other shard rated come out with the single plan's bits
    alone = np.bincount(pat.col[~lo], minlength=pat.items) == 0
    assert alone.any()
    assert_same_bits((parts[0] + parts[1])[alone], Rs[alone] + 0.0, "items rated in the root shard only")


@gpu
def test_backend_run_momentum(device):
    capi = device
    pat, L0, R0, val, alpha = _small()
    inst = capi.Instance(40, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.upload(L0, R0)
        plan.set_regularization(LAM_U, LAM_I)
        plan.set_momentum(BETA_U, BETA_I)
        plan.iterate(40)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    L, R = L0.copy(), R0.copy()
    best = capi.backend_run_momentum(inst, L, R, LAM_U, LAM_I, BETA_U, BETA_I)
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    want = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha).run(L0, R0, 40)
    assert_same_bits(L, want[0], "L against the model")
    assert_same_bits(R, want[1], "R against the model")
    L2, R2 = L0.copy(), R0.copy()
    assert capi.backend_run_momentum(inst, L2, R2, LAM_U, LAM_I, BETA_U, BETA_I, recommend=False) is None
    assert_same_bits(L2, Lp, "L without a recommendation")
    La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
    b0 = capi.backend_run_momentum(inst, La, Ra, LAM_U, LAM_I, 0.0)
    b1 = capi.backend_run_reg(inst, Lb, Rb, LAM_U, LAM_I)
    assert_same_bits(La, Lb, "beta 0: L of mf_backend_run_reg")
    assert_same_bits(Ra, Rb, "beta 0: R of mf_backend_run_reg")
    assert np.array_equal(b0, b1)


@gpu
@pytest.mark.parametrize("name,K", ZERO_FORMS, ids=lambda v: str(v))
def test_momentum_off_is_the_plain_library(device, orc, switches, name, K):
    """a plan that sets and then clears momentum gives the oracle's bits"""
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
        plan.set_momentum(BETA_U, BETA_I)
        plan.upload(L0, R0)
        plan.iterate(1)   # a momentum iteration in between: the history it leaves must not show afterwards
        plan.set_momentum(0.0, 0.0)
        desc = plan.describe()
        assert case["check"](desc, K) and "momentum=" not in desc, desc
        if case["steps"]:
            plan.upload(L0, R0)
            plan.upload_previous(random_prev(1, L0), random_prev(2, R0))
            plan.sweep_items()
            plan.sweep_users()
            plan.flip()
            L, R = plan.download()
            assert_same_bits(L, seeded[0], "%s L" % name)
            assert_same_bits(R, seeded[1], "%s R" % name)
        plan.upload(L0, R0)
        plan.iterate(2)
        L, R = plan.download()
        assert_same_bits(L, L2, "%s L after two" % name)
        assert_same_bits(R, R2, "%s R after two" % name)
    finally:
        plan.close()


@gpu
def test_momentum_converges_faster_on_ml100k(device, switches):
    """The feature's purpose, loosely: on ML100k from the reference's initialisation the training RMSE after 100 iterations
    at beta = 0.9 / 0.9 is below that after 400 plain iterations (a CPU float model gives 0.84 against 0.92)."""
    capi = device
    switches({})
    inst = capi.parse_file(golden_in("instML100k"))
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    rmse = {}
    for beta, iters in ((0.0, 400), (0.9, 100)):
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
        try:
            plan.set_momentum(beta)
            plan.upload(L0, R0)
            plan.iterate(iters)
            lo = plan.loss("train")
            rmse[beta] = float(np.sqrt(lo.sse / float(lo.count)))
        finally:
            plan.close()
    print("training RMSE: 400 plain iterations %.4f, 100 at beta 0.9 %.4f" % (rmse[0.0], rmse[0.9]))
    assert rmse[0.9] < rmse[0.0], rmse
