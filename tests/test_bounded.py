"""Box-constrained factors (mf_plan_set_bounds, mf_plan_get_bounds, mf_plan_project, mf_plan_bounds_active,
mf_backend_run_bounded, MATFACT_BOUNDS).

The definition is the library's own (include/matfact_hip.h): a seeded sweep finishes each row as without bounds -- seed, decay,
momentum, every e_n * Y in order -- and then every bounded column k < columns that is not the side's frozen column goes
through  if (y < lo) y = lo;  if (y > hi) y = hi;  with IEEE comparisons: a NaN stays the NaN it is, -0.0 stays under lo = 0.0,
a value equal to a bound keeps its bits.  An unseeded sweep does not project.  The model is the models of test_regularised,
test_frozen, test_momentum and test_weighted plus one function, clip(); every GPU comparison is bit for bit.
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
from test_frozen import pack, seq_mean
from test_momentum import BETA, MModel
from test_regularised import CASES, LAM_I, LAM_U, LARGE, WIDE, ZERO_FORMS, _case_id, _pick, _small, _step, _toy, differs, fast_dot
from test_regularised import expected as reg_expected
from test_sweep_edges import (CLASSES, GRID_CAP, PF_ROWS, SWITCHES, _single_wave, assert_same_bits, cls_signed, is_negzero, pattern,
                              seq_dot, signed_inputs)
from test_weighted import WModel, plain_weights

gpu = pytest.mark.gpu

LAM = (LAM_U, LAM_I)
LO, HI = 0.0, 0.5
INF = float("inf")
BOX = (LO, HI, -1)            # one side's bounds: (lo, hi, columns)
NO_BOX = (-INF, INF, -1)
NO_BETA = (0.0, 0.0)
NOT_FROZEN = (-1, -1)


# ------------------------------------------------------------------------------------------------ the model
def clip(new, lo, hi, columns, frozen, seeded):
    """the one function on top of the other files' models: the bounded columns of a seeded result, but the frozen one, are
    projected onto [lo, hi] by two comparisons and two selects"""
    if not seeded:
        return new
    n = new.shape[1] if columns < 0 else columns
    out = np.array(new)
    y = out[:, :n]
    y = np.where(y < lo, lo, y)
    y = np.where(y > hi, hi, y)
    if 0 <= frozen < n:
        y[:, frozen] = new[:, frozen]
    out[:, :n] = y
    return out


def bstep(m, L, R, bounds, Lp=None, Rp=None, lam=LAM, beta=NO_BETA, frozen=NOT_FROZEN, seed_u=True, seed_i=True, dot=seq_dot):
    """(L_new, R_new) of one iteration; bounds, lam, beta and frozen are (users, items), a side's bounds (lo, hi, columns)"""
    with np.errstate(all="ignore"):
        if isinstance(m, WModel):
            Ln, Rn = m.wstep(L, R, Lp, Rp, lam, beta, seed_u, seed_i, dot, frozen)
        else:
            Ln, Rn = m.mstep(L, R, Lp, Rp, lam, beta, seed_u, seed_i, dot, frozen)
        return clip(Ln, *bounds[0], frozen[0], seed_u), clip(Rn, *bounds[1], frozen[1], seed_i)


def brun(m, L, R, iters, bounds, lam=LAM, beta=NO_BETA, frozen=NOT_FROZEN):
    """`iters` iterations from rest; returns (L, R)"""
    Lp = Rp = None
    for _ in range(iters):
        Ln, Rn = bstep(m, L, R, bounds, Lp, Rp, lam, beta, frozen, dot=fast_dot)
        Lp, Rp, L, R = L, R, Ln, Rn
    return L, R


def counts(X, lo, hi, columns, frozen=-1):
    """(at_lo, at_hi, inside) over the bounded, non-frozen columns"""
    n = X.shape[1] if columns < 0 else columns
    keep = [k for k in range(n) if k != frozen]
    y = X[:, keep]
    with np.errstate(all="ignore"):
        return int((y == lo).sum()), int((y == hi).sum()), int(((y > lo) & (y < hi)).sum())


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def from_bits(b):
    return np.array([b], np.uint64).view(np.float64)[0]


NAN_A, NAN_B = from_bits(0x7FF8000000000123), from_bits(0xFFF8000000000456)   # two quiet NaNs with payloads
SPECIALS = np.array([NAN_A, INF, -INF, 0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1030, -2.0 ** -1030, LO, HI, np.nextafter(LO, -INF),
                     np.nextafter(LO, INF), np.nextafter(HI, -INF), np.nextafter(HI, INF), NAN_B, 0.25, -0.25, 0.75, 1e308, -1e308])


def hand_made(rows, K, shift=0):
    """rows x K, the specials in turn: every column meets many of them"""
    idx = (np.arange(rows * K) + shift) % len(SPECIALS)
    return np.ascontiguousarray(SPECIALS[idx].reshape(rows, K))


@functools.lru_cache(maxsize=None)
def expected(pat_name, cls, K, bu=BOX, bi=BOX, fu=-1, fi=-1):
    """test_regularised's inputs of one (pattern, class, K), and the bounded model's results on them."""
    base = reg_expected(pat_name, cls, K)
    x = type("BoundedExpected", (), {})()
    pat = x.pat = base.pat
    x.K, x.L0, x.R0, x.val, x.alpha = K, base.L0, base.R0, base.val, base.alpha
    m = x.model = MModel(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha)
    bounds, frozen = (bu, bi), (fu, fi)
    x.free = bstep(m, x.L0, x.R0, (NO_BOX, NO_BOX), frozen=frozen)
    x.seeded = bstep(m, x.L0, x.R0, bounds, frozen=frozen)
    x.unseeded = bstep(m, x.L0, x.R0, bounds, frozen=frozen, seed_u=False, seed_i=False)
    x.two = bstep(m, *x.seeded, bounds, frozen=frozen)
    return x


def check_guards(x, where):
    """on the model's results: each factor has at least a tenth of its elements clamped to lo, a tenth to hi and a tenth left
    alone, and the unseeded result holds elements outside the box"""
    for free, un in zip(x.free, x.unseeded):
        with np.errstate(all="ignore"):
            low, high = float((free < LO).mean()), float((free > HI).mean())
            alone = float(((free >= LO) & (free <= HI)).mean())
            outside = int(((un < LO) | (un > HI)).sum())
        assert low >= 0.10 and high >= 0.10 and alone >= 0.10, (where, low, high, alone)
        assert outside > 0, where


# ------------------------------------------------------------------------------------------------ CPU
BOUNDS_SYMBOLS = ("mf_plan_set_bounds", "mf_plan_get_bounds", "mf_plan_project", "mf_plan_bounds_active", "mf_backend_run_bounded")


def test_bounds_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in BOUNDS_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr) and "typedef struct mf_bounds" in hdr
    assert capi.hip().mf_backend_abi_version() == 5
    for name in ("set_bounds", "bounds", "project", "bounds_active"):
        assert callable(getattr(capi.Plan, name))
    assert callable(capi.backend_run_bounded) and C.sizeof(capi.Bounds) == 24


def test_bounds_argument_errors_come_before_any_hip_call(capi):
    """A NaN bound, lo > hi, columns < -1, an unknown side or generation and NULL are refused without a device.  columns > K
    can only be told with a plan, which needs a device: test_bounds_on_a_live_plan."""
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    nan = float("nan")
    lo, hi, n = C.c_double(), C.c_double(), C.c_int32()
    a = C.c_int64()
    assert h.mf_plan_set_bounds(None, 0, 0.0, 1.0, -1) == capi.MF_ERR_ARGUMENT
    for bad in ((nan, 1.0, -1), (0.0, nan, -1), (nan, nan, -1), (1.0, 0.0, -1), (INF, -INF, -1), (0.0, 1.0, -2), (0.0, 1.0, -(2 ** 31))):
        for side in (0, 1):
            assert h.mf_plan_set_bounds(fake, side, *bad) == capi.MF_ERR_ARGUMENT, bad
    for side in (-1, 2, 7):
        assert h.mf_plan_set_bounds(fake, side, 0.0, 1.0, -1) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_get_bounds(fake, side, C.byref(lo), C.byref(hi), C.byref(n)) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_project(fake, side, 0) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_bounds_active(fake, side, C.byref(a), None, None) == capi.MF_ERR_ARGUMENT
    for gen in (-1, 2):
        assert h.mf_plan_project(fake, 0, gen) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_get_bounds(None, 0, C.byref(lo), C.byref(hi), C.byref(n)) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_project(None, 0, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_bounds_active(None, 0, C.byref(a), None, None) == capi.MF_ERR_ARGUMENT


def test_a_refused_level_1_call_touches_nothing(capi):
    h = capi.hip()
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    good = capi.Bounds(0.0, 1.0, -1)
    nan = float("nan")

    def run(bu, bi, lam=0.1, beta=0.0, prob=p, Lx=L):
        return h.mf_backend_run_bounded(C.byref(prob) if prob is not None else None, None, Lx.ctypes.data if Lx is not None else None,
                                        R.ctypes.data, None, lam, 0.1, beta, 0.0, C.byref(bu) if bu is not None else None,
                                        C.byref(bi) if bi is not None else None, 0)
    for bad in (capi.Bounds(nan, 1.0, -1), capi.Bounds(0.0, nan, -1), capi.Bounds(1.0, 0.0, -1), capi.Bounds(0.0, 1.0, -2),
                capi.Bounds(0.0, 1.0, inst.feats + 1)):
        assert run(bad, good) == capi.MF_ERR_ARGUMENT and run(good, bad) == capi.MF_ERR_ARGUMENT and run(None, bad) == capi.MF_ERR_ARGUMENT
    assert run(good, good, lam=-1.0) == capi.MF_ERR_ARGUMENT and run(good, good, beta=nan) == capi.MF_ERR_ARGUMENT
    assert run(good, good, prob=None) == capi.MF_ERR_ARGUMENT and run(good, good, Lx=None) == capi.MF_ERR_ARGUMENT
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)


BAD_BOUNDS = ["", "abc", "0", "0,", ",1", "0,x", "0,1x", "1,0", "nan,1", "0,nan", "0,1,2", "0,1,2,", "0,1,3,2", "0,1,nan,2", "0,1,2,3,4",
              "inf,-inf", "0;1"]
FORBIDDEN = [dict(MATFACT_DEVICES="0"), dict(MATFACT_MATS="/dev/null"), dict(MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_RESUME="x.ck"),
             dict(MATFACT_TOPN="3"), dict(MATFACT_SIMILAR="3", MATFACT_SIMILAR_OUT="sim.out")]


@pytest.mark.parametrize("env", [dict(MATFACT_BOUNDS=v) for v in BAD_BOUNDS] + [dict(e, MATFACT_BOUNDS="0,inf") for e in FORBIDDEN],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_bounds_refusals_die_with_empty_stdout(capi, env, tmp_path):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, golden_in("inst0")], capture_output=True, cwd=tmp_path, env=dict(clean, **env))
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_BOUNDS" in r.stderr, r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("K", [3, 6, 100])
@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed"])
def test_model_at_default_bounds_is_the_regularised_model(pat_name, K):
    """This tests the model: with the default bounds, and with any infinite bounds over any columns, it is test_regularised's
    model bit for bit, seeded and unseeded; with [0, 0.5] it is not, and the guards of the GPU tests hold."""
    base = reg_expected(pat_name, "signed", K)
    x = expected(pat_name, "signed", K)
    for got, want, what in ((x.free, base.seeded, "seeded"), (x.unseeded, base.unseeded, "unseeded")):
        assert_same_bits(got[0], want[0], "%s K=%d %s L" % (pat_name, K, what))
        assert_same_bits(got[1], want[1], "%s K=%d %s R" % (pat_name, K, what))
    some = bstep(x.model, x.L0, x.R0, ((-INF, INF, K // 2), (-INF, INF, 0)))
    assert_same_bits(some[0], base.seeded[0], "infinite bounds over some columns, L")
    assert_same_bits(some[1], base.seeded[1], "infinite bounds over no column, R")
    assert differs(x.seeded[0], base.seeded[0]) > 0.5 and differs(x.seeded[1], base.seeded[1]) > 0.5
    check_guards(x, (pat_name, K))
    for X in x.seeded + x.two:
        assert X.min() >= LO and X.max() <= HI


def test_clip_on_a_hand_made_matrix():
    """NaN, +-inf, +-0.0, subnormals, the bounds and their neighbours one ulp away, element by element against the definition
    written as a loop; the frozen column and the columns from `columns` on keep their bits."""
    X = hand_made(9, 7)
    for lo, hi in ((LO, HI), (0.25, HI), (-INF, HI), (LO, INF), (HI, HI)):
        for columns, frozen in ((-1, -1), (7, 3), (5, 3), (5, 6), (0, -1), (1, 0)):
            got = clip(X, lo, hi, columns, frozen, True)
            n = 7 if columns < 0 else columns
            for r in range(9):
                for k in range(7):
                    y = X[r, k]
                    if k < n and k != frozen:
                        if y < lo:
                            y = lo
                        if y > hi:
                            y = hi
                    assert bits(got[r, k]) == bits(y), (lo, hi, columns, frozen, r, k)
            assert clip(X, lo, hi, columns, frozen, False) is X
    got = clip(SPECIALS[None, :], LO, HI, -1, -1, True)[0]
    want = {0: NAN_A, 15: NAN_B, 1: HI, 2: LO, 3: 0.0, 4: -0.0, 5: 5e-324, 6: LO, 9: LO, 10: HI, 11: LO, 12: 5e-324,
            13: np.nextafter(HI, -INF), 14: HI, 19: HI, 20: LO}
    for at, v in want.items():
        assert bits(got[at]) == bits(v), (at, got[at], v)
    assert counts(SPECIALS[None, :], LO, HI, -1) == (3, 1, 5)   # +0.0, -0.0 and lo itself; hi; NaN in none of the three


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


def _bounded_plan(capi, pat, K, val, alpha, bounds, lam=LAM, beta=NO_BETA, frozen=NOT_FROZEN, **kw):
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val, **kw)
    plan.set_regularization(*lam)
    plan.set_momentum(*beta)
    plan.set_frozen_columns(*frozen)
    plan.set_bounds("users", *bounds[0])
    plan.set_bounds("items", *bounds[1])
    return plan


def _describe_bounds(bounds, K):
    def side(b):
        lo, hi, n = b
        if (lo == -INF and hi == INF) or n == 0:
            return "-"
        return "[%s,%s]x%d" % (("%.17g" % lo), ("%.17g" % hi), K if n < 0 else n)
    if side(bounds[0]) == "-" and side(bounds[1]) == "-":
        return None
    return " bounds=%s/%s" % (side(bounds[0]), side(bounds[1]))


def run_form(capi, switches, case, x, bounds, frozen=NOT_FROZEN):
    """one seeded step, one unseeded step and two iterate(1) of a plan in the form of `case`, against the model"""
    K, pat = case["K"], x.pat
    switches(case["env"])
    if case.get("nch"):
        switches({"MF_SWEEP_NCH": case["nch"]})
    plan = _bounded_plan(capi, pat, K, x.val, x.alpha, bounds, frozen=frozen)
    try:
        desc = plan.describe()
        assert case["check"](desc, K), desc
        want = _describe_bounds(bounds, K)
        assert (want in desc) if want else ("bounds=" not in desc), desc
        where = "%s [%s]" % (_case_id(case) if "nch" in case else "%s-K%d" % (case["name"], K), desc.split(" loss=")[0])
        if case["steps"]:
            L, R = _step(plan, x.L0, x.R0, True, True)
            assert_same_bits(R, x.seeded[1], where + ": seeded item sweep")
            assert_same_bits(L, x.seeded[0], where + ": seeded user sweep")
            L, R = _step(plan, x.L0, x.R0, False, False)
            assert_same_bits(R, x.unseeded[1], where + ": item sweep from zero")
            assert_same_bits(L, x.unseeded[0], where + ": user sweep from zero")
        plan.upload(x.L0, x.R0)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.seeded[0], where + ": L after one iteration")
        assert_same_bits(R, x.seeded[1], where + ": R after one iteration")
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.two[0], where + ": L after two iterations")
        assert_same_bits(R, x.two[1], where + ": R after two iterations")
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_bounded_sweeps_through_every_form(device, switches, case):
    """1. [0, 0.5] on both sides at LAM_U / LAM_I in every sweep form, at the rule's chunk size and at 5: a seeded step is
    projected, an unseeded one is not, a second seeded step starts from projected factors."""
    x = expected(case["pat"], "signed", case["K"])
    check_guards(x, _case_id(case))
    run_form(device, switches, case, x, (BOX, BOX))


COLUMN_FORMS = [("reg", 3), ("reg", 129), ("dma-ct", 100), ("dma-ct", 256), ("dma-rt", 6), ("db", 64), ("pair", 100), ("long", 30),
                ("long-nodpp", 30), ("coop", 10), ("es-sw8", 64), ("es-sw4", 10)] + WIDE


@gpu
@pytest.mark.parametrize("name,K", COLUMN_FORMS, ids=lambda v: str(v))
def test_columns_and_frozen(device, switches, name, K):
    """2. columns = K - 2 with the frozen columns of the biased layout (users K - 1, items K - 2: both outside the range);
    columns = K with those frozen columns inside the range -- their old values lie outside the box in more than half of the
    rows and are kept --; columns = 0 (nothing is projected) on one side and K on the other."""
    case = _pick(name, K)
    F = K - 2
    for bu, bi, fu, fi in (((LO, HI, F), (LO, HI, F), F + 1, F), ((LO, HI, K), (LO, HI, K), F + 1, F), ((LO, HI, 0), (LO, HI, K), -1, -1),
                           ((LO, HI, K), (LO, HI, 0), 0, -1)):
        x = expected(case["pat"], "signed", K, bu, bi, fu, fi)
        for new, old, free, b, f in ((x.seeded[0], x.L0, x.free[0], bu, fu), (x.seeded[1], x.R0, x.free[1], bi, fi)):
            n = b[2]
            assert new[:, :n].size == 0 or (np.delete(new[:, :n], f, axis=1) if 0 <= f < n else new[:, :n]).max() <= HI
            if n < K:
                assert_same_bits(new[:, n:], free[:, n:], "the model leaves the unbounded columns alone")
                assert n == K - 1 or ((free[:, n:] < LO) | (free[:, n:] > HI)).mean() > 0.5
            if f >= 0:
                assert_same_bits(new[:, f], old[:, f], "the model keeps the frozen column")
                assert ((old[:, f] < LO) | (old[:, f] > HI)).mean() > 0.5
        run_form(device, switches, case, x, (bu, bi), (fu, fi))


@gpu
@pytest.mark.parametrize("cls", ["zeros", "nonfinite", "subnormal-users", "subnormal-items"])
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("long", 30), ("es-sw4", 10), ("reg", 7)], ids=lambda v: str(v))
def test_special_values_through_the_clamp(device, switches, name, K, cls):
    """3. NaN stays NaN, -0.0 stays -0.0 under lo = 0.0, subnormals stay: one seeded step (and the rest of run_form)."""
    case = _pick(name, K)
    x = expected(case["pat"], cls, K)
    if cls == "nonfinite":
        assert np.isnan(x.seeded[0]).any() and np.isnan(x.seeded[1]).any()
        for new, free in zip(x.seeded, x.free):
            assert np.array_equal(np.isnan(new), np.isnan(free))      # the clamp neither makes nor removes a NaN
            assert not np.isinf(new).any() and np.isinf(free).any()   # and every infinity went to a bound
    if cls == "zeros":
        assert is_negzero(x.seeded[0]).sum() >= 10 and np.array_equal(is_negzero(x.seeded[0]), is_negzero(x.free[0]))
    run_form(device, switches, case, x, (BOX, BOX))


@gpu
@pytest.mark.parametrize("lo,hi", [(LO, HI), (0.25, HI), (-INF, HI), (LO, INF)], ids=lambda v: str(v))
def test_project_on_the_hand_made_matrix(device, switches, lo, hi):
    """3. mf_plan_project on the hand-made matrix of the CPU test, uploaded as factors into caller-owned buffers whose pitch is
    wider than K: every special value comes back as clip() gives it, bit for bit (NaN payloads included), the frozen column
    and the unbounded columns keep their bits, the other generation is untouched and the padding is still +0.0."""
    import torch
    capi = device
    K = 10
    pat, _, _, val, alpha = _toy(K)
    ld = capi.row_pitch(K)
    assert ld > K
    dev = torch.device("cuda", 0)
    rb = [torch.zeros((pat.items, ld), dtype=torch.float64, device=dev) for _ in range(2)]
    lb = [torch.zeros((pat.users, ld), dtype=torch.float64, device=dev) for _ in range(2)]
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val, items_ext=[t.data_ptr() for t in rb], items_pitch=ld,
                     users_ext=[t.data_ptr() for t in lb], users_pitch=ld)
    try:
        assert plan.pitches() == (ld, ld)
        assert capi.hip().mf_plan_project(plan._h, 0, 0) == capi.MF_ERR_STATE   # no factors yet
        assert capi.hip().mf_plan_bounds_active(plan._h, 0, None, None, None) == capi.MF_ERR_STATE
        Lh, Rh = hand_made(pat.users, K), hand_made(pat.items, K, 5)
        plan.upload(Lh, Rh)
        plan.set_frozen_columns(4, -1)
        plan.set_bounds("users", lo, hi, 7)
        plan.set_bounds("items", lo, hi, -1)
        cur_l = next(t for t in lb if t.data_ptr() == plan.users_current_ptr())
        cur_r = next(t for t in rb if t.data_ptr() == plan.items_current_ptr())
        nxt_r = next(t for t in rb if t.data_ptr() == plan.items_next_ptr())
        nxt_r[:, :K] = torch.from_numpy(Rh)
        torch.cuda.synchronize()   # torch's stream wrote the buffer; the plan's own (non-blocking) stream projects it
        plan.project("users")
        plan.project("items", "next")
        plan.synchronize()
        L, R = plan.download()
        assert np.array_equal(bits(L), bits(clip(Lh, lo, hi, 7, 4, True))), "current users"
        assert np.array_equal(bits(R), bits(Rh)), "current items are not the buffer that was projected"
        assert np.array_equal(bits(nxt_r[:, :K].cpu().numpy()), bits(clip(Rh, lo, hi, -1, -1, True))), "next items"
        assert np.array_equal(bits(cur_l[:, :K].cpu().numpy()), bits(L)) and np.array_equal(bits(cur_r[:, :K].cpu().numpy()), bits(R))
        for t in lb + rb:
            assert not bits(t[:, K:].cpu().numpy()).any(), "padding"
        assert plan.bounds_active("users") == counts(L, lo, hi, 7, 4)
        plan.project("items")
        assert plan.bounds_active("items") == counts(clip(Rh, lo, hi, -1, -1, True), lo, hi, -1)
    finally:
        plan.close()


MOMENTUM_FORMS = [("reg", 3), ("dma-ct", 30), ("dma-ct", 100), ("db", 64), ("pair", 100), ("long", 30), ("long-nodpp", 30), ("coop", 10),
                  ("es-sw4", 10)] + WIDE


@gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["momentum", "momentum+weights"])
@pytest.mark.parametrize("name,K", MOMENTUM_FORMS, ids=lambda v: str(v))
def test_bounds_with_momentum_and_weights(device, switches, name, K, weighted):
    """4. the MOM and WGT instances: three iterations from rest under momentum -- X_prev and X_old are projected values -- and
    with per-entry weights on top; ("long", 30) runs the seed-preparation launch of the extreme rows, which does not project."""
    capi = device
    case = _pick(name, K)
    base = reg_expected(case["pat"], "signed", K)
    pat = base.pat
    w = plain_weights(9100 + K, pat.nnz) if weighted else None
    m = WModel(pat.users, pat.items, pat.row, pat.col, base.val, base.alpha, w) if weighted else \
        MModel(pat.users, pat.items, pat.row, pat.col, base.val, base.alpha)
    want, L, R, Lp, Rp = [], base.L0, base.R0, None, None
    for _ in range(3):
        Ln, Rn = bstep(m, L, R, (BOX, BOX), Lp, Rp, LAM, BETA)
        Lp, Rp, L, R = L, R, Ln, Rn
        want.append((L, R))
    free = m.wstep(base.L0, base.R0, None, None, LAM, BETA) if weighted else m.mstep(base.L0, base.R0, None, None, LAM, BETA)
    third_without_history = bstep(m, *want[1], (BOX, BOX), None, None, LAM, BETA)
    assert differs(want[0][0], free[0]) > 0.5 and differs(want[2][0], third_without_history[0]) > 0.1
    switches(case["env"])
    plan = _bounded_plan(capi, pat, K, base.val, base.alpha, (BOX, BOX), beta=BETA, weight=w)
    try:
        desc = plan.describe()
        assert case["check"](desc, K) and " momentum=" in desc and (" weighted=1" in desc) == weighted, desc
        plan.upload(base.L0, base.R0)
        for it in range(3):
            plan.iterate(1)
            L, R = plan.download()
            assert_same_bits(L, want[it][0], "%s K=%d: L after %d" % (name, K, it + 1))
            assert_same_bits(R, want[it][1], "%s K=%d: R after %d" % (name, K, it + 1))
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("mode", ["decay", "momentum", "weights", "momentum+weights"])
@pytest.mark.parametrize("K", [3, 10, 30, 40])
def test_toy_loop_inside_one_launch(device, switches, K, mode):
    """4. iterate(9) of a toy instance runs inside one launch (sweep_resident_kernel: K <= 4, <= 16, <= 32 and the generic form,
    each in its plain, MOM and WGT instances): the model's bits and the bits of the two-launch path (MF_RESIDENT=0); columns
    K - 1 on the users, a frozen column inside the items' range."""
    capi = device
    pat, L0, R0, val, alpha = _toy(K)
    beta = BETA if "momentum" in mode else NO_BETA
    w = plain_weights(77 + K, pat.nnz) if "weights" in mode else None
    m = WModel(pat.users, pat.items, pat.row, pat.col, val, alpha, w) if w is not None else MModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    bounds, frozen = ((LO, HI, K - 1), BOX), (-1, 1)
    want = brun(m, L0, R0, 9, bounds, LAM, beta, frozen)
    assert differs(want[0], brun(m, L0, R0, 9, (NO_BOX, NO_BOX), LAM, beta, frozen)[0]) > 0.3
    for resident in (None, "0"):
        env = {} if resident is None else {"MF_RESIDENT": resident}
        switches(env)
        plan = _bounded_plan(capi, pat, K, val, alpha, bounds, beta=beta, frozen=frozen, weight=w)
        try:
            loop = path_of_plan(plan.describe(), pat, K, 9, env, weighted=w is not None)[0]
            assert loop == ("toy" if resident is None else "sweeps"), (K, mode, resident, loop)
            plan.upload(L0, R0)
            plan.iterate(9)
            L, R = plan.download()
            assert_same_bits(L, want[0], "K=%d %s MF_RESIDENT=%s L" % (K, mode, resident))
            assert_same_bits(R, want[1], "K=%d %s MF_RESIDENT=%s R" % (K, mode, resident))
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("name", ["both-K10", "users-2^20-K10"])
def test_plain_decay_instances_above_262144_rows(device, switches, name):
    """5. sweep_dma_kernel<K, 1, decay> without the pipelined phases is what a bounded sweep of more than 262144 rows launches;
    no smaller launch reaches it.  One seeded and one unseeded step against the model, every row of both factors."""
    capi = device
    K, env, make, form = LARGE[name]
    switches(env)
    pat = make()
    assert max(pat.users, pat.items) > PF_ROWS and (name != "users-2^20-K10" or pat.users > GRID_CAP)
    L0, R0, val = signed_inputs(7000 + K, pat, K)
    alpha = 1e-3
    m = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    plan = _bounded_plan(capi, pat, K, val, alpha, (BOX, BOX))
    try:
        desc = plan.describe()
        assert form in desc and _single_wave(desc, K, K) and " bounds=[0,0.5]x10/[0,0.5]x10" in desc, desc
        for seed in (True, False):
            want = bstep(m, L0, R0, (BOX, BOX), seed_u=seed, seed_i=seed)
            if seed:
                free = bstep(m, L0, R0, (NO_BOX, NO_BOX))
                # the clamp shows: about half of a signed factor is negative (the 300 item rows of the 2^20-user pattern: 0.49)
                assert differs(want[0], free[0]) > 0.25 and differs(want[1], free[1]) > 0.25
            L, R = _step(plan, L0, R0, seed, seed)
            assert_same_bits(R, want[1], "%s: item sweep, seed=%s" % (name, seed))
            assert_same_bits(L, want[0], "%s: user sweep, seed=%s" % (name, seed))
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("name,K", ZERO_FORMS, ids=lambda v: str(v))
def test_unbounded_is_the_library_of_before(device, orc, switches, name, K):
    """6. A plan never told anything, and a plan told bounds and then the default again, give the oracle's bits and the same
    mf_plan_describe."""
    capi = device
    case = _pick(name, K)
    pat = pattern(case["pat"])
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    with np.errstate(all="ignore"):
        seeded = orc.tile_step(0, pat.users, 0, pat.items, K, pat.row, pat.col, val, alpha, L0, R0, True, True)
        L2, R2 = L0.copy(), R0.copy()
        orc.factorize(orc.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, val), L2, R2)
    switches(case["env"])
    descs = []
    for told in (False, True):
        plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
        try:
            assert plan.bounds("users") == NO_BOX and plan.bounds("items") == NO_BOX
            if told:
                plan.set_bounds("users", LO, HI, K - 1)
                plan.set_bounds("items", -1.0, INF)
                assert plan.bounds("users") == (LO, HI, K - 1) and plan.bounds("items") == (-1.0, INF, -1)
                assert " bounds=[0,0.5]x%d/[-1,inf]x%d" % (K - 1, K) in plan.describe(), plan.describe()
                plan.set_bounds("users")
                plan.set_bounds("items")
            descs.append(plan.describe())
            assert case["check"](descs[-1], K) and "bounds=" not in descs[-1], descs[-1]
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
    assert descs[0] == descs[1]


@gpu
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("long", 30), ("es-sw4", 10), ("coop", 10)], ids=lambda v: str(v))
def test_infinite_bounds_on_a_plan_with_everything(device, switches, name, K):
    """6. Infinite bounds over some columns on a regularised, frozen, momentum, weighted plan give that plan's bits."""
    capi = device
    case = _pick(name, K)
    base = reg_expected(case["pat"], "signed", K)
    pat = base.pat
    w = plain_weights(9100 + K, pat.nnz)
    switches(case["env"])
    got = []
    for bounds in ((NO_BOX, NO_BOX), ((-INF, INF, K - 1), (-INF, INF, 0))):
        plan = _bounded_plan(capi, pat, K, base.val, base.alpha, bounds, beta=BETA, frozen=(K - 1, 0), weight=w)
        try:
            assert "bounds=" not in plan.describe()
            plan.upload(base.L0, base.R0)
            plan.iterate(3)
            got.append(plan.download())
        finally:
            plan.close()
    m = WModel(pat.users, pat.items, pat.row, pat.col, base.val, base.alpha, w)
    want = m.wrun(base.L0, base.R0, 3, LAM, BETA, frozen=(K - 1, 0))
    for (L, R), what in zip(got, ("default", "infinite")):
        assert_same_bits(L, want[0], "%s K=%d %s bounds: L" % (name, K, what))
        assert_same_bits(R, want[1], "%s K=%d %s bounds: R" % (name, K, what))


@gpu
def test_bounds_on_a_live_plan(device, switches):
    """columns > K and every other bad value are refused on a live plan with nothing changed; bounds are legal before the
    upload and read at every launch: a change between two calls of iterate holds from the second on (graph replays too)."""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({"MF_ITER_MODE": "sweeps"})
    m = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    mid = brun(m, L0, R0, 130, (BOX, BOX))
    end = brun(m, *mid, 130, ((-0.25, 0.25, 5), NO_BOX))
    plan = capi.Plan(pat.users, pat.items, 10, alpha, pat.row, pat.col, val)
    try:
        plan.set_regularization(*LAM)
        plan.set_bounds("users", *BOX)
        plan.set_bounds("items", *BOX)
        for bad in ((0.0, 1.0, 11), (0.0, 1.0, -2), (float("nan"), 1.0, -1), (1.0, 0.0, -1)):
            with pytest.raises(capi.HipBackendError) as err:
                plan.set_bounds("users", *bad)
            assert err.value.status == capi.MF_ERR_ARGUMENT and plan.bounds("users") == BOX
        plan.upload(L0, R0)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, mid[0], "L after 130")
        assert_same_bits(R, mid[1], "R after 130")
        plan.set_bounds("users", -0.25, 0.25, 5)
        plan.set_bounds("items")
        assert " bounds=[-0.25,0.25]x5/- " in plan.describe() + " ", plan.describe()
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, end[0], "L after 260, bounds changed at 130")
        assert_same_bits(R, end[1], "R after 260, bounds changed at 130")
    finally:
        plan.close()


@gpu
def test_two_user_shards_on_one_gpu(device, switches):
    """7. Users are bounded in the sweep, items are unbounded in it: shard 0's item sweep is seeded, shard 1's is not, the host
    adds the two items_next in shard order, writes the sum into each shard's next-generation buffer and each shard calls
    mf_plan_project(items, next).  Against the numpy model of exactly that procedure."""
    import torch
    capi = device
    K, cut = 30, 333
    base = reg_expected("pair", "signed", K)
    pat = base.pat
    assert cut % 1024 and 0 < cut < pat.users
    switches({"MF_ITER_MODE": "sweeps"})
    ld = capi.row_pitch(K)
    dev = torch.device("cuda", 0)
    lo = pat.row < cut
    shards = []
    try:
        for sel, begin, count, seeded in ((lo, 0, cut, True), (~lo, cut, pat.users - cut, False)):
            row, col, val = pat.row[sel], pat.col[sel], base.val[sel]
            rb = [torch.zeros((pat.items, ld), dtype=torch.float64, device=dev) for _ in range(2)]
            plan = capi.Plan(pat.users, pat.items, K, base.alpha, row, col, val, user_begin=begin, user_count=count,
                             items_ext=[t.data_ptr() for t in rb], items_pitch=ld)
            shards.append((plan, rb, begin, count, seeded, MModel(count, pat.items, row - begin, col, val, base.alpha)))
            plan.set_regularization(*LAM)
            plan.set_bounds("users", *BOX)
            plan.upload(base.L0[begin:begin + count], base.R0)
            plan.sweep_items(seed_from_old=seeded)
            plan.sweep_users()
            plan.synchronize()
        parts, model_parts, model_L = [], [], []
        for plan, rb, begin, count, seeded, m in shards:
            nxt = next(t for t in rb if t.data_ptr() == plan.items_next_ptr())
            parts.append(nxt[:, :K].cpu().numpy().copy())
            Lm, Rm = bstep(m, base.L0[begin:begin + count], base.R0, (BOX, NO_BOX), seed_i=seeded)
            model_parts.append(Rm)
            model_L.append(Lm)
            assert_same_bits(parts[-1], Rm, "shard at %d: items_next before the sum" % begin)
        total = parts[0] + parts[1]
        assert ((total < LO) | (total > HI)).mean() > 0.5
        want_R = clip(model_parts[0] + model_parts[1], *BOX, -1, True)
        for (plan, rb, begin, count, seeded, m), Lm in zip(shards, model_L):
            nxt = next(t for t in rb if t.data_ptr() == plan.items_next_ptr())
            nxt[:, :K] = torch.from_numpy(total).to(dev)
            torch.cuda.synchronize()   # torch's stream wrote the sum; the plan's own (non-blocking) stream projects it
            plan.set_bounds("items", *BOX)
            plan.project("items", "next")
            plan.flip()
            Lb, R = plan.download()
            assert_same_bits(R, want_R, "shard at %d: the projected sum" % begin)
            assert_same_bits(Lb, Lm, "shard at %d: user block" % begin)
    finally:
        for s in shards:
            s[0].close()


@gpu
@pytest.mark.parametrize("what", ["inst30-40-10-2-10", "pair-K100"])
def test_bounds_active_equals_the_model(device, switches, what):
    """8. the three counts after iterate(5), which add up to rows x bounded columns (nothing is NaN).  The box of the bundled
    instance cuts its factors, which start inside (0, 0.1): every count of the model is above zero."""
    capi = device
    if what == "pair-K100":
        K = 100
        base = reg_expected("pair", "signed", K)
        pat, L0, R0, val, alpha = base.pat, base.L0, base.R0, base.val, base.alpha
        users, items, row, col = pat.users, pat.items, pat.row, pat.col
    else:
        inst = capi.parse_file(golden_in(what))
        K, users, items, row, col, val, alpha = inst.feats, inst.users, inst.items, inst.row, inst.col, inst.val, inst.alpha
        L0, R0 = capi.init_factors(users, items, K)
    switches({})
    lo, hi = (LO, HI) if what == "pair-K100" else (0.03, 0.07)
    bounds = ((lo, hi, K - 3), (lo, hi, -1))
    m = MModel(users, items, row, col, val, alpha)
    Lm, Rm = brun(m, L0, R0, 5, bounds, frozen=(1, -1))
    plan = capi.Plan(users, items, K, alpha, row, col, val)
    try:
        plan.set_regularization(*LAM)
        plan.set_frozen_columns(1, -1)
        plan.set_bounds("users", *bounds[0])
        plan.set_bounds("items", *bounds[1])
        plan.upload(L0, R0)
        plan.iterate(5)
        L, R = plan.download()
        assert_same_bits(L, Lm, what + " L")
        assert_same_bits(R, Rm, what + " R")
        cu, ci = plan.bounds_active("users"), plan.bounds_active("items")
        assert cu == counts(Lm, lo, hi, K - 3, 1) and ci == counts(Rm, lo, hi, -1), (cu, ci)
        assert sum(cu) == users * (K - 4) and sum(ci) == items * K and min(cu + ci) > 0, (cu, ci)
        only = C.c_int64()
        assert capi.hip().mf_plan_bounds_active(plan._h, 1, None, C.byref(only), None) == 0 and only.value == cu[1]
    finally:
        plan.close()


def _cli(capi, path, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, env=dict(clean, **env))


@gpu
def test_backend_run_bounded_equals_the_plan_path(device):
    """9. level 1 on inst1000-1000-100-2-30: the factors and the recommendations of the plan path; NULL records are
    mf_backend_run_weighted."""
    capi = device
    inst = capi.parse_file(golden_in("inst1000-1000-100-2-30") + ".gz") if not os.path.exists(golden_in("inst1000-1000-100-2-30")) else \
        capi.parse_file(golden_in("inst1000-1000-100-2-30"))
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    bu, bi = (LO, HI, inst.feats - 1), (LO, INF, -1)
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_regularization(*LAM)
        plan.set_momentum(*BETA)
        plan.set_bounds("users", *bu)
        plan.set_bounds("items", *bi)
        plan.upload(L0, R0)
        plan.iterate(inst.iters)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    assert Lp[:, :-1].min() >= LO and Lp[:, :-1].max() <= HI and Lp[:, -1].min() < LO and Rp.min() >= LO and Rp.max() > HI
    L, R = L0.copy(), R0.copy()
    best = capi.backend_run_bounded(inst, L, R, bu, bi, None, LAM_U, LAM_I, BETA[0], BETA[1])
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
    b0 = capi.backend_run_bounded(inst, La, Ra, None, None, None, LAM_U, LAM_I, BETA[0], BETA[1])
    b1 = capi.backend_run_weighted(inst, None, Lb, Rb, LAM_U, LAM_I, BETA[0], BETA[1])
    assert_same_bits(La, Lb, "no records: L of mf_backend_run_weighted")
    assert_same_bits(Ra, Rb, "no records: R of mf_backend_run_weighted")
    assert np.array_equal(b0, b1)


@gpu
def test_cli_bounds(device, orc):
    """9. MATFACT_BOUNDS=0,inf prints the .out of that plan's recommend(); with MATFACT_BIAS=1 the packed plan's, its bias
    columns free; four numbers give the items their own box; MATFACT_BOUNDS=-inf,inf prints the reference's bytes."""
    capi = device
    name = "inst30-40-10-2-10"
    path = golden_in(name)
    inst = capi.parse_file(path)
    F = inst.feats
    L0, R0 = capi.init_factors(inst.users, inst.items, F)

    def plan_out(K, val, Lx, Rx, bu, bi, frozen=NOT_FROZEN):
        plan = capi.Plan(inst.users, inst.items, K, inst.alpha, inst.row, inst.col, val)
        try:
            plan.set_frozen_columns(*frozen)
            plan.set_bounds("users", *bu)
            plan.set_bounds("items", *bi)
            plan.upload(Lx, Rx)
            plan.iterate(inst.iters)
            L, R = plan.download()
            return L, R, orc.format_out(plan.recommend()).encode()
        finally:
            plan.close()
    L, R, want = plan_out(F, inst.val, L0, R0, (0.0, INF, F), (0.0, INF, F))
    assert L.min() >= 0.0 and R.min() >= 0.0 and ((L == 0.0).sum() > 0 or (R == 0.0).sum() > 0)
    m = MModel(inst.users, inst.items, inst.row, inst.col, inst.val, inst.alpha)
    Lm, Rm = brun(m, L0, R0, inst.iters, ((0.0, INF, -1), (0.0, INF, -1)), lam=(0.0, 0.0))
    assert_same_bits(L, Lm, "NMF plan against the model, L")
    assert_same_bits(R, Rm, "NMF plan against the model, R")
    r = _cli(capi, path, MATFACT_BOUNDS="0,inf")
    assert r.returncode == 0 and r.stdout == want, (r.returncode, r.stdout[:80], r.stderr[:200])
    assert want != open(os.path.join(GOLDEN, name + ".out"), "rb").read()
    _, _, want4 = plan_out(F, inst.val, L0, R0, (0.0, 0.5, F), (-0.25, 1e300, F))
    r = _cli(capi, path, MATFACT_BOUNDS="0,0.5,-0.25,1e300")
    assert r.returncode == 0 and r.stdout == want4 and want4 != want, (r.returncode, r.stdout[:80], r.stderr[:200])
    r = _cli(capi, path, MATFACT_BOUNDS="-inf,inf")
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLDEN, name + ".out"), "rb").read(), r
    mu = seq_mean(inst.val)
    Lb, Rb, wantb = plan_out(F + 2, inst.val - mu, pack(L0, np.zeros(inst.users), 1), pack(R0, np.zeros(inst.items), 0),
                             (0.0, INF, F), (0.0, INF, F), (F + 1, F))
    assert Lb[:, :F].min() >= 0.0 and Rb[:, :F].min() >= 0.0 and (Lb[:, F].min() < 0.0 or Rb[:, F + 1].min() < 0.0)   # the biases stay free
    r = _cli(capi, path, MATFACT_BOUNDS="0,inf", MATFACT_BIAS="1")
    assert r.returncode == 0 and r.stdout == wantb, (r.returncode, r.stdout[:80], r.stderr[:200])


@gpu
def test_nmf_on_ml100k(device, switches):
    """10. instML100k, bounds [0, +inf), 50 iterations from the reference's init: every element >= 0, inside + at_lo covers
    everything, and the factors are the model's."""
    capi = device
    path = golden_in("instML100k")
    inst = capi.parse_file(path if os.path.exists(path) else path + ".gz")
    K = inst.feats
    L0, R0 = capi.init_factors(inst.users, inst.items, K)
    switches({})
    nmf = (0.0, INF, -1)
    m = MModel(inst.users, inst.items, inst.row, inst.col, inst.val, inst.alpha)
    Lm, Rm = brun(m, L0, R0, 50, (nmf, nmf), lam=(0.0, 0.0))
    plan = capi.Plan(inst.users, inst.items, K, inst.alpha, inst.row, inst.col, inst.val)
    try:
        plan.set_bounds("users", *nmf)
        plan.set_bounds("items", *nmf)
        assert " bounds=[0,inf]x%d/[0,inf]x%d" % (K, K) in plan.describe(), plan.describe()
        plan.upload(L0, R0)
        plan.iterate(50)
        L, R = plan.download()
        cu, ci = plan.bounds_active("users"), plan.bounds_active("items")
    finally:
        plan.close()
    assert (L >= 0.0).all() and (R >= 0.0).all()
    assert cu[1] == 0 and ci[1] == 0 and cu[0] + cu[2] == L.size and ci[0] + ci[2] == R.size, (cu, ci)
    assert_same_bits(L, Lm, "ML100k NMF: L")
    assert_same_bits(R, Rm, "ML100k NMF: R")
