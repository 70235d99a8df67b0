"""Every kernel at the wide K no narrow test launches: 257 to 4096, the largest K the library accepts.

The sweeps' own rows of wide K are rows of the tables they belong to (FORMS of test_sweep_edges.py, and through
test_regularised.WIDE the per-form tables of the regularised, frozen, momentum, weighted and bounded modules; KS of test_loss.py
and of test_certification_boundary.py; the exact-K lists of the top-N, rank and similar-items modules).  Here is what has no
table to go into:

A  a guard on the tables themselves (CPU): the kernel tables of mf_plan.hip.h are read as text, choose_sweep's K-to-instance
   rule is restated in a dozen lines, and every instance of every table must be launched by a row of FORMS under the
   switches that row sets -- the run-time-K instances at both ends of their range of K.  An instance added to a table
   without a row fails here, without a GPU;
B  the limits: K = 4096 runs, 4097 and 4098 are refused with MF_ERR_UNSUPPORTED by mf_plan_create and by mf_backend_run,
   nothing is written for a refused K and the next plan works;
C  what composes the extensions at wide K: one plan per form with weights, both lambdas, both betas and an uploaded
   history, a frozen column and a box on each side; the box cut one column either side of a register boundary;
   mf_backend_run_biased at F = 4094, the largest it accepts; mf_plan_penalty, mf_plan_project and mf_plan_bounds_active;
D  mf_plan_predict above K = 256.

Every comparison is bit for bit (assert_same_bits) against the CPU oracle or the numpy models of the modules named."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_bounded import BOX, HI, LO, _bounded_plan, bstep, clip, counts, hand_made, run_form
from test_bounded import bits as u64
from test_bounded import expected as bounded_expected
from test_frozen import BiasModel, fstep, pack, seq_mean
from test_loss import model_total
from test_momentum import BETA, random_prev
from test_regularised import LAM_I, LAM_U, WIDE, Model, _pick, differs, row_squares
from test_regularised import expected as reg_expected
from test_sweep_edges import CASES, SWITCHES, assert_same_bits, cls_signed, pattern, wide_nch
from test_weighted import WModel, planted_weights

gpu = pytest.mark.gpu

LAM = (LAM_U, LAM_I)
LARGEST_K = 4096


# ------------------------------------------------------------------------------------------------ A: the table guard
HEADER = os.path.join(ROOT, "recommender-system_amd", "csrc", "mf_plan.hip.h")


def sweep_tables(text):
    """{table: [(KT, KPMAX or NPASS)]} of the four kernel tables, in table order.  An LDS-DMA instance of a compile-time K
    has its passes from K (128 columns a pass)."""
    def body(name):
        found = re.findall(r"const SweepVariant %s\[\] = \{(.*?)\};" % name, text, re.S)
        assert len(found) == 1, name
        return found[0]
    two = r"\bvariant<(\d+), (\d+)>\(\)"
    return {"kSpecialised": [(int(kt), int(kp)) for kt, kp in re.findall(two, body("kSpecialised"))],
            "kDma": [(int(kt), -(-int(kt) // 128)) for kt in re.findall(r"\bdma_variant<(\d+)>\(\)", body("kDma"))],
            "kDmaGeneric": [(0, int(n)) for n in re.findall(r"\bdma_generic_variant<(\d+)>\(\)", body("kDmaGeneric"))],
            "kGeneric": [(int(kt), int(kp)) for kt, kp in re.findall(two, body("kGeneric"))]}


def dispatch(tables, K, reg):
    """choose_sweep's rule: (table, KT, KPMAX or NPASS) of K, None for a K it refuses.  `reg`: MF_SWEEP_IMPL=reg."""
    if not reg:
        for kt, np_ in tables["kDma"]:
            if kt == K:
                return ("kDma", kt, np_)
        if K % 2 == 0:
            for _, np_ in tables["kDmaGeneric"]:
                if K <= 128 * np_:
                    return ("kDmaGeneric", 0, np_)
    for kt, kp in tables["kSpecialised"]:
        if kt == K:
            return ("kSpecialised", kt, kp)
    for _, kp in tables["kGeneric"]:
        if K <= 64 * kp:
            return ("kGeneric", 0, kp)
    return None


def unreached(tables, cases):
    """What the rows of `cases` leave out: instances no row is dispatched to, and ends of a run-time-K instance's range of K
    (over both settings of MF_SWEEP_IMPL) that no row runs."""
    reached = {}
    for c in cases:
        if c["env"].get("MF_ITER_MODE") != "sweeps":       # the errors + streams iteration launches other kernels
            continue
        inst = dispatch(tables, c["K"], c["env"].get("MF_SWEEP_IMPL") == "reg")
        reached.setdefault(inst, set()).add(c["K"])
    largest = 64 * max(kp for _, kp in tables["kGeneric"])
    span = {}
    for K in range(1, largest + 1):
        for reg in (False, True):
            span.setdefault(dispatch(tables, K, reg), set()).add(K)
    missing = []
    for name, rows in tables.items():
        for kt, width in rows:
            inst = (name, kt, width)
            if not reached.get(inst):
                missing.append((inst, "no row"))
            elif kt == 0:
                missing += [(inst, "K=%d" % k) for k in (min(span[inst]), max(span[inst])) if k not in reached[inst]]
    return missing


def test_every_instance_of_the_sweep_tables_is_launched_by_a_row_of_the_table():
    text = open(HEADER).read()
    tables = sweep_tables(text)
    assert all(tables.values()) and all(kt == 0 for kt, _ in tables["kGeneric"]) and all(kt > 0 for kt, _ in tables["kSpecialised"])
    widest = re.findall(r"constexpr int kLargestK = (\d+) \* mf::kWave;", text)
    assert widest == [str(max(kp for _, kp in tables["kGeneric"]))] and 64 * int(widest[0]) == LARGEST_K
    for reg in (False, True):
        assert dispatch(tables, LARGEST_K, reg) == ("kGeneric", 0, 64)
        assert dispatch(tables, LARGEST_K + 1, reg) is None and dispatch(tables, LARGEST_K + 2, reg) is None
    # the rule on the K the tables' own comments name
    assert dispatch(tables, 100, False) == ("kDma", 100, 1) and dispatch(tables, 256, False) == ("kDma", 256, 2)
    assert dispatch(tables, 100, True) == ("kSpecialised", 100, 2) and dispatch(tables, 300, False) == ("kDmaGeneric", 0, 4)
    assert dispatch(tables, 257, False) == ("kGeneric", 0, 8) and dispatch(tables, 1026, False) == ("kGeneric", 0, 32)
    assert unreached(tables, CASES) == []
    # ... and an instance added to a table without a row is reported, as is a range whose end moved
    grown = dict(tables, kDmaGeneric=tables["kDmaGeneric"] + [(0, 16)])
    assert unreached(grown, CASES) == [(("kDmaGeneric", 0, 16), "K=2048")]          # 1026 falls to it; its last K has no row
    grown = dict(tables, kGeneric=tables["kGeneric"] + [(0, 128)])
    assert (("kGeneric", 0, 128), "no row") in unreached(grown, CASES)
    grown = dict(tables, kDma=tables["kDma"] + [(40, 1)])
    assert (("kDma", 40, 1), "no row") in unreached(grown, CASES)
    fewer = [c for c in CASES if c["K"] != 4096]
    assert unreached(tables, fewer) == [(("kGeneric", 0, 64), "K=4096")]


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


# ------------------------------------------------------------------------------------------------ B: the limits
@gpu
def test_the_largest_k_runs_and_a_larger_one_is_refused(device, orc, switches):
    """K = 4096 is created and iterates (the oracle's bits); 4097 and 4098 -- an odd and an even K past the last table row --
    are MF_ERR_UNSUPPORTED from mf_plan_create and from mf_backend_run, whose factors keep every bit; a plan created after
    the refusals works."""
    capi = device
    switches({})
    pat = pattern("wide")
    for K in (LARGEST_K + 1, LARGEST_K + 2):
        L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
        with pytest.raises(capi.HipBackendError) as err:
            capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED, K
        L, R = L0.copy(), R0.copy()
        with pytest.raises(capi.HipBackendError) as err:
            capi.backend_run(capi.Instance(1, alpha, K, pat.users, pat.items, pat.row, pat.col, val), L, R)
        assert err.value.status == capi.MF_ERR_UNSUPPORTED, K
        assert_same_bits(L, L0, "K=%d: L after the refused run" % K)
        assert_same_bits(R, R0, "K=%d: R after the refused run" % K)
    for K in (LARGEST_K, 10):
        L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
        Lo, Ro = L0.copy(), R0.copy()
        orc.factorize(orc.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, val), Lo, Ro)
        plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
        try:
            desc = plan.describe()
            assert desc.startswith("sweep_kernel<KT=0,KPMAX=64> K=4096 nch=4 " if K == LARGEST_K else "sweep_dma_kernel<KT=10,"), desc
            plan.upload(L0, R0)
            plan.iterate(2)
            L, R = plan.download()
        finally:
            plan.close()
        assert_same_bits(L, Lo, "K=%d: L after two iterations" % K)
        assert_same_bits(R, Ro, "K=%d: R after two iterations" % K)
        best = capi.backend_run(capi.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, val), L0, R0)
        assert_same_bits(L0, Lo, "K=%d: mf_backend_run, L" % K)
        assert np.array_equal(best, orc.recommend(orc.Instance(2, alpha, K, pat.users, pat.items, pat.row, pat.col, val), Lo, Ro))


# ------------------------------------------------------------------------------------------------ C: the extensions, composed
# per form: the frozen columns (users, items) and the boxes (users, items).  reg-wide 4095: lane 62 and lane 0 of register 63,
# the users' box ends one lane into that register; 513: the lone lane of the ninth register frozen, the box ends in front of
# it; dma-rt 1024: the .y of the last piece and the first piece of the fifth pass, a box that ends inside that piece.
COMPOSED = {("reg-wide", 513): ((512, 0), ((LO, HI, 512), BOX)),
            ("reg-wide", 4095): ((4094, 4032), ((LO, HI, 4033), BOX)),
            ("dma-rt", 1024): ((1023, 512), ((LO, HI, 1022), (0.25, HI, 513)))}


def test_the_composed_cases_are_the_wide_forms():
    assert sorted(COMPOSED) == sorted(WIDE) and sorted(CUTS) == sorted(WIDE[1:])


@gpu
@pytest.mark.parametrize("name,K", WIDE, ids=lambda v: str(v))
def test_everything_in_one_plan(device, switches, name, K):
    """Weights, both lambdas, both betas with an uploaded history, a frozen column and a box on each side, two iterations:
    bstep over WModel."""
    capi = device
    case = _pick(name, K)
    frozen, bounds = COMPOSED[name, K]
    base = reg_expected(case["pat"], "signed", K)
    pat = base.pat
    w = planted_weights(9000 + K, pat)
    Lp, Rp = random_prev(5000 + K, base.L0), random_prev(6000 + K, base.R0)
    m = WModel(pat.users, pat.items, pat.row, pat.col, base.val, base.alpha, w)
    one = bstep(m, base.L0, base.R0, bounds, Lp, Rp, LAM, BETA, frozen)
    two = bstep(m, *one, bounds, base.L0, base.R0, LAM, BETA, frozen)
    # the guards, on the model: every ingredient shows in the first step
    for without in (dict(bounds=((-np.inf, np.inf, -1),) * 2), dict(lam=(0.0, 0.0)), dict(beta=(0.0, 0.0)), dict(frozen=(-1, -1))):
        kw = dict(dict(bounds=bounds, lam=LAM, beta=BETA, frozen=frozen), **without)
        other = bstep(m, base.L0, base.R0, kw["bounds"], Lp, Rp, kw["lam"], kw["beta"], kw["frozen"])
        assert differs(other[0], one[0]) > 0.0 and differs(other[1], one[1]) > 0.0, (name, K, list(without))
    ones = WModel(pat.users, pat.items, pat.row, pat.col, base.val, base.alpha, np.ones(pat.nnz))
    assert differs(bstep(ones, base.L0, base.R0, bounds, Lp, Rp, LAM, BETA, frozen)[0], one[0]) > 0.1
    switches(case["env"])
    plan = _bounded_plan(capi, pat, K, base.val, base.alpha, bounds, LAM, BETA, frozen, weight=w)
    try:
        desc = plan.describe()
        assert case["check"](desc, K) and wide_nch(desc, dict(case, nch=None)), desc
        assert " lambda=" in desc and " momentum=" in desc and " frozen=%d/%d" % frozen in desc and " bounds=" in desc and " weighted=1" in desc, desc
        where = "%s K=%d [%s]" % (name, K, desc.split(" loss=")[0])
        plan.upload(base.L0, base.R0)
        plan.upload_previous(Lp, Rp)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, one[0], where + ": L after one iteration")
        assert_same_bits(R, one[1], where + ": R after one iteration")
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, two[0], where + ": L after two iterations")
        assert_same_bits(R, two[1], where + ": R after two iterations")
    finally:
        plan.close()


# the box cut one column either side of a boundary (users, items), twice per form: 4032 is lane 0 of register 63; 512 the
# first piece of the fifth pass, 2 the first piece alone, 1022 = K - 2 the bias layout's
CUTS = {("reg-wide", 4095): ((4031, 4033), (4032, 4032)), ("dma-rt", 1024): ((2, 512), (1022, 511))}


@gpu
@pytest.mark.parametrize("name,K,cut", [(n, K, c) for (n, K), cs in CUTS.items() for c in cs], ids=lambda v: str(v))
def test_box_columns_either_side_of_a_boundary(device, switches, name, K, cut):
    """`columns` of the two sides at `cut`, no frozen column: the columns from the cut on keep the free model's bits -- more
    than half of them lie outside the box --, the ones in front are projected."""
    case = _pick(name, K)
    bu, bi = (LO, HI, cut[0]), (LO, HI, cut[1])
    x = bounded_expected(case["pat"], "signed", K, bu, bi)
    for new, free, n in ((x.seeded[0], x.free[0], cut[0]), (x.seeded[1], x.free[1], cut[1])):
        assert new[:, :n].min() >= LO and new[:, :n].max() <= HI
        assert_same_bits(new[:, n:], free[:, n:], "the model leaves the unbounded columns alone")
        assert ((free[:, n] < LO) | (free[:, n] > HI)).mean() > 0.5 and ((free[:, n - 1] < LO) | (free[:, n - 1] > HI)).mean() > 0.5
    run_form(device, switches, case, x, (bu, bi))


@gpu
def test_backend_run_biased_at_the_largest_f(device, switches):
    """F = 4094, the largest mf_backend_run_biased accepts: the packed plan has K = 4096, the frozen columns 4095 and 4094 sit
    in lanes 63 and 62 of register 63.  One iteration on "wide" from random biases: the explicit-bias model, and the packed
    frozen-column model through pack."""
    capi = device
    switches({})
    F = LARGEST_K - 2
    pat = pattern("wide")
    L0, R0, val, alpha = cls_signed(6000 + F, pat, F)
    rng = np.random.default_rng(F)
    bu0, bi0 = rng.uniform(-1, 1, pat.users), rng.uniform(-1, 1, pat.items)
    mu = seq_mean(val)
    Lm, Rm, bum, bim = BiasModel(pat.users, pat.items, pat.row, pat.col, val - mu, alpha).step(L0, R0, bu0, bi0, LAM_U, LAM_I)
    packed = fstep(Model(pat.users, pat.items, pat.row, pat.col, val - mu, alpha), pack(L0, bu0, 1), pack(R0, bi0, 0), LAM_U, LAM_I, F + 1, F)
    assert_same_bits(packed[0], pack(Lm, bum, 1), "the packed model, users")
    assert_same_bits(packed[1], pack(Rm, bim, 0), "the packed model, items")
    assert differs(bum, bu0) > 0.5 and differs(bim, bi0) > 0.5 and differs(Lm, L0) > 0.5
    L, R, bu, bi = L0.copy(), R0.copy(), bu0.copy(), bi0.copy()
    got_mu, best = capi.backend_run_biased(capi.Instance(1, alpha, F, pat.users, pat.items, pat.row, pat.col, val), L, R, bu, bi,
                                           LAM_U, LAM_I, iters=1, recommend=False)
    assert best is None
    assert_same_bits(np.array([got_mu]), np.array([mu]), "mu")
    assert_same_bits(L, Lm, "L")
    assert_same_bits(R, Rm, "R")
    assert_same_bits(bu, bum, "user biases")
    assert_same_bits(bi, bim, "item biases")


PEN_KC = 32       # kPenKC: columns mf_plan_penalty stages per step


@gpu
@pytest.mark.parametrize("K", [257, 1024, 4095])
def test_penalty_project_and_bounds_active(device, switches, K):
    """70 users (five 16-row workgroups of the penalty, the last of 6; two 64-row steps of the box kernels) x 40 items.
    K = 257 is the first K above a multiple of the penalty's 32-column step that exceeds 256: eight full steps and one
    column.  mf_plan_penalty against row_squares and the blocked total; mf_plan_project on the hand-made matrix of
    test_bounded (every special value in every column) against clip, and mf_plan_bounds_active against counts -- columns
    K - 2 with the frozen column inside the range on the users' side, all K on the items'."""
    capi = device
    switches({})
    assert K != 257 or ((K - 1) % PEN_KC == 0 and K - 1 == 256)
    users, items = 70, 40
    rng = np.random.default_rng(K)
    cells = np.sort(rng.choice(users * items, 300, replace=False))
    row, col = (cells // items).astype(np.int32), (cells % items).astype(np.int32)
    val = rng.integers(-10, 11, len(row)) / 2.0
    L = rng.uniform(-1, 1, (users, K)) * 10.0 ** rng.integers(-4, 5, (users, 1))
    R = rng.uniform(-1, 1, (items, K)) * 10.0 ** rng.integers(-4, 5, (items, 1))
    plan = capi.Plan(users, items, K, 1e-3, row, col, val)
    try:
        plan.upload(L, R)
        usq, isq, ur, ir = plan.penalty(rows=True)
        assert_same_bits(ur, row_squares(L), "K=%d: user rows" % K)
        assert_same_bits(ir, row_squares(R), "K=%d: item rows" % K)
        assert_same_bits(np.array([usq, isq]), np.array([model_total(ur), model_total(ir)]), "K=%d: totals" % K)
        # a row whose squares are summed in another order, or whose last column is dropped, has other bits
        assert differs(ur, row_squares(L[:, ::-1])) > 0.5 and differs(ur, row_squares(L[:, :K - 1])) > 0.5
        Lh, Rh = hand_made(users, K), hand_made(items, K, 5)
        frozen, cols = K // 2, K - 2
        plan.upload(Lh, Rh)
        plan.set_frozen_columns(frozen, -1)
        plan.set_bounds("users", LO, HI, cols)
        plan.set_bounds("items", 0.25, HI, -1)
        plan.project("users")
        plan.project("items")
        plan.synchronize()
        Lg, Rg = plan.download()
        want_l, want_r = clip(Lh, LO, HI, cols, frozen, True), clip(Rh, 0.25, HI, -1, -1, True)
        assert np.array_equal(u64(Lg), u64(want_l)), "K=%d: projected users (NaN payloads included)" % K
        assert np.array_equal(u64(Rg), u64(want_r)), "K=%d: projected items" % K
        assert differs(want_l, Lh) > 0.1 and np.array_equal(u64(want_l[:, cols:]), u64(Lh[:, cols:])) and np.array_equal(u64(want_l[:, frozen]), u64(Lh[:, frozen]))
        cu, ci = plan.bounds_active("users"), plan.bounds_active("items")
        assert cu == counts(want_l, LO, HI, cols, frozen) and ci == counts(want_r, 0.25, HI, -1), (K, cu, ci)
        assert min(cu + ci) > 0 and sum(cu) < users * (cols - 1) and sum(ci) < items * K       # the NaNs are in no count
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ D: predict
@gpu
@pytest.mark.parametrize("K", [301, 1024, LARGEST_K])
def test_predict_above_256(device, orc, switches, K):
    """mf_plan_predict on 64 x 200: every element of B against oracle.predict_row (k ascending from 0.0, unfused)"""
    capi = device
    switches({})
    users, items = 64, 200
    rng = np.random.default_rng(300 + K)
    L = rng.uniform(-1, 1, (users, K)) * 10.0 ** rng.integers(-3, 4, (users, 1))
    R = rng.uniform(-1, 1, (items, K))
    L[7, K - 1], R[11, 0] = -0.0, 5e-324
    cells = np.sort(rng.choice(users * items, 500, replace=False))
    row, col = (cells // items).astype(np.int32), (cells % items).astype(np.int32)
    plan = capi.Plan(users, items, K, 0.01, row, col, np.ones(len(row)))
    try:
        plan.upload(L, R)
        B = plan.predict()
    finally:
        plan.close()
    want = np.stack([orc.predict_row(np.ascontiguousarray(L[u]), R) for u in range(users)])
    assert_same_bits(B, want, "K=%d: B" % K)
    assert differs(want, L @ R.T) > 0.5                     # another summation order has other bits: the test can tell
