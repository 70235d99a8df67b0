"""The three ALS solves (als_kernel, gram_block_kernel, als_cg_kernel) at the edges the modules of their features do not launch.

tests/test_als.py, tests/test_implicit.py and tests/test_als_cg.py define the models and compare every form with them bit for
bit; here is what reading the launch code against those modules shows they leave out:

A  a guard on the instance tables (CPU): kAlsForm, als_cg_fn and kGramFn of mf_plan.hip.h are read as text, the rule that takes a
   (form, K) to an instance is restated in a few lines -- the blocks per thread NB from als_blocks and the thread count --, and
   the K lists the GPU tests iterate over must reach every instance, both ends of the range of K of every run-time-K instance
   and every compile-time K of the conjugate-gradient table, in its explicit and in its implicit instantiation (the instances
   of one pass, K <= 128; tests/test_implicit_cg.py launches them).  The ends of the NB ranges then run here, on the `pair` pattern
   with random factors (the planted instances of the other modules have R = 2 I or a triangular Y: zero products off the
   diagonal cannot see a wrong block-to-thread mapping);
B  the split side: MF_SWEEP_LONG=128 on `skewed` gives both sides extreme rows, so launch_als launches every solve twice
   into the same three counters; on `long-items` only the items split.  Dispatch order is no part of the definition: the
   expected bits are those of the models, which know no split;
C  value classes: range, zeros and nonfinite of tests/test_sweep_edges.py, and scale classes built here -- the signed class
   with Y and the ratings times 2^e -- that hand sqrt and `/` subnormal pivots and divisors, pivots near 2^1000 and Gram
   elements that overflow.  The condition each scale class is there for is asserted on the model alone, on the CPU;
D  conjugate gradient at the gather chunks 15, 14, 13 and 12 of K = 189 .. 256 on rows of chunk - 1, chunk, chunk + 1, 2 chunk
   and 2 chunk + 1 entries, and at 64, 255 and 256 steps: the loop's exit at the limit of 256.

Every GPU comparison is assert_same_bits on both factor matrices and equality of the three counters of both sides."""
import functools
import os
import re

import numpy as np
import pytest

import test_als as direct_mod
import test_als_cg as cg_mod
import test_implicit as implicit_mod
import test_implicit_cg as icg_mod
from conftest import ROOT
from test_als import KINDS, LAM, AlsModel, als_plan, hand_iteration
from test_als import check_form as direct_check_form
from test_als import expected as direct_expected
from test_als import forms_of as direct_forms
from test_als_cg import CgModel, cg_plan, chunk_of
from test_als_cg import check_form as cg_check_form
from test_als_cg import expected as cg_expected
from test_als_cg import forms_of as cg_forms
from test_implicit import ImplicitModel, _variant, four_grams, gram, implicit_plan, sparse_entries
from test_implicit import check_form as implicit_check_form
from test_implicit import expected as implicit_expected
from test_regularised import LAM_I, LAM_U, differs
from test_stream_order import long_rows
from test_sweep_edges import CLASSES, SWITCHES, WIDE_LENS, assert_same_bits, cls_signed, is_subnormal, pattern

gpu = pytest.mark.gpu

CSRC = os.path.join(ROOT, "recommender-system_amd", "csrc")
LAM0 = (0.0, 0.0)
CONF = 40.0

# the ends of the NB ranges that ALL_K of test_als.py / test_implicit.py and GRAM_K leave out; they run here on `pair` only
# (the whole parametrisation of those modules at K = 124 / 125 would put model solves of 2600 rows into every later run)
WAVE_EDGE_K = (20, 21, 31, 32)
WG_EDGE_K = (88, 89, 124, 125)
NB_EDGE_K = WAVE_EDGE_K + WG_EDGE_K


# ------------------------------------------------------------------------------------------------ A: the table guard
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    found = re.findall(r"constexpr int %s = (\d+);" % name, text)
    assert len(found) == 1, name
    return int(found[0])


def als_tables():
    """The instance tables as the launch code indexes them: {"explicit" / "implicit": {form: threads, bs, max_k, nbs},
    "gram": threads, bs, max_k, nbs, "cg" / "icg": fixed [(KT, NP)], dma [NP], general [NP]}"""
    plan, als, grm = _source("mf_plan.hip.h"), _source("mf_als.hip.h"), _source("mf_gram.hip.h")
    names = {"mf::kAlsThreads": _const(als, "kAlsThreads"), "mf::kWave": _const(_source("mf_common.hip.h"), "kWave"),
             "mf::kAlsMaxK": _const(als, "kAlsMaxK"), "mf::kAlsWaveMaxK": _const(als, "kAlsWaveMaxK")}
    body = re.findall(r"const AlsForm kAlsForm\[kAlsForms\] = \{(.*?)\n\};", plan, re.S)
    assert len(body) == 1
    tables = {"explicit": {}, "implicit": {}}
    for chunk in body[0].split('{"')[1:]:
        name, threads, bs, max_k = re.match(r'(\w+)", ([\w:]+), (\d+), [\w:]+, ([\w:]+),', chunk).groups()
        for kind, tail in (("explicit", ">"), ("implicit", ", mf::AlsImplicit>")):
            inst = re.findall(r"mf::als_kernel<([\w:]+), (\d+), (\d+)%s" % re.escape(tail), chunk)
            assert inst and all(t == threads and b == bs for t, b, _ in inst), (name, kind, inst)
            tables[kind][name] = dict(threads=names[threads], bs=int(bs), max_k=names[max_k], nbs=[int(nb) for _, _, nb in inst])
    nbs = [int(nb) for nb in re.findall(r"mf::gram_block_kernel<(\d+)>", re.findall(r"const GramFn kGramFn\[\d+\] = \{(.*?)\};", plan)[0])]
    tables["gram"] = dict(threads=_const(grm, "kGramThreads"), bs=_const(grm, "kGramBS"), max_k=names["mf::kAlsMaxK"], nbs=nbs)
    fn = re.findall(r"inline const void \*als_cg_fn\(int form, int K\)\n\{(.*?)\n\}", plan, re.S)
    assert len(fn) == 1
    fixed = [(int(k), int(kt), int(np_)) for k, kt, np_ in re.findall(r"case (\d+): return als_cg_instance<(\d+), (\d+), true, IM\.\.\.>\(\);", fn[0])]
    assert fixed and all(k == kt for k, kt, _ in fixed)
    run_time = re.findall(r"als_cg_instance<0, (\d+), (true|false), IM\.\.\.>\(\)", fn[0])
    tables["cg"] = dict(fixed=[(kt, np_) for _, kt, np_ in fixed], dma=sorted(int(n) for n, d in run_time if d == "true"),
                        general=sorted(int(n) for n, d in run_time if d == "false"))
    # the implicit instantiation of the same table: als_cg_instance leaves out what is not of one pass, als_cg_fn every K above
    # kAlsMaxK
    inst = re.findall(r"inline const void \*als_cg_instance\(\)\n\{(.*?)\n\}", plan, re.S)
    assert len(inst) == 1 and re.match(r"\s*if constexpr \(sizeof\.\.\.\(IM\) == 0\)\s*return \(const void \*\) mf::als_cg_kernel<KT, NP, DMA>;"
                                       r"\s*else if constexpr \(NP == 1\)\s*return \(const void \*\) mf::als_icg_kernel<KT, NP, DMA>;"
                                       r"\s*else\s*return nullptr;$", inst[0]), inst
    assert "(sizeof...(IM) == 1 && K > mf::kAlsMaxK)) return nullptr;" in fn[0]
    tables["icg"] = dict(fixed=[(kt, np_) for kt, np_ in tables["cg"]["fixed"] if np_ == 1], dma=[n for n in tables["cg"]["dma"] if n == 1],
                         general=[n for n in tables["cg"]["general"] if n == 1], max_k=names["mf::kAlsMaxK"])
    return tables


def als_blocks(K, bs):
    kb = -(-K // bs)
    return kb * (kb + 1) // 2


def nb_of(rec, K):
    """launch_als / launch_gram: blocks of the triangle per thread, the index (plus one) into the form's instances"""
    return -(-als_blocks(K, rec["bs"]) // rec["threads"])


def cg_passes(K):
    return -(-((K + 1) // 2) // 64)


def direct_name(rec, nb, implicit):
    return "als_kernel<%d, %d, %d%s>" % (rec["threads"], rec["bs"], nb, ", AlsImplicit" if implicit else "")


def cg_name(kt, np_, dma, implicit=False):
    return "%s<%d, %d, %s>" % ("als_icg_kernel" if implicit else "als_cg_kernel", kt, np_, "true" if dma else "false")


def instance_of(tables, table, form, K):
    """the instance a (form, K) reaches, by name; None where the form does not take the K"""
    if table in ("explicit", "implicit"):
        rec = tables[table][form]
        return direct_name(rec, nb_of(rec, K), table == "implicit") if 1 <= K <= rec["max_k"] else None
    if table == "gram":
        rec = tables["gram"]
        return "gram_block_kernel<%d>" % nb_of(rec, K) if 1 <= K <= rec["max_k"] else None
    implicit = table == "icg"
    if not 1 <= K <= (tables["icg"]["max_k"] if implicit else cg_mod.MAX_K):
        return None
    if form == "fixed":
        return next((cg_name(kt, np_, True, implicit) for kt, np_ in tables[table]["fixed"] if kt == K), None)
    if form == "dma":
        return cg_name(0, cg_passes(K), True, implicit) if K % 2 == 0 else None
    return cg_name(0, cg_passes(K), False, implicit)


def all_instances(tables, table):
    if table in ("explicit", "implicit"):
        return [(f, direct_name(rec, nb, table == "implicit")) for f, rec in tables[table].items() for nb in rec["nbs"]]
    if table == "gram":
        return [(None, "gram_block_kernel<%d>" % nb) for nb in tables["gram"]["nbs"]]
    cg, im = tables[table], table == "icg"
    return ([("fixed", cg_name(kt, np_, True, im)) for kt, np_ in cg["fixed"]] + [("dma", cg_name(0, n, True, im)) for n in cg["dma"]]
            + [("general", cg_name(0, n, False, im)) for n in cg["general"]])


def unreached(tables, table, cases):
    """What the (form, K) of `cases` leave out of one table: instances nothing reaches ("no K"), and ends of a run-time-K
    instance's range of K that nothing runs; a K whose instance is not in the table at all is reported too"""
    reached, span = {}, {}
    for form, K in cases:
        reached.setdefault((form, instance_of(tables, table, form, K)), set()).add(K)
    forms = sorted({f for f, _ in all_instances(tables, table)}, key=str)
    for form in forms:
        for K in range(1, cg_mod.MAX_K + 1):
            span.setdefault((form, instance_of(tables, table, form, K)), set()).add(K)
    listed = all_instances(tables, table)
    missing = [(name, "K=%d has no instance" % min(ks)) for (form, name), ks in sorted(span.items(), key=str) if name and (form, name) not in listed]
    for form, name in listed:
        got = reached.get((form, name), set())
        if not got:
            missing.append((name, "no K"))
        elif "<0," in name or table not in ("cg", "icg"):   # a run-time K: both ends of its range
            ends = (min(span[(form, name)]), max(span[(form, name)]))
            missing += [(name, "K=%d" % k) for k in ends if k not in got]
    return missing


def k_lists(edges=True):
    """the (form, K) every table is launched with by the GPU tests of the three modules and, `edges`, of this one"""
    extra = NB_EDGE_K if edges else ()
    new_cg = () if edges else (20, 50, 130)
    cases = next(m for m in implicit_mod.test_both_sides_in_every_form.pytestmark if m.name == "parametrize").args[1]
    implicit_k = tuple(sorted({K for _, K in cases}))
    return {"explicit": [(f, K) for K in direct_mod.ALL_K + extra for f in direct_forms(K)],
            "implicit": [(f, K) for K in implicit_k + extra for f in direct_forms(K)],
            "gram": [(None, K) for K in implicit_mod.GRAM_K + (WG_EDGE_K if edges else ())],
            "cg": [(f, K) for K in cg_mod.ALL_K if K not in new_cg for f in cg_forms(K)],
            "icg": [(f, K) for K in icg_mod.ALL_K for f in cg_forms(K)]}


def gaps(tables, lists):
    return {t: unreached(tables, t, lists[t]) for t in ("explicit", "implicit", "gram", "cg", "icg")}


def test_every_instance_of_the_als_tables_is_launched_at_both_ends_of_its_range():
    tables = als_tables()
    # the tables as they stand, and the ranges of NB recomputed from als_blocks and the thread counts
    for t in ("explicit", "implicit"):
        assert {f: (r["threads"], r["bs"], r["max_k"], r["nbs"]) for f, r in tables[t].items()} == {"wg": (256, 4, 128, [1, 2, 3]), "wave": (64, 2, 32, [1, 2, 3])}
        assert set(tables[t]) == set(direct_mod.FORMS) and all(tables[t][f]["max_k"] == direct_mod.FORMS[f]["max_k"] for f in tables[t])
    assert tables["gram"] == dict(threads=256, bs=4, max_k=128, nbs=[1, 2, 3])
    assert [kt for kt, _ in tables["cg"]["fixed"]] == list(cg_mod.FIXED_K) and all(np_ == cg_passes(kt) for kt, np_ in tables["cg"]["fixed"])
    assert tables["cg"]["dma"] == [1, 2] and tables["cg"]["general"] == [1, 2]
    assert [kt for kt, _ in tables["icg"]["fixed"]] == list(icg_mod.FIXED_K) and tables["icg"]["dma"] == tables["icg"]["general"] == [1]
    wg, wave = tables["explicit"]["wg"], tables["explicit"]["wave"]
    assert [nb_of(wg, K) for K in (1, 88, 89, 124, 125, 128)] == [1, 1, 2, 2, 3, 3]
    assert [nb_of(wave, K) for K in (1, 20, 21, 30, 31, 32)] == [1, 1, 2, 2, 3, 3]
    assert [cg_passes(K) for K in (1, 128, 129, 130, 256)] == [1, 1, 2, 2, 2]
    # every K a form takes has an instance, and the lists reach every instance at both ends
    lists = k_lists()
    found = gaps(tables, lists)
    for t, missing in found.items():
        print(t, missing)
    assert found == {"explicit": [], "implicit": [], "gram": [], "cg": [], "icg": []}
    # ... which they did not before this module and the three K added to ALL_K of test_als_cg.py
    before = gaps(tables, k_lists(edges=False))
    for t, missing in before.items():
        print("before:", t, missing)
    ends = lambda name, ks: [(name, "K=%d" % k) for k in ks]   # noqa: E731
    assert before["explicit"] == (ends("als_kernel<256, 4, 1>", [88]) + ends("als_kernel<256, 4, 2>", [89, 124]) + ends("als_kernel<256, 4, 3>", [125])
                                  + ends("als_kernel<64, 2, 1>", [20]) + ends("als_kernel<64, 2, 2>", [21]) + [("als_kernel<64, 2, 3>", "no K")])   # K = 31, 32
    assert before["implicit"] == [(n.replace(">", ", AlsImplicit>"), k) for n, k in before["explicit"]]
    assert before["gram"] == ends("gram_block_kernel<1>", [88]) + ends("gram_block_kernel<2>", [89, 124]) + ends("gram_block_kernel<3>", [125])
    assert before["cg"] == [("als_cg_kernel<20, 1, true>", "no K"), ("als_cg_kernel<50, 1, true>", "no K"), ("als_cg_kernel<0, 2, true>", "K=130")]
    assert before["icg"] == []   # tests/test_implicit_cg.py came with its list whole
    # a grown table is reported: a ninth fixed K, a fourth NB, a third number of passes
    grown = dict(tables, cg=dict(tables["cg"], fixed=tables["cg"]["fixed"] + [(40, 1)]))
    assert unreached(grown, "cg", lists["cg"]) == [("als_cg_kernel<40, 1, true>", "no K")]
    grown = dict(tables, cg=dict(tables["cg"], general=[1, 2, 3]))
    assert unreached(grown, "cg", lists["cg"]) == [("als_cg_kernel<0, 3, false>", "no K")]
    grown = dict(tables, icg=dict(tables["icg"], fixed=tables["icg"]["fixed"] + [(40, 1)]))
    assert unreached(grown, "icg", lists["icg"]) == [("als_icg_kernel<40, 1, true>", "no K")]
    for t in ("explicit", "implicit"):
        grown = dict(tables, **{t: dict(tables[t], wg=dict(tables[t]["wg"], nbs=[1, 2, 3, 4]))})
        assert unreached(grown, t, lists[t]) == [(direct_name(tables[t]["wg"], 4, t == "implicit"), "no K")]
    grown = dict(tables, gram=dict(tables["gram"], nbs=[1, 2, 3, 4]))
    assert unreached(grown, "gram", lists["gram"]) == [("gram_block_kernel<4>", "no K")]
    # a table that lost an instance some K needs, and a range whose end moved, are reported as well
    fewer = dict(tables, gram=dict(tables["gram"], nbs=[1, 2]))
    assert ("gram_block_kernel<3>", "K=125 has no instance") in unreached(fewer, "gram", lists["gram"])
    moved = dict(tables, explicit=dict(tables["explicit"], wave=dict(tables["explicit"]["wave"], threads=32)))
    assert unreached(moved, "explicit", lists["explicit"]) != []


# ------------------------------------------------------------------------------------------------ the inputs of C and D
# Y and the ratings of the signed class times 2^e.  With s = 2^e the direct solve's matrix is s^2 G and its right-hand side
# s^2 b: the pivots handed to sqrt are s^2 times those of the unscaled row.  In the conjugate-gradient solve r is of order
# s^2, q of order s^4 and pq of order s^6, so its exponents are a third of the direct solve's.
DIRECT_SCALES = {"subnormal-pivots": -515.0, "large-pivots": 500.0, "overflow": 511.0}
CG_SCALES = {"subnormal-pq": -175.0, "near-overflow": 166.0, "overflow": 169.0}
SCALE_K = (10, 17, 100)
# the direct solve's lambdas: none, the modules' 0.05 / 0.3 (which a scaled Gram matrix swamps or vanishes under) and those
# times 2^(2e), which keep the ridge comparable with the matrix: every row is positive definite in exact arithmetic
DIRECT_LAMS = ("lambda0", "lambda", "scaled")
CG_LAMS = ("lambda0", "scaled")


def scaled_lam(name, e):
    if name == "lambda0":
        return LAM0
    if name == "lambda":
        return LAM
    return (LAM_U * 2.0 ** e * 2.0 ** e, LAM_I * 2.0 ** e * 2.0 ** e)


class Observer:
    """what the models hand to sqrt and divide by, of the rows still in the solve"""

    def __init__(self):
        self.pivots, self.divisors, self.gram, self.pq, self.rs = [], [], [], {}, {}

    def __call__(self, what, *a):
        if what == "pivot":
            self.pivots.append(a[1][a[2]])
        elif what == "divisor":
            self.divisors.append(a[1][a[2]])
        elif what == "gram":
            self.gram.append(a[1].ravel())
        else:
            getattr(self, what).setdefault(a[0], []).append((a[1], a[2]))

    def upto(self, what, step):
        """(rows, values) of the divisors `what` of steps 1 .. step"""
        seen = [rv for s, lst in getattr(self, what).items() if s <= step for rv in lst]
        return np.concatenate([r for r, _ in seen]), np.concatenate([v for _, v in seen])


def scale_inputs(K, e):
    pat = pattern("wide")
    L0, R0, val, _ = cls_signed(4500 + K, pat, K)
    return pat, L0, R0 * 2.0 ** e, val * 2.0 ** e


@functools.lru_cache(maxsize=None)
def direct_scale_expected(cls, K, lam_name):
    """one model iteration per kind of the direct solve on a scale class, the users' solve of "ridge" observed"""
    e = DIRECT_SCALES[cls]
    pat, L0, R0, val = scale_inputs(K, e)
    lam = scaled_lam(lam_name, e)
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
    x = type("Expected", (), {})()
    x.pat, x.L0, x.R0, x.val, x.lam, x.want, x.seen = pat, L0, R0, val, lam, {}, Observer()
    for kind in KINDS:
        L1, cu = m.solve(1, L0, R0, lam[0], kind, observer=x.seen if kind == "ridge" else None)
        R1, ci = m.solve(0, R0, L1, lam[1], kind)
        x.want[kind] = (L1, R1, cu, ci)
    check, _ = m.solve(1, L0, R0, lam[0], "ridge")   # the observer only looks
    assert_same_bits(check, x.want["ridge"][0], "observed and unobserved solve")
    return x


@functools.lru_cache(maxsize=None)
def cg_scale_expected(cls, K, lam_name):
    """the same for the conjugate-gradient solve after 1 and after 3 steps: want[kind, steps]"""
    e = CG_SCALES[cls]
    pat, L0, R0, val = scale_inputs(K, e)
    lam = scaled_lam(lam_name, e)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    x = type("Expected", (), {})()
    x.pat, x.L0, x.R0, x.val, x.lam, x.want, x.seen = pat, L0, R0, val, lam, {}, Observer()
    for kind in KINDS:
        users = m.solve(1, L0, R0, lam[0], kind, (1, 3), observer=x.seen if kind == "ridge" else None)
        for steps in (1, 3):
            L1, cu = users[steps]
            R1, ci = m.solve(0, R0, L1, lam[1], kind, steps)
            x.want[kind, steps] = (L1, R1, cu, ci)
    check = m.solve(1, L0, R0, lam[0], "ridge", 3)[0]
    assert_same_bits(check, x.want["ridge", 3][0], "observed and unobserved solve")
    return x


def changed_rows(new, old):
    return int((np.ascontiguousarray(new).view(np.uint64) != np.ascontiguousarray(old).view(np.uint64)).any(axis=1).sum())


@pytest.mark.parametrize("K", SCALE_K)
@pytest.mark.parametrize("cls", list(DIRECT_SCALES))
def test_direct_scale_classes_meet_their_conditions_on_the_model(cls, K):
    """The users' solve of kind "ridge".  With the ridge scaled like the matrix every row with entries is positive definite in
    exact arithmetic, and the class's condition holds at every K.  At lambda 0 a row of fewer than K entries is singular -- on
    `wide` that is every row at K = 100 and three quarters of them at K = 17 --, so "at least half of the rows solved" can hold
    at K = 10 only: there it is asserted at lambda 0 too, at the other K the values handed to sqrt alone."""
    with_entries = int((pattern("wide").ulen > 0).sum())
    for lam_name in ("lambda0", "scaled"):
        x = direct_scale_expected(cls, K, lam_name)
        cu = x.want["ridge"][2]
        pivots, G = np.concatenate(x.seen.pivots), np.concatenate(x.seen.gram)
        many = lam_name == "scaled" or K == 10
        print(cls, K, lam_name, cu, "pivots %g .. %g, subnormal %d, inf %d; Gram inf %d" % (
            pivots.min(), pivots.max(), int(is_subnormal(pivots).sum()), int(np.isinf(pivots).sum()), int(np.isinf(G).sum())))
        assert sum(cu) == x.pat.users and cu[1] == x.pat.users - with_entries and not np.isnan(G).any()
        if cls == "subnormal-pivots":
            assert is_subnormal(pivots).sum() >= 100 and pivots.max() < 2.0 ** -1022   # every pivot of a row that stays in the solve
            assert not many or cu[0] >= with_entries / 2
        elif cls == "large-pivots":
            assert np.isfinite(G).all() and (pivots[pivots > 0.0] > 2.0 ** 900).all() and pivots.max() > 2.0 ** 1000
            assert not many or cu[0] >= with_entries / 2
            assert np.isfinite(x.want["ridge"][0]).all()
        else:
            assert np.isposinf(G).sum() >= 100 and np.isposinf(pivots).any() and cu[2] > 0
            assert not many or cu[0] > 0
            if lam_name == "scaled":   # rows with and without an infinite pivot are solved: NaN rows and finite ones are stored
                assert 0 < int(np.isnan(x.want["ridge"][0]).any(axis=1).sum()) < cu[0]
    # the plain lambdas on the same inputs: what the scaled matrix swamps (or, subnormal, vanishes under)
    x = direct_scale_expected(cls, K, "lambda")
    if cls == "subnormal-pivots":
        assert x.want["ridge"][2][0] == with_entries and np.concatenate(x.seen.pivots).min() >= LAM_U


@pytest.mark.parametrize("K", SCALE_K)
@pytest.mark.parametrize("cls", list(CG_SCALES))
def test_cg_scale_classes_meet_their_conditions_on_the_model(cls, K):
    """The users' solve of kind "ridge", at lambda 0 and with lambda * 2^(2e)"""
    with_entries = int((pattern("wide").ulen > 0).sum())
    for lam_name in CG_LAMS:
        x = cg_scale_expected(cls, K, lam_name)
        for steps in (1, 3):
            L1, _, cu, _ = x.want["ridge", steps]
            rows, pq = x.seen.upto("pq", steps)
            changed = changed_rows(L1, x.L0)
            print(cls, K, lam_name, steps, cu, "changed %d, pq %g .. %g, subnormal %d, inf %d" % (
                changed, pq.min(), pq.max(), int(is_subnormal(pq).sum()), int(np.isinf(pq).sum())))
            assert sum(cu) == x.pat.users and cu[1] == x.pat.users - with_entries and not np.isnan(L1).any()
            if cls == "subnormal-pq":
                assert len(np.unique(rows[is_subnormal(pq)])) >= with_entries / 2 and changed >= with_entries / 2
            elif cls == "near-overflow":
                assert np.isfinite(pq).all() and pq.max() > 2.0 ** 1000 and cu[0] >= with_entries - 1 and changed >= with_entries - 1
            else:   # alpha = rs / inf = 0.0: the row is stored as solved and holds x0's bits
                assert len(np.unique(rows[np.isinf(pq)])) >= with_entries / 2 and 0 < changed < with_entries / 2


VALUE_CLASSES = ("range", "zeros", "nonfinite")


def class_inputs(cls, K):
    pat = pattern("wide")
    L0, R0, val, _ = CLASSES[cls](4600 + K, pat, K)
    return pat, L0, R0, val


@functools.lru_cache(maxsize=None)
def class_expected(solver, cls, K, lam):
    """{kind (direct), (kind, steps) (cg), None (implicit): (L1, R1, cu, ci)} of one value class on `wide`"""
    pat, L0, R0, val = class_inputs(cls, K)
    want = {}
    if solver == "direct":
        m = AlsModel(pat.users, pat.items, pat.row, pat.col, val)
        for kind in KINDS:
            want[kind] = m.iteration(L0, R0, lam, kind)
    elif solver == "cg":
        m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
        for kind in KINDS:
            users = m.solve(1, L0, R0, lam[0], kind, (1, 3))
            for steps in (1, 3):
                L1, cu = users[steps]
                R1, ci = m.solve(0, R0, L1, lam[1], kind, steps)
                want[kind, steps] = (L1, R1, cu, ci)
    else:
        want[None] = ImplicitModel(pat.users, pat.items, pat.row, pat.col, val).iteration(L0, R0, lam, CONF)
    return want


@pytest.mark.parametrize("cls", VALUE_CLASSES)
def test_value_classes_do_their_job_on_the_models(cls):
    """K = 10: what each class is there for shows in the models' results"""
    pat, L0, R0, val = class_inputs(cls, 10)
    with_entries = int((pat.ulen > 0).sum())
    for lam in (LAM0, LAM):
        d = class_expected("direct", cls, 10, lam)["ridge"]
        c = class_expected("cg", cls, 10, lam)["ridge", 3]
        i = class_expected("implicit", cls, 10, lam)[None]
        print(cls, lam, "direct", d[2], d[3], "cg", c[2], c[3], "implicit", i[2], i[3])
        assert sum(d[2]) == sum(c[2]) == sum(i[2]) == pat.users and sum(d[3]) == sum(c[3]) == sum(i[3]) == pat.items
        if cls == "range":      # factors and ratings over 80 binades: finite throughout, and most rows move
            assert all(np.isfinite(a).all() for w in (d, c, i) for a in w[:2])
            assert changed_rows(d[0], L0) >= with_entries / 2 and changed_rows(c[0], L0) >= with_entries / 2
        elif cls == "zeros":    # whole rows of zeros in Y: zero pivots and zero pq at lambda 0, none with a ridge
            assert (d[2][2] > 0 and d[3][2] > 0) if lam == LAM0 else (d[2][2] == 0 and c[2][2] == 0 and i[2][2] == 0)
        else:                   # a NaN row, infinities and 2^1000 on the planted rows: they reach a few rows of each side
            for w in (d, c):
                assert w[2][2] + w[3][2] > 0 and w[2][0] >= with_entries / 2
                assert 0 < int(np.isnan(w[1]).any(axis=1).sum()) + w[3][2] < pat.items / 2
            # the implicit solve starts every row at the Gram of the whole other side: the infinity in R reaches every user,
            # the NaN row of L (kept) every item, and every row of both sides is kept, as the header documents
            assert i[2] == (0, 0, pat.users) and i[3] == (0, 0, pat.items)
            assert_same_bits(i[0], L0, "implicit, nonfinite: L kept")
            assert_same_bits(i[1], R0, "implicit, nonfinite: R kept")


# ------------------------------------------------------------------------------------------------ D: the model's many steps
MANY_STEPS = (64, 255, 256)


@functools.lru_cache(maxsize=None)
def many_steps_expected(K, lam):
    """kind ridge-count on `wide`: {steps: (L1, R1, cu, ci)} from one run of the model per side and step count"""
    pat = pattern("wide")
    L0, R0, val, _ = cls_signed(4700 + K, pat, K)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    users = m.solve(1, L0, R0, lam[0], "ridge-count", MANY_STEPS)
    want = {}
    for steps in MANY_STEPS:
        L1, cu = users[steps]
        R1, ci = m.solve(0, R0, L1, lam[1], "ridge-count", steps)
        want[steps] = (L1, R1, cu, ci)
    return pat, L0, R0, val, want


@pytest.mark.parametrize("K", [10, 129])
def test_step_255_and_step_256_differ_on_the_model(K):
    """an exit one step early or late at the limit shows: at lambda 0 the last step still moves rows (rounding noise keeps rs
    away from 0.0); with the ridge no row turns out not positive definite in 256 steps"""
    pat, L0, R0, val, want = many_steps_expected(K, LAM0)
    moved = changed_rows(want[256][0], want[255][0])
    print(K, "rows of L that step 256 moves at lambda 0:", moved, "counters", want[255][2], want[256][2])
    assert moved >= 5 and changed_rows(want[255][0], want[64][0]) >= 5
    with_ridge = many_steps_expected(K, LAM)[4]
    assert all(with_ridge[s][2][2] == 0 and with_ridge[s][3][2] == 0 for s in MANY_STEPS)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def device(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.fixture
def switches(monkeypatch):
    """set_all(env): no switch but those of env -- none from the caller's environment, none from the call before"""
    keys = SWITCHES + ("MF_ALS_FORM", "MF_ALS_CG_FORM")

    def set_all(env):
        for k in keys:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    set_all({})
    return set_all


def run_and_compare(plan, L0, R0, want, where, iterate=False):
    """one hand-driven iteration, or one mf_plan_iterate, from (L0, R0) against (L1, R1, cu, ci)"""
    plan.upload(L0, R0)
    if iterate:
        plan.iterate(1)
        got = (plan.als_info("users"), plan.als_info("items"))
        assert got == want[2:], (where, got, want[2:])
    else:
        hand_iteration(plan, where, want[2:])
    L, R = plan.download()
    assert_same_bits(L, want[0], where + ": L")
    assert_same_bits(R, want[1], where + ": R")
    return L, R


# ---- A: the ends of the NB ranges
@gpu
@pytest.mark.parametrize("K", NB_EDGE_K)
def test_direct_solve_at_the_ends_of_the_nb_ranges(device, switches, K):
    capi = device
    for kind in KINDS:
        x = direct_expected("pair", K, kind)
        assert x.cu[0] > 600 and x.cu[2] == 0 and x.ci[2] == 0 and differs(x.L1, x.L0) > 0.9
        for form in direct_forms(K):
            switches({"MF_ALS_FORM": form})
            plan = als_plan(capi, x.pat, K, x.val, kind)
            try:
                direct_check_form(plan, form, kind)
                run_and_compare(plan, x.L0, x.R0, (x.L1, x.R1, x.cu, x.ci), "pair K=%d %s [%s]" % (K, kind, form))
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("K", NB_EDGE_K)
def test_implicit_solve_at_the_ends_of_the_nb_ranges(device, switches, K):
    capi = device
    weighted = bool(NB_EDGE_K.index(K) % 2)
    x = implicit_expected("pair", K, CONF, weighted)
    assert x.cu == (x.pat.users, 0, 0) and x.ci == (x.pat.items, 0, 0)
    for form in direct_forms(K):
        switches({"MF_ALS_FORM": form})
        plan = implicit_plan(capi, x.pat, K, x.val, CONF, weight=x.w)
        try:
            implicit_check_form(plan, form, CONF)
            run_and_compare(plan, x.L0, x.R0, (x.L1, x.R1, x.cu, x.ci), "pair K=%d weighted=%d [%s]" % (K, weighted, form))
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("K", WG_EDGE_K)
def test_gram_at_the_ends_of_the_nb_ranges(device, switches, K):
    """1025 users and 2049 items: two and three blocks of rows, the last of one row"""
    capi = device
    users, items = 1025, 2049
    pat = sparse_entries(users, items, 90 + K)
    plan = capi.Plan(users, items, K, 1e-3, pat.row, pat.col, np.ones(pat.nnz))
    try:
        nxt, cur = four_grams(plan, users, items, K, np.random.default_rng(9000 + K))
        for gen, (L, R) in (("current", cur), ("next", nxt)):
            assert_same_bits(plan.gram("users", gen), gram(L), "users %d x %d %s" % (users, K, gen))
            assert_same_bits(plan.gram("items", gen), gram(R), "items %d x %d %s" % (items, K, gen))
    finally:
        plan.close()


# ---- B: the split side
SPLIT = {"MF_SWEEP_LONG": "128"}


def check_split(capi, switches, make_plan, form_key, form, pat, K, inputs, want, where, sides="both"):
    """The plan of `make_plan` under `form` with the switch: the sides it must split, one hand-driven iteration and one
    mf_plan_iterate against the unsplit model; without the switch `skewed` splits nothing.

    An odd K has no split: the products form of the extreme-row path exists in the LDS-DMA sweep variants only, which take
    even K, so the plan of an odd K lists no extreme rows and describes none (no long_rows= at all).  Such a K is run all the
    same, and the description is asserted, so a products form for odd K shows here."""
    L0, R0 = inputs
    if pat.name == "skewed":
        switches({form_key: form})
        plan = make_plan()
        try:
            # long_rows= counts ALL rows of a side that a tiny sweep runs as one cooperative launch (coop_nch > 0; the small K
            # here): such a side has no extreme rows either, and the ALS launch does not look at it
            desc, n = plan.describe(), long_rows(plan.describe())
            whole = n is not None and " coop_nch=0 " not in desc and n[0] in (0, pat.items) and n[1] in (0, pat.users)
            assert (n == (0, 0) or whole) if K % 2 == 0 else n is None, desc
        finally:
            plan.close()
    switches(dict(SPLIT, **{form_key: form}))
    plan = make_plan()
    try:
        desc = plan.describe()
        n = long_rows(desc)
        assert "MF_SWEEP_LONG=128" in desc, desc
        if K % 2:
            assert n is None and desc.startswith("sweep_kernel<"), desc
        elif sides == "both":
            assert n is not None and 0 < n[0] < pat.items and 0 < n[1] < pat.users, desc
            assert n == (int((pat.ilen >= 128).sum()), int((pat.ulen >= 128).sum())), desc
        else:
            assert n is not None and 0 < n[0] < pat.items and n[1] == 0, desc
        assert sum(want[2]) == pat.users and sum(want[3]) == pat.items
        run_and_compare(plan, L0, R0, want, where + " split, hand-driven")
        run_and_compare(plan, L0, R0, want, where + " split, iterate", iterate=True)
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [10, 30, 100])
def test_split_side_direct(device, switches, K, kind):
    capi = device
    x = direct_expected("skewed", K, kind)
    for form in direct_forms(K):
        check_split(capi, switches, lambda: als_plan(capi, x.pat, K, x.val, kind), "MF_ALS_FORM", form, x.pat, K, (x.L0, x.R0),
                    (x.L1, x.R1, x.cu, x.ci), "skewed K=%d %s [%s]" % (K, kind, form))


@gpu
@pytest.mark.parametrize("K", [10, 100])
def test_split_side_implicit(device, switches, K):
    capi = device
    conf, weighted = _variant("skewed", K)
    x = implicit_expected("skewed", K, conf, weighted)
    for form in direct_forms(K):
        check_split(capi, switches, lambda: implicit_plan(capi, x.pat, K, x.val, conf, weight=x.w), "MF_ALS_FORM", form, x.pat, K, (x.L0, x.R0),
                    (x.L1, x.R1, x.cu, x.ci), "skewed K=%d conf=%g [%s]" % (K, conf, form))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [10, 64, 17, 256])
def test_split_side_cg(device, switches, K, kind):
    capi = device
    x = cg_expected("skewed", K, kind, 3)
    for form in cg_forms(K):
        check_split(capi, switches, lambda: cg_plan(capi, x.pat, K, x.val, kind, 3), "MF_ALS_CG_FORM", form, x.pat, K, (x.L0, x.R0),
                    (x.L1, x.R1, x.cu, x.ci), "skewed K=%d %s steps=3 [%s]" % (K, kind, form))


@functools.lru_cache(maxsize=None)
def split_not_pd_expected(solver, K):
    """`skewed` at lambda 0: a row of fewer than K entries is singular, kept or solved on rounding noise as the model decides"""
    pat = pattern("skewed")
    L0, R0, val, _ = cls_signed(4800 + K, pat, K)
    if solver == "direct":
        want = AlsModel(pat.users, pat.items, pat.row, pat.col, val).iteration(L0, R0, LAM0, "ridge")
    else:
        want = CgModel(pat.users, pat.items, pat.row, pat.col, val).iteration(L0, R0, LAM0, "ridge", 3)
    return pat, L0, R0, val, want


@pytest.mark.parametrize("solver,K", [("direct", 30), ("cg", 10)])
def test_split_inputs_keep_short_rows_as_not_positive_definite_on_the_model(solver, K):
    """both launches of a split side add to all three counters: the long rows are solved, among the short ones of the second
    launch some are kept as not positive definite, some are solved, and user 5 has no entries"""
    pat, L0, R0, val, want = split_not_pd_expected(solver, K)
    print(solver, K, want[2], want[3])
    for lens, old, new, counts in ((pat.ulen, L0, want[0], want[2]), (pat.ilen, R0, want[1], want[3])):
        moved = (np.ascontiguousarray(new).view(np.uint64) != np.ascontiguousarray(old).view(np.uint64)).any(axis=1)
        assert (lens >= 128).any() and moved[lens >= 128].all()
        assert counts[2] > 0 and (moved & (lens < 128)).any() and counts[2] <= int((~moved & (lens > 0) & (lens < 128)).sum())
    assert want[2][1] == 1 and pat.ulen[5] == 0


@gpu
@pytest.mark.parametrize("solver,K", [("direct", 30), ("cg", 10)])
def test_split_side_counts_rows_that_are_not_positive_definite(device, switches, solver, K):
    capi = device
    pat, L0, R0, val, want = split_not_pd_expected(solver, K)
    if solver == "direct":
        for form in direct_forms(K):
            check_split(capi, switches, lambda: als_plan(capi, pat, K, val, "ridge", LAM0), "MF_ALS_FORM", form, pat, K, (L0, R0), want,
                        "skewed K=%d lambda 0 [%s]" % (K, form))
    else:
        for form in cg_forms(K):
            check_split(capi, switches, lambda: cg_plan(capi, pat, K, val, "ridge", 3, LAM0), "MF_ALS_CG_FORM", form, pat, K, (L0, R0), want,
                        "skewed K=%d lambda 0 steps=3 [%s]" % (K, form))


@gpu
@pytest.mark.parametrize("solver", ["direct", "implicit", "cg"])
def test_split_of_the_item_side_alone(device, switches, solver):
    """`long-items`: items of up to 2600 entries, no user of 128"""
    capi = device
    pat = pattern("long-items")
    assert pat.ulen.max() < 128 <= pat.ilen.max()
    if solver == "direct":
        K = 30
        for kind in KINDS:
            x = direct_expected("long-items", K, kind)
            for form in direct_forms(K):
                check_split(capi, switches, lambda: als_plan(capi, pat, K, x.val, kind), "MF_ALS_FORM", form, pat, K, (x.L0, x.R0),
                            (x.L1, x.R1, x.cu, x.ci), "long-items K=%d %s [%s]" % (K, kind, form), sides="items")
    elif solver == "implicit":
        K = 10
        conf, weighted = _variant("long-items", K)
        x = implicit_expected("long-items", K, conf, weighted)
        for form in direct_forms(K):
            check_split(capi, switches, lambda: implicit_plan(capi, pat, K, x.val, conf, weight=x.w), "MF_ALS_FORM", form, pat, K, (x.L0, x.R0),
                        (x.L1, x.R1, x.cu, x.ci), "long-items K=%d conf=%g [%s]" % (K, conf, form), sides="items")
    else:
        K = 100
        for kind in KINDS:
            x = cg_expected("long-items", K, kind, 3)
            for form in cg_forms(K):
                check_split(capi, switches, lambda: cg_plan(capi, pat, K, x.val, kind, 3), "MF_ALS_CG_FORM", form, pat, K, (x.L0, x.R0),
                            (x.L1, x.R1, x.cu, x.ci), "long-items K=%d %s steps=3 [%s]" % (K, kind, form), sides="items")


# ---- C: value classes
LAMS = {"lambda0": LAM0, "lambda": LAM}


@gpu
@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("K", SCALE_K)
@pytest.mark.parametrize("cls", VALUE_CLASSES)
def test_value_classes_through_the_direct_solve(device, switches, cls, K, lam):
    capi = device
    pat, L0, R0, val = class_inputs(cls, K)
    want = class_expected("direct", cls, K, LAMS[lam])
    for kind in KINDS:
        for form in direct_forms(K):
            switches({"MF_ALS_FORM": form})
            plan = als_plan(capi, pat, K, val, kind, LAMS[lam])
            try:
                run_and_compare(plan, L0, R0, want[kind], "%s K=%d %s %s [%s]" % (cls, K, kind, lam, form))
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("K", SCALE_K)
@pytest.mark.parametrize("cls", VALUE_CLASSES)
def test_value_classes_through_the_cg_solve(device, switches, cls, K, lam):
    capi = device
    pat, L0, R0, val = class_inputs(cls, K)
    want = class_expected("cg", cls, K, LAMS[lam])
    for kind in KINDS:
        for steps in (1, 3):
            for form in cg_forms(K):
                switches({"MF_ALS_CG_FORM": form})
                plan = cg_plan(capi, pat, K, val, kind, steps, LAMS[lam])
                try:
                    run_and_compare(plan, L0, R0, want[kind, steps], "%s K=%d %s steps=%d %s [%s]" % (cls, K, kind, steps, lam, form))
                finally:
                    plan.close()


@gpu
@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("K", SCALE_K)
@pytest.mark.parametrize("cls", VALUE_CLASSES)
def test_value_classes_through_the_implicit_solve(device, switches, cls, K, lam):
    """a NaN or an infinity in Y reaches the Gram of the whole side and through it every row: kept, as the header says"""
    capi = device
    pat, L0, R0, val = class_inputs(cls, K)
    want = class_expected("implicit", cls, K, LAMS[lam])[None]
    for form in direct_forms(K):
        switches({"MF_ALS_FORM": form})
        plan = implicit_plan(capi, pat, K, val, CONF, LAMS[lam])
        try:
            run_and_compare(plan, L0, R0, want, "%s K=%d %s [%s]" % (cls, K, lam, form))
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("lam", DIRECT_LAMS)
@pytest.mark.parametrize("K", SCALE_K)
@pytest.mark.parametrize("cls", list(DIRECT_SCALES))
def test_scale_classes_through_the_direct_solve(device, switches, cls, K, lam):
    capi = device
    x = direct_scale_expected(cls, K, lam)
    for kind in KINDS:
        for form in direct_forms(K):
            switches({"MF_ALS_FORM": form})
            plan = als_plan(capi, x.pat, K, x.val, kind, x.lam)
            try:
                run_and_compare(plan, x.L0, x.R0, x.want[kind], "%s K=%d %s %s [%s]" % (cls, K, kind, lam, form))
            finally:
                plan.close()


@gpu
@pytest.mark.parametrize("lam", CG_LAMS)
@pytest.mark.parametrize("K", SCALE_K)
@pytest.mark.parametrize("cls", list(CG_SCALES))
def test_scale_classes_through_the_cg_solve(device, switches, cls, K, lam):
    capi = device
    x = cg_scale_expected(cls, K, lam)
    for kind in KINDS:
        for steps in (1, 3):
            for form in cg_forms(K):
                switches({"MF_ALS_CG_FORM": form})
                plan = cg_plan(capi, x.pat, K, x.val, kind, steps, x.lam)
                try:
                    run_and_compare(plan, x.L0, x.R0, x.want[kind, steps], "%s K=%d %s steps=%d %s [%s]" % (cls, K, kind, steps, lam, form))
                finally:
                    plan.close()


# ---- D: chunk sizes 12 to 15, and many steps
CHUNK_K = {189: 15, 190: 15, 200: 14, 213: 13, 214: 13, 226: 12, 255: 12, 256: 12}


def test_the_chunks_of_wide_k_and_the_row_lengths_that_go_with_them():
    pat = pattern("wide")
    assert pat.ulen[:38].tolist() == WIDE_LENS and pat.ilen[65:103].tolist() == WIDE_LENS
    for K, chunk in CHUNK_K.items():
        assert chunk_of(K) == chunk and cg_passes(K) == 2
        assert {chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1} <= set(WIDE_LENS), K
        # phase_b_four leaves every tail: 0 .. 3 entries behind whole fours in a chunk of a row
        assert {min(chunk, n - c0) % 4 for n in WIDE_LENS for c0 in range(0, n, chunk)} == {0, 1, 2, 3}
    assert cg_forms(190) == ["dma", "general"] and cg_forms(189) == ["general"] and cg_forms(256) == ["fixed", "dma", "general"]


@gpu
@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("K", list(CHUNK_K))
def test_row_lengths_around_the_chunks_of_the_two_pass_kernels(device, switches, K, lam):
    """`wide` has users and items of 0 .. 34, 63, 64 and 65 entries: chunk - 1, chunk, chunk + 1, 2 chunk and 2 chunk + 1 of the
    chunks 15, 14, 13 and 12 these K have.  At lambda 0 every row is singular (no row has K entries): kept or solved as the
    model decides"""
    capi = device
    pat = pattern("wide")
    chunk = chunk_of(K)
    assert chunk == CHUNK_K[K] and {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1} <= set(pat.ulen[:38]) and pat.ulen[:38].tolist() == pat.ilen[65:103].tolist()
    L0, R0, val, _ = cls_signed(4100 + K, pat, K)
    m = CgModel(pat.users, pat.items, pat.row, pat.col, val)
    for kind in KINDS:
        users = m.solve(1, L0, R0, LAMS[lam][0], kind, (1, 3))
        for steps in (1, 3):
            L1, cu = users[steps]
            R1, ci = m.solve(0, R0, L1, LAMS[lam][1], kind, steps)
            assert cu[1] > 0 and (lam != "lambda" or (cu[2] == 0 and ci[2] == 0))
            for form in cg_forms(K):
                switches({"MF_ALS_CG_FORM": form})
                plan = cg_plan(capi, pat, K, val, kind, steps, LAMS[lam])
                try:
                    cg_check_form(plan, form, kind, steps, K)
                    run_and_compare(plan, L0, R0, (L1, R1, cu, ci), "wide K=%d %s steps=%d [%s] %s" % (K, kind, steps, form, lam))
                finally:
                    plan.close()


@gpu
@pytest.mark.parametrize("lam", list(LAMS))
@pytest.mark.parametrize("K", [10, 129])
def test_many_steps_and_the_exit_at_the_limit(device, switches, K, lam):
    capi = device
    pat, L0, R0, val, want = many_steps_expected(K, LAMS[lam])
    assert cg_mod.MAX_STEPS == MANY_STEPS[-1]
    for steps in MANY_STEPS:
        for form in cg_forms(K):
            switches({"MF_ALS_CG_FORM": form})
            plan = cg_plan(capi, pat, K, val, "ridge-count", steps, LAMS[lam])
            try:
                cg_check_form(plan, form, "ridge-count", steps, K)
                run_and_compare(plan, L0, R0, want[steps], "wide K=%d steps=%d [%s] %s" % (K, steps, form, lam))
            finally:
                plan.close()
