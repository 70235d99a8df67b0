"""Per-entry confidence weights (mf_plan_create_weighted, mf_plan_weight_total, mf_backend_run_weighted, MATFACT_WEIGHTS).

The definition is the library's own (include/matfact_hip.h).  A plan may carry one weight w_n per training entry, in the
entries' order; in every sweep of either side

    e_n = (c2 * (val_n - dot_n)) * w_n        the plain e_n first, then one more rounded multiply, nothing fused

and everything behind e_n -- seed, decay, frozen column, momentum, the order of the sum -- is untouched.  The training loss
of a weighted plan has q_n = (d_n * d_n) * w_n; the held-out loss stays unweighted.  The model below is numpy on the CPU
and follows that text on top of test_momentum's model; every GPU comparison is bit for bit (assert_same_bits of
test_sweep_edges.py).  The weights are uniform in [0.25, 4): inexact, so a reassociated product shows; 0.0, 1.0, 2^-1030 and
2^600 are planted on a few entries of ordinary rows and of the planted short rows.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in, to_text
from test_iterate_path import iterate_path_of, path_of_plan, toy_lds_bytes
from test_loss import KS as LOSS_KS
from test_loss import loss_shape
from test_loss import instance as loss_instance
from test_loss import model_p, model_total, seq_sum
from test_momentum import BETA, BETA_I, BETA_U, LAM, MModel, msweep, random_prev
from test_momentum import expected as momentum_expected
from test_regularised import CASES, LAM_I, LAM_U, LARGE, WIDE, ZERO_FORMS, _case_id, _pick, _small, _toy, decay, differs, fast_dot
from test_sweep_edges import (GRID_CAP, PF_ROWS, SINGLE, SWEEPS, SWITCHES, _single_wave, assert_same_bits, cls_signed, is_negzero, pattern,
                              pattern_both_large, seq_dot, signed_inputs)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa  # noqa: E402

gpu = pytest.mark.gpu

SPECIAL_WEIGHTS = [0.0, 1.0, 2.0 ** -1030, 2.0 ** 600]


# ------------------------------------------------------------------------------------------------ the model
def e_definition(c2, val, dot, w):
    """e_n = (c2 * (val_n - dot_n)) * w_n: three roundings, in this order"""
    d = val - dot
    e = c2 * d
    return e * w


def e_mutant_weight_on_c2(c2, val, dot, w):
    return (c2 * w) * (val - dot)


def e_mutant_weight_on_d(c2, val, dot, w):
    return c2 * (w * (val - dot))


def e_mutant_weight_on_val(c2, val, dot, w):
    return c2 * ((w * val) - dot)


MUTANTS = {"(c2 * w) * d": e_mutant_weight_on_c2, "c2 * (w * d)": e_mutant_weight_on_d, "c2 * ((w * val) - dot)": e_mutant_weight_on_val}


def plain_weights(seed, nnz):
    return np.random.default_rng(seed).uniform(0.25, 4.0, nnz)


def planted_weights(seed, pat):
    """uniform(0.25, 4) with 0.0, 1.0, 2^-1030 and 2^600 on eight entries of ordinary rows and eight of the planted short rows"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, pat.nnz)
    short = np.isin(pat.row, pat.planted_users) | np.isin(pat.col, pat.planted_items)
    for pool in (np.flatnonzero(~short), np.flatnonzero(short)):
        w[rng.choice(pool, 8, replace=False)] = SPECIAL_WEIGHTS * 2
    return w


class WModel(MModel):
    """test_momentum's model with one weight per entry, in the entries' order"""

    def __init__(self, users, items, row, col, val, alpha, w):
        super().__init__(users, items, row, col, val, alpha)
        self.w = np.asarray(w, np.float64)
        assert self.w.shape == self.val.shape

    def wstep(self, L, R, Lp=None, Rp=None, lam=LAM, beta=BETA, seed_u=True, seed_i=True, dot=seq_dot, frozen=(-1, -1), e_of=e_definition,
              w_users=None, w_items=None):
        """(L_new, R_new) of one iteration from the frozen L, R with the histories Lp, Rp (None: at rest); lam, beta and frozen
        are (users, items).  w_users / w_items: the weights a mutant gives one side."""
        with np.errstate(all="ignore"):
            c2 = self.alpha * 2
            p = dot(L, R, self.row, self.col)
            eu = e_of(c2, self.val, p, self.w if w_users is None else w_users)
            ei = e_of(c2, self.val, p, self.w if w_items is None else w_items)
            Ln = msweep(L, L if Lp is None else Lp, R, eu, self.us, self.col, decay(self.alpha, lam[0]), beta[0], seed_u, frozen[0])
            Rn = msweep(R, R if Rp is None else Rp, L, ei, self.its, self.row, decay(self.alpha, lam[1]), beta[1], seed_i, frozen[1])
        return Ln, Rn

    def wrun(self, L, R, iters, lam=LAM, beta=BETA, prev=(None, None), frozen=(-1, -1)):
        Lp, Rp = prev
        for _ in range(iters):
            Ln, Rn = self.wstep(L, R, Lp, Rp, lam, beta, dot=fast_dot, frozen=frozen)
            Lp, Rp, L, R = L, R, Ln, Rn
        return L, R, Lp, Rp


def position_mutant(own, w):
    """the weights a side would see if the file-order array were read at the side's own positions: the entry at position q of
    the side's order (stable by `own`) takes w[q]"""
    order = np.argsort(own, kind="stable")
    out = np.empty_like(w)
    out[order] = w[:len(order)]
    return out


def wmodel_rows(L, R, row, col, val, w, users, user_begin=0):
    """weighted row sums of the loss: q_n = (d_n * d_n) * w_n, added per user in entry order from 0.0"""
    row = np.asarray(row, np.int64) - user_begin
    with np.errstate(all="ignore"):
        d = np.asarray(val, np.float64) - model_p(L, R, row, np.asarray(col, np.int64))
        q = d * d
        if w is not None:
            q = q * w
        return entry_order_sums(q, row, users)


def entry_order_sums(q, row, users):
    order = np.argsort(row, kind="stable")
    ptr = np.searchsorted(row[order], np.arange(users + 1))
    q = np.asarray(q, np.float64)[order]
    with np.errstate(all="ignore"):
        return np.array([seq_sum(q[ptr[i]:ptr[i + 1]]) for i in range(users)], np.float64).reshape(users)


@functools.lru_cache(maxsize=None)
def expected(pat_name, cls, K):
    """test_momentum's inputs of one (pattern, class, K) with the planted weights, and the weighted model's results."""
    u = momentum_expected(pat_name, cls, K)
    x = type("Expected", (), {})()
    x.pat, x.K, x.L0, x.R0, x.val, x.alpha, x.Lp, x.Rp, x.unweighted = u.pat, K, u.L0, u.R0, u.val, u.alpha, u.Lp, u.Rp, u
    pat = x.pat
    x.w = planted_weights(9000 + K, pat)
    m = x.model = WModel(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha, x.w)
    x.seeded = m.wstep(x.L0, x.R0, x.Lp, x.Rp)
    x.unseeded = m.wstep(x.L0, x.R0, x.Lp, x.Rp, seed_u=False, seed_i=False)
    x.rest1 = m.wstep(x.L0, x.R0)
    x.rest2 = m.wstep(*x.rest1, x.L0, x.R0)
    if cls == "signed":
        check_guards(x, pat_name)
    return x


def check_guards(x, where):
    """asserted on the model itself, so that the inputs keep doing their job: weighting shows in more than half of the
    elements of each factor, and the definition differs somewhere in each factor from every mutant"""
    m, pat = x.model, x.pat
    assert differs(x.seeded[0], x.unweighted.seeded[0]) > 0.5 and differs(x.seeded[1], x.unweighted.seeded[1]) > 0.5, where
    for name, e_of in MUTANTS.items():
        got = m.wstep(x.L0, x.R0, x.Lp, x.Rp, e_of=e_of)
        assert differs(got[0], x.seeded[0]) > 0.0 and differs(got[1], x.seeded[1]) > 0.0, (where, name)
    ones = np.ones(pat.nnz)
    users_only = m.wstep(x.L0, x.R0, x.Lp, x.Rp, w_items=ones)
    items_only = m.wstep(x.L0, x.R0, x.Lp, x.Rp, w_users=ones)
    assert differs(users_only[1], x.seeded[1]) > 0.5 and differs(items_only[0], x.seeded[0]) > 0.5, (where, "one side only")
    assert_same_bits(users_only[0], x.seeded[0], "weights on the users' side only: L is the definition's")
    # the file is row-sorted and not column-sorted: file-order weights read at CSC positions give the items other weights
    assert (np.diff(pat.row) >= 0).all() and not (np.diff(pat.col) >= 0).all()
    moved = m.wstep(x.L0, x.R0, x.Lp, x.Rp, w_items=position_mutant(pat.col, x.w))
    assert differs(moved[1], x.seeded[1]) > 0.5, (where, "permutation mutant")


# ------------------------------------------------------------------------------------------------ CPU
WEIGHT_SYMBOLS = ("mf_plan_create_weighted", "mf_plan_weight_total", "mf_backend_run_weighted")


def test_weight_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in WEIGHT_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr)
    assert capi.hip().mf_backend_abi_version() == 5
    assert "e_n  = (c2 * (val_n - dot_n)) * w_n" in hdr and "q_n = (d_n * d_n) * w_n" in hdr
    assert "mf_backend_run_multi does not weight" in hdr and "comes out +0.0" in hdr
    assert callable(capi.Plan.weight_total) and callable(capi.run_weighted) and callable(capi.backend_run_weighted)


def test_weight_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    w = np.ones(4)
    out = C.c_void_p()
    total = C.c_double()
    assert h.mf_plan_create_weighted(None, None, w.ctypes.data) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_create_weighted(C.byref(out), None, w.ctypes.data) == capi.MF_ERR_ARGUMENT and not out.value
    bad = capi.Shard()
    bad.users_total, bad.items, bad.features, bad.user_count, bad.nnz = 3, 3, 0, 3, 0   # features < 1
    assert h.mf_plan_create_weighted(C.byref(out), C.byref(bad), w.ctypes.data) == capi.MF_ERR_ARGUMENT and not out.value
    assert h.mf_plan_weight_total(None, C.byref(total), None) == capi.MF_ERR_ARGUMENT
    inst = capi.parse_file(golden_in("inst0"))
    p, keep = capi._problem(inst)
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    wi = np.ones(inst.nnz)
    ok = (0.1, 0.1, 0.5, 0.5)
    assert h.mf_backend_run_weighted(None, wi.ctypes.data, L.ctypes.data, R.ctypes.data, None, *ok, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_run_weighted(C.byref(p), wi.ctypes.data, None, R.ctypes.data, None, *ok, 0) == capi.MF_ERR_ARGUMENT
    assert h.mf_backend_run_weighted(C.byref(p), wi.ctypes.data, L.ctypes.data, None, None, *ok, 0) == capi.MF_ERR_ARGUMENT
    for v in (-0.5, float("nan"), float("inf")):
        for args in ((v, 0.1, 0.5, 0.5), (0.1, v, 0.5, 0.5), (0.1, 0.1, v, 0.5), (0.1, 0.1, 0.5, v)):
            assert h.mf_backend_run_weighted(C.byref(p), wi.ctypes.data, L.ctypes.data, R.ctypes.data, None, *args, 0) == capi.MF_ERR_ARGUMENT, args
    L2, R2 = capi.init_factors(inst.users, inst.items, inst.feats)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)   # a refused call touches nothing


@pytest.mark.parametrize("K", [3, 6, 100])
@pytest.mark.parametrize("pat_name", ["pair", "long-items", "skewed"])
def test_model_guards_and_weights_of_one(pat_name, K):
    """expected() asserts the guards; with all weights 1.0 the model is test_momentum's, bit for bit, seeded, unseeded and
    from rest; a zero weight gives a zero product, and a -0.0 accumulator that meets a +0.0 product comes out +0.0."""
    x = expected(pat_name, "signed", K)
    u, pat = x.unweighted, x.pat
    one = WModel(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha, np.ones(pat.nnz))
    for got, want, what in ((one.wstep(x.L0, x.R0, x.Lp, x.Rp), u.seeded, "seeded"),
                            (one.wstep(x.L0, x.R0, x.Lp, x.Rp, seed_u=False, seed_i=False), u.unseeded, "unseeded"),
                            (one.wstep(x.L0, x.R0), u.rest1, "from rest")):
        assert_same_bits(got[0], want[0], "weights 1.0, %s, L" % what)
        assert_same_bits(got[1], want[1], "weights 1.0, %s, R" % what)
    assert sorted(set(x.w[np.isin(x.w, SPECIAL_WEIGHTS)])) == sorted(SPECIAL_WEIGHTS)
    z = e_definition(2e-3, np.array([1.0, -1.0]), np.zeros(2), np.zeros(2))
    assert (z == 0.0).all() and is_negzero(z).tolist() == [False, True]
    assert not is_negzero(np.array([-0.0]) + z[:1] * 0.5).any() and is_negzero(np.array([-0.0]) + z[1:] * 0.5).all()


@pytest.mark.parametrize("users", [1, 1023, 1025, 3000])
def test_host_total_of_row_weight_sums_equals_the_blocked_model(capi, users):
    """mf_backend_loss_total is the host twin of mf_plan_weight_total's total: blocks cut at global multiples of 1024,
    user_begin inside a block."""
    rng = np.random.default_rng(users)
    lens = rng.integers(0, 9, users)
    row = np.repeat(np.arange(users), lens)
    w = rng.uniform(0.25, 4.0, len(row)) * 10.0 ** rng.integers(-6, 7, len(row))
    s = entry_order_sums(w, row, users)
    acc = 0.0
    first = int(np.flatnonzero(lens)[0]) if lens.any() else 0
    for v in w[row == first]:
        acc = acc + v
    assert_same_bits(np.array([s[first]]), np.array([acc]), "row sum of weights is sequential")
    for begin in (700, 0):
        assert_same_bits(np.array([capi.loss_total(s, begin)]), np.array([model_total(s, begin)]), "begin %d" % begin)


FORBIDDEN = [dict(MATFACT_DEVICES="0"), dict(MATFACT_MATS="/dev/null"), dict(MATFACT_CHECKPOINT="x.ck"), dict(MATFACT_RESUME="x.ck"),
             dict(MATFACT_TOPN="3"), dict(MATFACT_SIMILAR="3", MATFACT_SIMILAR_OUT="sim.out")]


def _weights_file(path, inst, w, row=None, col=None):
    d = dict(iters=inst.iters, alpha=inst.alpha, feats=inst.feats, users=inst.users, items=inst.items,
             row=inst.row if row is None else row, col=inst.col if col is None else col, val=w)
    with open(path, "w") as f:
        f.write(to_text(d))
    return str(path)


def _cli(capi, path, cwd=None, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    return subprocess.run([capi.CLI_PATH, path], capture_output=True, cwd=cwd, env=dict(clean, **env))


@pytest.mark.parametrize("env", FORBIDDEN, ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_cli_weights_refusals_die_with_empty_stdout(capi, env, tmp_path):
    inst = capi.parse_file(golden_in("inst0"))
    wf = _weights_file(tmp_path / "w.in", inst, np.ones(inst.nnz))
    r = _cli(capi, golden_in("inst0"), cwd=tmp_path, MATFACT_WEIGHTS=wf, **env)
    assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_WEIGHTS works on the single-GPU path only" in r.stderr, r
    assert len(r.stderr.decode().strip().splitlines()) == 1, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["w.in"]


def test_cli_weights_file_must_match_the_input(capi, tmp_path):
    inst = capi.parse_file(golden_in("inst0"))
    assert inst.nnz >= 3
    r = _cli(capi, golden_in("inst0"), cwd=tmp_path, MATFACT_WEIGHTS=str(tmp_path / "missing.in"))
    assert r.returncode == 255 and r.stdout == b"" and b"Unable to open input file." in r.stderr, r
    fewer = capi.Instance(inst.iters, inst.alpha, inst.feats, inst.users, inst.items, inst.row[:-1], inst.col[:-1], inst.val[:-1])
    col = inst.col.copy()
    free = next(c for c in range(inst.items) if not ((inst.row == inst.row[1]) & (inst.col == c)).any())
    col[1] = free                                           # one pair changed, the count kept
    cases = {"count": _weights_file(tmp_path / "count.in", fewer, np.ones(inst.nnz - 1)),
             "pair": _weights_file(tmp_path / "pair.in", inst, np.ones(inst.nnz), col=col),
             "size": _weights_file(tmp_path / "size.in", capi.Instance(inst.iters, inst.alpha, inst.feats, inst.users + 1, inst.items,
                                                                       inst.row, inst.col, inst.val), np.ones(inst.nnz))}
    for what, wf in cases.items():
        r = _cli(capi, golden_in("inst0"), cwd=tmp_path, MATFACT_WEIGHTS=wf)
        assert r.returncode == 255 and r.stdout == b"" and b"MATFACT_WEIGHTS: the file must hold the input's" in r.stderr, (what, r)


def test_the_recorded_option_matrix_still_passes(capi, tmp_path):
    """the command line's answers to every recorded combination of the older options are unchanged: the existing test, run
    as it is"""
    import test_cli
    test_cli.test_cli_option_matrix_is_the_recorded_one(capi, tmp_path)


WEIGHTED_KERNELS = (r"mf::sweep_dma_kernel<\d+, \d+, [5-8], \d+>", r"mf::sweep_kernel<\d+, \d+, (true|false), true>",
                    r"mf::sweep_db_kernel<\d+, \d+, (true|false), true>", r"mf::sweep_pair_kernel<\d+, 1, (true|false), true>",
                    r"mf::sweep_coop_kernel<\d+, (true|false), true>", r"mf::sweep_resident_kernel<\d+, (true|false), true>",
                    r"mf::loss_dma_w_kernel<\d+, \d+>", r"mf::loss_reg_w_kernel", r"mf::weight_rows_kernel")


def _unweighted_twin(name):
    """the decay / momentum / products / errors (or unweighted loss) instance a weighted instance was built on"""
    m = re.search(r"mf::sweep_dma_kernel<(\d+), (\d+), ([5-8]), (\d+)>", name)
    if m:
        mode = {"5": "3", "6": "4", "7": "1", "8": "2"}[m.group(3)]
        return name.replace(m.group(0), "mf::sweep_dma_kernel<%s, %s, %s, %s>" % (m.group(1), m.group(2), mode, m.group(4)))
    if "loss_dma_w_kernel" in name or "loss_reg_w_kernel" in name:
        return name.replace("_w_kernel", "_kernel")
    return name.replace(", true>(mf::", ", false>(mf::")


def test_weighted_instances_isa():
    """Every weighted instance of the built library: no fused multiply-add, nothing in scratch, and more v_mul_f64 than its
    unweighted twin -- the multiply by the weight where e_n (q_n in the loss) is formed; the instances exist in the numbers
    the variant tables ask for."""
    if not isa.have_tools() or not os.path.exists(isa.DEFAULT_LIB):
        pytest.skip("needs llvm-objdump/llvm-readelf/c++filt and the built library")
    kernels, meta = isa.disassemble(), isa.metadata()
    found = {pat: [n for n in kernels if re.search(pat, n)] for pat in WEIGHTED_KERNELS}
    # LDS-DMA form: modes 5 / 6 plain (K <= 128) and pipelined, 7 and 8, for seven K; four modes for four run-time-K widths
    assert len(found[WEIGHTED_KERNELS[0]]) == 6 * 6 + 4 + 4 * 4, sorted(found[WEIGHTED_KERNELS[0]])
    assert len(found[WEIGHTED_KERNELS[1]]) == 2 * 14 and len(found[WEIGHTED_KERNELS[2]]) == 2 * 11
    assert len(found[WEIGHTED_KERNELS[3]]) == 2 * 2 and len(found[WEIGHTED_KERNELS[4]]) == 2 * 7 and len(found[WEIGHTED_KERNELS[5]]) == 2 * 4
    assert len(found[WEIGHTED_KERNELS[6]]) == 11 and len(found[WEIGHTED_KERNELS[7]]) == 1 and len(found[WEIGHTED_KERNELS[8]]) == 1
    for names in found.values():
        for n in names:
            body = kernels[n]
            fused = [i for i in body if re.match(r"v_(fma|fmac|mad|pk_fma)\w*_f64", i)]
            assert not fused, (n, fused[:3])
            assert not [i for i in body if i.startswith("scratch_")], n
            m = meta[n]
            assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0, (n, m)
            if "weight_rows" not in n:
                twin = _unweighted_twin(n)
                assert twin in kernels, (n, twin)
                muls = [sum(1 for i in kernels[k] if isa.split(i)[0].startswith("v_mul_f64")) for k in (n, twin)]
                assert muls[0] > muls[1] > 0, (n, twin, muls)


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


def _plan(capi, pat, K, val, alpha, w, lam=LAM, beta=BETA, **kw):
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val, weight=w, **kw)
    plan.set_regularization(*lam)
    plan.set_momentum(*beta)
    return plan


def _null_weight_plan(capi, pat, K, val, alpha):
    """a Plan made by mf_plan_create_weighted with weight == NULL, which the Python class does not offer"""
    plan = capi.Plan.__new__(capi.Plan)
    plan.users_total, plan.items, plan.feats, plan.user_begin, plan.user_count, plan.nnz = pat.users, pat.items, K, 0, pat.users, pat.nnz
    row, col, v = np.ascontiguousarray(pat.row, np.int32), np.ascontiguousarray(pat.col, np.int32), np.ascontiguousarray(val, np.float64)
    s = capi.Shard()
    s.users_total, s.items, s.features, s.user_begin, s.user_count, s.nnz = pat.users, pat.items, K, 0, pat.users, pat.nnz
    s.row, s.col, s.val, s.alpha = row.ctypes.data, col.ctypes.data, v.ctypes.data, float(alpha)
    plan._h = C.c_void_p()
    plan.weighted = False
    rc = capi.hip().mf_plan_create_weighted(C.byref(plan._h), C.byref(s), None)
    assert rc == capi.MF_OK, rc
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
def test_weighted_sweeps_through_every_form(device, switches, case):
    """A seeded step with a chosen history, an unseeded step, and two iterate(1) from rest against the model -- in every sweep
    form, at the rule's chunk size and at 5, at lambda 0.05 / 0.3 and beta 0.9 / 0.3; the plan says weighted=1 and names the
    form the unweighted plan of the same case takes."""
    capi = device
    K = case["K"]
    x = expected(case["pat"], "signed", K)
    switches(case["env"])
    if case["nch"]:
        switches({"MF_SWEEP_NCH": case["nch"]})
    plain = _plan(capi, x.pat, K, x.val, x.alpha, None)
    plain_desc = plain.describe()
    plain.close()
    plan = _plan(capi, x.pat, K, x.val, x.alpha, x.w)
    try:
        desc = plan.describe()
        assert case["check"](desc, K), desc
        assert ("MF_SWEEP_NCH=5" in desc) == (case["nch"] == "5"), desc
        assert " weighted=1" in desc and "weighted" not in plain_desc and desc.replace(" weighted=1", "") == plain_desc, (desc, plain_desc)
        where = "%s [%s]" % (_case_id(case), desc.split(" loss=")[0])
        if case["steps"]:
            L, R = _step(plan, x.L0, x.R0, (x.Lp, x.Rp), True, True)
            assert_same_bits(R, x.seeded[1], where + ": seeded item sweep")
            assert_same_bits(L, x.seeded[0], where + ": seeded user sweep")
            L, R = _step(plan, x.L0, x.R0, (x.Lp, x.Rp), False, False)
            assert_same_bits(R, x.unseeded[1], where + ": item sweep from zero")
            assert_same_bits(L, x.unseeded[0], where + ": user sweep from zero")
        plan.upload(x.L0, x.R0)
        plan.upload_previous(x.Lp, x.Rp)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.seeded[0], where + ": L after iterate(1) with a chosen history")
        assert_same_bits(R, x.seeded[1], where + ": R after iterate(1) with a chosen history")
        plan.upload(x.L0, x.R0)
        plan.iterate(1)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, x.rest2[0], where + ": L after two iterations from rest")
        assert_same_bits(R, x.rest2[1], where + ": R after two iterations from rest")
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("name,K", ZERO_FORMS, ids=lambda v: str(v))
def test_plain_decay_only_and_weights_of_one(device, orc, switches, name, K):
    """A weighted plan with lambda and beta at 0 (the decay-weighted instance at d = 1.0) and one with lambda only equal the
    model; a plan created with weight = NULL, and one with all weights 1.0, give the oracle's plain bits, and the NULL plan's
    describe string is the unweighted plan's."""
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], "signed", K)
    pat, m = x.pat, x.model
    switches(case["env"])
    zero = (0.0, 0.0)
    for lam in (zero, LAM):
        one = m.wstep(x.L0, x.R0, lam=lam, beta=zero)
        two = m.wstep(*one, lam=lam, beta=zero)
        assert differs(one[0], m.wstep(x.L0, x.R0, lam=LAM if lam == zero else zero, beta=zero)[0]) > 0.5
        plan = _plan(capi, pat, K, x.val, x.alpha, x.w, lam=lam, beta=zero)
        try:
            desc = plan.describe()
            assert case["check"](desc, K) and " weighted=1" in desc and "momentum=" not in desc and ("lambda=" in desc) == (lam != zero), desc
            where = "%s K=%d lambda=%s" % (name, K, lam)
            if case["steps"]:
                L, R = _step(plan, x.L0, x.R0, None, True, True)
                assert_same_bits(R, one[1], where + ": item sweep")
                assert_same_bits(L, one[0], where + ": user sweep")
            plan.upload(x.L0, x.R0)
            plan.iterate(2)
            L, R = plan.download()
            assert_same_bits(L, two[0], where + ": L after two iterations")
            assert_same_bits(R, two[1], where + ": R after two iterations")
        finally:
            plan.close()
    with np.errstate(all="ignore"):
        seeded = orc.tile_step(0, pat.users, 0, pat.items, K, pat.row, pat.col, x.val, x.alpha, x.L0, x.R0, True, True)
        L2, R2 = x.L0.copy(), x.R0.copy()
        orc.factorize(orc.Instance(2, x.alpha, K, pat.users, pat.items, pat.row, pat.col, x.val), L2, R2)
    ref = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    ref_desc = ref.describe()
    ref.close()
    for null in (True, False):
        plan = (_null_weight_plan(capi, pat, K, x.val, x.alpha) if null else
                capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val, weight=np.ones(pat.nnz)))
        try:
            desc = plan.describe()
            assert case["check"](desc, K) and (desc == ref_desc if null else desc.replace(" weighted=1", "") == ref_desc), (desc, ref_desc)
            where = "%s K=%d %s" % (name, K, "weight NULL" if null else "weights 1.0")
            if null:
                with pytest.raises(capi.HipBackendError) as err:
                    plan.weight_total()
                assert err.value.status == capi.MF_ERR_STATE
            if case["steps"]:
                L, R = _step(plan, x.L0, x.R0, None, True, True)
                assert_same_bits(L, seeded[0], where + " L")
                assert_same_bits(R, seeded[1], where + " R")
            plan.upload(x.L0, x.R0)
            plan.iterate(2)
            L, R = plan.download()
            assert_same_bits(L, L2, where + " L after two")
            assert_same_bits(R, R2, where + " R after two")
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("beta", [BETA, (0.0, 0.0)], ids=["momentum", "decay"])
@pytest.mark.parametrize("name", list(LARGE))
def test_plain_weighted_instances_above_262144_rows(device, switches, name, beta):
    """sweep_dma_kernel<K, 1, weighted decay | weighted momentum> without the pipelined phases is what a weighted sweep of
    more than 262144 rows launches (a weighted cfg4 user sweep); no smaller launch reaches them.  The shapes of
    test_plain_decay_instances_above_262144_rows: both sides just above 262144 rows at K = 10 and K = 100, and 2^20 + 130
    users, where the launch is capped at 2^20 workgroups and 130 of them walk a second row.  One seeded and one unseeded step
    against the model, every row of both factors."""
    capi = device
    K, env, make, form = LARGE[name]
    switches(env)
    pat = make()
    assert max(pat.users, pat.items) > PF_ROWS and (name != "users-2^20-K10" or pat.users > GRID_CAP)
    L0, R0, val = signed_inputs(7000 + K, pat, K)
    Lp, Rp = random_prev(7100, L0), random_prev(7200, R0)
    alpha = 1e-3
    w = plain_weights(7300, pat.nnz)
    m = WModel(pat.users, pat.items, pat.row, pat.col, val, alpha, w)
    unweighted = MModel(pat.users, pat.items, pat.row, pat.col, val, alpha).mstep(L0, R0, Lp, Rp, beta=beta)
    plan = _plan(capi, pat, K, val, alpha, w, beta=beta)
    try:
        desc = plan.describe()
        assert form in desc and _single_wave(desc, K, K) and " weighted=1" in desc, desc
        for seed in (True, False):
            want = m.wstep(L0, R0, Lp, Rp, beta=beta, seed_u=seed, seed_i=seed)
            if seed:
                assert differs(want[0], unweighted[0]) > 0.5 and differs(want[1], unweighted[1]) > 0.5
            L, R = _step(plan, L0, R0, (Lp, Rp), seed, seed)
            assert_same_bits(R, want[1], "%s: item sweep, seed=%s beta=%s" % (name, seed, beta))
            assert_same_bits(L, want[0], "%s: user sweep, seed=%s beta=%s" % (name, seed, beta))
    finally:
        plan.close()


PERMUTED = [("dma", SINGLE, 30), ("es", {"MF_ITER_MODE": "es", "MF_ES_SW": "4"}, 10)]


@gpu
@pytest.mark.parametrize("build", [None, "host"])
@pytest.mark.parametrize("order", ["permuted", "row-sorted"])
@pytest.mark.parametrize("form,env,K", PERMUTED, ids=lambda v: v if isinstance(v, str) else "")
def test_weights_follow_their_entries_through_the_build(device, switches, form, env, K, order, build):
    """A file that is neither row- nor column-sorted (the device build's staging copy, and bucket() under MF_BUILD=host), and
    the row-sorted file: item sweep and user sweep equal the model.  A weight array that stayed in file order -- read at the
    CSR or CSC position -- gives other bits, asserted on the model."""
    capi = device
    pat = pattern("pair")
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    w = planted_weights(9100 + K, pat)
    row, col = pat.row, pat.col
    if order == "permuted":
        perm = np.random.default_rng(31).permutation(pat.nnz)
        row, col, val, w = (np.ascontiguousarray(a[perm]) for a in (row, col, val, w))
        assert not (np.diff(row) >= 0).all() and not (np.diff(col) >= 0).all()
    m = WModel(pat.users, pat.items, row, col, val, alpha, w)
    one = m.wstep(L0, R0)
    two = m.wstep(*one, L0, R0)
    stayed = m.wstep(L0, R0, w_users=position_mutant(row, w), w_items=position_mutant(col, w))
    assert differs(stayed[1], one[1]) > 0.5 and (order == "row-sorted" or differs(stayed[0], one[0]) > 0.5)
    switches(env)
    if build:
        switches({"MF_BUILD": build})
    plan = capi.Plan(pat.users, pat.items, K, alpha, row, col, val, weight=w)
    try:
        plan.set_regularization(*LAM)
        plan.set_momentum(*BETA)
        desc = plan.describe()
        assert ("MF_BUILD=host" in desc) == (build == "host") and " weighted=1" in desc, desc
        assert ("iterate=errors+resident-streams(" in desc) == (form == "es"), desc
        where = "%s %s MF_BUILD=%s" % (form, order, build)
        if form != "es":
            L, R = _step(plan, L0, R0, None, True, True)
            assert_same_bits(R, one[1], where + ": item sweep")
            assert_same_bits(L, one[0], where + ": user sweep")
        plan.upload(L0, R0)
        plan.iterate(2)
        L, R = plan.download()
        assert_same_bits(L, two[0], where + ": L after two iterations")
        assert_same_bits(R, two[1], where + ": R after two iterations")
        total, rows = plan.weight_total(rows=True)
        want_rows = entry_order_sums(w, row.astype(np.int64), pat.users)
        assert_same_bits(rows, want_rows, where + ": row sums of the weights")
        assert_same_bits(np.array([total]), np.array([model_total(want_rows)]), where + ": total of the weights")
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("cls", ["zeros", "nonfinite"])
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("long", 30), ("es-sw4", 10)], ids=lambda v: str(v))
def test_special_values_meet_special_weights(device, switches, name, K, cls):
    """"zeros" and "nonfinite" with the planted weights.  nonfinite: the entry whose e_n is +inf carries weight 0 -- NaN by the
    rule, inf * 0.  zeros: every entry of a user whose row is all -0.0 carries weight 0 -- the products are zeros, and the
    -0.0 accumulator comes out +0.0 wherever one of them is +0.0.  Both asserted on the model first."""
    capi = device
    case = _pick(name, K)
    u = momentum_expected(case["pat"], cls, K)
    pat = u.pat
    w = planted_weights(9200 + K, pat)
    where = "%s K=%d %s" % (name, K, cls)
    if cls == "nonfinite":
        n = int(np.flatnonzero(pat.row == pat.planted_users[6])[0])
        assert np.isinf(u.val[n])
        w[n] = 0.0
    else:
        r = next(int(i) for i in range(pat.users) if pat.ulen[i] > 0 and is_negzero(u.L0[i]).all() and i not in pat.planted_users)
        w[pat.row == r] = 0.0
    m = WModel(pat.users, pat.items, pat.row, pat.col, u.val, u.alpha, w)
    one = m.wstep(u.L0, u.R0, u.Lp, u.Rp, beta=(0.0, 0.0))
    unseeded = m.wstep(u.L0, u.R0, u.Lp, u.Rp, beta=(0.0, 0.0), seed_u=False, seed_i=False)
    two = m.wstep(*one, beta=(0.0, 0.0))
    if cls == "nonfinite":
        assert np.isnan(one[0][pat.row[n]]).all() and np.isnan(one[1][pat.col[n]]).all(), where   # inf * 0
    else:
        assert (one[0][r] == 0.0).all() and (~is_negzero(one[0][r])).any(), where          # (-0.0) + (+0.0)
        assert is_negzero(u.L0[r] * decay(u.alpha, LAM_U)).all()
    switches(case["env"])
    plan = _plan(capi, pat, K, u.val, u.alpha, w, beta=(0.0, 0.0))
    try:
        assert case["check"](plan.describe(), K), plan.describe()
        if case["steps"]:
            for seed, want in ((True, one), (False, unseeded)):
                L, R = _step(plan, u.L0, u.R0, None, seed, seed)
                assert_same_bits(R, want[1], "%s: item sweep, seed=%s" % (where, seed))
                assert_same_bits(L, want[0], "%s: user sweep, seed=%s" % (where, seed))
        plan.upload(u.L0, u.R0)
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


@gpu
@pytest.mark.parametrize("K", [3, 10, 30, 40])
def test_toy_loop_inside_one_launch(device, switches, K):
    """iterate(9) of a toy instance runs inside one launch (sweep_resident_kernel<4 | 16 | 32 | 0, momentum or not, weighted>):
    the model's bits and the bits of the two-launch path (MF_RESIDENT=0), with and without momentum; then nine more, which
    read their history from the other buffer."""
    capi = device
    pat, L0, R0, val, alpha = _toy(K)
    w = plain_weights(60 + K, pat.nnz)
    w[:2] = [0.0, 1.0]
    m = WModel(pat.users, pat.items, pat.row, pat.col, val, alpha, w)
    for beta in (BETA, (0.0, 0.0)):
        w9, w18 = m.wrun(L0, R0, 9, beta=beta), m.wrun(L0, R0, 18, beta=beta)
        assert differs(w9[0], MModel(pat.users, pat.items, pat.row, pat.col, val, alpha).run(L0, R0, 9, beta=beta)[0]) > 0.5
        for mode in (None, "0"):
            env = {} if mode is None else {"MF_RESIDENT": mode}
            switches(env)
            plan = _plan(capi, pat, K, val, alpha, w, beta=beta)
            try:
                where = "K=%d MF_RESIDENT=%s beta=%s" % (K, mode, beta)
                loop = path_of_plan(plan.describe(), pat, K, 9, env, weighted=True)[0]
                assert loop == ("toy" if mode is None else "sweeps"), (where, loop)
                plan.upload(L0, R0)
                plan.iterate(9)
                L, R = plan.download()
                assert_same_bits(L, w9[0], where + " 9: L")
                assert_same_bits(R, w9[1], where + " 9: R")
                plan.iterate(9)
                L, R = plan.download()
                assert_same_bits(L, w18[0], where + " 9 + 9: L")
                assert_same_bits(R, w18[1], where + " 9 + 9: R")
            finally:
                plan.close()


@gpu
def test_toy_loop_at_the_edge_of_its_lds_rule(device, switches):
    """The toy rule looks at the unweighted footprint (<= 60 KiB) and the weighted launch asks for 16 bytes more per entry.
    600 users + 424 items at K = 3 with 170 entries: 1024 threads, 57 400 bytes unweighted, 60 120 with the weights -- the
    largest toy instance there is at this K (the rule bounds entries x K: test_iterate_path.py).  The request cannot pass
    64 KiB: 60 KiB + 16 x 512 / K bytes needs (users + items) x K above 3500, so K >= 4 and at most 2 KiB of weights."""
    capi = device
    K, U, I, nnz = 3, 600, 424, 170
    rng = np.random.default_rng(321)
    cells = np.sort(rng.choice(U * I, nnz, replace=False))
    from test_sweep_edges import Pattern
    pat = Pattern("toy-edge", U, I, (cells // I).astype(np.int32), (cells % I).astype(np.int32))
    L0, R0, val, alpha = cls_signed(322, pat, K)
    plain_need, weighted_need = toy_lds_bytes(U, I, K, nnz), toy_lds_bytes(U, I, K, nnz, True)
    assert U + I == 1024 and plain_need == 57400 <= 60 * 1024 and weighted_need == 60120 == plain_need + 16 * nnz
    # the largest: one entry more and the rule, asked with every other term as it is, turns the instance away
    assert iterate_path_of(U, I, K, nnz, 9, weighted=True)[0] == "toy" and iterate_path_of(U, I, K, nnz + 1, 9, weighted=True)[0] == "sweeps"
    w = plain_weights(323, nnz)
    m = WModel(U, I, pat.row, pat.col, val, alpha, w)
    want = m.wrun(L0, R0, 9)
    for mode in (None, "0"):
        env = {} if mode is None else {"MF_RESIDENT": mode}
        switches(env)
        plan = _plan(capi, pat, K, val, alpha, w)
        try:
            loop = path_of_plan(plan.describe(), pat, K, 9, env, weighted=True)[0]
            assert loop == ("toy" if mode is None else "sweeps"), (mode, loop)
            plan.upload(L0, R0)
            plan.iterate(9)
            L, R = plan.download()
            assert_same_bits(L, want[0], "MF_RESIDENT=%s L" % mode)
            assert_same_bits(R, want[1], "MF_RESIDENT=%s R" % mode)
        finally:
            plan.close()


@gpu
@pytest.mark.parametrize("name,K", [("dma-ct", 100), ("es-sw4", 10)], ids=lambda v: str(v))
def test_zero_weight_is_leaving_the_entry_out(device, switches, name, K):
    """On "signed" inputs no accumulator is +-0.0, so a zero product changes nothing: weight 0 on a random tenth of the
    entries and 1 on the rest gives, after five iterations, the factors of an unweighted plan built from the other nine
    tenths in the same order -- bit for bit.  The two models agree (asserted first), so the precondition holds for this seed."""
    capi = device
    case = _pick(name, K)
    pat = pattern(case["pat"])
    L0, R0, val, alpha = cls_signed(4000 + K, pat, K)
    out = np.random.default_rng(77 + K).random(pat.nnz) < 0.1
    w = np.where(out, 0.0, 1.0)
    keep = ~out
    row, col, kval = (np.ascontiguousarray(a[keep]) for a in (pat.row, pat.col, val))
    full = WModel(pat.users, pat.items, pat.row, pat.col, val, alpha, w).wrun(L0, R0, 5)
    part = MModel(pat.users, pat.items, row, col, kval, alpha).run(L0, R0, 5)
    assert_same_bits(full[0], part[0], "the two models, L")
    assert_same_bits(full[1], part[1], "the two models, R")
    assert differs(full[0], MModel(pat.users, pat.items, pat.row, pat.col, val, alpha).run(L0, R0, 5)[0]) > 0.5
    switches(case["env"])
    got = []
    for plan in (_plan(capi, pat, K, val, alpha, w), capi.Plan(pat.users, pat.items, K, alpha, row, col, kval)):
        try:
            plan.set_regularization(*LAM)
            plan.set_momentum(*BETA)
            plan.upload(L0, R0)
            plan.iterate(5)
            got.append(plan.download())
        finally:
            plan.close()
    assert_same_bits(got[0][0], got[1][0], "weighted against the smaller plan, L")
    assert_same_bits(got[0][1], got[1][1], "weighted against the smaller plan, R")
    assert_same_bits(got[0][0], full[0], "L against the model")
    assert_same_bits(got[0][1], full[1], "R against the model")


def _check_weighted_loss(plan, L, R, row, col, val, w, where):
    out, rs = plan.loss("train", rows=True)
    ms = wmodel_rows(L, R, row, col, val, w, plan.user_count, plan.user_begin)
    assert out.count == len(row), (where, out.count)
    assert_same_bits(rs, ms, where + ": row_sse")
    assert_same_bits(np.array([out.sse]), np.array([model_total(ms, plan.user_begin)]), where + ": sse")
    return ms


@gpu
@pytest.mark.parametrize("K", LOSS_KS)
def test_weighted_training_loss_equals_the_model(device, switches, K):
    """test_loss's shape -- 1100 users x 260 items, users 0 and 5 empty, user 3 with 260 entries, below the few-rows bound --
    at its K: the LDS-DMA forms for even K, the register-staged one for odd K.  The training loss is the weighted model's,
    the held-out loss on the same plan the unweighted model's, and weights of 1.0 give the unweighted bits."""
    capi = device
    switches({})
    U, I = loss_shape(K)                       # 100 x 100 at K = 4095, where a factor row is 32 KiB
    row, col, val, L, R = loss_instance(K, U, I, K)
    w = plain_weights(K, len(row))
    w[:4] = SPECIAL_WEIGHTS
    plan = capi.Plan(U, I, K, 0.01, row, col, val, weight=w)
    try:
        desc = plan.describe()
        assert ("loss=loss_dma_kernel(" if K % 2 == 0 and K <= 1024 else "loss=loss_reg_kernel(") in desc and " weighted=1" in desc, desc
        plan.upload(L, R)
        ms = _check_weighted_loss(plan, L, R, row, col, val, w, "K=%d" % K)
        plain = wmodel_rows(L, R, row, col, val, None, U)
        assert differs(ms, plain) > 0.5 and ms[0] == 0.0 and ms[5] == 0.0
        plan.set_heldout(row[::3], col[::3], val[::3] + 0.5)
        out, rs = plan.loss("heldout", rows=True)
        hs = wmodel_rows(L, R, row[::3], col[::3], val[::3] + 0.5, None, U)
        assert_same_bits(rs, hs, "K=%d: the held-out loss is unweighted" % K)
        assert_same_bits(np.array([out.sse]), np.array([model_total(hs)]), "K=%d: held-out sse" % K)
    finally:
        plan.close()
    ones = capi.Plan(U, I, K, 0.01, row, col, val, weight=np.ones(len(row)))
    try:
        ones.upload(L, R)
        out, rs = ones.loss("train", rows=True)
        assert_same_bits(rs, plain, "K=%d: weights 1.0 give the unweighted row sums" % K)
        assert_same_bits(np.array([out.sse]), np.array([model_total(plain)]), "K=%d: weights 1.0, sse" % K)
    finally:
        ones.close()


@gpu
@pytest.mark.parametrize("nch", [None, "1", "5", "64"])
def test_weighted_loss_at_the_ordinary_chunk_and_every_chunk_size(device, switches, nch):
    """2500 users (above the few-rows bound: the ordinary chunk) with a full row, and MF_SWEEP_NCH = 1, 5, 64"""
    capi = device
    switches({} if nch is None else {"MF_SWEEP_NCH": nch})
    K, users = 20, 2500
    row, col, val, L, R = loss_instance(users, users, 300, K, density=0.02, full=(7, users - 1))
    w = plain_weights(users, len(row))
    plan = capi.Plan(users, 300, K, 0.01, row, col, val, weight=w)
    try:
        plan.upload(L, R)
        _check_weighted_loss(plan, L, R, row, col, val, w, "users=%d nch=%s" % (users, nch))
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("users", [1, 1023, 1024, 1025, 3000])
def test_weight_total(device, users):
    capi = device
    begin, items, K = 700, 1500, 10
    rng = np.random.default_rng(users)
    n = min(users * items, 4000)
    cells = np.sort(rng.choice(users * items, n, replace=False))
    row, col = (cells // items + begin).astype(np.int32), (cells % items).astype(np.int32)
    val = rng.integers(-10, 11, n) / 2.0
    w = rng.uniform(0.25, 4.0, n) * 10.0 ** rng.integers(-6, 7, n)
    plan = capi.Plan(begin + users + 5, items, K, 1e-3, row, col, val, user_begin=begin, user_count=users, weight=w)
    try:
        total, rows = plan.weight_total(rows=True)
        want = entry_order_sums(w, row.astype(np.int64) - begin, users)
        assert_same_bits(rows, want, "row sums")
        assert_same_bits(np.array([total]), np.array([model_total(want, begin)]), "total")
        assert_same_bits(np.array([total]), np.array([capi.loss_total(rows, begin)]), "host twin")
        assert plan.weight_total() == total
    finally:
        plan.close()
    plain = capi.Plan(begin + users + 5, items, K, 1e-3, row, col, val, user_begin=begin, user_count=users)
    try:
        with pytest.raises(capi.HipBackendError) as err:
            plain.weight_total()
        assert err.value.status == capi.MF_ERR_STATE
    finally:
        plain.close()


@gpu
def test_monitored_loop_watches_the_weighted_loss(device, switches):
    """iterate_monitored(30, 7) on a weighted plan: every point is the model's weighted SSE of the model's factors at that
    iteration, and the factors are those of iterate(iters_done)."""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({})
    w = plain_weights(5, pat.nnz)
    m = WModel(pat.users, pat.items, pat.row, pat.col, val, alpha, w)
    plan, other = _plan(capi, pat, 10, val, alpha, w), _plan(capi, pat, 10, val, alpha, w)
    try:
        plan.upload(L0, R0)
        other.upload(L0, R0)
        done, pts = plan.iterate_monitored(30, every=7)
        assert done == 30 and [p.iter for p in pts] == [0, 7, 14, 21, 28, 30]
        state, at = (L0, R0, None, None), 0
        for p in pts:
            state = m.wrun(state[0], state[1], p.iter - at, prev=(state[2], state[3]))
            at = p.iter
            rows = wmodel_rows(state[0], state[1], pat.row, pat.col, val, w, pat.users)
            assert p.train.count == pat.nnz and p.heldout.count == 0
            assert_same_bits(np.array([p.train.sse]), np.array([model_total(rows)]), "point %d" % p.iter)
            assert differs(rows, wmodel_rows(state[0], state[1], pat.row, pat.col, val, None, pat.users)) > 0.5
        other.iterate(done)
        Lm, Rm = plan.download()
        Lo, Ro = other.download()
        assert_same_bits(Lm, Lo, "L of the monitored loop")
        assert_same_bits(Rm, Ro, "R of the monitored loop")
        assert_same_bits(Lm, state[0], "L against the model")
        assert_same_bits(Rm, state[1], "R against the model")
    finally:
        plan.close()
        other.close()


@gpu
@pytest.mark.parametrize("graph", [None, "0"])
def test_graph_replay(device, switches, graph):
    """iterate(130) = four replays of a captured 32-iteration graph plus two eager iterations: the weight pointers are constant
    for the plan's life"""
    capi = device
    pat, L0, R0, val, alpha = _small()
    switches({"MF_ITER_MODE": "sweeps"})
    if graph:
        switches({"MF_GRAPH": graph})
    w = plain_weights(6, pat.nnz)
    want = WModel(pat.users, pat.items, pat.row, pat.col, val, alpha, w).wrun(L0, R0, 130)
    assert differs(want[0], MModel(pat.users, pat.items, pat.row, pat.col, val, alpha).run(L0, R0, 130)[0]) > 0.5
    plan = _plan(capi, pat, 10, val, alpha, w)
    try:
        assert ("MF_GRAPH=0" in plan.describe()) == (graph == "0"), plan.describe()
        plan.upload(L0, R0)
        plan.iterate(130)
        L, R = plan.download()
        assert_same_bits(L, want[0], "L after 130")
        assert_same_bits(R, want[1], "R after 130")
        Lq, Rq = plan.download_previous()
        assert_same_bits(Lq, want[2], "previous L after 130")
        assert_same_bits(Rq, want[3], "previous R after 130")
    finally:
        plan.close()


@gpu
def test_two_user_shards_on_one_gpu(device, switches):
    """Each shard is created with its slice of the weights; the item sweep is seeded on shard 0 only.  As in the shard tests of
    the decay and of momentum, the caller's sum adds the entries in the sharded run's order, so what is compared is: each
    shard's items_next and user block with the model of that shard, the user blocks with the single weighted plan, and the sum
    with the single plan on the items rated in the root shard alone (+ 0.0 turns the single plan's -0.0 into the sum's +0.0)."""
    capi = device
    K, cut = 30, 333
    x = expected("pair", "signed", K)
    pat = x.pat
    assert cut % 1024 and 0 < cut < pat.users
    switches({"MF_ITER_MODE": "sweeps"})
    single = _plan(capi, pat, K, x.val, x.alpha, x.w)
    Ls, Rs = _step(single, x.L0, x.R0, (x.Lp, x.Rp), True, True)
    single.close()
    assert_same_bits(Ls, x.seeded[0], "single plan, L")
    assert_same_bits(Rs, x.seeded[1], "single plan, R")
    lo = pat.row < cut
    parts = []
    for sel, begin, count, seeded in ((lo, 0, cut, True), (~lo, cut, pat.users - cut, False)):
        row, col, val, w = pat.row[sel], pat.col[sel], x.val[sel], x.w[sel]
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, row, col, val, user_begin=begin, user_count=count, weight=w)
        try:
            plan.set_regularization(LAM_U, LAM_I)
            plan.set_momentum(BETA_U, BETA_I)
            Lb, Rn = _step(plan, x.L0[begin:begin + count], x.R0, (x.Lp[begin:begin + count], x.Rp), seeded, True)
        finally:
            plan.close()
        m = WModel(count, pat.items, row - begin, col, val, x.alpha, w)
        Lm, Rm = m.wstep(x.L0[begin:begin + count], x.R0, x.Lp[begin:begin + count], x.Rp, seed_i=seeded)
        assert_same_bits(Rn, Rm, "shard at %d: items_next" % begin)
        assert_same_bits(Lb, Lm, "shard at %d: user block against the model" % begin)
        assert_same_bits(Lb, Ls[begin:begin + count], "shard at %d: user block against the single plan" % begin)
        parts.append(Rn)
    alone = np.bincount(pat.col[~lo], minlength=pat.items) == 0
    assert alone.any()
    with np.errstate(all="ignore"):
        assert_same_bits((parts[0] + parts[1])[alone], Rs[alone] + 0.0, "items rated in the root shard only")


@gpu
@pytest.mark.parametrize("name,K", [("reg", 3), ("dma-ct", 100), ("pair", 100), ("long", 30), ("coop", 10)], ids=lambda v: str(v))
def test_frozen_columns_keep_their_bits_under_weights(device, switches, name, K):
    capi = device
    case = _pick(name, K)
    x = expected(case["pat"], "signed", K)
    fu, fi = K - 1, K - 2
    switches(case["env"])
    plan = _plan(capi, x.pat, K, x.val, x.alpha, x.w)
    try:
        plan.set_frozen_columns(fu, fi)
        assert case["check"](plan.describe(), K), plan.describe()
        one = x.model.wstep(x.L0, x.R0, x.Lp, x.Rp, frozen=(fu, fi))
        two = x.model.wstep(*one, x.L0, x.R0, frozen=(fu, fi))
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
        assert_same_bits(L, two[0], where + ": L after two iterations")
        assert_same_bits(R, two[1], where + ": R after two iterations")
    finally:
        plan.close()


@gpu
def test_backend_run_weighted(device):
    capi = device
    pat, L0, R0, val, alpha = _small()
    w = plain_weights(8, pat.nnz)
    inst = capi.Instance(40, alpha, 10, pat.users, pat.items, pat.row, pat.col, val)
    plan = _plan(capi, pat, 10, val, alpha, w)
    try:
        plan.upload(L0, R0)
        plan.iterate(40)
        Lp, Rp = plan.download()
        bp = plan.recommend()
    finally:
        plan.close()
    L, R = L0.copy(), R0.copy()
    best = capi.run_weighted(inst, w, L, R, LAM_U, LAM_I, BETA_U, BETA_I)
    assert_same_bits(L, Lp, "L")
    assert_same_bits(R, Rp, "R")
    assert np.array_equal(best, bp)
    want = WModel(pat.users, pat.items, pat.row, pat.col, val, alpha, w).wrun(L0, R0, 40)
    assert_same_bits(L, want[0], "L against the model")
    assert_same_bits(R, want[1], "R against the model")
    L2, R2 = L0.copy(), R0.copy()
    assert capi.run_weighted(inst, w, L2, R2, LAM_U, LAM_I, BETA_U, BETA_I, recommend=False) is None
    assert_same_bits(L2, Lp, "L without a recommendation")
    La, Ra, Lb, Rb = L0.copy(), R0.copy(), L0.copy(), R0.copy()
    b0 = capi.run_weighted(inst, None, La, Ra, LAM_U, LAM_I, BETA_U, BETA_I)
    b1 = capi.backend_run_momentum(inst, Lb, Rb, LAM_U, LAM_I, BETA_U, BETA_I)
    assert_same_bits(La, Lb, "weight NULL: L of mf_backend_run_momentum")
    assert_same_bits(Ra, Rb, "weight NULL: R of mf_backend_run_momentum")
    assert np.array_equal(b0, b1)


@gpu
@pytest.mark.parametrize("name", ["inst30-40-10-2-10", "inst0"])
def test_cli_weights(device, orc, name, tmp_path):
    """MATFACT_WEIGHTS alone, with MATFACT_LAMBDA + MATFACT_MOMENTUM, and with MATFACT_LOSS: stdout is the .out of the weighted
    plan's own recommendation, and with MATFACT_LOSS every stderr RMSE parses back (%.17g) to the bits of the plan's monitored
    loop -- the weighted one.  A weights file of all 1 reproduces the bundled .out byte for byte."""
    capi = device
    path = golden_in(name)
    inst = capi.parse_file(path)
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    ones = _weights_file(tmp_path / "ones.in", inst, np.ones(inst.nnz))
    r = _cli(capi, path, MATFACT_WEIGHTS=ones)
    assert r.returncode == 0 and r.stdout == open(os.path.join(GOLDEN, name + ".out"), "rb").read() and r.stderr == b"", r
    w = plain_weights(12, inst.nnz)
    w[0] = 0.0
    wf = _weights_file(tmp_path / "w.in", inst, w)
    assert_same_bits(capi.parse_file(wf).val, w, "the weights survive the file")

    def session(lam, beta, every=None):
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val, weight=w)
        try:
            plan.set_regularization(*lam)
            plan.set_momentum(*beta)
            plan.upload(L0, R0)
            pts = None
            if every:
                done, pts = plan.iterate_monitored(inst.iters, every=every)
                assert done == inst.iters
            else:
                plan.iterate(inst.iters)
            return orc.format_out(plan.recommend()).encode(), pts
        finally:
            plan.close()
    unweighted = _cli(capi, path)
    want, _ = session((0.0, 0.0), (0.0, 0.0))
    r = _cli(capi, path, MATFACT_WEIGHTS=wf)
    assert r.returncode == 0 and r.stdout == want and r.stderr == b"", r
    want2, _ = session(LAM, BETA)
    r = _cli(capi, path, MATFACT_WEIGHTS=wf, MATFACT_LAMBDA="0.05,0.3", MATFACT_MOMENTUM="0.9,0.3")
    assert r.returncode == 0 and r.stdout == want2 and r.stderr == b"", r
    every = max(inst.iters // 4, 1)
    want3, pts = session((0.0, 0.0), (0.0, 0.0), every)
    assert want3 == want
    r = _cli(capi, path, MATFACT_WEIGHTS=wf, MATFACT_LOSS=str(every))
    assert r.returncode == 0 and r.stdout == want, r
    its = [ln.split() for ln in r.stderr.decode().splitlines() if ln.startswith("iter ")]
    assert [int(t[1]) for t in its] == [p.iter for p in pts]
    got = np.array([float(t[3]) for t in its])
    assert_same_bits(got, np.array([np.sqrt(p.train.sse / float(p.train.count)) for p in pts]), "train_rmse on stderr")
    plain = _cli(capi, path, MATFACT_LOSS=str(every))
    plain_rmse = np.array([float(ln.split()[3]) for ln in plain.stderr.decode().splitlines() if ln.startswith("iter ")])
    assert differs(got, plain_rmse) > 0.5 and unweighted.returncode == 0   # the line carries the weighted loss
