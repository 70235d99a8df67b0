"""ALS on user shards: the solve cut at the normal equations (mf_backend_als_normal_pitch, mf_plan_als_normal,
mf_plan_als_solve_normal; include/matfact_hip.h, "ALS on user shards").

The model is composed from the models of the single-plan solves: per shard steps 1-4 of every row from 0.0 (gram_rhs of
tests/test_als.py; under the implicit kind with e_n as the weight for the triangle and a_n c_n as the value for b), the
records summed elementwise in shard order, then steps 5-10 (cholesky_solve of tests/test_als.py) on the sums -- under the
implicit kind on S + N with the summed Grams of the shards' blocks of the other side (gram of tests/test_implicit.py).  Every
comparison is bit for bit (assert_same_bits), the three row counters included.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_als import (FORMS, KINDS, LAM, NO_BOX, AlsModel, _not_pd_inputs, als_plan, cholesky_solve, forms_of, gram_rhs, hand_iteration,
                      sides, triangle)
from test_als import als_solve as single_als_solve
from test_als_edges import long_rows
from test_implicit import ImplicitModel, gram, implicit_plan, implicit_solve
from test_regularised import LAM_I, LAM_U, _small, differs
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits, cls_signed, pattern
from test_weighted import plain_weights

gpu = pytest.mark.gpu

CSRC = os.path.join(ROOT, "recommender-system_amd", "csrc")
NORMAL_SYMBOLS = ("mf_backend_als_normal_pitch", "mf_plan_als_normal", "mf_plan_als_solve_normal")
# the K every form is launched at: both ends of the range of K of every instance of kAlsNormalForm (test I below)
FORM_K = {"wave": (1, 2, 20, 21, 30, 31, 32), "wg": (1, 17, 88, 89, 100, 124, 125, 128)}
CONF = 40.0
ALL_KINDS = KINDS + ("implicit",)


def pitch_of(K):
    return (K * (K + 1) // 2 + K + 1 + 1) // 2 * 2


# ------------------------------------------------------------------------------------------------ the model
def normal_records(rows, val, wgt, X_old, Y, frozen=-1, conf=None):
    """mf_plan_als_normal of one side of one plan: (nrows, T + K + 1) -- triangle, b, count -- over the plan's own entries.
    conf None: the explicit kinds; otherwise the implicit kind's steps 1-4, the triangle from 0.0 all the same."""
    K = Y.shape[1]
    T = K * (K + 1) // 2
    N = np.zeros((rows.nrows, T + K + 1))
    with np.errstate(all="ignore"):
        if conf is not None:
            en = conf * wgt if wgt is not None else np.full(len(val), float(conf))
            cn = 1.0 + en
            ac = val * cn
        for r in np.flatnonzero(rows.cnt > 0):
            if conf is None:
                G, b = gram_rhs(rows, r, val, wgt, Y, X_old[r, frozen] if frozen >= 0 else 0.0, frozen)
            else:
                G = gram_rhs(rows, r, val, en, Y, 0.0, -1)[0]     # y_n[p] * (y_n[q] * e_n)
                b = gram_rhs(rows, r, ac, None, Y, 0.0, -1)[1]    # ac_n * y_n[p]
            N[r, :T], N[r, T:T + K] = G, b
        N[:, T + K] = rows.cnt.astype(np.float64)
    return N


def solve_records(N, S, X_old, lam, kind, frozen=-1, box=NO_BOX):
    """mf_plan_als_solve_normal: steps 5-10 on the (summed) records -> (X_new, (solved, kept_empty, kept_not_pd)).  S: the
    (summed) Gram record's triangle, added on the left under the implicit kind."""
    K = X_old.shape[1]
    T = K * (K + 1) // 2
    tp, tq = triangle(K)
    cntd = N[:, T + K]
    X_new = X_old.copy()
    lo, hi, ncols = box
    with np.errstate(all="ignore"):
        todo = np.arange(len(N)) if kind == "implicit" else np.flatnonzero(cntd > 0.0)
        tri = S[None, :] + N[todo, :T] if kind == "implicit" else N[todo, :T]
        G, b = np.zeros((len(todo), K, K)), N[todo, T:T + K].copy()
        G[:, tp, tq] = tri
        ridge = lam * cntd[todo] if kind == "ridge-count" else np.full(len(todo), float(lam))
        d = np.arange(K)
        G[:, d, d] = G[:, d, d] + ridge[:, None]
        if frozen >= 0:
            G[:, frozen, :frozen] = 0.0
            G[:, frozen + 1:, frozen] = 0.0
            G[:, frozen, frozen] = 1.0
            b[:, frozen] = X_old[todo, frozen]
        x, ok = cholesky_solve(G, b) if len(todo) else (b, np.ones(0, bool))
        head = x[:, :ncols]
        head = np.where(head < lo, lo, head)
        head = np.where(head > hi, hi, head)
        x = np.concatenate([head, x[:, ncols:]], axis=1)
        if frozen >= 0:
            x[:, frozen] = X_old[todo, frozen]
        X_new[todo[ok]] = x[ok]
    not_pd = int((~ok).sum())
    return X_new, (len(todo) - not_pd, len(N) - len(todo), not_pd)


class Shard:
    """the entries of the users begin .. begin + count, rows local to the block"""

    def __init__(self, pat, val, wgt, begin, count):
        self.begin, self.count = int(begin), int(count)
        self.sel = (pat.row >= begin) & (pat.row < begin + count)
        self.row, self.col, self.val = pat.row[self.sel], pat.col[self.sel], np.asarray(val)[self.sel]
        self.wgt = None if wgt is None else np.asarray(wgt)[self.sel]
        self.side = sides(self.count, pat.items, self.row - self.begin, self.col)


def shards_of(pat, val, wgt, cuts):
    return [Shard(pat, val, wgt, b, e - b) for b, e in zip(cuts[:-1], cuts[1:])]


def summed_item_records(shards, blocks, R_old, frozen=-1, conf=None):
    """the shards' item records against their blocks of L, and the Grams of those blocks, each summed in shard order"""
    with np.errstate(all="ignore"):
        N = S = None
        for sh, Lb in zip(shards, blocks):
            n = normal_records(sh.side[0], sh.val, sh.wgt, R_old, Lb, frozen, conf)
            s = gram(Lb)
            N, S = (n, s) if N is None else (N + n, S + s)
    return N, S


def sharded_iteration(shards, L0, R0, lam, kind, conf=None):
    """the procedure of AlsShardedFactorization: every shard's user solve, the summed records, the solve of the sums"""
    blocks, cu = [], []
    for sh in shards:
        Lb = L0[sh.begin:sh.begin + sh.count]
        if kind == "implicit":
            got = implicit_solve(sh.side[1], sh.val, sh.wgt, Lb, R0, lam[0], conf)
        else:
            got = single_als_solve(sh.side[1], sh.val, sh.wgt, Lb, R0, lam[0], kind)
        blocks.append(got[0])
        cu.append(got[1])
    N, S = summed_item_records(shards, blocks, R0, -1, conf if kind == "implicit" else None)
    R1, ci = solve_records(N, S, R0, lam[1], kind)
    return blocks, R1, cu, ci


# ------------------------------------------------------------------------------------------------ CPU
def test_normal_entries_are_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    for s in NORMAL_SYMBOLS:
        assert re.search(r"\bint(64_t)? %s\(" % s, hdr) and s in capi.HIP_SYMBOLS, s
        assert hasattr(capi.hip(), s), s
    assert re.search(r"#define MATFACT_HIP_ABI_VERSION 5\b", hdr) and capi.hip().mf_backend_abi_version() == 5
    assert callable(capi.als_normal_pitch) and callable(capi.Plan.als_normal) and callable(capi.Plan.als_solve_normal)
    contract = hdr[hdr.index("The plan's stream"):hdr.index("int mf_plan_set_stream")]
    assert "mf_plan_als_normal," in contract.split("Host only")[0] and "mf_plan_als_solve_normal" in contract.split("Host only")[0]
    from recommender_system_amd import sharded
    assert callable(sharded.AlsShardedFactorization)


def test_normal_pitch(capi):
    assert [capi.als_normal_pitch(K) for K in (1, 2, 3, 128)] == [4, 6, 10, 8386]
    for K in range(1, 140):
        p = capi.als_normal_pitch(K)
        assert p == pitch_of(K) and p % 2 == 0 and 0 <= p - (K * (K + 1) // 2 + K + 1) <= 1
    assert capi.als_normal_pitch(0) == 0 and capi.als_normal_pitch(-3) == 0


def test_normal_argument_errors_come_before_any_hip_call(capi):
    h = capi.hip()
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused on its other arguments
    buf = C.c_void_p(4096)
    assert h.mf_plan_als_normal(None, 0, 0, buf, 8) == capi.MF_ERR_ARGUMENT
    assert h.mf_plan_als_solve_normal(None, 0, buf, 8) == capi.MF_ERR_ARGUMENT
    for side in (-1, 2):
        assert h.mf_plan_als_normal(fake, side, 0, buf, 8) == capi.MF_ERR_ARGUMENT
        assert h.mf_plan_als_solve_normal(fake, side, buf, 8) == capi.MF_ERR_ARGUMENT
    for gen in (-1, 2):
        assert h.mf_plan_als_normal(fake, 0, gen, buf, 8) == capi.MF_ERR_ARGUMENT


def _model_inputs(K=6, weighted=False):
    pat, L0, R0, val, _ = _small(users=21, items=37, nnz=200, K=K, seed=19)
    return pat, L0, R0, val, (plain_weights(5, pat.nnz) if weighted else None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_one_shard_is_the_single_plan_model(kind, weighted):
    pat, L0, R0, val, w = _model_inputs(weighted=weighted)
    (one,) = shards_of(pat, val, w, (0, pat.users))
    m = AlsModel(pat.users, pat.items, pat.row, pat.col, val, w)
    for frozen, box in ((-1, NO_BOX), (2, (-0.5, 0.25, 4))):
        for side, X, Y, lam in ((1, L0, R0, LAM_U), (0, R0, L0, LAM_I)):
            N = normal_records(one.side[side], one.val, one.wgt, X, Y, frozen)
            got, counts = solve_records(N, None, X, lam, kind, frozen, box)
            want, wcounts = m.solve(side, X, Y, lam, kind, frozen, box)
            assert_same_bits(got, want, "%s side %d frozen %d" % (kind, side, frozen))
            assert counts == wcounts and counts[0] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_two_shards_differ_from_the_single_plan_only_where_both_rated(kind):
    pat, L0, R0, val, w = _model_inputs()
    shards = shards_of(pat, val, w, (0, 10, pat.users))
    N, _ = summed_item_records(shards, [L0[:10], L0[10:]], R0)
    got, counts = solve_records(N, None, R0, LAM_I, kind)
    want, wcounts = AlsModel(pat.users, pat.items, pat.row, pat.col, val).solve(0, R0, L0, LAM_I, kind)
    assert counts == wcounts
    in0, in1 = shards[0].side[0].cnt > 0, shards[1].side[0].cnt > 0
    both, one = in0 & in1, in0 ^ in1
    assert both.sum() >= 10 and one.sum() >= 3
    assert_same_bits(got[~both], want[~both], "items that one shard alone rated, or none")
    assert (got[both].view(np.uint64) != want[both].view(np.uint64)).any(axis=1).sum() >= 1   # the sum is re-associated


@pytest.mark.parametrize("weighted", [False, True])
def test_one_implicit_shard_is_not_the_single_plan_model(weighted):
    """S + (0.0 + t1 + ...) is not ((S + t1) + ...): the guard against a model -- or a kernel -- that starts the chain at S"""
    pat, L0, R0, val, w = _model_inputs(weighted=weighted)
    (one,) = shards_of(pat, val, w, (0, pat.users))
    N, S = summed_item_records([one], [L0], R0, -1, CONF)
    got, counts = solve_records(N, S, R0, LAM_I, "implicit")
    want, wcounts = ImplicitModel(pat.users, pat.items, pat.row, pat.col, val, w).solve(0, R0, L0, LAM_I, CONF)
    assert counts == wcounts == (pat.items, 0, 0)
    rows = (got.view(np.uint64) != want.view(np.uint64)).any(axis=1)
    assert rows.sum() >= 1 and np.allclose(got, want, rtol=1e-9, atol=1e-12)
    cold = one.side[0].cnt == 0    # S + 0.0 is S: a row without entries has the single plan's bits
    if cold.any():
        assert_same_bits(got[cold], want[cold], "cold rows")


def normal_tables():
    """kAlsNormalForm of mf_plan.hip.h read as text: per form its threads, block side, widest K and the NB of its instances"""
    plan, als = open(os.path.join(CSRC, "mf_plan.hip.h")).read(), open(os.path.join(CSRC, "mf_als.hip.h")).read()

    def const(text, name):
        (v,) = re.findall(r"constexpr int %s = (\d+);" % name, text)
        return int(v)
    names = {"mf::kAlsThreads": const(als, "kAlsThreads"), "mf::kWave": const(open(os.path.join(CSRC, "mf_common.hip.h")).read(), "kWave"),
             "mf::kAlsMaxK": const(als, "kAlsMaxK"), "mf::kAlsWaveMaxK": const(als, "kAlsWaveMaxK")}
    (body,) = re.findall(r"const AlsNormalForm kAlsNormalForm\[kAlsForms\] = \{(.*?)\n\};", plan, re.S)
    out = {}
    for chunk in body.split('{"')[1:]:
        name, threads, bs, max_k = re.match(r'(\w+)", ([\w:]+), (\d+), [\w:]+, ([\w:]+),', chunk).groups()
        form = dict(threads=names[threads], bs=int(bs), max_k=names[max_k])
        for kind, tail in (("explicit", ">"), ("implicit", ", mf::AlsImplicit>")):
            inst = re.findall(r"mf::als_normal_kernel<([\w:]+), (\d+), (\d+)%s" % re.escape(tail), chunk)
            assert inst and all(t == threads and b == bs for t, b, _ in inst), (name, kind, inst)
            form[kind] = [int(nb) for _, _, nb in inst]
        assert re.findall(r"mf::als_solve_normal_kernel<([\w:]+)>", chunk) == [threads], name
        out[name] = form
    return out


def test_every_instance_of_the_normal_table_is_launched_at_both_ends_of_its_range():
    tables = normal_tables()
    assert sorted(tables) == sorted(FORMS) == sorted(FORM_K)
    for name, form in tables.items():
        assert form["max_k"] == FORMS[name]["max_k"] and form["explicit"] == form["implicit"] == [1, 2, 3]

        def nb_of(K):
            kb = (K + form["bs"] - 1) // form["bs"]
            return (kb * (kb + 1) // 2 + form["threads"] - 1) // form["threads"]
        ks = range(1, form["max_k"] + 1)
        assert sorted({nb_of(K) for K in ks}) == [1, 2, 3], name
        for nb in (1, 2, 3):   # the explicit lists of test A and the implicit ones of test A' are the same FORM_K
            span = [K for K in ks if nb_of(K) == nb]
            assert span[0] in FORM_K[name] and span[-1] in FORM_K[name], (name, nb, span[0], span[-1])
        assert 1 in FORM_K[name] and form["max_k"] in FORM_K[name]   # the one solve instance of the form


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


def cuda():
    import torch
    return torch.device("cuda", 0)


def normal_buffer(rows, pitch, fill=np.nan):
    """(rows + 1, pitch) float64 on the device, every double `fill`, complete before the plan's stream is used"""
    import torch
    buf = torch.full((rows + 1, pitch), fill, dtype=torch.float64, device=cuda())
    torch.cuda.synchronize()
    return buf


def rows_of(plan, side):
    return plan.items if side == "items" else plan.user_count


def cut_solve(plan, side, other, pitch=None, buf=None):
    """als_normal then als_solve_normal of one side through a buffer of its own -> the side's counters"""
    pitch = pitch_of(plan.feats) if pitch is None else pitch
    buf = normal_buffer(rows_of(plan, side), pitch) if buf is None else buf
    plan.als_normal(side, other, buf.data_ptr(), pitch)
    plan.als_solve_normal(side, buf.data_ptr(), pitch)
    return plan.als_info(side)


def cut_iteration(plan):
    cu = cut_solve(plan, "users", "current")
    ci = cut_solve(plan, "items", "next")
    plan.flip()
    return cu, ci


def download_records(plan, buf, K):
    import torch
    plan.synchronize()
    torch.cuda.synchronize()
    return buf[:, :pitch_of(K)].cpu().numpy()


# ---- A: the whole plan under the explicit kinds: the cut solve is als_solve
@gpu
@pytest.mark.parametrize("form,K", [(f, K) for f in FORM_K for K in FORM_K[f]])
def test_whole_plan_cut_solve_is_als_solve(device, switches, form, K):
    capi = device
    pat = pattern("pair")
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    switches({"MF_ALS_FORM": form})
    for kind in KINDS:
        ref, cut = als_plan(capi, pat, K, val, kind), als_plan(capi, pat, K, val, kind)
        try:
            where = "pair K=%d %s [%s]" % (K, kind, form)
            assert " als_form=%s(" % form in cut.describe()
            ref.upload(L0, R0)
            cut.upload(L0, R0)
            want = hand_iteration(ref, where)
            assert cut_iteration(cut) == want, where
            assert want[0][0] > 600 and want[1][0] > 90 and want[0][1] == int((pat.ulen == 0).sum())
            (L, R), (L1, R1) = cut.download(), ref.download()
            assert_same_bits(L, L1, where + ": L")
            assert_same_bits(R, R1, where + ": R")
            assert differs(L1, L0) > 0.9 and differs(R1, R0) > 0.9
        finally:
            ref.close()
            cut.close()


@gpu
@pytest.mark.parametrize("pat_name,K", [("small", 10), ("pair", 17)])
def test_cut_solve_with_weights_frozen_box_and_lambda_all_at_once(device, switches, pat_name, K):
    capi = device
    if pat_name == "small":
        pat, L0, R0, val, _ = _small()
    else:
        pat = pattern(pat_name)
        L0, R0, val, _ = cls_signed(4300 + K, pat, K)
    w = plain_weights(77, pat.nnz)
    frozen, box = (K - 1, 0), ((-1.0, 1.0, -1 if K == 10 else K - 1), (-1.5, 0.75, max(K // 2, 1)))
    for kind in KINDS:
        for form in forms_of(K):
            switches({"MF_ALS_FORM": form})
            ref, cut = als_plan(capi, pat, K, val, kind, weight=w), als_plan(capi, pat, K, val, kind, weight=w)
            try:
                where = "%s K=%d %s [%s]" % (pat_name, K, kind, form)
                for p in (ref, cut):
                    p.set_frozen_columns(*frozen)
                    p.set_bounds("users", *box[0])
                    p.set_bounds("items", *box[1])
                    p.upload(L0, R0)
                want = hand_iteration(ref, where)
                assert cut_iteration(cut) == want, where
                (L, R), (L1, R1) = cut.download(), ref.download()
                assert_same_bits(L, L1, where + ": L")
                assert_same_bits(R, R1, where + ": R")
                assert (L1[:, K - 1] == L0[:, K - 1]).all() and (np.abs(L1[:, :K - 1]) == 1.0).any()
            finally:
                ref.close()
                cut.close()


# ---- A': the implicit instances at the same K: the model of the procedure (the single plan's bits are not expected)
@gpu
@pytest.mark.parametrize("form,K", [(f, K) for f in FORM_K for K in FORM_K[f]])
def test_whole_plan_cut_solve_under_the_implicit_kind(device, switches, form, K):
    capi = device
    pat, L0, R0, val, _ = _small(K=K)
    w = plain_weights(31 + K, pat.nnz) if K % 2 else None
    (one,) = shards_of(pat, val, w, (0, pat.users))
    Nu = normal_records(one.side[1], one.val, one.wgt, L0, R0, -1, CONF)
    L1, cu = solve_records(Nu, gram(R0), L0, LAM_U, "implicit")
    Ni = normal_records(one.side[0], one.val, one.wgt, R0, L1, -1, CONF)
    R1, ci = solve_records(Ni, gram(L1), R0, LAM_I, "implicit")
    switches({"MF_ALS_FORM": form})
    plan = implicit_plan(capi, pat, K, val, CONF, weight=w)
    try:
        where = "small K=%d implicit [%s]" % (K, form)
        plan.upload(L0, R0)
        assert cut_iteration(plan) == (cu, ci), where
        assert cu == (pat.users, 0, 0) and ci == (pat.items, 0, 0)
        L, R = plan.download()
        assert_same_bits(L, L1, where + ": L")
        assert_same_bits(R, R1, where + ": R")
    finally:
        plan.close()


# ---- B: the records
def lengths_pattern(lens, items):
    """user u rates the first lens[u] items: row lengths by design"""
    row = np.repeat(np.arange(len(lens)), lens)
    col = np.concatenate([np.arange(n) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    return Pattern("lengths", len(lens), items, row, col)


@gpu
@pytest.mark.parametrize("nrows", [1, 4, 5])
@pytest.mark.parametrize("form,K", [("wave", 21), ("wg", 33)])
def test_records(device, switches, form, K, nrows):
    """rows of 0, 1, chunk - 1, chunk, chunk + 1 and 3 chunk + 1 entries on sides of 1, 4 and 5 rows (the wave form packs four
    rows per workgroup); K = 21 and 33: a record of two passes of the store loop in either form"""
    capi = device
    chunk = FORMS[form]["chunk"]
    lens6 = [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 1]
    items = 3 * chunk + 2                      # one item nobody rates
    T, np_ = K * (K + 1) // 2, pitch_of(K)
    assert np_ > 2 * (256 if form == "wg" else 64)
    switches({"MF_ALS_FORM": form})
    for shift in range(0, 6, 1 if nrows == 1 else 3):
        lens = [lens6[(shift + i) % 6] for i in range(nrows)]
        pat = lengths_pattern(lens, items)
        rng = np.random.default_rng(4500 + K + shift)     # a side of one row of no or one entry: cls_signed wants two entries
        L0, R0, val = rng.uniform(-1, 1, (pat.users, K)), rng.uniform(-1, 1, (pat.items, K)), rng.integers(-10, 11, pat.nnz) / 2.0
        w = plain_weights(9 + shift, pat.nnz)
        for kind, weight, frozen, pitch in (("ridge", None, (-1, -1), np_), ("ridge-count", w, (3, 1), np_ + 6), ("implicit", w, (-1, -1), np_)):
            if kind == "implicit":
                plan = implicit_plan(capi, pat, K, val, CONF, weight=weight)
            else:
                plan = als_plan(capi, pat, K, val, kind, weight=weight)
            try:
                plan.set_frozen_columns(*frozen)
                plan.upload(L0, R0)
                (one,) = shards_of(pat, val, weight, (0, pat.users))
                for side, X, Y, other in (("users", L0, R0, "items"), ("items", R0, L0, "users")):
                    where = "%s %s lens %s %s" % (form, kind, lens, side)
                    s = 0 if side == "items" else 1
                    rows = rows_of(plan, side)
                    buf = normal_buffer(rows, pitch)
                    plan.als_normal(side, "current", buf.data_ptr(), pitch)
                    got = download_records(plan, buf, K)
                    whole = buf.cpu().numpy()
                    want = normal_records(one.side[s], one.val, one.wgt, X, Y, frozen[1 - s], CONF if kind == "implicit" else None)
                    assert not np.isnan(got).any(), where
                    assert_same_bits(got[:rows, :T + K + 1], want, where + ": triangle, b, count")
                    assert (got[:, T + K + 1:].view(np.uint64) == 0).all(), where + ": pads are +0.0"
                    assert np.isnan(whole[:, np_:]).all(), where + ": beyond the minimum pitch nothing is written"
                    empty = one.side[s].cnt == 0
                    assert (got[:rows][empty].view(np.uint64) == 0).all() and (empty.any() or side == "users"), where + ": a row without entries is +0.0"
                    if kind == "implicit":
                        assert_same_bits(got[rows, :T], plan.gram(other, "current"), where + ": the Gram record")
                        assert_same_bits(got[rows, :T], gram(Y), where + ": the Gram record, model")
                        assert (got[rows, T:].view(np.uint64) == 0).all()
                    else:
                        assert (got[rows].view(np.uint64) == 0).all(), where + ": the Gram record is +0.0"
            finally:
                plan.close()


# ---- C: user shards
def holed_pair():
    """the `pair` pattern without the entries of item 7: an item rated nowhere"""
    p = pattern("pair")
    keep = p.col != 7
    return Pattern("pair-hole", p.users, p.items, p.row[keep], p.col[keep])


def run_shards(capi, pat, K, val, w, cuts, kind, L0, R0, lam=LAM, other="next", user_solve=True):
    """the procedure on one GPU: every shard's user solve and records, the sum in shard order by torch, every shard's solve of
    the sum -> per shard (L block, R, users' counters, items' counters)"""
    import torch
    pitch = pitch_of(K)
    plans, bufs, out = [], [], []
    try:
        for b, e in zip(cuts[:-1], cuts[1:]):
            sel = (pat.row >= b) & (pat.row < e)
            kw = dict(weight=None if w is None else w[sel], user_begin=int(b), user_count=int(e - b))
            sub = Pattern("shard", pat.users, pat.items, pat.row[sel], pat.col[sel])
            plan = implicit_plan(capi, sub, K, val[sel], CONF, lam, **kw) if kind == "implicit" else als_plan(capi, sub, K, val[sel], kind, lam, **kw)
            plans.append(plan)
            plan.upload(L0[b:e], R0)
            with pytest.raises(capi.HipBackendError) as err:
                plan.als_solve("items", "next")
            assert err.value.status == capi.MF_ERR_UNSUPPORTED
            if user_solve:
                plan.als_solve("users", "current")
            bufs.append(normal_buffer(pat.items, pitch))
            plan.als_normal("items", other, bufs[-1].data_ptr(), pitch)
        for plan in plans:
            plan.synchronize()
        total = bufs[0]
        for buf in bufs[1:]:
            total = total + buf
        torch.cuda.synchronize()
        for plan in plans:
            cu = plan.als_info("users")
            plan.als_solve_normal("items", total.data_ptr(), pitch)
            ci = plan.als_info("items")
            if user_solve:
                plan.flip()
                out.append(plan.download() + (cu, ci))
            else:   # only the item half ran: its result is in the next generation
                plan.als_solve("users", "current")
                plan.flip()
                out.append((None, plan.download(want_l=False)[1], None, ci))
    finally:
        for plan in plans:
            plan.close()
    return out


@gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("cuts", [(0, 333), (0, 1, 333)], ids=["two", "three-one-without-entries"])
def test_user_shards_on_one_gpu(device, switches, kind, cuts):
    capi = device
    K = 30
    pat = holed_pair()
    cuts = cuts + (pat.users,)
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    w = plain_weights(61, pat.nnz) if kind != "ridge" else None
    shards = shards_of(pat, val, w, cuts)
    if len(cuts) == 4:
        assert shards[0].count == 1 and len(shards[0].val) == 0
    blocks, R1, cu, ci = sharded_iteration(shards, L0, R0, LAM, kind, CONF)
    if kind == "implicit":
        single = ImplicitModel(pat.users, pat.items, pat.row, pat.col, val, w).iteration(L0, R0, LAM, CONF)
    else:
        single = AlsModel(pat.users, pat.items, pat.row, pat.col, val, w).iteration(L0, R0, LAM, kind)
    assert_same_bits(np.concatenate(blocks), single[0], "model: the user blocks are the single plan's")
    rated = [sh.side[0].cnt > 0 for sh in shards]
    nowhere, several = ~np.any(rated, axis=0), np.sum(rated, axis=0) > 1
    late = ~rated[-2] & rated[-1] & ~several      # empty in the shard before the last, rated in the last alone
    assert nowhere[7] and late.sum() >= 5 and several.sum() >= 50
    if kind == "implicit":
        assert ci == (pat.items, 0, 0)
    else:
        assert ci == (pat.items - int(nowhere.sum()), int(nowhere.sum()), 0)
        assert_same_bits(R1[~several], single[1][~several], "model: items one shard alone rated are the single plan's")
        assert differs(R1[several], single[1][several]) > 0.1
    if kind == "ridge-count":   # the summed count is the ridge's factor
        assert differs(R1[several], solve_records(*summed_item_records(shards, blocks, R0), R0, LAM_I, "ridge")[0][several]) > 0.9
    switches({})
    got = run_shards(capi, pat, K, val, w, cuts, kind, L0, R0)
    for g, (L, R, gcu, gci) in enumerate(got):
        where = "%s shard %d of %d" % (kind, g, len(got))
        assert_same_bits(L, blocks[g], where + ": L block")
        assert_same_bits(R, R1, where + ": R, the model of the procedure")
        assert gcu == cu[g] and gci == ci, (where, gcu, cu[g], gci, ci)
        assert differs(R[late], R0[late]) > 0.9, where + ": an item empty in one shard and rated in the next is solved"
        if kind != "implicit":
            assert_same_bits(R[7], R0[7], where + ": an item rated nowhere keeps its bits")


# ---- D: edge values
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_rows_not_positive_definite_after_the_sum(device, switches, kind):
    """the `wide` pattern with zero rows, NaN and infinities (tests/test_als.py) at lambda 0 on two shards: short rows stay
    singular after the sum, and the NaN the user solve leaves in L reaches the item records"""
    capi = device
    K = 10
    pat, L0, R0, val, _ = _not_pd_inputs(K)
    cuts = (0, 50, pat.users)
    lam = (0.0, 0.0)
    shards = shards_of(pat, val, None, cuts)
    blocks, R1, cu, ci = sharded_iteration(shards, L0, R0, lam, kind)
    assert np.isnan(np.concatenate(blocks)).any() and ci[2] >= 8 and ci[0] >= 8 and sum(c[2] for c in cu) >= 8
    kept = (R1.view(np.uint64) == R0.view(np.uint64)).all(axis=1)
    assert kept.sum() >= ci[1] + ci[2]
    switches({})
    for g, (L, R, gcu, gci) in enumerate(run_shards(capi, pat, K, val, None, cuts, kind, L0, R0, lam)):
        where = "%s shard %d" % (kind, g)
        assert_same_bits(L, blocks[g], where + ": L block")
        assert_same_bits(R, R1, where + ": R")
        assert_same_bits(R[kept], R0[kept], where + ": a kept row holds X_old's bits")
        assert gcu == cu[g] and gci == ci, (where, gcu, gci, ci)


@gpu
def test_a_nan_in_y_keeps_every_row_under_the_implicit_kind(device, switches):
    capi = device
    K = 10
    pat, L0, R0, val, _ = _small()
    L0 = L0.copy()
    L0[45, 3] = np.nan      # in the second shard's block: its Gram, and so the sum, is NaN
    cuts = (0, 30, pat.users)
    shards = shards_of(pat, val, None, cuts)
    N, S = summed_item_records(shards, [L0[:30], L0[30:]], R0, -1, CONF)
    R1, ci = solve_records(N, S, R0, LAM_I, "implicit")
    assert np.isnan(S).any() and ci == (0, 0, pat.items)
    switches({})
    for g, (_, R, _, gci) in enumerate(run_shards(capi, pat, K, val, None, cuts, "implicit", L0, R0, other="current", user_solve=False)):
        assert gci == ci, (g, gci)
        assert_same_bits(R, R0, "shard %d: every row keeps X_old's bits" % g)


# ---- E: the split side
@gpu
def test_cut_solve_on_a_split_side(device, switches):
    """MF_SWEEP_LONG=128 on `skewed` gives both sides extreme rows: both row lists of walk_row_lists launch, into one buffer
    and the same three counters"""
    capi = device
    K = 10
    pat = pattern("skewed")
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    switches({"MF_SWEEP_LONG": "128", "MF_ALS_FORM": "wg"})
    ref, cut = als_plan(capi, pat, K, val, "ridge"), als_plan(capi, pat, K, val, "ridge")
    try:
        n = long_rows(cut.describe())
        assert n is not None and 0 < n[0] < pat.items and 0 < n[1] < pat.users, cut.describe()
        ref.upload(L0, R0)
        cut.upload(L0, R0)
        want = hand_iteration(ref, "split")
        assert cut_iteration(cut) == want and sum(want[0]) == pat.users and sum(want[1]) == pat.items
        (L, R), (L1, R1) = cut.download(), ref.download()
        assert_same_bits(L, L1, "split: L")
        assert_same_bits(R, R1, "split: R")
    finally:
        ref.close()
        cut.close()


# ---- F: refusals
def refused(capi, call, status):
    with pytest.raises(capi.HipBackendError) as err:
        call()
    assert err.value.status == status, (err.value.status, status)


@gpu
def test_refusals_change_nothing(device, switches):
    capi = device
    import torch
    K = 10
    pat, L0, R0, val, alpha = _small()
    pitch = pitch_of(K)
    switches({})
    buf = normal_buffer(pat.items, pitch + 2)
    ptr = buf.data_ptr()
    A, S, U = capi.MF_ERR_ARGUMENT, capi.MF_ERR_STATE, capi.MF_ERR_UNSUPPORTED

    def both(plan, status, side="items", other="next", p=ptr, pt=pitch):
        refused(capi, lambda: plan.als_normal(side, other, p, pt), status)
        if other == "next":
            refused(capi, lambda: plan.als_solve_normal(side, p, pt), status)

    def untouched(plan, where):
        plan.synchronize()
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()), where
        L, R = plan.download()
        assert_same_bits(L, L0, where + ": L")
        assert_same_bits(R, R0, where + ": R")
        assert plan.als_info("items") == (0, 0, 0)

    plan = als_plan(capi, pat, K, val, "ridge")
    try:
        both(plan, S)                                  # no factors
        plan.upload(L0, R0)
        for side in (-1, 2):
            both(plan, A, side=side)
        for gen in (-1, 2):
            both(plan, A, other=gen)
        both(plan, A, p=None)
        both(plan, A, p=ptr + 8)                        # not 16-byte aligned
        both(plan, A, pt=pitch + 1)
        both(plan, A, pt=pitch - 2)
        plan.set_als("off")
        both(plan, S)
        plan.set_als("ridge-count")
        plan.set_als_cg(3)
        both(plan, U)
        plan.set_als_cg(0)
        untouched(plan, "explicit refusals")
        both_ok = cut_solve(plan, "items", "current", pitch + 2, buf)      # and the accepted call works on the same plan
        assert both_ok[0] > 0
    finally:
        plan.close()
    buf.fill_(float("nan"))
    torch.cuda.synchronize()
    plan = implicit_plan(capi, pat, K, val, CONF)
    try:
        plan.upload(L0, R0)
        plan.set_implicit_cg(3)
        both(plan, U)
        plan.set_implicit_cg(0)
        plan.set_frozen_columns(-1, 2)
        both(plan, U, side="items")
        untouched(plan, "implicit refusals")
        user_buf = normal_buffer(pat.users, pitch)
        plan.als_normal("users", "current", user_buf.data_ptr(), pitch)   # the users have no frozen column
        plan.synchronize()
    finally:
        plan.close()
    pat9, L9, R9, val9, _ = _small(K=129)
    plan = capi.Plan(pat9.users, pat9.items, 129, alpha, pat9.row, pat9.col, val9)
    try:
        plan.set_als_cg(2)
        plan.set_als("ridge")
        plan.upload(L9, R9)
        big = normal_buffer(pat9.items, pitch_of(129))
        both(plan, U, p=big.data_ptr(), pt=pitch_of(129))
        plan.synchronize()
        torch.cuda.synchronize()
        assert bool(torch.isnan(big).all())
    finally:
        plan.close()


# ---- G: stream order
@gpu
@pytest.mark.parametrize("kind", ["ridge-count", "implicit"])
def test_normal_sum_and_solve_on_one_caller_stream_without_host_synchronisation(device, switches, kind):
    """als_normal, torch's in-place sum and als_solve_normal enqueued back to back on one non-default stream that is busy when
    the first call is made; the synchronised run of the same steps is the reference"""
    capi = device
    import torch
    K = 30
    pat = pattern("pair")
    L0, R0, val, _ = cls_signed(4000 + K, pat, K)
    pitch = pitch_of(K)
    switches({})
    rng = np.random.default_rng(5)
    extra_host = np.zeros((pat.items + 1, pitch))
    extra_host[:, :K * (K + 1) // 2 + K] = rng.uniform(-0.01, 0.01, (pat.items + 1, K * (K + 1) // 2 + K))
    extra_host[np.arange(0, pat.items, 5), K * (K + 1) // 2 + K] = 1.0     # some counts move
    results = []
    for ordered in (False, True):
        plan = implicit_plan(capi, pat, K, val, CONF) if kind == "implicit" else als_plan(capi, pat, K, val, kind)
        try:
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
    assert i_sync == i_ord and i_sync[0] > 90
    assert_same_bits(N_ord, N_sync, "the summed records")
    assert_same_bits(R_ord, R_sync, "R")
    assert differs(R_sync, R0) > 0.9


# ---- H: 64-bit offsets
@gpu
def test_records_beyond_two_to_the_31_doubles(device, switches):
    """rows = 5, K = 2, pitch = 2^29 + 2: record 4 starts beyond 2^31 doubles, the Gram record at 5 (2^29 + 2).  The buffer
    is never read whole"""
    capi = device
    import torch
    K, pitch = 2, (1 << 29) + 2
    T, np_ = 3, pitch_of(2)
    pat = lengths_pattern([3, 0, 9, 1, 17], 20)
    L0, R0, val, _ = cls_signed(77, pat, K)
    assert pat.ulen.tolist() == [3, 0, 9, 1, 17]
    assert 4 * pitch > 1 << 31
    (one,) = shards_of(pat, val, None, (0, pat.users))
    want = normal_records(one.side[1], one.val, None, L0, R0, -1, CONF)
    L1, cu = solve_records(want, gram(R0), L0, LAM_U, "implicit")
    switches({})
    buf = torch.empty((pat.users + 1, pitch), dtype=torch.float64, device=cuda())
    buf[:, :np_ + 2] = float("nan")
    buf[:, -2:] = float("nan")
    torch.cuda.synchronize()
    plan = implicit_plan(capi, pat, K, val, CONF)
    try:
        plan.upload(L0, R0)
        plan.als_normal("users", "current", buf.data_ptr(), pitch)
        plan.synchronize()
        got = buf[:, :np_ + 2].cpu().numpy()
        assert_same_bits(got[:5, :T + K + 1], want, "the five records")
        assert_same_bits(got[5, :T], gram(R0), "the Gram record")
        assert (got[5, T:np_].view(np.uint64) == 0).all() and np.isnan(got[:, np_:]).all() and bool(torch.isnan(buf[:, -2:]).all())
        plan.als_solve_normal("users", buf.data_ptr(), pitch)
        assert plan.als_info("users") == cu == (5, 0, 0)
        plan.flip()
        assert_same_bits(plan.download(want_r=False)[0], L1, "the solve from records beyond 2^31 doubles")
    finally:
        plan.close()
        del buf
        torch.cuda.empty_cache()
