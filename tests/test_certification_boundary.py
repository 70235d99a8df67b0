"""The top-1 certification and the filter report at their decision edge.

A user is certified when best - second > thr_i = margin(K) * ||L[i]|| * max||R[j]|| + 1e-300 (recommend_mfma_kernel's header).
The other modules pin the ANSWERS of that machinery on random factors, whose gaps are 1e-1 against a thr of 1e-12: a
runner-up lost on its way through the score registers of a lane, the 16 lanes of a row, the two item halves of a tile, the
successive tiles, merge_splits_kernel or certify_filters changes no answer there.  Here the decision itself is pinned.

The instance (boundary_instance): standard-normal factors, and for each of 33 planted users an anchor item scaled to twice
the largest row norm of R with L[u] = 3 * R[anchor] and a twin item R[twin] = f * R[anchor], so that anchor and twin are
the user's two best items at every K.  The twin pairs sit 1, 16, 48, 64, 128 and 256 items apart, across every boundary of
the item splits the tests force (128, 256, 384, 512), on the last item, as a triple over three tiles, and once with the
twin rated.  f is 1, 1 + 2^-52, 1 - 2^-52, 1 - margin / 4 (a gap of T / 4) or 1 - 4 margin (a gap of 4 T), each with the
larger twin at the lower and at the higher index.  The TRUE gap g of every pair is computed in exact arithmetic
(fractions.Fraction over the K products) and the user classified against T = margin * ||L[u]|| * max||R[j]|| from
long-double norms:
    tie    g <= T / 2
    clear  g >= 2 T, and the third-best reference score more than 2 T below the best.
Any computed score is within gamma_K * ||l|| * ||r|| <= T / 8 of the exact one, whatever the summation order, so a tie has a
computed gap <= 3 T / 4 (below thr: it must NOT be certified) and a clear one >= 1.75 T (it MUST be); the kernel's norms
are off by at most (K + 2) * 2^-53, which the two classes leave room for.  Nothing here is measured on the code under test.

The reference is oracle.predict_row (the sequential, unfused sum); a score is within T_u / 4 of it, which bounds the
filter report's best and second and the loss of its arg.

The anchors' large norms put a twin pair on top of the rows of about half of the UNPLANTED users as well.  Those are
classified too, from the reference rows (a reference gap <= T / 4 is a true gap <= T / 2, one >= 2.25 T a true gap >= 2 T),
so that ties <= exact-pass users <= users - clears leaves room for a handful of users, not for a hundred, and the per-user
assertions on the filter report cover everybody.  The planted users are what guarantees every site, kind and order.
"""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_topn import assert_same, model_topn  # noqa: E402

USERS, ITEMS = 200, 517              # four 64-user (two 128-user) blocks, the last partial; five tiles, the last of 5 items
KS_FORMS = [16, 20, 32, 40, 48, 60, 64, 66, 70, 72, 80, 90, 96, 98, 100, 104, 112, 128, 256]   # test_recommend_every_chunk_depth_and_staging_form's
# Above K = 256 every plan takes recommend_mfma_kernel with both operands staged through registers, 128 users a workgroup
# (the resident-L image ends at K = 100 and the 64-user kernels at 256; MF_RECOMMEND_BDMA / _HALF then change nothing, the
# four FORMS run the same kernel, and the plan's description has no entry for the top-1 pass that a test could read: the
# form follows from launch_recommend's rule alone): the first even and the first odd K of that range -- the odd one takes the non-vector
# instance --, a K of 32 chunks less one (1000 = 31 x 32 + 8) and the largest K, whose margin is 16 times that of 256.
KS_WIDE = [258, 301, 1000, 4096]
KS = KS_FORMS + [2, 4, 6, 17, 33] + KS_WIDE
KS_SPLIT_MATRIX = (100, 48, 256, 17)
KS_GRID = (100, 48, 256, 17, 30)
FORMS = [("1", "1"), ("1", "all"), ("1", "0"), ("0", "0")]      # (MF_RECOMMEND_BDMA, MF_RECOMMEND_HALF)

# (lo, hi) item pairs, three per site: one user each for a tie with the larger twin at lo, a tie with it at hi, a clear pair
SITES = [
    ("lanes of a row, +1", [(5, 6), (7, 8), (9, 10)]),
    ("registers of a lane, +16", [(20, 36), (21, 37), (22, 38)]),
    ("registers of a lane, +48", [(67, 115), (68, 116), (69, 117)]),
    ("item halves of a tile, +64", [(140, 204), (141, 205), (142, 206)]),
    ("successive tiles, +128", [(200, 328), (201, 329), (202, 330)]),
    ("successive tiles, +256", [(40, 296), (41, 297), (42, 298)]),
    ("across item 384 (two splits)", [(383, 384), (382, 385), (381, 386)]),
    ("across item 256 (three splits)", [(255, 256), (254, 257), (253, 258)]),
    ("across item 512 (three splits; the partial tile)", [(511, 512), (510, 513), (509, 514)]),
    ("across item 128 (a split per tile)", [(127, 128), (126, 129), (125, 130)]),
]
LAST_PAIR = (450, ITEMS - 1)         # tie, the larger twin first: the runner-up is the last item of the partial tile
TRIPLE = (300, 470, 60)              # best, 2^-52 below it, margin / 4 below it: tiles 2, 3 and 0
RATED_PAIR = (350, 351)              # exact duplicates, 351 rated by its user: the user is clear
TIE_KINDS = ["dup", "ulp_up", "ulp_dn", "quarter"]
# block edges of the 64- and the 128-user kernels first, each followed by an ordinary user
PLANTED_USERS = [0, 1, 15, 14, 16, 17, 31, 30, 32, 33, 63, 47, 64, 48, 65, 62, 127, 66, 128, 79, 129, 80, USERS - 1, 95, 96,
                 111, 112, 126, 130, 143, 144, 191, 192]
EDGE_USERS = [0, 15, 16, 31, 32, 63, 64, 65, 127, 128, 129, USERS - 1]
FULL_USER, ONE_USER, EMPTY_USER, TWO_USER = 100, 101, 102, 103      # nothing / one item / everything / two items unrated
CUTS = (6, 128, 256, 300, 384, 512)  # inside a tile, tile edges, across (200, 328) and (40, 296), the last five items


def margin_of(K):
    """mf_backend_recommend_margin restated: 8 (K + 8) 2^-53"""
    return 8.0 * (K + 8) * 2.0 ** -53


def _factor(kind, K):
    m = margin_of(K)
    return {"dup": 1.0, "ulp_up": 1.0 + 2.0 ** -52, "ulp_dn": 1.0 - 2.0 ** -52, "quarter": 1.0 - m / 4, "clear4": 1.0 - 4 * m}[kind]


def _plantings():
    """[(user, anchor item, twin item, kind, site)]: R[twin] = f(kind) * R[anchor], L[user] = 3 * R[anchor]"""
    def place(lo, hi, kind, big_lo):
        # the anchor is the larger twin except for "ulp_up", whose twin is the larger one
        anchor_lo = big_lo != (kind == "ulp_up")
        return (lo, hi, kind) if anchor_lo else (hi, lo, kind)

    out = []
    for p, (site, pairs) in enumerate(SITES):
        out.append(place(*pairs[0], TIE_KINDS[p % 4], True) + (site,))
        out.append(place(*pairs[1], TIE_KINDS[(p + 2) % 4], False) + (site,))
        out.append(place(*pairs[2], "clear4", p % 2 == 0) + (site,))
    out.append(place(*LAST_PAIR, "quarter", True) + ("the last item",))
    out.append((TRIPLE[0], TRIPLE[1], "ulp_dn", "a triple over three tiles"))
    out.append((RATED_PAIR[0], RATED_PAIR[1], "dup", "the twin is rated"))
    assert len(out) == len(PLANTED_USERS) and set(EDGE_USERS) <= set(PLANTED_USERS)
    return [(u,) + pl for u, pl in zip(PLANTED_USERS, out)]


def _long_norms(X):
    return np.sqrt((X.astype(np.longdouble) ** 2).sum(axis=1))


def _exact_score(l, r):
    return sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(l, r)), Fraction(0))


_instances = {}


def boundary_instance(orc, K):
    """The planted instance at K, with its reference rows, its classes and the generator's own assertions; built once per K
    and read-only."""
    if K in _instances:
        return _instances[K]
    rng = np.random.default_rng(9000 + K)
    L = rng.standard_normal((USERS, K))
    R = rng.standard_normal((ITEMS, K))
    norm_big = 2.0 * float(np.sqrt((R * R).sum(axis=1)).max())
    rated = rng.random((USERS, ITEMS)) < 0.2
    rated[FULL_USER, :] = True
    rated[ONE_USER, :] = True
    rated[ONE_USER, 44] = False
    rated[EMPTY_USER, :] = False
    rated[TWO_USER, :] = True
    rated[TWO_USER, [130, 131]] = False
    plantings = _plantings()
    used = [j for pl in plantings for j in pl[1:3]] + [TRIPLE[2]]
    assert len(set(used)) == len(used) and max(used) == ITEMS - 1
    for u, a, b, kind, site in plantings:
        R[a] *= norm_big / np.sqrt((R[a] * R[a]).sum())
        R[b] = _factor(kind, K) * R[a]
        L[u] = 3.0 * R[a]
        rated[u, [a, b]] = False
    # the twins 4 T below their anchor are rated by every unplanted user: on top of such a user's row (its score there is
    # cos(angle) times the planted user's) the pair would be 4 T cos(angle) apart, which is neither a tie nor clear
    others = np.setdiff1d(np.arange(USERS), PLANTED_USERS + [EMPTY_USER])
    for u, a, b, kind, site in plantings:
        if kind == "clear4":
            rated[others, b] = True
    R[TRIPLE[2]] = _factor("quarter", K) * R[TRIPLE[0]]
    rated[plantings[-2][0], TRIPLE[2]] = False
    rated[plantings[-1][0], RATED_PAIR[1]] = True
    row, col = np.nonzero(rated)
    row, col = row.astype(np.int32), col.astype(np.int32)
    val = rng.integers(1, 6, row.shape[0]).astype(np.float64)

    B = np.stack([orc.predict_row(np.ascontiguousarray(L[u]), R) for u in range(USERS)])
    assert np.isfinite(B).all()
    masked = np.where(rated, -np.inf, B)
    rmax = float(_long_norms(R).max())
    lnorm = _long_norms(L)
    margin = margin_of(K)
    ties, clears, planted = [], [], []
    for u, a, b, kind, site in plantings:
        T = margin * float(lnorm[u]) * rmax
        order = np.argsort(-masked[u], kind="stable")
        if site == "the twin is rated":
            g = _exact_score(L[u], R[a]) - max(_exact_score(L[u], R[j]) for j in order[1:3])
            assert order[0] == a and rated[u, b], (K, u)
            third = masked[u, order[1]]
        else:
            g = abs(_exact_score(L[u], R[a]) - _exact_score(L[u], R[b]))
            assert {int(order[0]), int(order[1])} == {a, b}, (K, u, site, order[:3])      # the reference's top two
            third = masked[u, order[2]]
        if g <= Fraction(T) / 2:
            cls = "tie"
            ties.append(u)
        else:
            assert g >= 2 * Fraction(T) and masked[u, order[0]] - third > 2 * T, (K, u, site, float(g), T)
            cls = "clear"
            clears.append(u)
        assert cls == ("clear" if kind == "clear4" or site == "the twin is rated" else "tie"), (K, u, site, kind, float(g), T)
        planted.append(dict(user=u, anchor=a, twin=b, kind=kind, site=site, cls=cls, T=T, gap=float(g)))
    assert len(ties) >= 8 and len(clears) >= 8
    # Everybody else, from the reference rows alone: a reference score is within gamma_K * ||l|| * ||r|| <= T / 8 of the exact
    # one, so a reference gap <= T / 4 is a true gap <= T / 2 (a tie) and one >= 2.25 T a true gap >= 2 T (clear; the third
    # best lies below the second).  The anchors' large norms put a twin pair on top of many an unplanted user as well, so
    # without these the count of exact-pass users would say little about the planted ones.
    srt = np.sort(masked, axis=1)
    T_all = margin * lnorm.astype(np.float64) * rmax
    with np.errstate(invalid="ignore"):
        g_ref = srt[:, -1] - srt[:, -2]                    # inf with one unrated item, NaN with none
    others = np.setdiff1d(np.arange(USERS), PLANTED_USERS)
    planted_ties, planted_clears = list(ties), list(clears)
    ties += [int(u) for u in others if g_ref[u] <= T_all[u] / 4]
    clears += [int(u) for u in others if g_ref[u] >= 2.25 * T_all[u]]
    assert FULL_USER not in ties + clears and ONE_USER in clears
    want = orc.recommend(orc.Instance(1, 0.01, K, USERS, ITEMS, row, col, val), L, R)
    top_items, top_scores = model_topn(orc, USERS, ITEMS, row, col, L, R, 3)
    assert np.array_equal(top_items[:, 0], want)
    inst = dict(K=K, L=L, R=R, row=row, col=col, val=val, rated=rated, B=B, masked=masked, margin=margin, planted=planted,
                ties=np.sort(np.array(ties)), clears=np.sort(np.array(clears)), planted_ties=np.array(planted_ties),
                planted_clears=np.array(planted_clears), want=want, top_items=top_items, top_scores=top_scores)
    for v in inst.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _instances[K] = inst
    return inst


def check_filter_report(inst, f, norm, rmax, where, u0=0):
    """Section 3 of the module's contract, for the users u0 .. u0 + len(f): best, second and arg of a filter report against
    the reference rows; the planted classes against thr.  Returns (ties held back, clears certified)."""
    n = f.shape[0]
    masked, margin = inst["masked"][u0:u0 + n], inst["margin"]
    srt = np.sort(masked, axis=1)
    top1, top2 = srt[:, -1], srt[:, -2]                   # -inf with fewer than one / two unrated items
    none = ~np.isfinite(top1)
    T = margin * norm * rmax
    assert np.isfinite(T).all() and (T > 0).all(), where
    with np.errstate(invalid="ignore"):
        ok = (f["best"] == top1) | (np.abs(f["best"] - top1) <= T / 4)
        assert ok.all(), (where, "best", u0 + np.flatnonzero(~ok)[:8], f["best"][~ok][:4], top1[~ok][:4])
        ok = (f["second"] == top2) | (np.isfinite(top2) & (np.abs(f["second"] - top2) <= T / 4))
        assert ok.all(), (where, "second", u0 + np.flatnonzero(~ok)[:8], f["second"][~ok][:4], top2[~ok][:4], T[~ok][:4])
    assert np.array_equal(f["arg"] < 0, none) and (f["arg"][none] == -1).all(), (where, "arg = -1 exactly for fully rated users")
    live = np.flatnonzero(~none)
    assert (f["arg"][live] < ITEMS).all() and not inst["rated"][u0 + live, f["arg"][live]].any(), (where, "arg is rated")
    ok = inst["B"][u0 + live, f["arg"][live]] >= top1[live] - T[live] / 2
    assert ok.all(), (where, "arg", u0 + live[~ok][:8])
    assert (f["best"][none] == -np.inf).all() and (f["second"][none] == -np.inf).all()
    assert (f["nonfinite"] == 0).all(), (where, "nonfinite", u0 + np.flatnonzero(f["nonfinite"])[:8])
    thr = margin * (norm * rmax) + 1e-300                 # cert_margin's expression
    with np.errstate(invalid="ignore"):
        gap = f["best"] - f["second"]                     # NaN for -inf - -inf: no planted user
    ties = inst["ties"][inst["ties"] >= u0] - u0
    clears = inst["clears"][inst["clears"] >= u0] - u0
    bad = ties[~(gap[ties] <= thr[ties])]
    assert bad.size == 0, (where, "tie certified", [(p["user"], p["site"], p["kind"]) for p in inst["planted"] if p["user"] - u0 in bad])
    bad = clears[~(gap[clears] > thr[clears])]
    assert bad.size == 0, (where, "clear held back", [(p["user"], p["site"], p["kind"]) for p in inst["planted"] if p["user"] - u0 in bad])
    return len(ties), len(clears)


def records_from(S, rated, j0=0):
    """mf_filter records of the score block S (users x its items, rated masked out), arg GLOBAL: what a pass with S for
    scores reports"""
    import recommender_system_amd as rs
    masked = np.where(rated, -np.inf, S)
    f = np.zeros(S.shape[0], rs.capi.FILTER_DTYPE)
    if S.shape[1] == 0:
        f["best"], f["second"], f["arg"] = -np.inf, -np.inf, -1
        return f
    order = np.argsort(-masked, axis=1, kind="stable")
    cols = np.arange(S.shape[0])
    f["best"] = masked[cols, order[:, 0]]
    f["second"] = masked[cols, order[:, 1]] if S.shape[1] > 1 else -np.inf
    f["arg"] = np.where(np.isfinite(f["best"]), order[:, 0] + j0, -1)
    return f


def double_norms(X):
    return np.sqrt((X * X).sum(axis=1))


# ------------------------------------------------------------------------------------------------ CPU
def test_margin_is_the_headers(capi):
    for K in KS + [30]:
        assert capi.recommend_margin(K) == margin_of(K)
        assert 2 * (K * 2.0 ** -53 / (1 - K * 2.0 ** -53)) <= margin_of(K) / 4          # 2 gamma_K <= margin / 4


@pytest.mark.parametrize("K", sorted(set(KS) | set(KS_GRID)))
def test_generator_classes_hold_for_any_summation_order(orc, K):
    """The generator's assertions at every K used below, and the class reasoning with numpy's L @ R.T standing in for "any
    summation order": its top-2 gap is <= thr for every tie and > thr for every clear user, its report passes the checks
    the GPU report has to pass."""
    inst = boundary_instance(orc, K)
    kinds = {(p["site"], p["cls"]) for p in inst["planted"]}
    for site, _ in SITES:
        assert (site, "tie") in kinds and (site, "clear") in kinds
    assert set(EDGE_USERS) <= {p["user"] for p in inst["planted"]}
    assert {p["cls"] for p in inst["planted"] if p["user"] in EDGE_USERS} == {"tie", "clear"}
    for p in inst["planted"]:
        assert p["gap"] <= p["T"] / 2 or p["gap"] >= 2 * p["T"]
    S = inst["L"] @ inst["R"].T
    f = records_from(S, inst["rated"])
    nt, nc = check_filter_report(inst, f, double_norms(inst["L"]), float(double_norms(inst["R"]).max()), ("numpy", K))
    assert nt >= 8 and nc >= 8 and len(inst["planted_ties"]) + len(inst["planted_clears"]) == len(PLANTED_USERS)
    assert set(inst["planted_ties"]) <= set(inst["ties"]) and set(inst["planted_clears"]) <= set(inst["clears"])
    assert not set(inst["ties"]) & set(inst["clears"])
    print("K %d: %d ties, %d clear users of %d" % (K, nt, nc, USERS))
    assert f["arg"][FULL_USER] == -1 and f["second"][ONE_USER] == -np.inf and np.isfinite(f["second"][TWO_USER])


def _partitions():
    for n in range(0, 4):
        for cuts in itertools.combinations(CUTS, n):
            yield [0] + list(cuts) + [ITEMS]


@pytest.mark.parametrize("K", [100, 17])
def test_certify_filters_holds_the_classes_over_every_partition(orc, K):
    """certify_filters on records built from L @ R.T, over every partition into 1 to 4 blocks with cuts out of CUTS (42 of
    them): no tie certain, every clear user certain -- pair inside one block or across two --, certain answers the
    reference's."""
    import importlib
    sh = importlib.import_module("recommender_system_amd.sharded")
    inst = boundary_instance(orc, K)
    S = inst["L"] @ inst["R"].T
    norm, rmax = double_norms(inst["L"]), float(double_norms(inst["R"]).max())
    count = 0
    for ib in _partitions():
        filters = [records_from(S[:, a:b], inst["rated"][:, a:b], a) for a, b in zip(ib[:-1], ib[1:])]
        ans, certain = sh.certify_filters(filters, norm, rmax, inst["margin"])
        assert not certain[inst["ties"]].any(), (ib, inst["ties"][certain[inst["ties"]]])
        assert certain[inst["clears"]].all(), (ib, inst["clears"][~certain[inst["clears"]]])
        assert np.array_equal(ans[certain], inst["want"][certain]), ib
        assert certain[FULL_USER] and ans[FULL_USER] == -1
        count += 1
    assert count == 42


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


def _env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def settings_of(K):
    """(BDMA, HALF, ARES, SPLIT) of every plan at K: the four forms, the split rule and no split; every split at the four K
    of the split matrix; the image without a resident L at K = 64"""
    splits = [None, "0", "2", "3"] if K in KS_SPLIT_MATRIX else [None, "0"]
    out = [(b, h, None, s) for b, h in FORMS for s in splits]
    if K == 64:
        out += [("1", "0", "0", s) for s in splits]
    return out


def _plan_under(capi, monkeypatch, inst, setting, u0=0):
    bdma, half, ares, split = setting
    _env(monkeypatch, "MF_RECOMMEND_BDMA", bdma)
    _env(monkeypatch, "MF_RECOMMEND_HALF", half)
    _env(monkeypatch, "MF_RECOMMEND_ARES", ares)
    _env(monkeypatch, "MF_RECOMMEND_SPLIT", split)
    m = inst["row"] >= u0
    plan = capi.Plan(USERS, ITEMS, inst["K"], 0.01, inst["row"][m], inst["col"][m], inst["val"][m], user_begin=u0, user_count=USERS - u0)
    plan.upload(inst["L"][u0:], inst["R"])
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_top1_certifies_no_tie_and_every_clear_user(gpu, orc, K, monkeypatch):
    """mf_plan_recommend under every form and split: the reference's answers, and ties <= exact-pass users <= users - clears
    (a lost runner-up certifies a tie; a kernel that certifies nobody does not pass either).  recommend_topn(3) of the same
    plan against the model, items and score bits."""
    inst = boundary_instance(orc, K)
    nt, nc = len(inst["ties"]), len(inst["clears"])
    for setting in settings_of(K):
        plan = _plan_under(gpu, monkeypatch, inst, setting)
        best = plan.recommend()
        sent = plan.recommend_info()
        it, sc = plan.recommend_topn(3)
        plan.close()
        assert np.array_equal(best, inst["want"]), (K, setting, np.flatnonzero(best != inst["want"])[:8])
        assert nt <= sent <= USERS - nc, (K, setting, "ties %d, exact-pass users %d, users - clears %d" % (nt, sent, USERS - nc))
        assert_same(it, sc, inst["top_items"], inst["top_scores"], (K, setting))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_filter_report_per_user(gpu, orc, K, monkeypatch):
    """mf_plan_recommend_filter under every form and split: best, second and arg of every user against the reference row,
    every tie held back and every clear user certified by the returned norms."""
    inst = boundary_instance(orc, K)
    for setting in settings_of(K):
        plan = _plan_under(gpu, monkeypatch, inst, setting)
        if K == 60:
            assert plan.pitches() == (64, 64)             # the plan's own padded rows
        f, norm, rmax = plan.recommend_filter()
        plan.close()
        check_filter_report(inst, f, norm, rmax, (K, setting))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [100, 60, 17])
def test_filter_report_of_a_shard_from_user_77(gpu, orc, K, monkeypatch):
    inst = boundary_instance(orc, K)
    for setting in settings_of(K)[:4]:
        plan = _plan_under(gpu, monkeypatch, inst, setting, u0=77)
        f, norm, rmax = plan.recommend_filter()
        best = plan.recommend()
        plan.close()
        assert f.shape[0] == USERS - 77 and np.array_equal(best, inst["want"][77:])
        nt, nc = check_filter_report(inst, f, norm, rmax, (K, setting, "from 77"), u0=77)
        assert nt >= 4 and nc >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("K", [100, 48, 256, 17])
def test_nan_row_and_inf_entry_are_never_certified(gpu, orc, K, monkeypatch):
    """A NaN row of L: that user is not certified, and the classes of everybody else hold on the screening path its
    workgroup now takes.  An inf entry in an item: no user with that item unrated is certified."""
    import importlib
    sh = importlib.import_module("recommender_system_amd.sharded")
    inst = boundary_instance(orc, K)
    nan_user, inf_item = 150, 333
    assert nan_user not in PLANTED_USERS and not inst["rated"][nan_user].all()
    ties, clears = inst["ties"][inst["ties"] != nan_user], inst["clears"][inst["clears"] != nan_user]
    for split in (None, "0"):
        for what in ("nan", "inf"):
            L, R = inst["L"].copy(), inst["R"].copy()
            if what == "nan":
                L[nan_user, :] = np.nan
            else:
                R[inf_item, 3] = np.inf
            _env(monkeypatch, "MF_RECOMMEND_SPLIT", split)
            plan = gpu.Plan(USERS, ITEMS, K, 0.01, inst["row"], inst["col"], inst["val"])
            plan.upload(L, R)
            f, norm, rmax = plan.recommend_filter()
            best = plan.recommend()
            sent = plan.recommend_info()
            plan.close()
            ans, certain = sh.certify_filters([f], norm, rmax, inst["margin"])
            want = orc.recommend(orc.Instance(1, 0.01, K, USERS, ITEMS, inst["row"], inst["col"], inst["val"]), L, R)
            assert np.array_equal(best, want), (K, split, what)
            assert np.array_equal(ans[certain], want[certain]), (K, split, what)
            if what == "nan":
                assert not certain[nan_user] and not certain[ties].any() and certain[clears].all(), (K, split)
                assert len(ties) + 1 <= sent <= USERS - len(clears), (K, split, len(ties), sent, len(clears))
            else:
                open_ = ~inst["rated"][:, inf_item]
                assert open_.sum() > 100 and not certain[open_].any(), (K, split, np.flatnonzero(certain & open_)[:8])
                assert certain[FULL_USER] and sent >= open_.sum()


GRID_CUTS = {"one block": [0, ITEMS], "a cut inside tiles": [0, 300, ITEMS], "cuts on tile edges": [0, 128, 384, ITEMS],
             "a first block of 6, a last of 5 items": [0, 6, 256, 512, ITEMS]}


def _scan(brow, rated_row):
    """(best, first, first_nan) of recommend_kernel's scan over one block: numpy"""
    open_ = np.flatnonzero(~rated_row)
    if open_.size == 0:
        return -1, -1, 0
    first = int(open_[0])
    cand = open_[~np.isnan(brow[open_])]
    best = int(cand[np.argmax(brow[cand])]) if cand.size else -1
    return best, first, int(np.isnan(brow[first]))


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["rule", "0"])
@pytest.mark.parametrize("cuts", sorted(GRID_CUTS))
@pytest.mark.parametrize("K", KS_GRID)
def test_grid_certification_end_to_end(gpu, orc, K, cuts, split, monkeypatch):
    """A filter per item block, certify_filters over them, the exact scan of the rest merged in item order: the reference's
    answers; every tie in the exact pass, every clear user certain whether its pair lies inside a block or across two;
    every candidate record of the exact pass against the reference row, the score bit for bit.  Under the split rule a
    block this small is one tile per split; without a split a workgroup walks the block's tiles as it does on a large
    problem, with the cheap-reject bar carried from tile to tile."""
    _env(monkeypatch, "MF_RECOMMEND_SPLIT", None if split == "rule" else split)
    import importlib
    sh = importlib.import_module("recommender_system_amd.sharded")
    capi = gpu
    inst = boundary_instance(orc, K)
    ib = GRID_CUTS[cuts]
    across = [p for p in inst["planted"] if np.searchsorted(ib, p["anchor"], "right") != np.searchsorted(ib, p["twin"], "right")]
    if len(ib) > 2:
        assert {p["cls"] for p in across} == {"tie", "clear"} and len(across) < len(inst["planted"])
    plans, filts = [], []
    for a, b in zip(ib[:-1], ib[1:]):
        sel = (inst["col"] >= a) & (inst["col"] < b)
        plan = capi.Plan(USERS, b - a, K, 0.01, inst["row"][sel], inst["col"][sel] - np.int32(a), inst["val"][sel])
        plan.upload(inst["L"], np.ascontiguousarray(inst["R"][a:b]))
        f, norm, rmax = plan.recommend_filter()
        f["arg"][f["arg"] >= 0] += a
        plans.append(plan)
        filts.append((f, norm, rmax))
    ans, certain = sh.certify_filters([f[0] for f in filts], filts[0][1], float(np.max([f[2] for f in filts])), inst["margin"])
    todo = np.flatnonzero(~certain).astype(np.int32)
    assert not certain[inst["ties"]].any(), (K, ib, "tie certified", inst["ties"][certain[inst["ties"]]])
    assert certain[inst["clears"]].all(), (K, ib, "clear held back", inst["clears"][~certain[inst["clears"]]])
    assert np.array_equal(ans[certain], inst["want"][certain]), (K, ib)
    acc = None
    for (a, b), plan in zip(zip(ib[:-1], ib[1:]), plans):
        cand = plan.recommend_scored()[todo] if len(ib) == 2 else plan.recommend_scored_users(todo)
        plan.close()
        for t, u in enumerate(todo):
            best, first, first_nan = _scan(inst["B"][u, a:b], inst["rated"][u, a:b])
            c = cand[t]
            assert (c["best"], c["first"], c["first_nan"]) == (best, first, first_nan), (K, ib, a, u, c)
            if best >= 0:
                assert np.float64(c["score"]).view(np.int64) == inst["B"][u, a + best].view(np.int64), (K, ib, a, u)
        for name in ("best", "first"):
            cand[name][cand[name] >= 0] += a
        acc = cand if acc is None else sh.merge_candidates(acc, cand)
    ans[todo] = sh.finish_candidates(acc)
    assert np.array_equal(ans, inst["want"]), (K, ib, np.flatnonzero(ans != inst["want"])[:8])
