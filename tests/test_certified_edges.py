"""The certified matrix-core passes (top-1, top-N, ranks of held-out entries) at the edges the other modules leave out.

A  every K that launch_topn / the rank launch dispatch to an own template instance, both LDS forms of the four-wave ones;
B  tile, list and block edges: 1 .. 193 users x 1 .. 513 items, N beyond the unrated items, held-out sets around the 64- and
   256-entry blocks, item splits that do not divide the tiles, a user shard that starts at a user that is no multiple of 64;
C  row pitch != K on matrix-core forms: the plan's own padded buffers (K = 60) and caller-owned buffers whose padding is NaN;
D  an R buffer between 2^31 and 2^32 bytes (32-bit unsigned row offsets) and beyond 2^32 (the hand-over to the other forms);
E  power-of-two scaling of the factors: the reference's answers do not change, so neither may ours, and the certification
   must not certify MORE under scaling than it does unscaled (a norm that underflows shrinks the threshold).

The models are test_topn.py's and test_rank.py's (the header's definitions over exact sequential scores, oracle.predict_row);
every comparison is np.array_equal on int32 over all users / entries and assert_same's bit comparison of the scores.
"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import random_instance

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_loss import assert_bits, check_loss  # noqa: E402
from test_rank import TIED, _check_against_topn, heldout_for, model_ranks, rank_of  # noqa: E402
from test_topn import _plan, _rated_sets, assert_same, model_row, model_topn, planted_instance  # noqa: E402


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


# ------------------------------------------------------------------------------------------------ A: every dispatched K
KS_DISPATCHED = [16, 20, 32, 40, 48, 60, 64, 80, 96, 100, 112, 128, 256]     # the 13 K of launch_topn and the rank launch


def shape_of(K):
    """(k-steps per chunk, waves) of the instance K is dispatched to (certified_shape, mf_certified.hip.h: K % 20 is tested before K % 16)."""
    if K % 20 == 0 and K <= 100:
        return 5, 4
    if K % 16 == 0 and K <= 96:
        return 4, 4
    return {112: (4, 8), 128: (8, 8), 256: (8, 8)}[K]


def ring_lds(qc):
    """rec_mfma2_lds: a ring of 3 chunks of 2 qc k-pairs x 128 items x 16 bytes"""
    return 3 * (2 * qc) * 128 * 16


def list_lds(n):
    """topn_list_lds: 64 users x 2 item halves x (n + 1) entries of a double and an int"""
    return 64 * 2 * (n + 1) * (8 + 4)


def topn_form(K, n):
    """1: two workgroups per CU (four waves, ring + lists + 3 KB of static arrays within half of the CU's 160 KB); else 2"""
    qc, waves = shape_of(K)
    return 1 if waves == 4 and ring_lds(qc) + list_lds(n) + 3 * 1024 <= 80 * 1024 else 2


def rank_form(K):
    qc, waves = shape_of(K)
    return 1 if waves == 4 and ring_lds(qc) + 4 * 1024 <= 80 * 1024 else 2


def switch_over(K):
    """the largest N <= 32 that still runs two per CU (0: none does, 32: all do)"""
    return max([n for n in range(1, 33) if topn_form(K, n) == 1], default=0)


NS_A = sorted({1, 10, 11, 32} | {n for K in KS_DISPATCHED for n in (switch_over(K), switch_over(K) + 1) if 1 <= n <= 32})


def test_the_lds_rule_gives_both_forms_to_every_four_wave_k():
    """The rule restated above, from the sizes alone: the twenty family switches after N = 10, the sixteen family after
    N = 18, the eight-wave shapes never run two per CU -- so NS_A holds an N on either side for every four-wave K."""
    assert [switch_over(K) for K in (20, 100, 16, 96, 112, 128, 256)] == [10, 10, 18, 18, 0, 0, 0]
    assert NS_A == [1, 10, 11, 18, 19, 32]
    for K in KS_DISPATCHED:
        forms = {topn_form(K, n) for n in NS_A}
        assert forms == ({1, 2} if shape_of(K)[1] == 4 else {2}), K
        assert rank_form(K) == (1 if shape_of(K)[1] == 4 else 2)
    assert shape_of(80) == (5, 4)        # never the sixteen family's <5, 4>, which no K reaches


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["rule", "0"])
@pytest.mark.parametrize("K", KS_DISPATCHED)
def test_topn_every_dispatched_k_and_both_lds_forms(gpu, orc, K, split, monkeypatch):
    capi = gpu
    _env(monkeypatch, "MF_RECOMMEND_SPLIT", None if split == "rule" else split)
    users, items = 150, 700
    row, col, val, L, R = planted_instance(K, users, items, K)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 32)
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    best = plan.recommend()
    assert np.array_equal(best, orc.recommend(orc.Instance(1, 0.01, K, users, items, row, col, val), L, R))
    ran = {}
    for n in NS_A:
        it, sc = plan.recommend_topn(n)
        assert_same(it, sc, mi[:, :n], ms[:, :n], (K, n, split))
        assert np.array_equal(it[:, 0], best), (K, n, split)
        exact_users, ran[n] = plan.recommend_topn_info()
        assert ran[n] == topn_form(K, n), (K, n, ran[n])
        assert exact_users >= 2, (K, n, exact_users)        # the NaN and the inf user at least
    assert set(ran.values()) == ({1, 2} if shape_of(K)[1] == 4 else {2}), (K, ran)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["rule", "0"])
@pytest.mark.parametrize("K", KS_DISPATCHED)
def test_rank_every_dispatched_k(gpu, orc, K, split, monkeypatch):
    capi = gpu
    _env(monkeypatch, "MF_RECOMMEND_SPLIT", None if split == "rule" else split)
    users, items = 150, 700
    row, col, val, L, R = planted_instance(K, users, items, K)
    hrow, hcol, hval = heldout_for(K, users, items, row, col)
    hrow = np.concatenate([hrow, np.array([3, 3, 4, 4, 4], np.int32)])      # the NaN and the inf user, whatever the draw gave
    hcol = np.concatenate([hcol, np.array([0, 699, 5, 350, 698], np.int32)])
    hval = np.concatenate([hval, np.ones(5)])
    want = model_ranks(orc, users, items, row, col, L, R, hrow, hcol)
    assert (want == -1).any() and (want == -2).any() and (want >= 0).sum() > 300
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    plan.set_heldout(hrow, hcol, hval)
    got = plan.rank_heldout()
    assert got.dtype == np.int32 and np.array_equal(got, want), (K, split, np.flatnonzero(got != want)[:8])
    exact_entries, form = plan.rank_heldout_info()
    special = int(np.count_nonzero(((hrow == 3) | (hrow == 4)) & (want != -1)))
    assert form in (1, 2) and form == rank_form(K), (K, form)
    assert special >= 2 and exact_entries >= special, (exact_entries, special)
    nan_users = {i for i in range(users)
                 if np.isnan(orc.predict_row(np.ascontiguousarray(L[i]), R)[np.setdiff1d(np.arange(items), col[row == i])]).any()}
    assert _check_against_topn(plan, hrow, hcol, got, nan_users, (K, split)) > 300
    plan.close()


# ------------------------------------------------------------------------------------------------ B: tile, list and block edges
KS_B = [100, 48, 256, 30]        # five-chunk twenty family, sixteen family, eight waves, exact form
# every user count of {1, 63, 64, 65, 127, 128, 129, 193} and every item count of {1, 2, 63, 64, 65, 127, 128, 129, 385, 513}
SHAPES_B = [(1, 1), (1, 513), (193, 1), (63, 2), (64, 63), (65, 64), (127, 65), (128, 127), (129, 128), (193, 129),
            (63, 385), (129, 513), (64, 513)]
NS_B = [1, 4, 16, 32]            # planted users 5, 6, 8 keep exactly 1, 4, 16 unrated items; 32 exceeds many rows and item counts


def edge_instance(seed, users, items, K):
    """planted_instance (ties, NaN user, inf entry, full / empty / nearly full rows) where it fits; for fewer than nine
    users the same ratings density and duplicated R rows without the special users"""
    if users >= 9:
        return planted_instance(seed, users, items, K)
    rng = np.random.default_rng(seed)
    row, col = np.nonzero(rng.random((users, items)) < 0.15)
    val = rng.integers(1, 6, row.shape[0]).astype(np.float64)
    L = rng.standard_normal((users, K))
    R = rng.standard_normal((items, K))
    for a, b in [(3, 11), (7, 40), (100, 101), (200, 13)]:
        if max(a, b) < items:
            R[b] = R[a]
    return row.astype(np.int32), col.astype(np.int32), val, L, R


def heldout_edge_sets(seed, users, items, row, col):
    """name -> (hrow, hcol): sizes around the 64-entry rank blocks and the 256-entry finish blocks, drawn over all pairs (so
    training pairs, the tied items and repeats occur), all on one user, one per user, one pair 70 times"""
    rng = np.random.default_rng(seed)
    tied = [t for t in TIED if t < items]
    sets = {}
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        hr, hc = rng.integers(0, users, n), rng.integers(0, items, n)
        if tied:
            k = rng.random(n) < 0.2
            hc[k] = rng.choice(tied, int(k.sum()))
        sets["%d entries" % n] = (hr, hc)
    sets["130 on one user"] = (np.full(130, users - 1), rng.integers(0, items, 130))
    sets["one on every user"] = (np.arange(users), rng.integers(0, items, users))
    rated = _rated_sets(users, row, col)
    free = [(u, j) for u in (users - 1, 0, users // 2) for j in (items - 1, 0, items // 2) if j not in rated[u]]
    pair = free[0] if free else (users - 1, items - 1)
    sets["one pair 70 times"] = (np.full(70, pair[0]), np.full(70, pair[1]))
    return {k: (np.asarray(a, np.int32), np.asarray(b, np.int32)) for k, (a, b) in sets.items()}


def _forms_for(K, plan, n_items):
    """what the info calls must report for this K: the exact form for K = 30, a matrix-core form otherwise"""
    ti, tf = plan.recommend_topn_info()
    if K == 30 or n_items == 0:
        assert (ti, tf) == (-1, 0), (K, ti, tf)
    else:
        assert tf in (1, 2) and ti >= 0, (K, ti, tf)


def _check_topn_and_ranks(capi, orc, K, users, items, row, col, val, L, R, seed, where):
    mi, ms = model_topn(orc, users, items, row, col, L, R, 32)
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    best = plan.recommend()
    assert np.array_equal(best, orc.recommend(orc.Instance(1, 0.01, K, users, items, row, col, val), L, R)), where
    for n in NS_B:
        it, sc = plan.recommend_topn(n)
        assert_same(it, sc, mi[:, :n], ms[:, :n], (where, n))
        assert np.array_equal(it[:, 0], best), (where, n)
        _forms_for(K, plan, items)
    for name, (hrow, hcol) in heldout_edge_sets(seed, users, items, row, col).items():
        plan.set_heldout(hrow, hcol, np.ones(hrow.shape[0]))
        want = model_ranks(orc, users, items, row, col, L, R, hrow, hcol)
        got = plan.rank_heldout()
        assert np.array_equal(got, want), (where, name, np.flatnonzero(got != want)[:8])
        ei, ef = plan.rank_heldout_info()
        assert ((ei, ef) == (-1, 0)) if K == 30 else (ef in (1, 2) and ei >= 0), (where, name, ei, ef)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("users,items", SHAPES_B)
@pytest.mark.parametrize("K", KS_B)
def test_edges_topn_and_rank_across_tile_list_and_block_edges(gpu, orc, K, users, items):
    row, col, val, L, R = edge_instance(1000 * K + 7 * users + items, users, items, K)
    _check_topn_and_ranks(gpu, orc, K, users, items, row, col, val, L, R, K + users + items, (K, users, items))


@pytest.mark.gpu
@pytest.mark.parametrize("split", [None, "0", "2", "3", "7"])
@pytest.mark.parametrize("K", KS_B)
def test_edges_item_splits_that_do_not_divide_the_tiles(gpu, orc, K, split, monkeypatch):
    """513 items are five tiles of 128: 2, 3 and 7 splits leave a short or an empty last split"""
    _env(monkeypatch, "MF_RECOMMEND_SPLIT", split)
    for users in (1, 64, 129):
        row, col, val, L, R = edge_instance(77 * K + users, users, 513, K)
        _check_topn_and_ranks(gpu, orc, K, users, 513, row, col, val, L, R, K + users, (K, users, 513, split))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS_B)
def test_edges_user_shards_from_a_user_that_is_no_multiple_of_64(gpu, orc, K):
    """shards [0, 77) and [77, 193): top-N (items and score bits) and ranks of the shards concatenated are the whole plan's"""
    capi = gpu
    users, items = 193, 385
    row, col, val, L, R = planted_instance(500 + K, users, items, K)
    hrow, hcol, hval = heldout_for(K, users, items, row, col)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 32)
    whole = _plan(capi, users, items, K, row, col, val, L, R)
    wi, ws = whole.recommend_topn(32)
    assert_same(wi, ws, mi, ms, (K, "whole"))
    whole.set_heldout(hrow, hcol, hval)
    wr = whole.rank_heldout()
    assert np.array_equal(wr, model_ranks(orc, users, items, row, col, L, R, hrow, hcol))
    whole.close()
    gi, gs, gr = np.full_like(wi, -99), np.full_like(ws, 7.0), np.full_like(wr, -99)
    for u0, uc in ((0, 77), (77, users - 77)):
        m = (row >= u0) & (row < u0 + uc)
        h = (hrow >= u0) & (hrow < u0 + uc)
        p = capi.Plan(users, items, K, 0.01, row[m], col[m], val[m], user_begin=u0, user_count=uc)
        p.upload(L[u0:u0 + uc], R)
        assert np.array_equal(p.recommend(), wi[u0:u0 + uc, 0])
        for n in (1, 10, 32):
            it, sc = p.recommend_topn(n)
            assert_same(it, sc, mi[u0:u0 + uc, :n], ms[u0:u0 + uc, :n], (K, u0, n))
        gi[u0:u0 + uc], gs[u0:u0 + uc] = it, sc
        p.set_heldout(hrow[h], hcol[h], hval[h])
        gr[h] = p.rank_heldout()
        p.close()
    assert_same(gi, gs, wi, ws, (K, "shards"))
    live = wi >= 0
    assert np.array_equal(gs[live].view(np.int64), ws[live].view(np.int64)) and np.array_equal(gr, wr)


# ------------------------------------------------------------------------------------------------ C: row pitch
def pitch_instance(seed, users, items, K):
    """finite factors (the plan iterates), duplicated R rows, an empty and a full row, a held-out set with training pairs"""
    d = random_instance(seed, users, items, K, density=0.12, iters=4, alpha=1e-4, empty_rows=(2,), full_rows=(7,))
    rng = np.random.default_rng(seed + 1)
    L = rng.standard_normal((users, K)) * 0.3
    R = rng.standard_normal((items, K)) * 0.3
    R[11], R[40], R[101] = R[3], R[7], R[100]
    return d, L, R, heldout_for(seed, users, items, d["row"], d["col"])


def pitch_ops(orc, plan, d, L, R, held, where):
    """recommend, top-N, ranks, both losses and predict of the plan's current factors (= L, R) against the models"""
    users, items, K, row, col, val = d["users"], d["items"], d["feats"], d["row"], d["col"], d["val"]
    assert np.array_equal(plan.recommend(), orc.recommend(orc.Instance(**d), L, R)), where
    mi, ms = model_topn(orc, users, items, row, col, L, R, 32)
    for n in (10, 32):
        it, sc = plan.recommend_topn(n)
        assert_same(it, sc, mi[:, :n], ms[:, :n], (where, n))
    plan.set_heldout(*held)
    got = plan.rank_heldout()
    assert np.array_equal(got, model_ranks(orc, users, items, row, col, L, R, held[0], held[1])), where
    sent = (plan.recommend_info(), plan.recommend_topn_info(), plan.rank_heldout_info())
    if K != 30:
        assert sent[0] >= 0 and sent[1][1] in (1, 2) and sent[2][1] in (1, 2), (where, sent)
    check_loss(plan, L, R, row, col, val, "train", str(where))
    check_loss(plan, L, R, held[0], held[1], held[2], "heldout", str(where))
    B = plan.predict()
    for i in range(users):
        assert_bits(B[i], orc.predict_row(np.ascontiguousarray(L[i]), R), "%s predict row %d" % (where, i))
    return sent


def pitch_run(orc, plan, d, L, R, held, where):
    """the operations on the uploaded factors, four iterations against the oracle, the operations on the iterated factors"""
    plan.upload(L, R)
    sent = pitch_ops(orc, plan, d, L, R, held, (where, "uploaded"))
    plan.iterate(4)
    Lg, Rg = plan.download()
    Lo, Ro = L.copy(), R.copy()
    orc.factorize(orc.Instance(**d), Lo, Ro, iters=4)
    assert np.isfinite(Lo).all() and np.isfinite(Ro).all()
    assert np.array_equal(Lg, Lo) and np.array_equal(Rg, Ro), where
    return sent, pitch_ops(orc, plan, d, Lg, Rg, held, (where, "iterated"))


@pytest.mark.gpu
@pytest.mark.parametrize("padded", [True, False])
def test_pitch_of_the_plans_own_buffers_at_k_60(gpu, orc, padded, monkeypatch):
    """K = 60 is the only matrix-core K whose own rows are padded (480 bytes -> 512): every operation reads rows at pitch 64"""
    capi = gpu
    _env(monkeypatch, "MF_ROW_PITCH", None if padded else "0")
    d, L, R, held = pitch_instance(60, 150, 300, 60)
    plan = capi.Plan(150, 300, 60, d["alpha"], d["row"], d["col"], d["val"])
    assert plan.pitches() == ((64, 64) if padded else (60, 60))
    pitch_run(orc, plan, d, L, R, held, ("own", padded))
    plan.close()


def _pitches(K):
    """K + 2, K rounded up to 16, 2 K: for K = 64 and 256 the second is K itself (a caller-owned buffer with packed rows: no
    padding to check), for K = 30 it equals K + 2 -- 12 of the 14 cases have padding"""
    return sorted({K + 2, (K + 15) // 16 * 16, 2 * K})


def _nan_tensors(rows, pitch):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.full((rows, pitch), float("nan"), dtype=torch.float64, device=dev) for _ in range(2)]


def _padding_untouched(tensors, K, fill_bits, where):
    for g, t in enumerate(tensors):
        a = t.cpu().numpy()
        assert (a[:, K:].view(np.int64) == fill_bits).all(), (where, "generation", g)


@pytest.mark.gpu
@pytest.mark.parametrize("K,pitch", [(K, p) for K in (60, 100, 64, 256, 30) for p in _pitches(K)])
def test_pitch_of_caller_owned_buffers_with_nan_padding(gpu, orc, K, pitch):
    """Both factors in caller-owned buffers filled with NaN: a read of the padding poisons a result, a write to it shows in
    the read-back (both generations, bit for bit)."""
    capi = gpu
    users, items = 150, 300
    d, L, R, held = pitch_instance(K + pitch, users, items, K)
    lb, rb = _nan_tensors(users, pitch), _nan_tensors(items, pitch)
    fill_bits = int(rb[0][0, 0].cpu().numpy().view(np.int64))
    plan = capi.Plan(users, items, K, d["alpha"], d["row"], d["col"], d["val"], items_ext=[t.data_ptr() for t in rb],
                     items_pitch=pitch, users_ext=[t.data_ptr() for t in lb], users_pitch=pitch)
    assert plan.pitches() == (pitch, pitch)
    sent = pitch_run(orc, plan, d, L, R, held, (K, pitch))
    plan.synchronize()
    Lg, Rg = plan.download()
    plan.close()
    if pitch > K:
        _padding_untouched(lb, K, fill_bits, (K, pitch, "L"))
        _padding_untouched(rb, K, fill_bits, (K, pitch, "R"))
    # the iterated factors are in one generation of the caller's tensors
    assert any(np.array_equal(t.cpu().numpy()[:, :K], Rg) for t in rb) and any(np.array_equal(t.cpu().numpy()[:, :K], Lg) for t in lb)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["items", "users"])
def test_pitch_of_one_caller_owned_side_beside_an_own_one(gpu, orc, side):
    capi = gpu
    users, items, K, pitch = 150, 300, 100, 102
    d, L, R, held = pitch_instance(9 + len(side), users, items, K)
    ext = _nan_tensors(items if side == "items" else users, pitch)
    fill_bits = int(ext[0][0, 0].cpu().numpy().view(np.int64))
    kw = {side + "_ext": [t.data_ptr() for t in ext], side + "_pitch": pitch}
    plan = capi.Plan(users, items, K, d["alpha"], d["row"], d["col"], d["val"], **kw)
    own = capi.row_pitch(K)
    assert plan.pitches() == ((own, pitch) if side == "items" else (pitch, own))
    sent = pitch_run(orc, plan, d, L, R, held, (side,))
    plan.synchronize()
    plan.close()
    _padding_untouched(ext, K, fill_bits, (side,))


# ------------------------------------------------------------------------------------------------ D: R beyond 2^31 and 2^32 bytes
def _threads():
    return min(16, os.cpu_count() or 1)


def _random_rows(seed, rows, K):
    """standard-normal rows, every slice from its own seeded stream, filled by a pool of threads: the 2.8e8 .. 5.6e8 draws of
    one R are the largest cost of these tests when one thread draws them"""
    out = np.empty((rows, K))
    cuts = np.linspace(0, rows, 4 * _threads() + 1).astype(np.int64)
    streams = np.random.SeedSequence(seed).spawn(len(cuts) - 1)

    def fill(t):
        np.random.default_rng(streams[t]).standard_normal(out=out[cuts[t]:cuts[t + 1]])

    with ThreadPoolExecutor(_threads()) as pool:
        list(pool.map(fill, range(len(cuts) - 1)))
    return out


def _distinct(rng, lo, hi, n):
    while True:
        x = rng.integers(lo, hi, n)
        if np.unique(x).size == n:
            return x


def _big_r_case(capi, orc, K, items, boundary, expect_32bit_forms, users):
    """`users`: the issue's 256 shrunk until the test costs no more than test_buffers_beyond_2_31_bytes_spot_checks (the
    oracle rows and the numpy models over them grow with users x items; the item count is what the test is about)"""
    t0 = time.perf_counter()
    rng = np.random.default_rng(K + items)
    ldr = capi.row_pitch(K)
    size = items * ldr * 8
    if expect_32bit_forms:
        assert 2 ** 31 < size < 2 ** 32
    else:
        assert size >= 2 ** 32
    jb = boundary // (8 * ldr) + 1                     # every row from jb on starts above the byte offset `boundary`
    assert boundary >= 2 ** 31 and jb + 4000 < items
    L = rng.standard_normal((users, K))
    R = _random_rows(K + items, items, K)
    # winner, second and third place planted: above the boundary for the even users, below it for the odd ones
    planted = np.empty((users, 3), np.int64)
    for u in range(users):
        base = (jb if u % 2 == 0 else 0) + 1000 + 3 * u
        for t, c in enumerate((3.0, 2.5, 2.0)):
            planted[u, t] = base + t
            R[base + t] = c * L[u]
    # ten rated items per user, three of them in the upper part; none of them planted (those lie in [1000, 1768) + {0, jb})
    rated = [np.sort(np.concatenate([_distinct(rng, 2000, jb, 7), _distinct(rng, jb + 2000, items, 3)])) for _ in range(users)]
    row = np.repeat(np.arange(users, dtype=np.int32), 10)
    col = np.concatenate(rated).astype(np.int32)
    val = np.ones(row.shape[0])
    # four held-out entries per user: the second place (above for the even users), two more above, one below, a rated pair
    hrow = np.repeat(np.arange(users, dtype=np.int32), 4)
    hcol = np.stack([np.where(np.arange(users) % 2 == 0, planted[:, 1], jb + 1900 - np.arange(users)),
                     items - 1 - np.arange(users), 500 + np.arange(users), [r[8] for r in rated]], 1).reshape(-1).astype(np.int32)
    assert (hcol.reshape(users, 4)[:, :2] >= jb).all() and (hcol.reshape(users, 4)[:, 2] < jb).all()

    t1 = time.perf_counter()
    plan = _plan(capi, users, items, K, row, col, val, L, R)
    assert plan.pitches()[1] == ldr
    t2 = time.perf_counter()
    best = plan.recommend()
    info1 = plan.recommend_info()
    ti, ts = plan.recommend_topn(5)
    tinfo = plan.recommend_topn_info()
    plan.set_heldout(hrow, hcol, np.ones(hrow.shape[0]))
    ranks = plan.rank_heldout()
    rinfo = plan.rank_heldout_info()
    plan.close()
    t3 = time.perf_counter()
    # top-1: only the two-per-CU form is gated on 32-bit offsets; without it the 128-user matrix-core form runs (64-bit rows)
    assert info1 >= 0
    if expect_32bit_forms:
        assert tinfo[1] in (1, 2) and rinfo[1] in (1, 2) and tinfo[0] >= 0 and rinfo[0] >= 0
    else:
        assert tinfo == (-1, 0) and rinfo == (-1, 0)

    def one(u):      # the models over ONE exact row per user (the row is 9 .. 22 MB: none is kept)
        b = orc.predict_row(np.ascontiguousarray(L[u]), R)
        masked = b.copy()
        masked[rated[u]] = -np.inf                     # _check_recommend_rows' rule: rated items never win, scores are finite
        mi, ms = model_row(b, rated[u], items, 5)
        rk = [rank_of(b, set(rated[u].tolist()), items, int(j)) for j in hcol[4 * u:4 * u + 4]]
        return int(np.argmax(masked)), mi, ms, rk

    with ThreadPoolExecutor(_threads()) as pool:
        res = list(pool.map(one, range(users)))
    print("\nK %d, %d items, %d users: instance %.2f s, plan + upload %.2f s, three passes %.2f s, models %.2f s"
          % (K, items, users, t1 - t0, t2 - t1, t3 - t2, time.perf_counter() - t3))
    want_best = np.array([r[0] for r in res], np.int32)
    assert np.array_equal(want_best[0::2], planted[0::2, 0]) and np.array_equal(want_best[1::2], planted[1::2, 0])
    assert np.array_equal(best, want_best), np.flatnonzero(best != want_best)[:8]
    assert_same(ti, ts, np.stack([r[1] for r in res]), np.stack([r[2] for r in res]), (K, items))
    assert np.array_equal(ti[:, :3], planted)
    want_ranks = np.array([r[3] for r in res], np.int32).reshape(-1)
    assert np.array_equal(ranks, want_ranks), np.flatnonzero(ranks != want_ranks)[:8]
    assert (want_ranks.reshape(users, 4)[:, 3] == -1).all() and (want_ranks.reshape(users, 4)[0::2, 0] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K,items", [(256, 1_100_000), (100, 2_800_000)])
def test_r_between_2_31_and_2_32_bytes_keeps_32_bit_offsets_unsigned(gpu, orc, K, items):
    """The two-per-CU forms address R rows with a 32-bit byte offset: rows above 2^31 bytes hold the planted winners of
    half of the users, so an offset that is sign-extended or wraps names another item"""
    _big_r_case(gpu, orc, K, items, 2 ** 31, True, 64)


@pytest.mark.gpu
def test_r_beyond_2_32_bytes_hands_over_to_the_64_bit_forms(gpu, orc):
    """2.2e6 items x K = 256 are 4.5e9 bytes: top-N and ranks take the exact form for every user, top-1 the 128-user
    matrix-core form; winners planted above 2^32 bytes.

    Cost: 3.27 s on the MI355X beside 2.16 s (+ 1.52 s of set-up) of test_buffers_beyond_2_31_bytes_spot_checks[auto] in the
    same run -- above that yardstick, and not for the users: 1.99 s are the three passes themselves (the exact forms walk
    2.2e6 items of K = 256 with one wave per user / entry, however few there are), 0.27 s the instance, 0.68 s the models of
    32 users.  The item count is what makes R exceed 2^32 bytes and stays."""
    _big_r_case(gpu, orc, 256, 2_200_000, 2 ** 32, False, 32)


# ------------------------------------------------------------------------------------------------ E: power-of-two scaling
PAIRS = [(0, 0), (-540, 300), (300, -540), (-520, 0), (-300, -300), (500, 500), (-537, 537)]


def top1_near_tie_instance():
    """test_mfma_certification_sends_near_ties_to_the_exact_pass's instance"""
    u, i, k = 200, 300, 64
    rng = np.random.default_rng(3)
    L = rng.standard_normal((u, k))
    R = rng.standard_normal((i, k))
    R[200:] = R[:100] * (1 + 2.0 ** -52)
    d = random_instance(2, u, i, k, density=0.05)
    hrow = np.repeat(np.arange(u, dtype=np.int32), 2)
    hcol = np.stack([(np.arange(u) * 3 + 1) % i, (np.arange(u) * 3 + 201) % i], 1).reshape(-1).astype(np.int32)
    return u, i, k, d["row"], d["col"], d["val"], L, R, hrow, hcol


def twin_instance():
    """test_topn_certification_near_ties_and_separated's instance with test_rank.py's held-out entries"""
    users, items, K = 130, 256, 64
    rng = np.random.default_rng(7)
    L = rng.standard_normal((users, K))
    R = rng.standard_normal((items, K))
    R[1::2] = R[0::2] * (1.0 + 2.0 ** -52)
    row = np.repeat(np.arange(users, dtype=np.int32), 2)
    col = (np.arange(2 * users, dtype=np.int32) * 7) % items
    hrow = np.repeat(np.arange(users, dtype=np.int32), 2)
    hcol = np.stack([(np.arange(users) * 2 + 10) % items, (np.arange(users) * 2 + 11) % items], 1).reshape(-1).astype(np.int32)
    return users, items, K, row, col, np.ones(row.shape[0]), L, R, hrow, hcol


INSTANCES = {"top1-near-ties": top1_near_tie_instance, "twins": twin_instance}


def _models(orc, inst, L, R):
    users, items, K, row, col, val, _, _, hrow, hcol = inst
    best = orc.recommend(orc.Instance(1, 0.0, K, users, items, row, col, val), L, R)
    mi, ms = model_topn(orc, users, items, row, col, L, R, 3)
    return best, mi, ms, model_ranks(orc, users, items, row, col, L, R, hrow, hcol)


@pytest.mark.parametrize("a,b", PAIRS)
@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_power_of_two_scaling_leaves_the_reference_answers_alone(orc, name, a, b):
    """The premise of E, on the CPU: L * 2^a and R * 2^b scale every exact score by 2^(a+b) without rounding"""
    inst = INSTANCES[name]()
    users, items, K, row, col, val, L, R, hrow, hcol = inst
    Ls, Rs = np.ldexp(L, a), np.ldexp(R, b)
    assert np.array_equal(np.ldexp(Ls, -a), L) and np.array_equal(np.ldexp(Rs, -b), R)      # the scaling itself is exact
    b0, i0, s0, r0 = _models(orc, inst, L, R)
    b1, i1, s1, r1 = _models(orc, inst, Ls, Rs)
    assert np.array_equal(b1, b0) and np.array_equal(i1, i0) and np.array_equal(r1, r0)
    assert (i0 >= 0).all() and (r0 >= -1).all() and (r0 >= 0).any()
    if abs(a + b) < 900:
        assert_bits(s1, np.ldexp(s0, a + b), "top-3 scores")
        for u in range(users):
            assert_bits(orc.predict_row(np.ascontiguousarray(Ls[u]), Rs), np.ldexp(orc.predict_row(np.ascontiguousarray(L[u]), R), a + b), u)


def true_norm_scaled(X):
    """per row (e, n): the row's norm is n * 2^e, n computed with the row scaled by its largest entry's exponent first
    (a plain sum of K <= 1024 squares of numbers below 1 is within (K + 2) * 2^-53 of the truth)"""
    e = np.frexp(np.abs(X).max(axis=1))[1]
    return e, np.sqrt((np.ldexp(X, -e[:, None]) ** 2).sum(axis=1))


def assert_norms_are_no_underestimate(norm, rmax, L, R, where):
    """each reported norm is non-finite or >= (1 - 2^-40) * the true one: the condition the certification rests on"""
    slack = 1.0 - 2.0 ** -40
    el, nl = true_norm_scaled(L)
    with np.errstate(over="ignore"):
        ok = ~np.isfinite(norm) | (np.ldexp(norm, -el) >= slack * nl)
        assert ok.all(), (where, "norm", np.flatnonzero(~ok)[:8], norm[~ok][:4])
        er, nr = true_norm_scaled(R)
        ok = np.ldexp(np.full(R.shape[0], rmax), -er) >= slack * nr
    assert not np.isfinite(rmax) or ok.all(), (where, "rmax", rmax, np.flatnonzero(~ok)[:8])


def _gpu_run(capi, inst, L, R):
    users, items, K, row, col, val, _, _, hrow, hcol = inst
    plan = capi.Plan(users, items, K, 0.0, row, col, val)
    plan.upload(L, R)
    best = plan.recommend()
    sent = [plan.recommend_info()]
    it, sc = plan.recommend_topn(3)
    sent.append(plan.recommend_topn_info()[0])
    plan.set_heldout(hrow, hcol, np.ones(hrow.shape[0]))
    ranks = plan.rank_heldout()
    sent.append(plan.rank_heldout_info()[0])
    assert plan.recommend_topn_info()[1] in (1, 2) and plan.rank_heldout_info()[1] in (1, 2)
    _, norm, rmax = plan.recommend_filter()
    plan.close()
    return best, it, sc, ranks, sent, norm, rmax


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", PAIRS)
@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_certification_does_not_depend_on_the_magnitude_of_the_factors(gpu, orc, name, a, b):
    """Answers equal the model on the scaled factors; no pass certifies more than it does unscaled; the norms the
    certification uses are never underestimates.

    Measured on the MI355X (exact-pass users of top-1 / users of top-3 / entries of the ranks), unscaled against scaled: see
    DESIGN.md section 8."""
    inst = INSTANCES[name]()
    L, R = inst[6], inst[7]
    Ls, Rs = np.ldexp(L, a), np.ldexp(R, b)
    _, _, _, _, sent0, norm0, rmax0 = _gpu_run(gpu, inst, L, R)
    best, it, sc, ranks, sent, norm, rmax = _gpu_run(gpu, inst, Ls, Rs)
    print("\n%s (%d, %d): exact pass top-1 / top-3 / rank entries: unscaled %s, scaled %s; min norm %g, rmax %g"
          % (name, a, b, sent0, sent, np.min(norm), rmax))
    wb, wi, ws, wr = _models(orc, inst, Ls, Rs)
    assert np.array_equal(best, wb), np.flatnonzero(best != wb)[:8]
    assert_same(it, sc, wi, ws, (name, a, b))
    assert np.array_equal(ranks, wr), np.flatnonzero(ranks != wr)[:8]
    assert min(sent0) > 0, sent0                     # near ties: every pass sends somebody unscaled
    for what, s0, s1 in zip(("top-1 users", "top-N users", "rank entries"), sent0, sent):
        assert s1 >= s0, ("certified more under scaling than unscaled", what, s0, s1)
    assert_norms_are_no_underestimate(norm0, rmax0, L, R, (name, "unscaled"))
    assert_norms_are_no_underestimate(norm, rmax, Ls, Rs, (name, a, b))


def _subnormal_and_zero_instances():
    users, items, K, row, col, val, L, R, hrow, hcol = twin_instance()
    rng = np.random.default_rng(99)
    tiny = 2.0 ** -1074 * rng.integers(1, 2 ** 40, K) * rng.choice([-1.0, 1.0], K)       # all subnormal, signs mixed
    assert (np.abs(tiny) < 2.0 ** -1022).all() and (tiny != 0).all()
    Ls, Rs = L.copy(), R.copy()
    Ls[17] = tiny
    Rs[40] = tiny[::-1]
    Lz = L.copy()
    Lz[17] = 0.0
    Lz[18] = -0.0
    return {"subnormal-rows": (users, items, K, row, col, val, Ls, Rs, hrow, hcol),
            "zero-rows": (users, items, K, row, col, val, Lz, R, hrow, hcol)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["subnormal-rows", "zero-rows"])
def test_subnormal_and_zero_rows_among_ordinary_ones(gpu, orc, name):
    """One all-subnormal user row and one all-subnormal item row; an all-zero user row (every score +-0.0: all ties, the
    lowest index wins).  Answers against the models, the norms sound."""
    inst = _subnormal_and_zero_instances()[name]
    L, R = inst[6], inst[7]
    best, it, sc, ranks, sent, norm, rmax = _gpu_run(gpu, inst, L, R)
    wb, wi, ws, wr = _models(orc, inst, L, R)
    assert np.array_equal(best, wb), np.flatnonzero(best != wb)[:8]
    assert_same(it, sc, wi, ws, name)
    assert np.array_equal(ranks, wr), np.flatnonzero(ranks != wr)[:8]
    assert_norms_are_no_underestimate(norm, rmax, L, R, name)
    if name == "zero-rows":
        rated = _rated_sets(inst[0], inst[3], inst[4])
        for u in (17, 18):
            assert wb[u] == min(set(range(inst[1])) - set(rated[u])) and norm[u] == 0.0
