"""The single-process multi-shard run (mf_backend_run_multi, mf_multi.hip.h) and its peer reduce (peer_allreduce_kernel,
mf_collective.hip.h) against a bit-exact model of their definition in include/matfact_hip.h.

The model is plain numpy over the CPU oracle: the side with more rows ("A": the users, or the items when items > users)
is cut into contiguous blocks balanced by entry count, every shard runs oracle.shard_step on its entries in file order
(shard 0 seeds the replicated factor "B" from the old one, the others from zero) and B_new is the sum of the shards'
partials, left to right in shard order.  Nothing here has a tolerance: every factor comparison is on the uint64 views,
NaN by position (sign and payload of a NaN are free, as everywhere else in this project), so -0.0 and +0.0 differ.

What only this file reaches: the second trip of the reduce's grid-stride loop, its scalar tail (odd element count), empty
slices, slice bounds at shard counts that do not divide the pair count, 16 shards, shards without rows (in both cut
directions), the items-cut form of the entry split at the bit level, and special values through the reduce."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import random_instance
from oracle import oracle as O

MAX_SHARDS = 16                    # mf::kMaxShards, the ABI's limit
ONE_PASS = 2048 * 256 * 2          # doubles of a slice that one trip of the reduce's grid-stride loop covers
NEG_ZERO = np.uint64(0x8000000000000000)


# ------------------------------------------------------------------------------------------------ the model
def cut_items(d):
    """True when the items are cut (roles of (row, L) and (col, R) exchanged); the users are cut when users >= items."""
    return d["items"] > d["users"]


def balance_blocks(counts, ndev):
    """begin[0..ndev] over the keys of the cut side from the per-key entry counts: one cursor that only moves forward"""
    nkeys = len(counts)
    cnt = [0] * (nkeys + 1)
    for k in range(nkeys):
        cnt[k + 1] = cnt[k] + int(counts[k])
    begin = [0] * (ndev + 1)
    u = 0
    for g in range(1, ndev):
        target = cnt[nkeys] * g // ndev
        while u < nkeys and cnt[u] < target:
            u += 1
        begin[g] = u
    begin[ndev] = nkeys
    return begin


def owners(key, begin):
    """the shard whose block [begin[g], begin[g+1]) holds each key; a block without keys owns nothing"""
    return np.searchsorted(np.asarray(begin[1:], np.int64), key, side="right")


def model_run_multi(d, ndev, L0, R0, reverse_sum=False, seed_shard=0, cut=None, partials=None):
    """(L, R, begin) of mf_backend_run_multi with ndev shards.  reverse_sum, seed_shard and cut (blocks other than the
    rule's) exist for the tests that prove the comparison can tell a wrong run from the right one; partials (a list)
    receives every iteration's list of B partials."""
    swap = cut_items(d)
    key, other = (d["col"], d["row"]) if swap else (d["row"], d["col"])
    nkeys, nrows_b = (d["items"], d["users"]) if swap else (d["users"], d["items"])
    K = d["feats"]
    A = np.array(R0 if swap else L0, np.float64, order="C")
    B = np.array(L0 if swap else R0, np.float64, order="C")
    assert A.shape == (nkeys, K) and B.shape == (nrows_b, K)
    begin = balance_blocks(np.bincount(key, minlength=nkeys), ndev) if cut is None else list(cut)
    own = owners(key, begin)
    shard = []
    for g in range(ndev):
        idx = np.flatnonzero(own == g)          # file order inside the shard
        shard.append(tuple(np.ascontiguousarray(a[idx]) for a in (key, other, d["val"])))
    for _ in range(d["iters"]):
        A_new, parts = np.empty_like(A), []
        for g, (k, o, v) in enumerate(shard):
            b0, b1 = begin[g], begin[g + 1]
            blk, P = O.shard_step(b0, b1 - b0, nrows_b, K, k, o, v, d["alpha"], np.ascontiguousarray(A[b0:b1]), B,
                                  g == seed_shard)
            A_new[b0:b1] = blk
            parts.append(P)
        if partials is not None:
            partials.append(parts)
        seq = parts[::-1] if reverse_sum else parts
        with np.errstate(all="ignore"):
            B_new = seq[0]
            for P in seq[1:]:
                B_new = B_new + P                # (((P_0 + P_1) + P_2) + ...), elementwise in float64
        A, B = A_new, B_new
    L, R = (B, A) if swap else (A, B)
    return L, R, begin


def model_best(d, L, R):
    """oracle.recommend on the factors the run RETURNED.  The oracle walks the entries with the reference's cursor, which
    wants them (row, col)-sorted; the rated set does not depend on the file order, so a permuted file is sorted first."""
    order = np.lexsort((d["col"], d["row"]))
    ds = dict(d, row=d["row"][order], col=d["col"][order], val=d["val"][order])
    return O.recommend(O.Instance(**ds), np.ascontiguousarray(L), np.ascontiguousarray(R))


def slice_bounds(nb, ndev):
    """the ndev + 1 bounds of the reduce slices of an nb-element buffer: whole pairs, the odd element to the last shard"""
    return [((nb // 2) * g // ndev) * 2 for g in range(ndev)] + [nb]


def reduce_slice(flat, nb, ndev):
    """(shard, begin, end) of the reduce slice that element `flat` of the nb-element replicated buffer falls in"""
    b = slice_bounds(nb, ndev)
    g = int(np.searchsorted(np.asarray(b[1:], np.int64), flat, side="right"))
    assert 0 <= flat < nb and b[g] <= flat < b[g + 1], (flat, nb, ndev)
    return g, b[g], b[g + 1]


def assert_bits(got, want, what, ndev=None, pitch=None, begin=None):
    """Where `want` holds a NaN, `got` holds a NaN; every other element is the same uint64.  On a mismatch the message
    names the first differing (row, column) and, for the replicated factor (pitch given), the flat element index in the
    padded buffer and the reduce slice it falls in; for the cut factor (begin given) the shard that owns the row."""
    got = np.ascontiguousarray(got, np.float64)
    want = np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape and got.ndim == 2, (what, got.shape, want.shape)
    g, w = got.view(np.uint64), want.view(np.uint64)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (g != w))
    if not bad.any():
        return
    r, c = (int(x[0]) for x in np.nonzero(bad))
    lines = ["%s: %d of %d elements differ in %d rows; first at (row %d, column %d): got %r (%#018x), model %r (%#018x)" % (
        what, int(bad.sum()), bad.size, int(bad.any(axis=1).sum()), r, c, got[r, c], int(g[r, c]), want[r, c], int(w[r, c]))]
    if pitch is not None:
        flat, nb = r * pitch + c, got.shape[0] * pitch
        s, b, e = reduce_slice(flat, nb, ndev)
        lines.append("flat element %d of %d (pitch %d), in the reduce slice of shard %d [%d, %d) of %d shards, trip %d of "
                     "that slice's loop" % (flat, nb, pitch, s, b, e, ndev, (flat - b) // ONE_PASS))
        rr, cc = np.nonzero(bad)
        per = np.bincount(np.searchsorted(np.asarray(slice_bounds(nb, ndev)[1:], np.int64), rr * pitch + cc, side="right"),
                          minlength=ndev)
        lines.append("differing elements per reduce slice: %s" % per.tolist())
    if begin is not None:
        s = int(owners(np.array([r]), begin)[0])
        lines.append("row %d belongs to shard %d, block [%d, %d); blocks %s" % (r, s, begin[s], begin[s + 1], begin))
    raise AssertionError("\n".join(lines))


# ------------------------------------------------------------------------------------------------ fixtures
def permuted(d, seed=3):
    perm = np.random.default_rng(seed).permutation(len(d["row"]))
    return dict(d, row=np.ascontiguousarray(d["row"][perm]), col=np.ascontiguousarray(d["col"][perm]),
                val=np.ascontiguousarray(d["val"][perm]))


def from_mask(mask, feats, iters, alpha, seed):
    """(row, col)-sorted instance with ratings in [1, 5) on the True cells of mask"""
    row, col = np.nonzero(np.asarray(mask, bool))
    val = np.random.default_rng(seed).random(len(row)) * 4 + 1
    return dict(iters=iters, alpha=alpha, feats=feats, users=mask.shape[0], items=mask.shape[1], row=row.astype(np.int32),
                col=col.astype(np.int32), val=val.astype(np.float64))


@functools.lru_cache(maxsize=None)
def main_fixture(side, order):
    """The two shapes of the tolerance tests in test_gpu_parity.py: users cut (empty users, one who rated everything) and
    items cut; sorted by (row, col), or the same file permuted so that it takes the bucketing pass."""
    if side == "users":
        d = random_instance(91, 230, 140, 30, density=0.25, iters=12, alpha=0.002, empty_rows=(3, 100), full_rows=(8,))
    else:
        d = random_instance(17, 24, 900, 20, density=0.3, iters=10, alpha=0.001, empty_rows=(3,))
    assert cut_items(d) == (side == "items")
    return permuted(d) if order == "permuted" else d


def init(d):
    L0, R0 = O.init_factors(d["users"], d["items"], d["feats"])
    return L0, R0


@functools.lru_cache(maxsize=None)
def main_model(side, order, ndev):
    d = main_fixture(side, order)
    out = model_run_multi(d, ndev, *init(d))
    for a in out[:2]:
        a.setflags(write=False)
    return out


def serial(d, L0, R0):
    L, R = L0.copy(), R0.copy()
    O.factorize(O.Instance(**d), L, R)
    return L, R


# ------------------------------------------------------------------------------------------------ the model on the CPU
def test_assert_bits_sees_zero_signs_and_nan_positions():
    a = np.array([[0.0, 1.0, np.nan], [5e-324, np.inf, -2.0]])
    assert_bits(a, a.copy(), "identical")
    other = a.copy()
    other.view(np.uint64)[0, 2] = 0xfff8000000000000          # another NaN: the same class
    assert_bits(other, a, "NaN payloads")
    for r, c, v in ((0, 0, -0.0), (1, 0, 1e-323), (1, 1, -np.inf), (0, 2, 1.0), (0, 1, np.nan), (1, 0, 0.0)):
        b = a.copy()
        b[r, c] = v
        with pytest.raises(AssertionError, match=r"first at \(row %d, column %d\)" % (r, c)):
            assert_bits(b, a, "changed", ndev=3, pitch=4)
    with pytest.raises(AssertionError, match=r"flat element 6 of 8 \(pitch 4\), in the reduce slice of shard 2 \[4, 8\)"):
        assert_bits(np.array([[0.0] * 3, [0.0, 0.0, -0.0]]), np.zeros((2, 3)), "slice", ndev=3, pitch=4)
    with pytest.raises(AssertionError, match=r"row 1 belongs to shard 2, block \[1, 2\)"):
        assert_bits(np.array([[0.0], [1.0]]), np.zeros((2, 1)), "block", begin=[0, 0, 1, 2])
    assert [reduce_slice(e, 3, 5)[0] for e in range(3)] == [4, 4, 4]          # nb = 3: only the last shard has a slice
    assert [reduce_slice(e, 10, 3)[0] for e in range(10)] == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2]


@pytest.mark.parametrize("name", ["users", "items", "users-permuted", "items-permuted", "7x5"])
def test_model_with_one_shard_is_the_serial_program(name):
    if name == "7x5":
        d = random_instance(5, 7, 5, 3, density=0.5, iters=9, alpha=0.01)
    else:
        d = main_fixture(name.split("-")[0], "permuted" if name.endswith("permuted") else "sorted")
    L0, R0 = init(d)
    L, R, begin = model_run_multi(d, 1, L0, R0)
    Ls, Rs = serial(d, L0, R0)
    assert begin == [0, max(d["users"], d["items"])]
    assert_bits(L, Ls, "L")
    assert_bits(R, Rs, "R")
    assert not np.array_equal(L, L0) and not np.array_equal(R, R0)


def heavy_pattern():
    """40 keys, one of which holds more than half of the entries"""
    counts = np.ones(40, np.int64)
    counts[[5, 17]] = 0
    counts[23] = 60
    return counts


@pytest.mark.parametrize("name", ["uniform", "heavy", "empty"])
def test_blocks_tile_the_keys_for_every_shard_count(name):
    counts = {"uniform": np.full(40, 3, np.int64), "heavy": heavy_pattern(), "empty": np.zeros(40, np.int64)}[name]
    key = np.repeat(np.arange(40), counts)
    repeats = 0
    for ndev in range(1, MAX_SHARDS + 1):
        begin = balance_blocks(counts, ndev)
        assert len(begin) == ndev + 1 and begin[0] == 0 and begin[-1] == 40, (ndev, begin)
        assert all(a <= b for a, b in zip(begin, begin[1:])), (ndev, begin)      # no gap, no overlap: [b[g], b[g+1])
        own = owners(key, begin)
        assert ((own >= 0) & (own < ndev)).all()
        for g in range(ndev):
            assert ((key[own == g] >= begin[g]) & (key[own == g] < begin[g + 1])).all(), (ndev, g, begin)
            if begin[g] == begin[g + 1]:
                repeats += 1
                assert (own != g).all()
        assert sum(int((own == g).sum()) for g in range(ndev)) == len(key)
    if name == "heavy":
        # 97 entries, 21 before the heavy key: targets 19, 38, 58, 77 -> the block of the heavy key, then three empty ones
        assert repeats > 0 and balance_blocks(counts, 5) == [0, 21, 24, 24, 24, 40]
    if name == "empty":
        assert balance_blocks(counts, 5) == [0, 0, 0, 0, 0, 40]      # no entries: every key goes to the last shard
    if name == "uniform":
        assert balance_blocks(counts, 4) == [0, 10, 20, 30, 40] and balance_blocks(counts, 3) == [0, 14, 27, 40]


def test_cut_of_the_toy_instance_has_shards_without_rows():
    d = toy_users_cut()
    begin = balance_blocks(np.bincount(d["row"], minlength=7), 5)
    # counts 0 1 5 4 0 1 1, prefix sums 0 0 1 6 10 10 11 12, targets 2 4 7 9
    assert begin == [0, 3, 3, 4, 4, 7], begin


@pytest.mark.parametrize("ndev", [3, 5, 16])
def test_reversed_sum_order_changes_bits_on_the_main_fixture(ndev):
    """The GPU comparison can tell the shard order of the sum from its reverse only if the two differ on the fixture."""
    for side in ("users", "items"):
        d = main_fixture(side, "sorted")
        L, R, _ = main_model(side, "sorted", ndev)
        Lr, Rr, _ = model_run_multi(d, ndev, *init(d), reverse_sum=True)
        changed = int((L.view(np.uint64) != Lr.view(np.uint64)).sum() + (R.view(np.uint64) != Rr.view(np.uint64)).sum())
        print("%s cut, %d shards: reversed sum order changes %d of %d factor elements" % (side, ndev, changed, L.size + R.size))
        assert changed > 0, "the fixture is too small: summing the %d partials in reversed order changes no bit" % ndev
        # and the model stays the serial program up to the re-association of that sum
        Ls, Rs = serial(d, *init(d))
        assert np.abs(L - Ls).max() < 1e-9 and np.abs(R - Rs).max() < 1e-9
        assert not np.array_equal(L, Ls) or not np.array_equal(R, Rs)


def test_seeding_shard_and_cut_are_observable_with_two_shards():
    """With two shards the sum is commutative; which shard seeds is still visible (x + 0 against 0 + x differ once the
    partials are rounded sums), and so is a cut moved by one row."""
    d = main_fixture("users", "sorted")
    L, R, begin = main_model("users", "sorted", 2)
    L1, R1, _ = model_run_multi(d, 2, *init(d), seed_shard=1)
    assert not np.array_equal(R, R1) or not np.array_equal(L, L1)
    L2, R2, _ = model_run_multi(d, 2, *init(d), cut=[0, begin[1] + 1, begin[2]])
    assert not np.array_equal(R, R2) or not np.array_equal(L, L2)


# ------------------------------------------------------------------------------------------------ the GPU against the model
def run_gpu(capi, d, ndev, L0, R0):
    L, R = np.array(L0, np.float64, order="C"), np.array(R0, np.float64, order="C")
    inst = capi.Instance(d["iters"], d["alpha"], d["feats"], d["users"], d["items"], d["row"], d["col"], d["val"])
    best = capi.backend_run_multi(inst, L, R, [0] * ndev)
    return L, R, best


def compare(capi, d, ndev, got, model, tag):
    L, R, best = got
    Lm, Rm, begin = model
    swap, pitch = cut_items(d), capi.row_pitch(d["feats"])
    assert_bits(L, Lm, "%s: L" % (tag,), ndev, pitch if swap else None, None if swap else begin)
    assert_bits(R, Rm, "%s: R" % (tag,), ndev, None if swap else pitch, begin if swap else None)
    mb = model_best(d, L, R)
    assert np.array_equal(best, mb), (tag, "best", np.flatnonzero(best != mb)[:8], best[best != mb][:8], mb[best != mb][:8])


def check(capi, monkeypatch, d, ndev, L0=None, R0=None, model=None, tag="", threadings=(None, "0")):
    """mf_backend_run_multi([0] * ndev) against the model at MF_MULTI_THREADS default and =0, and the two against each other"""
    if L0 is None:
        L0, R0 = init(d)
    if model is None:
        model = model_run_multi(d, ndev, L0, R0)
    res = []
    for thr in threadings:
        if thr is None:
            monkeypatch.delenv("MF_MULTI_THREADS", raising=False)
        else:
            monkeypatch.setenv("MF_MULTI_THREADS", thr)
        got = run_gpu(capi, d, ndev, L0, R0)
        t = capi.multi_last_timing()
        assert t["shards"] == ndev and t["reducer"] == "peer", t
        if ndev > 1:
            assert t["host_threads"] == (ndev if thr is None else 1), t
        compare(capi, d, ndev, got, model, (tag, ndev, "threads" if thr is None else "one thread"))
        res.append(got)
    for other in res[1:]:
        assert_bits(other[0], res[0][0], "%s: L, one thread against threads" % (tag,))
        assert_bits(other[1], res[0][1], "%s: R, one thread against threads" % (tag,))
        assert np.array_equal(other[2], res[0][2])
    return res[0], model


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["sorted", "permuted"])
@pytest.mark.parametrize("ndev", [2, 3, 5, 7, 16])
@pytest.mark.parametrize("side", ["users", "items"])
def test_main_fixture_bit_for_bit(gpu, monkeypatch, side, ndev, order):
    """Both cut directions, shard counts that do and do not divide the pair count of the replicated buffer, all 16 lanes
    of the unrolled reduce, slices of the caller's array and the bucketing pass (the model sums in the permuted order)."""
    d = main_fixture(side, order)
    check(gpu, monkeypatch, d, ndev, model=main_model(side, order, ndev), tag="%s cut, %s" % (side, order))
    # sorted by the cut key -> the shards are slices of the caller's array; a (row, col)-sorted file is not sorted by column
    assert gpu.multi_last_timing()["sliced"] == (order == "sorted" and side == "users")


@pytest.mark.gpu
@pytest.mark.parametrize("ndev", [2, 3])
@pytest.mark.parametrize("shape", [(9, 7, 3), (12, 5, 7), (5, 8, 7)])
def test_scalar_tail_of_the_reduce(gpu, monkeypatch, shape, ndev):
    """Odd K keeps the pitch at K, an odd number of replicated rows then makes the element count odd: the last shard's
    slice ends in one element that no pair covers.  The last element must get a non-zero partial from a shard other than 0,
    or a skipped tail (shard 0's partial left in place) would go unseen."""
    U, I, K = shape
    mask = np.random.default_rng(U * 100 + I).random((U, I)) < 0.6
    mask[-1, :] = True                      # a user who rated everything: best = -1; the last item gets a late entry
    mask[:, -1] = True
    d = from_mask(mask, K, 7, 0.01, 11)
    rows_b = min(U, I)
    assert (rows_b * gpu.row_pitch(K)) % 2 == 1, (rows_b, gpu.row_pitch(K))
    parts = []
    L0, R0 = init(d)
    model = model_run_multi(d, ndev, L0, R0, partials=parts)
    for it in parts:
        assert any(P[-1, -1] != 0.0 for P in it[1:]), "no shard but 0 contributes to the last element"
    (L, R, best), _ = check(gpu, monkeypatch, d, ndev, L0, R0, model, tag="tail %s" % (shape,))
    assert best[-1] == -1


def toy_users_cut():
    """7 x 5: user 2 rated everything, user 3 four items, users 0 and 4 nothing"""
    mask = np.zeros((7, 5), bool)
    mask[1, 2] = mask[5, 0] = mask[6, 4] = True
    mask[2, :] = True
    mask[3, 1:] = True
    return from_mask(mask, 3, 8, 0.01, 21)


def toy_items_cut():
    """5 x 9: item 4 rated by everybody, three more entries; items 1, 2, 3, 5, 6 without entries"""
    mask = np.zeros((5, 9), bool)
    mask[:, 4] = True
    mask[0, 0] = mask[3, 7] = mask[2, 8] = True
    return from_mask(mask, 3, 8, 0.01, 22)


@pytest.mark.gpu
@pytest.mark.parametrize("ndev", [5, 16])
@pytest.mark.parametrize("toy", ["users", "items"])
def test_shards_without_rows(gpu, monkeypatch, toy, ndev):
    """A few heavy rows hold the entries: some blocks are empty.  Their plans have user_count = 0 at user_begin > 0, sweep,
    take part in the reduce and are asked for recommendations; with the items cut, the user blocks of the recommendation
    pass have empty members too."""
    d = toy_users_cut() if toy == "users" else toy_items_cut()
    assert cut_items(d) == (toy == "items")
    L0, R0 = init(d)
    model = model_run_multi(d, ndev, L0, R0)
    begin = model[2]
    assert len(set(begin)) < len(begin), "no empty shard: %s" % begin
    assert any(begin[g] == begin[g + 1] and begin[g] > 0 for g in range(ndev)), begin
    if toy == "items":
        ub = balance_blocks(np.bincount(d["row"], minlength=d["users"]), ndev)
        assert ndev < 16 or len(set(ub)) < len(ub), ub
    (L, R, best), _ = check(gpu, monkeypatch, d, ndev, L0, R0, model, tag="toy %s" % toy)
    if toy == "users":
        assert best[2] == -1 and (np.delete(best, 2) >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one-row-K3-5-shards", "two-rows-K2-16-shards"])
def test_empty_slices_of_the_reduce(gpu, monkeypatch, case):
    """Fewer element pairs than shards: the leading shards own no slice and launch nothing; with one row of K = 3 the last
    shard takes the only pair and the tail."""
    if case.startswith("one"):
        mask = np.ones((6, 1), bool)
        mask[3, 0] = False
        d, ndev = from_mask(mask, 3, 6, 0.01, 31), 5
    else:
        mask = np.random.default_rng(32).random((20, 2)) < 0.7
        d, ndev = from_mask(mask, 2, 6, 0.01, 32), 16
    nb = d["items"] * gpu.row_pitch(d["feats"])
    assert nb // 2 < ndev and (nb % 2 == 1) == case.startswith("one"), nb
    slices = {reduce_slice(e, nb, ndev)[0] for e in range(nb)}
    assert slices == ({ndev - 1} if case.startswith("one") else slices) and len(slices) < ndev
    (L, R, best), _ = check(gpu, monkeypatch, d, ndev, tag=case)
    if case.startswith("one"):
        assert list(best) == [-1, -1, -1, 0, -1, -1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["no-entries", "no-iterations", "square", "one-more-item"])
def test_degenerate_runs_and_the_switch_of_the_cut_side(gpu, monkeypatch, case):
    if case == "no-entries":
        d = from_mask(np.zeros((6, 4), bool), 3, 4, 0.01, 41)
    elif case == "no-iterations":
        d = dict(random_instance(42, 9, 6, 4, density=0.5), iters=0)
    else:
        U, I = (6, 6) if case == "square" else (6, 7)
        mask = np.random.default_rng(43).random((U, I)) < 0.5
        mask[4, :] = True                    # rated everything: best = -1
        d = from_mask(mask, 4, 6, 0.01, 43)
    L0, R0 = init(d)
    (L, R, best), model = check(gpu, monkeypatch, d, 3, L0, R0, tag=case)
    if case in ("no-entries", "no-iterations"):
        assert_bits(L, L0, "L untouched")
        assert_bits(R, R0, "R untouched")
    if case == "no-entries":
        assert model[2] == [0, 0, 0, 6]
    if case in ("square", "one-more-item"):
        # users == items cuts the users (a (row, col)-sorted file is then sliced), one more item cuts the items
        assert cut_items(d) == (case == "one-more-item")
        assert gpu.multi_last_timing()["sliced"] == (case == "square")
        assert len(model[2]) == 4 and model[2][-1] == (7 if case == "one-more-item" else 6)
        assert best[4] == -1


def grid_stride_instance(gpu):
    """users = items = N with 4 entries per user at the column offsets 0, N/4, N/2, 3N/4 (mod N): the cut falls at N/2
    exactly and each half of the users touches every item.  K = 1000 keeps N, and with it the U * I * K products of the
    recommendation model, small: what the reduce sees is only the element count N * pitch."""
    K = 1000
    pitch = gpu.row_pitch(K)
    N = 4 * (-(-(2 * ONE_PASS + 2) // (4 * pitch)) + 1)
    u = np.arange(N)
    col = np.sort((u[:, None] + np.array([0, N // 4, N // 2, 3 * N // 4])[None, :]) % N, axis=1)
    row = np.repeat(u, 4)
    val = np.random.default_rng(51).random(4 * N) * 4 + 1
    return dict(iters=2, alpha=1e-4, feats=K, users=N, items=N, row=row.astype(np.int32),
                col=col.reshape(-1).astype(np.int32), val=val), pitch


@pytest.mark.gpu
def test_second_trip_of_the_grid_stride_loop(gpu, monkeypatch):
    """The reduce's grid is capped at 2048 blocks of 256 pairs: a slice above 1 048 576 doubles takes a second trip through
    the loop (at cfg4 on 8 GPUs every slice does).  Two shards, every item with an entry in both: an element the loop
    skipped would keep shard 0's partial and differ from the model."""
    d, pitch = grid_stride_instance(gpu)
    N = d["items"]
    nb = N * pitch
    lo, hi = ((nb // 2) * 1 // 2) * 2, nb
    assert lo > ONE_PASS and hi - lo > ONE_PASS, (nb, lo, hi)
    parts = []
    L0, R0 = init(d)
    model = model_run_multi(d, 2, L0, R0, partials=parts)
    begin = model[2]
    assert begin == [0, N // 2, N]
    for g in range(2):
        in_g = (d["row"] >= begin[g]) & (d["row"] < begin[g + 1])
        assert len(np.unique(d["col"][in_g])) == N, "an item has no entry in shard %d" % g
    for it in parts:
        assert (it[1] != 0.0).all(axis=1).all() and (it[0] != model[1]).any(axis=1).all()
    check(gpu, monkeypatch, d, 2, L0, R0, model, tag="grid-stride", threadings=(None,))


# ------------------------------------------------------------------------------------------------ special values through the reduce
def special_instance():
    """12 x 8, K = 4, three shards of four users; item 5 has no entry; every other item is rated in every shard"""
    mask = np.random.default_rng(61).random((12, 8)) < 0.5
    mask[[0, 4, 8], :] = True
    mask[:, 5] = False
    d = from_mask(mask, 4, 2, 0.01, 61)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("ndev", [1, 2, 3])
def test_negative_zero_in_the_replicated_factor(gpu, monkeypatch, ndev):
    """A row of the replicated factor without entries: shard 0 carries the old value, every other shard +0.0, and
    (-0.0) + 0.0 = +0.0.  One shard (MF_MULTI_FORCE=1: the sharded path) adds nothing and keeps the sign."""
    d = special_instance()
    L0, R0 = init(d)
    R0[5, 1] = -0.0
    R0[5, 3] = -0.0
    model = model_run_multi(d, ndev, L0, R0)
    want = NEG_ZERO if ndev == 1 else np.uint64(0)
    assert (model[1][5, [1, 3]].view(np.uint64) == want).all() and np.array_equal(model[1][5, [0, 2]], R0[5, [0, 2]])
    monkeypatch.setenv("MF_MULTI_FORCE", "1")
    (L, R, best), _ = check(gpu, monkeypatch, d, ndev, L0, R0, model, tag="-0.0")
    assert (R[5, [1, 3]].view(np.uint64) == want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["inf-minus-inf", "nan-in-the-last-shard", "subnormal"])
def test_special_values_through_the_reduce(gpu, monkeypatch, case):
    d = special_instance()
    d = dict(d, val=d["val"].copy())
    L0, R0 = init(d)
    begin = balance_blocks(np.bincount(d["row"], minlength=12), 3)
    own = owners(d["row"], begin)
    assert all((own == g).any() for g in range(3)), begin
    parts = []
    if case == "inf-minus-inf":
        # +inf rating in shard 1, -inf rating in shard 2, both of item 2: the partials are +inf and -inf, their sum NaN
        d["val"][np.flatnonzero((own == 1) & (d["col"] == 2))[0]] = np.inf
        d["val"][np.flatnonzero((own == 2) & (d["col"] == 2))[0]] = -np.inf
    elif case == "nan-in-the-last-shard":
        d["val"][np.flatnonzero((own == 2) & (d["col"] == 6))[-1]] = np.nan
    else:
        # R below 2^-1022, ratings of ~1e-308 and L of ~0.1: errors, products and the shards' partial sums are subnormal
        R0 = R0 * 1e-309
        d["val"] = d["val"] * 1e-308
    model = model_run_multi(d, 3, L0, R0, partials=parts)
    first = parts[0]
    if case == "inf-minus-inf":
        assert (first[1][2] == np.inf).all() and (first[2][2] == -np.inf).all() and np.isfinite(first[0]).all()
        assert np.isnan(model[1][2]).all() and np.isfinite(model[1][5]).all()
    elif case == "nan-in-the-last-shard":
        assert np.isnan(first[2][6]).all() and not np.isnan(first[0]).any() and not np.isnan(first[1]).any()
        assert np.isnan(model[1][6]).all() and np.isfinite(model[1][5]).all()
    else:
        tiny = np.finfo(np.float64).tiny
        for P in first[1:]:
            rated = np.delete(P, 5, axis=0)
            assert ((np.abs(rated) < tiny) & (rated != 0.0)).all()
        assert ((np.abs(model[1]) < tiny) & (model[1] != 0.0)).all() and (model[1] != R0)[[0, 1, 2, 3, 4, 6, 7]].all()
    check(gpu, monkeypatch, d, 3, L0, R0, model, tag=case)


# ------------------------------------------------------------------------------------------------ recommendations follow the returned factors
def near_tie_instance():
    """Items 0 and 1 are twins: rated 5.0 by the same users (everything else is rated about 1), with initial rows one ulp
    apart in two columns.  Their scores for the users who rated neither end within an ulp or two of each other (or equal:
    then the lower index wins), the sharded sum moves them by as much, and which twin wins is decided by the factors the
    run returned.  The seed is one at which the CPU model shows that; the test below holds it to it."""
    rng = np.random.default_rng(76)
    U, I, K = 60, 40, 6
    mask = rng.random((U, I)) < 0.3
    raters = rng.random(U) < 0.5
    mask[:, 0] = mask[:, 1] = raters
    d = from_mask(mask, K, 6, 0.004, 76)
    d["val"] = np.where(d["col"] < 2, 5.0, d["val"] * 0.25)
    L0, R0 = init(d)
    R0[1] = R0[0]
    for k in rng.choice(K, 2, replace=False):
        R0[1, k] = np.nextafter(R0[0, k], rng.choice([0.0, 1.0]))
    return d, L0, R0


def test_near_tie_fixture_separates_the_sharded_factors_from_the_serial_ones():
    d, L0, R0 = near_tie_instance()
    Ls, Rs = serial(d, L0, R0)
    bs = model_best(d, Ls, Rs)
    last_bit = 0
    for ndev in (3, 5):
        L, R, _ = model_run_multi(d, ndev, L0, R0)
        b = model_best(d, L, R)
        twins = np.flatnonzero((b >= 0) & (b < 2))
        s = np.array([O.predict_row(L[i], R)[:2] for i in twins])
        close = (s[:, 0] != s[:, 1]) & (np.abs(s[:, 0] - s[:, 1]) <= 2 * np.spacing(np.abs(s[:, 0])))
        flipped = int((b != bs).sum())
        print("near tie, %d shards: %d users pick a twin, the twins' scores differ by 1 or 2 ulp for %d of them, %d picks "
              "differ from those of the serial factors" % (ndev, len(twins), int(close.sum()), flipped))
        assert flipped > 0, "the serial factors give the same picks: the fixture cannot tell whose factors were ranked"
        last_bit += int(close.sum())
    assert last_bit > 0, "the twins' scores are nowhere an ulp or two apart"


@pytest.mark.gpu
@pytest.mark.parametrize("ndev", [3, 5])
def test_near_tie_follows_the_returned_factors(gpu, monkeypatch, ndev):
    d, L0, R0 = near_tie_instance()
    check(gpu, monkeypatch, d, ndev, L0, R0, tag="near tie")


# ------------------------------------------------------------------------------------------------ argument edges
def raw_run_multi(capi, d, ndev, L, R):
    inst = capi.Instance(d["iters"], d["alpha"], d["feats"], d["users"], d["items"], d["row"], d["col"], d["val"])
    p, keep = capi._problem(inst)
    best = np.full(d["users"], -7, np.int32)
    dev = np.zeros(max(ndev, 1), np.int32)
    return capi.hip().mf_backend_run_multi(C.byref(p), L, R, best, dev, ndev), best


def bad_entry_instances():
    """an out-of-range row or column in the first and in the last entry, of a sorted file and of an unsorted one"""
    base = random_instance(81, 9, 6, 3, density=0.5, iters=3, alpha=0.01)
    out = []
    for order in ("sorted", "permuted"):
        d0 = permuted(base, 9) if order == "permuted" else base
        for pos in (0, -1):
            for field, value in (("row", 9), ("row", -1), ("col", 6), ("col", -1)):
                d = dict(d0, **{field: d0[field].copy()})
                d[field][pos] = value
                out.append(((order, pos, field, value), d))
    return base, out


def test_argument_edges_are_refused_before_any_hip_call(capi):
    """Shard counts outside 1..16 and entries outside the matrix give MF_ERR_ARGUMENT from the host checks alone: the same
    answer on a machine without a GPU (where the first HIP call would answer MF_ERR_NO_DEVICE), the factors untouched."""
    base, bad = bad_entry_instances()
    L0, R0 = init(base)
    L, R = L0.copy(), R0.copy()
    for ndev in (0, 17, -1):
        assert raw_run_multi(capi, base, ndev, L, R)[0] == capi.MF_ERR_ARGUMENT, ndev
    for ndev in (2, 3, 16):
        for where, d in bad:
            rc, best = raw_run_multi(capi, d, ndev, L, R)
            assert rc == capi.MF_ERR_ARGUMENT and (best == -7).all(), (ndev, where, rc)
    assert_bits(L, L0, "L after refused calls")
    assert_bits(R, R0, "R after refused calls")


@pytest.mark.gpu
def test_good_call_after_refused_calls_gives_the_model(gpu, monkeypatch):
    base, bad = bad_entry_instances()
    L0, R0 = init(base)
    L, R = L0.copy(), R0.copy()
    for ndev in (0, 17):
        assert raw_run_multi(gpu, base, ndev, L, R)[0] == gpu.MF_ERR_ARGUMENT
    for where, d in bad:
        assert raw_run_multi(gpu, d, 3, L, R)[0] == gpu.MF_ERR_ARGUMENT, where
    assert_bits(L, L0, "L after refused calls")
    assert_bits(R, R0, "R after refused calls")
    check(gpu, monkeypatch, base, 3, L0, R0, tag="after refused calls")
    check(gpu, monkeypatch, permuted(base, 9), 3, L0, R0, tag="after refused calls, permuted")
