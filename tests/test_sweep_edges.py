"""The two factor sweeps on special values and at their launch-size edges.

Every other sweep test feeds init_factors (positive, uniform in [0, 1/K)), ratings 1..5 and a small alpha, and compares with
np.array_equal -- which calls -0.0 and +0.0 equal and any result holding a NaN different.  Here:

A  six value classes (signed, wide exponent range, signed zeros, subnormal users / items, inf and NaN) go through every
   sweep form the library ships, each forced with the documented switches and confirmed through Plan.describe() -- every
   instance of the kernel tables at both ends of its range of K, up to K = 4096, the largest the library accepts
   (WIDE_FORMS; tests/test_wide_k.py checks the table against mf_plan.hip.h);
B  launches just above 262144 rows (where the plain accumulate form replaces the pipelined one) and just above 2^20 rows
   (where the row loop of a workgroup makes a second trip);
C  the oracle is pinned to the reference's own results on signed ratings and on runs that diverge to inf and NaN.

The comparison is assert_same_bits: NaN in exactly the same positions (a GPU does not produce x86's 0xfff8000000000000,
so NaN is compared as a class) and every other element equal as uint64 -- the sign of zero, infinities and subnormals
count.  Expected values are the CPU oracle's (orc.tile_step / orc.factorize) on the same arrays."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, to_text
from test_loss import model_p, model_rows, model_total

sys.path.insert(0, GOLDEN)
import make_golden  # noqa: E402  (special_instance: the instances of reference_special.npz, rebuilt from their seeds)

gpu = pytest.mark.gpu

SWITCHES = ("MF_ITER_MODE", "MF_SWEEP_IMPL", "MF_SWEEP_SKEW", "MF_SWEEP_LONG", "MF_SWEEP_NCH", "MF_SWEEP_DB", "MF_SWEEP_PAIR",
            "MF_ES_SW", "MF_OS_DPP", "MF_ROW_PITCH", "MF_RESIDENT", "MF_GRAPH", "MF_GRAPH_MAX", "MF_BUILD")


# ------------------------------------------------------------------------------------------------ the comparison
def assert_same_bits(got, expected, where):
    """NaN sits in exactly the same positions; every other element is equal as uint64."""
    got = np.ascontiguousarray(got, np.float64)
    expected = np.ascontiguousarray(expected, np.float64)
    assert got.shape == expected.shape, (where, got.shape, expected.shape)
    g, e = got.view(np.uint64), expected.view(np.uint64)
    if np.array_equal(g, e):
        return
    gn, en = np.isnan(got), np.isnan(expected)
    bad = (gn != en) | (~gn & ~en & (g != e))
    if not bad.any():
        return
    bad2, g2, e2 = (x.reshape(got.shape[0] if got.ndim else 1, -1) for x in (bad, g, e))
    rows = np.flatnonzero(bad2.any(axis=1))
    lines = ["%s: %d of %d elements differ in %d of %d rows (NaN compared as a class, everything else by its bits); first rows %s"
             % (where, int(bad.sum()), bad.size, len(rows), bad2.shape[0], rows[:12].tolist())]
    for r in rows[:4]:
        cols = np.flatnonzero(bad2[r])
        lines.append("  row %d, %d columns, first %s" % (r, len(cols), cols[:8].tolist()))
        for c in cols[:4]:
            lines.append("    [%d, %d] got 0x%016x (%r)  expected 0x%016x (%r)"
                         % (r, c, int(g2[r, c]), float(g2[r, c:c + 1].view(np.float64)[0]), int(e2[r, c]),
                            float(e2[r, c:c + 1].view(np.float64)[0])))
    raise AssertionError("\n".join(lines))


def is_negzero(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64) == np.uint64(0x8000000000000000)


def is_subnormal(x):
    a = np.abs(x)
    return (a > 0) & (a < 2.0 ** -1022)


def test_assert_same_bits_sees_what_array_equal_does_not():
    a = np.array([[0.0, 1.0, np.nan], [5e-324, np.inf, -2.0]])
    assert_same_bits(a, a.copy(), "identical")
    other_nan = a.copy()
    other_nan.view(np.uint64)[0, 2] = 0xfff8000000000000          # x86's NaN against numpy's: the same class
    assert other_nan.view(np.uint64)[0, 2] != a.view(np.uint64)[0, 2]
    assert_same_bits(other_nan, a, "NaN payloads")
    for r, c, v in ((0, 0, -0.0), (1, 0, 1e-323), (1, 1, -np.inf), (0, 2, 1.0), (0, 1, np.nan), (1, 0, 0.0)):
        b = a.copy()
        b[r, c] = v
        with pytest.raises(AssertionError) as err:
            assert_same_bits(b, a, "planted")
        assert "[%d, %d] got 0x" % (r, c) in str(err.value) and "1 of 6 elements differ" in str(err.value), str(err.value)
    assert_same_bits(np.array([1.0, np.nan]), np.array([1.0, np.nan]), "1-D")
    with pytest.raises(AssertionError):
        assert_same_bits(np.array([1.0, -0.0]), np.array([1.0, 0.0]), "1-D")


# ------------------------------------------------------------------------------------------------ sparsity patterns
class Pattern:
    def __init__(self, name, users, items, row, col, planted_users=(), planted_items=()):
        order = np.lexsort((col, row))                      # file order: by user, then item
        self.name, self.users, self.items = name, int(users), int(items)
        self.row = np.ascontiguousarray(np.asarray(row)[order], np.int32)
        self.col = np.ascontiguousarray(np.asarray(col)[order], np.int32)
        self.planted_users, self.planted_items = list(planted_users), list(planted_items)
        self.ulen = np.bincount(self.row, minlength=self.users)
        self.ilen = np.bincount(self.col, minlength=self.items)

    @property
    def nnz(self):
        return len(self.row)

    def by_item(self):
        """Stable order of the entries by item (within an item: by user, the file order)."""
        if not hasattr(self, "_by_item"):
            self._by_item = np.argsort(self.col, kind="stable")
        return self._by_item


PLANTED = 12


def _plant(name, users, items, row, col, seed, first_user=0, items_below=None):
    """PLANTED more users and PLANTED more items with one or two entries each (against the original rows, users from
    first_user on, items below items_below): the short rows on which all products of a sum can be -0.0 and on which the
    non-finite plants sit."""
    rng = np.random.default_rng(seed)
    rows, cols = [np.asarray(row, np.int64)], [np.asarray(col, np.int64)]
    for t in range(PLANTED):
        n = 1 + t % 2
        rows.append(np.full(n, users + t))
        cols.append(np.sort(rng.choice(items if items_below is None else items_below, n, replace=False)))
        cols.append(np.full(n, items + t))
        rows.append(np.sort(rng.choice(np.arange(first_user, users), n, replace=False)))
    return Pattern(name, users + PLANTED, items + PLANTED, np.concatenate(rows), np.concatenate(cols),
                   range(users, users + PLANTED), range(items, items + PLANTED))


@functools.lru_cache(maxsize=None)
def pattern(name):
    if name == "pair":
        # test_wave_pair_sweep_bit_exact: empty rows, one-entry rows, rows of exactly one / two chunks +- 1, a few long rows
        U, I = 700, 90
        rng = np.random.default_rng(900)
        lens = rng.integers(0, 12, U)
        lens[:40] = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 5, 4, 3, 1, 90, 89, 88, 47, 48, 49, 0, 0, 1, 1, 2, 2, 31, 33,
                     90, 90, 77, 76, 75, 20, 21, 22, 23, 24]
        row = np.repeat(np.arange(U), lens)
        col = np.concatenate([np.sort(rng.choice(I, int(n), replace=False)) for n in lens if n])
        return _plant(name, U, I, row, col, 901, first_user=40)
    if name == "long-items":
        # test_ordered_sums_every_depth_class_with_and_without_seed: item rows of 20 ... 2600 entries
        U, I = 2600, 48
        rng = np.random.default_rng(1000)
        lens = np.unique(np.concatenate([[U, U - 1, 2049, 1040, 1025, 777, 512, 511, 300, 129, 128, 127, 65, 33, 20],
                                         rng.integers(20, U, 12)]))[::-1]
        rows, cols = [], []
        for j, n in enumerate(lens[:I]):
            r = np.sort(rng.choice(U, int(n), replace=False))
            rows.append(r)
            cols.append(np.full(len(r), j))
        I = len(rows)
        return _plant(name, U, I, np.concatenate(rows), np.concatenate(cols), 1001)
    if name == "skewed":
        # test_row_cooperative_sweep_bit_exact: 150 x 700, ten users with ~630 ratings, five items rated by everybody
        rng = np.random.default_rng(500)
        mask = rng.random((150, 700)) < 0.08
        mask[:10, :] = rng.random((10, 700)) < 0.9
        mask[:, :5] = True
        mask[5, :] = False
        row, col = np.nonzero(mask)
        return _plant(name, 150, 700, row, col, 501)
    if name == "wide":
        # the rows of K up to 4096 (a factor row is 32 KiB there): the block-diagonal [[A, 0], [0, A^T]], A = 38 x 65 with rows
        # of WIDE_LENS entries -- users 0..37 and items 65..102 have exactly those lengths (the planted rows stay off them):
        # n - 1, n, n + 1, 2n, 2n + 1 of every chunk size these plans use (4, 5, 12, 16), about 1600 entries in all
        rng = np.random.default_rng(1100)
        na, ma = len(WIDE_LENS), 65
        arow = np.repeat(np.arange(na), WIDE_LENS)
        acol = np.concatenate([np.sort(rng.choice(ma, int(n), replace=False)) for n in WIDE_LENS if n])
        row = np.concatenate([arow, na + acol])
        col = np.concatenate([acol, ma + arow])
        return _plant(name, na + ma, ma + na, row, col, 1101, first_user=na, items_below=ma)
    raise KeyError(name)


WIDE_LENS = list(range(35)) + [63, 64, 65]


def test_patterns_are_the_ones_the_forms_need():
    p = pattern("pair")
    assert (p.users, p.items) == (700 + PLANTED, 90 + PLANTED) and p.nnz >= 4096      # (errors + streams: >= 4096 entries)
    assert p.ulen[:12].tolist() == [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65] and p.ulen[16] == 90
    assert sorted(set(p.ulen[p.planted_users])) == [1, 2] and sorted(set(p.ilen[p.planted_items])) == [1, 2]
    q = pattern("long-items")
    assert q.ilen.max() >= 2600 and (q.ilen[:q.items - PLANTED] >= 20).all() and sorted(set(q.ilen[q.planted_items])) == [1, 2]
    s = pattern("skewed")
    assert (s.ulen[:10] > 500).sum() >= 9 and s.ulen[5] == 0 and (s.ilen[:5] >= 149).all()
    w = pattern("wide")
    assert (w.users, w.items) == (103 + PLANTED, 103 + PLANTED) and 1500 <= w.nnz <= 1700
    assert w.ulen[:38].tolist() == WIDE_LENS and w.ilen[65:103].tolist() == WIDE_LENS      # both sides, every length
    for n in (4, 5, 12, 16):                                                               # the chunk sizes of the wide plans
        assert {n - 1, n, n + 1, 2 * n, 2 * n + 1} <= set(WIDE_LENS), n
    assert sorted(set(w.ulen[w.planted_users])) == [1, 2] and sorted(set(w.ilen[w.planted_items])) == [1, 2]
    assert not ((w.row < 38) & (w.col >= 65)).any() and not ((w.row >= 38) & (w.row < 103) & (w.col < 65)).any()   # block-diagonal
    for x in (p, q, s, w):
        key =x.row.astype(np.int64) * x.items + x.col
        assert (np.diff(key) > 0).all(), x.name                                       # sorted, no duplicate entry


# ------------------------------------------------------------------------------------------------ value classes
def seq_dot(L, R, row, col):
    """dot(L[row], R[col]) per entry as the serial loop forms it (k ascending from +0.0, multiply and add apart)."""
    with np.errstate(all="ignore"):
        return model_p(L, R, row, col)


def _signed_ratings(rng, n):
    val = rng.integers(-10, 11, n) / 2.0
    z = rng.choice(n, max(n // 16, 2), replace=False)
    val[z[::2]] = 0.0
    val[z[1::2]] = -0.0
    return val


def cls_signed(seed, pat, K):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (pat.users, K)), rng.uniform(-1, 1, (pat.items, K)), _signed_ratings(rng, pat.nnz), 1e-3


def cls_range(seed, pat, K):
    rng = np.random.default_rng(seed)

    def draw(shape):
        return np.ldexp(rng.uniform(1, 2, shape) * rng.choice([-1.0, 1.0], shape), rng.integers(-40, 41, shape))
    return draw((pat.users, K)), draw((pat.items, K)), draw(pat.nnz), 2.0 ** -45


def cls_zeros(seed, pat, K):
    rng = np.random.default_rng(seed)
    values = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    prob = np.array([0.25, 0.25] + [1 / 12] * 6)
    L0 = rng.choice(values, (pat.users, K), p=prob)
    R0 = rng.choice(values, (pat.items, K), p=prob)
    # whole rows of +0.0 and of -0.0 on both sides: the rows without entries among them (they keep their sign in a seeded
    # sweep and must come out +0.0 from an unseeded one), and rows with entries
    for X, lens, planted in ((L0, pat.ulen, pat.planted_users), (R0, pat.ilen, pat.planted_items)):
        free = np.setdiff1d(np.arange(len(lens)), planted)
        empty, full = free[lens[free] == 0], free[lens[free] > 0]
        neg = np.concatenate([empty[::2], rng.choice(full, 6, replace=False)])
        pos = np.concatenate([empty[1::4], rng.choice(np.setdiff1d(full, neg), 6, replace=False)])
        X[neg] = -0.0
        X[pos] = 0.0
    val = rng.integers(-3, 4, pat.nnz).astype(np.float64)
    # about 40 % of the ratings, and every rating of a planted row, are the exact dot product: e is exactly +0.0 there and
    # every product e * y is a zero with the sign of y
    exact = rng.random(pat.nnz) < 0.4
    exact |= np.isin(pat.row, pat.planted_users) | np.isin(pat.col, pat.planted_items)
    val[exact] = seq_dot(L0, R0, pat.row, pat.col)[exact]
    return L0, R0, val, 0.25


def cls_subnormal_users(seed, pat, K):
    L0, R0, val, _ = cls_signed(seed, pat, K)
    return L0 * 2.0 ** -1030, R0, val * 2.0 ** -1030, 0.25


def cls_subnormal_items(seed, pat, K):
    L0, R0, val, _ = cls_signed(seed, pat, K)
    return L0, R0 * 2.0 ** -1030, val * 2.0 ** -1030, 0.25


def cls_nonfinite(seed, pat, K):
    """"signed" plus: a user row all NaN, +inf in L0, -inf in R0, 2^600 and -2^600 in one column, 2^1000, a NaN and a +inf
    rating -- all on the planted (one- or two-entry) rows, so that one step contaminates a few rows only."""
    L0, R0, val, alpha = cls_signed(seed, pat, K)
    rng = np.random.default_rng(seed + 1)
    pu, pi = pat.planted_users, pat.planted_items
    k = [int(x) for x in rng.integers(0, K, 4)]
    L0[pu[0], :] = np.nan
    L0[pu[1], k[0]] = np.inf
    R0[pi[0], k[1]] = -np.inf
    L0[pu[2], k[2]] = 2.0 ** 600
    L0[pu[3], k[2]] = -2.0 ** 600
    L0[pu[4], k[3]] = 2.0 ** 1000
    val[np.flatnonzero(pat.row == pu[5])[0]] = np.nan
    val[np.flatnonzero(pat.row == pu[6])[0]] = np.inf
    return L0, R0, val, alpha


CLASSES = {"signed": cls_signed, "range": cls_range, "zeros": cls_zeros, "subnormal-users": cls_subnormal_users,
           "subnormal-items": cls_subnormal_items, "nonfinite": cls_nonfinite}


def all_negzero_sums(e, Y, own, other, nrows):
    """Number of (row, column) sums of a sweep whose products e_n * Y[other_n][k] are ALL -0.0 (rows with entries only):
    from a zero start such a sum is +0.0; a kernel that starts from its first product gets -0.0."""
    with np.errstate(all="ignore"):
        prod = e[:, None] * Y[other]
    notneg = np.zeros((nrows, Y.shape[1]), np.int64)
    np.add.at(notneg, own, ~is_negzero(prod))
    return int(((notneg == 0) & (np.bincount(own, minlength=nrows) > 0)[:, None]).sum())


class Expected:
    pass


@functools.lru_cache(maxsize=None)
def expected(pat_name, cls, K):
    """Inputs of one (pattern, class, K), the oracle's results on them and the class's guard conditions -- asserted on the
    ORACLE's results, so that the inputs keep doing their job.  Computed once, shared by every form and chunk size."""
    from oracle import oracle as orc
    pat = pattern(pat_name)
    x = Expected()
    x.pat, x.K = pat, K
    x.L0, x.R0, x.val, x.alpha = CLASSES[cls](4000 + K, pat, K)
    U, I = pat.users, pat.items
    with np.errstate(all="ignore"):
        x.seeded = orc.tile_step(0, U, 0, I, K, pat.row, pat.col, x.val, x.alpha, x.L0, x.R0, True, True)
        x.unseeded = orc.tile_step(0, U, 0, I, K, pat.row, pat.col, x.val, x.alpha, x.L0, x.R0, False, False)
        L2, R2 = x.L0.copy(), x.R0.copy()
        orc.factorize(orc.Instance(2, x.alpha, K, U, I, pat.row, pat.col, x.val), L2, R2)
        x.two = (L2, R2)
    everything = x.seeded + x.unseeded + x.two
    where = (pat_name, cls, K)
    if cls != "nonfinite":
        assert not any(np.isnan(a).any() for a in everything), where
    if cls == "zeros":
        e = (x.alpha * 2) * (x.val - seq_dot(x.L0, x.R0, pat.row, pat.col))
        x.negzero_sums = (all_negzero_sums(e, x.L0, pat.col, pat.row, I), all_negzero_sums(e, x.R0, pat.row, pat.col, U))
        assert min(x.negzero_sums) >= 10, (where, x.negzero_sums)                     # item side, user side
        # ... and the oracle gives +0.0 for every one of them from a zero start: no -0.0 anywhere in an unseeded result
        assert not is_negzero(x.unseeded[0]).any() and not is_negzero(x.unseeded[1]).any(), where
        x.negzero_seeded = int(is_negzero(x.seeded[0]).sum())
        if pat_name == "pair":
            assert x.negzero_seeded >= 100, (where, x.negzero_seeded)
    if cls.startswith("subnormal"):
        side = 0 if cls == "subnormal-users" else 1
        new, old = x.seeded[side], (x.L0, x.R0)[side]
        x.subnormal = float(is_subnormal(new).mean())
        x.changed = float((new.view(np.uint64) != old.view(np.uint64)).mean())
        assert is_subnormal(old).all() and x.changed > 0.5, (where, x.changed)
        # rows of up to ~200 entries stay below 2^-1022 whatever the signs (ratings <= 5 * 2^-1030, |y| < 1)
        assert x.subnormal == 1.0 if pat_name == "pair" else x.subnormal > 0.5, (where, x.subnormal)
    if cls == "nonfinite":
        x.nan_rows = [int(np.isnan(a).any(axis=1).sum()) for a in x.seeded]
        x.inf_only_rows = [int((np.isinf(a).any(axis=1) & ~np.isnan(a).any(axis=1)).sum()) for a in x.seeded]
        for n, a in zip(x.nan_rows, x.seeded):
            assert 1 <= n <= a.shape[0] / 10, (where, x.nan_rows)
        assert sum(x.inf_only_rows) >= 1, (where, x.inf_only_rows)
    return x


GUARDED = ([(p, c, K) for p in ("pair", "long-items", "skewed") for c in CLASSES for K in (3, 6, 100)]
           + [("wide", c, K) for c in CLASSES for K in (513, 4095)])


@pytest.mark.parametrize("pat_name,cls,K", GUARDED, ids=["%s-%s-%d" % g for g in GUARDED])
def test_value_classes_do_their_job_on_the_oracle(pat_name, cls, K):
    """The guard conditions of every class (no NaN outside "nonfinite"; sums of nothing but -0.0 on both sides and -0.0
    results for "zeros"; a subnormal factor most of whose bits change; NaN in a few rows only and inf without NaN for
    "nonfinite") hold on the oracle's own results, on every pattern part A uses -- the wide one at the K of its rows."""
    x = expected(pat_name, cls, K)
    if cls == "zeros" and pat_name == "pair":
        print("zeros, K=%d: %d -0.0 in the seeded user result, all-(-0.0) sums items/users %s" % (K, x.negzero_seeded, x.negzero_sums))
    if cls == "nonfinite":
        assert np.isnan(x.two[1]).any() and np.isinf(x.seeded[0]).any()


# ------------------------------------------------------------------------------------------------ A: every sweep form
def _form(name, env, ks, pat, check, steps=True, nchs=(None, "5"), without=()):
    """rows of the table: `check` confirms the form in Plan.describe(); `nchs`: the chunk sizes a row runs at (the rule's, "5");
    `without`: value classes a row leaves out"""
    return [dict(name=name, env=env, K=k, pat=pat, check=check, steps=steps, nchs=nchs, without=without) for k in ks]


def _single_wave(desc, K, kt):
    return (desc.startswith("sweep_dma_kernel<KT=%d," % kt) and "long_rows=0/0 " in desc and "double_buffered=0/0(" in desc
            and "wave_pair=0/0(" in desc and "iterate=sweeps" in desc)


def _slice_width(K, first):
    """MF_ES_SW names the slice width the resident streams launch tries FIRST; a width that would cut K into more than
    eight slices is passed over for the next of 8, 4, 2 (every slice re-reads the records)."""
    return next(w for w in (first, 8, 4, 2) if -(-K // w) <= 8)


LDS_PER_CU = 160 * 1024


def tile_geometry(K, dma):
    """(bytes in front of the tile, tile row stride in bytes) of a plan's single-wave form: the LDS-DMA forms keep the x
    row, rounded up to 256 bytes, in front of rows of an odd number of 16-byte pieces; the register-staged form has rows of
    K | 1 doubles and nothing in front of them."""
    return (-(-K * 8 // 256) * 256, 16 * ((K >> 1) | 1)) if dma else (0, 8 * (K | 1))


def rule_nch(K, dma, forced=None):
    """Entries per chunk of the ordinary single-wave launch (the nch= of Plan.describe()) as chunk_rule states it: 16, cut to
    what a sixth of a CU's LDS holds but not below 12, cut to what the whole LDS holds; MF_SWEEP_NCH where that fits."""
    head, row = tile_geometry(K, dma)

    def fit(budget):
        return min(64, (budget - head) // row) if budget > head else 0
    nch = 16
    if head + nch * row > LDS_PER_CU // 6:
        nch = max(12, fit(LDS_PER_CU // 6))
    nch = min(nch, fit(LDS_PER_CU))
    if forced and head + forced * row <= LDS_PER_CU:
        nch = forced
    return nch


def generic_width(K, widths):
    """the first instance of a run-time-K table (64 columns per register, 128 per LDS-DMA pass) that holds K"""
    return next(w for w in widths if K <= w[1] * w[0])


REG_WIDTHS = [(kp, 64) for kp in (1, 2, 4, 8, 16, 32, 64)]
DMA_WIDTHS = [(np_, 128) for np_ in (1, 2, 4, 8)]


def _reg_wide(d, K):
    """the run-time-K register-staged instance of this K, and the whole LDS request where the rule ends on it"""
    kp = generic_width(K, REG_WIDTHS)[0]
    return (d.startswith("sweep_kernel<KT=0,KPMAX=%d> K=%d " % (kp, K)) and "iterate=sweeps" in d
            and (K != 4095 or " nch=5 stride=4095 lds=163800 " in d) and (K != 4096 or " nch=4 stride=4097 " in d))


def _dma_wide(d, K):
    return _single_wave(d, K, 0) and d.startswith("sweep_dma_kernel<KT=0,NPASS=%d> K=%d " % (generic_width(K, DMA_WIDTHS)[0], K))


def _db_wide(d, K):
    return (d.startswith("sweep_dma_kernel<KT=0,NPASS=%d> K=%d " % (generic_width(K, DMA_WIDTHS)[0], K))
            and "double_buffered=1/1(" in d and "long_rows=0/0 " in d and "iterate=sweeps" in d)


def _long_wide(d, K, dpp):
    """the extreme-row path beside the instance of this K: compile-time K = 128 (one pass) and 256 (two), else run-time K"""
    kt = K if K in (128, 256) else 0
    npass = -(-K // 128) if kt else generic_width(K, DMA_WIDTHS)[0]
    return (d.startswith("sweep_dma_kernel<KT=%d,NPASS=%d> K=%d " % (kt, npass, K)) and "long_rows=0/" not in d and "long_rows=" in d
            and ("MF_OS_DPP=0" in d) == (not dpp) and ("MF_OS_DPP" in d) == (not dpp) and "iterate=sweeps" in d)


def _reg_rt(d, K):
    return d.startswith("sweep_kernel<KT=0,KPMAX=%d> K=%d " % (generic_width(K, REG_WIDTHS)[0], K)) and "iterate=sweeps" in d


def _coop(d, K):
    return "long_rows=" in d and "long_rows=0/0 " not in d and "coop_nch=0 " not in d and "iterate=sweeps" in d


SWEEPS = {"MF_ITER_MODE": "sweeps"}
SINGLE = dict(SWEEPS, MF_SWEEP_PAIR="0", MF_SWEEP_DB="0")
LONG = dict(SWEEPS, MF_SWEEP_LONG="24")
# The rows of K above the narrow end of every family (the "wide" pattern: a factor row is up to 32 KiB), and the narrow rows
# the table guard of tests/test_wide_k.py found missing.  All carry wide=True: their description is also checked for the
# rule's nch, and the per-form tables of the other modules take their ends from the rows above, not from these.
#   reg-wide   the natural dispatch of an odd K above 256 and of every K above 1024, and MF_SWEEP_IMPL=reg: every KPMAX of
#              8 .. 64 once with lane 0 of its last register alone (64 * KPMAX / 2 + 1) and once full, the first even K past
#              the LDS-DMA range (1026) and the two plans at the edge of a CU's LDS (4095: five rows, 163800 bytes; 4096: four)
#   dma-rt     four passes (258, 512) and eight: one lane of the fifth (514), the seventh (770), the last piece (1022), full
#   coop       the cooperative form exists for the seven compile-time K.  The rule's 48 KiB budget holds eight entries up
#              to K = 50 (14 tiles of a row stride each per entry), so K = 100, 128 and 256 are reached through MF_SWEEP_NCH
#              only -- their rows run at "5" alone
#   reg-ct     the register-staged instances of a compile-time K, which MF_SWEEP_IMPL=reg picks at the K of the LDS-DMA table
#   reg, dma-rt (on "pair")   the first and the last K of the narrow run-time-K instances: tests/test_wide_k.py asks for both
#              ends of every instance's range (64 registers' worth of columns; 126 and 254: the last even K below a
#              compile-time one).  K = 1 and K = 2 leave the "zeros" class out: its guard -- ten sums of nothing but -0.0 on
#              each side -- cannot hold on one or two columns of a hundred item rows, and the class reaches both instances
#              at K = 3 and K = 6
REG = dict(SWEEPS, MF_SWEEP_IMPL="reg")
WIDE_FORMS = (
    _form("reg-ct", REG, [20, 30, 50, 128, 256], "pair",
          lambda d, K: d.startswith("sweep_kernel<KT=%d,KPMAX=%d> K=%d " % (K, -(-K // 64), K)) and "iterate=sweeps" in d)
    + _form("reg", REG, [1], "pair", _reg_rt, without=("zeros",))
    + _form("reg", REG, [64, 127, 255], "pair", _reg_rt)
    + _form("dma-rt", SINGLE, [2], "pair", _dma_wide, without=("zeros",))
    + _form("dma-rt", SINGLE, [126, 254], "pair", _dma_wide)
    + _form("reg-wide", SWEEPS, [257, 513, 1025, 1026, 2049, 4095, 4096], "wide", _reg_wide)
    + _form("reg-wide", REG, [512, 1024, 2048], "wide", _reg_wide)
    + _form("dma-rt", SINGLE, [258, 512, 514, 770, 1022, 1024], "wide", _dma_wide)
    + _form("db", dict(SWEEPS, MF_SWEEP_DB="1"), [130, 300, 1024], "wide", _db_wide)
    + _form("long", LONG, [64, 128, 130, 256, 300, 1024], "long-items", lambda d, K: _long_wide(d, K, True))
    + _form("long-nodpp", dict(LONG, MF_OS_DPP="0"), [64, 128, 130, 256, 300, 1024], "long-items", lambda d, K: _long_wide(d, K, False))
    + _form("coop", SWEEPS, [20], "skewed", lambda d, K: _coop(d, K) and d.startswith("sweep_dma_kernel<KT=20,"))
    + _form("coop", SWEEPS, [100, 128, 256], "skewed",
            lambda d, K: _coop(d, K) and d.startswith("sweep_dma_kernel<KT=%d," % K) and " coop_nch=5 " in d, nchs=("5",))
)
FORMS = (
    _form("reg", dict(SWEEPS, MF_SWEEP_IMPL="reg"), [3, 7, 10, 65, 100, 129], "pair",
          lambda d, K: d.startswith("sweep_kernel<") and "iterate=sweeps" in d)
    + _form("dma-ct", SINGLE, [10, 20, 30, 50, 100, 128, 256], "pair", lambda d, K: _single_wave(d, K, K))
    + _form("dma-rt", SINGLE, [6, 64, 96, 130, 300], "pair", lambda d, K: _single_wave(d, K, 0))
    + _form("db", dict(SWEEPS, MF_SWEEP_DB="1"), [64, 100, 256], "pair",
            lambda d, K: "double_buffered=1/1(" in d and "long_rows=0/0 " in d and "iterate=sweeps" in d)
    + _form("pair", dict(SWEEPS, MF_SWEEP_PAIR="1"), [100, 128], "pair",
            lambda d, K: "wave_pair=1/1(" in d and "long_rows=0/0 " in d and "iterate=sweeps" in d)
    + _form("long", dict(SWEEPS, MF_SWEEP_LONG="24"), [6, 30, 100], "long-items",
            lambda d, K: "long_rows=0/" not in d and "long_rows=" in d and "MF_OS_DPP" not in d and "iterate=sweeps" in d)
    + _form("long-nodpp", dict(SWEEPS, MF_SWEEP_LONG="24", MF_OS_DPP="0"), [6, 30, 100], "long-items",
            lambda d, K: "long_rows=0/" not in d and "long_rows=" in d and "MF_OS_DPP=0" in d and "iterate=sweeps" in d)
    + _form("coop", SWEEPS, [10, 30, 50], "skewed",
            lambda d, K: "long_rows=" in d and "long_rows=0/0 " not in d and "coop_nch=0 " not in d and "iterate=sweeps" in d)
    + [f for sw in ("8", "4", "2")
       for f in _form("es-sw" + sw, {"MF_ITER_MODE": "es", "MF_ES_SW": sw}, [6, 10, 30, 50, 64], "pair",
                      lambda d, K, sw=sw: "iterate=errors+resident-streams(" in d and
                      ", %d-column slices of Y in LDS" % _slice_width(K, int(sw)) in d, steps=False)]
    + [dict(f, wide=True) for f in WIDE_FORMS]
)
CASES = [dict(f, nch=nch) for f in FORMS for nch in f["nchs"]]


def _case_id(c):
    return "%s-K%d-nch%s" % (c["name"], c["K"], c["nch"] or "rule")


def wide_nch(desc, case):
    """the nch= of a wide row's description is chunk_rule's for the form the description names"""
    nch = rule_nch(case["K"], desc.startswith("sweep_dma_kernel<"), int(case["nch"]) if case["nch"] else None)
    return " K=%d " % case["K"] in desc and " nch=%d " % nch in desc


def test_every_form_of_the_issue_is_in_the_table():
    ks = {}
    for c in CASES:
        ks.setdefault(c["name"], set()).add(c["K"])
    assert ks["reg"] == {3, 7, 10, 65, 100, 129, 1, 64, 127, 255} and ks["dma-ct"] == {10, 20, 30, 50, 100, 128, 256}
    assert ks["reg-ct"] == {20, 30, 50, 128, 256} and ks["reg-wide"] == {257, 512, 513, 1024, 1025, 1026, 2048, 2049, 4095, 4096}
    assert ks["dma-rt"] == {6, 64, 96, 130, 300, 2, 126, 254, 258, 512, 514, 770, 1022, 1024} and ks["db"] == {64, 100, 256, 130, 300, 1024}
    assert ks["pair"] == {100, 128}
    assert ks["long"] == ks["long-nodpp"] == {6, 30, 100, 64, 128, 130, 256, 300, 1024} and ks["coop"] == {10, 20, 30, 50, 100, 128, 256}
    assert ks["es-sw8"] == ks["es-sw4"] == ks["es-sw2"] == {6, 10, 30, 50, 64}
    assert set(ks) == {"reg", "reg-ct", "reg-wide", "dma-ct", "dma-rt", "db", "pair", "long", "long-nodpp", "coop", "es-sw8", "es-sw4", "es-sw2"}
    # every row at the rule's chunk size and at 5, but the cooperative rows the rule's budget does not reach: at 5 alone
    only5 = [f for f in FORMS if f["nchs"] == ("5",)]
    assert sorted((f["name"], f["K"]) for f in only5) == [("coop", 100), ("coop", 128), ("coop", 256)]
    assert len(CASES) == 2 * len(FORMS) - len(only5) and {c["nch"] for c in CASES} == {None, "5"}
    assert len({_case_id(c) for c in CASES}) == len(CASES)
    # every row runs the six classes, but K = 1 and K = 2 (see WIDE_FORMS): five
    assert sorted((f["name"], f["K"]) for f in FORMS if f["without"]) == [("dma-rt", 2), ("reg", 1)]
    assert len(CASES_BY_CLASS) == len(CASES) * len(CLASSES) - 2 * 2
    # the natural dispatch of the wide register-staged rows sets no MF_SWEEP_IMPL; the full-register ones force it
    for f in FORMS:
        if f["name"] == "reg-wide":
            assert ("MF_SWEEP_IMPL" in f["env"]) == (f["K"] in (512, 1024, 2048)), f["K"]


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


CASES_BY_CLASS = [(c, cls) for c in CASES for cls in CLASSES if cls not in c["without"]]


@gpu
@pytest.mark.parametrize("case,cls", CASES_BY_CLASS, ids=["%s-%s" % (_case_id(c), cls) for c, cls in CASES_BY_CLASS])
def test_special_values_through_every_sweep_form(device, switches, case, cls):
    """One value class through one sweep form: both sweeps seeded from the old generation and from zero (orc.tile_step with
    the matching l_is_root / r_is_root), then two whole iterations (orc.factorize) -- NaN in the same places, the same bits
    everywhere else.  The errors + resident streams form runs whole iterations only."""
    capi = device
    K = case["K"]
    x = expected(case["pat"], cls, K)
    pat = x.pat
    switches(case["env"])
    if case["nch"]:
        switches({"MF_SWEEP_NCH": case["nch"]})
    plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val)
    try:
        desc = plan.describe()
        assert case["check"](desc, K), desc
        assert ("MF_SWEEP_NCH=5" in desc) == (case["nch"] == "5"), desc
        if case.get("wide"):
            assert wide_nch(desc, case), desc
        where = "%s %s K=%d [%s]" % (_case_id(case), cls, K, desc.split(" loss=")[0])
        if case["steps"]:
            for seed, want in ((True, x.seeded), (False, x.unseeded)):
                plan.upload(x.L0, x.R0)
                plan.sweep_items(seed_from_old=seed)
                plan.sweep_users(seed_from_old=seed)
                plan.flip()
                L, R = plan.download()
                assert_same_bits(R, want[1], "%s: item sweep, %s" % (where, "seeded" if seed else "from zero"))
                assert_same_bits(L, want[0], "%s: user sweep, %s" % (where, "seeded" if seed else "from zero"))
        plan.upload(x.L0, x.R0)
        plan.iterate(2)
        L, R = plan.download()
        assert_same_bits(L, x.two[0], where + ": L after two iterations")
        assert_same_bits(R, x.two[1], where + ": R after two iterations")
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ B: launch sizes
EDGE_LENS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 90]
PF_ROWS = 262144          # launches of more rows (K <= 128) take the plain accumulate form
GRID_CAP = 1 << 20        # workgroups of a sweep, products or loss launch: more rows mean a second trip of the row loop


def _edge_lens(n):
    return np.array([EDGE_LENS[t % len(EDGE_LENS)] for t in range(n)])


@functools.lru_cache(maxsize=None)
def pattern_both_large():
    """B1: 262144 + 77 users x 262144 + 5 items.  On both sides the first and the last hundred rows have the lengths
    EDGE_LENS in turn, every other row one or two entries."""
    U, I, H = PF_ROWS + 77, PF_ROWS + 5, 100
    ou, oi = np.arange(H, U - H), np.arange(H, I - H)                 # the ordinary rows of both sides
    rows, cols = [ou], [oi[np.arange(len(ou)) % len(oi)]]             # one entry per ordinary user: items get one or two
    su, si = np.concatenate([np.arange(H), np.arange(U - H, U)]), np.concatenate([np.arange(H), np.arange(I - H, I)])
    lens = np.concatenate([_edge_lens(H), _edge_lens(H)])
    # the special users' entries: one more for ordinary items 1000, 1001, ...; the special items': for users 10000, ...
    rows.append(np.repeat(su, lens))
    cols.append(oi[1000 + np.arange(lens.sum())])
    cols.append(np.repeat(si, lens))
    rows.append(ou[10000 + np.arange(lens.sum())])
    return Pattern("both-large", U, I, np.concatenate(rows), np.concatenate(cols))


@functools.lru_cache(maxsize=None)
def pattern_one_large(users_large):
    """B2: 2^20 + 130 rows on the large side (first and last hundred: EDGE_LENS in turn, the others one or two entries),
    300 on the other."""
    N, M, H = GRID_CAP + 130, 300, 100
    rng = np.random.default_rng(77)
    lens = 1 + (rng.random(N) < 0.5).astype(np.int64)
    lens[:H] = _edge_lens(H)
    lens[N - H:] = _edge_lens(H)
    big = np.repeat(np.arange(N), lens)
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    small = rng.integers(0, M, len(big))
    second = np.flatnonzero(np.arange(len(big)) - first[big] == 1)   # the second entry of a row: another column
    small[second] = (small[second - 1] + 1 + rng.integers(0, M - 1, len(second))) % M
    for r in np.concatenate([np.arange(H), np.arange(N - H, N)]):
        if lens[r] > 2:
            small[first[r]:first[r] + lens[r]] = rng.choice(M, int(lens[r]), replace=False)
    if users_large:
        return Pattern("users-large", N, M, big, small)
    return Pattern("items-large", M, N, small, big)


def test_launch_size_patterns():
    p = pattern_both_large()
    assert (p.users, p.items) == (PF_ROWS + 77, PF_ROWS + 5)
    for lens in (p.ulen, p.ilen):
        assert lens[:100].tolist() == _edge_lens(100).tolist() and lens[-100:].tolist() == _edge_lens(100).tolist()
        assert set(lens[100:-100].tolist()) == {1, 2}
    for users_large in (True, False):
        q = pattern_one_large(users_large)
        lens, other = (q.ulen, q.ilen) if users_large else (q.ilen, q.ulen)
        assert len(lens) == GRID_CAP + 130 and len(other) == 300 and other.min() > 0
        assert lens[:100].tolist() == _edge_lens(100).tolist() and lens[-100:].tolist() == _edge_lens(100).tolist()
        assert set(lens[100:-100].tolist()) == {1, 2}
        key = q.row.astype(np.int64) * q.items + q.col
        assert (np.diff(key) > 0).all()


def test_the_oracle_gives_the_same_bits_on_entries_stably_sorted_by_item(orc):
    """run_steps hands the oracle an item-heavy instance sorted by item: a sum's terms and their order do not change."""
    for name, cls in (("pair", "range"), ("skewed", "nonfinite"), ("long-items", "zeros")):
        x = expected(name, cls, 6)
        pat, order = x.pat, x.pat.by_item()
        assert (np.diff(pat.col[order]) >= 0).all() and not (np.diff(order) > 0).all()
        for seed, want in ((True, x.seeded), (False, x.unseeded)):
            with np.errstate(all="ignore"):
                L, R = orc.tile_step(0, pat.users, 0, pat.items, 6, np.ascontiguousarray(pat.row[order]),
                                     np.ascontiguousarray(pat.col[order]), np.ascontiguousarray(x.val[order]), x.alpha,
                                     x.L0, x.R0, seed, seed)
            assert_same_bits(L, want[0], "%s %s seed=%s L" % (name, cls, seed))
            assert_same_bits(R, want[1], "%s %s seed=%s R" % (name, cls, seed))


def big_factor(rng, n, K):
    """n x K doubles in (-1, 1), every row different from its neighbours and from the row 2^20 before it: a block of 65536
    random rows, scaled per block by a signed power of two (filling 2 GB from the generator would take seconds)."""
    base = rng.uniform(-1, 1, (min(n, 65536), K))
    out = np.empty((n, K))
    for b, s in enumerate(range(0, n, 65536)):
        blk = out[s:s + 65536]
        np.multiply(base[:len(blk)], (-1.0) ** b * 2.0 ** -(b % 5), out=blk)
    return out


def signed_inputs(seed, pat, K):
    rng = np.random.default_rng(seed)
    return big_factor(rng, pat.users, K), big_factor(rng, pat.items, K), _signed_ratings(rng, pat.nnz)


def run_steps(plan, orc, pat, K, alpha, L0, R0, val, where):
    """One seeded and one unseeded step, every row of both factors against orc.tile_step (the two oracle runs on threads
    of their own, beside the GPU's work: at 2^20 rows and K = 100 each takes as long as everything else together)."""
    U, I = pat.users, pat.items
    row, col = pat.row, pat.col
    if I > U:
        # The oracle walks the entries in the order given, and by user that order jumps all over a 2^20-row item factor.
        # Stably sorted by item instead, every user still meets its items in ascending order and every item its users in
        # ascending order -- each sum has the same terms in the same order, so the same bits -- and the walk is sequential
        # (half the oracle's time).  The plan gets the entries in file order.
        order = pat.by_item()
        row, col, val = (np.ascontiguousarray(a[order]) for a in (row, col, val))
    with ThreadPoolExecutor(2) as pool:
        want = {seed: pool.submit(orc.tile_step, 0, U, 0, I, K, row, col, val, alpha, L0, R0, seed, seed)
                for seed in (True, False)}
        plan.upload(L0, R0)
        for seed in (True, False):
            plan.sweep_items(seed_from_old=seed)
            plan.sweep_users(seed_from_old=seed)
            plan.flip()
            L, R = plan.download()
            plan.flip()                                              # back to the uploaded generation: a sweep writes the other one only
            Lo, Ro = want[seed].result()
            assert_same_bits(R, Ro, "%s: item sweep, seed=%s" % (where, seed))
            assert_same_bits(L, Lo, "%s: user sweep, seed=%s" % (where, seed))


@gpu
@pytest.mark.parametrize("K", [10, 20, 30, 50, 100, 128])
def test_plain_accumulate_form_just_above_262144_rows(device, orc, switches, K):
    """More than 262144 rows on both sides: both sweeps take the plain accumulate form of the compile-time K
    (sweep_dma_kernel<K, passes, accumulate> without the pipelined phases) -- what cfg4's user sweep runs, and what no
    smaller launch reaches.  A twin plan of exactly 262144 rows takes the pipelined form."""
    capi = device
    switches(SWEEPS)
    twin = capi.Plan(PF_ROWS, PF_ROWS, K, 1e-3, np.arange(PF_ROWS, dtype=np.int32), np.arange(PF_ROWS, dtype=np.int32),
                     np.ones(PF_ROWS))
    desc = twin.describe()
    twin.close()
    assert " accumulate=pf/pf " in desc and _single_wave(desc, K, K), desc
    pat = pattern_both_large()
    L0, R0, val = signed_inputs(5000 + K, pat, K)
    plan = capi.Plan(pat.users, pat.items, K, 1e-3, pat.row, pat.col, val)
    try:
        desc = plan.describe()
        assert " accumulate=plain/plain " in desc and _single_wave(desc, K, K), desc
        run_steps(plan, orc, pat, K, 1e-3, L0, R0, val, "K=%d, %d x %d" % (K, pat.users, pat.items))
    finally:
        plan.close()


SECOND_TRIP = {
    "reg-K3": (3, dict(SWEEPS, MF_SWEEP_IMPL="reg"), lambda d, big: d.startswith("sweep_kernel<")),
    "dma-rt-K6": (6, SINGLE, lambda d, big: _single_wave(d, 6, 0)),
    "dma-ct-plain-K10": (10, SINGLE, lambda d, big: _single_wave(d, 10, 10) and
                         (" accumulate=pf/plain " if big == 0 else " accumulate=plain/pf ") in d),
    "db-K10": (10, dict(SWEEPS, MF_SWEEP_DB="1"),
               lambda d, big: "double_buffered=1/1(" in d and d.startswith("sweep_dma_kernel<KT=10,") and "long_rows=0/0 " in d),
    "pair-K100": (100, dict(SWEEPS, MF_SWEEP_PAIR="1"), lambda d, big: "wave_pair=1/1(" in d and "long_rows=0/0 " in d),
    "dma-ct-pf-K256": (256, SINGLE, lambda d, big: _single_wave(d, 256, 256) and " accumulate=pf/pf " in d),
}


@gpu
@pytest.mark.parametrize("large", ["users", "items"])
@pytest.mark.parametrize("form", list(SECOND_TRIP))
def test_second_trip_of_the_row_loop_just_above_2_to_20_rows(device, orc, switches, form, large):
    """2^20 + 130 rows on one side: a launch is min(rows, 2^20) workgroups, so 130 workgroups walk a second row -- the last
    hundred rows with the chunk-edge lengths among them.  Per-row state (accumulators, tile parity and barriers of the pair
    form, the buffers of the double-buffered form, the registers of the pipelined phases) and the LDS hand-over from one row
    to the next must be right there.  The K = 10 plan also runs the training loss, whose kernels have the same loop and cap.
    K = 256 is the one K whose launch takes the pipelined form at this size: 2.1 GB per factor generation, some 10 GB of host
    memory, and still every row of both factors after both steps (measured below the yardstick uncut, so not cut)."""
    capi = device
    K, env, check = SECOND_TRIP[form]
    switches(env)
    pat = pattern_one_large(large == "users")
    side = 0 if large == "users" else 1
    L0, R0, val = signed_inputs(6000 + K, pat, K)
    alpha = 1e-3
    plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
    try:
        desc = plan.describe()
        assert check(desc, side), desc
        where = "%s, %s large [%s]" % (form, large, desc.split(" loss=")[0])
        if form == "dma-ct-plain-K10":
            plan.upload(L0, R0)
            out, rs = plan.loss("train", rows=True)
            d = val - seq_dot(L0, R0, pat.row, pat.col)
            q = d * d                                               # row sums in entry order from 0.0, all rows at once
            first = np.concatenate([[0], np.cumsum(pat.ulen)[:-1]])
            ms = np.zeros(pat.users)
            for j in range(int(pat.ulen.max())):
                has = pat.ulen > j
                ms[has] = ms[has] + q[first[has] + j]
            few = np.concatenate([np.arange(40), np.arange(pat.users - 40, pat.users)]) if side == 0 else np.arange(2)
            sel = np.isin(pat.row, few)
            assert_same_bits(ms[few], model_rows(L0[few], R0, np.searchsorted(few, pat.row[sel]), pat.col[sel], val[sel], len(few)),
                             where + ": the vectorised row sums against model_rows of test_loss.py")
            assert out.count == pat.nnz
            assert_same_bits(rs, ms, where + ": row sums of the training loss")
            assert_same_bits(np.array([out.sse]), np.array([model_total(ms)]), where + ": training SSE")
        run_steps(plan, orc, pat, K, alpha, L0, R0, val, where)
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ C: the oracle, pinned
def test_oracle_equals_the_reference_on_signed_and_diverging_runs(orc):
    """reference_special.npz (tests/golden/make_golden.py): the reference's own L, R, B on 40 x 30, K = 6 instances with
    ratings in [-5, 5] -- alpha 0.5 and 3.0 (inf after six or seven iterations, NaN after one more), 0.05 (grows, finite
    after eight) and 0.002 (converges) -- after 1, 2, 3, 5, 6, 7 and 8 iterations.  The oracle gives NaN in the same places
    and the same bits everywhere else; where oracle/_ref is built, the live reference still gives the recorded results."""
    snap = np.load(os.path.join(GOLDEN, "reference_special.npz"))
    seen_nan = seen_inf = 0
    for n, alpha in enumerate(make_golden.SPECIAL_ALPHAS):
        d = make_golden.special_instance(n)
        for key in ("row", "col", "val"):
            assert_same_bits(d[key].astype(np.float64), snap["%s_%d" % (key, n)].astype(np.float64), "instance %d %s" % (n, key))
        inst = orc.Instance(**d)
        for it in make_golden.SPECIAL_ITERS:
            Lr, Rr, Br = (snap["%s_%d_%d" % (m, n, it)] for m in "LRB")
            where = "alpha %g after %d iterations" % (alpha, it)
            if orc.ref_available():
                with np.errstate(all="ignore"):
                    live = orc.ref_run(inst, iters=it)
                for a, b, m in zip(live, (Lr, Rr, Br), "LRB"):
                    assert_same_bits(a, b, "live reference, %s, %s" % (where, m))
            L, R = orc.init_factors(inst.users, inst.items, inst.feats)
            with np.errstate(all="ignore"):
                orc.factorize(inst, L, R, iters=it)
                B = np.stack([orc.predict_row(L[i], R) for i in range(inst.users)])
            assert_same_bits(L, Lr, where + ", L")
            assert_same_bits(R, Rr, where + ", R")
            assert_same_bits(B, Br, where + ", B")
            seen_nan += int(np.isnan(Lr).any())
            seen_inf += int(np.isinf(Lr).any())
    assert seen_nan >= 3 and seen_inf >= 2          # the fixture does hold diverged states
    text = open(os.path.join(GOLDEN, "instDiverge.in")).read()
    assert text == to_text(make_golden.special_instance(make_golden.DIVERGE))
    inst = orc.parse_in(text, is_text=True)
    L, R = orc.init_factors(inst.users, inst.items, inst.feats)
    with np.errstate(all="ignore"):
        orc.factorize(inst, L, R)
        best = orc.recommend(inst, L, R)
    assert np.isnan(L).any() and orc.format_out(best) == open(os.path.join(GOLDEN, "instDiverge.out")).read()


@gpu
def test_cli_prints_the_reference_bytes_on_a_diverging_instance(device):
    r = subprocess.run([device.CLI_PATH, os.path.join(GOLDEN, "instDiverge.in")], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(os.path.join(GOLDEN, "instDiverge.out"), "rb").read()


@gpu
@pytest.mark.parametrize("mode", ["auto", "sweeps", "reg"])
def test_backend_run_leaves_the_reference_nan_pattern(device, switches, mode):
    """mf_backend_run on the diverging instances, stopped where the reference's factors are finite but huge, all inf, and
    all NaN: NaN where the reference has NaN, the reference's bits everywhere else."""
    capi = device
    switches({"auto": {}, "sweeps": SWEEPS, "reg": dict(SWEEPS, MF_SWEEP_IMPL="reg")}[mode])
    snap = np.load(os.path.join(GOLDEN, "reference_special.npz"))
    for n in range(len(make_golden.SPECIAL_ALPHAS)):
        d = make_golden.special_instance(n)
        inst = capi.Instance(d["iters"], d["alpha"], d["feats"], d["users"], d["items"], d["row"], d["col"], d["val"])
        for it in make_golden.SPECIAL_ITERS:
            L, R = capi.init_factors(inst.users, inst.items, inst.feats)
            capi.backend_factorize(inst, L, R, iters=it)
            where = "%s, alpha %g after %d iterations" % (mode, d["alpha"], it)
            assert_same_bits(L, snap["L_%d_%d" % (n, it)], where + ", L")
            assert_same_bits(R, snap["R_%d_%d" % (n, it)], where + ", R")
    inst = capi.parse_file(os.path.join(GOLDEN, "instDiverge.in"))
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    best = capi.backend_run(inst, L, R)
    it = make_golden.SPECIAL_ITERS[-1]
    assert inst.iters == it and np.isnan(snap["L_%d_%d" % (make_golden.DIVERGE, it)]).any()
    assert_same_bits(L, snap["L_%d_%d" % (make_golden.DIVERGE, it)], mode + ", backend_run, L")
    assert_same_bits(R, snap["R_%d_%d" % (make_golden.DIVERGE, it)], mode + ", backend_run, R")
    assert "".join("%d\n" % b for b in best if b >= 0) == open(os.path.join(GOLDEN, "instDiverge.out")).read()
