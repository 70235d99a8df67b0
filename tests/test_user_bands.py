"""The user sweep in item bands (mf_schedule.h: band_count / bands_at_launch / band_cut; launch_sweep; the kSweepResume
instances of sweep_dma_kernel).

A user sweep in B bands is B launches, band b walking the entries of every row whose item id lies in band b's range, the
partial row handed on through the next-generation buffer.  The chain of adds per element is the one chain of the single
launch, so every result here is compared bit for bit: with MF_SWEEP_BANDS=0 on the same instance, and with the CPU oracle.

CPU tests: tests/bands_main.cpp includes only mf_schedule.h and prints the band ranges, the offset cut of a row and the two
rules; they are checked against a model written here.  GPU tests: forced band counts on small instances with planted rows,
and every plan the rule excludes."""
import functools
import os
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
ITERS = 3
ALPHA = 1e-3


def clean_env(monkeypatch, **env):
    """No MF_* switch but those given (a plan reads the environment when it is created)."""
    for k in list(os.environ):
        if k.startswith("MF_"):
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


# ------------------------------------------------------------------------------------------------ the host functions
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bands") / "bands_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "bands_main.cpp")])
    return exe


def ask(program, tmp_path, lines):
    inp = tmp_path / "input.txt"
    inp.write_text("\n".join(lines) + "\n")
    out = subprocess.run([program, str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines), (lines, out)
    return [[int(x) for x in ln.split()[1:]] for ln in out]


def model_first(items, bands):
    return [b * items // bands for b in range(bands + 1)]


def test_band_ranges_are_equal_ascending_and_cover_the_items(program, tmp_path):
    shapes = [(200, 1), (200, 2), (200, 3), (200, 8), (200, 237), (64, 8), (64, 100), (1, 1), (1, 5), (3, 8), (100000, 12),
              (2 ** 31 - 65, 4096)]
    got = ask(program, tmp_path, ["first %d %d" % s for s in shapes])
    for (items, bands), first in zip(shapes, got):
        assert first == model_first(items, bands), (items, bands)
        assert first[0] == 0 and first[-1] == items and all(a <= b for a, b in zip(first, first[1:])), (items, bands)
        widths = [b - a for a, b in zip(first, first[1:])]
        assert max(widths) - min(widths) <= 1, (items, bands)              # equal ranges
        assert (0 in widths) == (items < bands), (items, bands)            # empty ones only where items < bands


def test_offset_cut_of_a_row(program, tmp_path):
    rng = np.random.default_rng(5)
    cases = []
    for items, bands in ((200, 1), (200, 2), (200, 3), (200, 8), (64, 8), (64, 100), (3, 8), (1, 4)):
        first = model_first(items, bands)
        rows = [[], list(range(items)), [0], [items - 1],
                sorted(set(first[:-1])),                                    # an entry on every band's first item
                sorted(set(f - 1 for f in first[1:] if f > 0))]             # ... and on every band's last one
        rows += [sorted(rng.choice(items, n, replace=False).tolist()) for n in (1, min(items, 7), min(items, 40))]
        cases += [(items, bands, row) for row in rows]
    got = ask(program, tmp_path, ["cut %d %d %d %s" % (i, b, len(r), " ".join(map(str, r))) for i, b, r in cases])
    for (items, bands, row), off in zip(cases, got):
        first = model_first(items, bands)
        assert off == [int(np.searchsorted(row, f, side="left")) for f in first[:-1]] + [len(row)], (items, bands, row)
        # band b holds exactly the entries whose id is in its range, in the row's order
        for b in range(bands):
            assert row[off[b]:off[b + 1]] == [j for j in row if first[b] <= j < first[b + 1]], (items, bands, b, row)


def count_line(user_side=1, sorted_=1, weighted=0, extreme=0, single_wave=1, fixed_k=1, nrows=1000000, items=100000,
               nnz=100000000, longest_column=1150, y_bytes=80000000, l2_bytes=32 << 20, forced=-1):
    return "count %d %d %d %d %d %d %d %d %d %d %d %d %d" % (user_side, sorted_, weighted, extreme, single_wave, fixed_k, nrows,
                                                            items, nnz, longest_column, y_bytes, l2_bytes, forced)


def test_band_count_rule(program, tmp_path):
    (consts,) = ask(program, tmp_path, ["consts"])
    rule, floor, most, table = consts
    assert rule >= 0 and floor >= 1 and most >= 1024
    lines = {
        "cfg4": count_line(),                                              # the size rule on the flagship shape
        "forced8": count_line(forced=8), "forced1": count_line(forced=1), "forced0": count_line(forced=0),
        "forced_small": count_line(nrows=300, items=200, nnz=9000, y_bytes=200 * 800, forced=8),   # a forced count needs no size
        "forced_more_than_items": count_line(nrows=300, items=64, nnz=5000, y_bytes=64 * 128, forced=100),
        "forced_capped": count_line(nrows=300, items=64, nnz=5000, forced=10 ** 6),
        "forced_table_too_large": count_line(forced=most),                 # (4096 + 1) x 1e6 ints
        "y_in_l2": count_line(items=40000, y_bytes=32 << 20),
        "y_above_l2": count_line(items=40000, y_bytes=(32 << 20) + 800),
        "y_4_l2": count_line(y_bytes=4 * (32 << 20)), "y_above_4_l2": count_line(y_bytes=4 * (32 << 20) + 800),
        "forced_y_large": count_line(y_bytes=64 * (32 << 20), forced=2),
        "hot_column": count_line(longest_column=4000), "no_hot_column": count_line(longest_column=3999),   # mean column 1000
        "forced_hot_column": count_line(longest_column=999104, forced=2),
        "short_rows": count_line(nnz=1000000 * max(rule, 1) * floor - 1),
        "floor_rows": count_line(nnz=1000000 * max(rule, 1) * floor),
        "item_side": count_line(user_side=0, forced=8), "unsorted": count_line(sorted_=0, forced=8),
        "weighted": count_line(weighted=1, forced=8), "extreme": count_line(extreme=1, forced=8),
        "pair": count_line(single_wave=0, forced=8), "runtime_k": count_line(fixed_k=0, forced=8),
        "no_rows": count_line(nrows=0, forced=8), "no_items": count_line(items=0, forced=8), "no_entries": count_line(nnz=0, forced=8),
    }
    got = {k: v[0] for k, v in zip(lines, ask(program, tmp_path, list(lines.values())))}
    want = dict(cfg4=rule, forced8=8, forced1=1, forced0=0, forced_small=8, forced_more_than_items=100, forced_capped=most,
                forced_table_too_large=0, y_in_l2=0, y_above_l2=rule, y_4_l2=rule, y_above_4_l2=0, forced_y_large=2, hot_column=0, no_hot_column=rule, forced_hot_column=2, short_rows=0, floor_rows=rule, item_side=0, unsorted=0,
                weighted=0, extreme=0, pair=0, runtime_k=0, no_rows=0, no_items=0, no_entries=0)
    assert got == want
    assert (most + 1) * 1000000 * 4 > table >= (most + 1) * 300 * 4


def test_bands_run_only_for_a_seeded_plain_launch(program, tmp_path):
    accumulate, decay, momentum, decay_w, momentum_w = range(5)            # mf_sched::Flavour
    cases = [((8, 1, accumulate, 0), 1), ((1, 1, accumulate, 0), 1), ((0, 1, accumulate, 0), 0), ((8, 0, accumulate, 0), 0),
             ((8, 1, decay, 0), 0), ((8, 1, momentum, 0), 0), ((8, 1, decay_w, 0), 0), ((8, 1, momentum_w, 0), 0),
             ((8, 1, accumulate, 1), 0), ((8, 0, accumulate, 1), 0)]
    got = ask(program, tmp_path, ["launch %d %d %d %d" % c for c, _ in cases])
    assert [g[0] for g in got] == [w for _, w in cases]


# ------------------------------------------------------------------------------------------------ the instances
SHAPES = {
    # name: users, items, K, density, MF_SWEEP_NCH (16: the chunk of a large launch, so 17 and 33 entries are 2 and 3 chunks)
    "k100": (300, 200, 100, 0.15, 16),
    "k10": (300, 64, 10, 0.25, None),
    # 600 rows: a launch of 512 to 32768 rows is dispatched longest row first, through a rowlist
    "rowlist": (600, 64, 10, 0.25, None),
}
BANDS = ("1", "2", "3", "8", "more")


def band_counts(items):
    return {"1": 1, "2": 2, "3": 3, "8": 8, "more": items + 37}


@functools.lru_cache(maxsize=None)
def instance(shape):
    """(row, col)-sorted instance with the planted rows 0..9; every band geometry of BANDS meets several of them."""
    U, I, K, density, _ = SHAPES[shape]
    rng = np.random.default_rng(1000 + U + I + K)
    mask = rng.random((U, I)) < density
    firsts = sorted({f for b in (2, 3, 8) for f in model_first(I, b)[:-1]})
    lasts = sorted({f - 1 for b in (2, 3, 8) for f in model_first(I, b)[1:]})
    w8 = I // 8
    plant = {
        0: [],                                                  # an empty row
        1: range(2 * w8, 3 * w8),                               # all entries in one band (of 8, and of 2 and 3 unless it straddles)
        2: range(I - w8, I),                                    # no entry in the first band
        3: range(0, w8),                                        # none in the last band
        4: firsts,                                              # an entry exactly on a band's first item
        5: lasts,                                               # ... and on a band's last one
        6: range(I // 3 + 1, I // 3 + 18),                      # 17 entries in the middle band of 3
        7: range(I // 2, min(I, I // 2 + 33)) if I >= 66 else range(I - 33, I),   # 33 entries in the upper band of 2 (in the one band at 64 items)
        8: [I - 1],                                             # one entry, the last item
        9: [0],                                                 # one entry, the first item
    }
    for r, cols in plant.items():
        mask[r, :] = False
        mask[r, list(cols)] = True
    assert mask[6].sum() == 17 and mask[7].sum() == 33
    row, col = np.nonzero(mask)
    val = rng.integers(1, 6, row.shape[0]).astype(np.float64)
    return types.SimpleNamespace(users=U, items=I, feats=K, nnz=int(row.shape[0]), iters=ITERS, alpha=ALPHA,
                                 row=np.ascontiguousarray(row, np.int32), col=np.ascontiguousarray(col, np.int32), val=val)


def shape_env(shape, bands):
    env = {"MF_ITER_MODE": "sweeps", "MF_SWEEP_BANDS": bands}   # sweeps: small factors would run errors + streams instead
    if SHAPES[shape][4]:
        env["MF_SWEEP_NCH"] = SHAPES[shape][4]
    return env


def both_generations(plan):
    """(L, R) of the current generation and of the one before it (the other buffers)."""
    cur = plan.download()
    plan.flip()
    prev = plan.download()
    plan.flip()
    return cur, prev


def run_plan(capi, inst, iters=ITERS, prepare=None, weight=None, **plan_kw):
    """describe() in front of and behind `iters` iterations from the reference's initial factors, and both generations."""
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val, weight=weight, **plan_kw)
    try:
        if prepare:
            prepare(plan)
        plan.upload(L0, R0)
        before = plan.describe()
        plan.iterate(iters)
        cur, prev = both_generations(plan)
        return before, plan.describe(), cur, prev
    finally:
        plan.close()


_oracle_cache, _single_cache = {}, {}


def oracle_generations(orc, shape):
    """The oracle's factors after ITERS and after ITERS - 1 iterations, computed once per shape."""
    if shape not in _oracle_cache:
        inst = instance(shape)
        out = []
        for iters in (ITERS, ITERS - 1):
            L, R = orc.init_factors(inst.users, inst.items, inst.feats)
            orc.factorize(inst, L, R, iters=iters)
            out.append((L, R))
        _oracle_cache[shape] = out
    return _oracle_cache[shape]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def told_bands(desc):
    """The band count a plan describes: user_bands=N, 0 when it tells none."""
    for tok in desc.split():
        if tok.startswith("user_bands="):
            return int(tok.split("=")[1])
    return 0


@gpu
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bands_give_the_bits_of_one_launch_and_of_the_oracle(capi, orc, monkeypatch, shape, bands):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    inst = instance(shape)
    n = band_counts(inst.items)[bands]
    if shape not in _single_cache:
        clean_env(monkeypatch, **shape_env(shape, 0))
        _single_cache[shape] = run_plan(capi, inst)
        assert told_bands(_single_cache[shape][0]) == 0 and "MF_SWEEP_BANDS=0" in _single_cache[shape][0]
    clean_env(monkeypatch, **shape_env(shape, n))
    before, after, cur, prev = run_plan(capi, inst)
    assert told_bands(before) == n and told_bands(after) == n and "iterate=sweeps" in before, before
    _, _, cur1, prev1 = _single_cache[shape]
    oracle = oracle_generations(orc, shape)
    for name, got, one, want in (("current", cur, cur1, oracle[0]), ("previous", prev, prev1, oracle[1])):
        for side in (0, 1):
            assert same_bits(got[side], one[side]), "%s %s of %s in %d bands differs from one launch" % (name, "LR"[side], shape, n)
            assert same_bits(got[side], want[side]), "%s %s of %s in %d bands differs from the oracle" % (name, "LR"[side], shape, n)


def test_rowlist_shape_is_dispatched_through_a_rowlist(tmp_path_factory):
    """The `rowlist` shape has the row count at which dispatch_order (mf_schedule.h) lists all rows longest first."""
    exe = str(tmp_path_factory.mktemp("order") / "order_main")
    src = tmp_path_factory.mktemp("order_src") / "order_main.cpp"
    src.write_text('#include <cstdio>\n#include "%s"\n'
                   'int main(int, char **argv) {\n'
                   '  FILE *f = fopen(argv[1], "r"); int n = 0, K = 0; long long nnz = 0;\n'
                   '  if (!f || fscanf(f, "%%d %%d %%lld", &n, &K, &nnz) != 3) return 2;\n'
                   '  std::vector<int> ptr((size_t) n + 1);\n'
                   '  for (int &v : ptr) if (fscanf(f, "%%d", &v) != 1) return 2;\n'
                   '  mf_sched::Problem pb; pb.K = K; pb.nnz = nnz;\n'
                   '  mf_sched::Rows rows{ptr.data(), n}; mf_sched::Side s; s.max_row_len = rows.longest();\n'
                   '  mf_sched::dispatch_order(pb, rows, s);\n'
                   '  printf("%%d %%zu\\n", (int) s.lpt, s.short_rows.size());\n'
                   '  return 0;\n}\n' % os.path.join(ROOT, "recommender-system_amd", "csrc", "mf_schedule.h"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src)])
    for shape, want in (("rowlist", "1 600"), ("k10", "0 0")):
        inst = instance(shape)
        ptr = np.concatenate([[0], np.cumsum(np.bincount(inst.row, minlength=inst.users))])
        inp = src.parent / (shape + ".txt")
        inp.write_text("%d %d %d\n%s\n" % (inst.users, inst.feats, inst.nnz, " ".join(map(str, ptr))))
        assert subprocess.run([exe, str(inp)], check=True, capture_output=True, text=True).stdout.strip() == want, shape


# ------------------------------------------------------------------------------------------------ the plans the rule excludes
def weights(inst):
    return 0.5 + np.random.default_rng(7).random(inst.nnz)


EXCLUDED = {
    # name: (prepare(plan), keyword arguments of run_plan)
    "decay": (lambda p: p.set_regularization(0.05, 0.0), {}),
    "momentum": (lambda p: p.set_momentum(0.5, 0.0), {}),
    "frozen": (lambda p: p.set_frozen_columns(3, -1), {}),
    "bounds": (lambda p: p.set_bounds("users", 0.0, 0.08), {}),
    "adaptive": (lambda p: p.set_adaptive("users", "adam", eta=1e-3), {}),
    "weights": (None, {"weight": "weights"}),
    "als": (lambda p: (p.set_regularization(0.05), p.set_als("ridge")), {}),
}
# ... and the user side stays plain under these: the bands run
INCLUDED = {
    "item-decay": lambda p: p.set_regularization(0.0, 0.05),
    "item-momentum": lambda p: p.set_momentum(0.0, 0.5),
    "item-frozen": lambda p: p.set_frozen_columns(-1, 3),
    "item-bounds": lambda p: p.set_bounds("items", 0.0, 0.08),
}


def ab(capi, monkeypatch, inst, shape, forced, **kw):
    """The same run with `forced` bands and with MF_SWEEP_BANDS=0."""
    if kw.get("weight") == "weights":
        kw["weight"] = weights(inst)
    out = []
    for bands in (forced, 0):
        clean_env(monkeypatch, **shape_env(shape, bands))
        out.append(run_plan(capi, inst, **kw))
    return out


def assert_same_run(a, b, where):
    for name, x, y in (("current", a[2], b[2]), ("previous", a[3], b[3])):
        for side in (0, 1):
            assert same_bits(x[side], y[side]), "%s: %s %s differs from MF_SWEEP_BANDS=0" % (where, name, "LR"[side])


@gpu
@pytest.mark.parametrize("case", list(EXCLUDED))
def test_excluded_flavour_runs_no_bands(capi, monkeypatch, case):
    prepare, kw = EXCLUDED[case]
    inst = instance("k10")
    a, b = ab(capi, monkeypatch, inst, "k10", 4, prepare=prepare, iters=2, **kw)
    assert told_bands(a[0]) == 0 and told_bands(a[1]) == 0 and "MF_SWEEP_BANDS=4" in a[0], a[0]
    assert_same_run(a, b, case)


@gpu
@pytest.mark.parametrize("case", list(INCLUDED))
def test_item_side_rules_leave_the_user_bands(capi, monkeypatch, case):
    inst = instance("k10")
    a, b = ab(capi, monkeypatch, inst, "k10", 4, prepare=INCLUDED[case], iters=2)
    assert told_bands(a[0]) == 4 and told_bands(a[1]) == 4, a[0]
    assert_same_run(a, b, case)


@gpu
def test_rule_changed_between_iterations(capi, monkeypatch):
    """The rule is read at every launch: bands, then a decayed sweep in one launch, then bands again."""
    inst = instance("k10")
    runs = []
    for bands in (4, 0):
        clean_env(monkeypatch, **shape_env("k10", bands))
        L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, inst.row, inst.col, inst.val)
        plan.upload(L0, R0)
        told = []
        for lam in (0.0, 0.05, 0.0):
            plan.set_regularization(lam, 0.0)
            told.append(told_bands(plan.describe()))
            plan.iterate(1)
        runs.append((told, both_generations(plan)))
        plan.close()
    assert runs[0][0] == [4, 0, 4] and runs[1][0] == [0, 0, 0]
    for g in (0, 1):
        for side in (0, 1):
            assert same_bits(runs[0][1][g][side], runs[1][1][g][side])


@gpu
def test_unsorted_file_runs_no_bands(capi, monkeypatch):
    """Item ids not ascending inside the rows: the plan keeps the file order, the band cut needs ascending ids."""
    inst = instance("k10")
    rng = np.random.default_rng(11)
    order = np.lexsort((rng.random(inst.nnz), inst.row))      # rows in order, the entries of a row shuffled
    shuffled = types.SimpleNamespace(**{**vars(inst), "col": np.ascontiguousarray(inst.col[order]), "val": np.ascontiguousarray(inst.val[order])})
    assert (np.diff(shuffled.col)[np.diff(shuffled.row) == 0] < 0).any()
    a, b = ab(capi, monkeypatch, shuffled, "k10", 4, iters=2)
    assert told_bands(a[0]) == 0 and told_bands(a[1]) == 0, a[0]
    assert_same_run(a, b, "unsorted")


@gpu
def test_unseeded_user_sweep_of_a_shard_keeps_one_launch(capi, orc, monkeypatch):
    """A shard of the users whose user sweep is launched unseeded (the non-root contribution of a 2-D grid): one launch, no
    bands told, the bits of MF_SWEEP_BANDS=0 and of the oracle's tile step; a seeded sweep of the same plan runs the bands."""
    inst = instance("k10")
    u0, uc = 100, 150
    keep = (inst.row >= u0) & (inst.row < u0 + uc)
    row, col, val = inst.row[keep], inst.col[keep], inst.val[keep]
    L0, R0 = capi.init_factors(inst.users, inst.items, inst.feats)
    got = {}
    for bands in (4, 0):
        clean_env(monkeypatch, **shape_env("k10", bands))
        plan = capi.Plan(inst.users, inst.items, inst.feats, inst.alpha, row, col, val, user_begin=u0, user_count=uc)
        plan.upload(L0[u0:u0 + uc], R0)
        assert told_bands(plan.describe()) == bands
        for seeded in (False, True):
            plan.sweep_users(seed_from_old=seeded)
            plan.flip()
            got[bands, seeded] = (plan.download(want_r=False)[0], told_bands(plan.describe()))
            plan.flip()
        plan.close()
    assert got[4, False][1] == 0 and got[4, True][1] == 4 and got[0, False][1] == 0 and got[0, True][1] == 0
    for seeded in (False, True):
        assert same_bits(got[4, seeded][0], got[0, seeded][0]), seeded
        want = orc.tile_step(u0, uc, 0, inst.items, inst.feats, row, col, val, inst.alpha, L0[u0:u0 + uc].copy(), R0, seeded, True)[0]
        assert same_bits(got[4, seeded][0], want), seeded
