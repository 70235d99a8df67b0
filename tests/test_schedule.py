"""The sweep schedule (csrc/mf_schedule.h) pinned on a golden recorded from the library BEFORE the rules became pure
functions (tests/golden/sweep_schedule.json; profiles/sweep_schedule/ keeps how it was recorded).  No order and no form
of a sweep changes a bit of the factors, so no parity test can see a wrong schedule rule: this file is what pins them.

CPU test: tests/schedule_main.cpp includes only mf_schedule.h; it gets each case's two row-pointer arrays, K, the switches
and the capability values the recording library saw, and prints every scalar and every table of the decision.
GPU test: the plan of every case describes itself as the recording library did (plans are created, no sweep runs)."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

GOLDEN_FILE = os.path.join(GOLDEN, "sweep_schedule.json")
# kernel constants of the resident streams launch (mf_resident.hip.h) the workgroup table is cut by
RESIDENT = dict(waves=8, rows=63, wave_lds=4608)
FREE_BYTES = 256 << 30   # where the recording library never asked: any figure, the cap is not consulted
LONG_LIST = 300          # lists longer than this are stored and compared by their SHA-256


# ---------------------------------------------------------------------------------------------------- the instances
def _sorted(row, col):
    order = np.lexsort((col, row))
    return np.ascontiguousarray(row[order], np.int32), np.ascontiguousarray(col[order], np.int32)


def shape_uniform():
    """600 x 520, density 0.1: no skew anywhere."""
    rng = np.random.default_rng(101)
    row, col = np.nonzero(rng.random((600, 520)) < 0.1)
    return 600, 520, row.astype(np.int32), col.astype(np.int32)


def shape_hot_item():
    """2000 x 300, ~3e4 entries: users of 8..21 entries, item 0 rated by 1500 users."""
    U, I = 2000, 300
    rng = np.random.default_rng(202)
    lens = rng.integers(8, 22, U)
    row = np.repeat(np.arange(U), lens)
    col = np.concatenate([rng.choice(np.arange(1, I), int(n), replace=False) for n in lens])
    hot = np.sort(rng.choice(U, 1500, replace=False))
    return (U, I) + _sorted(np.concatenate([row, hot]), np.concatenate([col, np.zeros(1500, np.int64)]))


def shape_pair_rule():
    """The 8000 x 1500 instance of test_gpu_parity.test_wave_pair_rule_and_extreme_rows_beside_it."""
    U, I = 8000, 1500
    rng = np.random.default_rng(4242)
    pop = (np.arange(I) + 1.0) ** -1.1
    pop /= pop.sum()
    lens = np.clip((rng.pareto(1.3, U) * 18 + 12).astype(np.int64), 4, 900)
    rows, cols = [], []
    for u in range(U):
        c = np.unique(np.concatenate([[0], rng.choice(I, int(lens[u]), replace=False, p=pop)]))
        rows.append(np.full(len(c), u, np.int32))
        cols.append(c.astype(np.int32))
    return U, I, np.concatenate(rows), np.concatenate(cols)


def shape_long_user():
    """5000 x 200, 8 entries per user on average, user 1234 with 190."""
    U, I = 5000, 200
    rng = np.random.default_rng(404)
    lens = rng.integers(4, 13, U)
    lens[1234] = 190
    row = np.repeat(np.arange(U, dtype=np.int32), lens)
    col = np.concatenate([np.sort(rng.choice(I, int(n), replace=False)) for n in lens]).astype(np.int32)
    return U, I, row, col


def shape_large_skewed():
    """The 40000 x 300 instance of test_gpu_parity.test_dispatch_order_of_a_large_skewed_sweep."""
    U, I = 40000, 300
    rng = np.random.default_rng(77)
    lens = rng.integers(20, 41, U)
    lens[rng.choice(U, 60, replace=False)] = rng.integers(250, 301, 60)
    row = np.repeat(np.arange(U, dtype=np.int32), lens)
    col = np.concatenate([np.sort(rng.choice(I, int(n), replace=False)) for n in lens]).astype(np.int32)
    return U, I, row, col


def shape_ml100k_like():
    """943 x 1682 with 1e5 entries at random places."""
    U, I = 943, 1682
    cell = np.sort(np.random.default_rng(808).choice(U * I, 100000, replace=False))
    return U, I, (cell // I).astype(np.int32), (cell % I).astype(np.int32)


def shape_empty():
    return 50, 40, np.zeros(0, np.int32), np.zeros(0, np.int32)


SHAPES = dict(uniform=shape_uniform, hot_item=shape_hot_item, pair_rule=shape_pair_rule, long_user=shape_long_user,
              large_skewed=shape_large_skewed, ml100k_like=shape_ml100k_like, empty=shape_empty)

# name -> (shape, K, switches, user_count or None for all users)
CASES = {
    "a": ("uniform", 100, {}, None),
    "b-K50": ("hot_item", 50, {}, None),
    "b-K30": ("hot_item", 30, {}, None),
    "c": ("pair_rule", 100, {}, None),
    "d": ("long_user", 20, {}, None),
    "e": ("large_skewed", 100, {}, None),
    "f-db1": ("pair_rule", 100, {"MF_SWEEP_DB": "1"}, None),
    "f-pair0": ("pair_rule", 100, {"MF_SWEEP_PAIR": "0"}, None),
    "f-pair1": ("pair_rule", 100, {"MF_SWEEP_PAIR": "1"}, None),
    "f-skew0": ("pair_rule", 100, {"MF_SWEEP_SKEW": "0"}, None),
    "f-long500": ("pair_rule", 100, {"MF_SWEEP_LONG": "500"}, None),
    "f-nch7": ("pair_rule", 100, {"MF_SWEEP_NCH": "7"}, None),
    "g-uniform": ("uniform", 101, {}, None),
    "g-skewed": ("pair_rule", 101, {}, None),
    "h-K10": ("ml100k_like", 10, {}, None),
    "h-K100": ("ml100k_like", 100, {}, None),
    "i-no-entries": ("empty", 100, {}, None),
    "i-no-users": ("empty", 100, {}, 0),
}

_shape_cache = {}


def instance(case):
    """(users_total, items, user_count, row, col, K, switches) of a case; the shapes are generated once."""
    shape, K, env, uc = CASES[case]
    if shape not in _shape_cache:
        _shape_cache[shape] = SHAPES[shape]()
    U, I, row, col = _shape_cache[shape]
    return U, I, U if uc is None else uc, row, col, K, env


def row_pointers(nrows, key):
    return np.concatenate([[0], np.cumsum(np.bincount(key, minlength=nrows)[:nrows])]).astype(np.int64)


def set_switches(monkeypatch, env):
    """This file's own switch handling: every MF_* switch cleared (MF_HIP_LIB names the library, it is no switch)."""
    for k in list(os.environ):
        if k.startswith("MF_") and k != "MF_HIP_LIB":
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------- the dump format and its digest
def parse_dump(text):
    """The line format both the recording dump and schedule_main print -> one dict per plan.  Scalars in full; a list in
    full up to LONG_LIST entries, else {"n", "sha256"} of its decimal text."""
    names = dict(
        plan=["K", "nnz", "items", "uc"],
        caps=["prod", "pf", "pair", "coop", "db", "row_bytes", "xs_bytes", "single_nch"],
        consts=["coop_producers", "coop_waves", "slice_cols", "block_entries", "wave", "lds_per_cu"],
        switches=["skew", "sweep_nch", "sweep_long_set", "sweep_long", "sweep_pair", "sweep_db"],
        side=["nrows", "max_row_len", "prio_len", "lpt", "n_long", "n_short", "long_len", "n_seg", "coop_all", "use_db", "use_pair"],
        sched=["coop_nch", "coop_lds", "coop_block", "scratch_entries", "prod_nch", "prod_lds"],
        es_in=["enabled", "res_sw"],
        es=["es_mode", "es_nch", "es_lds_errors", "es_nseg", "res_sw", "res_nwg", "res_lds"],
    )
    plans, cur = [], None
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        key, vals = w[0], w[1:]
        if key == "plan":
            cur = {}
            plans.append(cur)
        if key == "side":
            cur["side%s" % vals[0]] = dict(zip(names["side"], map(int, vals[1:])))
        elif key == "free":
            cur.setdefault("free", {})[vals[0]] = int(vals[1])
        elif key in ("side_low", "ncu"):
            cur[key] = int(vals[0])
        elif key in names:
            cur[key] = {n: (float(v) if n == "sweep_long" else int(v)) for n, v in zip(names[key], vals)}
        else:   # a list: name, count, entries
            assert int(vals[0]) == len(vals) - 1, line[:80]
            body = " ".join(vals[1:])
            cur.setdefault("lists", {})[key] = ([int(v) for v in vals[1:]] if len(vals) - 1 <= LONG_LIST else
                                               {"n": len(vals) - 1, "sha256": hashlib.sha256(body.encode()).hexdigest()})
    return plans


def program_input(case, gold, free_bytes=None):
    """The text schedule_main reads: the recorded capabilities, limits and switches, then the two row-pointer arrays."""
    U, I, uc, row, col, K, _ = instance(case)
    cptr, rptr = row_pointers(I, col), row_pointers(uc, row)
    g = gold
    free = min(g.get("free", {"-": FREE_BYTES}).values()) if free_bytes is None else free_bytes
    head = [K, len(row), I, uc] + [g["caps"][n] for n in ("prod", "pf", "pair", "coop", "db", "row_bytes", "xs_bytes", "single_nch")]
    head += [g["consts"][n] for n in ("coop_producers", "coop_waves", "slice_cols", "block_entries", "wave", "lds_per_cu")]
    s = g["switches"]
    head += [s["skew"], s["sweep_nch"], s["sweep_long_set"], repr(float(s["sweep_long"])), s["sweep_pair"], s["sweep_db"]]
    head += [free, g["es_in"]["enabled"], g["es_in"]["res_sw"], g.get("ncu", 256), RESIDENT["rows"], RESIDENT["wave_lds"]]
    return " ".join(map(str, head)) + "\n" + " ".join(map(str, cptr)) + "\n" + " ".join(map(str, rptr)) + "\n"


# ---------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schedule") / "schedule_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "schedule_main.cpp")])
    return exe


def test_the_golden_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


def test_the_generators_are_deterministic():
    for name, make in SHAPES.items():
        a, b = make(), make()
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), name


@pytest.mark.parametrize("case", list(CASES))
def test_schedule_rules_give_the_recorded_decision(program, golden, case, tmp_path):
    gold = golden["cases"][case]["schedule"]
    inp = tmp_path / "input.txt"
    inp.write_text(program_input(case, gold))
    out = subprocess.run([program, str(inp)], check=True, capture_output=True, text=True).stdout
    (got,) = parse_dump(out)
    for key in ("side0", "side1", "sched", "es"):
        want = {k: v for k, v in gold[key].items() if k in got[key]} if key == "sched" else gold[key]
        assert got[key] == want, (case, key, got[key], want)
    assert got.get("side_low") == gold.get("side_low"), case
    assert sorted(got.get("lists", {})) == sorted(gold.get("lists", {})), case
    for name, want in gold.get("lists", {}).items():
        assert got["lists"][name] == want, (case, name)


def test_scratch_cap_raises_the_threshold(program, golden, tmp_path):
    """The cap no recording can reach (it would need a nearly full device): the scratch may hold a quarter of the free bytes,
    at 8 bytes x K rounded up to whole 8-column slices per entry.  Case d's one extreme row has 190 entries at K = 20 (three
    slices, 192 bytes per entry): with room for 190 entries it stays extreme, with room for 189 the threshold doubles past
    it, nothing is split and the side gets its dispatch order instead."""
    gold = golden["cases"]["d"]["schedule"]
    inp = tmp_path / "input.txt"
    for entries, n_long in ((190, 1), (189, 0)):
        inp.write_text(program_input("d", gold, free_bytes=4 * 192 * entries))
        (got,) = parse_dump(subprocess.run([program, str(inp)], check=True, capture_output=True, text=True).stdout)
        assert got["side1"]["n_long"] == n_long and got["side1"]["lpt"] == 1 - n_long, (entries, got["side1"])
        assert got["sched"]["scratch_entries"] == (190 + gold["consts"]["block_entries"]) * n_long, (entries, got["sched"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_plan_describes_itself_as_recorded(capi, golden, case, monkeypatch):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    U, I, uc, row, col, K, env = instance(case)
    set_switches(monkeypatch, env)
    val = np.ones(len(row), np.float64)
    plan = capi.Plan(U, I, K, 1e-4, row, col, val, user_begin=0, user_count=uc)
    desc = plan.describe()
    plan.close()
    assert desc == golden["cases"][case]["describe"], case
