"""How an iteration runs (csrc/mf_schedule.h: iterate_path, toy_lds_bytes, toy_kmax) against its truth table, written out
here and independent of the header.

CPU tests in the manner of test_launch_choice.py: tests/iterate_path_main.cpp includes only mf_schedule.h, reads cases from
stdin and prints one line per case.  The cases are every combination of the rule's eight boolean inputs crossed with each
bound at, and one past, its edge -- 86016 of them.  A second mode prints toy_lds_bytes and toy_kmax of given shapes.

iterate_path_of / path_of_plan are what the GPU tests of the feature modules ask which loop a call of theirs runs in: the
library tells nobody (timing apart), so a test that claims the toy loop or the graph path asserts it through the rule the
library itself consults, with every term of it, instead of restating two of them.

GPU test: iteration counts at the edges of the rule, on the smallest instances each loop exists on, bit for bit against the
oracle or the adaptive model after the path is asserted."""
import atexit
import functools
import itertools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits, device, switches  # noqa: F401

gpu = pytest.mark.gpu

LOOPS = ("als", "toy", "es", "sweeps")   # mf_sched::Loop, in the enum's order
GRAPH_ITERS = 32
FLAGS = ("als", "whole", "timing", "adaptive", "es", "extreme", "resident", "graph")
INPUTS = ("rows", "bytes", "nnz", "K", "iters") + FLAGS + ("graph_max",)
ROWS = (0, 1, 1024, 1025)
BYTES = (60 * 1024, 60 * 1024 + 1)
WORK = (512, 513)                 # nnz * K, as nnz at K = 1
GRAPH_MAX_MINUS_WORK = (1, 0, -1)   # nnz * K one below MF_GRAPH_MAX, equal to it, one above
ITERS = (0, 7, 8, 127, 128, 129, 160)


def expected(c):
    """The truth table: (loop, replays, eager) of one case."""
    iters, work = c["iters"], c["nnz"] * c["K"]
    if c["als"]:
        return "als", 0, iters
    fits = c["whole"] and 0 < c["rows"] <= 1024 and c["bytes"] <= 61440 and work <= 512
    if fits and not c["timing"] and iters >= 8 and c["resident"] and not c["adaptive"]:
        return "toy", 0, iters
    loop = "es" if c["es"] and not c["adaptive"] else "sweeps"
    if work < c["graph_max"] and not c["timing"] and not c["extreme"] and iters >= 128 and c["graph"]:
        return loop, iters // 32, iters % 32
    return loop, 0, iters


@functools.lru_cache(maxsize=None)
def program():
    """tests/iterate_path_main.cpp, compiled once per process"""
    tmp = tempfile.mkdtemp(prefix="iterate_path")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "iterate_path_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "iterate_path_main.cpp")])
    return exe


def run_program(mode, lines):
    out = subprocess.run([program(), mode], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True)
    return out.stdout.splitlines()


def _parse(line):
    left, right = line.split(":")
    f = left.split()
    c = dict(zip(INPUTS, [int(v) for v in f[:-1]] + [float(f[-1])]))
    loop, replays, eager = map(int, right.split())
    return c, (LOOPS[loop], replays, eager)


def toy_lds_bytes(users, items, K, nnz, weighted=False):
    """mf_sched::toy_lds_bytes of a shape"""
    return int(run_program("shape", ["%d %d %d %d %d 64" % (users, items, K, nnz, weighted)])[0].split()[0])


def iterate_path_of(users, items, K, nnz, iters, *, weighted=False, timing=False, adaptive=False, als=False, es=False, extreme=False,
                    whole=True, env=None):
    """(loop, replays, eager) of mf_plan_iterate(iters) on a plan of this shape: `timing` as plan.timing was set, `adaptive` any
    side with an adaptive rule, `als` an ALS kind, `es` / `extreme` what the plan's description says (path_of_plan reads them),
    the switches MF_RESIDENT, MF_GRAPH and MF_GRAPH_MAX from `env`, the test's environment dictionary, read as the library
    reads them.  `weighted` is the plan's and alters nothing: the rule looks at the unweighted footprint."""
    env = env or {}
    off = lambda k: env.get(k, "")[:1] == "0"   # noqa: E731
    line = "%d %d %d %d %d %d %d %d %d %d %d %d %d %r" % (users, items, nnz, K, iters, als, whole, timing, adaptive, es, extreme,
                                                        not off("MF_RESIDENT"), not off("MF_GRAPH"), float(env.get("MF_GRAPH_MAX", 2e6)))
    c, path = _parse(run_program("plan", [line])[0])
    assert (c["rows"], c["nnz"], c["K"], c["iters"]) == (users + items, nnz, K, iters), (line, c)
    return path


def described_path_inputs(desc, users, items):
    """the two inputs of the rule that only a plan's description tells.  Errors + streams where iterate= says so.  Extreme rows
    where long_rows=<items>/<users> counts some on a side: a side's count is its n_long, or all its rows where the side is one
    cooperative launch (coop_nch != 0 says that some side is), and a side with extreme rows never has all its rows among them
    -- the schedule only lists rows of at least four times the mean length unless MF_SWEEP_LONG sets the length, and then no
    side is cooperative.  The register-staged form (sweep_kernel<, odd K) has no extreme-row path and no such count."""
    m = re.search(r" long_rows=(\d+)/(\d+) ", desc)
    assert m or desc.startswith("sweep_kernel<"), desc
    counts = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
    coop = bool(m) and " coop_nch=0 " not in desc
    extreme = any(n > 0 and not (coop and n == rows) for n, rows in zip(counts, (items, users)))
    return dict(es=" iterate=errors+resident-streams(" in desc, extreme=extreme)


def path_of_plan(desc, pat, K, iters, env=None, **kw):
    """iterate_path_of for a whole-instance plan of the pattern `pat` with the description `desc`"""
    return iterate_path_of(pat.users, pat.items, K, pat.nnz, iters, env=env, **described_path_inputs(desc, pat.users, pat.items), **kw)


# ------------------------------------------------------------------------------------------------ CPU: the rule
def product():
    for flags in itertools.product((0, 1), repeat=len(FLAGS)):
        for rows, nbytes, work, rel, iters in itertools.product(ROWS, BYTES, WORK, GRAPH_MAX_MINUS_WORK, ITERS):
            yield (rows, nbytes, work, 1, iters) + flags + (float(work + rel),)


@pytest.fixture(scope="module")
def cases():
    """[(inputs as the program read them, (loop, replays, eager))]"""
    lines = ["%d %d %d %d %d " % c[:5] + " ".join(map(str, c[5:13])) + " %r" % c[13] for c in product()]
    return [_parse(line) for line in run_program("path", lines)]


def test_every_combination_is_enumerated_once(cases):
    want = set(product())
    got = [tuple(c[k] for k in INPUTS) for c, _ in cases]
    assert len(got) == len(want) == 256 * 4 * 2 * 2 * 3 * 7 and set(got) == want


def test_the_path_is_the_truth_table(cases):
    for c, got in cases:
        assert got == expected(c), (c, got, expected(c))
        assert got[1] * GRAPH_ITERS + got[2] == c["iters"], (c, got)


def test_outcomes_no_call_may_have(cases):
    seen = set()
    for c, (loop, replays, eager) in cases:
        seen.add((loop, replays > 0))
        if c["timing"]:
            assert loop != "toy" and replays == 0, c
        if c["adaptive"]:
            assert loop not in ("toy", "es"), c
        if c["extreme"]:
            assert replays == 0, c
        if c["als"]:
            assert (loop, replays) == ("als", 0), c
        else:
            assert loop != "als", c
    # every loop is taken; the two that a graph may hold with and without replays, the other two never with
    assert seen == {("als", False), ("toy", False), ("es", False), ("es", True), ("sweeps", False), ("sweeps", True)}


# ------------------------------------------------------------------------------------------------ CPU: the toy loop's figures
def test_toy_kmax_is_the_ladder():
    shapes = [(K, threads) for K in (4, 5, 16, 17, 32, 33) for threads in (256, 320)]
    got = [int(line.split()[1]) for line in run_program("shape", ["1 1 %d 0 0 %d" % s for s in shapes])]
    want = {4: (4, 4), 5: (16, 16), 16: (16, 16), 17: (32, 0), 32: (32, 0), 33: (0, 0)}
    assert got == [want[K][threads == 320] for K, threads in shapes]


def test_toy_lds_bytes_of_the_largest_toy_instance():
    """600 + 424 rows at K = 3 with 170 entries (test_weighted's edge instance)"""
    assert toy_lds_bytes(600, 424, 3, 170) == 57400 and toy_lds_bytes(600, 424, 3, 170, True) == 60120


def test_no_toy_instance_has_more_than_256_threads_at_a_k_above_16():
    """what toy_kmax's comment claims: 257 rows or more at K >= 17 are over the rule's 60 KiB even without an entry, so the
    K <= 32 instance, bounded to 256 threads, is never refused a toy launch it would have served"""
    shapes = [(rows, K) for rows in range(257, 1025) for K in range(17, 33)]
    out = run_program("shape", ["%d 0 %d 0 0 %d" % (rows, K, (rows + 63) // 64 * 64) for rows, K in shapes])
    assert len(out) == len(shapes) == 768 * 16
    assert min(int(line.split()[0]) for line in out) == 16 * 257 * 17 + 259 * 4 + 64 > 60 * 1024
    assert {int(line.split()[1]) for line in out} == {0}


def test_the_helper_reads_the_switches_as_the_library_does():
    toy = (6, 5, 3, 12)
    assert iterate_path_of(*toy, 9) == ("toy", 0, 9) and iterate_path_of(*toy, 7) == ("sweeps", 0, 7)
    assert iterate_path_of(*toy, 9, env={"MF_RESIDENT": "0"}) == ("sweeps", 0, 9)
    assert iterate_path_of(*toy, 9, env={"MF_RESIDENT": "1"}) == ("toy", 0, 9)
    assert iterate_path_of(*toy, 9, timing=True) == iterate_path_of(*toy, 9, adaptive=True) == ("sweeps", 0, 9)
    assert iterate_path_of(*toy, 9, whole=False) == ("sweeps", 0, 9) and iterate_path_of(*toy, 9, als=True) == ("als", 0, 9)
    mid = (30, 40, 10, 170)
    assert iterate_path_of(*mid, 130) == ("sweeps", 4, 2) and iterate_path_of(*mid, 130, es=True) == ("es", 4, 2)
    assert iterate_path_of(*mid, 130, env={"MF_GRAPH": "0"}) == iterate_path_of(*mid, 130, extreme=True) == ("sweeps", 0, 130)
    assert iterate_path_of(*mid, 130, env={"MF_GRAPH_MAX": "1700"}) == ("sweeps", 0, 130)
    assert iterate_path_of(*mid, 130, env={"MF_GRAPH_MAX": "1701"}) == ("sweeps", 4, 2)


def test_extreme_rows_are_read_from_a_description_beside_a_cooperative_side():
    desc = "sweep_dma_kernel<KT=30,NPASS=1> K=30 pitch=32/32 nch=16 row_bytes=256 lds=4352 long_rows=%d/%d coop_nch=%d double_buffered=0/0(nch=16) iterate=sweeps"
    users, items = 300, 200
    for counts, coop_nch, want in (((0, 0), 0, False), ((3, 0), 0, True), ((0, 2), 0, True), ((200, 0), 14, False), ((0, 300), 14, False),
                                   ((200, 300), 14, False), ((200, 5), 14, True), ((4, 300), 14, True)):
        assert described_path_inputs(desc % (counts + (coop_nch,)), users, items) == dict(es=False, extreme=want), (counts, coop_nch)
    assert described_path_inputs("sweep_kernel<KT=0,KPMAX=1> K=3 nch=16 stride=4 lds=512 accumulate=plain/plain iterate=sweeps", 6, 5) == \
        dict(es=False, extreme=False)


# ------------------------------------------------------------------------------------------------ GPU: the edges, run
@gpu
def test_iteration_counts_at_the_edges_of_the_rule(device, orc, switches, monkeypatch):
    """Each case asserts its path through the rule, then compares L and R bit for bit: with the oracle, or with test_adaptive's
    model where a side is adaptive.  A timed call is the one place where the path shows: nine launches per side."""
    from test_adaptive import LAM, NUM_U, State, AModel, _bundled, finish, same_state   # these modules import this one
    from test_regularised import Model, _toy, decay
    capi = device

    @functools.lru_cache(maxsize=None)
    def oracle(key, iters):
        pat, K, alpha, val, L0, R0 = shapes[key]
        Lo, Ro = L0.copy(), R0.copy()
        orc.factorize(orc.Instance(iters, alpha, K, pat.users, pat.items, pat.row, pat.col, val), Lo, Ro)
        return Lo, Ro

    def only(env):
        for k in SWITCHES:   # the case before set its own
            monkeypatch.delenv(k, raising=False)
        switches(env)

    def run(key, iters, env, want_path, timing=False):
        pat, K, alpha, val, L0, R0 = shapes[key]
        only(env)
        plan = capi.Plan(pat.users, pat.items, K, alpha, pat.row, pat.col, val)
        try:
            plan.timing(timing)
            where = "%s iterate(%d) %s timing=%s" % (key, iters, env, timing)
            assert path_of_plan(plan.describe(), pat, K, iters, env, timing=timing) == want_path, (where, plan.describe())
            plan.upload(L0, R0)
            plan.iterate(iters)
            L, R = plan.download()
            assert_same_bits(L, oracle(key, iters)[0], where + ": L")
            assert_same_bits(R, oracle(key, iters)[1], where + ": R")
            if timing:
                t = plan.timing_read()
                assert (t["item_launches"], t["user_launches"]) == (iters, iters), (where, t)
        finally:
            plan.close()

    pat, L0, R0, val, alpha = _toy(3)
    inst, Lb, Rb = _bundled()
    mid = Pattern("inst30-40", inst.users, inst.items, inst.row, inst.col)
    assert (mid.users, mid.items, inst.feats, mid.nnz) == (30, 40, 10, 170) and np.array_equal(mid.row, inst.row) and np.array_equal(mid.col, inst.col)
    shapes = {"toy": (pat, 3, alpha, val, L0, R0), "mid": (mid, inst.feats, inst.alpha, inst.val, Lb, Rb)}

    run("toy", 7, {}, ("sweeps", 0, 7))
    run("toy", 8, {}, ("toy", 0, 8))
    run("toy", 9, {}, ("sweeps", 0, 9), timing=True)
    run("mid", 127, {}, ("sweeps", 0, 127))
    run("mid", 128, {}, ("sweeps", 4, 0))
    run("mid", 129, {}, ("sweeps", 4, 1))
    run("mid", 160, {}, ("sweeps", 5, 0))
    run("mid", 128, {"MF_GRAPH": "0"}, ("sweeps", 0, 128))
    run("mid", 128, {"MF_GRAPH_MAX": str(mid.nnz * inst.feats)}, ("sweeps", 0, 128))   # the bound is strict
    run("mid", 128, {"MF_ITER_MODE": "es"}, ("es", 4, 0))

    # the toy shape with one adaptive side: the sweeps, the users by the adaptive model and the items by the plain one
    m = AModel(pat.users, pat.items, pat.row, pat.col, val, alpha)
    L, R, su = L0, R0, State(L0.shape)
    for _ in range(8):
        gu, _ = m.gradients(L, R)
        Ln, su = finish("rmsprop", NUM_U, gu, L, su, decay(alpha, LAM[0]))
        L, R = Ln, Model.step(m, L, R, *LAM)[1]
    only({})
    plan = capi.Plan(pat.users, pat.items, 3, alpha, pat.row, pat.col, val)
    try:
        plan.set_regularization(*LAM)
        plan.set_adaptive("users", "rmsprop", *NUM_U)
        assert path_of_plan(plan.describe(), pat, 3, 8, {}, adaptive=True) == ("sweeps", 0, 8), plan.describe()
        plan.upload(L0, R0)
        plan.iterate(8)
        Lg, Rg = plan.download()
        assert_same_bits(Lg, L, "toy, adaptive users: L")
        assert_same_bits(Rg, R, "toy, adaptive users: R")
        same_state(plan, "users", su, "toy, adaptive users", False)
    finally:
        plan.close()
