"""The plan's stream-ordering contract on a caller-owned stream (mf_plan_set_stream, mf_plan_synchronize, mf_plan_destroy).

Every other GPU test lets a plan keep its own stream and reads back through a synchronising download() straight after the
work: a launch, copy, memset, fork or join of the library that is not ordered on the plan's stream shows there by luck at
best.  Here every plan runs on a non-default torch stream that is BUSY when the library is called, as it is under a
collective ("sweeps and collective on ONE stream"; sharded.py; bench.py --gpus N).

Two instruments.
  Poison  every plan has caller-owned factor buffers (torch, float64, at capi.row_pitch(K): K = 30 has pitch 32 and real
          padding), all NaN: upload() of all-NaN factors arms the plan, torch.full left NaN in the other generation and in
          the padding.  The real inputs reach the buffers through torch copies ON THE STREAM, behind the gate.  Work of the
          library that runs too early therefore reads NaN values -- never an index, a pointer or a size -- and leaves NaN
          where the model has numbers.
  Gate    torch.cuda._sleep on the stream, long enough that everything the host enqueues behind it is still waiting when
          the host is done.  Its length is calibrated once per module (fixture `gate`): 20 times the host time of the
          longest enqueue section here -- the larger of iterate(130) with its graph capture and instantiation and of the
          six iterations of the 3 x 2 grid loop with a stream per plan --, at most 0.5 s.
A gated test is honest through its CONDITION, not through the margin: for calls that only enqueue, the stream and the
gate's own event are still unfinished right after the last call returned; for calls that are complete on return, the call
took at least half the measured gate time on the host clock.  A test whose condition does not hold FAILS as inconclusive.

The consumer is torch on the same stream: clones of the buffers the calls wrote, then NaN over all buffers again (legal: it
is ordered behind the plan's work).  After stream.synchronize() the clones are compared with the models of the other test
modules through assert_same_bits, all elements and the NaN padding, no tolerance.

A  every launch path of the sweeps behind a closed gate      C  many plans in one process: the sharded and the grid loop
B  the passes that are complete on return                    D  set_stream, synchronize, destroy; the drivers' refusals
"""
import functools
import importlib
import re
import time
import types

import numpy as np
import pytest
import torch

from conftest import random_instance
from test_iterate_path import iterate_path_of, path_of_plan
from test_bounded import BOX, NO_BOX, bstep, clip, counts
from test_loss import model_total
from test_momentum import BETA as TOY_BETA
from test_momentum import LAM as TOY_LAM
from test_momentum import MModel
from test_multi_shards import model_run_multi
from test_rank import heldout_for, model_ranks
from test_regularised import LAM_I, LAM_U, _toy, fast_dot, row_squares
from test_regularised import expected as reg_expected
from test_similar import assert_same as assert_similar
from test_similar import model_similar
from test_sweep_edges import SWEEPS, SWITCHES, assert_same_bits, device, expected, pattern, pattern_both_large, signed_inputs, switches  # noqa: F401
from test_topn import _rated_sets, model_topn, planted_instance
from test_topn import assert_same as assert_topn
from test_weighted import WModel, entry_order_sums, plain_weights, wmodel_rows

gpu = pytest.mark.gpu

NAN = float("nan")
LAM = (LAM_U, LAM_I)
BETA = (0.9, 0.5)
LONG = dict(SWEEPS, MF_SWEEP_LONG="24")
ES = {"MF_ITER_MODE": "es"}
GATE_MARGIN, GATE_CAP_MS = 20.0, 500.0
POOL = 8                  # further streams of the module: one per plan of the largest loop (six tiles) and one for the sums
INCONCLUSIVE = ("inconclusive: %s -- the gate (%.1f ms on the device, calibrated from an enqueue section of %.2f ms) did not stay "
                "closed over the calls under test, so their ordering was not exercised")


def cuda():
    return torch.device("cuda", 0)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(cuda())


def padded(X, ld):
    """X in the leading columns of NaN rows of pitch ld: what a caller-owned buffer must hold, padding included"""
    out = np.full((X.shape[0], ld), NAN)
    out[:, :X.shape[1]] = X
    return out


def nan_like(X):
    return np.full(X.shape, NAN)


# ------------------------------------------------------------------------------------------------ poison
class Buffers:
    """The caller-owned factor buffers of one plan: two generations per side at the library's pitch, NaN everywhere."""

    def __init__(self, capi, users, items, K):
        self.K, self.ld = K, capi.row_pitch(K)
        self.l = [torch.full((users, self.ld), NAN, dtype=torch.float64, device=cuda()) for _ in range(2)]
        self.r = [torch.full((items, self.ld), NAN, dtype=torch.float64, device=cuda()) for _ in range(2)]
        self.by_ptr = {int(t.data_ptr()): t for t in self.l + self.r}

    def plan_args(self):
        pitch = 0 if self.ld == self.K else self.ld          # 0 declares K; a declared pitch has to be even
        return dict(items_ext=[t.data_ptr() for t in self.r], items_pitch=pitch, users_ext=[t.data_ptr() for t in self.l],
                    users_pitch=pitch)

    def cur(self, plan):
        return self.by_ptr[int(plan.users_current_ptr())], self.by_ptr[int(plan.items_current_ptr())]

    def nxt(self, plan):
        return self.by_ptr[int(plan.users_next_ptr())], self.by_ptr[int(plan.items_next_ptr())]

    def write(self, plan, L, R, Lp=None, Rp=None):
        """torch copies of device tensors into the current generation (and the previous one into the next-generation buffers),
        on torch's current stream"""
        K = self.K
        cl, cr = self.cur(plan)
        cl[:, :K].copy_(L)
        cr[:, :K].copy_(R)
        nl, nr = self.nxt(plan)
        if Lp is not None:
            nl[:, :K].copy_(Lp)
        if Rp is not None:
            nr[:, :K].copy_(Rp)

    def clones(self, plan):
        """(current L, current R, next L, next R), cloned on torch's current stream"""
        return [t.clone() for t in self.cur(plan) + self.nxt(plan)]

    def poison(self):
        for t in self.l + self.r:
            t.fill_(NAN)


def poisoned_plan(capi, users_total, items, K, alpha, row, col, val, **kw):
    """(plan, buffers): caller-owned NaN buffers, have_factors armed by one upload of all-NaN factors"""
    count = kw.get("user_count", users_total)
    bufs = Buffers(capi, count, items, K)
    torch.cuda.synchronize()                                  # the fills are done before the plan's own stream uploads
    plan = capi.Plan(users_total, items, K, alpha, row, col, val, **kw, **bufs.plan_args())
    try:
        assert plan.pitches() == (bufs.ld, bufs.ld)
        plan.upload(np.full((count, K), NAN), np.full((items, K), NAN))
    except BaseException:
        plan.close()
        raise
    return plan, bufs


# ------------------------------------------------------------------------------------------------ gate
class Gate:
    """cycles == 0 is the open gate of the calibration: nothing is enqueued for it and no condition is applied"""

    def __init__(self, stream, cycles=0, ms=0.0, enqueue_ms=0.0):
        self.s, self.cycles, self.ms, self.enqueue_ms = stream, cycles, ms, enqueue_ms
        self.last_enqueue_ms = 0.0
        self.pool, self._independent = [], None

    def independent(self):
        """A stream of the pool whose work runs while the gate on `s` is closed.  The runtime multiplexes its streams onto a
        few hardware queues, and two streams that share one are serialised whatever the library does: the first stream of
        the pool that finishes a small fill behind a closed gate on `s` is taken, once per module."""
        if self._independent is None:
            for c in self.pool:
                shut = self.close(self.s)
                with torch.cuda.stream(c):
                    probe = torch.zeros(64, dtype=torch.float64, device=cuda())
                c.synchronize()
                ran_beside = not shut.query()
                self.s.synchronize()
                del probe
                if ran_beside:
                    self._independent = c
                    break
            else:
                self.inconclusive("no stream of the pool runs beside the gated one")
        return self._independent

    def close(self, stream=None):
        """the gate on `stream` and an event straight behind it: the gate is closed while the event is unfinished"""
        stream = self.s if stream is None else stream
        with torch.cuda.stream(stream):
            if self.cycles:
                torch.cuda._sleep(self.cycles)
            done = torch.cuda.Event()
            done.record(stream)
        return done

    def inconclusive(self, what):
        if self.cycles:
            pytest.fail(INCONCLUSIVE % (what, self.ms, self.enqueue_ms))


def _sleep_ms(stream, cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        torch.cuda._sleep(cycles)
        b.record(stream)
    stream.synchronize()
    return a.elapsed_time(b)


@pytest.fixture(scope="module")
def gate(device):
    """Calibration, once per module: the device time of torch.cuda._sleep per cycle (two events); the host time of
    iterate(130) of the graph case, which captures and instantiates, on an idle stream (the slower of two calls); the host
    time of the longest enqueue section this module has, the six iterations of the 3 x 2 grid loop with a stream per plan,
    on idle streams (the second of two runs: the first also loads torch's kernels); a gate of GATE_MARGIN times the larger
    of the two, at most GATE_CAP_MS; and the device time of that gate (two events).  The figures are printed."""
    capi = device
    s = torch.cuda.Stream(cuda())
    pool = [torch.cuda.Stream(cuda()) for _ in range(POOL)]      # created once: torch hands out a ring of 32 streams per device
    assert len({st.cuda_stream for st in pool + [s]}) == POOL + 1 and all(st.cuda_stream for st in pool + [s])
    _sleep_ms(s, 1000)
    probe = 2_000_000
    per_ms = probe / _sleep_ms(s, probe)
    mp = pytest.MonkeyPatch()
    plan = None
    try:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        mp.setenv("MF_ITER_MODE", "sweeps")
        x = expected("pair", "signed", 30)
        plan, bufs = poisoned_plan(capi, x.pat.users, x.pat.items, 30, x.alpha, x.pat.row, x.pat.col, x.val)
        plan.set_stream(s.cuda_stream)
        dL, dR = to_dev(x.L0), to_dev(x.R0)
        torch.cuda.synchronize()
        host = []
        for _ in range(2):
            with torch.cuda.stream(s):
                bufs.write(plan, dL, dR)
            s.synchronize()
            t0 = time.perf_counter()
            plan.iterate(130)
            host.append((time.perf_counter() - t0) * 1e3)
            s.synchronize()
        plan.close()
        plan = None
        d, L0, R0 = grid_fixture()
        rows, cols = len(GRID_UB) - 1, len(GRID_IB) - 1
        groups = {"items": [[gr * cols + gc for gr in range(rows)] for gc in range(cols)],
                  "users": [[gr * cols + gc for gc in range(cols)] for gr in range(rows)]}
        loop = []
        for _ in range(2):
            parts = grid_parts(capi, d, GRID_UB, GRID_IB, L0, R0)
            try:
                dry = Gate(s)
                dry.pool = pool
                run_loop(dry, parts, groups, "own")
                loop.append(dry.last_enqueue_ms)
            finally:
                close_parts(parts)
    finally:
        mp.undo()
        if plan is not None:
            plan.close()
    enqueue_ms = max(max(host), loop[1])
    want_ms = min(GATE_CAP_MS, GATE_MARGIN * enqueue_ms)
    cycles = max(int(want_ms * per_ms), 1)
    ms = _sleep_ms(s, cycles)
    print("\nstream_order calibration: _sleep %.1f cycles per ms; iterate(130) enqueue %.3f / %.3f ms on the host; grid loop enqueue "
          "%.3f / %.3f ms; gate of %d cycles asked for %.1f ms, measured %.1f ms on the device"
          % (per_ms, host[0], host[1], loop[0], loop[1], cycles, want_ms, ms))
    gate = Gate(s, cycles, ms, enqueue_ms)
    gate.pool = pool
    return gate


def behind_gate(gate, plan, bufs, L0, R0, calls, where, prev=(None, None)):
    """Steps 1-6 of a gated test of calls that only enqueue: calls(plan, bufs) makes them and may return clones of its own.
    Returns the numpy clones (current L, current R, next L, next R) followed by those."""
    s = gate.s
    dev_in = [None if a is None else to_dev(a) for a in (L0, R0) + tuple(prev)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        shut = gate.close(s)
        bufs.write(plan, *dev_in)
        mid = calls(plan, bufs) or []
        busy = not s.query()                      # host only: nothing is enqueued between the last call and the clones
        got = bufs.clones(plan) + mid
        closed = not shut.query()
        bufs.poison()
    s.synchronize()
    if not (busy and closed):
        gate.inconclusive(where)
    return [t.cpu().numpy() for t in got]


def same_generations(got, gens, ld, where):
    """the clones against the model: the current generation is the last of `gens`, the next-generation buffers hold the one
    before it; NaN padding included"""
    (Ln, Rn), (Lb, Rb) = gens[-1], gens[-2]
    assert np.isfinite(Ln).all() and np.isfinite(Rn).all(), where + ": the model's result has to differ from what NaN inputs give"
    assert_same_bits(got[1], padded(Rn, ld), where + ": current R")
    assert_same_bits(got[0], padded(Ln, ld), where + ": current L")
    assert_same_bits(got[3], padded(Rb, ld), where + ": R of the generation before, in the next-generation buffer")
    assert_same_bits(got[2], padded(Lb, ld), where + ": L of the generation before, in the next-generation buffer")
    if len(got) > 4:                                    # sweeps called one by one: what each had written when it returned
        assert_same_bits(got[5], padded(Rn, ld), where + ": items_next straight after the item sweep")
        assert_same_bits(got[4], padded(Ln, ld), where + ": users_next straight after the user sweep")


# ------------------------------------------------------------------------------------------------ the models
@functools.lru_cache(maxsize=None)
def plain_generations(pat_name, K, iters):
    """[(L0, R0), (L1, R1), ...] of the serial oracle on the "signed" inputs of tests/test_sweep_edges.py"""
    from oracle import oracle as orc
    x = expected(pat_name, "signed", K)
    return oracle_generations(orc, x.pat, K, x.alpha, x.val, x.L0, x.R0, iters)


def oracle_generations(orc, pat, K, alpha, val, L0, R0, iters):
    inst = orc.Instance(1, alpha, K, pat.users, pat.items, pat.row, pat.col, val)
    gens = [(L0, R0)]
    L, R = L0.copy(), R0.copy()
    for _ in range(iters):
        with np.errstate(all="ignore"):
            orc.factorize(inst, L, R, iters=1)
        gens.append((L.copy(), R.copy()))
    return gens


def rule_generations(m, L0, R0, iters, bounds=(NO_BOX, NO_BOX), lam=(0.0, 0.0), beta=(0.0, 0.0), frozen=(-1, -1)):
    """the same from rest under an update rule: test_bounded's bstep over test_momentum's / test_weighted's model"""
    gens, Lp, Rp, L, R = [(L0, R0)], None, None, L0, R0
    for _ in range(iters):
        Ln, Rn = bstep(m, L, R, bounds, Lp, Rp, lam, beta, frozen, dot=fast_dot)
        Lp, Rp, L, R = L, R, Ln, Rn
        gens.append((L, R))
    return gens


def long_rows(desc):
    m = re.search(r" long_rows=(\d+)/(\d+) ", desc)
    return (int(m.group(1)), int(m.group(2))) if m else None


def test_padded_and_the_generation_comparison_can_fail():
    X = np.arange(6.0).reshape(2, 3)
    P = padded(X, 4)
    assert P.shape == (2, 4) and np.isnan(P[:, 3]).all() and np.array_equal(P[:, :3], X)
    gens = [(X, X + 1), (X + 2, X + 3)]
    good = [padded(X + 2, 4), padded(X + 3, 4), padded(X, 4), padded(X + 1, 4)]
    same_generations(good, gens, 4, "identical")
    for t in range(4):
        for r, c, v in ((0, 0, NAN), (1, 3, 0.0), (1, 2, -0.0)):       # a poisoned element, a written padding, a wrong bit
            bad = [a.copy() for a in good]
            bad[t][r, c] = v
            with pytest.raises(AssertionError):
                same_generations(bad, gens, 4, "planted")


# ------------------------------------------------------------------------------------------------ A: the sweeps' launch paths
class Source:
    """inputs of one A case: pattern, factors, ratings, alpha"""

    def __init__(self, pat, L0, R0, val, alpha):
        self.pat, self.L0, self.R0, self.val, self.alpha = pat, L0, R0, val, alpha


@functools.lru_cache(maxsize=None)
def source(name, K):
    if name == "both-large":
        pat = pattern_both_large()
        return Source(pat, *signed_inputs(5000 + K, pat, K), 1e-3)
    if name == "toy":
        return Source(*_toy(K))
    x = expected(name, "signed", K)
    return Source(x.pat, x.L0, x.R0, x.val, x.alpha)


def _no_setup(plan):
    pass


def _iterate(n):
    return lambda plan, bufs: plan.iterate(n)


def _steps(seeded):
    """the two sweeps one by one, each followed at once -- nothing in between -- by a clone of the buffer it wrote: a sweep
    that returned with its extreme rows unjoined shows in the first clone, whatever the second sweep then hides"""
    def calls(plan, bufs):
        plan.sweep_items(seeded)
        r_new = bufs.nxt(plan)[1].clone()
        plan.sweep_users(seeded)
        l_new = bufs.nxt(plan)[0].clone()
        plan.flip()
        return [l_new, r_new]
    return calls


def _one_kernel(K):
    return lambda d: d.startswith("sweep_dma_kernel<KT=%d," % K) and long_rows(d) == (0, 0) and " iterate=sweeps" in d


def _deferred(d):
    """extreme rows on the item side only: mf_plan_iterate leaves their ordered sums running under the user sweep"""
    n = long_rows(d)
    return n is not None and n[0] > 0 and n[1] == 0 and " coop_nch=0 " in d and " iterate=sweeps" in d


def _both_sides(d):
    """extreme rows on both sides: the user sweep would reuse the scratch, so the join is not deferred"""
    n = long_rows(d)
    return n is not None and n[0] > 0 and n[1] > 0 and " coop_nch=0 " in d and " iterate=sweeps" in d


def _plain_large(d):
    """more than 262144 rows of at most 90 entries on both sides: MF_SWEEP_LONG=24 is raised to 128 entries by the rule, so no
    row is extreme and both sweeps are the plain accumulate instance in one launch of 262144+ workgroups"""
    return _one_kernel(30)(d) and " accumulate=plain/plain " in d


def _coop(d):
    n = long_rows(d)
    return n is not None and n != (0, 0) and " coop_nch=0 " not in d and " iterate=sweeps" in d


def _es(d):
    return " iterate=errors+resident-streams(" in d


def _graphed(check):
    """what mf_plan_iterate asks of a plan before it captures: no extreme rows, graphs on, nnz * K below the default bound"""
    return lambda d: check(d) and "MF_GRAPH" not in d and ("long_rows=0/0 " in d)


def _oracle_model(iters):
    return lambda name, K, src: plain_generations(name, K, iters)


def _unseeded_model(name, K, src):
    x = expected(name, "signed", K)
    return [(x.L0, x.R0), x.unseeded]


def _both_large_model(name, K, src):
    from oracle import oracle as orc
    return oracle_generations(orc, src.pat, K, src.alpha, src.val, src.L0, src.R0, 2)


def _rule_model(iters, weights=None, **rule):
    def model(name, K, src):
        pat = src.pat
        if weights is None:
            m = MModel(pat.users, pat.items, pat.row, pat.col, src.val, src.alpha)
        else:
            m = WModel(pat.users, pat.items, pat.row, pat.col, src.val, src.alpha, weights(pat))
        return rule_generations(m, src.L0, src.R0, iters, **rule)
    return model


def _momentum_setup(plan):
    plan.set_momentum(*BETA)


FROZEN = (2, 5)
BOXES = ((0.0, 0.5, -1), (0.0, 0.5, 20))            # users: all columns, items: the leading 20


def _composed_setup(plan):
    plan.set_regularization(*LAM)
    plan.set_frozen_columns(*FROZEN)
    plan.set_bounds("users", *BOXES[0])
    plan.set_bounds("items", *BOXES[1])


def _toy_setup(plan):
    plan.set_regularization(*TOY_LAM)
    plan.set_momentum(*TOY_BETA)


def _weights(pat):
    return plain_weights(7030, pat.nnz)


def _weighted_setup(plan):
    plan.set_regularization(*LAM)


def _case(name, pat, K, env, check, calls, model, setup=_no_setup, weights=None, timed=False, path=None):
    """path: (iters, (loop, replays, eager)) -- what the rule of mf_plan_iterate (test_iterate_path.py) must say of the case's one call"""
    return dict(name=name, pat=pat, K=K, env=env, check=check, calls=calls, model=model, setup=setup, weights=weights, timed=timed, path=path)


def a_cases():
    out = []
    for K in (30, 100):
        out += [_case("one-kernel-per-side-K%d-steps" % K, "pair", K, SWEEPS, _one_kernel(K), _steps(True), _oracle_model(1)),
                _case("one-kernel-per-side-K%d-iterate3" % K, "pair", K, SWEEPS, _one_kernel(K), _iterate(3), _oracle_model(3)),
                _case("unseeded-K%d-steps" % K, "pair", K, SWEEPS, _one_kernel(K), _steps(False), _unseeded_model)]
    for K in (30, 256):
        out += [_case("extreme-rows-join-deferred-K%d-iterate2" % K, "long-items", K, LONG, _deferred, _iterate(2), _oracle_model(2)),
                _case("extreme-rows-K%d-steps" % K, "long-items", K, LONG, _deferred, _steps(True), _oracle_model(1))]
    out += [_case("extreme-rows-both-sides-K30-iterate2", "skewed", 30, LONG, _both_sides, _iterate(2), _oracle_model(2)),
            _case("both-large-K30-iterate2", "both-large", 30, LONG, _plain_large, _iterate(2), _both_large_model),
            _case("cooperative-K30-iterate2", "skewed", 30, SWEEPS, _coop, _iterate(2), _oracle_model(2))]
    for pat, env, check in (("pair", SWEEPS, _one_kernel(30)), ("long-items", LONG, _deferred)):
        out += [_case("momentum-from-rest-%s-K30-iterate3" % pat, pat, 30, env, check, _iterate(3), _rule_model(3, beta=BETA),
                      setup=_momentum_setup),
                _case("momentum-from-rest-%s-K30-steps" % pat, pat, 30, env, check, _steps(True), _rule_model(1, beta=BETA),
                      setup=_momentum_setup)]
    out += [_case("decay-frozen-box-K30-iterate3", "pair", 30, SWEEPS, _one_kernel(30), _iterate(3),
                  _rule_model(3, bounds=BOXES, lam=LAM, frozen=FROZEN), setup=_composed_setup),
            _case("errors-resident-streams-K30-iterate3", "pair", 30, ES, _es, _iterate(3), _oracle_model(3)),
            _case("graph-sweeps-K30-iterate130", "pair", 30, SWEEPS, _graphed(_one_kernel(30)), _iterate(130), _oracle_model(130),
                  path=(130, ("sweeps", 4, 2))),
            _case("graph-es-K30-iterate130", "pair", 30, ES, _graphed(_es), _iterate(130), _oracle_model(130), path=(130, ("es", 4, 2))),
            _case("toy-loop-in-one-launch-K3-iterate9", "toy", 3, {}, lambda d: " iterate=sweeps" in d, _iterate(9),
                  _rule_model(9, lam=TOY_LAM, beta=TOY_BETA), setup=_toy_setup, path=(9, ("toy", 0, 9))),
            _case("weighted-twins-K30-iterate3", "pair", 30, SWEEPS, lambda d: _one_kernel(30)(d) and " weighted=1" in d, _iterate(3),
                  _rule_model(3, weights=_weights, lam=LAM), setup=_weighted_setup, weights=_weights),
            _case("timed-plan-K30-iterate3", "pair", 30, SWEEPS, _one_kernel(30), _iterate(3), _oracle_model(3), timed=True)]
    return out


A_CASES = a_cases()


def test_every_launch_path_of_the_issue_is_in_the_table():
    names = [c["name"] for c in A_CASES]
    assert len(set(names)) == len(names) == 24
    for part in ("one-kernel-per-side-K30-steps", "one-kernel-per-side-K100-iterate3", "unseeded-K100", "join-deferred-K256", "extreme-rows-K30-steps",
                 "both-sides", "both-large", "cooperative", "momentum-from-rest-pair-K30-iterate3", "momentum-from-rest-long-items-K30-steps", "decay-frozen-box",
                 "errors-resident-streams", "graph-sweeps", "graph-es", "toy-loop", "weighted-twins", "timed-plan"):
        assert any(part in n for n in names), part
    # the shapes alone, before a plan says the rest: one launch runs the toy's nine iterations, iterate(130) of the pair captures
    toy, pair = source("toy", 3).pat, source("pair", 30).pat
    assert iterate_path_of(toy.users, toy.items, 3, toy.nnz, 9) == ("toy", 0, 9)
    assert iterate_path_of(pair.users, pair.items, 30, pair.nnz, 130) == ("sweeps", 4, 2)
    assert [c["name"] for c in A_CASES if c["path"]] == ["graph-sweeps-K30-iterate130", "graph-es-K30-iterate130", "toy-loop-in-one-launch-K3-iterate9"]


@gpu
@pytest.mark.parametrize("case", A_CASES, ids=[c["name"] for c in A_CASES])
def test_sweep_launch_paths_behind_a_closed_gate(device, switches, gate, case):
    """One launch path of the sweeps on a busy caller-owned stream: gate, torch writes the inputs, the calls, torch clones
    what they wrote and poisons the buffers again, all without a host synchronisation.  Both generations, padding included,
    are the model's bits."""
    capi = device
    K = case["K"]
    src = source(case["pat"], K)
    pat = src.pat
    gens = case["model"](case["pat"], K, src)
    switches(case["env"])
    w = case["weights"](pat) if case["weights"] else None
    plan, bufs = poisoned_plan(capi, pat.users, pat.items, K, src.alpha, pat.row, pat.col, src.val, weight=w)
    try:
        case["setup"](plan)
        plan.timing(case["timed"])
        desc = plan.describe()
        assert case["check"](desc), desc
        if case["path"]:
            iters, want = case["path"]
            assert path_of_plan(desc, pat, K, iters, case["env"], timing=case["timed"], weighted=w is not None) == want, desc
        plan.set_stream(gate.s.cuda_stream)
        where = "%s [%s]" % (case["name"], desc.split(" loss=")[0])
        got = behind_gate(gate, plan, bufs, src.L0, src.R0, case["calls"], where)
        same_generations(got, gens, bufs.ld, where)
        if case["timed"]:
            t = plan.timing_read()
            assert (t["item_launches"], t["user_launches"]) == (3, 3) and t["item_ms"] > 0.0 and t["user_ms"] > 0.0, t
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ B: complete on return
B_USERS, B_ITEMS = 150, 300
B_BOX = (-0.5, 0.5)
B_LISTED = np.array([149, 3, 4, 0, 77, 1, 2, 5], np.int32)


class BInstance:
    pass


@functools.lru_cache(maxsize=None)
def b_instance(K):
    x = BInstance()
    x.K = K
    x.row, x.col, x.val, x.L, x.R = planted_instance(K, B_USERS, B_ITEMS, K)
    x.hrow, x.hcol, x.hval = heldout_for(K, B_USERS, B_ITEMS, x.row, x.col)
    x.w = plain_weights(K, len(x.row))
    rng = np.random.default_rng(8800 + K)
    x.Lp, x.Rp = rng.standard_normal(x.L.shape), rng.standard_normal(x.R.shape)
    return x


def model_candidates(orc, x, only=None):
    """mf_candidate per user as include/matfact_hip.h defines it, from exact rows: (best, first, first_nan, score)"""
    rated = _rated_sets(B_USERS, x.row, x.col)
    sel = range(B_USERS) if only is None else [int(u) for u in only]
    best, first, first_nan = (np.full(len(sel), -1, np.int32) for _ in range(3))
    score = np.full(len(sel), NAN)
    for t, i in enumerate(sel):
        b = orc.predict_row(np.ascontiguousarray(x.L[i]), x.R)
        alive = np.ones(B_ITEMS, bool)
        alive[np.asarray(rated[i], np.int64)] = False
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            first_nan[t] = 0
            continue
        first[t], first_nan[t] = idx[0], int(np.isnan(b[idx[0]]))
        cand = idx[~np.isnan(b[idx])]
        if cand.size:
            best[t] = cand[int(np.argmax(b[cand]))]
            score[t] = b[best[t]]
    return best, first, first_nan, score


def same_candidates(cand, model, where):
    best, first, first_nan, score = model
    assert np.array_equal(cand["best"], best) and np.array_equal(cand["first"], first), where
    live = first >= 0
    assert np.array_equal(cand["first_nan"][live] != 0, first_nan[live] != 0), where
    has = best >= 0
    assert np.array_equal(cand["score"][has].view(np.uint64), score[has].view(np.uint64)), where + ": scores"


def _answers(orc, x, L):
    inst = orc.Instance(1, 0.01, x.K, B_USERS, B_ITEMS, x.row, x.col, x.val)
    with np.errstate(all="ignore"):
        return orc.recommend(inst, np.ascontiguousarray(L), x.R)


def check_recommend(got, orc, x, ref):
    want = _answers(orc, x, x.L)
    assert (want != _answers(orc, x, nan_like(x.L))).sum() > B_USERS // 2       # NaN scores give the first unrated item: it can tell
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def check_topn(got, orc, x, ref):
    mi, ms = model_topn(orc, B_USERS, B_ITEMS, x.row, x.col, x.L, x.R, 10)
    ni, _ = model_topn(orc, B_USERS, B_ITEMS, x.row, x.col, nan_like(x.L), x.R, 10)
    assert (mi != ni).any(axis=1).sum() > B_USERS // 2
    assert_topn(got[0], got[1], mi, ms, "recommend_topn(10)")


def check_scored(got, orc, x, ref):
    model = model_candidates(orc, x)
    assert (model[0] != model[1]).sum() > B_USERS // 2                          # best is not simply the first unrated item
    same_candidates(got, model, "recommend_scored")


def check_scored_users(got, orc, x, ref):
    same_candidates(got, model_candidates(orc, x, B_LISTED), "recommend_scored_users")


def check_filter(got, orc, x, ref):
    """pass 1 alone has no bit-exact CPU model (its scores are the matrix cores'): the report is the bits of the same call on a
    plan that was never on a busy stream, and what it certifies is the oracle's answer"""
    sh = importlib.import_module("recommender_system_amd.sharded")
    capi = importlib.import_module("recommender_system_amd").capi
    f, norm, rmax = got
    rf, rnorm, rrmax = ref.recommend_filter()
    assert f.tobytes() == rf.tobytes() and np.array_equal(norm.view(np.uint64), rnorm.view(np.uint64)) and rmax == rrmax
    ans, certain = sh.certify_filters([f], norm, rmax, capi.recommend_margin(x.K))
    want = _answers(orc, x, x.L)
    assert np.array_equal(ans[certain], want[certain]) and not certain[3]       # user 3 is the NaN row
    if x.K == 100:
        assert certain.sum() > B_USERS // 2 and (f["nonfinite"] == 0).sum() > B_USERS // 2   # under NaN factors nobody is certified


def check_ranks(got, orc, x, ref):
    want = model_ranks(orc, B_USERS, B_ITEMS, x.row, x.col, x.L, x.R, x.hrow, x.hcol)
    assert (want >= 0).sum() > len(want) // 2                                   # NaN scores would be MF_RANK_NAN
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def check_similar(metric):
    def check(got, orc, x, ref):
        mi, ms = model_similar(orc, x.R, metric, 10)
        assert (mi >= 0).all()
        assert_similar(got[0], got[1], mi, ms, "similar_items(10, %s)" % metric)
    return check


def _check_loss(got, ms, count, where):
    out, rs = got
    assert out.count == count, (where, out.count)
    assert np.isfinite(ms).sum() > B_USERS // 2
    assert_same_bits(rs, ms, where + ": row_sse")
    assert_same_bits(np.array([out.sse]), np.array([model_total(ms)]), where + ": sse")


def check_loss_train(got, orc, x, ref):
    _check_loss(got, wmodel_rows(x.L, x.R, x.row, x.col, x.val, x.w, B_USERS), len(x.row), "loss(train)")


def check_loss_heldout(got, orc, x, ref):
    _check_loss(got, wmodel_rows(x.L, x.R, x.hrow, x.hcol, x.hval, None, B_USERS), len(x.hrow), "loss(heldout)")


def check_penalty(got, orc, x, ref):
    usq, isq, ur, ir = got
    assert_same_bits(ur, row_squares(x.L), "penalty: user rows")
    assert_same_bits(ir, row_squares(x.R), "penalty: item rows")
    assert_same_bits(np.array([usq, isq]), np.array([model_total(row_squares(x.L)), model_total(row_squares(x.R))]), "penalty: totals")
    assert np.isfinite(isq)


def check_weight_total(got, orc, x, ref):
    total, rows = got
    want = entry_order_sums(x.w, x.row.astype(np.int64), B_USERS)
    assert_same_bits(rows, want, "weight_total: rows")
    assert_same_bits(np.array([total]), np.array([model_total(want)]), "weight_total")


def check_bounds_active(got, orc, x, ref):
    want = counts(x.L, B_BOX[0], B_BOX[1], -1)
    assert got == want and want[2] > 0 and counts(nan_like(x.L), B_BOX[0], B_BOX[1], -1) == (0, 0, 0), (got, want)


def check_predict(got, orc, x, ref):
    with np.errstate(all="ignore"):
        want = np.stack([orc.predict_row(np.ascontiguousarray(x.L[i]), x.R) for i in range(B_USERS)])
    assert_same_bits(got, want, "predict")


def check_download(got, orc, x, ref):
    assert_same_bits(got[0], x.L, "download: L")
    assert_same_bits(got[1], x.R, "download: R")


def check_download_previous(got, orc, x, ref):
    assert_same_bits(got[0], x.Lp, "download_previous: L")
    assert_same_bits(got[1], x.Rp, "download_previous: R")


B_CALLS = {
    "recommend": (lambda p: p.recommend(), check_recommend),
    "recommend_topn": (lambda p: p.recommend_topn(10), check_topn),
    "recommend_scored": (lambda p: p.recommend_scored(), check_scored),
    "recommend_scored_users": (lambda p: p.recommend_scored_users(B_LISTED), check_scored_users),
    "recommend_filter": (lambda p: p.recommend_filter(), check_filter),
    "rank_heldout": (lambda p: p.rank_heldout(), check_ranks),
    "similar_items-cosine": (lambda p: p.similar_items(10, "cosine"), check_similar("cosine")),
    "similar_items-dot": (lambda p: p.similar_items(10, "dot"), check_similar("dot")),
    "loss-train": (lambda p: p.loss("train", rows=True), check_loss_train),
    "loss-heldout": (lambda p: p.loss("heldout", rows=True), check_loss_heldout),
    "penalty": (lambda p: p.penalty(rows=True), check_penalty),
    "weight_total": (lambda p: p.weight_total(rows=True), check_weight_total),
    "bounds_active": (lambda p: p.bounds_active("users"), check_bounds_active),
    "predict": (lambda p: p.predict(), check_predict),
    "download": (lambda p: p.download(), check_download),
    "download_previous": (lambda p: p.download_previous(), check_download_previous),
}


@pytest.fixture(scope="module")
def b_plans(device):
    """per K: (the poisoned plan on the gated stream, its buffers, a plan of the same instance with its own buffers and
    stream that holds the good factors); created by the first test that asks, closed with the module"""
    capi = device
    made = {}

    def get(K, stream):
        if K not in made:
            x = b_instance(K)
            plan, bufs = poisoned_plan(capi, B_USERS, B_ITEMS, K, 0.01, x.row, x.col, x.val, weight=x.w)
            ref = capi.Plan(B_USERS, B_ITEMS, K, 0.01, x.row, x.col, x.val, weight=x.w)
            made[K] = (plan, bufs, ref)
            ref.upload(x.L, x.R)
            for p in (plan, ref):
                p.set_heldout(x.hrow, x.hcol, x.hval)
                p.set_bounds("users", *B_BOX)
            plan.upload_previous(nan_like(x.L), nan_like(x.R))     # both sides have a history: the next-generation buffers
            plan.set_stream(stream.cuda_stream)
        return made[K]
    yield get
    for plan, bufs, ref in made.values():
        plan.close()
        ref.close()


@gpu
@pytest.mark.parametrize("name", list(B_CALLS))
@pytest.mark.parametrize("K", [100, 30])
def test_calls_that_are_complete_on_return_behind_a_closed_gate(device, orc, switches, gate, b_plans, K, name):
    """A call that returns data to the host, on a busy caller-owned stream: gate, torch writes the good factors, the call.
    The call took at least half the gate's time, the stream is idle when it returns, and the answer is the model's."""
    switches({})
    x = b_instance(K)
    plan, bufs, ref = b_plans(K, gate.s)
    s = gate.s
    call, check = B_CALLS[name]
    dev_in = [to_dev(a) for a in (x.L, x.R, x.Lp, x.Rp)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gate.close(s)
        bufs.write(plan, *dev_in)
        t0 = time.perf_counter()
        got = call(plan)
        took_ms = (time.perf_counter() - t0) * 1e3
        idle = s.query()
        bufs.poison()
    s.synchronize()
    if took_ms < gate.ms / 2:
        gate.inconclusive("%s K=%d returned after %.2f ms" % (name, K, took_ms))
    assert idle, "%s K=%d returned with work pending on its stream" % (name, K)
    check(got, orc, x, ref)
    if name == "recommend_topn":
        assert plan.recommend_topn_info()[1] == (1 if K == 100 else 0)          # two workgroups per CU on the matrix cores / exact form


# ------------------------------------------------------------------------------------------------ C: many plans in one process
T_LOOP = 6
ROW_CUTS = [0, 25, 61, 90]
GRID_UB, GRID_IB = [0, 25, 61, 90], [0, 31, 70]
PAIR_CUT = 333


@functools.lru_cache(maxsize=None)
def row_fixture():
    """the instance of test_plan_sharded_sweeps_match_oracle_shard_step: 90 x 60, K = 20"""
    from oracle import oracle as orc
    d = random_instance(31, 90, 60, 20, density=0.3, iters=T_LOOP, alpha=0.003)
    return d, *orc.init_factors(90, 60, 20)


@functools.lru_cache(maxsize=None)
def grid_fixture():
    """the instance of test_tile_sweeps_match_oracle_tile_step: 90 x 70, K = 7"""
    from oracle import oracle as orc
    d = random_instance(77, 90, 70, 7, density=0.3, iters=T_LOOP, alpha=0.003)
    return d, *orc.init_factors(90, 70, 7)


@functools.lru_cache(maxsize=None)
def pair_fixture():
    x = reg_expected("pair", "signed", 30)
    pat = x.pat
    d = dict(iters=T_LOOP, alpha=x.alpha, feats=30, users=pat.users, items=pat.items, row=pat.row, col=pat.col, val=x.val)
    return d, x.L0, x.R0


def left_to_right(parts, reverse=False):
    seq = parts[::-1] if reverse else parts
    with np.errstate(all="ignore"):
        acc = seq[0]
        for P in seq[1:]:
            acc = acc + P
    return acc


def shard_entries(d, lo, hi, j0=None, j1=None):
    sel = (d["row"] >= lo) & (d["row"] < hi)
    if j0 is not None:
        sel &= (d["col"] >= j0) & (d["col"] < j1)
    return (np.ascontiguousarray(d["row"][sel], np.int32), np.ascontiguousarray(d["col"][sel], np.int32),
            np.ascontiguousarray(d["val"][sel], np.float64))


def model_row_loop(d, cuts, L0, R0, iters, reverse=False):
    """generations [(L, R), ...] of the row-sharded loop: oracle.shard_step per shard, the partial R added left to right"""
    from oracle import oracle as orc
    K, gens = d["feats"], [(L0, R0)]
    ent = [shard_entries(d, cuts[g], cuts[g + 1]) for g in range(len(cuts) - 1)]
    L, R = L0, R0
    for _ in range(iters):
        Ln, parts = np.empty_like(L), []
        for g, (row, col, val) in enumerate(ent):
            b0, b1 = cuts[g], cuts[g + 1]
            blk, P = orc.shard_step(b0, b1 - b0, d["items"], K, row, col, val, d["alpha"], np.ascontiguousarray(L[b0:b1]), R, g == 0)
            Ln[b0:b1] = blk
            parts.append(P)
        L, R = Ln, left_to_right(parts, reverse)
        gens.append((L, R))
    return gens


def model_grid_loop(d, ub, ib, L0, R0, iters, reverse=False):
    """the same for the grid: oracle.tile_step per tile, R added over the grid column, L over the grid row, both left to right"""
    from oracle import oracle as orc
    K, gens = d["feats"], [(L0, R0)]
    rows, cols = len(ub) - 1, len(ib) - 1
    ent = {(gr, gc): shard_entries(d, ub[gr], ub[gr + 1], ib[gc], ib[gc + 1]) for gr in range(rows) for gc in range(cols)}
    L, R = L0, R0
    for _ in range(iters):
        aux = {}
        for (gr, gc), (row, col, val) in ent.items():
            aux[gr, gc] = orc.tile_step(ub[gr], ub[gr + 1] - ub[gr], ib[gc], ib[gc + 1] - ib[gc], K, row, col, val, d["alpha"],
                                        np.ascontiguousarray(L[ub[gr]:ub[gr + 1]]), np.ascontiguousarray(R[ib[gc]:ib[gc + 1]]), gc == 0, gr == 0)
        Ln, Rn = np.empty_like(L), np.empty_like(R)
        for gr in range(rows):
            Ln[ub[gr]:ub[gr + 1]] = left_to_right([aux[gr, gc][0] for gc in range(cols)], reverse)
        for gc in range(cols):
            Rn[ib[gc]:ib[gc + 1]] = left_to_right([aux[gr, gc][1] for gr in range(rows)], reverse)
        L, R = Ln, Rn
        gens.append((L, R))
    return gens


def model_composed_loop(d, cut, L0, R0, iters):
    """the sharded flow of include/matfact_hip.h on two user shards: lambda on both sides, the users bounded in their sweep,
    the items unbounded in theirs, summed in shard order and projected after the sum (tests/test_bounded.py's model)"""
    gens, L, R = [(L0, R0)], L0, R0
    blocks = [(0, cut), (cut, d["users"])]
    models = []
    for b0, b1 in blocks:
        row, col, val = shard_entries(d, b0, b1)
        models.append(MModel(b1 - b0, d["items"], row - b0, col, val, d["alpha"]))
    for _ in range(iters):
        Ln, parts = np.empty_like(L), []
        for g, ((b0, b1), m) in enumerate(zip(blocks, models)):
            blk, P = bstep(m, np.ascontiguousarray(L[b0:b1]), R, (BOX, NO_BOX), lam=LAM, seed_i=g == 0, dot=fast_dot)
            Ln[b0:b1] = blk
            parts.append(P)
        L, R = Ln, clip(left_to_right(parts), *BOX, -1, True)
        gens.append((L, R))
    return gens


def differs(a, b):
    return float((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).mean())


def test_torch_add_on_the_cpu_gives_numpys_bits():
    """the stand-in for the all-reduce is torch.add: IEEE addition, element by element, as numpy's a + b"""
    rng = np.random.default_rng(12)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1030, -2.0 ** -1030, 2.0 ** -1022, np.inf, -np.inf, NAN, 1.0, -1.0, 1e308, -1e308,
                        2.0 ** 53, 1.0 + 2.0 ** -52])
    a = np.concatenate([np.repeat(special, len(special)), rng.standard_normal(4096) * 10.0 ** rng.integers(-300, 300, 4096)])
    b = np.concatenate([np.tile(special, len(special)), rng.standard_normal(4096) * 10.0 ** rng.integers(-300, 300, 4096)])
    with np.errstate(all="ignore"):
        want = a + b
    got = torch.add(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() >= 2 * len(special)      # NaN by position
    keep = ~np.isnan(want)
    assert np.array_equal(got[keep].view(np.uint64), want[keep].view(np.uint64))
    assert (want.view(np.uint64) == np.uint64(0x8000000000000000)).any() and np.isinf(want).any()
    assert ((np.abs(want) > 0) & (np.abs(want) < 2.0 ** -1022)).any()


def test_loop_models_with_one_shard_are_the_serial_oracle(orc):
    for (d, L0, R0), run in ((row_fixture(), lambda d, L0, R0: model_row_loop(d, [0, d["users"]], L0, R0, T_LOOP)),
                             (grid_fixture(), lambda d, L0, R0: model_grid_loop(d, [0, d["users"]], [0, d["items"]], L0, R0, T_LOOP)),
                             (pair_fixture(), lambda d, L0, R0: model_row_loop(d, [0, d["users"]], L0, R0, T_LOOP))):
        L, R = L0.copy(), R0.copy()
        with np.errstate(all="ignore"):
            orc.factorize(orc.Instance(**d), L, R, iters=T_LOOP)
        gens = run(d, L0, R0)
        assert len(gens) == T_LOOP + 1
        assert_same_bits(gens[-1][0], L, "one shard: L")
        assert_same_bits(gens[-1][1], R, "one shard: R")


def test_row_loop_model_is_the_multi_shard_model_and_its_sum_order_shows():
    d, L0, R0 = row_fixture()
    gens = model_row_loop(d, ROW_CUTS, L0, R0, T_LOOP)
    L, R, begin = model_run_multi(d, 3, L0, R0, cut=ROW_CUTS)
    assert begin == ROW_CUTS
    assert_same_bits(gens[-1][0], L, "three shards: L")
    assert_same_bits(gens[-1][1], R, "three shards: R")
    rev = model_row_loop(d, ROW_CUTS, L0, R0, T_LOOP, reverse=True)
    assert differs(rev[-1][1], R) > 0.1 and differs(rev[-1][0], L) > 0.1        # the comparison can tell the order of the sum
    assert differs(gens[-1][1], model_row_loop(d, [0, 90], L0, R0, T_LOOP)[-1][1]) > 0.1
    d, L0, R0 = pair_fixture()
    gens = model_row_loop(d, [0, PAIR_CUT, d["users"]], L0, R0, T_LOOP)
    L, R, _ = model_run_multi(d, 2, L0, R0, cut=[0, PAIR_CUT, d["users"]])
    assert_same_bits(gens[-1][0], L, "pair, two shards: L")
    assert_same_bits(gens[-1][1], R, "pair, two shards: R")
    # a sum of two is commutative: what shows on two shards is the cut, against the serial run
    assert differs(gens[-1][1], model_row_loop(d, [0, d["users"]], L0, R0, T_LOOP)[-1][1]) > 0.1
    comp = model_composed_loop(d, PAIR_CUT, L0, R0, T_LOOP)
    assert differs(comp[-1][1], gens[-1][1]) > 0.5 and ((comp[-1][1] == 0.0) | (comp[-1][1] == 0.5)).mean() > 0.1


def test_grid_loop_model_sum_order_shows():
    d, L0, R0 = grid_fixture()
    gens = model_grid_loop(d, GRID_UB, GRID_IB, L0, R0, T_LOOP)
    rev = model_grid_loop(d, GRID_UB, GRID_IB, L0, R0, T_LOOP, reverse=True)
    assert differs(rev[-1][1], gens[-1][1]) > 0.1 and differs(rev[-1][0], gens[-1][0]) > 0.1
    one = model_grid_loop(d, [0, 90], [0, 70], L0, R0, T_LOOP)
    assert differs(one[-1][0], gens[-1][0]) > 0.1


class Part:
    """one plan of a sharded or grid run: its buffers, its stream, its block of the inputs and whether its sweeps are seeded"""

    def __init__(self, plan, bufs, rows, cols, seed_items, seed_users):
        self.plan, self.bufs, self.rows, self.cols = plan, bufs, rows, cols
        self.seed_items, self.seed_users = seed_items, seed_users
        self.stream = None

    def next_tensor(self, side):
        nl, nr = self.bufs.nxt(self.plan)
        return nr if side == "items" else nl


def run_loop(gate, parts, groups, layout, composed=False):
    """T_LOOP iterations of the loop of sharded.py with the collectives replaced by torch.add in a fixed order, no host
    synchronisation inside, a closed gate in front.  groups: {"items": lists of part indices whose items_next are summed in
    that order, "users": the same for users_next}.  layout "one": every plan and the sums on one stream; "own": a stream per
    plan and one for the sums, torch events carrying the dependencies.  Returns the clones per part."""
    own = layout == "own"
    for n, p in enumerate(parts):
        p.stream = gate.pool[n] if own else gate.s
        p.plan.set_stream(p.stream.cuda_stream)
    sums = gate.pool[len(parts)] if own else gate.s
    streams = list({id(p.stream): p.stream for p in parts}.values())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    shut = [gate.close(st) for st in streams]
    for p in parts:
        with torch.cuda.stream(p.stream):
            p.bufs.write(p.plan, p.dL, p.dR)
    keep = []                                    # the sums stay alive until the streams that read them are done

    def summed(side, swept):
        if not groups[side]:
            return
        if own:
            for e in swept:
                sums.wait_event(e)
        accs = []
        with torch.cuda.stream(sums):
            for grp in groups[side]:
                acc = parts[grp[0]].next_tensor(side)
                for i in grp[1:]:
                    acc = torch.add(acc, parts[i].next_tensor(side))
                accs.append(acc)
            done = torch.cuda.Event()
            done.record(sums)
        keep.extend(accs)
        for grp, acc in zip(groups[side], accs):
            for i in grp:
                p = parts[i]
                with torch.cuda.stream(p.stream):
                    if own:
                        p.stream.wait_event(done)
                    if len(grp) > 1:
                        p.next_tensor(side).copy_(acc)
                if composed and side == "items":
                    p.plan.set_bounds("items", *BOX)
                    p.plan.project("items", "next")

    def swept(p):
        if not own:
            return None
        e = torch.cuda.Event()
        e.record(p.stream)
        return e
    for _ in range(T_LOOP):
        ev = []
        for p in parts:
            if composed:
                p.plan.set_bounds("items", *NO_BOX)           # the item sweep does not project: its result is a partial sum
            p.plan.sweep_items(p.seed_items)
            ev.append(swept(p))
        summed("items", ev)
        ev = []
        for p in parts:
            p.plan.sweep_users(p.seed_users)
            ev.append(swept(p))
        summed("users", ev)
        for p in parts:
            p.plan.flip()
    busy = all(not st.query() for st in streams)
    got = []
    for p in parts:
        with torch.cuda.stream(p.stream):
            got.append(p.bufs.clones(p.plan))
    closed = all(not e.query() for e in shut)
    gate.last_enqueue_ms = (time.perf_counter() - t0) * 1e3
    for p in parts:
        with torch.cuda.stream(p.stream):
            p.bufs.poison()
    for st in streams + [sums]:
        st.synchronize()
    if not (busy and closed):
        gate.inconclusive("%d plans, layout %s" % (len(parts), layout))
    return [[t.cpu().numpy() for t in g] for g in got]


def same_parts(got, parts, gens, where):
    (Ln, Rn), (Lb, Rb) = gens[-1], gens[-2]
    assert np.isfinite(Ln).all() and np.isfinite(Rn).all()
    for n, (g, p) in enumerate(zip(got, parts)):
        ld, (u0, u1), (j0, j1) = p.bufs.ld, p.rows, p.cols
        assert_same_bits(g[1], padded(Rn[j0:j1], ld), "%s, plan %d: current R" % (where, n))
        assert_same_bits(g[0], padded(Ln[u0:u1], ld), "%s, plan %d: current L" % (where, n))
        assert_same_bits(g[3], padded(Rb[j0:j1], ld), "%s, plan %d: R of the generation before" % (where, n))
        assert_same_bits(g[2], padded(Lb[u0:u1], ld), "%s, plan %d: L of the generation before" % (where, n))


def row_parts(capi, d, cuts, L0, R0):
    parts = []
    try:
        for g in range(len(cuts) - 1):
            b0, b1 = cuts[g], cuts[g + 1]
            row, col, val = shard_entries(d, b0, b1)
            plan, bufs = poisoned_plan(capi, d["users"], d["items"], d["feats"], d["alpha"], row, col, val, user_begin=b0, user_count=b1 - b0)
            p = Part(plan, bufs, (b0, b1), (0, d["items"]), g == 0, True)
            p.dL, p.dR = to_dev(L0[b0:b1]), to_dev(R0)
            parts.append(p)
    except BaseException:
        close_parts(parts)
        raise
    return parts


def grid_parts(capi, d, ub, ib, L0, R0):
    parts = []
    try:
        for gr in range(len(ub) - 1):
            for gc in range(len(ib) - 1):
                row, col, val = shard_entries(d, ub[gr], ub[gr + 1], ib[gc], ib[gc + 1])
                plan, bufs = poisoned_plan(capi, d["users"], ib[gc + 1] - ib[gc], d["feats"], d["alpha"], row, col - np.int32(ib[gc]), val,
                                           user_begin=ub[gr], user_count=ub[gr + 1] - ub[gr])
                p = Part(plan, bufs, (ub[gr], ub[gr + 1]), (ib[gc], ib[gc + 1]), gr == 0, gc == 0)
                p.dL, p.dR = to_dev(L0[ub[gr]:ub[gr + 1]]), to_dev(R0[ib[gc]:ib[gc + 1]])
                parts.append(p)
    except BaseException:
        close_parts(parts)
        raise
    return parts


def close_parts(parts):
    for p in parts:
        p.plan.close()


@gpu
@pytest.mark.parametrize("layout", ["one", "own"])
@pytest.mark.parametrize("name", ["90x60-K20-three-shards", "pair-K30-two-shards"])
def test_row_sharded_loop_in_one_process(device, switches, gate, name, layout):
    """ShardedFactorization._step across G plans of one process: item sweeps (shard 0 seeded), the sum of every items_next in
    shard order written back to every shard, user sweeps, flips -- six iterations without a host synchronisation."""
    capi = device
    switches(SWEEPS)
    (d, L0, R0), cuts = (row_fixture(), ROW_CUTS) if name.startswith("90x60") else (pair_fixture(), [0, PAIR_CUT, pattern("pair").users])
    gens = model_row_loop(d, cuts, L0, R0, T_LOOP)
    parts = row_parts(capi, d, cuts, L0, R0)
    try:
        got = run_loop(gate, parts, {"items": [list(range(len(parts)))], "users": []}, layout)
        same_parts(got, parts, gens, "%s, layout %s" % (name, layout))
    finally:
        close_parts(parts)


@gpu
@pytest.mark.parametrize("layout", ["one", "own"])
def test_grid_loop_in_one_process(device, switches, gate, layout):
    """GridFactorization._step across the six tiles of a 3 x 2 grid: item sweeps seeded on grid row 0 and summed over the
    grid column, user sweeps seeded on grid column 0 and summed over the grid row."""
    capi = device
    switches(SWEEPS)
    d, L0, R0 = grid_fixture()
    gens = model_grid_loop(d, GRID_UB, GRID_IB, L0, R0, T_LOOP)
    parts = grid_parts(capi, d, GRID_UB, GRID_IB, L0, R0)
    rows, cols = len(GRID_UB) - 1, len(GRID_IB) - 1
    groups = {"items": [[gr * cols + gc for gr in range(rows)] for gc in range(cols)],
              "users": [[gr * cols + gc for gc in range(cols)] for gr in range(rows)]}
    try:
        got = run_loop(gate, parts, groups, layout)
        same_parts(got, parts, gens, "3 x 2 grid, layout %s" % layout)
    finally:
        close_parts(parts)


@gpu
def test_composed_sharded_flow_in_one_process(device, switches, gate):
    """The sharded flow the header documents, on the two `pair` shards: lambda 0.05 / 0.3, the users bounded to [0, 0.5] in
    their sweep, the items left unbounded in theirs, summed, then mf_plan_project(items, next) on every shard."""
    capi = device
    switches(SWEEPS)
    d, L0, R0 = pair_fixture()
    cuts = [0, PAIR_CUT, d["users"]]
    gens = model_composed_loop(d, PAIR_CUT, L0, R0, T_LOOP)
    parts = row_parts(capi, d, cuts, L0, R0)
    try:
        for p in parts:
            p.plan.set_regularization(*LAM)
            p.plan.set_bounds("users", *BOX)
        got = run_loop(gate, parts, {"items": [[0, 1]], "users": []}, "one", composed=True)
        same_parts(got, parts, gens, "composed flow")
    finally:
        close_parts(parts)


# ------------------------------------------------------------------------------------------------ D: set_stream, synchronize, destroy
def _pair_plan(capi, K=30):
    x = expected("pair", "signed", K)
    plan, bufs = poisoned_plan(capi, x.pat.users, x.pat.items, K, x.alpha, x.pat.row, x.pat.col, x.val)
    return x, plan, bufs


@gpu
def test_set_stream_synchronises_the_stream_it_leaves(device, switches, gate):
    """A gate and an item sweep pending on s1: set_stream(s2) returns only when s1 is idle, and the sweep's result is in the
    buffer then."""
    capi = device
    switches(SWEEPS)
    x, plan, bufs = _pair_plan(capi)
    s1, s2 = gate.s, gate.independent()
    try:
        plan.set_stream(s1.cuda_stream)
        dL, dR = to_dev(x.L0), to_dev(x.R0)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            gate.close(s1)
            bufs.write(plan, dL, dR)
        plan.sweep_items(True)
        busy = not s1.query()
        t0 = time.perf_counter()
        plan.set_stream(s2.cuda_stream)
        took_ms = (time.perf_counter() - t0) * 1e3
        idle = s1.query()
        R = bufs.nxt(plan)[1].cpu().numpy()
        if not busy or took_ms < gate.ms / 2:
            gate.inconclusive("set_stream returned after %.2f ms" % took_ms)
        assert idle, "mf_plan_set_stream returned while the stream it left had work pending"
        assert_same_bits(R, padded(x.seeded[1], bufs.ld), "items_next when set_stream returned")
    finally:
        plan.close()


@gpu
def test_a_plan_moved_between_streams_gives_the_serial_bits(device, switches, gate):
    """s1 -> s2 -> 0 (the plan's own stream) between iterations.  After the move to s2 a gate on s1 does not delay the plan:
    the iteration completes, read back through download(), while s1 is still busy."""
    capi = device
    switches(SWEEPS)
    x, plan, bufs = _pair_plan(capi)
    gens = plain_generations("pair", 30, 3)
    s1, s2 = gate.s, gate.independent()
    try:
        plan.set_stream(s1.cuda_stream)
        got = behind_gate(gate, plan, bufs, x.L0, x.R0, _iterate(1), "first iteration on s1")
        same_generations(got, gens[:2], bufs.ld, "on s1")
        dL, dR = to_dev(gens[1][0]), to_dev(gens[1][1])
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            bufs.write(plan, dL, dR)
        plan.set_stream(s2.cuda_stream)
        shut = gate.close(s1)
        plan.iterate(1)
        L, R = plan.download()
        if s1.query() or shut.query():
            gate.inconclusive("the gate on the stream the plan left opened before download() returned")
        assert_same_bits(L, gens[2][0], "on s2: L")
        assert_same_bits(R, gens[2][1], "on s2: R")
        plan.set_stream(None)
        plan.iterate(1)
        L, R = plan.download()
        assert_same_bits(L, gens[3][0], "on the plan's own stream: L")
        assert_same_bits(R, gens[3][1], "on the plan's own stream: R")
        s1.synchronize()
    finally:
        plan.close()


@gpu
def test_synchronize_behind_a_closed_gate(device, switches, gate):
    capi = device
    switches(SWEEPS)
    x, plan, bufs = _pair_plan(capi)
    s = gate.s
    try:
        plan.set_stream(s.cuda_stream)
        dL, dR = to_dev(x.L0), to_dev(x.R0)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            gate.close(s)
            bufs.write(plan, dL, dR)
        plan.iterate(1)
        busy = not s.query()
        t0 = time.perf_counter()
        plan.synchronize()
        took_ms = (time.perf_counter() - t0) * 1e3
        idle = s.query()
        if not busy or took_ms < gate.ms / 2:
            gate.inconclusive("synchronize returned after %.2f ms" % took_ms)
        assert idle
        gens = plain_generations("pair", 30, 1)
        same_generations([t.cpu().numpy() for t in bufs.cur(plan) + bufs.nxt(plan)], gens, bufs.ld, "after synchronize")
    finally:
        plan.close()


@gpu
def test_close_with_an_iteration_pending_on_the_callers_stream(device, switches, gate):
    """mf_plan_destroy behind a closed gate: when it returns, with no synchronisation by the caller, the caller's buffers
    hold the model's bits."""
    capi = device
    switches(SWEEPS)
    x, plan, bufs = _pair_plan(capi)
    s = gate.s
    try:
        plan.set_stream(s.cuda_stream)
        dL, dR = to_dev(x.L0), to_dev(x.R0)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            gate.close(s)
            bufs.write(plan, dL, dR)
        plan.iterate(2)
        tensors = bufs.cur(plan) + bufs.nxt(plan)
        busy = not s.query()
        t0 = time.perf_counter()
        plan.close()
        took_ms = (time.perf_counter() - t0) * 1e3
        got = [t.cpu().numpy() for t in tensors]
        if not busy or took_ms < gate.ms / 2:
            gate.inconclusive("close returned after %.2f ms" % took_ms)
        same_generations(got, plain_generations("pair", 30, 2), bufs.ld, "after close")
    finally:
        plan.close()
        s.synchronize()


class StandInPlan:
    """what the drivers of sharded.py touch of a plan when they are built"""

    def __init__(self):
        self.streams = []

    def set_stream(self, handle):
        self.streams.append(handle)


@pytest.mark.parametrize("driver", ["sharded", "grid"])
def test_the_drivers_refuse_the_default_stream_and_gpu_buffers_without_a_stream(driver):
    """Handle 0 is "the plan's own stream" to mf_plan_set_stream: the collective would not be ordered against the sweeps."""
    sh = importlib.import_module("recommender_system_amd.sharded")
    cpu = [torch.zeros((4, 3), dtype=torch.float64) for _ in range(2)]
    on_gpu = [types.SimpleNamespace(is_cuda=True, data_ptr=lambda n=n: 256 * (n + 1)) for n in range(2)]

    def build(plan, bufs, stream):
        if driver == "sharded":
            return sh.ShardedFactorization(plan, bufs, 0, 2, stream=stream)
        return sh.GridFactorization(plan, bufs, bufs, 0, (1, 1), stream=stream)
    plan = StandInPlan()
    with pytest.raises(ValueError, match="non-default CUDA stream"):
        build(plan, cpu, types.SimpleNamespace(cuda_stream=0))
    with pytest.raises(ValueError, match="explicit stream"):
        build(plan, on_gpu, None)
    assert plan.streams == []
    build(plan, cpu, None)                                    # the CPU stand-in of the gloo tests
    build(plan, on_gpu, types.SimpleNamespace(cuda_stream=0x7f00))
    assert plan.streams == [0x7f00]
