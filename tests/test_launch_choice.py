"""The launch-time choice of a sweep's main launch (csrc/mf_schedule.h: single_wave_pipelined, launch_form, launch_flavour,
launch_geometry) against its truth table, written out here and independent of the header.

CPU test in the manner of test_schedule.py: tests/launch_choice_main.cpp includes only mf_schedule.h, enumerates every
combination of {coop_all, use_db, use_pair, the variant has a pipelined instance, K = 128 / 256, n_short and nrows at and one
past 262144, decay, momentum, weighted, few_rows} -- 2048 cases -- and prints the chosen (form, flavour, geometry source) of
each.  The results are the values of the enums, so the order of the enums -- the two indices of the kernel grid
SweepVariant::fn[form][flavour] of mf_plan.hip.h -- is pinned with them.

GPU test: each (form, flavour) pair runs its own instance, bit for bit -- one seeded iteration of each flavour in a fresh
plan, in the pipelined, the double-buffered and the wave-pair form at K = 128 and in the pipelined and the double-buffered
form at K = 256, against the models of the feature tests.  The launches are of fewer than 2048 rows, so the single-wave forms
take the large chunk; the LDS request of each case is read back from the plan's description and, the double-buffered form at
K = 128 apart, must exceed 64 KiB, the default limit of a kernel's dynamic LDS that raise_form_limits lifts.
What the test cannot see (profiles/launch_grid/README.md): on the HIP runtime it was written on, a library built never to
raise a limit passed every case -- that runtime launches a request of up to 80 KiB without the attribute -- so a forgotten
limit shows here only on a runtime that enforces it."""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_bounded import NO_BETA, NO_BOX, bstep
from test_momentum import BETA, MModel, random_prev
from test_regularised import LAM_I, LAM_U
from test_sweep_edges import SWITCHES, Pattern, assert_same_bits, cls_signed
from test_weighted import WModel, plain_weights

gpu = pytest.mark.gpu

FORMS = ("plain", "pipelined", "pair", "db", "coop")
FLAVOURS = ("accumulate", "decay", "momentum", "decay_w", "momentum_w")
GEOMETRIES = ("single", "few", "pair", "db", "coop", "coop_single_nch")
PF_ROWS = 262144   # up to this many rows a launch of one-pass rows (K <= 128) takes the pipelined form
INPUTS = ("coop_all", "use_db", "use_pair", "has_pf", "K", "n_short", "nrows", "decay", "momentum", "weighted", "few_rows")


def expected(c):
    """The truth table: (form, flavour, geometry source) of one case."""
    if c["coop_all"]:
        form = "coop"
    elif c["use_db"]:
        form = "db"
    elif c["use_pair"]:
        form = "pair"
    elif c["has_pf"] and (c["K"] > 128 or (c["n_short"] <= PF_ROWS and c["nrows"] <= PF_ROWS)):
        form = "pipelined"
    else:
        form = "plain"
    if c["weighted"]:
        flavour = "momentum_w" if c["momentum"] else "decay_w"
    elif c["momentum"]:
        flavour = "momentum"
    else:
        flavour = "decay" if c["decay"] else "accumulate"
    if form == "coop":   # its own LDS request; the single-wave chunk size when the launch is not one of few rows
        geometry = "coop" if c["few_rows"] else "coop_single_nch"
    elif form in ("db", "pair"):
        geometry = form
    else:
        geometry = "few" if c["few_rows"] else "single"
    return form, flavour, geometry


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """[(inputs, (form, flavour, geometry))] as the program prints them."""
    exe = str(tmp_path_factory.mktemp("launch_choice") / "launch_choice_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "launch_choice_main.cpp")])
    out = []
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        left, right = line.split(":")
        form, flavour, geometry = map(int, right.split())
        out.append((dict(zip(INPUTS, map(int, left.split()))), (FORMS[form], FLAVOURS[flavour], GEOMETRIES[geometry])))
    return out


def test_every_combination_is_enumerated_once(cases):
    rows = (PF_ROWS, PF_ROWS + 1)
    want = set(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (128, 256), rows, rows, (0, 1), (0, 1), (0, 1), (0, 1)))
    got = [tuple(c[k] for k in INPUTS) for c, _ in cases]
    assert len(got) == len(want) == 2048 and set(got) == want


def test_the_choice_is_the_truth_table(cases):
    for c, got in cases:
        assert got == expected(c), (c, got, expected(c))


def test_outcomes_no_launch_may_have(cases):
    """A weighted plan has no accumulate instance; momentum without weights never runs a decay instance (the momentum
    instances carry the decay); K = 256 has no plain instance but the accumulate one, so where the variant has a pipelined
    instance -- every K = 256 variant with an LDS-DMA form does -- the single-wave launch is never the plain form, at any
    row count."""
    seen = set()
    for c, (form, flavour, geometry) in cases:
        seen.add((form, flavour, geometry))
        if c["weighted"]:
            assert flavour in ("decay_w", "momentum_w"), c
        if c["momentum"] and not c["weighted"]:
            assert flavour == "momentum", c
        if c["K"] == 256 and c["has_pf"]:
            assert form != "plain", c
        if c["K"] == 128 and c["has_pf"] and not (c["coop_all"] or c["use_db"] or c["use_pair"]):   # the bound, at and one past
            assert (form == "pipelined") == (c["n_short"] == PF_ROWS and c["nrows"] == PF_ROWS), c
    # ... and every form meets every flavour, every geometry source is taken
    assert {(f, fl) for f, fl, _ in seen} == set(itertools.product(FORMS, FLAVOURS))
    assert {g for _, _, g in seen} == set(GEOMETRIES)


# ------------------------------------------------------------------------------------------------ GPU: the LDS limits
LAM = (LAM_U, LAM_I)
NO_LAM = (0.0, 0.0)
# flavour -> (weighted, lambda, beta): what makes launch_sweep pick that column of the grid
FLAVOUR_RULES = {"accumulate": (False, NO_LAM, NO_BETA), "decay": (False, LAM, NO_BETA), "momentum": (False, LAM, BETA),
                 "decay_w": (True, LAM, NO_BETA), "momentum_w": (True, LAM, BETA)}
FORM_SWITCHES = {"pipelined": {}, "db": {"MF_SWEEP_DB": "1"}, "pair": {"MF_SWEEP_PAIR": "1"}}
LDS_DEFAULT = 64 * 1024


def lds_request(desc, form):
    """the LDS request of a main launch of few rows in `form`, from the figures mf_plan_describe prints: the tile row stride,
    the single-wave chunk and its request (which gives the bytes in front of the tile), the few-rows request that the row-sum
    launch of the loss shares with the sweeps (chunk_rule), and the chunk of the two-tile forms"""
    num = lambda pat: int(re.search(pat, desc).group(1))   # noqa: E731
    nch, row_bytes, lds = num(r" nch=(\d+) "), num(r" row_bytes=(\d+) "), num(r" row_bytes=\d+ lds=(\d+) ")
    head = lds - nch * row_bytes
    if form == "pipelined":
        return num(r" loss=\w+\(nch=\d+/\d+ lds=\d+/(\d+)\)")
    return head + 2 * num(r" double_buffered=\d/\d\(nch=(\d+)\)" if form == "db" else r" wave_pair=\d/\d\(nch=(\d+)\)") * row_bytes


@functools.lru_cache(maxsize=None)
def few_rows_pattern():
    """80 x 70, every user 4..19 entries but five of 65..70, and three items rated by 70 users or more: rows of more than one
    large chunk on both sides, under 4096 entries (the iteration stays the two sweeps)."""
    U, I = 80, 70
    rng = np.random.default_rng(4300)
    mask = np.zeros((U, I), bool)
    for u in range(U):
        n = (65, 66, 68, 69, 70)[u // 16] if u % 16 == 3 else int(rng.integers(4, 20))
        mask[u, rng.choice(I, n, replace=False)] = True
    mask[rng.choice(U, 72, replace=False), 0] = True
    mask[rng.choice(U, 75, replace=False), 33] = True
    mask[:, 69] = True
    row, col = np.nonzero(mask)
    return Pattern("few-rows", U, I, row, col)


def test_the_few_rows_pattern_is_what_the_limits_need():
    pat = few_rows_pattern()
    assert (pat.users, pat.items) == (80, 70) and max(pat.users, pat.items) < 2048 and pat.nnz < 4096
    assert (pat.ulen > 64).sum() == 5 and (pat.ilen > 64).sum() == 3


@functools.lru_cache(maxsize=None)
def limits_expected(K):
    """inputs at one K and, per flavour, the model's (L, R) after one seeded iteration; computed once, shared by the forms"""
    pat = few_rows_pattern()
    x = type("LimitsExpected", (), {})()
    x.pat, x.K = pat, K
    x.L0, x.R0, x.val, x.alpha = cls_signed(4300 + K, pat, K)
    x.prev = (random_prev(4301 + K, x.L0), random_prev(4302 + K, x.R0))
    x.w = plain_weights(4303 + K, pat.nnz)
    x.want = {}
    for flavour, (weighted, lam, beta) in FLAVOUR_RULES.items():
        m = WModel(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha, x.w) if weighted else \
            MModel(pat.users, pat.items, pat.row, pat.col, x.val, x.alpha)
        x.want[flavour] = bstep(m, x.L0, x.R0, (NO_BOX, NO_BOX), *x.prev, lam=lam, beta=beta)
    return x


@gpu
@pytest.mark.parametrize("form,K", [("pipelined", 128), ("db", 128), ("pair", 128), ("pipelined", 256), ("db", 256)])
def test_every_flavour_of_a_form_runs_its_own_instance(capi, monkeypatch, form, K):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORM_SWITCHES[form].items():
        monkeypatch.setenv(k, v)
    x = limits_expected(K)
    pat = x.pat
    seen = set()
    for flavour, (weighted, lam, beta) in FLAVOUR_RULES.items():
        plan = capi.Plan(pat.users, pat.items, K, x.alpha, pat.row, pat.col, x.val, weight=x.w if weighted else None)
        try:
            desc = plan.describe()
            assert desc.startswith("sweep_dma_kernel<KT=%d," % K) and "long_rows=0/0 coop_nch=0 " in desc, desc
            assert ("double_buffered=1/1(" in desc) == (form == "db") and ("wave_pair=1/1(nch=32)" in desc) == (form == "pair"), desc
            assert "accumulate=pf/pf iterate=sweeps" in desc and (" weighted=1" in desc) == weighted, desc
            assert (lds_request(desc, form) > LDS_DEFAULT) == ((form, K) != ("db", 128)), (lds_request(desc, form), desc)
            plan.set_regularization(*lam)
            plan.set_momentum(*beta)
            plan.upload(x.L0, x.R0)
            plan.upload_previous(*x.prev)
            plan.iterate(1)
            L, R = plan.download()
        finally:
            plan.close()
        where = "%s K=%d %s" % (form, K, flavour)
        assert_same_bits(L, x.want[flavour][0], where + ": L")
        assert_same_bits(R, x.want[flavour][1], where + ": R")
        seen.add(np.ascontiguousarray(L).tobytes())
    assert len(seen) == len(FLAVOUR_RULES)   # the five rules are five different results: no flavour ran as another
