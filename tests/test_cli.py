"""The command line as a whole: its option rules (which MATFACT_* combinations it refuses, with which message, before it
opens anything) against the recorded matrix, and the order of its stages on the fullest combination it accepts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden_in

sys.path.insert(0, GOLDEN)
import make_golden  # noqa: E402


def test_cli_option_matrix_is_the_recorded_one(capi, tmp_path):
    """Every subset of at most three of the twelve rule variables and every malformed value of the per-feature tests, on an
    input that does not exist: return code, stdout and stderr equal the record (tests/golden/cli_matrix.json, written by
    make_golden.cli_matrix from the command line as it was before its options became a table)."""
    want = json.load(open(os.path.join(GOLDEN, "cli_matrix.json")))
    envs = make_golden.cli_matrix_envs()
    assert [r["env"] for r in want["runs"]] == envs and len(envs) == 299 + 48
    assert len(set(want["stderr"])) == len(want["stderr"])
    refused = 0
    for r in want["runs"]:
        got = make_golden.cli_run(capi.CLI_PATH, r["env"], str(tmp_path))
        assert got == (r["returncode"], r["stdout"], want["stderr"][r["stderr"]]), (r["env"], got)
        assert got[0] == 255 and got[1] == ""
        refused += "Unable to open input file." not in got[2]
    assert 0 < refused < len(envs)
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("GPU tests need an MI355X; mf_backend_device_count() = %d" % capi.device_count())
    return capi


def _number(text, expected, where):
    """a %.17g field parses back to exactly the float the plan gave (NaN for NaN)"""
    got = np.array([float(text)])
    assert np.array_equal(got.view(np.uint64), np.array([expected], np.float64).view(np.uint64)) or \
        (np.isnan(got[0]) and np.isnan(expected)), (where, text, repr(expected))


@pytest.mark.gpu
def test_cli_stage_order_on_the_fullest_combination(gpu, orc, tmp_path):
    """MATFACT_BIAS + MATFACT_LAMBDA + MATFACT_LOSS=7 + MATFACT_HELDOUT + MATFACT_RANK on inst30-40-10-2-10 with 60 iterations
    (8 * 7 + 4: the last monitored step is a short one): stdout is the .out of the packed plan's recommend(); stderr carries the
    points, then mu, then the penalty, then the ranks, every number the plan's own bits."""
    capi = gpu
    text = open(golden_in("inst30-40-10-2-10")).read().split("\n", 1)
    path = str(tmp_path / "inst60.in")
    with open(path, "w") as f:
        f.write("60\n" + text[1])
    inst = capi.parse_file(path)
    assert (inst.iters, inst.users, inst.items, inst.feats, inst.nnz) == (60, 30, 40, 10, 170)
    F, n = inst.feats, 150
    rng = np.random.default_rng(3)
    hrow = rng.integers(0, inst.users, n).astype(np.int32)
    hcol = rng.integers(0, inst.items, n).astype(np.int32)
    hval = (1 + (hrow + hcol) % 5).astype(np.float64)
    hpath = str(tmp_path / "held.in")
    with open(hpath, "w") as f:
        f.write("%d\n%r\n%d\n%d %d %d\n" % (inst.iters, float(inst.alpha), F, inst.users, inst.items, n))
        f.writelines("%d %d %d\n" % (r, c, v) for r, c, v in zip(hrow.tolist(), hcol.tolist(), hval.tolist()))
    lam_u, lam_i = 0.05, 0.3

    # the expected values: the unchanged library through the plan, on the packed K = F + 2 problem
    mu = capi.bias_mean(inst.val)
    L0, R0 = capi.init_factors(inst.users, inst.items, F)
    plan = capi.Plan(inst.users, inst.items, F + 2, inst.alpha, inst.row, inst.col, inst.val - mu)
    plan.upload(capi.bias_pack(L0, None, 1), capi.bias_pack(R0, None, 0))
    plan.set_heldout(hrow, hcol, hval - mu)
    plan.set_regularization(lam_u, lam_i)
    plan.set_frozen_columns(F + 1, F)
    done, trace = plan.iterate_monitored(60, 7)
    lsq, rsq = plan.penalty()
    fin = plan.loss("train")
    m = capi.rank_metrics(plan.rank_heldout(), hrow, 10)
    best = plan.recommend()
    plan.close()
    assert done == 60 and [p.iter for p in trace] == list(range(0, 57, 7)) + [60]

    clean = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([capi.CLI_PATH, path], capture_output=True,
                       env=dict(clean, MATFACT_BIAS="1", MATFACT_LAMBDA="0.05,0.3", MATFACT_LOSS="7", MATFACT_HELDOUT=hpath,
                                MATFACT_RANK="10"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == orc.format_out(best).encode()
    lines = [ln.split() for ln in r.stderr.decode().splitlines()]
    print("\n" + r.stderr.decode())
    assert [" ".join(w[:2]) for w in lines] == ["iter %d" % p.iter for p in trace] + ["bias mu", "penalty lambda", "heldout_rank cutoff"]
    for w, p in zip(lines, trace):
        assert w[2::2] == ["train_rmse", "heldout_rmse"] and len(w) == 6 and p.train.count == inst.nnz and p.heldout.count == n
        _number(w[3], p.train.rmse, "train_rmse at iteration %d" % p.iter)
        _number(w[5], p.heldout.rmse, "heldout_rmse at iteration %d" % p.iter)
    w = lines[len(trace)]
    assert len(w) == 3
    _number(w[2], mu, "mu")
    w = lines[len(trace) + 1]
    assert w[4::2] == ["users_sq", "items_sq", "objective"] and len(w) == 10
    for got, expected, where in zip([w[2], w[3]] + w[5::2], (lam_u, lam_i, lsq, rsq, (fin.sse + lam_u * lsq) + lam_i * rsq),
                                    ("lambda_users", "lambda_items", "users_sq", "items_sq", "objective")):
        _number(got, expected, where)
    w = lines[len(trace) + 2]
    assert w[1::2] == ["cutoff", "evaluated", "masked", "nan", "users", "hits", "hit_rate", "mrr", "ndcg"] and len(w) == 19
    assert [int(x) for x in w[2:13:2]] == [10, m.evaluated, m.masked, m.nan, m.users, m.hits]
    assert m.evaluated + m.masked + m.nan == n and m.evaluated > 0
    for got, expected, where in zip(w[14::2], (m.hit_rate, m.mrr, m.ndcg), ("hit_rate", "mrr", "ndcg")):
        _number(got, expected, where)
