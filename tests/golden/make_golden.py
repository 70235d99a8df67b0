#!/usr/bin/env python3
"""Generates the committed golden fixtures from the REAL reference (oracle/_ref, built from /root/reference
by oracle/Makefile).  Run in the build container only -- the reference does not exist on the GPU box.

  <name>.in[.gz]     copy of the reference's own sample input  (data file of the reference's test set)
  <name>.out         copy of the reference's own golden output (samples/<name>.out)
  <name>.factors.npz L and R after {1, 2, 10, iters} iterations, produced by calling the reference's
                     compiled matrix_factorization() (matFact.c:29) through oracle/_ref/libmatfact_ref.so,
                     plus the reference binary's stdout for cross-checking the .out copy.
  <name>.in.gz       (LARGE_INPUTS) the reference's larger sample inputs, gzipped, no factors
  reference_random.npz  seeded random instances and the reference's L, R, B on them (RANDOM_CASES)
  reference_special.npz signed ratings, three diverging step sizes and one that converges: the reference's L, R, B
                        after 1, 2, 3, 5, 6, 7 and 8 iterations (inf and NaN included)
  instDiverge.in/.out   one of the diverging instances as an input file, and the reference binary's stdout on it
  cli_matrix.json       what this project's own command line answers to every combination of its MATFACT_* rule variables
                        (`make_golden.py cli_matrix <matFact>`; needs no reference)

Fixtures are data only (inputs and expected outputs); no reference source text is stored.
"""
import gzip
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

SAMPLES = "/root/reference/samples"
HERE = os.path.dirname(os.path.abspath(__file__))

# name -> iteration counts to snapshot ("full" = the header's iteration count)
CASES = {
    "inst0": [1, 2, 10, "full"],
    "inst1": [1, 2, 10, "full"],
    "inst2": [1, 2, 10, "full"],
    "inst30-40-10-2-10": [1, 2, 10, "full"],
    "inst1000-1000-100-2-30": [1, "full"],
    "instML100k": [1, "full"],
}
GZIP = {"instML100k", "inst1000-1000-100-2-30"}


def main():
    O.build(ref=True)
    assert O.ref_available(), "oracle/_ref is missing"
    for name, snaps in CASES.items():
        src = os.path.join(SAMPLES, name + ".in")
        inst = O.parse_in(src)
        if name in GZIP:
            with open(src, "rb") as f, gzip.GzipFile(os.path.join(HERE, name + ".in.gz"), "wb", mtime=0) as g:
                shutil.copyfileobj(f, g)
        else:
            shutil.copyfile(src, os.path.join(HERE, name + ".in"))
        shutil.copyfile(os.path.join(SAMPLES, name + ".out"), os.path.join(HERE, name + ".out"))
        stdout = O.ref_cli(src, "serial")
        assert stdout == open(os.path.join(SAMPLES, name + ".out")).read(), name
        arrays = {}
        for s in snaps:
            it = inst.iters if s == "full" else s
            L, R, _B = O.ref_run(inst, iters=it)
            arrays["L_%s" % s] = L
            arrays["R_%s" % s] = R
            print(name, "iters", it, "done", flush=True)
        np.savez_compressed(os.path.join(HERE, name + ".factors.npz"), **arrays)
    # the .mats dumps of the three tiny instances (6-decimal prints of L, R, B per iteration)
    for name in ("inst0", "inst1", "inst2"):
        shutil.copyfile(os.path.join(SAMPLES, name + ".mats"), os.path.join(HERE, name + ".mats"))
    large_inputs()
    reference_random()
    reference_special()


# the reference's larger samples, inputs only (the GPU tests compare the backend with the oracle on them); gzip keeps
# every one under 1 MiB
LARGE_INPUTS = ["inst50000-5000-100-2-5", "inst400-50000-30-200-500", "inst600-10000-10-40-400"]

# random instances through the reference's own compiled functions (test_oracle_pinned.py: users, items, K per case)
RANDOM_CASES = [(7, 9, 3), (20, 15, 8), (33, 50, 13), (64, 70, 32)]


def large_inputs():
    for name in LARGE_INPUTS:
        with open(os.path.join(SAMPLES, name + ".in"), "rb") as f, \
                gzip.GzipFile(os.path.join(HERE, name + ".in.gz"), "wb", mtime=0) as g:
            shutil.copyfileobj(f, g)


def reference_random():
    """reference_random.npz: per case the instance (row, col, val) and the reference's L, R and B after its 7
    iterations (alpha 0.004, user 1 without ratings, user 2 rating every item)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from conftest import random_instance  # noqa: E402
    O.build(ref=True)
    assert O.ref_available(), "oracle/_ref is missing"
    arrays = {}
    for seed, (u, i, k) in enumerate(RANDOM_CASES):
        d = random_instance(100 + seed, u, i, k, density=0.3, iters=7, alpha=0.004, empty_rows=(1,), full_rows=(2,))
        L, R, B = O.ref_run(O.Instance(**d))
        arrays.update({"row_%d" % seed: d["row"], "col_%d" % seed: d["col"], "val_%d" % seed: d["val"],
                       "L_%d" % seed: L, "R_%d" % seed: R, "B_%d" % seed: B})
    np.savez_compressed(os.path.join(HERE, "reference_random.npz"), **arrays)


# instances with ratings in [-5, 5] (multiples of 0.5): three step sizes at which the run diverges to inf and then NaN
# within a few iterations, and one at which it does not (tests/test_sweep_edges.py)
SPECIAL_SHAPE = (40, 30, 6)
SPECIAL_ALPHAS = [0.5, 0.05, 3.0, 0.002]
SPECIAL_ITERS = [1, 2, 3, 5, 6, 7, 8]   # 6 and 7: where inf and NaN first appear at alpha 0.5 and 3.0
DIVERGE = 0   # the instance written out as instDiverge.in / .out (its header asks for SPECIAL_ITERS[-1] iterations)


def special_instance(n):
    """Instance n of reference_special.npz (shared with tests/test_sweep_edges.py, which rebuilds it from the seed)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from conftest import random_instance  # noqa: E402
    u, i, k = SPECIAL_SHAPE
    d = random_instance(700 + n, u, i, k, density=0.3, iters=SPECIAL_ITERS[-1], alpha=SPECIAL_ALPHAS[n], empty_rows=(1,),
                        full_rows=(2,))
    d["val"] = np.random.default_rng(800 + n).integers(-10, 11, len(d["row"])) / 2.0
    return d


def reference_special():
    """reference_special.npz: per instance (row, col, val) and the reference's own L, R, B after 1, 2, 3, 5, 6, 7 and 8
    iterations (NaN as the reference's machine wrote it); instDiverge.in / .out: one diverging instance as a file and the reference
    binary's stdout on it."""
    sys.path.insert(0, os.path.dirname(HERE))
    from conftest import to_text  # noqa: E402
    O.build(ref=True)
    assert O.ref_available(), "oracle/_ref is missing"
    arrays = {}
    with np.errstate(all="ignore"):
        for n in range(len(SPECIAL_ALPHAS)):
            d = special_instance(n)
            arrays.update({"row_%d" % n: d["row"], "col_%d" % n: d["col"], "val_%d" % n: d["val"]})
            for it in SPECIAL_ITERS:
                L, R, B = O.ref_run(O.Instance(**d), iters=it)
                arrays.update({"L_%d_%d" % (n, it): L, "R_%d_%d" % (n, it): R, "B_%d_%d" % (n, it): B})
            print("special", n, "alpha", d["alpha"], "NaN in L after", SPECIAL_ITERS[-1], "iterations:", int(np.isnan(L).sum()), flush=True)
    np.savez_compressed(os.path.join(HERE, "reference_special.npz"), **arrays)
    path = os.path.join(HERE, "instDiverge.in")
    with open(path, "w") as f:
        f.write(to_text(special_instance(DIVERGE)))
    with open(os.path.join(HERE, "instDiverge.out"), "w") as f:
        f.write(O.ref_cli(path, "serial"))


# the command line's option rules (tests/test_cli.py): every MATFACT_* variable that takes part in a rule, with a valid value
CLI_VALID = [("MATFACT_TOPN", "3"), ("MATFACT_LOSS", "5"), ("MATFACT_HELDOUT", "held.in"), ("MATFACT_RANK", "10"),
             ("MATFACT_SIMILAR", "3"), ("MATFACT_SIMILAR_OUT", "s.txt"), ("MATFACT_LAMBDA", "0.1"), ("MATFACT_BIAS", "1"),
             ("MATFACT_DEVICES", "0"), ("MATFACT_MATS", "/dev/null"), ("MATFACT_CHECKPOINT", "x.ck"), ("MATFACT_RESUME", "x.ck")]
# the malformed values of the per-feature refusal tests (test_topn, test_loss, test_rank, test_similar, BAD_LAMBDA of
# test_regularised, BAD_BIAS of test_frozen) as (variable, values, the companions those tests set next to it)
CLI_MALFORMED = [
    ("MATFACT_TOPN", ["0", "33", "ten", "3x", ""], {}),
    ("MATFACT_LOSS", ["0", "-3", "five", "", "5x", "5,", "5,abc"], {}),
    ("MATFACT_RANK", ["0", "-2", "ten", "3x", ""], {"MATFACT_LOSS": "5", "MATFACT_HELDOUT": "held.in"}),
    ("MATFACT_SIMILAR", ["0", "33", "ten", "3x", "", "3,", "3,euclid", "3,cosine,dot"], {}),
    ("MATFACT_SIMILAR", ["3,dot"], {"MATFACT_SIMILAR_OUT": ""}),
    ("MATFACT_SIMILAR", ["3"], {"MATFACT_SIMILAR_OUT": "s.txt", "MATFACT_LOSS": "1"}),
    ("MATFACT_LAMBDA", ["", "abc", "-1", "-0.5,0.1", "0.1,-2", "nan", "inf", "1e999", "0.1,", "0.1,x", "0.1x", "0.1,0.2,0.3",
                        ",0.1"], {}),
    ("MATFACT_BIAS", ["", "0", "2", "yes", "1 ", "11", "-1", "true"], {}),
]


def cli_matrix_envs():
    """The environments of cli_matrix.json: every subset of at most three of CLI_VALID (299), then CLI_MALFORMED."""
    import itertools
    envs = [dict(c) for k in range(4) for c in itertools.combinations(CLI_VALID, k)]
    return envs + [dict(companions, **{name: v}) for name, values, companions in CLI_MALFORMED for v in values]


def cli_run(cli, env, cwd):
    """(returncode, stdout, stderr) of `cli missing.in` in the directory `cwd` with exactly `env` of the MATFACT_* variables set:
    option and parse errors come before any GPU call, so the run ends the same way with or without a GPU"""
    import subprocess
    base = {k: v for k, v in os.environ.items() if not k.startswith("MATFACT_")}
    r = subprocess.run([cli, "missing.in"], capture_output=True, cwd=cwd, env=dict(base, **env))
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def cli_matrix(cli):
    """cli_matrix.json: what the command line at `cli` answers to every environment of cli_matrix_envs() -- the refusal's
    message, or the parser's on the missing input where the combination is accepted.  Each distinct stderr text is stored once."""
    import json
    import tempfile
    messages, runs = [], []
    with tempfile.TemporaryDirectory() as cwd:
        for env in cli_matrix_envs():
            code, out, err = cli_run(os.path.abspath(cli), env, cwd)
            if err not in messages:
                messages.append(err)
            runs.append({"env": env, "returncode": code, "stdout": out, "stderr": messages.index(err)})
        assert not os.listdir(cwd), os.listdir(cwd)
    with open(os.path.join(HERE, "cli_matrix.json"), "w") as f:
        f.write('{"stderr": %s,\n"runs": [\n%s\n]}\n' % (json.dumps(messages, indent=0),   # one run per line
                                                     ",\n".join(json.dumps(r, sort_keys=True) for r in runs)))
    print("cli_matrix.json: %d runs, %d distinct stderr texts" % (len(runs), len(messages)))


if __name__ == "__main__":
    # no argument: every fixture; otherwise only the parts named (main, large_inputs, reference_random, reference_special),
    # or `cli_matrix <path of the matFact to record from>`
    if sys.argv[1:2] == ["cli_matrix"]:
        cli_matrix(sys.argv[2])
        sys.exit(0)
    for part in sys.argv[1:] or ["main"]:
        {"main": main, "large_inputs": large_inputs, "reference_random": reference_random,
         "reference_special": reference_special}[part]()
