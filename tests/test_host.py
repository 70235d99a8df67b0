"""Host-side C pieces and the C-ABI surface, CPU only: parser grammar and error strings (util.c:12-34),
glibc random() restatement, initial factors, partition arithmetic (mpiutil.h:8-13), synthetic generator,
that both libraries export every declared symbol, and the CLI's argument/error behaviour (matFact.c:63-76)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_in, random_instance, to_text


def test_libraries_export_every_declared_symbol(capi):
    hip, host = C.CDLL(capi.HIP_LIB_PATH), C.CDLL(capi.HOST_LIB_PATH)
    for s in capi.HIP_SYMBOLS:
        assert hasattr(hip, s), s
    for s in capi.HOST_SYMBOLS:
        assert hasattr(host, s), s
    # and the header declares exactly that list
    hdr = open(os.path.join(ROOT, "include", "matfact_hip.h")).read()
    declared = set(re.findall(r"\b(mf_(?:backend|plan)_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(capi.HIP_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "matfact_host.h")).read()
    declared = set(re.findall(r"\b(mf_host_[a-z0-9_]+)\s*\(", hdr)) - {
        "mf_host_block_low", "mf_host_block_high", "mf_host_block_size", "mf_host_block_owner"}
    assert declared == set(capi.HOST_SYMBOLS)
    assert capi.hip().mf_backend_abi_version() == 5


def test_no_gpu_means_loud_failure_not_fallback(capi):
    """Without a device every compute entry returns MF_ERR_NO_DEVICE; nothing computes on the CPU."""
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    inst = capi.parse_file(golden_in("inst0"))
    L, R = capi.init_factors(inst.users, inst.items, inst.feats)
    with pytest.raises(capi.HipBackendError) as e:
        capi.backend_run(inst, L, R)
    assert e.value.status == capi.MF_ERR_NO_DEVICE


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "recommender-system_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "liboracle" not in text and "import oracle" not in text and "from oracle" not in text, f


@pytest.mark.parametrize("name", ["inst0", "inst1", "inst2", "inst30-40-10-2-10", "inst1000-1000-100-2-30"])
def test_parser_matches_reference_grammar(capi, orc, name):
    a, b = capi.parse_file(golden_in(name)), orc.parse_in(golden_in(name))
    assert (a.iters, a.alpha, a.feats, a.users, a.items) == (b.iters, b.alpha, b.feats, b.users, b.items)
    assert np.array_equal(a.row, b.row) and np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)


def test_parser_free_layout_and_number_forms(capi):
    # any white space layout; 2.0 / 2.000000 / 2e0 / +2 forms (fscanf %lf), negative ints
    inst = capi.parse_text("3\t1e-3 2\n\n2 3\n2   0 0 2.0 1\n2 2.500000\n")
    assert (inst.iters, inst.alpha, inst.feats, inst.users, inst.items, inst.nnz) == (3, 1e-3, 2, 2, 3, 2)
    assert inst.row.tolist() == [0, 1] and inst.col.tolist() == [0, 2] and inst.val.tolist() == [2.0, 2.5]
    # "%d" stops at '.', the next "%lf" continues there, as fscanf does
    inst = capi.parse_text("5.5 3 1 1 0")
    assert (inst.iters, inst.alpha, inst.feats) == (5, 0.5, 3)


@pytest.mark.parametrize("text,status,msg", [
    ("", 2, "Error in int argument."),
    ("x", 2, "Error in int argument."),
    ("10 abc", 3, "Error in double argument."),
    ("10 0.1 ", 2, "Error in int argument."),
    ("10 0.1 2 3 4", 4, "Error in multiple int argument."),
    ("10 0.1 2 3 4 2 0 0 1.0 1 1", 5, "Error in non-zero entry."),
    ("10 0.1 2 3 4 1 0 0 zz", 5, "Error in non-zero entry."),
])
def test_parser_error_strings(capi, text, status, msg):
    with pytest.raises(capi.ParseError) as e:
        capi.parse_text(text)
    assert e.value.status == status and str(e.value) == msg


def test_parser_missing_file(capi):
    with pytest.raises(capi.ParseError) as e:
        capi.parse_file("/nonexistent/file.in")
    assert str(e.value) == "Unable to open input file."


def test_random_restatement_matches_libc(capi):
    libc = C.CDLL(None)
    libc.random.restype = C.c_long
    for seed in (0, 1, 42, 2 ** 31):
        libc.srandom(C.c_uint(seed))
        g = capi.Rand()
        capi.host().mf_host_srandom(C.byref(g), seed)
        for _ in range(2000):
            assert capi.host().mf_host_random(C.byref(g)) == libc.random()
    g = capi.Rand()
    capi.host().mf_host_srandom(C.byref(g), 0)
    assert capi.host().mf_host_random(C.byref(g)) == 1804289383   # srandom(0) behaves as seed 1


@pytest.mark.parametrize("shape", [(3, 5, 2), (30, 40, 10), (943, 1682, 30), (1, 1, 1), (0, 4, 3)])
def test_init_factors_bit_equal_to_oracle(capi, orc, shape):
    u, i, k = shape
    L, R = capi.init_factors(u, i, k)
    Lo, Ro = orc.init_factors(u, i, k)
    assert np.array_equal(L, Lo) and np.array_equal(R, Ro)
    if u >= 3:
        Lb, Rb = capi.init_factors_block(u, i, k, 1, u - 2)
        assert np.array_equal(Lb, Lo[1:u - 1]) and np.array_equal(Rb, Ro)


def test_init_matches_inst0_mats_first_value(capi):
    L, R = capi.init_factors(3, 5, 2)
    assert abs(L[0, 0] * 2 - 0.840188) < 5e-7       # inst0.mats "Initial matrix L" 0.420094


def test_partition_block_rule_and_balance(capi):
    # BLOCK_LOW(id, p, n) = id*n/p  (mpiutil.h:8)
    for n, p in [(10, 3), (943, 8), (7, 8), (1000000, 8)]:
        b = capi.partition_users(n, p)
        assert b.tolist() == [i * n // p for i in range(p + 1)]
    # entry-balanced cuts: monotone, at row boundaries, each part within one row of the ideal share
    counts = np.random.default_rng(1).integers(0, 200, 5000)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    b = capi.partition_users(5000, 8, ptr)
    assert b[0] == 0 and b[-1] == 5000 and np.all(np.diff(b) >= 0)
    share = ptr[b[1:]] - ptr[b[:-1]]
    assert share.sum() == ptr[-1] and np.all(np.abs(share - ptr[-1] / 8) <= 2 * counts.max())


def test_synthetic_generator_properties(capi):
    users, items = 2000, 300
    row, col, val = capi.synth_block(0xC0FFEE + 4, users, items, 5, 15)
    counts = np.bincount(row, minlength=users)
    assert counts.min() >= 5 and counts.max() <= 15
    key = row.astype(np.int64) * items + col
    assert np.all(np.diff(key) > 0)                      # strictly (row, col)-sorted, no duplicates
    assert col.min() >= 0 and col.max() < items and set(np.unique(val)) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    # any block equals the corresponding slice of the whole (rank-local generation)
    r2, c2, v2 = capi.synth_block(0xC0FFEE + 4, users, items, 5, 15, u0=700, count=300)
    sel = (row >= 700) & (row < 1000)
    assert np.array_equal(r2, row[sel]) and np.array_equal(c2, col[sel]) and np.array_equal(v2, val[sel])
    # min_row > items is clipped to items (a user can rate each item once)
    r3, c3, _ = capi.synth_block(1, 10, 4, 6, 9)
    assert np.bincount(r3, minlength=10).tolist() == [4] * 10


@pytest.mark.parametrize("columns", ["uniform", "zipf"])
def test_survey_generators_exact_nnz_distinct_columns(capi, columns):
    """SURVEY 8d's generator: m ~ U[min, max] rescaled so that the row counts sum to nnz EXACTLY, m distinct columns per
    row -- uniform, or Zipf(1.0) item popularity (hot columns) --, sorted, ratings in {1..5}; a pure function of (seed, user):
    any block of users equals the corresponding slice of the whole."""
    users, items, nnz = 3000, 400, 123_457
    row, col, val = capi.synth_block(0xC0FFEE + 4, users, items, 20, 60, columns=columns, target_nnz=nnz)
    assert len(row) == nnz
    counts = np.bincount(row, minlength=users)
    raw, total = capi.synth_counts(0xC0FFEE + 4, users, items, 20, 60)
    assert np.all(np.abs(counts - raw * (nnz / total)) <= 1.0 + 1e-9)          # within one of the scaled raw draw
    key = row.astype(np.int64) * items + col
    assert np.all(np.diff(key) > 0)                      # strictly (row, col)-sorted: distinct columns inside a row
    assert col.min() >= 0 and col.max() < items and set(np.unique(val)) == {1.0, 2.0, 3.0, 4.0, 5.0}
    per_item = np.bincount(col, minlength=items)
    if columns == "uniform":
        assert per_item.max() < 2.0 * per_item.mean()    # binomial around nnz / items
    else:
        top = np.sort(per_item)[::-1]
        assert top[0] > 0.95 * users and top[0] > 5 * np.median(per_item)   # the hottest item is rated by nearly everybody
        assert abs(int(np.argmax(per_item)) - 0) > 0 or True                # (its id is scattered, not necessarily 0)
    parts = [capi.synth_block(0xC0FFEE + 4, users, items, 20, 60, u0=a, count=b, columns=columns, target_nnz=nnz)
             for a, b in ((0, 1), (1, 1233), (1234, 1766))]
    for i, whole in enumerate((row, col, val)):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), whole)
    # rows longer than half of the items: the uniform draw picks the complement; every item at most once
    r, c, _ = capi.synth_block(3, 50, 40, 25, 40, columns=columns, target_nnz=0)
    k = r.astype(np.int64) * 40 + c
    assert np.all(np.diff(k) > 0) and np.bincount(r, minlength=50).min() >= 25 and c.max() < 40


def _run_cli(capi, args):
    return subprocess.run([capi.CLI_PATH] + args, capture_output=True, text=True)


def test_cli_argument_errors(capi):
    r = _run_cli(capi, [])
    assert r.returncode == 255 and r.stdout == ""
    assert r.stderr == "Run ./matFact.out fileError: Missing input file name.\n"     # matFact.c:65-66
    r = _run_cli(capi, ["a", "b"])
    assert r.returncode == 255
    r = _run_cli(capi, ["/nonexistent.in"])
    assert r.returncode == 255 and r.stderr == "Error: Unable to open input file.\n" and r.stdout == ""


def test_cli_parse_error(capi, tmp_path):
    p = tmp_path / "bad.in"
    p.write_text("10 0.1 2 3 4 2 0 0 1.0")
    r = _run_cli(capi, [str(p)])
    assert r.returncode == 255 and r.stderr == "Error: Error in non-zero entry.\n" and r.stdout == ""


def test_headers_are_plain_c(tmp_path):
    """The drop-in boundary must be consumable by the reference's C compiler (gcc, C99, no C++)."""
    src = tmp_path / "inc.c"
    src.write_text('#include "matfact_hip.h"\n#include "matfact_host.h"\n'
                   'int main(void) { mf_problem p; mf_shard s; (void) p; (void) s; '
                   'return (int) mf_host_block_low(1, 2, 10) - 5 + (MF_OK != 0); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bench_accounting_and_skewed_generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    # A_upd(K) = 16 + 16K per update over two sweeps + 16K per owned row
    nnz, K, U, I = 1000, 100, 50, 20
    assert b.algorithmic_bytes(nnz, K, U) + b.algorithmic_bytes(nnz, K, I) == nnz * (16 + 16 * K) + 16 * K * (U + I)
    row, col, val = b.skewed_instance(7, 300, 200, 6000)
    key = row.astype(np.int64) * 200 + col
    assert np.all(np.diff(key) > 0) and col.max() < 200 and row.max() == 299
    lens = np.bincount(row, minlength=300)
    assert lens.min() >= 20 and lens.max() > 3 * np.median(lens)          # power-law activity
    pop = np.bincount(col, minlength=200)
    assert pop.max() > 4 * np.median(pop)                                 # power-law popularity


def test_bench_dump_rows_fixed_and_bounded():
    """--dump-outputs: the same rows in every run, in index order, and L plus R under 64 MB at every configuration."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 2 * b.DUMP_BYTES + 1024 <= 64e6
    for cfg in b.CONFIGS.values():
        for n, seed in ((cfg["users"], 1), (cfg["items"], 2)):
            rows = b.dump_rows(n, cfg["feats"], seed)
            assert np.array_equal(rows, b.dump_rows(n, cfg["feats"], seed))
            assert rows.size * cfg["feats"] * 8 <= b.DUMP_BYTES and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.array_equal(b.dump_rows(943, 30, 1), np.arange(943))        # a small factor is written whole


def test_parallel_parser_equals_sequential_semantics(capi, orc, tmp_path):
    """Inputs large enough for the parallel body parser (>= 65536 entries): same entries as the reference
    grammar gives, number forms included; irregular bodies fall back to the sequential parser and its errors."""
    rng = np.random.default_rng(11)
    n = 70000
    row = np.sort(rng.integers(0, 5000, n)).astype(np.int32)
    col = rng.integers(0, 4000, n).astype(np.int32)
    val = rng.integers(1, 6, n).astype(np.float64)
    forms = ["%d %d %.1f", "%d\t%d   %.6f", "%d %d %d", "%d %d %.3e"]
    lines = ["7", "0.00025", "12", "5000 4000 %d" % n]
    frac = rng.random(n)
    vals = np.where(frac < 0.1, val + 0.123456789012, val)
    for i in range(n):
        if frac[i] < 0.1:
            lines.append("%d %d %.12f" % (row[i], col[i], vals[i]))
        else:
            f = forms[i % len(forms)]
            lines.append(f % (row[i], col[i], int(val[i])) if f.endswith("%d") else f % (row[i], col[i], val[i]))
    text = "\n".join(lines) + "\n"
    inst = capi.parse_text(text)
    ref = orc.parse_in(text, is_text=True)
    assert (inst.iters, inst.alpha, inst.feats, inst.users, inst.items, inst.nnz) == (7, 0.00025, 12, 5000, 4000, n)
    assert np.array_equal(inst.row, ref.row) and np.array_equal(inst.col, ref.col)
    assert np.array_equal(inst.val, ref.val)            # bit-equal to Python's correctly rounded float()
    # one bad token deep inside the body: the sequential parser's error is what the caller sees
    bad = text.replace("\n%d %d" % (row[40000], col[40000]), "\n%d x%d" % (row[40000], col[40000]), 1)
    with pytest.raises(capi.ParseError) as e:
        capi.parse_text(bad)
    assert str(e.value) == "Error in non-zero entry."
    # too few entries
    with pytest.raises(capi.ParseError) as e:
        capi.parse_text(text[: len(text) // 2])
    assert str(e.value) == "Error in non-zero entry."
    # fscanf splits "12.5" read with %d into 12 and .5 -- the fast path must not accept it as one token
    odd = text.replace("\n%d %d " % (row[30000], col[30000]), "\n%d.5 %d " % (row[30000], col[30000]), 1)
    with pytest.raises(capi.ParseError) as e:       # %d reads 12, the next %d meets ".5" and fails
        capi.parse_text(odd)
    assert str(e.value) == "Error in non-zero entry."


@pytest.mark.parametrize("shape", [(150000, 3000, 37), (3000, 300000, 20), (1, 2200000, 3), (2200000, 1, 2)])
def test_parallel_init_equals_the_sequential_generator(capi, orc, shape):
    """Above ~4e6 draws the initial factors are produced by several threads, each jumping its generator ahead
    (matrix power of the lagged-Fibonacci recurrence): must equal glibc's srandom(0)/random() stream draw for draw
    (the oracle calls libc), for whole instances and for user blocks."""
    u, i, k = shape
    L, R = capi.init_factors(u, i, k)
    Lo, Ro = orc.init_factors(u, i, k)
    assert np.array_equal(L, Lo) and np.array_equal(R, Ro)
    u0, uc = u // 3, max(1, u // 2)
    uc = min(uc, u - u0)
    Lb, Rb = capi.init_factors_block(u, i, k, u0, uc)
    assert np.array_equal(Lb, Lo[u0:u0 + uc]) and np.array_equal(Rb, Ro)


def test_binary_cache_of_parsed_inputs(capi, tmp_path):
    """MATFACT_CACHE.  First parse misses and writes <content hash>-<size>.mfcache, the second one maps it
    (same header, same entries, no parse); the key is the file's CONTENT: an edited file misses; a truncated or foreign
    cache file is ignored; parse errors are reported as without a cache and leave nothing behind."""
    import numpy as np
    d = random_instance(3, 40, 30, 5, density=0.4, iters=7, alpha=0.01, float_ratings=True)
    src = tmp_path / "a.in"
    src.write_text(to_text(d))
    cache = tmp_path / "cache"
    cache.mkdir()
    plain = capi.parse_file(str(src))
    first, hit1 = capi.parse_file_cached(str(src), str(cache))
    files = sorted(os.listdir(cache))
    assert not hit1 and len(files) == 1 and files[0].endswith("-%d.mfcache" % src.stat().st_size)
    second, hit2 = capi.parse_file_cached(str(src), str(cache))
    assert hit2
    for inst in (first, second):
        assert (inst.iters, inst.alpha, inst.feats, inst.users, inst.items) == \
               (plain.iters, plain.alpha, plain.feats, plain.users, plain.items)
        assert np.array_equal(inst.row, plain.row) and np.array_equal(inst.col, plain.col)
        assert np.array_equal(inst.val, plain.val)
    # an edited file (same length, one digit changed) has another key
    txt = src.read_text()
    i = txt.rindex("\n", 0, len(txt) - 1) + 1
    edited = txt[:i] + txt[i:].replace(txt[i], "9" if txt[i] != "9" else "8", 1)
    assert len(edited) == len(txt) and edited != txt
    src.write_text(edited)
    third, hit3 = capi.parse_file_cached(str(src), str(cache))
    assert not hit3 and len(os.listdir(cache)) == 2
    # a damaged cache file is ignored and rewritten
    src.write_text(txt)
    victim = os.path.join(str(cache), files[0])
    with open(victim, "r+b") as f:
        f.truncate(100)
    again, hit4 = capi.parse_file_cached(str(src), str(cache))
    assert not hit4 and np.array_equal(again.val, plain.val)
    assert capi.parse_file_cached(str(src), str(cache))[1]
    # errors: same status as the plain parser, no cache file written
    bad = tmp_path / "bad.in"
    bad.write_text("3\n0.1\n2\n2 2 1\n0 0 x\n")
    n = len(os.listdir(cache))
    with pytest.raises(capi.ParseError) as e:
        capi.parse_file_cached(str(bad), str(cache))
    assert str(e.value) == "Error in non-zero entry." and len(os.listdir(cache)) == n
    with pytest.raises(capi.ParseError):
        capi.parse_file_cached(str(tmp_path / "missing.in"), str(cache))
    # no directory: the plain parser, no failure
    inst, hit = capi.parse_file_cached(str(src), str(tmp_path / "nowhere"))
    assert not hit and np.array_equal(inst.val, plain.val)
    # one flipped byte in the BODY (the size still fits the header): the stored hash of the entries catches it
    with open(victim, "r+b") as f:
        f.seek(64 + 16 * 5 + 8)
        b = f.read(1)
        f.seek(64 + 16 * 5 + 8)
        f.write(bytes([b[0] ^ 0x10]))
    again, hit5 = capi.parse_file_cached(str(src), str(cache))
    assert not hit5 and np.array_equal(again.val, plain.val) and np.array_equal(again.col, plain.col)
    assert capi.parse_file_cached(str(src), str(cache))[1]


def test_binary_cache_header_only_instance_and_many_open_problems(capi, tmp_path):
    """A header-only instance (nnz == 0) is cached as a bare 64-byte header; the hit points one past the mapping's end and
    must be released as a mapping, not handed to free() (round-2 advisor finding: `free(): invalid pointer`).  More
    cached problems may be open at once than the 16 slots the first version had."""
    import ctypes as C
    cache = tmp_path / "cache"
    cache.mkdir()
    empty = tmp_path / "empty.in"
    empty.write_text("1 0.1 2\n2 2 0\n")
    for expect_hit in (False, True, True):
        inst, hit = capi.parse_file_cached(str(empty), str(cache))   # parses, splits and frees the problem
        assert hit == expect_hit and (inst.users, inst.items, len(inst.row)) == (2, 2, 0)
    h = capi.host()
    live = []
    for n in range(40):
        f = tmp_path / ("m%d.in" % n)
        f.write_text("1 0.1 2\n3 3 2\n0 %d 1.0\n2 1 %d.5\n" % (n % 3, n))
        for _ in range(2):   # miss (writes the cache), then hit (kept open)
            p = capi.Problem()
            hit = C.c_int(0)
            assert h.mf_host_parse_file_cached(os.fsencode(str(f)), os.fsencode(str(cache)), C.byref(p), C.byref(hit)) == 0
            if hit.value:
                live.append(p)
            else:
                h.mf_host_free_problem(C.byref(p))
    assert len(live) == 40
    for n, p in enumerate(live):
        assert p.nnz == 2 and p.entries[1].value == n + 0.5
        h.mf_host_free_problem(C.byref(p))
        assert not p.entries


def test_every_switch_the_library_reads_is_documented():
    """One class of switches: the MF_* names the HIP sources read from the environment are exactly those of the
    "Documented" table of DESIGN.md 8b (MF_HIP_LIB apart: the Python binding reads it), and mf_config::describe() can
    name each of them."""
    import glob
    csrc = os.path.join(ROOT, "recommender-system_amd", "csrc")
    read = set()
    for path in glob.glob(os.path.join(csrc, "*.hip*")):
        read |= set(re.findall(r'getenv\("(MF_\w+)"\)', open(path).read()))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("*Documented*"):]
    rows = re.search(r"\n\n((?:\|[^\n]*\n)+)", table).group(1).splitlines()[2:]
    documented = set()
    for row in rows:
        documented |= set(re.findall(r"`(MF_[A-Z0-9_]+)", row.split(" | ")[0]))
    assert len(rows) > 5 and "MF_HIP_LIB" in documented
    assert read == documented - {"MF_HIP_LIB"}, (sorted(read - documented), sorted(documented - read))
    config = open(os.path.join(csrc, "mf_config.hip.h")).read()
    describe = config[config.index("std::string describe() const"):]
    named = set(re.findall(r'add\("(MF_\w+)"', describe))
    assert read == named, sorted(read ^ named)
