"""estislands: the command line against TCLAP's recorded answers, the open and parse errors and the runs that need no device
(CPU), the oracle's own edge cases, the host code under AddressSanitizer, and on the GPU the island catalogue
(include/defuse_est.h through defuse_amd/est.py) and the drop-in binary against tests/estislands_oracle.py."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import estislands_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "estislands")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_answers", "tclap_estislands.json")

# tools/estislands.cpp:27-30, in the form of tests/test_cli_ref.py's SPECS: (flag, name, description, type, required)
SPEC = ("Identify products of cotranscribed regions using est islands", [
    ("e", "ests", "EST Alignments Filename", "string", 1), ("b", "breaks", "Breakpoint Alignments Filename", "string", 1),
    ("o", "output", "Output Filtered Alignments Filename", "string", 1)])
# command lines that end inside the parser
FAILING_LINES = [["--help"], ["-h"], ["--version"], [], ["-e", "a"], ["-e", "a", "-e", "b"], ["--bogus", "1"], ["stray"], ["-e"], ["-eb"],
                 ["--ests=a"], ["-e", "a", "-b"], ["--", "-e", "a"], ["-e", "a", "-b", "b"], ["-e", "a", "-b", "b", "-o", "c", "d"]]
# command lines TCLAP accepts
PARSED_LINES = [["-e", "E", "-b", "B", "-o", "O"], ["--output", "-", "--breaks", "-", "--ests", "-"]]


def specs_digest():
    return hashlib.sha256(json.dumps([SPEC, FAILING_LINES, PARSED_LINES], sort_keys=True).encode()).hexdigest()


def run_tool(est, brk, out, env=None, tool=TOOL, cwd=None):
    e = dict(os.environ, **(env or {}))
    p = subprocess.run([tool, "-e", est, "-b", brk, "-o", out], capture_output=True, env=e, timeout=900, stdin=subprocess.DEVNULL, cwd=cwd)
    return p.stdout.decode("latin-1"), p.stderr.decode("latin-1"), p.returncode


def est_row(chrom, ts, te):
    return b"585\t0\t0\t0\t0\t0\t0\t0\t0\t+\tq\t1\t0\t1\t%s\t0\t%s\t%s\t1\t1,\t0,\t0," % (chrom, ts, te)


def break_row(chrom, ts, te, name=b"b"):
    return b"1\t0\t0\t0\t0\t0\t0\t0\t+\t%s\t1\t0\t1\t%s\t0\t%s\t%s\t1\t1,\t0,\t0," % (name, chrom, ts, te)


# ---------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def tool(built):
    from defuse_amd import build
    build.build_tools()
    return TOOL


@pytest.fixture(scope="module")
def tclap_answers():
    with open(GOLDEN) as f:
        d = json.load(f)
    assert d["specs_sha256"] == specs_digest(), "SPEC or the command lines changed: tests/golden/make_estislands_answers.py"
    return {tuple(a["args"]): a for a in d["answers"]}


def test_cli_equals_tclap(tool, tclap_answers, tmp_path):
    for args in FAILING_LINES:
        ref = tclap_answers[tuple(args)]
        assert ref["returncode"] != 0 or args[0] in ("--help", "-h", "--version"), args
        got = subprocess.run([tool] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL, cwd=tmp_path)
        assert (got.returncode, got.stdout, got.stderr) == (ref["returncode"], ref["stdout"], ref["stderr"]), args


def test_parsed_values_equal_tclap(tool, tclap_answers, tmp_path):
    """What TCLAP parses, the tool takes as file names: "-" is a file of that name, not stdin."""
    ref = tclap_answers[tuple(PARSED_LINES[0])]
    assert ref["returncode"] == 0 and "ests\tE\n" in ref["stdout"] and "output\tO\n" in ref["stdout"]
    ref = tclap_answers[tuple(PARSED_LINES[1])]
    assert ref["returncode"] == 0 and "ests\t-\n" in ref["stdout"] and "breaks\t-\n" in ref["stdout"]
    for args, name in zip(PARSED_LINES, ("E", "-")):
        got = subprocess.run([tool] + args, input="1\t" * 30, capture_output=True, text=True, cwd=tmp_path)
        assert (got.returncode, got.stdout, got.stderr) == (1, "", "Error: Unable to open est file %s\n" % name), args
        assert os.listdir(tmp_path) == []


def _files(d, est=b"", brk=b""):
    e, b = os.path.join(d, "est.txt"), os.path.join(d, "breaks.psl")
    with open(e, "wb") as f:
        f.write(est)
    with open(b, "wb") as f:
        f.write(brk)
    return e, b


def test_open_errors_in_order(tool, tmp_path):
    """EST file, breaks file, output file: the first that cannot be opened is named, exit 1; the output exists only if both
    inputs opened."""
    d = str(tmp_path)
    est, brk = _files(d, est_row(b"chr1", b"100", b"200") + b"\n", break_row(b"chr1", b"120", b"150") + b"\n")
    out = os.path.join(d, "out.psl")
    nope = os.path.join(d, "nope")
    cases = [((nope, nope, out), "Error: Unable to open est file %s\n" % nope, False),
             ((nope, brk, out), "Error: Unable to open est file %s\n" % nope, False),
             ((est, nope, out), "Error: Unable to open break alignments file %s\n" % nope, False),
             ((est, brk, os.path.join(nope, "out")), "Error: Unable to open output file %s\n" % os.path.join(nope, "out"), False),
             ((est, brk, d), "Error: Unable to open output file %s\n" % d, False)]
    for (e, b, o), msg, _ in cases:
        assert run_tool(e, b, o, env={"DEFUSE_GPU": "999"}) == ("", msg, 1), (e, b, o)
        assert not os.path.exists(out)
    # a directory opens as an empty input (ifstream), so the output is created and stays empty
    assert run_tool(d, brk, out, env={"DEFUSE_GPU": "999"}) == ("", "", 0)
    assert open(out, "rb").read() == b""


def test_bad_integer_in_est_file(tool, tmp_path):
    """The reference dies of an uncaught bad_lexical_cast while reading the EST table: here an Error line, exit 1, and no
    output file, since the reference had not opened it yet — even when the breaks file is missing too."""
    d = str(tmp_path)
    body = b"".join(est_row(b"chr1", b"%d" % (k * 10), b"%d" % (k * 10 + 50)) + b"\n" for k in range(5000))
    for bad, shown in ((b"12x", "12x"), (b"", ""), (b"2147483648", "2147483648"), (b" 5", " 5")):
        est, brk = _files(d, body + est_row(b"chr2", b"7", bad) + b"\n" + body, break_row(b"chr1", b"20", b"40") + b"\n")
        out = os.path.join(d, "out.psl")
        for b in (brk, os.path.join(d, "missing")):
            want = "Error: bad integer '%s' in est file %s line 5001\n" % (shown, est)
            assert run_tool(est, b, out, env={"DEFUSE_GPU": "999"}) == ("", want, 1), bad
            assert not os.path.exists(out)
            assert eo.run(open(est, "rb").read(), None)[1:] == (want.replace(est, "EST"), 1)
    # a '\r' belongs to the last field: an 18-field CRLF row has a bad tEnd
    est, brk = _files(d, est_row(b"chr1", b"1", b"2").rsplit(b"\t", 4)[0] + b"\r\n", b"")
    assert run_tool(est, brk, os.path.join(d, "o"), env={"DEFUSE_GPU": "999"})[1:] == ("Error: bad integer '2\r' in est file %s line 1\n" % est, 1)


def test_runs_that_need_no_device(tool, tmp_path):
    """No used break rows, no EST rows, or no break row on a chromosome of the table: empty output, exit 0, and no device is
    opened (DEFUSE_GPU names one that does not exist, and this passes on a machine without a GPU)."""
    d = str(tmp_path)
    ests = b"".join(est_row(c, b"%d" % (k * 100), b"%d" % (k * 100 + 500)) + b"\n" for k in range(100) for c in (b"chr1", b"chrM"))
    row = break_row(b"chr1", b"10", b"20")
    junk_breaks = b"#comment\n\nmatch\tmis\n" + b"\t".join(row.split(b"\t")[:17]) + b"\n" + b"x" + row[1:] + b"\n"
    out = os.path.join(d, "out.psl")
    cases = [(ests, b""), (ests, junk_breaks), (b"", break_row(b"chr1", b"10", b"20") + b"\n"),
             (b"# only a header\n", break_row(b"chr1", b"10", b"20") + b"\n"), (ests, break_row(b"chr9", b"10", b"20") + b"\n"),
             (ests, break_row(b"chrMT_random", b"100", b"120") + b"\n")]
    for est_data, brk_data in cases:
        est, brk = _files(d, est_data, brk_data)
        with open(out, "wb") as f:
            f.write(b"old contents")
        assert run_tool(est, brk, out, env={"DEFUSE_GPU": "999"}) == ("", "", 0), (est_data[:40], brk_data[:40])
        assert open(out, "rb").read() == b"" == eo.run(est_data, brk_data)[0]
    # a bad integer in the breaks file with nothing to look up: the (empty) output exists, then the Error line
    est, brk = _files(d, b"", break_row(b"chr1", b"10", b"20") + b"\n" + break_row(b"chr1", b"1O", b"20") + b"\n")
    want = "Error: bad integer '1O' in break alignments file %s line 2\n" % brk
    assert run_tool(est, brk, out, env={"DEFUSE_GPU": "999"}) == ("", want, 1)
    assert open(out, "rb").read() == b""
    # the breaks file as the output: truncated before it is read, as the reference's ofstream does
    est, brk = _files(d, ests, break_row(b"chr1", b"10", b"20") + b"\n")
    assert run_tool(est, brk, brk, env={"DEFUSE_GPU": "999"}) == ("", "", 0)
    assert open(brk, "rb").read() == b""
    # DEFUSE_TIMING names the stages
    est, brk = _files(d, ests, b"")
    got = run_tool(est, brk, out, env={"DEFUSE_GPU": "999", "DEFUSE_TIMING": "1"})
    assert got[2] == 0
    for stage in ("read+parse", "catalogue", "lookup", "write"):
        assert "[estislands] %s " % stage in got[1]


def test_no_device_paths_under_asan(built, tmp_path):
    """The host code (threaded parse, id merge, error paths) under AddressSanitizer + UBSan."""
    from defuse_amd import build
    asan = build.build_sanitized("asan")["estislands"]
    env = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "DEFUSE_GPU": "999"}
    rng = np.random.default_rng(5)
    c, ts, te = eo.segment_columns(rng, 60000, degenerate=0.01)
    d = str(tmp_path)
    est_data = eo.est_table(rng, c, ts, te, crlf=True)
    assert len(est_data) > (1 << 20)                       # parsed in pieces
    bad = est_data + est_row(b"chr1", b"5", b"-") + b"\n"
    out = os.path.join(d, "out")
    for threads in ("1", "5"):
        e = dict(env, DEFUSE_THREADS=threads)
        est, brk = _files(d, est_data, b"#none\n")
        assert run_tool(est, brk, out, env=e, tool=asan) == ("", "", 0)
        est, brk = _files(d, bad, b"")
        r = run_tool(est, brk, out, env=e, tool=asan)
        assert r[2] == 1 and r[1].startswith("Error: bad integer '-' in est file") and "runtime error" not in r[1]
        est, brk = _files(d, b"", break_row(b"chr1", b"1", b"2") + b"\n" + break_row(b"chr1", b"+", b"2") + b"\n")
        r = run_tool(est, brk, out, env=e, tool=asan)
        assert r[2] == 1 and r[1].startswith("Error: bad integer '+'") and "AddressSanitizer" not in r[1]


# ---- the oracle's own edge cases
def test_oracle_padding_edges():
    isl = ([1000], [2000])
    assert eo.contained(isl, 700, 2300)                  # exactly +-300
    assert not eo.contained(isl, 699, 2300)
    assert not eo.contained(isl, 700, 2301)
    assert eo.contained(isl, 1500, 1600) and eo.contained(isl, 700, 1000)
    assert not eo.contained(isl, 700, 999)              # inside the padding, but the island starts after q.end: never visited
    assert not eo.contained(([], []), 1, 2)


def test_oracle_unvisited_later_island():
    """lower_bound, one step back, walk while island.start <= q.end: an island starting after q.end is never visited, even
    though its padding would contain q."""
    isl = eo.catalog({b"1": [(100, 200), (1000, 1100)]})[b"1"]
    assert isl == ([100, 1000], [200, 1100])
    assert not eo.contained(isl, 800, 950)               # inside [700, 1400], but 1000 > 950
    assert eo.contained(isl, 800, 1000)                  # now visited
    assert not eo.contained(isl, 150, 600) and eo.contained(isl, 150, 500)
    # the step back: a query starting after the last island's start still sees it
    assert eo.contained(isl, 1050, 1390)


def test_oracle_merge_rules():
    assert eo.merge([(10, 20), (21, 30)]) == [(10, 20), (21, 30)]       # start > end: a new island
    assert eo.merge([(10, 20), (20, 30)]) == [(10, 30)]                  # touching merges
    assert eo.merge([(10, 100), (20, 30), (40, 50)]) == [(10, 100)]      # nested
    assert eo.merge([(30, 40), (10, 20)]) == [(10, 20), (30, 40)]
    # degenerate first segment: the reference's loop emits it twice
    assert eo.merge([(50, 40)]) == [(50, 40), (50, 40)]
    assert eo.merge([(50, 40), (60, 70)]) == [(50, 40), (50, 40), (60, 70)]
    # a degenerate segment inside an island changes nothing; one past it resets the running end
    assert eo.merge([(10, 100), (50, 40), (60, 70)]) == [(10, 100)]
    assert eo.merge([(10, 20), (30, 25), (31, 32)]) == [(10, 20), (30, 25), (31, 32)]


def test_oracle_tie_order_invariance():
    """With end >= start everywhere, the islands do not depend on the order of equal starts."""
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(1, 40))
        s = rng.integers(0, 60, size=n)
        e = s + rng.integers(0, 30, size=n)
        segs = list(zip(s.tolist(), e.tolist()))
        want = eo.merge(segs)
        for _ in range(5):
            assert eo.merge([segs[k] for k in rng.permutation(n)]) == want


def test_oracle_canonical_order_on_degenerate_rows():
    """With end < start the order of equal starts matters; the canonical order is file order among equal starts."""
    a, b = (50, 40), (50, 80)
    assert eo.merge([(10, 20), a, b]) == [(10, 20), (50, 40), (50, 80)]
    assert eo.merge([(10, 20), b, a]) == [(10, 20), (50, 80)]
    cat = eo.read_ests(est_row(b"chrM", b"49", b"40") + b"\n" + est_row(b"MT", b"49", b"80") + b"\n" + est_row(b"M", b"9", b"20") + b"\n")
    assert list(cat) == [b"MT"] and eo.catalog(cat)[b"MT"] == ([10, 50, 50], [20, 40, 80])


def test_oracle_rows_and_names():
    text = (b"\n#x\t" + b"1\t" * 20 + b"\n" + est_row(b"chrM", b"+9", b"-20") + b"\r\n" + est_row(b"chrchr1", b"0", b"5") + b"\n"
            + b"12\t" * 16 + b"\n" + est_row(b"M", b"2147483647", b"0"))
    got = [(no, c, s, e) for no, _, c, s, e in eo.rows(text, eo.EST_FIELDS)]
    assert got == [(3, b"MT", 10, -20), (4, b"chr1", 1, 5), (6, b"MT", -2 ** 31, 0)]      # int(tStart) + 1 wraps as in C++


def test_library_exports_est():
    import ctypes
    from defuse_amd.dsa import LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for sym in ("est_catalog_create", "est_catalog_islands", "est_catalog_contained", "est_catalog_destroy", "est_last_error"):
        assert hasattr(lib, sym)


# ---------------------------------------------------------------------------------------------- GPU
def _oracle_islands(c, s, e, n_chrom):
    """The oracle's islands of columns with dense ids, flattened as est_catalog_islands returns them."""
    by = {}
    for k in range(len(c)):
        by.setdefault(int(c[k]), []).append((int(s[k]), int(e[k])))
    starts, ends, off = [], [], [0]
    for ch in range(n_chrom):
        isl = eo.merge(by.get(ch, []))
        starts += [x for x, _ in isl]
        ends += [y for _, y in isl]
        off.append(len(starts))
    return np.array(starts, dtype=np.int32), np.array(ends, dtype=np.int32), np.array(off, dtype=np.int64)


@pytest.mark.gpu
def test_gpu_islands_equal_oracle(built):
    from defuse_amd import est
    rng = np.random.default_rng(11)
    n = 2_100_000
    c, ts, te = eo.segment_columns(rng, n, n_chroms=40, span=300_000_000, degenerate=0.002)
    s, e = ts + 1, te
    # heavy ties: many equal starts, degenerate rows among them, and a chromosome that starts with a degenerate row
    s[:2000] = 500_000
    c[:2000] = 3
    c[2000], s[2000], e[2000] = 39, -5, -10
    c[2001], s[2001], e[2001] = 39, -5, 100
    c = np.where(c == 17, 18, c)                             # chromosome 17 without rows
    want = _oracle_islands(c, s, e, 41)
    with est.catalog(c, s, e, 41) as cat:
        got = cat.islands()
    assert int((e < s).sum()) > 1000
    assert len(want[0]) > 100000
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert want[2][17] == want[2][18] and want[2][41] == want[2][40]      # empty chromosomes 17 and 40
    # end >= start everywhere: every order of equal starts gives these islands; the catalogue of a shuffled input agrees
    ok = e >= s
    perm = rng.permutation(int(ok.sum()))
    c2, s2, e2 = c[ok][perm], s[ok][perm], e[ok][perm]
    with est.catalog(c2, s2, e2, 41) as cat:
        got = cat.islands()
    for g, w in zip(got, _oracle_islands(c[ok], s[ok], e[ok], 41)):
        assert np.array_equal(g, w)
    # n = 0, and extremes of int
    with est.catalog([], [], [], 3) as cat:
        g = cat.islands()
        assert len(g[0]) == 0 and list(g[2]) == [0, 0, 0, 0]
        r, t = cat.contained([0, 1], [1, 2], [3, 4])
        assert list(r) == [0, 0] and t.n_islands == 0
    xs = [-2 ** 31, -2 ** 31 + 5, 2 ** 31 - 10, 2 ** 31 - 1, 0]
    xe = [-2 ** 31 + 3, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0]
    with est.catalog([0] * 5, xs, xe, 1) as cat:
        assert [list(a) for a in cat.islands()] == [list(a) for a in _oracle_islands([0] * 5, xs, xe, 1)]


@pytest.mark.gpu
def test_gpu_contained_equals_oracle(built):
    from defuse_amd import est
    rng = np.random.default_rng(12)
    c, ts, te = eo.segment_columns(rng, 400_000, n_chroms=12, span=100_000_000, degenerate=0.001)
    s, e = ts + 1, te
    by = {}
    for k in range(len(c)):
        by.setdefault(int(c[k]), []).append((int(s[k]), int(e[k])))
    cat_o = {ch: eo.catalog({0: v})[0] for ch, v in by.items()}
    n = 1_050_000
    qc = rng.integers(-1, 13, size=n)                          # -1 and 12: chromosomes without islands
    pick = [cat_o[int(x)] if 0 <= x < 12 else None for x in qc]
    qs = np.zeros(n, dtype=np.int64)
    qe = np.zeros(n, dtype=np.int64)
    for k in range(n):
        isl = pick[k]
        r = rng.random()
        if isl is None or r < 0.1:
            qs[k] = int(rng.integers(0, 100_000_000))
            qe[k] = qs[k] + int(rng.integers(-5, 3000))
            continue
        j = int(rng.integers(0, len(isl[0])))
        a, b = isl[0][j], isl[1][j]
        if r < 0.5:
            qs[k], qe[k] = a - 300 + int(rng.integers(-1, 2)), b + 300 + int(rng.integers(-1, 2))
        else:
            qs[k] = a + int(rng.integers(-1500, 1500))
            qe[k] = qs[k] + int(rng.integers(-10, 6000))
    want = np.array([0 if pick[k] is None else int(eo.contained(pick[k], int(qs[k]), int(qe[k]))) for k in range(n)], dtype=np.uint8)
    with est.catalog(c, s, e, 12) as cat:
        got, t = cat.contained(qc, qs, qe)
        assert t.n_queries == n and t.n_contained == int(want.sum())
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (int(bad[0]), int(qc[bad[0]]), int(qs[bad[0]]), int(qe[bad[0]]))
        assert 0.05 < want.mean() < 0.95
    # hand-made edges: +-300, the unvisited later island, the step back
    with est.catalog([0, 0, 0], [1000, 100, 5000], [1100, 200, 5000], 1) as cat:
        qs = [700, 699, 700, 800, 800, 1050, -200, 4700]
        qe = [1400, 1400, 1401, 950, 1000, 1390, 500, 5300]
        got, _ = cat.contained([0] * 8, qs, qe)
        isl = eo.catalog({0: [(1000, 1100), (100, 200), (5000, 5000)]})[0]
        assert list(got) == [int(eo.contained(isl, a, b)) for a, b in zip(qs, qe)] == [1, 0, 0, 0, 1, 1, 1, 1]


def _tool_case(d, seed, n_est, n_break, crlf=False, degenerate=0.002):
    rng = np.random.default_rng(seed)
    c, ts, te = eo.segment_columns(rng, n_est, span=20_000_000, degenerate=degenerate)
    est_data = eo.est_table(rng, c, ts, te, crlf=crlf)
    cat = eo.catalog(eo.read_ests(est_data))
    qc, qs, qe = eo.queries_near(rng, cat, eo.CHROMS, n_break, span=20_000_000)
    brk_data = eo.break_psl(rng, qc, qs, qe, crlf=crlf)
    est, brk = _files(d, est_data, brk_data)
    return est, brk, est_data, brk_data


@pytest.mark.gpu
def test_gpu_tool_matches_oracle(tool, tmp_path):
    d = str(tmp_path)
    out = os.path.join(d, "out.psl")
    for seed, crlf, threads in ((1, False, "8"), (2, True, "3"), (3, False, "1")):
        est, brk, est_data, brk_data = _tool_case(d, seed, 300_000, 60_000, crlf=crlf)
        want_out, want_err, want_rc = eo.run(est_data, brk_data)
        assert want_rc == 0 and 6_000 < want_out.count(b"\n") < 57_000
        assert (b"\r\n" in want_out) == crlf
        got = run_tool(est, brk, out, env={"DEFUSE_THREADS": threads})
        assert got == ("", "", 0)
        assert open(out, "rb").read() == want_out, (seed, crlf)


@pytest.mark.gpu
def test_gpu_tool_bad_integer_in_breaks(tool, tmp_path):
    """The contained lines before the bad row, then the Error line, exit 1."""
    d = str(tmp_path)
    est, brk, est_data, brk_data = _tool_case(d, 4, 100_000, 20_000)
    ls = brk_data.split(b"\n")
    at = next(k for k in range(15000, len(ls)) if len(ls[k].split(b"\t")) >= 18)
    f = ls[at].split(b"\t")
    f[16] = b"9e5"
    ls[at] = b"\t".join(f)
    brk_data = b"\n".join(ls)
    with open(brk, "wb") as fh:
        fh.write(brk_data)
    want_out, want_err, want_rc = eo.run(est_data, brk_data)
    assert want_rc == 1 and want_out.count(b"\n") > 1500
    out = os.path.join(d, "out.psl")
    got = run_tool(est, brk, out)
    assert got == ("", want_err.replace("BREAKS", brk), 1)
    assert open(out, "rb").read() == want_out


@pytest.mark.gpu
def test_gpu_tool_runs_are_identical(tool, tmp_path):
    d = str(tmp_path)
    est, brk, est_data, brk_data = _tool_case(d, 5, 200_000, 50_000, degenerate=0.01)
    outs = []
    for k, threads in enumerate(("8", "2")):
        out = os.path.join(d, "out%d.psl" % k)
        got = run_tool(est, brk, out, env={"DEFUSE_THREADS": threads, "DEFUSE_TIMING": "1"})
        assert got[0] == "" and got[2] == 0
        for stage in ("read+parse", "catalogue", "lookup", "write"):
            assert "[estislands] %s " % stage in got[1]
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] == eo.run(est_data, brk_data)[0]
