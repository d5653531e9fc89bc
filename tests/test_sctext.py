"""include/defuse_sc.h, section "cluster text" (defuse_amd/csrc/sct_api.hip through defuse_amd/sctext.py): setcover's cluster
file parsed, covered, filtered and printed on the GPU, against tests/sctext_oracle.py byte for byte; the oracle itself against
oracle/setcover_oracle.py and against what the default tool prints; and the tool's DEFUSE_SC_DEVICE_TEXT=1 path against its
default path."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import abi, sctext_oracle as so
from tests import test_setcover as ts

TOOL = ts.TOOL
BAD_LINE_CASES = [m for m in ts.test_setcover_tool_reports_the_first_bad_line_as_a_serial_reader_would.pytestmark
                  if m.name == "parametrize" and m.args[0] == "bad,message"][0].args[1]
WRITER_BAD_LINE = "-3\t1\t12\t1\tchr1\t+\t5\t9"          # of test_setcover_tool_writer_reports_a_negative_cluster_id_on_an_end_one_line
WELL_FORMED = [(1, 0), (2, 1), (3, 2)]                  # (seed, big) of test_gpu_cover_matches_oracle; big: the wave path


def cluster_file(clusters, shuffle_seed=None):
    """The bytes ts.write_cluster_file writes for the clusters (and its lines shuffled, if asked)."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clusters.txt")
        ts.write_cluster_file(path, clusters)
        data = open(path, "rb").read()
    if shuffle_seed is not None:
        lines = data.decode().splitlines()
        np.random.default_rng(shuffle_seed).shuffle(lines)
        data = ("\n".join(lines) + "\n").encode()
    return data


@functools.lru_cache(maxsize=None)
def well_formed(seed, big):
    return cluster_file(ts.random_clusters(seed, big=big))


@functools.lru_cache(maxsize=None)
def expected(data, m):
    return so.setcover_text(data, m)


def text_of(lines, newline_at_end=True):
    return ("\n".join(lines) + ("\n" if newline_at_end else "")).encode()


def bad_line_file(bad, later_bad_line=True):
    """The file of the bad-line test: GOOD_LINES with `bad` as line 301 and (unless told otherwise) another bad line behind it."""
    lines = list(ts.GOOD_LINES)
    lines.insert(300, bad)
    if later_bad_line:
        lines.insert(361, "9\ty\t1")
    return text_of(lines)


# ---- no GPU: the binding, and the oracle pinned to behaviour that is tested already -------------------------------------------

def test_header_and_binding(built):
    from defuse_amd import sctext
    sizes, n_functions = abi.check("defuse_sc.h", sctext, r"sct_[a-z_]+", constants=sctext.CONSTANTS)
    assert n_functions == len(sctext.EXPORTS) == len(sctext.PROTOTYPES) == 9
    assert sizes == [ctypes.sizeof(sctext.SctResult), ctypes.sizeof(sctext.SctTiming)] == [80, 72]
    e = sctext.SctError(-4, "z")
    assert str(e) == "sct error -4: z" and e.code == -4
    assert (so.OK, so.READ_STOP, so.NEGATIVE_ELEMENT, so.WRITE_STOP) == (sctext.OK, sctext.READ_STOP, sctext.NEGATIVE_ELEMENT, sctext.WRITE_STOP)
    assert (so.EMPTY_LINE, so.FEW_FIELDS, so.BAD_INTEGER, so.BAD_CLUSTER_ID) == (1, 2, 3, 4)


@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("seed,big", WELL_FORMED)
def test_oracle_equals_the_setcover_oracle_on_well_formed_files(tmp_path, seed, big, m):
    from oracle import setcover_oracle as o
    data = well_formed(seed, big)
    p = tmp_path / "clusters.txt"
    p.write_bytes(data)
    exp = o.setcover(str(p), m)
    assert expected(data, m) == (so.OK, 0, 0, exp.encode()) and len(exp.splitlines()) > 100


@pytest.mark.parametrize("bad,message", BAD_LINE_CASES)
def test_oracle_stops_where_the_default_tool_does(built, tmp_path, bad, message):
    """Status, kind and line number of the oracle against the default tool's message (these runs end before a GPU is needed)."""
    from defuse_amd import build
    build.build_tools()
    data = bad_line_file(bad)
    p = tmp_path / "clusters.txt"
    p.write_bytes(data)
    r = subprocess.run([TOOL, "-c", str(p), "-m", "3", "-o", str(tmp_path / "out.sc")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr == message.format(n=301, path=str(p))
    status, kind, line, out = expected(data, 3)
    assert (status, line, out) == (so.READ_STOP, 301, b"")
    texts = {so.EMPTY_LINE: "Error: Empty clusters line 301 of", so.FEW_FIELDS: "Error: Format error for clusters line 301 of",
             so.BAD_INTEGER: "Failed to interpret line:\n" + bad + "\n", so.BAD_CLUSTER_ID: "Error: Invalid cluster ID for line 301 of"}
    assert r.stderr.startswith(texts[kind])


def test_oracle_integer_rule_and_lines():
    assert [so.lexical_int(f) for f in (b"+5", b"-0", b"007", b"2147483647", b"-2147483648")] == [5, 0, 7, 2147483647, -2147483648]
    assert [so.lexical_int(f) for f in (b"2147483648", b"-2147483649", b" 5", b"5 ", b"", b"+", b"-", b"12\r", b"1e3", b"0x1")] == [None] * 10
    assert so.lines_of(b"") == [] and so.lines_of(b"a") == [b"a"] and so.lines_of(b"a\n") == [b"a"] and so.lines_of(b"a\n\n") == [b"a", b""]


# ---- GPU: the library against the oracle, byte for byte ----------------------------------------------------------------------

def run_pieces(ctx, pieces, m):
    """pieces: (bytes, final) in order, each of which must be consumed whole.  Returns (result dict, output bytes)."""
    ctx.begin()
    for text, final in pieces:
        assert ctx.add(text, final=final) == len(text)
    res = ctx.cover(m)
    return res, ctx.fetch()


def check(data, m, piece=None, ctx=None, pieces=None):
    """One run of the library on `data` (in one piece, in pieces of `piece` bytes, or as the `pieces` given) against the
    oracle: status, kind, line, the stopping line's place in the input, the counts and every output byte."""
    from defuse_amd import sctext
    if pieces is not None:
        res, out = run_pieces(ctx, pieces, m)
    elif ctx is not None:
        res, out = run_pieces(ctx, [(data, True)], m)
    else:
        res, out = sctext.setcover_text(data, m, piece=piece)
    status, kind, line, exp = expected(data, m)
    assert (res["status"], res["stop_kind"], res["stop_line"]) == (status, kind, line)
    lines = so.lines_of(data)
    assert res["n_lines"] == len(lines)
    if line:
        assert data[res["stop_offset"]:res["stop_offset"] + res["stop_len"]] == lines[line - 1]
    assert res["out_bytes"] == len(out) == len(exp)
    assert out == exp
    if status in (so.OK, so.WRITE_STOP):
        assert res["n_kept_lines"] == exp.count(b"\n")
        members = [l.split(b"\t") for l in lines if so.parse(l)[2] == 0]
        assert res["n_members"] == len(members)
        assert res["n_clusters"] == max((int(f[0]) for f in members), default=-1) + 1
        assert res["max_element"] == max((int(f[2]) for f in members), default=-1)
    return res, out


@pytest.mark.gpu
@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("seed,big", WELL_FORMED)
def test_gpu_well_formed_files(built, seed, big, m):
    res, out = check(well_formed(seed, big), m)
    assert res["status"] == so.OK and out.count(b"\n") > 100


@pytest.mark.gpu
def test_gpu_lines_in_any_order(built):
    """The shuffled file of test_setcover_tool_cluster_lines_in_any_order: clusters[id] in file order whatever the lines' order."""
    data = cluster_file(ts.random_clusters(11, n_clusters=300, n_frag=900, big=1), shuffle_seed=5)
    res, out = check(data, 3)
    assert out.count(b"\n") > 100


@pytest.mark.gpu
@pytest.mark.parametrize("seed,big", WELL_FORMED)
def test_gpu_owner_equals_sc_cover(built, seed, big):
    from defuse_amd import sc, sctext
    clusters = ts.random_clusters(seed, big=big)
    sol, t = sc.cover(clusters)
    exp = np.full(max(e for c in clusters for e in c) + 1, -1, dtype=np.int32)
    for c, lst in enumerate(sol):
        exp[lst] = c
    with sctext.SctContext() as ctx:
        ctx.begin()
        ctx.add(well_formed(seed, big))
        res = ctx.cover(0)
        owner = ctx.owner()
        tm = ctx.timing()
    assert res["max_element"] + 1 == len(exp) and np.array_equal(owner, exp)
    assert (tm["n_components"], tm["n_large"]) == (t.n_components, t.n_large) and tm["n_pieces"] == 1


@functools.lru_cache(maxsize=None)
def pieces_file():
    """A file of several 4096-byte pieces whose last line is kept for m <= 1 (cluster 9999 owns fragment 99999 alone)."""
    data = cluster_file(ts.random_clusters(4, n_clusters=90, n_frag=300)) + b"9999\t0\t99999\t1\tchr1\t+\t7\t8\n9999\t1\t99999\t0\tchr2\t-\t9\t10\n"
    assert len(data) > 5 * 4096 and len(so.lines_of(data)) < 1500
    return data


def test_pieces_file_is_what_it_claims():
    """Precondition of test_gpu_pieces, on the oracle alone: the last line is kept exactly where its cluster is."""
    data = pieces_file()
    for m in (1, 3):
        status, _, _, out = expected(data, m)
        assert status == so.OK and out.endswith(b"chr2\t-\t9\t10\n") == (m == 1) and 100 < out.count(b"\n") < len(so.lines_of(data))
        assert expected(data[:-1], m)[3] == out


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3])
def test_gpu_pieces(built, m):
    """One file four ways: as one piece, as one piece per line, cut every 4096 bytes in the middle of lines with final = 0
    (the rest given again from `consumed`), and with its last newline removed.  One result, the same bytes."""
    from defuse_amd import sctext
    data = pieces_file()
    exp = expected(data, m)[3]
    assert exp.endswith(b"chr2\t-\t9\t10\n") == (m == 1)                       # the last line is kept where the cluster is
    whole, out = check(data, m)
    lines = data.split(b"\n")[:-1]
    with sctext.SctContext() as ctx:
        per_line, out1 = check(data, m, ctx=ctx, pieces=[(l + b"\n", k == len(lines) - 1) for k, l in enumerate(lines)])
        assert ctx.timing()["n_pieces"] == len(lines)
    cut, out2 = check(data, m, piece=4096)
    open_end, out3 = check(data[:-1], m)
    open_cut, out4 = check(data[:-1], m, piece=4096)
    assert out == out1 == out2 == out3 == out4 == exp
    for other in (per_line, cut, open_end, open_cut):
        assert other == whole
    # no newline anywhere in a non-final piece: nothing is consumed
    with sctext.SctContext() as ctx:
        ctx.begin()
        assert ctx.add(b"0\t0\t0", final=False) == 0 and ctx.add(b"0\t0\t0\n1\t0", final=False) == 6
        assert ctx.cover(0)["n_lines"] == 1 and ctx.fetch() == b"0\t0\t0\n"


@pytest.mark.gpu
def test_gpu_every_open_final_piece_gains_its_newline(built):
    """final = 1 on a piece that other pieces follow: its open last line ends there and gains a newline of its own, so the
    output can be longer than the input by one byte per piece."""
    from defuse_amd import sctext
    pieces = [(b"0\t0\t1\n0\t0\t2", True), (b"1\t0\t3", True), (b"1\t1\t3\tx\n", True), (b"2\t0\t4", True)]
    joined = b"0\t0\t1\n0\t0\t2\n1\t0\t3\n1\t1\t3\tx\n2\t0\t4\n"
    assert expected(joined, 0)[3] == joined
    with sctext.SctContext() as ctx:
        res, out = run_pieces(ctx, pieces, 0)
        assert (res["status"], res["n_lines"], res["n_kept_lines"], res["out_bytes"]) == (so.OK, 5, 5, len(joined)) and out == joined
        assert res["out_bytes"] == sum(len(t) for t, _ in pieces) + 3
        tm = ctx.timing()
        assert (tm["n_pieces"], tm["gather_bytes"]) == (4, len(joined) - 3)
        res, out = run_pieces(ctx, pieces, 2)                                          # only cluster 0 holds two fragments
        assert out == b"0\t0\t1\n0\t0\t2\n"


@pytest.mark.gpu
def test_gpu_empty_text_and_one_open_line(built):
    res, out = check(b"", 0)
    assert (res["status"], res["n_lines"], out) == (so.OK, 0, b"")
    for m, exp in ((0, b"0\t0\t0\n"), (1, b"0\t0\t0\n"), (2, b"")):
        res, out = check(b"0\t0\t0", m)
        assert (res["n_lines"], res["n_clusters"], res["max_element"], out) == (1, 1, 0, exp)


def test_line_shape_cases_are_what_they_claim():
    """Preconditions of test_gpu_line_shapes, on the oracle alone."""
    for name, (data, m) in LINE_SHAPES.items():
        status, _, _, out = expected(data, m)
        assert status == so.OK, name
        lines, kept = so.lines_of(data), so.lines_of(out)
        if name == "three_fields":
            assert all(l.count(b"\t") == 2 for l in lines) and 0 < len(kept) < len(lines)
        elif name == "long_lines":
            assert sorted(len(l) for l in kept)[-2:] == [5000 + 8, 70000 + 8] and max(len(l) for l in lines) == 70000 + 8
        elif name == "six_byte_lines":
            assert len(lines) == 200 and all(len(l) == 5 for l in lines) and 0 < len(kept) < 200
        elif name == "alternating":
            flags = [l in set(kept) for l in lines]
            assert flags[:300] == [True, False] * 150 and len(kept) == 151
        elif name == "all_kept":
            assert out == data and len(lines) > 300
        elif name == "none_kept":
            assert out == b"" and len(lines) > 300


def _line_shapes():
    rng = np.random.default_rng(21)
    three = ["%d\t%d\t%d" % (c, e, f) for c in range(30) for e in (0, 1) for f in rng.integers(0, 40, size=5)]
    long_lines = ["0\t0\t1\t1\tx", "0\t1\t1\t1\t" + "a" * 5000, "1\t0\t2\t1\ty", "1\t1\t2\t1\t" + "b" * 70000, "1\t1\t1\t1\t" + "c" * 300, "0\t0\t3\t1\tz"]
    six = ["%d\t%d\t%d" % (k % 7, (k // 7) % 2, k % 10) for k in range(200)]
    alternating = [l for k in range(150) for l in ("0\t0\t%d\t1\tkept" % k, "1\t1\t%d\t1\tdropped" % k)] + ["1\t0\t5000\t1\tkept"]
    disjoint = ["%d\t%d\t%d\t1\tchr1" % (c, e, 10 * c + k) for c in range(40) for e in (0, 1) for k in range(6)]
    return {"three_fields": (text_of(three), 2), "long_lines": (text_of(long_lines), 1), "six_byte_lines": (text_of(six), 2),
            "alternating": (text_of(alternating), 1), "all_kept": (text_of(disjoint), 6), "none_kept": (text_of(disjoint), 7)}


LINE_SHAPES = _line_shapes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LINE_SHAPES))
def test_gpu_line_shapes(built, name):
    data, m = LINE_SHAPES[name]
    check(data, m)
    check(data, m, piece=4096)
    check(data[:-1], m)


BASE = ["0\t0\t5\t1\ta", "0\t0\t6\t1\tb", "1\t0\t7\t1\tc", "1\t1\t7\t1\td", "0\t1\t5\t1\te"]


@pytest.mark.gpu
def test_gpu_integers_accepted(built):
    """+5, -0, 007 and 2147483647 are integers; a clusterEnd of 2, -1 or 2147483647 is skipped by the read pass, and the filter
    keeps the line when cluster and fragment match."""
    lines = BASE + ["+1\t0\t007\t1\tf", "-0\t0\t+6\t1\tg", "001\t1\t7\t1\th", "0\t2\t5\t1\ti", "0\t-1\t6\t1\tj", "1\t2147483647\t7\t1\tk",
                    "1\t+0\t8\t1\tl", "0\t-0\t9\t1\tm"]
    data = text_of(lines)
    res, out = check(data, 0)
    assert res["status"] == so.OK and out == data and res["n_members"] == 7                # every line is kept, the end-2 and end--1 ones too
    check(data, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("bad,kind", [
    ("1\t0\t2147483648\t1\tx", 3), ("2147483648\t1\t7", 3), ("-2147483649\t1\t7", 3), (" 5\t0\t7\t1\tx", 3), ("5 \t0\t7\t1\tx", 3), ("1\t\t7", 3), ("\t\t", 3),
    ("1\t0\t", 3), ("1\t0\t12\r", 3), ("1\t0\t+\t1", 3), ("1\t0x0\t7", 3), ("x", 2), ("x\t0", 2), ("\t", 2), ("1\t0", 2), ("-1\t0\t7\t1\tx", 4)])
def test_gpu_bad_lines(built, bad, kind):
    lines = BASE * 30
    lines.insert(77, bad)
    for newline_at_end in (True, False):
        res, _ = check(text_of(lines, newline_at_end), 0)
        assert (res["status"], res["stop_kind"], res["stop_line"]) == (so.READ_STOP, kind, 78)
    res, _ = check(text_of(BASE + [bad], False), 0)                                    # as the last line, without a newline
    assert (res["status"], res["stop_kind"], res["stop_line"]) == (so.READ_STOP, kind, len(BASE) + 1)


@pytest.mark.gpu
def test_gpu_empty_line_kinds(built):
    for data, line in ((b"\n", 1), (b"0\t0\t5\n\n", 2), (b"0\t0\t5\n\n0\t0\t6", 2), (b"\n0\t0\t5\n", 1)):
        res, _ = check(data, 0)
        assert (res["status"], res["stop_kind"], res["stop_line"], res["stop_len"]) == (so.READ_STOP, so.EMPTY_LINE, line, 0)


@pytest.mark.gpu
def test_gpu_ranges(built):
    """Fragments and cluster ids outside the tables on end-1 lines are never looked up and never kept; duplicate fragments
    inside a cluster keep every one of their lines; cluster ids have gaps."""
    lines = ["2\t0\t5\t1\ta", "2\t0\t5\t1\tdup", "2\t0\t9\t1\tb", "7\t0\t3\t1\tc", "7\t0\t3\t1\tdup", "7\t0\t3\t1\tdup2",
             "2\t1\t10\t1\tpast", "2\t1\t2147483647\t1\tpast", "2\t1\t-2147483648\t1\tpast", "7\t1\t-1\t1\tpast",
             "8\t1\t3\t1\tbeyond", "2147483647\t1\t3\t1\tbeyond", "500\t1\t5\t1\tbeyond", "4\t1\t5\t1\tgap", "0\t1\t3\t1\tgap",
             "2\t1\t5\t1\tkept", "7\t1\t3\t1\tkept"]
    data = text_of(lines)
    res, out = check(data, 0)
    assert (res["n_clusters"], res["max_element"], res["n_members"]) == (8, 9, 6)
    assert out == text_of(lines[:6] + lines[-2:])
    res, out = check(data, 2)                                                          # cluster 7 owns one fragment, however many lines name it
    assert out == text_of(lines[:3] + lines[-2:-1])


STOP_BASE = list(ts.GOOD_LINES)


def with_lines(*inserts):
    """GOOD_LINES with (1-based line number, text) inserted, the lowest first."""
    lines = list(STOP_BASE)
    for n, text in sorted(inserts):
        lines.insert(n - 1, text)
    return text_of(lines)


@pytest.mark.gpu
def test_gpu_stop_order(built):
    write_stop, negative, read_stop = WRITER_BAD_LINE, "5\t0\t-7\t1\tchr1", "7\t0"
    res, _ = check(with_lines((10, write_stop), (300, read_stop)), 3)
    assert (res["status"], res["stop_kind"], res["stop_line"]) == (so.READ_STOP, so.FEW_FIELDS, 300)
    res, _ = check(with_lines((10, negative), (300, read_stop)), 3)
    assert (res["status"], res["stop_kind"], res["stop_line"]) == (so.READ_STOP, so.FEW_FIELDS, 300)
    res, out = check(with_lines((10, negative), (300, write_stop)), 3)
    assert (res["status"], res["stop_kind"], res["stop_line"], out) == (so.NEGATIVE_ELEMENT, 0, 0, b"")
    res, out = check(with_lines((10, write_stop), (300, negative)), 3)
    assert res["status"] == so.NEGATIVE_ELEMENT
    data = with_lines((101, write_stop), (200, write_stop))
    res, out = check(data, 3)
    assert (res["status"], res["stop_kind"], res["stop_line"]) == (so.WRITE_STOP, so.BAD_CLUSTER_ID, 101)
    assert out == text_of(STOP_BASE[:100]) and res["n_lines"] == len(STOP_BASE) + 2     # every line in front is of a kept cluster
    check(data, 3, piece=4096)
    check(data, 7)                                                                     # a write stop with nothing kept in front


@pytest.mark.gpu
def test_gpu_limits_and_reuse(built):
    """len = 2^31 is DSA_E_LIMIT before anything is read; a ctx serves file after file, after a stop too."""
    from defuse_amd import sctext
    small = np.zeros(16, dtype=np.uint8)
    with sctext.SctContext() as ctx:
        ctx.begin()
        consumed = ctypes.c_int64(-1)
        rc = ctx._lib.sct_add(ctx.handle, small.ctypes.data, 2 ** 31, 1, ctypes.byref(consumed))
        assert (rc, consumed.value) == (sctext.DSA_E_LIMIT, 0) and b"2^31 - 1" in ctx._lib.sct_last_error()
        with pytest.raises(sctext.SctError) as e:
            ctx.add(b"0\t0\t0\n", final=2)
        assert e.value.code == sctext.DSA_E_ARG
        good, stopped = well_formed(1, 0), with_lines((300, "7\t0"))
        first, out = check(good, 3, ctx=ctx)
        assert check(stopped, 3, ctx=ctx)[0]["status"] == so.READ_STOP
        with pytest.raises(sctext.SctError) as e:                                     # a stop has no output to fetch from
            ctx.fetch(0, 1)
        assert e.value.code == sctext.DSA_E_ARG
        assert check(good, 3, ctx=ctx) == (first, out)
        assert check(good, 0, ctx=ctx)[0]["n_kept_lines"] > first["n_kept_lines"]
        assert ctx.fetch(5, 11) == expected(good, 0)[3][5:16]                           # a range of the output
        # sct_cover again on the same pieces, with another minimum
        assert ctx.cover(3) == first and ctx.fetch() == out


# ---- GPU: the tool with DEFUSE_SC_DEVICE_TEXT=1 against its default path ------------------------------------------------------

def run_tool(path, outp, device_text, m=3, timing=False):
    env = dict(os.environ)
    env.pop("DEFUSE_SC_DEVICE_TEXT", None)
    env.pop("DEFUSE_TIMING", None)
    if device_text:
        env["DEFUSE_SC_DEVICE_TEXT"] = "1"
    if timing:
        env["DEFUSE_TIMING"] = "1"
    r = subprocess.run([TOOL, "-c", str(path), "-m", str(m), "-o", str(outp)], capture_output=True, text=True, env=env, timeout=300)
    return r.returncode, r.stdout, r.stderr


def took_the_device_path(path, outp, expect):
    """The device-text run again with DEFUSE_TIMING=1: the stage lines on stderr say which path ran (the library's "pieces"
    line, and no "lines parsed" of the host reader), and everything else is `expect` = (exit code, stdout, stderr)."""
    code, stdout, stderr = run_tool(path, outp, True, timing=True)
    stages = [l for l in stderr.splitlines(True) if l.startswith("[setcover]")]
    assert any(l.startswith("[setcover] pieces ") and " parse " in l and " gather " in l for l in stages), stderr
    assert any(l.startswith("[setcover]   pieces on the device ") for l in stages), stderr
    assert not any("lines parsed" in l or "lines filtered" in l or "clusters laid out" in l for l in stages), stderr
    assert (code, stdout, "".join(l for l in stderr.splitlines(True) if not l.startswith("[setcover]"))) == expect


@pytest.mark.gpu
def test_tool_device_text_matches_the_default_path_and_the_oracle(built, tmp_path):
    from defuse_amd import build
    from oracle import setcover_oracle as o
    build.build_tools()
    p = tmp_path / "clusters.txt"
    ts.write_cluster_file(p, ts.random_clusters(7, n_clusters=500, n_frag=1500, big=1))       # the file of test_setcover_tool_matches_oracle
    outs = []
    for device_text in (False, True):
        outp = tmp_path / ("clusters.%d.sc" % device_text)
        assert run_tool(p, outp, device_text) == (0, "Reading clusters\nCalculating set cover solution\nWriting out clusters\n", "")
        outs.append(outp.read_text())
    exp = o.setcover(str(p), 3)
    assert outs[0] == outs[1] == exp and len(exp.splitlines()) > 100
    # the switch switches: the default path's stage lines name the host reader, the device-text path's the library
    code, _, stderr = run_tool(p, tmp_path / "clusters.timed.sc", False, timing=True)
    assert code == 0 and "[setcover]   lines parsed " in stderr and "[setcover] pieces " not in stderr
    took_the_device_path(p, tmp_path / "clusters.timed.sc", (0, "Reading clusters\nCalculating set cover solution\nWriting out clusters\n", ""))
    assert (tmp_path / "clusters.timed.sc").read_text() == exp


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [c[0] for c in BAD_LINE_CASES] + [WRITER_BAD_LINE, "5\t0\t-7\t1\tchr1"])
def test_tool_device_text_reports_as_the_default_path_does(built, tmp_path, bad):
    """The six bad-line cases, the writer's negative id (which names the output file) and a negative element: stdout, stderr
    and exit code of the two paths are the same bytes, and the device-text run is shown to be one."""
    from defuse_amd import build
    build.build_tools()
    p, outp = tmp_path / "clusters.txt", tmp_path / "out.sc"
    p.write_bytes(bad_line_file(bad, later_bad_line=bad in [c[0] for c in BAD_LINE_CASES]))
    default = run_tool(p, outp, False)
    device = run_tool(p, outp, True)
    assert default[0] == 1 and default[2] != ""
    assert device == default
    took_the_device_path(p, outp, default)
