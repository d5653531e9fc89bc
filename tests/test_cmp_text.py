"""include/defuse_cmp.h, section "alignment and cluster text" (defuse_amd/csrc/cmpt_api.hip through defuse_amd/cmptext.py):
clustermatepairs' alignment file parsed and its cluster file printed on the GPU, against tests/cmptext_oracle.py byte for
byte; the oracle itself against oracle/clustermatepairs_oracle.py; and the tool's DEFUSE_CMP_DEVICE_TEXT=1 path against its
default path."""
import ctypes
import functools

import numpy as np
import pytest

from tests import abi, cmp_cases, cmptext_oracle as co
from tests import cmp_problem_cases as pc

MFR = int(300 + 10 * 30)                # the tool's minFusionRange with -u 300 -s 30
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def text_of(lines, newline_at_end=True):
    return (b"\n".join(lines) + (b"\n" if newline_at_end else b""))


def line(frag=b"7", end=b"1", name=b"chr1", strand=b"+", start=b"100", stop=b"149", more=()):
    return b"\t".join((frag, end, name, strand, start, stop) + tuple(more))


@functools.lru_cache(maxsize=None)
def generated(which):
    lines = cmp_cases.two_loci() if which == "two_loci" else cmp_cases.many_loci(int(which))
    return "".join(lines).encode()


def small_text():
    """400 bytes: fragments of one to three lines, four names (one empty), both strands and read ends, extra fields."""
    rng = np.random.default_rng(11)
    names = [b"chr1", b"chr10", b"", b"chrX"]
    lines, frag = [], 0
    while len(text_of(lines)) < 300:
        for _ in range(int(rng.integers(1, 4))):
            lines.append(line(b"%d" % frag, b"12"[int(rng.integers(0, 2)):][:1], names[len(lines) % 4], b"+-"[int(rng.integers(0, 2)):][:1],
                              b"%d" % rng.integers(0, 5000), b"%d" % rng.integers(0, 5000), (b"x",) if rng.random() < 0.2 else ()))
        frag += int(rng.integers(1, 3))
    # one more line, its name as long as it takes: the text has exactly 400 bytes
    return text_of(lines + [line(b"%d" % frag, b"1", b"c" * (400 - len(text_of(lines)) - len(b"%d" % frag) - 10), b"+", b"1", b"2")])


# ---- no GPU: the binding, the argument checks, and the oracle pinned to behaviour that is tested already ----------------------

def test_header_and_binding(built):
    from defuse_amd import cmptext
    sizes, n_functions = abi.check("defuse_cmp.h", cmptext, r"cmpt_[a-z_]+", constants=cmptext.CONSTANTS)
    assert n_functions == len(cmptext.EXPORTS) == len(cmptext.PROTOTYPES) == 16
    assert sizes == [ctypes.sizeof(s) for s in cmptext.STRUCTS.values()] == [72, 72, 24, 56]
    e = cmptext.CmptError(-4, "z")
    assert str(e) == "cmpt error -4: z" and e.code == -4
    assert (co.EMPTY_LINE, co.FORMAT, co.BAD_FRAGMENT, co.BAD_POSITION) == (cmptext.EMPTY_LINE, cmptext.FORMAT, cmptext.BAD_FRAGMENT, cmptext.BAD_POSITION)


def test_arguments_are_checked_before_a_device_is_touched(built):
    """What can be told from the arguments alone, with no context at all (so no GPU either)."""
    from defuse_amd import cmptext
    lib = cmptext.lib()
    h, res, pr, n = ctypes.c_void_p(), cmptext.CmptResult(), cmptext.CmptPrintResult(), ctypes.c_int64(5)
    buf = np.zeros(16, dtype=np.uint8)
    assert lib.cmpt_create(0, 16, None) == cmptext.DSA_E_ARG
    for bad in (0, -1, (1 << 28) + 1):
        assert lib.cmpt_create(0, bad, ctypes.byref(h)) == cmptext.DSA_E_ARG and not h and b"max_names" in lib.cmpt_last_error()
    for fn in (lib.cmpt_add, lib.cmpt_add_device):
        assert fn(None, buf.ctypes.data, 16, 1, None) == cmptext.DSA_E_ARG
        assert fn(None, buf.ctypes.data, -1, 1, ctypes.byref(res)) == cmptext.DSA_E_ARG
        assert fn(None, buf.ctypes.data, 1 << 31, 1, ctypes.byref(res)) == cmptext.DSA_E_LIMIT and b"pieces" in lib.cmpt_last_error()
        assert fn(None, None, 16, 1, ctypes.byref(res)) == cmptext.DSA_E_ARG
        assert fn(None, buf.ctypes.data, 16, 2, ctypes.byref(res)) == cmptext.DSA_E_ARG
        assert fn(None, buf.ctypes.data, 16, 1, ctypes.byref(res)) == cmptext.DSA_E_ARG and b"no ctx" in lib.cmpt_last_error()
    for fn in (lib.cmpt_print_rows, lib.cmpt_print_rows_device):
        assert fn(None, buf.ctypes.data, 1, None) == cmptext.DSA_E_ARG
        assert fn(None, buf.ctypes.data, -1, ctypes.byref(pr)) == cmptext.DSA_E_ARG and pr.bad_row == -1
        assert fn(None, None, 1, ctypes.byref(pr)) == cmptext.DSA_E_ARG
        assert fn(None, buf.ctypes.data, 1 << 30, ctypes.byref(pr)) == cmptext.DSA_E_LIMIT
        assert fn(None, buf.ctypes.data, 1, ctypes.byref(pr)) == cmptext.DSA_E_ARG
    assert lib.cmpt_text_fetch(None, buf.ctypes.data, 16, None) == cmptext.DSA_E_ARG
    assert lib.cmpt_text_fetch(None, buf.ctypes.data, -1, ctypes.byref(n)) == cmptext.DSA_E_ARG and n.value == 0
    assert lib.cmpt_text_fetch(None, buf.ctypes.data, 16, ctypes.byref(n)) == cmptext.DSA_E_ARG
    assert lib.cmpt_begin(None) == lib.cmpt_view(None, None) == lib.cmpt_fetch(None, None, 0, None, 0) == cmptext.DSA_E_ARG
    assert lib.cmpt_names_fetch(None, None, 0, None, 0) == lib.cmpt_get_timing(None, None) == cmptext.DSA_E_ARG
    assert lib.cmpt_bin_upload_records_device(None, None, 0, 0) == lib.cmpt_bin_upload_fragments_device(None, None, 0, 0) == cmptext.DSA_E_ARG
    assert lib.cmpt_problems_rows_view(None, None, None) == cmptext.DSA_E_ARG
    lib.cmpt_destroy(None)


@pytest.mark.parametrize("which", ["two_loci", "3", "6"])
def test_oracle_equals_the_clustermatepairs_oracle(which):
    """Records, names and fragments are what read_fragments and the name loop of oracle/clustermatepairs_oracle.py give, and the
    printed lines are those of its output."""
    from oracle import clustermatepairs_oracle as o
    data = generated(which)
    lines = data.decode().splitlines(True)
    names, index, recs, starts = [], {}, [], []
    for raws in o.read_fragments(lines):
        starts.append(len(recs))
        for r in raws:
            if r["reference"] not in index:
                index[r["reference"]] = len(names)
                names.append(r["reference"])
            recs.append((int(r["fragment"]), r["region"][0], r["region"][1], index[r["reference"]] | (r["strand"] << 28) | (r["readEnd"] << 29)))
    s, res = co.parse(data)
    assert res["stop_line"] == 0 and res["n_lines"] == len(lines) and len(recs) >= 40
    assert (s.records, s.frag_start, [n.decode() for n in s.names]) == (recs, starts + [len(recs)], names)
    out, n_clusters = o.clustermatepairs(lines, 300, 30, 0.95, 5, em="c")
    rows = []
    for a, b in zip(*[iter(out.splitlines())] * 2):
        a, b = a.split("\t"), b.split("\t")
        assert (a[0], a[1], b[1]) == (b[0], "0", "1")
        rows.append({"cluster_id": int(a[0]), "fragment": (int(a[2]), int(b[2])), "read_end": (int(a[3]), int(b[3])), "ref": (index[a[4]], index[b[4]]),
                     "strand": ("+-".index(a[5]), "+-".index(b[5])), "start": (int(a[6]), int(b[6])), "end": (int(a[7]), int(b[7]))})
    assert n_clusters >= 2 and co.print_rows(rows, s.names) == (out.encode(), None)


def test_oracle_rules():
    ok = line()
    assert [co.parse_line(l)[0] for l in (b"", b"7\t1\tchr1\t+\t1", line(b"x"), line(b""), line(start=b"1 "), line(stop=b"2147483648"), ok, ok + b"\r")] == \
        [co.EMPTY_LINE, co.FORMAT, co.BAD_FRAGMENT, co.BAD_FRAGMENT, co.BAD_POSITION, co.BAD_POSITION, 0, co.BAD_POSITION]
    s, res = co.parse(text_of([line(b"7"), line(b"07", b"2", b"", b"-"), line(b"+7", b"11", b"chr1\r", b"--"), line(b"+7", more=(b"", b"z"))], False))
    assert s.records == [(7, 100, 149, co.meta(0, 0, 0)), (7, 100, 149, co.meta(1, 1, 1)), (7, 100, 149, co.meta(2, 0, 1)), (7, 100, 149, co.meta(0, 0, 0))]
    assert s.frag_start == [0, 1, 2, 4] and s.names == [b"chr1", b"", b"chr1\r"] and res["n_lines"] == 4
    # pieces: an open last line waits for its rest; a stop ends the stream and later pieces are passed over
    data = text_of([line(b"1"), line(b"1", name=b"b"), b"", line(b"2", name=b"c")])
    whole = co.parse(data)
    assert whole[1]["stop_line"] == 3 and whole[1]["stop_kind"] == co.EMPTY_LINE and whole[1]["stop_offset"] == data.index(b"\n\n") + 1
    assert whole[0].names == [b"chr1", b"b"] and whole[0].frag_start == [0, 2]
    for k in range(len(data) + 1):
        s, res = co.parse(data, cuts=(k,))
        assert (s.records, s.frag_start, s.names) == (whole[0].records, whole[0].frag_start, whole[0].names)
        assert {f: res[f] for f in res if f != "consumed"} == {f: whole[1][f] for f in res if f != "consumed"}


# ---- GPU: the library against the oracle, byte for byte ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def cmptext(built):
    from defuse_amd import cmptext as module
    return module


@pytest.fixture(scope="module")
def ctx(cmptext):
    with cmptext.CmptContext(max_names=64) as c:
        yield c


def same_stream(cmptext, ctx, want, res, want_res):
    from defuse_amd import cmp
    assert res == want_res
    recs, starts = ctx.fetch()
    assert recs.tobytes() == np.array(want.records, dtype=cmp.RECORD_DTYPE).reshape(len(want.records)).tobytes()
    assert starts.tolist() == want.frag_start
    assert ctx.names() == want.names
    v = ctx.view()
    assert (v.n_records, v.n_fragments, v.n_names, v.n_name_bytes) == (len(want.records), len(want.starts), len(want.names), sum(map(len, want.names)))


def check(cmptext, ctx, data, cuts=()):
    """One stream of `data`, in one piece or cut at `cuts`, against the oracle: every field of the result, the records, the
    fragment starts and the names."""
    want, want_res = co.parse(data, cuts)
    res = cmptext.parse_pieces(ctx, data, cuts)
    same_stream(cmptext, ctx, want, res, want_res)
    return want, res


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["two_loci", "3", "6"])
def test_generated_files(cmptext, ctx, which):
    data = generated(which)
    want, res = check(cmptext, ctx, data)
    assert res["stop_line"] == 0 and res["n_records"] >= 40 and res["n_names"] >= 2
    cuts = (len(data) // 3, len(data) // 3 + 1, 2 * len(data) // 3)
    check(cmptext, ctx, data, cuts)
    t = ctx.timing()               # (a piece that holds no whole line does not go up)
    assert t["n_pieces"] == 1 + sum(1 for a, b in zip((0,) + cuts, cuts) if b"\n" in data[a:b]) >= 3 and t["text_bytes"] == len(data) and all(t[k] > 0 for k in ("upload_ms", "tables_ms", "lines_ms", "names_ms", "layout_ms"))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["closed", "open_last_line", "prefix"])
def test_piece_cuts_at_every_byte(cmptext, ctx, form):
    """One 400-byte text cut in two at every offset: final = 0 then final = 1 on the text as it is and on the text without its
    last newline (an open last line with final = 1) give what the single call gives; and every prefix, given whole with
    final = 1, is the oracle's stream of that prefix (an open, often malformed, last line)."""
    data = small_text()
    assert len(data) == 400 and data.endswith(b"\n")
    if form == "prefix":
        kinds = set()
        for k in range(len(data) + 1):
            kinds.add(check(cmptext, ctx, data[:k])[1]["stop_kind"])
        assert kinds == {0, co.FORMAT, co.BAD_POSITION}
        return
    if form == "open_last_line":
        data = data[:-1]
    whole, whole_res = co.parse(data)
    assert whole_res["stop_line"] == 0 and len(whole.names) == 5 and b"" in whole.names and len(whole.starts) < len(whole.records)
    for k in range(len(data) + 1):
        res = cmptext.parse_pieces(ctx, data, (k,))
        same_stream(cmptext, ctx, whole, dict(res, consumed=0), dict(whole_res, consumed=0))
        assert res["consumed"] == len(data) - (data.rfind(b"\n", 0, k) + 1)


@pytest.mark.gpu
def test_text_in_device_memory(cmptext, ctx):
    """cmpt_add_device: unpadded text at an odd address, whole and in pieces; with final = 0 an open last line stays."""
    from tests.test_batch_assembly import DeviceArray
    data = small_text()[:-1]
    want, want_res = co.parse(data)
    with DeviceArray(np.frombuffer(b"#" + data + b"\t7\n7", dtype=np.uint8)) as d:
        ctx.begin()
        same_stream(cmptext, ctx, want, ctx.add_device(d.ptr + 1, len(data)), want_res)
        for k in (0, 1, 57, 200, 399):
            ctx.begin()
            used = ctx.add_device(d.ptr + 1, k, final=False)["consumed"]
            assert used == data.rfind(b"\n", 0, k) + 1
            res = ctx.add_device(d.ptr + 1 + used, len(data) - used)
            same_stream(cmptext, ctx, want, dict(res, consumed=0), dict(want_res, consumed=0))


@pytest.mark.gpu
def test_line_placement(cmptext, ctx):
    """Lines of 11 bytes, so that several end inside one 16-byte chunk and a workgroup span holds hundreds; and a line longer
    than a 4096-byte span, by its name, by its fragment field and by its ignored fields."""
    short = [line(b"%d" % (k % 10), b"1", b"", b"+-"[k % 2:][:1], b"%d" % (k % 7), b"%d" % (k % 9)) for k in range(1500)]
    assert all(len(l) == 10 for l in short)
    want, _ = check(cmptext, ctx, text_of(short))
    assert len(want.starts) == 1500 and want.names == [b""]
    long_name, long_frag = b"n" * 5000, b"0" * 4200 + b"12"
    lines = [line(b"1"), line(b"1", name=long_name), line(long_frag), line(long_frag, name=long_name, more=(b"x" * 9000,)), line(b"12")]
    want, res = check(cmptext, ctx, text_of(lines, False))
    assert want.names == [b"chr1", long_name] and want.frag_start == [0, 2, 4, 5] and res["n_records"] == 5
    check(cmptext, ctx, text_of(lines), cuts=(4096, 8192, 12000))


@pytest.mark.gpu
def test_fragments_are_compared_as_text(cmptext, ctx):
    runs = [b"7", b"7", b"07", b"07", b"+7", b"7", b"-0", b"0", b"+0", b"+0"]
    lines = [line(f) for f in runs]
    data = text_of(lines)
    want, _ = check(cmptext, ctx, data)
    assert want.frag_start == [0, 2, 4, 5, 6, 7, 8, 10] and {r[0] for r in want.records} == {7, 0}
    # a fragment that continues across a piece boundary (cut after line 1, 3, 9), and one that ends exactly there (2, 4, 5)
    ends = np.cumsum([len(l) + 1 for l in lines]).tolist()
    for k in (1, 3, 9, 2, 4, 5):
        check(cmptext, ctx, data, cuts=(ends[k - 1],))
    check(cmptext, ctx, data, cuts=tuple(ends[:-1]))


@pytest.mark.gpu
def test_names(cmptext, ctx):
    # the empty name, a prefix, and a '\r' that belongs to the name
    names = [b"", b"chr1", b"chr10", b"chr1\r"]
    want, _ = check(cmptext, ctx, text_of([line(b"%d" % k, name=names[k % 4]) for k in (3, 1, 2, 0, 1, 3, 2, 0)]))
    assert want.names == [b"chr1\r", b"chr1", b"chr10", b""]
    # 64 names in a table of 128 slots: probe chains; every name again, in another order
    many = [b"contig_%d" % (k * k) for k in range(64)]
    order = np.random.default_rng(5).permutation(64 * 3) % 64
    want, res = check(cmptext, ctx, text_of([line(b"%d" % k, name=many[j]) for k, j in enumerate(order)]))
    assert res["n_names"] == 64 and sorted(want.names) == sorted(many)
    # thousands of lines with the same two names, which first appear in adjacent lines of one wave
    want, _ = check(cmptext, ctx, text_of([line(b"%d" % (k // 2), name=(b"chrA", b"chrB")[k % 2]) for k in range(6000)]))
    assert want.names == [b"chrA", b"chrB"]
    want, _ = check(cmptext, ctx, text_of([line(b"5", name=(b"chrB", b"chrA")[(k % 64) < 33]) for k in range(6000)]))
    assert want.names == [b"chrA", b"chrB"] and want.frag_start == [0, 6000]
    # names first seen in piece 2 are numbered behind those of piece 1, whatever their lines' order inside it
    p1, p2 = text_of([line(b"1", name=b"b"), line(b"2", name=b"a")]), text_of([line(b"3", name=b"d"), line(b"4", name=b"a"), line(b"5", name=b"c")])
    want, _ = check(cmptext, ctx, p1 + p2, cuts=(len(p1),))
    assert want.names == [b"b", b"a", b"d", b"c"] and [r[3] & 0xFFFFFFF for r in want.records] == [0, 1, 2, 1, 3]
    # a name that first appears in or behind a stop line is absent
    want, res = check(cmptext, ctx, text_of([line(b"1", name=b"a"), line(b"x", name=b"late"), line(b"2", name=b"later")]))
    assert res["stop_line"] == 2 and want.names == [b"a"]


@pytest.mark.gpu
def test_max_names(cmptext):
    four = text_of([line(b"%d" % k, name=b"n%d" % (k % 4)) for k in range(40)])
    with cmptext.CmptContext(max_names=4) as c:
        want, res = check(cmptext, c, four)
        assert res["n_names"] == 4
        for data, cuts in ((four + line(b"9", name=b"n4") + b"\n", ()), (four + line(b"9", name=b"n4") + b"\n", (len(four),)),
                           (text_of([line(name=b"m%d" % k) for k in range(30)]), ())):
            with pytest.raises(cmptext.CmptError) as e:
                cmptext.parse_pieces(c, data, cuts)
            assert e.value.code == cmptext.DSA_E_LIMIT and "max_names" in str(e.value)
            assert co.parse(data, max_names=4)[0].too_many_names
            with pytest.raises(cmptext.CmptError) as e:          # the stream is over ...
                c.add(four)
            assert e.value.code == cmptext.DSA_E_ARG
            check(cmptext, c, four)                               # ... and the context as good as new after cmpt_begin
        # a fifth name behind a stop does not count
        want, res = check(cmptext, c, four + b"\n" + line(name=b"n4") + b"\n")
        assert res["stop_kind"] == co.EMPTY_LINE and res["n_names"] == 4


BAD = {co.EMPTY_LINE: b"", co.FORMAT: b"7\t1\tchr1\t+\t100", co.BAD_FRAGMENT: line(b"7x"), co.BAD_POSITION: line(stop=b"")}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(BAD))
def test_stops(cmptext, ctx, kind):
    good = [line(b"%d" % (k // 2), name=b"chr%d" % (k % 3)) for k in range(300)]
    for at in (0, 150, 299):
        lines = list(good)
        lines[at] = BAD[kind]
        data = text_of(lines)
        want, res = check(cmptext, ctx, data)
        assert (res["stop_kind"], res["stop_line"], res["n_records"], res["n_lines"]) == (kind, at + 1, at, at + 1)
        assert data[res["stop_offset"]:res["stop_offset"] + res["stop_len"]] == BAD[kind]
        # two bad lines: the earlier one wins, whatever its kind and wherever the later one lies
        for other in sorted(BAD):
            for later in {min(at + 1, 299), 299} - {at}:
                lines2 = list(lines)
                lines2[later] = BAD[other]
                assert check(cmptext, ctx, text_of(lines2))[1] == dict(res, consumed=len(text_of(lines2)))
        # in a later piece the line number is that of the whole stream, and pieces behind the stop are passed over
        cuts = tuple(c for c in (len(data) // 4, len(data) // 2, 3 * len(data) // 4))
        assert {f: v for f, v in check(cmptext, ctx, data, cuts)[1].items() if f != "consumed"} == {f: v for f, v in res.items() if f != "consumed"}
    if kind != co.EMPTY_LINE:                                   # the last line open
        check(cmptext, ctx, text_of(good[:7] + [BAD[kind]], False))


@pytest.mark.gpu
def test_integers(cmptext, ctx):
    fine = [b"2147483647", b"-2147483648", b"+2147483647", b"0", b"-0", b"+0", b"007", b"-000000000000000000012", b"+00"]
    bad = [b"2147483648", b"-2147483649", b"+2147483648", b"99999999999999999999", b"", b"+", b"-", b" 1", b"1 ", b"1\r", b"0x1", b"1e3", b"--1", b"1-"]
    want, res = check(cmptext, ctx, text_of([line(v, start=v, stop=v) for v in fine]))
    assert res["stop_line"] == 0 and [r[0] for r in want.records] == [INT_MAX, INT_MIN, INT_MAX, 0, 0, 0, 7, -12, 0] and all(r[0] == r[1] == r[2] for r in want.records)
    for v in bad:
        for k, kind in ((0, co.BAD_FRAGMENT), (4, co.BAD_POSITION), (5, co.BAD_POSITION)):
            f = [b"1", b"1", b"c", b"+", b"2", b"3"]
            f[k] = v
            _, res = check(cmptext, ctx, text_of([line(), b"\t".join(f)], newline_at_end=(v != b"1\r" or k != 5)))
            assert (res["stop_kind"], res["stop_line"]) == (kind, 2), (v, k)


def rows_of(cmp, tuples):
    rows = np.zeros(len(tuples), dtype=cmp.ROW_DTYPE)
    for k, (cid, e0, e1) in enumerate(tuples):
        rows[k]["cluster_id"] = cid
        for f, a, b in zip(("fragment", "read_end", "ref", "strand", "start", "end"), e0, e1):
            rows[k][f] = (a, b)
    return rows


@pytest.mark.gpu
def test_printer(cmptext, ctx):
    from defuse_amd import cmp
    from tests.test_batch_assembly import DeviceArray
    names = [b"chr1", b"", b"a_long_name_" + b"x" * 300, b"chr1\r"]
    check(cmptext, ctx, text_of([line(b"%d" % k, name=n) for k, n in enumerate(names)]))
    extremes = [INT_MIN, INT_MAX, 0, -1, 1, -9, 10, -10, 99, 100, 999999999, 1000000000, -1000000000]
    tuples = [(extremes[k % 13], (extremes[(k + 1) % 13], k % 2, k % 4, k % 2, extremes[(k + 2) % 13], extremes[(k + 3) % 13]),
               (extremes[(k + 4) % 13], (k + 1) % 2, (k + 1) % 4, 7 * (k % 3), extremes[(k + 5) % 13], extremes[(k + 6) % 13])) for k in range(52)]
    rows = rows_of(cmp, tuples)
    want, none = co.print_rows(rows, names)
    assert none is None and b"-2147483648\t0\t2147483647\t" in want and want.count(b"\n") == 104
    assert ctx.print_rows(rows) == want and ctx.printed == {"n_rows": 52, "text_bytes": len(want), "bad_row": -1}
    with DeviceArray(rows) as d:
        assert ctx.print_rows_device(d.ptr, 52) == want
    t = ctx.timing()
    assert t["out_bytes"] == len(want) and t["lengths_ms"] > 0 and t["write_ms"] > 0 and t["download_ms"] > 0
    with pytest.raises(cmptext.CmptError) as e:
        ctx.text(cap=len(want) - 1)
    assert e.value.code == cmptext.DSA_E_CAPACITY and e.value.needed == len(want)
    assert ctx.text(cap=len(want) + 5) == want
    # none, one, a few thousand
    assert ctx.print_rows(rows[:0]) == b"" and ctx.printed["text_bytes"] == 0 and ctx.text() == b""
    assert ctx.print_rows(rows[7:8]) == co.print_rows(rows[7:8], names)[0]
    rng = np.random.default_rng(2)
    big = rows[rng.integers(0, 52, size=5000)]
    big["cluster_id"] = np.arange(5000) // 3
    assert ctx.print_rows(big) == co.print_rows(big, names)[0]
    # a ref outside the dictionary: the lowest such row, and no text
    for bad_ref, end in ((4, 1), (-1, 0), (INT_MAX, 0)):
        broken = big.copy()
        broken["ref"][4000][end] = bad_ref
        broken["ref"][1234][1 - end] = bad_ref
        with pytest.raises(cmptext.CmptError) as e:
            ctx.print_rows(broken)
        assert e.value.code == cmptext.DSA_E_ARG and e.value.bad_row == 1234 == co.print_rows(broken, names)[1]
        assert ctx.text() == b""
    assert ctx.print_rows(rows) == want


def stats_of(st):
    return [getattr(st, f) for f, _ in st._fields_ if f not in ("device_ms", "pad_")]


def run_bins(cmp, binner):
    """cmp_bin_run on what is on the binner's device already"""
    st = cmp.Stats()
    rc = binner._lib.cmp_bin_run(binner.handle, MFR, ctypes.byref(st))
    assert rc == 0, binner._lib.cmp_last_error()
    binner.stats = st
    return stats_of(st), binner.fetch()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["3", "6"])
def test_hand_over_to_the_binner(cmptext, ctx, which):
    """cmp_bin_run after the device hand-over against cmp_bin_run after the host uploads of the restatement's records."""
    from defuse_amd import cmp
    data = generated(which)
    want, _ = check(cmptext, ctx, data, cuts=(len(data) // 2,))
    with cmp.Binner(0) as host, cmp.Binner(0) as dev:
        stats = stats_of(host.run(np.array(want.records, dtype=cmp.RECORD_DTYPE), np.array(want.frag_start, dtype=np.uint32), MFR))
        lists = host.fetch()
        ctx.hand_over(dev)
        stats_d, lists_d = run_bins(cmp, dev)
        assert stats_d == stats and stats[2] > 10 and stats[5] == -1
        for a, b in zip(lists, lists_d):
            assert a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def tools(built):
    from defuse_amd import build
    build.build_tools()
    return True


@pytest.mark.gpu
def test_device_rows_of_a_real_select(cmptext, ctx, tools, tmp_path):
    """Text in, text out, nothing in between on the host: parse, hand-over, bin pairs, problems, EM and select on the device, the
    rows printed where they are — against the host-rows form, the oracle's lines and the file the default tool writes."""
    from defuse_amd import cmp
    from oracle import clustermatepairs_oracle as ora
    data = generated("3")
    path = tmp_path / "spanning.txt"
    path.write_bytes(data)
    r = pc.run_tool(path, tmp_path / "clusters.txt")
    assert r.returncode == 0, r.stderr
    tool_file = (tmp_path / "clusters.txt").read_bytes()
    want, _ = check(cmptext, ctx, data)
    with cmp.Binner(0) as binner, cmp.Problems(0) as problems:
        ctx.hand_over(binner)
        run_bins(cmp, binner)
        c = problems.build(binner, MFR, 5, 300.0)
        off = problems.fetch(["prob_off"])["prob_off"]
        v = problems.view()
        prm = cmp.MpeParams(300.0, 30.0, ora.MatePairEM(300.0, 30.0, 0.95, 5).min_prob, 5, 0)
        ncl, _, status = cmp.cluster_batch(prm, off, None, None, None, None, None, on_device=(v.x, v.y, v.u, v.to_xo, v.to_yo, v.member))
        assert c.n_problems >= 8 and not status.any()
        n_rows = problems.select(0, c.n_problems, ncl, v.member)
        text = ctx.print_problems(problems)
        rows = problems.rows()
        assert ctx.printed["n_rows"] == n_rows == len(rows) > 50
        assert text == ctx.print_rows(rows) == co.print_rows(rows, want.names)[0] == tool_file


# ---- the tool with DEFUSE_CMP_DEVICE_TEXT=1 against the tool without ------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loci3", "config3"])
def test_tool_with_device_text(tools, tmp_path, name):
    """Clusters file, stdout and exit status of both paths, for one and three chunks; the timing lines say which path ran."""
    path = tmp_path / "spanning.txt"
    if name == "config3":
        cmp_cases.config3_write(20000, str(path))
    else:
        path.write_bytes(generated(name[4:]))
    outs = {}
    for chunks in ("1", "3"):
        for dev in ("0", "1"):
            env = {"DEFUSE_CMP_CHUNKS": chunks, "DEFUSE_TIMING": "1"}
            if dev == "1":
                env["DEFUSE_CMP_DEVICE_TEXT"] = "1"
            out = tmp_path / ("clusters.%s.%s" % (chunks, dev))
            r = pc.run_tool(path, out, env=env)
            assert r.returncode == 0, r.stderr
            for mark in ("alignment text on the device", "problems on the device", "cluster text on the device"):
                assert (mark in r.stderr) == (dev == "1"), r.stderr
            assert ("lines per piece" in r.stderr) == (dev == "0"), r.stderr
            outs[(chunks, dev)] = (out.read_bytes(), r.stdout)
    ref = outs[("1", "0")]
    assert len(ref[0]) > 500 and all(v == ref for v in outs.values())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(BAD))
def test_tool_reports_a_bad_line_as_the_default_path_does(tools, tmp_path, kind):
    lines = generated("3").splitlines()
    bad = {co.BAD_POSITION: line(b"5", start=b"12x", more=(b"tail",))}.get(kind, BAD[kind])
    for at, newline in ((0, True), (len(lines) // 2, True), (len(lines) - 1, False)):
        changed = list(lines)
        changed[at] = bad
        path = tmp_path / ("bad.%d.txt" % at)
        path.write_bytes(text_of(changed, newline))
        runs = [pc.run_tool(path, tmp_path / "unused.txt", env={"DEFUSE_CMP_DEVICE_TEXT": dev} if dev else None) for dev in ("", "1")]
        if kind == co.EMPTY_LINE and not newline:               # an empty open last line is no line
            assert runs[0].returncode == 0
        else:
            assert runs[0].returncode == 1 and ("line %d" % (at + 1) in runs[0].stderr or "line: %d" % (at + 1) in runs[0].stderr), runs[0].stderr
        assert (runs[1].returncode, runs[1].stderr, runs[1].stdout) == (runs[0].returncode, runs[0].stderr, runs[0].stdout)


@pytest.mark.gpu
def test_tool_with_device_text_falls_back_where_device_problems_does(tools, tmp_path):
    path = tmp_path / "spanning.txt"
    path.write_bytes(generated("3"))
    r0 = pc.run_tool(path, tmp_path / "a.txt")
    assert r0.returncode == 0, r0.stderr
    r = pc.run_tool(path, tmp_path / "b.txt", env={"DEFUSE_CMP_HOST_BINNING": "1", "DEFUSE_CMP_DEVICE_TEXT": "1", "DEFUSE_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert "DEFUSE_CMP_DEVICE_TEXT: stays on the host path" in r.stderr and "text on the device" not in r.stderr
    assert (tmp_path / "b.txt").read_bytes() == (tmp_path / "a.txt").read_bytes() and r.stdout == r0.stdout
