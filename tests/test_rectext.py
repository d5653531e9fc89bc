"""include/defuse_rec.h, section "alignment text": an alignment file parsed on the GPU straight into a record store
(defuse_amd/csrc/rect_api.hip through defuse_amd/rectext.py), and `defuse_glue sort_alignments`, the sort of the pipeline's
alignment files built from it.

The checker is tests/rectext_oracle.py.  Without a GPU it is pinned three ways: its stops against the messages of the host
evalsplitalign, its sorted text against GNU sort, and its records and results against rect_shared.hpp compiled into a host
program under ASan + UBSan.  On the GPU everything is compared with it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import abi
from tests import rec_case as rc
from tests import rectext_oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLUE = os.path.join(ROOT, "bin", "defuse_glue")
DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = -2, -3, -4
SPAN = 4096                                              # bytes one workgroup of the table kernels covers
C_ENV = dict(os.environ, LC_ALL="C")


def line(*v):
    """The plain line of nine values."""
    return b"%d\t" * 9 % v + b"\n"


def fields(*f):
    """A line of arbitrary field texts, each closed by a tab as a plain line's are."""
    return b"".join(x + b"\t" for x in f) + b"\n"


GOOD = [b"7", b"11", b"0", b"1", b"3", b"-4", b"25", b"25", b"90"]


def with_field(k, text):
    f = list(GOOD)
    f[k] = text
    return fields(*f)


def plain_file(seed, n):
    """n plain lines: rec_case's draw (edge values, negative values, every digit count) with the bool field in 0/1."""
    return b"".join(rc.lines_of(rc.draw(np.random.default_rng(seed), n, flags01=True)))


ACCEPTED = [b"2147483647", b"-2147483648", b"+7", b"007", b"-0"]
REFUSED = [b"2147483648", b"-2147483649", b"12345678901234567890", b"", b"-", b"+", b"1 ", b"1\r", b"1x"]
INT_FIELDS = [0, 1, 2, 4, 8]


def shape_cases():
    """(name, data, final): the line shapes, integers and stop orders every implementation of the rule is run on."""
    good = line(1, 2, 0, 1, 5, 6, 7, 8, 9)
    out = [("empty", b"", 1), ("one", good, 1), ("open_last", good + good[:-1], 1), ("open_last_kept", good + good[:-1], 0),
           ("no_newline", good[:-1], 0), ("no_newline_final", good[:-1], 1), ("empty_line", good + b"\n" + good, 1), ("only_newline", b"\n", 1)]
    for k in INT_FIELDS:
        out.append(("accepted_%d" % k, good + b"".join(with_field(k, t) for t in ACCEPTED) + good, 1))
        out += [("refused_%d_%d" % (k, j), good + with_field(k, t) + good, 1) for j, t in enumerate(REFUSED)]
    out.append(("bool_ok", with_field(3, b"0") + with_field(3, b"1"), 1))
    out += [("bool_%d" % j, good + with_field(3, t) + good, 1) for j, t in enumerate([b"2", b"01", b""])]
    # not plain, but records: a missing last tab, an extra field, a '\r' behind the last tab and inside the last field is a stop
    out.append(("missing_tab", good + good[:-2] + b"\n" + good, 1))
    out.append(("extra_field", good + good[:-1] + b"more\n" + good, 1))
    out.append(("cr_after_tab", good + good[:-1] + b"\r\n" + good, 1))
    out.append(("cr_in_field", good + good[:-2] + b"\r\t\n" + good, 1))
    # stop order
    out.append(("two_bad_lines", good + with_field(8, b"x") + with_field(0, b"y") + good, 1))
    out.append(("two_bad_fields", good + fields(b"1", b"x", b"0", b"2", b"5", b"y", b"7", b"8", b"9"), 1))
    out.append(("bool_before_int", good + fields(b"1", b"2", b"0", b"2", b"x", b"6", b"7", b"8", b"9"), 1))
    out.append(("few_beats_int", good + b"x\t2\t0\t1\t5\t6\t7\t8\n", 1))
    out.append(("bad_first", with_field(1, b"x") + good, 1))
    out.append(("bad_last", good + with_field(1, b"x"), 1))
    out.append(("bad_open_last", good + with_field(1, b"x")[:-1], 1))
    out.append(("bad_open_last_kept", good + with_field(1, b"x")[:-1], 0))
    # the id the reference's look-ahead has read: six fields, seven and eight with a good id, nine with a bad one
    out.append(("id_six", good + b"42\t2\t0\t1\t5\t6\n", 1))
    out.append(("id_seven", good + b"42\t2\t0\t1\t5\t6\t7\n", 1))
    out.append(("id_eight", good + b"-42\t2\t0\t1\t5\t6\t7\t8\n", 1))
    out.append(("id_seven_bad", good + b"4x\t2\t0\t1\t5\t6\t7\n", 1))
    out.append(("id_nine_bad", good + with_field(0, b"4x"), 1))
    out.append(("id_nine_good", good + with_field(5, b"4x"), 1))
    return out


# ---------------------------------------------------------------------------------------------- CPU
def test_header_and_binding_agree(built):
    from defuse_amd import rec, rectext
    sizes, n = abi.check("defuse_rec.h", rectext, r"rect_[a-z_]+", constants=rectext.CONSTANTS)
    assert sizes == [64, 32] and n == 5
    assert abi.check_functions("defuse_rec.h", rec, r"rec_[a-z_]+") == 14        # the store's own functions are untouched
    assert (ora.FEW_FIELDS, ora.BAD_INTEGER, ora.BAD_BOOL) == (rectext.FEW_FIELDS, rectext.BAD_INTEGER, rectext.BAD_BOOL)


def test_argument_errors_without_a_device(built):
    """What the arguments alone decide is decided before a device or the text is touched: the handles below are not objects
    and the text pointer is not memory."""
    from defuse_amd import rectext
    lib = rectext.lib()
    h = ctypes.c_void_p()
    for d in [999] + ([0] if lib.dsa_device_count() == 0 else []):
        assert lib.rect_create(d, ctypes.byref(h)) == DSA_E_DEVICE and not h.value
        assert lib.rect_last_error().startswith(b"no usable HIP device")
    with pytest.raises(rectext.RectError) as e:
        rectext.RectContext(999)
    assert e.value.code == DSA_E_DEVICE
    assert lib.rect_create(0, None) == DSA_E_ARG
    res = rectext.RectResult()
    fake, text = ctypes.c_void_p(16), ctypes.c_void_p(16)
    assert lib.rect_add(fake, fake, text, 4, 1, None) == DSA_E_ARG
    for args, code in [((fake, fake, text, -1, 1), DSA_E_ARG), ((fake, fake, text, 2 ** 31, 1), DSA_E_LIMIT), ((fake, fake, text, 2 ** 40, 0), DSA_E_LIMIT),
                       ((fake, fake, None, 4, 1), DSA_E_ARG), ((fake, fake, text, 4, 2), DSA_E_ARG), ((None, fake, text, 4, 1), DSA_E_ARG),
                       ((fake, None, text, 4, 1), DSA_E_ARG)]:
        res.consumed = 77
        assert lib.rect_add(*args, ctypes.byref(res)) == code, args
        assert len(lib.rect_last_error()) > 0 and res.consumed == 0 and res.stop_field == -1
    assert lib.rect_get_timing(None, None) == DSA_E_ARG
    lib.rect_destroy(None)                                          # a no-op


@pytest.fixture(scope="module")
def tools(built):
    from defuse_amd import build
    build.build_tools()
    return True


PLANTED = [("eight_fields", b"5\t2\t0\t1\t5\t6\t7\t8\n"), ("empty_line", b"\n"), ("int_0", with_field(0, b"1x")), ("int_1", with_field(1, b"")),
           ("int_8", with_field(8, b"2147483648")), ("bool_2", with_field(3, b"2")), ("bool_01", with_field(3, b"01")), ("bool_empty", with_field(3, b""))]


def test_oracle_stops_where_evalsplitalign_does(tools, tmp_path):
    """The host evalsplitalign (the default path) on a generated alignment file with one bad line planted: it exits 1 and its
    message names the kind and the field text the oracle gives for that line."""
    from tests.eval_case import generated_case
    from tests.test_eval import run_eval
    case, lines = generated_case(tmp_path, 3, n_fusions=12)
    lines = [l.encode() for l in lines]
    assert len(lines) > 10 and ora.parse(b"".join(lines))[0]["stop_line"] == 0 and ora.parse(b"".join(lines))[0]["n_other"] == 0
    at = len(lines) // 2
    for name, bad in PLANTED:
        data = b"".join(lines[:at]) + bad + b"".join(lines[at:])
        res, _ = ora.parse(data)
        assert res["stop_line"] == at + 1 and res["n_records"] == at
        path = tmp_path / (name + ".align")
        path.write_bytes(data)
        r, _ = run_eval(case, str(path), str(tmp_path / name))
        text = bad[:-1].decode()
        if res["stop_kind"] == ora.FEW_FIELDS:
            want = "Error: Format error for candidate reads line:\n" + text
        else:
            word = "boolean" if res["stop_kind"] == ora.BAD_BOOL else "integer"
            want = "Error: bad %s '%s' in candidate reads line: %s" % (word, text.split("\t")[res["stop_field"]], text)
        assert r.returncode == 1 and want in r.stderr, (name, res, r.stderr[-500:])
    kinds = [ora.parse(bad)[0] for _, bad in PLANTED]
    assert [(k["stop_kind"], k["stop_field"]) for k in kinds] == [(1, -1), (1, -1), (2, 0), (2, 1), (2, 8), (3, 3), (3, 3), (3, 3)]


def test_oracle_sorted_text_is_gnu_sort(tmp_path):
    """sorted_text of plain files (negative values, every digit count, a file without a final newline, an empty one) is
    `LC_ALL=C sort -n -k 1` of them, and `sort -m -n -k 1` of the files sorted one by one."""
    files = [plain_file(3, 700), b"", plain_file(4, 300)[:-1], plain_file(5, 1)]
    names = []
    for k, data in enumerate(files):
        names.append(str(tmp_path / ("part%d" % k)))
        open(names[-1], "wb").write(data)
        assert ora.parse(data)[0]["n_other"] == 0 and ora.parse(data)[0]["stop_line"] == 0
    exp = ora.sorted_text(files)
    assert len(exp) == sum(len(f) for f in files) + 1
    assert subprocess.run(["sort", "-n", "-k", "1"] + names, capture_output=True, check=True, env=C_ENV).stdout == exp
    for k, n in enumerate(names):
        subprocess.run(["sort", "-n", "-k", "1", "-o", n + ".sorted", n], check=True, env=C_ENV)
        assert open(n + ".sorted", "rb").read() == ora.sorted_text([files[k]])
    assert subprocess.run(["sort", "-m", "-n", "-k", "1"] + [n + ".sorted" for n in names], capture_output=True, check=True, env=C_ENV).stdout == exp


HOST = r'''
#include "%(root)s/defuse_amd/csrc/rect_shared.hpp"
#include "%(root)s/tools_src/defuse_host.hpp"
// argv[1]: a piece of alignment text, argv[2]: final.  Prints the rect_result a rect_add of it gives, then the records.  The
// text sits in a buffer of exactly its size, so that a read beyond it is a report; plain-ness is checked against the printer.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint8_t> held;
    for (int c; (c = fgetc(in)) != EOF;) held.push_back((uint8_t)c);
    fclose(in);
    const int64_t n = (int64_t)held.size();
    uint8_t* text = n ? new uint8_t[held.size()] : nullptr;
    if (n) memcpy(text, held.data(), held.size());
    const bool final = argv[2][0] == '1';
    rect_result res{};
    res.stop_field = -1;
    std::vector<dsa_record> recs;
    int64_t pos = 0;
    while (pos < n) {
        const uint8_t* nl = (const uint8_t*)memchr(text + pos, '\n', (size_t)(n - pos));
        if (!nl && !final) break;
        const int64_t e = nl ? nl - text : n;
        std::vector<int64_t> tabs;
        for (int64_t k = pos; k < e; ++k)
            if (text[k] == '\t') tabs.push_back(k);
        const rect_line L = rect_parse_line(text, pos, e, (int64_t)tabs.size(), [&](int64_t k) { return tabs.at((size_t)k); },
                                            [](const uint8_t* p, int64_t m, int& v) { return m >= 0 && defuse::field_int((const char*)p, (size_t)m, v); });
        if (L.kind) {
            res.stop_line = (int64_t)recs.size() + 1;
            res.stop_kind = L.kind; res.stop_field = L.field; res.stop_id_read = L.id_read; res.stop_id = L.id;
            break;
        }
        char printed[REC_MAX_LINE];
        const int len = rec_write_line(L.rec, printed);
        const bool same = (int64_t)(len - 1) == e - pos && memcmp(printed, text + pos, (size_t)(len - 1)) == 0;
        if (same != (L.plain != 0) || L.rec.pair_idx != 0) return 3;
        recs.push_back(L.rec);
        if (!L.plain) { ++res.n_other; if (!res.first_other) res.first_other = (int64_t)recs.size(); }
        pos = nl ? e + 1 : n;
        res.consumed = pos;
    }
    res.n_lines = res.n_records = (int64_t)recs.size();
    printf("%%lld %%lld %%lld %%lld %%lld %%lld %%d %%d %%d %%d\n", (long long)res.consumed, (long long)res.n_lines, (long long)res.n_records,
           (long long)res.stop_line, (long long)res.n_other, (long long)res.first_other, res.stop_kind, res.stop_field, res.stop_id_read, res.stop_id);
    for (const dsa_record& r : recs) {
        const int32_t* f = reinterpret_cast<const int32_t*>(&r);
        for (int k = 0; k < 10; ++k) printf("%%d%%c", f[k], k == 9 ? '\n' : ' ');
    }
    delete[] text;
    return 0;
}
'''
RESULT_KEYS = ["consumed", "n_lines", "n_records", "stop_line", "n_other", "first_other", "stop_kind", "stop_field", "stop_id_read", "stop_id"]


def test_shared_header_as_a_host_program(tmp_path):
    """rect_shared.hpp compiled by g++ into a stand-alone program under ASan + UBSan, with the host's own field_int: on every
    shape case and on a generated file it gives the oracle's result and records, without a report."""
    from tests.test_sanitizers import BAD, ENV
    src = tmp_path / "rect_host.cpp"
    src.write_text(HOST % {"root": ROOT})
    exe = str(tmp_path / "rect_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, str(src)])
    mixed = plain_file(8, 400)
    cases = shape_cases() + [("generated", mixed, 1), ("generated_cut", mixed[:len(mixed) // 2 + 7], 0)]
    assert len({name for name, _, _ in cases}) == len(cases)
    for name, data, final in cases:
        path = tmp_path / "case.txt"
        path.write_bytes(data)
        r = subprocess.run([exe, str(path), str(final)], capture_output=True, text=True, env=dict(os.environ, **ENV["asan"]), stdin=subprocess.DEVNULL, timeout=120)
        assert not any(b in r.stderr for b in BAD), (name, r.stderr[-3000:])
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        rows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        res, recs = ora.parse(data, bool(final))
        assert dict(zip(RESULT_KEYS, rows[0])) == res, name
        assert rows[1:] == [list(t) for t in recs.tolist()], name


def test_shape_cases_say_what_they_are_named_for():
    """The oracle on the cases the header's rules spell out: which integers are accepted and counted, what stops, and what wins."""
    got = {name: ora.parse(data, bool(final))[0] for name, data, final in shape_cases()}
    for k in INT_FIELDS:
        a = got["accepted_%d" % k]
        assert (a["stop_line"], a["n_records"], a["n_other"], a["first_other"]) == (0, 7, 3, 4)
        for j in range(len(REFUSED)):
            r = got["refused_%d_%d" % (k, j)]
            assert (r["stop_line"], r["stop_kind"], r["stop_field"], r["n_records"]) == (2, ora.BAD_INTEGER, k, 1)
    assert got["bool_ok"]["n_records"] == 2 and got["bool_ok"]["n_other"] == 0
    assert all((got["bool_%d" % j]["stop_kind"], got["bool_%d" % j]["stop_field"]) == (ora.BAD_BOOL, 3) for j in range(3))
    for name in ("missing_tab", "extra_field", "cr_after_tab"):
        assert (got[name]["n_records"], got[name]["n_other"], got[name]["first_other"], got[name]["stop_line"]) == (3, 1, 2, 0), name
    assert (got["cr_in_field"]["stop_kind"], got["cr_in_field"]["stop_field"]) == (ora.BAD_INTEGER, 8)
    assert (got["two_bad_lines"]["stop_line"], got["two_bad_lines"]["stop_field"]) == (2, 8)
    assert got["two_bad_fields"]["stop_kind"] == ora.BAD_INTEGER and got["two_bad_fields"]["stop_field"] == 1
    assert got["bool_before_int"]["stop_kind"] == ora.BAD_BOOL
    assert (got["few_beats_int"]["stop_kind"], got["few_beats_int"]["stop_field"], got["few_beats_int"]["stop_id_read"]) == (ora.FEW_FIELDS, -1, 0)
    assert got["bad_first"]["consumed"] == 0 and got["bad_first"]["stop_line"] == 1
    assert got["bad_last"]["stop_line"] == 2 and got["bad_open_last"]["stop_line"] == 2
    assert got["bad_open_last_kept"]["stop_line"] == 0 and got["bad_open_last_kept"]["n_records"] == 1
    assert (got["open_last"]["n_records"], got["open_last_kept"]["n_records"], got["no_newline"]["consumed"], got["no_newline_final"]["n_records"]) == (2, 1, 0, 1)
    assert got["open_last"]["n_other"] == 0 and got["empty_line"]["stop_kind"] == ora.FEW_FIELDS and got["only_newline"]["stop_line"] == 1
    ids = {n: (got[n]["stop_id_read"], got[n]["stop_id"]) for n in got if n.startswith("id_")}
    assert ids == {"id_six": (0, 0), "id_seven": (1, 42), "id_eight": (1, -42), "id_seven_bad": (0, 0), "id_nine_bad": (0, 0), "id_nine_good": (1, 7)}


def run_tool(args, env=None, name="defuse_glue"):
    exe = [GLUE, "sort_alignments"] if name == "defuse_glue" else [name]
    e = {k: v for k, v in os.environ.items() if k not in ("DEFUSE_SORT_PIECE_BYTES", "DEFUSE_TIMING")}
    e.update(env or {})
    return subprocess.run(exe + args, capture_output=True, env=e, timeout=300, stdin=subprocess.DEVNULL)


def test_tool_without_a_device(tools, tmp_path):
    """A device ordinal no machine has: lines to sort end the run with one Error line and status 1, and OUT is not created;
    empty files need no device and give an empty output; a missing file and a missing argument are status 1 too."""
    no_gpu = {"DEFUSE_GPU": "999"}
    some, empty, out = tmp_path / "some", tmp_path / "empty", tmp_path / "out"
    some.write_bytes(plain_file(2, 5))
    empty.write_bytes(b"")
    r = run_tool(["-o", str(out), str(empty), str(some)], env=no_gpu)
    assert r.returncode == 1 and r.stdout == b"" and not out.exists()
    assert r.stderr.startswith(b"Error: sorting on the GPU failed: ") and len(r.stderr.strip().splitlines()) == 1, r.stderr
    out.write_bytes(b"kept")
    r = run_tool(["-o", str(out), str(some)], env=no_gpu)
    assert r.returncode == 1 and out.read_bytes() == b"kept"
    r = run_tool(["-o", str(out), str(empty), str(empty)], env=no_gpu)
    assert (r.returncode, r.stdout, r.stderr, out.read_bytes()) == (0, b"", b"", b"")
    r = run_tool([str(empty)], env=no_gpu)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    assert run_tool([str(tmp_path / "absent")], env=no_gpu).returncode == 1
    r = run_tool([], env=no_gpu)
    assert r.returncode == 1 and r.stderr.startswith(b"Usage: sort_alignments")
    r = subprocess.run([GLUE], capture_output=True, text=True)
    assert r.returncode == 1 and "sort_alignments" in r.stderr


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev(built):
    """(RectContext, rec.Store) on device 0; both raise without a GPU: no fallback."""
    from defuse_amd import rec, rectext
    ctx, store = rectext.RectContext(0), rec.Store(0)
    yield ctx, store
    store.close()
    ctx.close()


def check(dev, data, final=True, clear=True):
    """One rect_add against the oracle: every field of the result, and the records the store gained."""
    ctx, store = dev
    if clear:
        store.clear()
    before = len(store)
    res, recs = ora.parse(data, final)
    got = ctx.add(store, data, final)
    assert got == res
    assert len(store) == before + res["n_records"]
    assert store.download()[before:].tolist() == recs.tolist()
    t = ctx.timing()
    assert (t["n_lines"], t["n_records"]) == (res["n_lines"], res["n_records"])
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_well_formed_files(dev, n):
    data = plain_file(100 + n, n)
    res = check(dev, data)
    assert (res["n_records"], res["n_other"], res["stop_line"], res["consumed"]) == (n, 0, 0, len(data))
    dev[1].sort()
    assert dev[1].text() == ora.sorted_text([data])


@pytest.mark.gpu
@pytest.mark.parametrize("open_last", [False, True])
def test_pieces(dev, open_last):
    """One file cut after every byte of its first three lines and at 16-byte and 4096-byte boundaries: final = 0 consumes the
    whole lines in front of the cut, the rest with final = 1 completes the same records."""
    ctx, store = dev
    data = plain_file(17, 400)
    data = data[:-1] if open_last else data
    assert len(data) > 3 * SPAN
    whole = check(dev, data)
    assert whole["n_records"] == 400 and whole["consumed"] == len(data)
    records = store.download().tolist()
    three = len(b"".join(data.split(b"\n")[:3])) + 3
    cuts = sorted(set(range(0, three + 1)) | set(range(16, 513, 16)) | {k * SPAN + d for k in (1, 2, 3) for d in (-16, 0, 16)} | {len(data) - 1, len(data)})
    for c in cuts:
        first = check(dev, data[:c], final=False)
        assert first["consumed"] <= c and (first["consumed"] == 0 or data[first["consumed"] - 1:first["consumed"]] == b"\n")
        rest = check(dev, data[first["consumed"]:], final=True, clear=False)
        assert first["n_records"] + rest["n_records"] == 400 and store.download().tolist() == records
    store.clear()
    assert ctx.add(store, data[:20].replace(b"\n", b" "), final=False)["consumed"] == 0 and len(store) == 0
    assert check(dev, b"")["consumed"] == 0


@pytest.mark.gpu
def test_table_edges(dev):
    short = b"0\t" * 9 + b"\n"
    # lines that start at every offset modulo 16
    data = b"".join(line(*[(7 * k + j) % 10 for j in range(9)]) for k in range(32))
    starts = np.cumsum([0] + [len(l) + 1 for l in data.split(b"\n")[:-1]])[:-1]
    assert set((starts % 16).tolist()) == set(range(16))
    assert check(dev, data)["n_other"] == 0
    # a line, and one field of it, across the end of a 4096-byte span
    prefix = short * 215
    straddle = prefix + line(12345678, -2147483648, 0, 1, 2147483647, 6, 7, 8, 9) + short * 3
    assert len(prefix) + 9 < SPAN < len(prefix) + 9 + 11
    assert check(dev, straddle)["n_records"] == 219
    # a run of the shortest lines, more than one span of them
    assert check(dev, short * 2048)["n_records"] == 2048
    # a line whose extra fields cross several spans, between plain lines
    long = short + short[:-1] + b"x\t" * 5000 + b"\n" + short * 300
    res = check(dev, long)
    assert (res["n_records"], res["n_other"], res["first_other"]) == (302, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["lines", "accepted", "refused", "bool", "other", "stop"])
def test_shape_cases(dev, group):
    """The integers, bools, line shapes and stop orders of shape_cases() (what each is, is asserted on the oracle above)."""
    prefix = {"lines": ("empty", "one", "open_", "no_newline", "empty_line", "only_newline"), "accepted": ("accepted_",), "refused": ("refused_",),
              "bool": ("bool_",), "other": ("missing_tab", "extra_field", "cr_"), "stop": ("two_", "few_", "bad_", "id_")}[group]
    cases = [c for c in shape_cases() if c[0].startswith(prefix)]
    assert cases
    for name, data, final in cases:
        check(dev, data, bool(final))


@pytest.mark.gpu
def test_stop_across_spans(dev):
    """Two bad lines in different 4096-byte spans (different workgroups of the line kernel too): the lower one wins, and the
    lines that are not plain are counted in front of it only."""
    short = b"0\t" * 9 + b"\n"
    odd = with_field(0, b"+7")
    data = short * 100 + odd + short * 200 + with_field(8, b"x") + short * 300 + odd + with_field(0, b"y") + short * 10
    assert len(short) * 300 > SPAN
    res = check(dev, data)
    assert (res["stop_line"], res["stop_field"], res["n_records"], res["n_other"], res["first_other"]) == (302, 8, 301, 1, 101)
    res = check(dev, short * 400 + with_field(8, b"x") + short * 300 + odd)
    assert (res["stop_line"], res["n_other"], res["first_other"]) == (401, 0, 0)


@pytest.mark.gpu
def test_the_store(dev):
    """Adding keeps what the store held; a stop grows it by exactly stop_line - 1; one ctx serves a small, a large and a small
    piece in turn."""
    ctx, store = dev
    held = rc.draw(np.random.default_rng(5), 300)
    store.clear()
    store.append(held)
    small, large = plain_file(31, 3), plain_file(32, 20000)
    for data in (small, large, small + with_field(2, b"x") + small, small):
        before = store.download().tolist()
        res = check(dev, data, clear=False)
        assert store.download()[:len(before)].tolist() == before
        assert res["stop_line"] == 0 or len(store) == len(before) + res["stop_line"] - 1
    assert store.download()[:300].tolist() == held.tolist() and len(store) == 300 + 3 + 20000 + 3 + 3


@pytest.mark.gpu
def test_sort_text_helper(built):
    from defuse_amd import rectext
    files = [plain_file(41, 500), b"", plain_file(42, 200)[:-1]]
    assert rectext.sort_text(files) == ora.sorted_text(files)
    with pytest.raises(ValueError):
        rectext.sort_text([files[0], with_field(0, b"007")])


@pytest.mark.gpu
def test_tool(tools, tmp_path):
    """Three chunk files (one empty, one without a final newline, one with negative ids) in 64-byte pieces: -o and stdout give
    GNU sort's bytes; a line that is not plain and a malformed line are declined with status 3 and OUT untouched."""
    rng = np.random.default_rng(9)
    files = [b"", b"".join(rc.lines_of(rc.draw(rng, 150, flags01=True, fusion_ids=[3, 20, 100, 7])))[:-1],
             b"".join(rc.lines_of(rc.draw(rng, 120, flags01=True, fusion_ids=[-5, -50, 3, 0])))]
    names = []
    for k, data in enumerate(files):
        names.append(str(tmp_path / ("chunk%d" % k)))
        open(names[-1], "wb").write(data)
    gnu = subprocess.run(["sort", "-n", "-k", "1"] + names, capture_output=True, check=True, env=C_ENV).stdout
    assert gnu == ora.sorted_text(files)
    small = {"DEFUSE_SORT_PIECE_BYTES": "64"}
    out = tmp_path / "sorted"
    r = run_tool(["-o", str(out)] + names, env=small)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"") and out.read_bytes() == gnu
    r = run_tool(names, env=dict(small, DEFUSE_TIMING="1"))
    assert r.returncode == 0 and r.stdout == gnu and r.stderr.count(b"[sort_alignments]") == 2
    link = tmp_path / "sort_alignments"                                     # the step is also selected by the program's name
    os.symlink(GLUE, link)
    r = run_tool(names, name=str(link))
    assert r.returncode == 0 and r.stdout == gnu
    lines = files[2].split(b"\n")
    for k, bad in enumerate((with_field(0, b"007"), b"5\t2\t0\t1\t5\t6\t7\t8\n", with_field(6, b"1x"))):      # not plain, and malformed twice
        planted = tmp_path / "planted"
        planted.write_bytes(b"\n".join(lines[:23]) + b"\n" + bad + b"\n".join(lines[23:]))
        declined = tmp_path / ("declined%d" % k)
        if k:
            declined.write_bytes(b"as it was")
        r = run_tool(["-o", str(declined), names[1], str(planted)], env=small)
        assert r.returncode == 3 and r.stdout == b"", (k, r.stderr)
        assert declined.read_bytes() == b"as it was" if k else not declined.exists()
        message = r.stderr.decode().strip().splitlines()
        assert len(message) == 1 and "%s line 24:" % planted in message[0] and "LC_ALL=C sort -n -k 1" in message[0], message
    r = run_tool(["-o", str(out), names[0], names[0]])
    assert (r.returncode, out.read_bytes()) == (0, b"")
