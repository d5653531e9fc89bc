"""The improper-mate SAM text and the reads' FASTQ text parsed on the GPU (include/defuse_text.h through defuse_amd/text.py),
and the device-pointer twins cand_enumerate_resident and bat_reads_create_device.

Yardsticks: tests/text_oracle.py, a Python restatement of the two contracts, which test_oracle_equals_the_host_parser pins
to ParseSamLine / FastqReader::next / field_int of tools_src/defuse_host.hpp; for the consumers cand_enumerate and
bat_reads_create on the oracle's arrays; for the chain the same chain fed from host-parsed arrays."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import abi
from tests import pipeline_case
from tests import text_oracle as ora
from tests.test_batch_assembly import DeviceArray, assert_same_batch, from_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
NAMES = [b"chr1", b"chr10", b"chr1_x", b"chr2", b"ENSG01|ENST01"]
SAM_FIELDS = ("consumed", "n_lines", "n_alignments", "stop_line", "n_bad_fragment", "stop_kind", "carry_out")
FASTQ_FIELDS = ("consumed", "n_records", "n_skipped", "stop_line", "stop_kind")


@pytest.fixture(scope="module")
def text(built):
    from defuse_amd import text as t
    return t


@pytest.fixture(scope="module")
def cand(built):
    from defuse_amd import cand as c
    return c


@pytest.fixture(scope="module")
def bat(built):
    from defuse_amd import bat as b
    return b


@pytest.fixture(scope="module")
def names(text):
    with text.Names(NAMES) as n:
        yield n


@pytest.fixture(scope="module")
def ctx(text, names):
    with text.Context(names) as c:
        yield c


# ---------------------------------------------------------------------------------------------- texts
def sam(qname=b"7/1", flag=b"0", rname=b"chr1", pos=b"100", seq=b"ACGTA", n_fields=11):
    f = [qname, flag, rname, pos, b"255", b"5M", b"*", b"0", b"0", seq, b"I" * len(seq), b"NM:i:0", b"XA:Z:a", b"XB:Z:b"]
    return b"\t".join(f[:n_fields])


def random_sam(seed, n_lines, bad=True, max_seq=160):
    """A SAM text of n_lines lines of every kind that is no stop (with bad=True one stopping line near the end)."""
    rng = np.random.default_rng(seed)
    out = [b"@HD\tVN:1.0", b"@SQ\tSN:chr1\tLN:5700"]
    rnames = NAMES + [b"chrUn", b"", b"chr", b"chr100"]
    while len(out) < n_lines:
        k = int(rng.integers(0, 40))
        frag = b"%d" % rng.integers(0, 5000)
        flag = int(rng.choice([0, 16, 64, 80, 128, 144, 4, 1 + 2, 0x40 | 0x80]))
        rname = rnames[int(rng.integers(0, len(rnames)))]
        seq = b"ACGT"[int(rng.integers(0, 4)):][:1] * int(rng.integers(0, max_seq))
        if k == 0:
            out.append(b"@CO\t" + b"x" * int(rng.integers(0, 50)))
        elif k == 1:
            out.append(sam(frag + b"/1", b"4", b"*", b"0", seq))
        elif k <= 8:
            out.append(sam(frag, b"%d" % flag, rname, b"%d" % rng.integers(0, 6000), seq))             # read end by the flag, or carried
        elif k == 9:
            out.append(sam(frag + b"/1/2", b"%d" % flag, rname, b"7", seq))
        elif k == 10:
            out.append(sam(b"r" + frag + b"/2", b"+%d" % flag, rname, b"007", seq))                     # a fragment that is no integer
        elif k == 11:
            out.append(sam(frag + b"/1", b"%d" % flag, rname, b"33", seq, n_fields=10))
        else:
            out.append(sam(frag + b"/%d" % rng.integers(1, 3), b"%d" % flag, rname, b"%d" % rng.integers(-5, 6000), seq, n_fields=int(rng.integers(10, 15))))
    if bad:
        out[-3] = sam(b"5/3")
    return b"\n".join(out) + b"\n"


def fq(name, seq=b"ACGTN", plus=b"+", qual=None):
    return name + b"\n" + seq + b"\n" + plus + b"\n" + (b"I" * len(seq) if qual is None else qual) + b"\n"


def sam_tuple(res):
    return tuple(int(getattr(res, f)) for f in SAM_FIELDS)


def check_sam(ctx, data, final=True, carry_in=0, names=None, name_list=NAMES):
    """One txt_parse_sam against the oracle: the whole result, the alignments, the line numbers, the view."""
    want = ora.parse_sam(data, name_list, final, carry_in)
    res = ctx.parse_sam(data, final, carry_in, names)
    assert sam_tuple(res) == tuple(want[f] for f in SAM_FIELDS)
    als, line_of = ctx.sam_alignments(lines=True)
    assert als.tolist() == want["alignments"] and line_of.tolist() == want["line_of"]
    v = ctx.sam_view()
    assert v.n == len(als) and v.alignments and v.line_of
    return want


def fastq_tuple(res):
    return tuple(int(getattr(res, f)) for f in FASTQ_FIELDS)


def store_of(data, reads):
    return data.tobytes(), [tuple(r) for r in reads.tolist()]


def check_fastq_files(ctx, text, files, max_read_len=None):
    """Whole files, one txt_fastq_add each, against the oracle; returns the oracle's records of all files."""
    ctx.fastq_begin()
    records = []
    for data in files:
        want = ora.parse_fastq(data, True, max_read_len or text.MAX_READ_LEN)
        assert fastq_tuple(ctx.fastq_add(data, True)) == tuple(want[f] for f in FASTQ_FIELDS)
        records += want["records"]
        assert store_of(*ctx.fastq_fetch()) == ora.read_store(records)
    v = ctx.fastq_view()
    assert v.bytes and v.reads and v.n_reads == sum(1 for r in records if not r[3])
    return records


# ---------------------------------------------------------------------------------------------- without a GPU
def test_text_header_and_binding_agree(text):
    """sizeof and offsetof of every struct of the header, as g++ and gcc -std=c99 see them, against the ctypes structs and
    the numpy dtypes; every declared function bound and exported."""
    consts = {"TXT_MAX_READ_LEN": text.MAX_READ_LEN, "TXT_SAM_EMPTY_LINE": text.SAM_EMPTY_LINE, "TXT_SAM_BAD_QNAME": text.SAM_BAD_QNAME,
              "TXT_FASTQ_BAD_NAME": text.FASTQ_BAD_NAME, "TXT_FASTQ_LONG_READ": text.FASTQ_LONG_READ}
    sizes, n = abi.check("defuse_text.h", text, r"(?:txt|cand|bat)_[a-z_]+", constants=consts,
                         dtypes=[(text.SamResult, text.SAM_RESULT_DTYPE), (text.FastqResult, text.FASTQ_RESULT_DTYPE)])
    assert text.SAM_RESULT_DTYPE.itemsize % 8 == 0 and text.FASTQ_RESULT_DTYPE.itemsize % 8 == 0
    assert sizes == [48, 32, 40, 40, 48] and n == 17
    assert (text.ALIGNMENT_DTYPE.itemsize, text.READ_DTYPE.itemsize) == (24, 24)
    for method in ("parse_sam", "sam_alignments", "fastq_begin", "fastq_add", "fastq_fetch", "reads_store"):
        assert hasattr(text.Context, method)
    assert callable(text.enumerate_resident) and hasattr(text, "Names")


def test_text_argument_errors_need_no_device(text, cand, bat):
    lib = text.lib()
    err = lambda: lib.txt_last_error().decode()
    h = ctypes.c_void_p()
    one = ctypes.c_void_p(1)           # stands for an object or a buffer: the argument errors are found before any is looked at
    data = np.frombuffer(b"chr1chr22chr1", dtype=np.uint8)

    def create(off=(0, 4, 9), nbytes=len(data), n_names=None, out=h, device=0):
        o = np.array(off, dtype=np.int64)
        return lib.txt_names_create(device, data.ctypes.data if nbytes else None, nbytes, o.ctypes.data if len(o) else None,
                                    len(o) - 1 if n_names is None else n_names, ctypes.byref(out) if out is not None else None)
    assert create(out=None) == E_ARG
    assert create(n_names=-1) == E_ARG and "negative" in err()
    assert create(nbytes=-1) == E_ARG and "negative" in err()
    assert create(off=(), n_names=2) == E_ARG and "null" in err()
    assert create(nbytes=0) == E_ARG and "name 0" in err()                                 # no bytes at all: every name ends outside
    assert create(n_names=2 ** 31) == E_LIMIT
    assert create(off=(-1, 4, 9)) == E_ARG and "name 0" in err()
    assert create(off=(0, 5, 4)) == E_ARG and "name 1" in err() and "ascend" in err()
    assert create(off=(0, 4, 14)) == E_ARG and "name 1" in err() and "outside" in err()     # one byte beyond
    assert create(off=(0, 4, 2 ** 62)) == E_ARG and "name 1" in err()
    assert create(off=(0, 4, 9, 13)) == E_ARG and "names 0 and 2" in err()                  # chr1 twice
    assert create(off=(0, 0, 4, 4)) == E_ARG and "names 0 and 2" in err()                   # the empty name twice
    assert create(device=999) == E_DEVICE and "999" in err()
    assert not h
    lib.txt_names_destroy(None)

    assert lib.txt_create(0, None) == E_ARG
    assert lib.txt_create(999, ctypes.byref(h)) == E_DEVICE and "999" in err() and not h
    assert lib.txt_create(-1, ctypes.byref(h)) == E_DEVICE and not h
    lib.txt_destroy(None)
    assert lib.txt_set_max_read_len(None, 5) == E_ARG

    res = text.SamResult()
    res.n_lines = -7
    buf = np.frombuffer(b"7/1\t0\n", dtype=np.uint8)
    for fn in (lib.txt_parse_sam, lib.txt_parse_sam_device):
        call = lambda c=one, n=one, t=buf.ctypes.data, ln=len(buf), final=1, carry=0, r=ctypes.byref(res): fn(c, n, t, ln, final, carry, r)
        assert call(r=None) == E_ARG
        assert call(ln=-1) == E_ARG and "negative" in err() and res.n_lines == 0
        assert call(t=None) == E_ARG and "null" in err()
        assert call(ln=2 ** 31) == E_LIMIT and "pieces" in err()                            # (the fake pointer is never read)
        assert call(t=1, ln=2 ** 40) == E_LIMIT and "pieces" in err()
        assert call(final=2) == E_ARG and "final" in err()
        assert call(final=-1) == E_ARG and "final" in err()
        assert call(carry=2) == E_ARG and "carry_in" in err()
        assert call(carry=-1) == E_ARG and "carry_in" in err()
        assert call(c=None) == E_ARG and "no ctx" in err()
        assert call(n=None) == E_ARG and "no names" in err()
    view, fview, timing = text.SamView(), text.FastqView(), text.TxtTiming()
    assert lib.txt_sam_view(None, ctypes.byref(view)) == E_ARG and lib.txt_fastq_view(None, ctypes.byref(fview)) == E_ARG
    assert lib.txt_get_timing(None, ctypes.byref(timing)) == E_ARG
    assert lib.txt_sam_fetch(None, None, 0, None, 0) == E_ARG and lib.txt_fastq_fetch(None, None, 0, None, 0) == E_ARG
    assert lib.txt_fastq_begin(None) == E_ARG
    fres = text.FastqResult()
    add = lambda c=one, t=buf.ctypes.data, ln=len(buf), final=1, r=ctypes.byref(fres): lib.txt_fastq_add(c, t, ln, final, r)
    assert add(r=None) == E_ARG
    assert add(ln=-1) == E_ARG and "negative" in err()
    assert add(t=None) == E_ARG and "null" in err()
    assert add(t=1, ln=2 ** 31) == E_LIMIT and "pieces" in err()
    assert add(final=2) == E_ARG and "final" in err()
    assert add(c=None) == E_ARG and "no ctx" in err()

    # the twins: cand_enumerate_resident and bat_reads_create_device
    cerr = lambda: lib.cand_last_error().decode()
    n_out, first_bad = ctypes.c_int64(-7), ctypes.c_int64(-7)
    res_call = lambda s=None, a=one, n=1, order=0, no=ctypes.byref(n_out), fb=ctypes.byref(first_bad): lib.cand_enumerate_resident(s, a, n, order, no, fb, None)
    assert res_call(no=None) == E_ARG and res_call(fb=None) == E_ARG
    assert res_call(n=-1) == E_ARG and "negative" in cerr() and (n_out.value, first_bad.value) == (0, -1)
    assert res_call(n=2 ** 31) == E_LIMIT
    assert res_call(a=None) == E_ARG and "no alignments" in cerr()
    assert res_call(order=2) == E_ARG and "order" in cerr()
    assert res_call(order=-1) == E_ARG and "order" in cerr()
    assert res_call() == E_ARG and "session" in cerr()                                       # (the device array is not looked at without one)
    berr = lambda: lib.bat_last_error().decode()
    rd = lambda b=one, nb=8, r=one, n=1, out=ctypes.byref(h), device=0: lib.bat_reads_create_device(device, b, nb, r, n, out)
    assert rd(out=None) == E_ARG
    assert rd(n=-1) == E_ARG and "negative" in berr()
    assert rd(nb=-1) == E_ARG and "negative" in berr()
    assert rd(r=None) == E_ARG and "null" in berr()
    assert rd(b=None) == E_ARG and "null" in berr()
    assert rd(n=2 ** 31) == E_LIMIT
    assert rd(device=999) == E_DEVICE and "999" in berr()
    assert not h
    # good arguments get as far as the device: no CPU path
    rc = lib.txt_create(0, ctypes.byref(h))
    assert rc in (0, E_DEVICE)
    if rc == 0:
        assert lib.txt_set_max_read_len(h, 0) == E_ARG and lib.txt_set_max_read_len(h, 2 ** 24 + 1) == E_ARG and lib.txt_set_max_read_len(h, 2 ** 24) == 0
        assert lib.txt_sam_view(h, ctypes.byref(view)) == 0 and view.n == 0 and view.alignments
        assert lib.txt_sam_view(h, None) == E_ARG
        assert lib.txt_sam_fetch(h, None, -1, None, 0) == E_ARG and lib.txt_sam_fetch(h, None, 1, None, 0) == E_ARG
        assert lib.txt_sam_fetch(h, None, 0, None, 0) == 0
        lib.txt_destroy(h)
    else:
        assert not h and "device" in err()


HOST_PROGRAM = r'''
#include "@ROOT@/tools_src/defuse_host.hpp"
// What the tools' host parser yields for a text file: "sam <file> <carry_in>" prints per record
//   A <line> <rname in hex, - if empty> <strand> <start> <end> <fragment or -1> <read end>
// with the read end carried as dosplitalign.cpp carries it, then "S <line> <kind>" at a stop and "N <lines consumed>";
// "fastq <file>" prints "R <fragment> <end> <length> <sequence in hex>" per record, "S <name line> <kind>" at a stop.
using namespace defuse;
static std::string hex(const char* p, size_t n)
{
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t k = 0; k < n; ++k) { s += d[(unsigned char)p[k] >> 4]; s += d[(unsigned char)p[k] & 15]; }
    return s.empty() ? "-" : s;
}
int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    if (mode == "sam") {
        const int carry = argc > 3 ? atoi(argv[3]) : 0;
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        LineReader lr(f);
        const char* l;
        size_t n, no = 0, consumed = 0;
        int readEnd = -1;
        SamFields a;
        while (lr.next(l, n)) {
            ++no;
            const int kind = ParseSamLine(l, n, a, readEnd);
            if (kind >= 2) { printf("S %zu %d\n", no, kind); break; }
            consumed = no;
            if (kind == 1) continue;
            int frag = 0;
            const bool ok = field_int(a.fragment, a.fragment_len, frag) && frag >= 0;
            printf("A %zu %s %d %d %d %d %d\n", no, hex(a.reference, a.reference_len).c_str(), (int)a.strand, a.region.start, a.region.end, ok ? frag : -1,
                   readEnd < 0 ? carry : readEnd);
        }
        printf("N %zu\n", consumed);
        fclose(f);
        return 0;
    }
    FastqReader in;
    std::ostringstream err;
    if (!in.open(argv[2], err)) return 2;
    FastqRecord r;
    size_t n_rec = 0;
    int stop = 0;
    while (in.next(r, err)) {
        int frag = 0;
        if (!field_int(r.fragment.data(), r.fragment.size(), frag)) { stop = 3; break; }
        if (r.sequence.size() >= ((size_t)1 << 24)) { stop = 4; break; }
        printf("R %d %d %zu %s\n", frag, r.end, r.sequence.size(), hex(r.sequence.data(), r.sequence.size()).c_str());
        ++n_rec;
    }
    if (!stop && err.str().find("read name") != std::string::npos) stop = 1;
    if (!stop && err.str().find("read end") != std::string::npos) stop = 2;
    if (stop) printf("S %zu %d\n", 4 * n_rec + 1, stop);
    return 0;
}
'''

# the rule tables: (text, carry_in) of the SAM cases, texts of the FASTQ cases.  The GPU tests walk the same tables.
TWENTY = b"12345678901234567890"
SAM_CASES = [
    (b"@HD\tVN:1.0\n" + sam() + b"\n", 0),
    (sam(rname=b"*") + b"\n" + sam() + b"\n", 0),
    (sam(rname=b"*", flag=b"x") + b"\n", 0),                       # stop 4 wins over the skip
    (sam(n_fields=9) + b"\n", 0),
    (sam(n_fields=10) + b"\n", 0), (sam(n_fields=10), 0), (sam(n_fields=14) + b"\n", 0), (sam(n_fields=14), 0),
    (sam() + b"\n\n" + sam(b"8/2") + b"\n", 0),                    # an empty line between good ones
    (sam(n_fields=10) + b"\r\n" + sam(b"8/2", n_fields=10) + b"\r\n", 0),
    (sam(n_fields=11) + b"\r\n", 0),
] + [(sam(flag=f) + b"\n" + sam(b"9", flag=f) + b"\n", 1) for f in (b"+16", b"-0", b"0016", b" 16", b"16 ", b"2147483647", b"2147483648", b"-2147483648",
                                                                     TWENTY, b"", b"+", b"-", b"1-6", b"0x10", b"0000000000000000000000064")] + [
    (sam(pos=b"2147483647", seq=b"AC") + b"\n", 0),
    (sam(pos=b"-2147483648", seq=b"") + b"\n", 0),
    (sam(pos=b"2147483648") + b"\n", 0), (sam(pos=TWENTY) + b"\n", 0), (sam(pos=b"") + b"\n", 0),
] + [(sam(q, fl) + b"\n", c) for q in (b"7/1", b"7/2", b"7/3", b"7/", b"/1", b"7/1/2", b"a/1", b"-3/1", b"2147483648/1", b"2147483647/2", b"+5/1", b"007/2",
                                        b"", b"/", b"//", b"7/12", b"7", TWENTY)
     for fl, c in ((b"0", 0), (b"0", 1), (b"64", 1), (b"128", 0), (b"192", 1))] + [
    (b"".join(sam(rname=r) + b"\n" for r in (b"chr1", b"chr10", b"chr1_x", b"chr", b"chr11", b"chr1_", b"chrX", b"", b"chr2", b"ENSG01|ENST01", b"chr1\r")), 0),
    (sam(b"5") + b"\n", 0), (sam(b"5") + b"\n", 1),                                                   # carried from carry_in
    (sam(b"5/2") + b"\n" + sam(b"6") + b"\n", 0), (sam(b"5", b"64") + b"\n" + sam(b"6") + b"\n", 1),  # from the line before
    (sam(b"5/2") + b"\n" + b"@x\n" * 39 + sam(b"6") + b"\n" + sam(b"7/1") + b"\n" + sam(rname=b"*") + b"\n", 0),   # from forty lines before
    (sam(b"5/2") + b"\n" + sam(b"6/9") + b"\n" + sam(b"7/1") + b"\n", 0),                             # the stop hands on what was told before it
]
FASTQ_CASES = [
    fq(b"@7/1") + fq(b"7/2"), fq(b"@7/1") + fq(b""), fq(b"@7"), fq(b"@7/"), fq(b"@7/3"), fq(b"@x/1"), fq(b"@/1"), fq(b"@-/1"), fq(b"@-3/1") + fq(b"@3/2"),
    fq(b"@7/1 extra/2"), fq(b"@7 extra/2"), fq(b"@+7/2/1"), fq(b"@2147483647/1") + fq(b"@2147483648/1"), fq(b"@-2147483648/2"),
    fq(b"@1/1") + fq(b"@2/2") + fq(b"@3/x") + fq(b"@4/1") + fq(b"@5/1"),                             # a stop in the third of five
    fq(b"@1/1", b""), fq(b"@1/1", b"", b"", b""), fq(b"@1/1\r", b"ACGT\r"),
    fq(b"@5/1", b"AAAA") + fq(b"@5/1", b"CC") + fq(b"@5/2", b"G"),                                   # one key twice
] + [fq(b"@1/1") + rest for rest in (b"@2/1", b"@2/1\n", b"@2/1\nAC", b"@2/1\nAC\n", b"@2/1\nAC\n+", b"@2/1\nAC\n+\n", b"@2/1\nAC\n+\nII", b"\n", b"\n\n\n")]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("text_host")
    src = d / "text_host.cpp"
    src.write_text(HOST_PROGRAM.replace("@ROOT@", ROOT))
    exe = d / "text_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fwrapv", "-pthread", "-o", str(exe), str(src)])
    return str(exe), d


def host_sam(host_program, data, carry_in, k):
    exe, d = host_program
    path = d / ("t%d.sam" % k)
    path.write_bytes(data)
    out = subprocess.run([exe, "sam", str(path), str(carry_in)], capture_output=True, text=True, check=True).stdout.splitlines()
    return [tuple(l.split()) for l in out]


def oracle_sam_lines(data, carry_in, name_list=NAMES):
    """The oracle's result in the host program's lines."""
    want = ora.parse_sam(data, name_list, True, carry_in)
    back = {k: n for k, n in enumerate(name_list)}
    lines = ora.split_lines(data, True)
    out = []
    for a, no in zip(want["alignments"], want["line_of"]):
        rname = back[a[0]] if a[0] >= 0 else data[lines[no - 1][0]:lines[no - 1][1]].split(b"\t")[2]
        out.append(("A", str(no), rname.hex() or "-") + tuple(str(x) for x in a[1:]))
    if want["stop_kind"]:
        out.append(("S", str(want["stop_line"]), str(want["stop_kind"])))
    out.append(("N", str(want["n_lines"])))
    return out


def test_oracle_equals_the_host_parser(host_program):
    """tests/text_oracle.py against ParseSamLine (the read end carried as dosplitalign.cpp carries it) and FastqReader::next +
    field_int of tools_src/defuse_host.hpp, on the rule tables and on random texts, stops included.  The FASTQ record
    with a negative fragment, which the library skips, is compared as the record the host parser reads."""
    n_records = 0
    texts = SAM_CASES + [(random_sam(s, 300), s & 1) for s in range(6)] + [(random_sam(9, 2000, bad=False), 1)]
    for k, (data, carry_in) in enumerate(texts):
        got = host_sam(host_program, data, carry_in, k)
        assert got == oracle_sam_lines(data, carry_in), (k, data[:200])
        n_records += sum(1 for l in got if l[0] == "A")
    assert n_records > 2000
    assert {l[2] for d, c in SAM_CASES for l in oracle_sam_lines(d, c) if l[0] == "S"} == {"2", "3", "4", "5"}
    exe, d = host_program
    kinds = set()
    for k, data in enumerate(FASTQ_CASES + [random_fastq(3, 200)]):
        path = d / ("t%d.fastq" % k)
        path.write_bytes(data)
        got = [tuple(l.split()) for l in subprocess.run([exe, "fastq", str(path)], capture_output=True, text=True, check=True).stdout.splitlines()]
        want = ora.parse_fastq(data, True)
        exp = [("R", str(f), str(e), str(len(s)), s.hex() or "-") for f, e, s, _ in want["records"]]
        if want["stop_kind"]:
            exp.append(("S", str(want["stop_line"]), str(want["stop_kind"])))
            kinds.add(want["stop_kind"])
        assert got == exp, (k, data[:200])
    assert kinds == {1, 2, 3}


def random_fastq(seed, n, end=1):
    rng = np.random.default_rng(seed)
    return b"".join(fq(b"@%d/%d" % (rng.integers(0, 1000), end), b"ACGTN"[int(rng.integers(0, 5)):][:1] * int(rng.integers(0, 200))) for _ in range(n))


# ---------------------------------------------------------------------------------------------- GPU: SAM
@pytest.mark.gpu
def test_sam_rule_table(text, ctx):
    stops = set()
    for data, carry_in in SAM_CASES:
        stops.add(check_sam(ctx, data, True, carry_in)["stop_kind"])
    assert stops == {0, 2, 3, 4, 5}
    # some of them spelled out, so that the oracle is not the only witness
    r = check_sam(ctx, sam(pos=b"2147483647", seq=b"AC") + b"\n")
    assert r["alignments"] == [(0, 0, 2147483647, -2147483648, 7, 0)]
    r = check_sam(ctx, sam(n_fields=10) + b"\r\n" + sam(b"8/2", n_fields=10) + b"\r\n")
    assert [a[3] for a in r["alignments"]] == [105, 105]                    # the '\r' counts into the sequence length
    r = check_sam(ctx, sam() + b"\n\n" + sam(b"8/2") + b"\n")
    assert (r["stop_kind"], r["stop_line"], r["n_alignments"], r["consumed"]) == (2, 2, 1, len(sam()) + 1)
    r = check_sam(ctx, sam(rname=b"*", flag=b"x") + b"\n")
    assert (r["stop_kind"], r["stop_line"], r["consumed"]) == (4, 1, 0)
    r = check_sam(ctx, sam(b"7/1/2", b"128") + b"\n")
    assert r["alignments"] == [(0, 0, 100, 104, -1, 1)] and r["n_bad_fragment"] == 1
    r = check_sam(ctx, sam(b"-3/1") + b"\n" + sam(b"2147483648/1") + b"\n" + sam(b"2147483647/2", b"+16") + b"\n")
    assert [(a[1], a[4], a[5]) for a in r["alignments"]] == [(0, -1, 0), (0, -1, 0), (1, 2147483647, 1)]
    r = check_sam(ctx, b"".join(sam(rname=n) + b"\n" for n in (b"chr1", b"chr10", b"chr1_x", b"chr11", b"", b"chr")))
    assert [a[0] for a in r["alignments"]] == [0, 1, 2, -1, -1, -1]
    r = check_sam(ctx, sam(b"5/2") + b"\n" + b"@x\n" * 39 + sam(b"6") + b"\n")
    assert [a[5] for a in r["alignments"]] == [1, 1] and r["carry_out"] == 1 and r["line_of"] == [1, 41]
    assert check_sam(ctx, sam(b"5") + b"\n", carry_in=1)["alignments"][0][5] == 1
    # the empty rname against a table with the empty name; names handed over in another order than the sorted one
    other = [b"chr2", b"", b"chr10", b"chr1"]
    with text.Names(other) as nm:
        r = check_sam(ctx, b"".join(sam(rname=n) + b"\n" for n in (b"", b"chr1", b"chr10", b"chr2", b"chr1_x")), names=nm, name_list=other)
        assert [a[0] for a in r["alignments"]] == [1, 3, 2, 0, -1]
    with text.Names([]) as nm:
        assert check_sam(ctx, sam() + b"\n", names=nm, name_list=[])["alignments"][0][0] == -1


@pytest.mark.gpu
def test_sam_geometry(text, ctx):
    # line lengths 1 .. 600: line starts at every offset modulo 16, 64 and 256
    lines = []
    for n in range(1, 601):
        base = sam(b"%d/1" % n, seq=b"", n_fields=10)
        lines.append(b"@" + b"c" * (n - 1) if n <= len(base) else sam(b"%d/1" % n, seq=b"A" * (n - len(base)), n_fields=10))
    assert [len(l) for l in lines] == list(range(1, 601))
    data = b"\n".join(lines) + b"\n"
    starts = np.cumsum([0] + [len(l) + 1 for l in lines[:-1]])
    assert len(set((starts % 256).tolist())) == 256
    r = check_sam(ctx, data)
    assert r["n_lines"] == 600 and r["n_alignments"] > 500
    # a 5 000-base and a 70 000-base record between short ones: lines longer than a workgroup's 4096 bytes
    data = b"".join(sam(b"%d/2" % k, seq=b"C" * n) + b"\n" for k, n in enumerate((3, 5000, 7, 70000, 0, 2)))
    r = check_sam(ctx, data)
    assert [a[3] - a[2] + 1 for a in r["alignments"]] == [3, 5000, 7, 70000, 0, 2]
    # 3 000 two-byte header lines around one record: more lines in a workgroup's span than it has lanes
    data = b"@\n" * 1500 + sam() + b"\n" + b"@\n" * 1500
    r = check_sam(ctx, data)
    assert (r["n_lines"], r["line_of"]) == (3001, [1501])
    # nothing, one newline, one line without a newline
    for data in (b"", b"\n", sam(), sam(n_fields=9), b"@", b"\t"):
        for final in (True, False):
            r = check_sam(ctx, data, final)
            if not final and not data.endswith(b"\n"):
                assert (r["consumed"], r["n_lines"], r["stop_kind"]) == (0, 0, 0)
    assert check_sam(ctx, b"\n")["stop_kind"] == 2 and check_sam(ctx, sam())["n_alignments"] == 1
    # the same text from host memory and from device memory
    data = random_sam(21, 2000)
    want = check_sam(ctx, data)
    assert want["stop_kind"] == 5 and want["n_alignments"] > 1500
    host = ctx.sam_alignments(lines=True)
    with DeviceArray(np.frombuffer(data, dtype=np.uint8)) as dev:
        res = ctx.parse_sam_device(dev.ptr, len(data))
        assert sam_tuple(res) == tuple(want[f] for f in SAM_FIELDS)
        got = ctx.sam_alignments(lines=True)
        assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes()
        cut = data.rfind(b"\n", 0, len(data) // 2)                          # final = 0: the device entry drops the unfinished line itself
        res = ctx.parse_sam_device(dev.ptr, cut + 10, final=False)
        assert sam_tuple(res) == tuple(ora.parse_sam(data[:cut + 10], NAMES, False)[f] for f in SAM_FIELDS) and cut < res.consumed <= cut + 10
    t = ctx.timing()
    assert t["text_bytes"] == cut + 10 and t["n_records"] == res.n_alignments and t["device_ms"] > 0
    # a short buffer: nothing is written
    lib = ctx._lib
    small = np.full(3, -1, dtype=np.int32)
    assert lib.txt_sam_fetch(ctx.handle, small.ctypes.data, 0, None, 0) == E_CAPACITY
    als = np.zeros(res.n_alignments, dtype=text.ALIGNMENT_DTYPE)
    assert lib.txt_sam_fetch(ctx.handle, als.ctypes.data, len(als), small.ctypes.data, 3) == E_CAPACITY and (small == -1).all() and not als.view(np.uint8).any()


def in_pieces(ctx, data, cuts, carry_in=0):
    """The text in pieces that end at `cuts` (the last one final), each call starting where the one before stopped consuming:
    (concatenated alignments, summed n_lines, stop kind, stop line within the whole text, carry_out)."""
    als, n_lines, begin, carry = [], 0, 0, carry_in
    for k, end in enumerate(cuts):
        final = k == len(cuts) - 1
        res = ctx.parse_sam(data[begin:end], final, carry)
        if res.n_alignments:
            als += ctx.sam_alignments().tolist()
        if res.stop_kind:
            return als, n_lines + res.n_lines, res.stop_kind, n_lines + res.stop_line, res.carry_out
        n_lines += res.n_lines
        begin += res.consumed
        carry = res.carry_out
    assert begin == len(data)
    return als, n_lines, 0, 0, carry


@pytest.mark.gpu
def test_sam_in_pieces(ctx):
    head = b"@HD\n" + sam(b"5", b"128") + b"\n" + sam(b"6") + b"\n@x\n" + sam(b"7/1") + b"\n" + sam(b"8", rname=b"*") + b"\n" + sam(b"9", seq=b"A" * 60) + b"\n"
    for last in (sam(b"1/3"), sam(b"1")):                          # with a stop in the last line, which has no newline, and without
        body = head + b"@" + b"c" * (400 - len(head) - len(last) - 2) + b"\n" + last
        assert len(body) == 400
        one = ora.parse_sam(body, NAMES, True, 0)
        want = (one["alignments"], one["n_lines"], one["stop_kind"], one["stop_line"], one["carry_out"])
        assert len(want[0]) >= 3
        for cut in range(len(body) + 1):
            assert in_pieces(ctx, body, [cut, len(body)]) == want, cut
    for bad in (True, False):
        data = random_sam(33, 2000, bad, max_seq=12)
        one = ora.parse_sam(data, NAMES, True, 1)
        want = (one["alignments"], one["n_lines"], one["stop_kind"], one["stop_line"], one["carry_out"])
        assert len(want[0]) > 1500 and bool(want[2]) == bad
        for size in ((1, 7, 4096) if bad else (7, 4096)):
            cuts = list(range(size, len(data), size)) + [len(data)]
            assert in_pieces(ctx, data, cuts, 1) == want, size


# ---------------------------------------------------------------------------------------------- GPU: into the enumeration
def oracle_chain_inputs(cand, case):
    """Tasks, mate regions with their dense reference numbering, reads and windows of a pipeline_case data set."""
    from oracle import dosplitalign_oracle as dora
    tasks = dora.create_tasks(case["fasta"], case["exons"], case["ufrag"], case["sfrag"], case["minread"], case["maxread"],
                              dora.read_align_region_pairs(case["regions"]))
    index, regs = {}, []
    for t in tasks.values():
        for ce in (0, 1):
            for loc in t.mate_regions[ce]:
                regs.append((index.setdefault(loc["refName"], len(index)), loc["strand"], loc["start"], loc["end"], cand.cluster_id(t.fusion_id, ce)))
    name_list = [n.encode() if isinstance(n, str) else n for n in index]
    windows = {t.fusion_id: (t.seq[0], t.seq[1]) for t in tasks.values()}
    return cand.regions(regs), name_list, windows


@pytest.fixture(scope="module")
def chain_case(tmp_path_factory, cand):
    case = pipeline_case.build(str(tmp_path_factory.mktemp("text_case")), seed=17, n_fusions=8, reads_per_fusion=25, lq=50)
    regs, name_list, windows = oracle_chain_inputs(cand, case)
    return case, regs, name_list, windows


@pytest.mark.gpu
def test_parse_into_the_enumeration(text, cand, chain_case):
    case, regs, name_list, _ = chain_case
    data = open(case["improper"], "rb").read()
    want = ora.parse_sam(data, name_list)
    host_als = cand.alignments(want["alignments"])
    assert len(host_als) > 150 and want["n_bad_fragment"] == 0 and (host_als["ref"] >= 0).all()
    with text.Names(name_list) as nm, text.Context(nm) as T, cand.Table(regs) as table:
        for order in (cand.ORDER_VISIT, cand.ORDER_FUSION):
            with table.session() as s:
                host = s.enumerate(host_als, order)
            assert len(host) > 100
            T.parse_sam(data)
            v = T.sam_view()
            with table.session() as s:
                ptr, n = text.enumerate_resident(s, v.alignments, v.n, order)
                assert from_device(ptr, n, cand.RECORD_DTYPE).tobytes() == host.tobytes()
                assert s.timing.n_kept == n and s.timing.download_ms == 0
        # a qname that is no integer: on a mate that overlaps nothing it changes nothing ...
        lines = data.split(b"\n")
        rec = [k for k, l in enumerate(lines) if l and not l.startswith(b"@") and l.split(b"\t")[2] != b"*"]
        hit = rec[40]
        f = lines[hit].split(b"\t")
        nowhere = b"\t".join([b"read/x/y", f[1], f[2], b"900000"] + f[4:])
        inside = b"\t".join([b"read/x/y"] + f[1:])
        far = b"\n".join(lines[:hit] + [nowhere] + lines[hit:])
        res = T.parse_sam(far)
        assert res.n_bad_fragment == 1 and res.n_alignments == len(host_als) + 1
        v = T.sam_view()
        with table.session() as s:
            host = s.enumerate(host_als, cand.ORDER_VISIT)
        with table.session() as s:
            ptr, n = text.enumerate_resident(s, v.alignments, v.n)
            got = from_device(ptr, n, cand.RECORD_DTYPE)
        k_far = rec.index(hit)                                                  # its index among the alignments
        shifted = host.copy()
        shifted["alignment"][host["alignment"] >= k_far] += 1
        assert got.tobytes() == shifted.tobytes()
        # ... inside a mate region it fails the call, names itself and leaves the session as it was
        res = T.parse_sam(b"\n".join(lines[:hit] + [inside] + lines[hit:]))
        assert res.n_bad_fragment == 1
        v = T.sam_view()
        with table.session() as s:
            with pytest.raises(cand.CandError) as e:
                text.enumerate_resident(s, v.alignments, v.n)
            assert e.value.code == E_ARG and e.value.first_bad == k_far and ("alignment %d:" % k_far) in str(e.value)
            dev, m = ctypes.c_void_p(1), ctypes.c_int64(-1)
            assert s._lib.cand_records_device(s.handle, ctypes.byref(dev), ctypes.byref(m)) == 0 and not dev.value and m.value == 0
            ptr, n = text.enumerate_resident(s, v.alignments, k_far)            # the alignments before it
            with table.session() as s2:
                assert from_device(ptr, n, cand.RECORD_DTYPE).tobytes() == s2.enumerate(host_als[:k_far]).tobytes()
            assert n > 0
        # a strand of 2 in a hand-made device array
        bad = host_als[:50].copy()
        bad["strand"][[17, 30]] = 2
        with DeviceArray(bad) as dev, table.session() as s:
            with pytest.raises(cand.CandError) as e:
                text.enumerate_resident(s, dev.ptr, len(bad))
            assert e.value.code == E_ARG and e.value.first_bad == -1 and "alignment 17:" in str(e.value)
        bad = host_als[:50].copy()
        bad["read_end"][9] = -1
        with DeviceArray(bad) as dev, table.session() as s:
            with pytest.raises(cand.CandError) as e:
                text.enumerate_resident(s, dev.ptr, len(bad))
            assert "alignment 9:" in str(e.value)
            assert text.enumerate_resident(s, dev.ptr, 0) == (0, 0)


# ---------------------------------------------------------------------------------------------- GPU: FASTQ
@pytest.mark.gpu
def test_fastq_rule_table_and_geometry(text, ctx):
    kinds = set()
    for data in FASTQ_CASES:
        ctx.fastq_begin()
        want = ora.parse_fastq(data, True)
        assert fastq_tuple(ctx.fastq_add(data, True)) == tuple(want[f] for f in FASTQ_FIELDS), data
        assert store_of(*ctx.fastq_fetch()) == ora.read_store(want["records"]), data
        kinds.add(want["stop_kind"])
    assert kinds == {0, 1, 2, 3}
    # spelled out
    one = lambda data, final=True: (ctx.fastq_begin(), fastq_tuple(ctx.fastq_add(data, final)))[1]
    assert one(fq(b"7/1")) == (len(fq(b"7/1")), 0, 0, 1, 1) and one(fq(b"")) == (len(fq(b"")), 0, 0, 1, 1)
    assert one(fq(b"@7"))[3:] == (1, 2) and one(fq(b"@7/"))[3:] == (1, 2) and one(fq(b"@7/3"))[3:] == (1, 2) and one(fq(b"@x/1"))[3:] == (1, 3)
    assert one(fq(b"@-3/1") + fq(b"@3/2")) == (len(fq(b"@-3/1") + fq(b"@3/2")), 1, 1, 0, 0)
    assert one(fq(b"@7/1 extra/2"))[1:] == (1, 0, 0, 0) and ctx.fastq_fetch()[1]["read_end"].tolist() == [0]
    five = fq(b"@1/1") + fq(b"@2/2") + fq(b"@3/x") + fq(b"@4/1") + fq(b"@5/1")
    assert one(five) == (len(five), 2, 0, 9, 2) and ctx.fastq_fetch()[1]["fragment"].tolist() == [1, 2]
    # incomplete groups: five, six and seven lines
    for rest in (b"@2/1\n", b"@2/1\nAC\n", b"@2/1\nAC\n+\n", b"@2/1\nAC\n+"):
        data = fq(b"@1/1") + rest
        assert one(data) == (len(data), 1, 0, 0, 0)
        assert one(data, False) == (len(fq(b"@1/1")), 1, 0, 0, 0)                     # final = 0 leaves them unconsumed
    data = fq(b"@1/1") + b"@2/1\nAC\n+\nII"                                           # eight lines, the last without a newline
    assert one(data) == (len(data), 2, 0, 0, 0) and one(data, False) == (len(fq(b"@1/1")), 1, 0, 0, 0)
    assert one(b"@2/1\nAC\n+\nII", False) == (0, 0, 0, 0, 0) and one(b"", True) == (0, 0, 0, 0, 0) and one(b"@2/1", False) == (0, 0, 0, 0, 0)
    # sequences of 0 .. 300 bases and one of 70 000; two-byte lines; the same key twice in one file and across two files
    seqs = [bytes(b"ACGTN"[(n + j) % 5] for j in range(n)) for n in range(301)] + [b"G" * 70000, b"T"]
    file1 = b"".join(fq(b"@%d/1" % k, s) for k, s in enumerate(seqs))
    file2 = b"".join(fq(b"@%d/2" % k, s[::-1]) for k, s in enumerate(seqs[:50])) + fq(b"@7/1", b"CCCCC") + fq(b"@7/1", b"TT")
    records = check_fastq_files(ctx, text, [file1, file2])
    assert len(records) == 303 + 52
    t = ctx.timing()
    assert t["n_records"] == 52 and t["gather_bytes"] == sum(len(s) for s in seqs[:50]) + 7 and t["text_bytes"] == len(file2)
    check_fastq_files(ctx, text, [b"@1/1\n\n\n\n" * 3000 + fq(b"@2/2", b"ACGT") + b"@3/1\n\n\n\n" * 3000])     # 24 000 lines of 0 and 4 bytes
    # of two records with one key the later one wins in the store made of it
    from defuse_amd import bat, cand
    cands = np.zeros(3, dtype=cand.RECORD_DTYPE)
    for k, (frag, rend) in enumerate(((7, 0), (7, 1), (300, 0))):
        cands[k] = (k, 3, frag, 0, rend, 0, 1, (0, 0, 0, 0))
    check_fastq_files(ctx, text, [file1, file2])
    with ctx.reads_store() as r, bat.Windows.from_dict({3: (b"ACGT", b"AC")}) as w, bat.Batch() as b:
        b.assemble(r, w, cands)
        got = b.fetch()
    assert got[2].tobytes() == b"TT" + seqs[7][::-1] + seqs[300] and got[3]["read_len"].tolist() == [2, 7, 300]
    # the stop-4 limit through the context's limit
    ctx.set_max_read_len(10)
    try:
        data = fq(b"@1/1", b"A" * 9) + fq(b"@2/1", b"A" * 10) + fq(b"@3/1")
        ctx.fastq_begin()
        want = ora.parse_fastq(data, True, 10)
        assert fastq_tuple(ctx.fastq_add(data, True)) == tuple(want[f] for f in FASTQ_FIELDS) == (len(data), 1, 0, 5, 4)
        assert fastq_tuple(ctx.fastq_add(fq(b"@x/1") + fq(b"@1/2"), True)) == (2 * len(fq(b"@x/1")), 0, 0, 1, 3)     # the next file counts its own lines
    finally:
        ctx.set_max_read_len(text.MAX_READ_LEN)
    # a short buffer: nothing is written
    check_fastq_files(ctx, text, [fq(b"@1/1") + fq(b"@2/1")])
    small = np.zeros(9, dtype=np.uint8)
    recs = np.zeros(2, dtype=text.READ_DTYPE)
    assert ctx._lib.txt_fastq_fetch(ctx.handle, small.ctypes.data, 9, recs.ctypes.data, 2) == E_CAPACITY and not small.any()
    assert ctx._lib.txt_fastq_fetch(ctx.handle, small.ctypes.data, 0, recs.ctypes.data, 1) == E_CAPACITY and not recs.view(np.uint8).any()


@pytest.mark.gpu
def test_fastq_in_pieces(text, ctx):
    """A file cut at every byte into two pieces, the second starting where the first stopped consuming; a stop in the second
    piece counts its line within the file; pieces after a stop are passed over."""
    data = fq(b"@1/1", b"ACGTACGTAC") + fq(b"@-2/1", b"AC") + fq(b"@3/2 x", b"") + fq(b"@4/1", b"N" * 40) + fq(b"@5/2", b"ACG") + fq(b"@5/2", b"T" * 17)
    data += fq(b"@6/1", b"T" * 10, qual=b"I" * (301 - len(data) - len(fq(b"@6/1", b"T" * 10, qual=b""))))[:-1]      # the last line has no newline
    assert len(data) == 300
    for body in (data, fq(b"@1/1") + fq(b"@2/1") + fq(b"@3/7") + fq(b"@4/1")):
        whole = ora.parse_fastq(body, True)
        for cut in range(len(body) + 1):
            ctx.fastq_begin()
            a = ctx.fastq_add(body[:cut], False)
            b = ctx.fastq_add(body[a.consumed:], True)
            assert a.consumed <= cut and b.consumed == len(body) - a.consumed
            stop = (a.stop_kind, a.stop_line) if a.stop_kind else (b.stop_kind, b.stop_line)
            assert (a.n_records + b.n_records, a.n_skipped + b.n_skipped) + stop == (whole["n_records"], whole["n_skipped"], whole["stop_kind"], whole["stop_line"]), cut
            assert store_of(*ctx.fastq_fetch()) == ora.read_store(whole["records"]), cut
    # after a stop the file's further pieces are passed over; the next file starts afresh
    ctx.fastq_begin()
    assert fastq_tuple(ctx.fastq_add(fq(b"@1/1") + fq(b"@2"), False))[1:] == (1, 0, 5, 2)
    assert fastq_tuple(ctx.fastq_add(fq(b"@3/1"), False)) == (len(fq(b"@3/1")), 0, 0, 5, 2)
    assert fastq_tuple(ctx.fastq_add(b"", True)) == (0, 0, 0, 5, 2)
    assert fastq_tuple(ctx.fastq_add(fq(b"@4/2"), True)) == (len(fq(b"@4/2")), 1, 0, 0, 0)
    assert ctx.fastq_fetch()[1]["fragment"].tolist() == [1, 4]


# ---------------------------------------------------------------------------------------------- GPU: into the store and the chain
@pytest.mark.gpu
def test_store_from_the_parse_and_the_whole_front(text, cand, bat, chain_case, gpu_ctx):
    case, regs, name_list, windows = chain_case
    sam_text = open(case["improper"], "rb").read()
    files = [open(case[k], "rb").read() for k in ("seq1", "seq2")]
    host_als = cand.alignments(ora.parse_sam(sam_text, name_list)["alignments"])
    records = [r for f in files for r in ora.parse_fastq(f)["records"]]
    data, recs = ora.read_store(records)
    host_data, host_recs = np.frombuffer(data, dtype=np.uint8), np.array(recs, dtype=bat.READ_DTYPE)
    assert len(host_recs) > 300
    with text.Names(name_list) as nm, text.Context(nm) as T, cand.Table(regs) as table, bat.Windows.from_dict(windows) as w, bat.Batch() as b:
        T.fastq_begin()
        for f in files:
            half = len(f) // 2
            first = T.fastq_add(f[:half], False)
            assert T.fastq_add(f[first.consumed:], True).stop_kind == 0
        got_data, got_recs = T.fastq_fetch()
        assert got_data.tobytes() == host_data.tobytes() and got_recs.tobytes() == host_recs.tobytes()
        with table.session() as s:
            host_cands = s.enumerate(host_als, cand.ORDER_FUSION)
        with T.reads_store() as r_dev, bat.Reads(host_data, host_recs) as r_host:
            T.fastq_begin()                                                       # the store has copied: the ctx is free again
            T.fastq_add(fq(b"@1/1"), True)
            b.assemble(r_host, w, host_cands)
            want = b.fetch()
            b.assemble(r_dev, w, host_cands)
            assert_same_batch(b.fetch(), want)
            assert len(want[3]) == len(host_cands) > 100 and len(want[2]) > 4000
            host_records = gpu_ctx.align_batch(*want)
            # the whole front: text -> enumeration -> assembly -> upload -> DP
            T.parse_sam(sam_text)
            v = T.sam_view()
            with table.session() as s:
                ptr, n = text.enumerate_resident(s, v.alignments, v.n, cand.ORDER_FUSION)
                view = b.assemble_device(r_dev, w, ptr, n)
                gpu_ctx.upload_device(view)
                assert gpu_ctx.run() == len(host_records)
                assert gpu_ctx.download().tobytes() == host_records.tobytes() and len(host_records) > 100
        # a hand-made device record with len = -1 is named
        bad = host_recs[:20].copy()
        bad["len"][[11, 15]] = -1
        with DeviceArray(host_data) as dbytes, DeviceArray(bad) as drecs:
            with pytest.raises(bat.BatError) as e:
                text.reads_from_device(dbytes.ptr, len(host_data), drecs.ptr, len(bad))
            assert e.value.code == E_ARG and "read 11:" in str(e.value) and "length" in str(e.value)
        bad = host_recs[:20].copy()
        bad["off"][3] = len(host_data) - bad["len"][3] + 1                          # one byte beyond
        bad["fragment"][8] = -1
        with DeviceArray(host_data) as dbytes, DeviceArray(bad) as drecs:
            with pytest.raises(bat.BatError) as e:
                text.reads_from_device(dbytes.ptr, len(host_data), drecs.ptr, len(bad))
            assert "read 3:" in str(e.value) and "outside" in str(e.value)
            with text.reads_from_device(dbytes.ptr, len(host_data), drecs.ptr, 0) as empty:
                assert empty.handle
