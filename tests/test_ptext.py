"""splitreads.seq and splitreads.break printed on the GPU (include/defuse_ptext.h through defuse_amd/ptext.py).

Yardsticks: for "%g" this C library's snprintf (the host program below) and Python's "%g" % x, which agree with each other;
for the lines pred.Context.format_seq / format_break on the rows and bytes of pred_fetch, with the status rules of the header
applied around them by `host_texts` below; for the chains the golden files."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import abi

from tests.test_pred import Store, make_task, random_case, rec, records_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "tests", "golden", "smoke")
CONFIG1 = os.path.join(ROOT, "tests", "golden", "config1")
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
NO_SPLIT, HOST_STATS, NO_TASK, OUT_OF_WINDOW, HOST_SEQ = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def ptext(built):
    from defuse_amd import ptext as p
    return p


@pytest.fixture(scope="module")
def pred(built):
    from defuse_amd import pred as p
    return p


@pytest.fixture(scope="module")
def bat(built):
    from defuse_amd import bat as b
    return b


@pytest.fixture(scope="module")
def ectx(built):
    from defuse_amd import eval as ev
    ctx = ev.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------- the checker
def taken(x):
    """What the formatter takes: +-0 and 2^-64 <= |x| < 2^64."""
    return x == 0 or (math.isfinite(x) and 2.0 ** -64 <= abs(x) < 2.0 ** 64)


def host_texts(pred, res, seq, tasks):
    """Per result row (seq line, break lines, status) as bytes, bytes, int; `tasks` maps a fusion id to an object with
    ref_name and strand (the align strand).  A missing line is b""."""
    out = []
    for row in res:
        fid, st = int(row["fusion_id"]), int(row["status"])
        if st & (NO_TASK | OUT_OF_WINDOW):
            out.append((b"", b"", st))
            continue
        t = tasks[fid]
        if st & NO_SPLIT:
            s = ("%d\tN\t0\t0\t-1\t-1\n" % fid).encode()
            b = "".join("%d\t%d\t%s\t%s\t0\n" % (fid, ce, t.ref_name[ce], "+" if t.strand[ce] == 0 else "-") for ce in (0, 1)).encode("latin-1")
            out.append((s, b, st))
            continue
        b = pred.Context.format_break(row, t.ref_name, t.strand).encode("latin-1")
        if st & HOST_STATS or not taken(float(row["pos_avg"])) or not taken(float(row["min_avg"])):
            out.append((b"", b, st | HOST_SEQ))
        else:
            out.append((pred.Context.format_seq(row, seq).encode("latin-1"), b, st))
    return out


def check_texts(T, exp):
    """Both texts and the whole line table of a ptext.Context against host_texts' rows."""
    seq_text, brk_text, lines = T.fetch()
    assert seq_text == b"".join(e[0] for e in exp)
    assert brk_text == b"".join(e[1] for e in exp)
    assert len(lines) == len(exp)
    so = bo = 0
    L = {k: lines[k].tolist() for k in lines.dtype.names}
    for k, (s, b, st) in enumerate(exp):
        assert (L["seq_off"][k], L["seq_len"][k], L["brk_off"][k], L["brk_len"][k], L["status"][k], L["pad_"][k]) == (so, len(s), bo, len(b), st, 0), k
        so += len(s)
        bo += len(b)
    v, t = T.view(), T.timing()
    assert (v.seq_text_len, v.brk_text_len, v.n_lines) == (so, bo, len(exp)) == (t["seq_text_bytes"], t["brk_text_bytes"], t["n_groups"])
    assert v.seq_text and v.brk_text and v.lines
    return seq_text, brk_text, lines


def groups_of(ev, rows):
    """Host-supplied groups: rows of (fusion_id, first, second, count, pos_sum, min_sum, status)."""
    g = np.zeros(len(rows), dtype=ev.GROUP_DTYPE)
    for k, (fid, first, second, count, pos, mn, st) in enumerate(rows):
        g[k]["fusion_id"], g[k]["best_first"], g[k]["best_second"], g[k]["count"] = fid, first, second, count
        g[k]["pos_sum"], g[k]["min_sum"], g[k]["status"] = pos, mn, st
    return g


def g_values(n_random):
    """The values of the issue's list (the host program below walks the same list with two million random ones)."""
    rng = np.random.default_rng(17)
    xs = [0.0, -0.0, -1.0, 0.5, 1234565.0, 1234575.0, 123456.5, 999999.5, 99999.95, 9.999995, 0.9999995, 0.0001, 9.999995e-05, 2.5e-05,
          2.0 ** -64, 2.0 ** -63, 2.0 ** 31, float(np.nextafter(2.0 ** 64, 0.0)), -(2.0 ** -64), -float(np.nextafter(2.0 ** 64, 0.0))]
    xs += [k / n for n in range(1, 301) for k in range(n + 1)]
    sevens = (1000005 + 10 * rng.integers(0, 899999, 20000)).astype(np.float64)
    for f in (0.1, 1.0, 10.0, 1000.0):
        xs += (sevens * f).tolist()
    bits = (rng.integers(0, 2, n_random, dtype=np.uint64) << np.uint64(63)) | (rng.integers(1023 - 64, 1023 + 64, n_random, dtype=np.uint64) << np.uint64(52)) | \
        rng.integers(0, 2 ** 52, n_random, dtype=np.uint64)
    xs += bits.view(np.float64).tolist()
    declined = [float("nan"), -float("nan"), float("inf"), -float("inf"), 2.0 ** 64, 2.0 ** -65, float(np.nextafter(2.0 ** -64, 0.0)), 5e-324, -4.9e-310,
                1e300]
    return np.array(xs, dtype=np.float64), np.array(declined, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- without a GPU
def test_ptext_header_and_binding_agree(ptext):
    """sizeof and offsetof of every struct of the header, as g++ and gcc -std=c99 see them, against the ctypes structs and
    the numpy dtypes; PTEXT_HOST_SEQ; every declared function bound and exported."""
    sizes, n = abi.check("defuse_ptext.h", ptext, r"ptext_[a-z_]+", constants={"PTEXT_HOST_SEQ": ptext.HOST_SEQ},
                         dtypes=[(ptext.End, ptext.END_DTYPE), (ptext.Line, ptext.LINE_DTYPE)])
    assert ptext.HOST_SEQ == 16 and ptext.HOST_SEQ & (NO_SPLIT | HOST_STATS | NO_TASK | OUT_OF_WINDOW) == 0
    assert ptext.END_DTYPE.itemsize % 8 == 0 and ptext.LINE_DTYPE.itemsize % 8 == 0
    assert sizes == [16, 40, 56, 48] and n == 10


def test_ptext_argument_errors_need_no_device(ptext):
    lib = ptext.lib()
    err = lambda: lib.ptext_last_error().decode()
    h = ctypes.c_void_p()
    one = ctypes.c_void_p(1)           # stands for an object: the argument errors are found before any is looked at
    data = np.frombuffer(b"chr1chr22", dtype=np.uint8)

    def end(fid=5, ce=0, name=0, strand=0):
        return np.array([(fid, ce, name, strand)], dtype=ptext.END_DTYPE)

    def create(ends, off=(0, 4, 9), nbytes=len(data), n_names=None, n_ends=None, out=h, device=0):
        e = np.concatenate(ends) if ends else np.zeros(0, dtype=ptext.END_DTYPE)
        o = np.array(off, dtype=np.int64)
        return lib.ptext_names_create(device, data.ctypes.data if nbytes else None, nbytes, o.ctypes.data if len(o) else None,
                                      len(o) - 1 if n_names is None else n_names, e.ctypes.data if len(e) else None, len(e) if n_ends is None else n_ends,
                                      ctypes.byref(out) if out is not None else None)
    good = [end(), end(5, 1, 1, 1)]
    assert create(good, out=None) == E_ARG
    assert create(good, n_ends=-1) == E_ARG and "negative" in err()
    assert create(good, n_names=-1) == E_ARG and "negative" in err()
    assert create(good, nbytes=-1) == E_ARG and "negative" in err()
    assert create([], n_ends=1) == E_ARG and "null" in err()
    assert create(good, off=(), n_names=2) == E_ARG and "null" in err()
    assert create(good, n_names=2 ** 31) == E_LIMIT and create(good, n_ends=2 ** 31) == E_LIMIT
    assert create(good, off=(-1, 4, 9)) == E_ARG and "name 0" in err()                             # a negative name
    assert create(good, off=(0, 5, 4)) == E_ARG and "name 1" in err() and "reversed" in err()
    assert create(good, off=(0, 4, 10)) == E_ARG and "name 1" in err() and "outside" in err()      # one byte beyond
    assert create(good, off=(0, 4, 2 ** 62)) == E_ARG and "name 1" in err()
    assert create(good + [end(6, 2)]) == E_ARG and "end 2" in err() and "cluster_end" in err()
    assert create([end(5, -1)]) == E_ARG and "end 0" in err() and "cluster_end" in err()
    assert create(good + [end(6, 0, 0, 2)]) == E_ARG and "end 2" in err() and "strand" in err()   # a bad strand
    assert create([end(), end(5, 1, 0, -1)]) == E_ARG and "end 1" in err() and "strand" in err()
    assert create([end(), end(5, 1, 2, 0)]) == E_ARG and "end 1" in err() and "name 2" in err()   # a bad index
    assert create([end(5, 0, -1)]) == E_ARG and "end 0" in err() and "name -1" in err()
    assert create(good + [end(6), end(5, 1, 0, 0)]) == E_ARG and "ends 1 and 3" in err() and "fusion_id 5" in err()     # a doubled key
    assert create([end(-1), end(2 ** 31 - 1), end(-1)]) == E_ARG and "ends 0 and 2" in err() and "fusion_id -1" in err()
    assert create(good, device=999) == E_DEVICE and "999" in err()
    assert not h

    assert lib.ptext_create(0, None) == E_ARG
    assert lib.ptext_create(999, ctypes.byref(h)) == E_DEVICE and "999" in err() and not h
    assert lib.ptext_create(-1, ctypes.byref(h)) == E_DEVICE and not h
    assert lib.ptext_format(None, one, one) == E_ARG and "no ctx" in err()
    assert lib.ptext_format(one, None, one) == E_ARG and "no pred ctx" in err()
    view, timing = ptext.View(), ptext.PtextTiming()
    assert lib.ptext_view(None, ctypes.byref(view)) == E_ARG and lib.ptext_get_timing(None, ctypes.byref(timing)) == E_ARG
    assert lib.ptext_fetch(None, None, 0, None, 0, None, 0) == E_ARG
    lib.ptext_destroy(None)
    lib.ptext_names_destroy(None)
    x, out, ln, total = np.array([1.5, 2.5]), np.zeros(64, np.uint8), np.zeros(2, np.int32), ctypes.c_int64(-1)
    fd = lambda n=2, cap=64, xp=x.ctypes.data, op=out.ctypes.data, lp=ln.ctypes.data, tp=ctypes.byref(total), device=0: \
        lib.ptext_format_doubles(device, xp, n, op, cap, lp, tp)
    assert fd(tp=None) == E_ARG
    assert fd(n=-1) == E_ARG and "negative" in err() and total.value == 0
    assert fd(cap=-1) == E_ARG and "negative" in err()
    assert fd(xp=None) == E_ARG and fd(lp=None) == E_ARG and fd(op=None) == E_ARG and "null" in err()
    assert fd(n=2 ** 30) == E_LIMIT
    assert fd(device=999) == E_DEVICE and "999" in err()
    assert not out.any() and not ln.any()
    # good arguments get as far as the device: no CPU path
    rc = lib.ptext_create(0, ctypes.byref(h))
    assert rc in (0, E_DEVICE)
    if rc == 0:
        view.n_lines = -1
        assert lib.ptext_format(h, one, None) == E_ARG and "no names" in err()
        assert lib.ptext_view(h, ctypes.byref(view)) == 0 and (view.n_lines, view.seq_text_len, view.brk_text_len) == (0, 0, 0)
        assert lib.ptext_view(h, None) == E_ARG
        assert lib.ptext_fetch(h, None, -1, None, 0, None, 0) == E_ARG and lib.ptext_fetch(h, None, 1, None, 0, None, 0) == E_ARG
        assert lib.ptext_fetch(h, None, 0, None, 0, None, 0) == 0
        lib.ptext_destroy(h)
    else:
        assert not h and "device" in err()


GCHECK = r'''
#include "@ROOT@/defuse_amd/csrc/ptext_shared.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
// The formatter of ptext_shared.hpp against this C library's snprintf("%g"), and its line writers against snprintf too.
// Prints the number of values compared; exit status 1 and the first mismatches on any difference.
static long long n_checked = 0, n_bad = 0;
static void same(double x)
{
    char want[64], got[PTEXT_G_MAX];                       // exactly the promised room: a longer text is an overflow
    const int nw = snprintf(want, sizeof want, "%g", x);
    const ptext_g g = ptext_g_of(x);
    const int len = ptext_g_length(g);
    const int ng = len >= 1 && len <= PTEXT_G_MAX ? ptext_g_write(g, got) : -1;
    ++n_checked;
    if (ng != nw || ng != len || memcmp(want, got, (size_t)nw) != 0) {
        if (++n_bad <= 20) printf("MISMATCH %a: want %s, got %.*s (length %d, promised %d)\n", x, want, ng > 0 ? ng : 0, got, ng, len);
    }
}
static void is(double x, const char* text)
{
    char want[64];
    snprintf(want, sizeof want, "%g", x);
    if (strcmp(want, text) != 0) {
        printf("this C library prints %a as %s, not %s\n", x, want, text);
        ++n_bad;
    }
    same(x);
}
static void declined(double x)
{
    const ptext_g g = ptext_g_of(x);
    char buf[PTEXT_G_MAX];
    ++n_checked;
    if (g.ok || ptext_g_length(g) != 0 || ptext_g_write(g, buf) != 0) {
        printf("NOT DECLINED %a\n", x);
        ++n_bad;
    }
}
static void lines(int32_t fid, int32_t status, long long count, double pos, double mn, int32_t b0, int32_t b1, const std::string& name)
{
    pred_result r{};
    r.fusion_id = fid; r.status = status; r.seq_len = 5; r.count = count; r.pos_avg = pos; r.min_avg = mn; r.break_pos[0] = b0; r.break_pos[1] = b1;
    const bool ns = status & EVAL_NO_SPLIT;
    char want[1024];
    const ptext_seq_parts s = ptext_seq_parts_of(r);
    int nw = snprintf(want, sizeof want, "\t0\t%lld\t%g\t%g\n", ns ? 0ll : count, ns ? -1.0 : pos, ns ? -1.0 : mn);
    std::vector<char> tail((size_t)s.tail);
    char head[12];
    ++n_checked;
    if (!s.ok || s.tail != nw || ptext_write_seq_tail(s, tail.data()) != nw || memcmp(want, tail.data(), (size_t)nw) != 0 || s.body != (ns ? 1 : 5) ||
        s.head != snprintf(want, sizeof want, "%d\t", fid) || rec_write_field(fid, head) != s.head || memcmp(want, head, (size_t)s.head) != 0) {
        printf("SEQ LINE of fusion %d\n", fid);
        ++n_bad;
    }
    for (int end = 0; end < 2; ++end) {
        nw = snprintf(want, sizeof want, "%d\t%d\t%s\t%c\t%d\n", fid, end, name.c_str(), end ? '-' : '+', ns ? 0 : (end ? b1 : b0));
        std::vector<char> line((size_t)ptext_break_length(r, end, (int32_t)name.size()));
        ++n_checked;
        if ((int)line.size() != nw || ptext_write_break(r, end, name.data(), (int32_t)name.size(), end, line.data()) != nw || memcmp(want, line.data(), (size_t)nw) != 0) {
            printf("BREAK LINE %d of fusion %d\n", end, fid);
            ++n_bad;
        }
    }
}
static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()                                      // splitmix64
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
int main(int argc, char** argv)
{
    const long long n_random = argc > 1 ? atoll(argv[1]) : 2000000;
    is(0.0, "0"); is(-0.0, "-0"); is(-1.0, "-1"); is(0.5, "0.5");
    is(1234565.0, "1.23456e+06"); is(1234575.0, "1.23458e+06"); is(123456.5, "123456");
    is(999999.5, "1e+06"); is(99999.95, "99999.9"); is(9.999995, "10"); is(0.9999995, "1");
    is(0.0001, "0.0001"); is(9.999995e-05, "0.0001"); is(2.5e-05, "2.5e-05");
    same(ldexp(1.0, -64)); same(ldexp(1.0, -63)); same(ldexp(1.0, 31)); same(nextafter(ldexp(1.0, 64), 0.0));
    same(-ldexp(1.0, -64)); same(-nextafter(ldexp(1.0, 64), 0.0));
    for (int n = 1; n <= 300; ++n)
        for (int k = 0; k <= n; ++k) same((double)k / (double)n);
    for (int k = 0; k < 20000; ++k) {
        const double v = (double)(1000005 + 10 * (long long)(rnd() % 899999));      // seven digits, the last a 5
        same(v * 0.1); same(v); same(v * 10.0); same(v * 1000.0);
    }
    for (long long k = 0; k < n_random; ++k) {
        const uint64_t r = rnd(), mant = rnd() & ((1ull << 52) - 1u);
        const uint64_t e2 = (uint64_t)(1023 - 64) + r % 128u;                       // 2^-64 <= |x| < 2^64
        const uint64_t bits = ((r >> 63) << 63) | (e2 << 52) | mant;
        double x;
        memcpy(&x, &bits, sizeof x);
        same(x);
    }
    declined(std::numeric_limits<double>::quiet_NaN()); declined(-std::numeric_limits<double>::quiet_NaN());
    declined(std::numeric_limits<double>::infinity()); declined(-std::numeric_limits<double>::infinity());
    declined(ldexp(1.0, 64)); declined(ldexp(1.0, -65)); declined(nextafter(ldexp(1.0, -64), 0.0));
    declined(std::numeric_limits<double>::denorm_min()); declined(-4.9e-310); declined(1e300);
    lines(7, 0, 3, 1.0 / 3.0, 0.25, 999, 5046, "chr1");
    lines(-2147483647 - 1, 0, 9223372036854775807ll, 1234565.0, 2.5e-05, -2147483647 - 1, 2147483647, "");
    lines(2147483647, EVAL_NO_SPLIT, 5, 0.0, 0.0, 17, 18, std::string(300, '|'));
    lines(12345, 0, 4294967296ll, 0.0, 0.5, 0, -1, "GL000|1.1");
    lines(0, 0, 9999999999ll, 0.5, 0.5, 10, 9, "X");
    lines(-5, 0, -10000000000ll, 0.5, 0.5, 10, 9, "X");
    printf("%lld values, %lld bad\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
'''


def test_formatter_as_a_host_program(tmp_path):
    """ptext_shared.hpp compiled as a stand-alone host program, plain and under ASan + UBSan, and run as a program: every
    value of the issue's list prints as snprintf("%g") prints it, the ties and the notation switch as spelled out there,
    and NaN, the infinities, 2^64, 2^-65 and denormals are declined."""
    from tests.test_sanitizers import BAD, ENV
    src = tmp_path / "gcheck.hip"
    src.write_text(GCHECK.replace("@ROOT@", ROOT))
    base = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17"]
    subprocess.check_call(base + ["-O1", "-o", str(tmp_path / "gcheck"), str(src)])
    subprocess.check_call(base + ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                                  "-Xarch_host", "-fno-omit-frame-pointer", "-o", str(tmp_path / "gcheck_asan"), str(src)])
    for exe, env in (("gcheck", {}), ("gcheck_asan", ENV["asan"])):
        r = subprocess.run([str(tmp_path / exe)], capture_output=True, text=True, env=dict(os.environ, LC_ALL="C", **env), stdin=subprocess.DEVNULL, timeout=600)
        assert not any(b in r.stderr for b in BAD), r.stderr[-3000:]
        assert r.returncode == 0, (exe, r.returncode, r.stdout[-3000:], r.stderr[-2000:])
        n = 20 + sum(n + 1 for n in range(1, 301)) + 80000 + 2000000 + 10 + 6 * 3
        assert r.stdout.splitlines()[-1] == "%d values, 0 bad" % n


# ---------------------------------------------------------------------------------------------- GPU: the formatter
@pytest.mark.gpu
def test_format_doubles_against_python(ptext):
    xs, declined = g_values(100000)
    assert all(taken(x) for x in xs.tolist()) and not any(taken(x) for x in declined.tolist())
    both = np.concatenate((xs[:5000], declined, xs[5000:], declined))          # declined ones among the others, and last
    want = [("%g" % x).encode() if taken(x) else b"" for x in both.tolist()]
    got = ptext.format_doubles(both)
    bad = [(k, both[k], want[k], got[k]) for k in range(len(both)) if got[k] != want[k]]
    assert not bad, bad[:10]
    assert ptext.format_doubles(np.zeros(0)) == []
    assert ptext.format_doubles(declined) == [b""] * len(declined)
    # the capacity protocol: nothing written, the size reported, a second call with room succeeds
    total = sum(len(w) for w in want[:1000])
    with pytest.raises(ptext.PtextError) as e:
        ptext.format_doubles(both[:1000], cap=total - 1)
    assert (e.value.code, e.value.bytes) == (E_CAPACITY, total)
    assert ptext.format_doubles(both[:1000], cap=total) == want[:1000]


# ---------------------------------------------------------------------------------------------- GPU: the lines
EDGE_NAMES = [b"", b"|", b"c|r", b"chr|", b"ch|r1", b"|" + b"x" * 298 + b"|"]
EDGE_FIDS = [7, 42, 123, 1234, 12345, 123456, 1234567, 12345678, 123456789, 2147483647, -12]
EDGE_COUNTS = [7, 42, 123, 1234, 12345, 123456, 1234567, 12345678, 123456789, 9876543210]


def edge_tasks():
    tasks = []
    for k, fid in enumerate(EDGE_FIDS):
        t = make_task(fid, b"ACGTN", b"acgtnacg", start=(1000 * k + 1, 77 + k), strand=(k % 2, 0),
                      name=(EDGE_NAMES[k % 6].decode(), EDGE_NAMES[(k + 1) % 6].decode()))
        t.strand = [(k // 2) % 2, (k + 1) % 2]                  # the align strand is not the sequence's
        tasks.append(t)
    return tasks


@pytest.mark.gpu
def test_word_edges_of_both_texts(bat, pred, ptext):
    """Sequences of 2-12 bytes behind fusion ids of 1-10 digits, counts of 1-10 digits and averages of every length, the
    groups shuffled: every sequence begins and ends at every byte phase of the .seq text; names of 0, 1, 3, 4, 5 and 300
    bytes.  One stray or missing byte at a seam breaks the equality of a whole text."""
    from defuse_amd import eval as ev
    rng = np.random.default_rng(23)
    tasks = edge_tasks()
    rows = []
    for fid in EDGE_FIDS:
        for length in range(2, 13):
            for rep in range(6):
                first = int(rng.integers(max(0, length - 8), min(5, length - 2) + 1))          # length = first + 1 + tail, tail 1..7
                tail = length - 1 - first
                count = EDGE_COUNTS[len(rows) % 10]
                avg = (0.0, 0.5, 1.0 / 3.0, 2.5e-05, 123456.5, 1234565.0, 17.0)[len(rows) % 7]
                rows.append((fid, first, 8 - tail - 1, count, avg * count, rng.random() * count, 0))
    order = rng.permutation(len(rows))
    groups = groups_of(ev, [rows[i] for i in order])
    with Store(bat, pred, tasks) as P, ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T:
        P.predict(groups)
        res, seq = P.fetch()
        assert (res["status"] == 0).all() and sorted(set(res["seq_len"].tolist())) == list(range(2, 13))
        T.format(P.ctx)
        exp = host_texts(pred, res, seq, P.oracle_tasks)
        seq_text, brk_text, lines = check_texts(T, exp)
        begins, ends = {}, {}
        for row, line in zip(res, lines):
            head = len("%d\t" % row["fusion_id"])
            begins.setdefault(int(row["seq_len"]), set()).add((int(line["seq_off"]) + head) % 4)
            ends.setdefault(int(row["seq_len"]), set()).add((int(line["seq_off"]) + head + int(row["seq_len"])) % 4)
        assert all(begins[n] == {0, 1, 2, 3} == ends[n] for n in range(2, 13)), (begins, ends)
        assert {len(str(c)) for c in res["count"].tolist()} == set(range(1, 11))
        assert b"\t9876543210\t" in seq_text and b"\n7\t0\t\t" in brk_text and b"\n7\t1\t|\t" in brk_text and (b"\t|" + b"x" * 298 + b"|\t") in brk_text
        assert T.timing()["gather_bytes"] == int(res["seq_len"].sum())


KINDS = ("plain", "no_split", "no_task", "out_of_window", "host_stats", "nan", "big")


def kind_row(kind, fid):
    """A host-supplied group of each kind on a task of edge_tasks (windows of 5 and 8 bases)."""
    return {"plain": (fid, 2, 3, 3, 1.0, 2.0, 0), "no_split": (fid, 0, 0, 5, 0.0, 0.0, NO_SPLIT), "no_task": (555, 1, 1, 2, 1.0, 1.0, 0),
            "out_of_window": (fid, 6, 1, 2, 1.0, 1.0, 0), "host_stats": (fid, 1, 1, 2, 0.0, 0.0, HOST_STATS), "nan": (fid, 3, 0, 1, float("nan"), 0.5, 0),
            "big": (fid, 0, 6, 1, 0.25, 2.0 ** 70, 0)}[kind]


@pytest.mark.gpu
def test_status_rules(bat, pred, ptext):
    """One group of each kind in every order of two neighbours; a group without lines first and last."""
    from defuse_amd import eval as ev
    tasks = edge_tasks()
    kinds = ["no_task"] + [k for a in KINDS for b in KINDS for k in (a, b)] + ["out_of_window"]
    pairs = set(zip(kinds, kinds[1:]))
    assert pairs == {(a, b) for a in KINDS for b in KINDS}
    groups = groups_of(ev, [kind_row(kind, EDGE_FIDS[k % len(EDGE_FIDS)]) for k, kind in enumerate(kinds)])
    want_status = {"plain": 0, "no_split": NO_SPLIT, "no_task": NO_TASK, "out_of_window": OUT_OF_WINDOW, "host_stats": HOST_STATS | HOST_SEQ,
                   "nan": HOST_SEQ, "big": HOST_SEQ}
    with Store(bat, pred, tasks) as P, ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T:
        P.predict(groups)
        res, seq = P.fetch()
        T.format(P.ctx)
        exp = host_texts(pred, res, seq, P.oracle_tasks)
        assert [e[2] for e in exp] == [want_status[k] for k in kinds]
        for kind, (s, b, _) in zip(kinds, exp):
            assert bool(s) == (kind in ("plain", "no_split")) and bool(b) == (kind not in ("no_task", "out_of_window")), kind
        seq_text, brk_text, lines = check_texts(T, exp)
        k = kinds.index("no_split")
        fid = int(res["fusion_id"][k])
        assert exp[k][0] == b"%d\tN\t0\t0\t-1\t-1\n" % fid and exp[k][1].count(b"\t0\n") == 2
        assert lines["seq_len"][0] == 0 == lines["brk_len"][0] and lines["seq_len"][-1] == 0 == lines["brk_len"][-1]
        assert lines["seq_off"][-1] == len(seq_text) and lines["brk_off"][-1] == len(brk_text)
        # a caller splices its own line in at seq_off of a PTEXT_HOST_SEQ row
        k = kinds.index("nan")
        assert lines["status"][k] == HOST_SEQ and lines["seq_len"][k] == 0 and lines["brk_len"][k] > 0
        assert seq_text[:int(lines["seq_off"][k])] == b"".join(e[0] for e in exp[:k])


@pytest.mark.gpu
def test_names(bat, pred, ptext):
    from defuse_amd import eval as ev
    tasks = edge_tasks()
    name_bytes, name_off, ends = ptext.pack_names(tasks)

    def refused(e, *words):
        with pytest.raises(ptext.PtextError) as err:
            ptext.Names(name_bytes, name_off, e)
        assert err.value.code == E_ARG and all(w in str(err.value) for w in words), str(err.value)
    e = ends.copy()
    e[5] = e[2]
    refused(e, "ends 2 and 5", "fusion_id %d" % ends[2]["fusion_id"])                  # a doubled key
    e = ends.copy()
    e[3]["name"] = len(name_off) - 1
    refused(e, "end 3", "name %d" % (len(name_off) - 1))                               # an index outside the table
    e = ends.copy()
    e[4]["strand"] = 2
    refused(e, "end 4", "strand 2")
    # the ends in any order give the same texts; a group whose end has no entry is refused by its number
    groups = groups_of(ev, [kind_row("no_task", 0), kind_row("plain", EDGE_FIDS[0]), kind_row("out_of_window", EDGE_FIDS[3]), kind_row("plain", EDGE_FIDS[3]),
                            kind_row("no_split", EDGE_FIDS[3]), kind_row("plain", EDGE_FIDS[5])])
    missing = np.array([x for x in ends[::-1] if not (x["fusion_id"] == EDGE_FIDS[3] and x["cluster_end"] == 1) and x["fusion_id"] != EDGE_FIDS[5]])
    with Store(bat, pred, tasks) as P, ptext.Names(name_bytes, name_off, ends[::-1]) as N, ptext.Names(name_bytes, name_off, missing) as M, \
            ptext.Names(name_bytes, name_off, ends[:0]) as none, ptext.Context(N) as T:
        P.predict(groups)
        res, seq = P.fetch()
        T.format(P.ctx)
        exp = host_texts(pred, res, seq, P.oracle_tasks)
        check_texts(T, exp)
        with pytest.raises(ptext.PtextError) as err:
            T.format(P.ctx, names=M)
        assert err.value.code == E_ARG and "group 3" in str(err.value) and "cluster end 1" in str(err.value) and "fusion_id %d" % EDGE_FIDS[3] in str(err.value)
        v = T.view()
        assert (v.n_lines, v.seq_text_len, v.brk_text_len) == (0, 0, 0) and T.fetch()[0] == b"" and T.fetch()[1] == b""
        with pytest.raises(ptext.PtextError) as err:
            T.format(P.ctx, names=none)
        assert err.value.code == E_ARG and "group 1" in str(err.value) and "cluster end 0" in str(err.value)
        T.format(P.ctx)
        check_texts(T, exp)
        P.predict(groups[[0, 2]])                                                      # no group needs a name
        T.format(P.ctx, names=none)
        check_texts(T, [(b"", b"", NO_TASK), (b"", b"", OUT_OF_WINDOW)])


def random_names(tasks, seed):
    rng = np.random.default_rng(seed)
    pool = ["chr%d" % k for k in range(1, 23)] + ["X", "GL000192.1", "ENST|1|x"]
    for t in tasks:
        t.ref_name = [pool[int(rng.integers(0, len(pool)))] for _ in (0, 1)]
        t.strand = [int(rng.integers(0, 2)) for _ in (0, 1)]
    return tasks


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_against_the_host(bat, pred, ptext, ectx, seed):
    tasks, records = random_case(seed)
    random_names(tasks, seed)
    gaps = np.random.default_rng(seed).integers(0, 4, 2 * len(tasks)).tolist()
    with Store(bat, pred, tasks, gaps) as P, ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T:
        groups, _ = ectx.evaluate(records)
        P.predict(groups)
        res, seq = P.fetch()
        T.format(P.ctx)
        exp = host_texts(pred, res, seq, P.oracle_tasks)
        status = [e[2] for e in exp]
        assert len(exp) == 2060 and status.count(0) > 1000 and sum(1 for s in status if s & NO_TASK) == 60
        assert status.count(OUT_OF_WINDOW) > 20 and status.count(NO_SPLIT) > 20 and status.count(HOST_STATS | HOST_SEQ) > 3
        seq_text, brk_text, _ = check_texts(T, exp)
        assert len(seq_text) > 500000 and brk_text.count(b"\n") == 2 * sum(1 for e in exp if e[1])
        # the same through the resident entry
        from tests.test_batch_assembly import DeviceArray
        with DeviceArray(records) as dev:
            ectx.evaluate_device(dev.ptr, len(records))
        P.predict_resident(ectx)
        T.format(P.ctx)
        assert T.fetch()[0] == seq_text and T.fetch()[1] == brk_text


@pytest.mark.gpu
def test_context_reuse_and_capacities(bat, pred, ptext, ectx):
    from defuse_amd import eval as ev
    tasks, records = random_case(4, n_tasks=300)
    random_names(tasks, 4)
    fid = records["fusion_id"]
    heads = np.flatnonzero(np.concatenate(([True], fid[1:] != fid[:-1])))
    cut = lambda a, b: records[heads[a]:heads[b]]
    with Store(bat, pred, tasks) as P, ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T:
        # format before any prediction
        with pytest.raises(ptext.PtextError) as err:
            T.format(P.ctx)
        assert err.value.code == E_ARG and "completed prediction" in str(err.value)
        # growing, then shrinking, then nothing: nothing of an earlier call may show
        for part in (cut(0, 20), cut(0, 359), cut(100, 103), records[:0], cut(5, 6)):
            groups, _ = ectx.evaluate(part)
            P.predict(groups)
            T.format(P.ctx)
            check_texts(T, host_texts(pred, *P.fetch(), P.oracle_tasks))
        groups, _ = ectx.evaluate(cut(0, 50))
        P.predict(groups)
        T.format(P.ctx)
        seq_text, brk_text, lines = T.fetch()
        assert len(seq_text) > 0 and len(brk_text) > 0
        # the capacity protocol of ptext_fetch: nothing is written when one of the three does not fit
        lib, h = T._lib, T.handle
        s2, b2, l2 = np.full(len(seq_text), 7, np.uint8), np.full(len(brk_text), 7, np.uint8), np.zeros(len(lines), ptext.LINE_DTYPE)
        fetch = lambda sc, bc, lc: lib.ptext_fetch(h, s2.ctypes.data, sc, b2.ctypes.data, bc, l2.ctypes.data, lc)
        assert fetch(len(s2) - 1, len(b2), len(l2)) == E_CAPACITY
        msg = lib.ptext_last_error().decode()
        assert str(len(s2)) in msg and str(len(b2)) in msg and str(len(l2)) in msg
        assert fetch(len(s2), len(b2) - 1, len(l2)) == E_CAPACITY and fetch(len(s2), len(b2), len(l2) - 1) == E_CAPACITY
        assert lib.ptext_fetch(h, None, 0, None, 0, None, 0) == E_CAPACITY
        assert (s2 == 7).all() and (b2 == 7).all() and not l2.view(np.uint8).any()
        assert lib.ptext_fetch(h, None, len(s2), b2.ctypes.data, len(b2), l2.ctypes.data, len(l2)) == E_ARG
        assert fetch(len(s2), len(b2), len(l2)) == 0
        assert s2.tobytes() == seq_text and b2.tobytes() == brk_text and l2.tobytes() == lines.tobytes() and T.timing()["download_ms"] > 0
        # format after a failed prediction: the pred ctx has none, and the texts are empty
        with ev.Context(0) as fresh:
            with pytest.raises(pred.PredError):
                P.predict_resident(fresh)
        with pytest.raises(ptext.PtextError) as err:
            T.format(P.ctx)
        assert err.value.code == E_ARG and "completed prediction" in str(err.value)
        v = T.view()
        assert (v.n_lines, v.seq_text_len, v.brk_text_len) == (0, 0, 0) and lib.ptext_fetch(h, None, 0, None, 0, None, 0) == 0
        P.predict(groups[:0])                                                # a completed prediction of nothing
        assert T.format(P.ctx).n_lines == 0
        P.predict(groups)
        T.format(P.ctx)
        assert T.fetch()[0] == seq_text and T.fetch()[1] == brk_text


@pytest.mark.gpu
def test_text_offsets_are_formed_in_64_bits(bat, pred, ptext):
    """The shape of test_pred's 64-bit test: 300 groups on one task with a window of 2^24 bases, 5.03e9 bytes of .seq text.
    The line that lies across byte 2^32 and the last one are read back from the device alone."""
    from defuse_amd import eval as ev
    from tests.test_batch_assembly import from_device
    n0, n_groups = 2 ** 24, 300
    rng = np.random.default_rng(3)
    w0 = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n0)].tobytes()
    t = make_task(5, w0, b"acgtn", b"NN", b"n.", name=("chr|7", "chrX"))
    t.strand = [1, 0]
    groups = np.zeros(n_groups, dtype=ev.GROUP_DTYPE)
    groups["fusion_id"], groups["best_first"], groups["best_second"], groups["count"] = 5, n0, 1, 3
    groups["pos_sum"], groups["min_sum"] = 1.0, 2.0
    want = b"5\t" + b"NN" + w0 + b"|gtnn." + b"\t0\t3\t0.333333\t0.666667\n"
    with Store(bat, pred, [t]) as P, ptext.Names.from_oracle([t]) as N, ptext.Context(N) as T:
        try:
            P.predict(groups)
            v = T.format(P.ctx)
        except (pred.PredError, ptext.PtextError) as e:
            if not (e.code == E_DEVICE and "memory" in str(e).lower()):
                raise
            pytest.skip("the device refused the memory of %d text bytes: %s" % (n_groups * len(want), e))
        assert v.n_lines == n_groups and v.seq_text_len == n_groups * len(want) > 2 ** 32
        tm = T.timing()
        print("%d .seq bytes: lengths %.2f ms, write %.2f ms, gather %.1f ms" % (v.seq_text_len, tm["lengths_ms"], tm["write_ms"], tm["gather_ms"]))
        lines = from_device(v.lines, n_groups, ptext.LINE_DTYPE)
        assert lines["seq_off"].tolist() == [k * len(want) for k in range(n_groups)] and lines["seq_off"][-1] > 2 ** 32
        assert (lines["seq_len"] == len(want)).all() and (lines["status"] == 0).all()
        brk = b"5\t0\tchr|7\t-\t%d\n5\t1\tchrX\t+\t%d\n" % (100 + n0 - 1, 200 + 2)
        assert lines["brk_off"].tolist() == [k * len(brk) for k in range(n_groups)] and (lines["brk_len"] == len(brk)).all()
        across = 2 ** 32 // len(want)
        assert lines["seq_off"][across] < 2 ** 32 < lines["seq_off"][across] + len(want)
        for k in (n_groups - 1, across, 0):
            got = from_device(v.seq_text + int(lines["seq_off"][k]), len(want), np.uint8)
            assert got.tobytes() == want, k
        assert from_device(v.brk_text, v.brk_text_len, np.uint8).tobytes() == brk * n_groups
        assert tm["gather_bytes"] == n_groups * (n0 + 8)


# ---------------------------------------------------------------------------------------------- GPU: the chains
@pytest.mark.gpu
def test_smoke_vector_through_the_whole_resident_chain(bat, pred, ptext, gpu_ctx, ectx):
    """test_pred's chain, one link longer: SAM records up, the bytes of splitreads.break down."""
    from defuse_amd import cand
    from oracle import dosplitalign_oracle as ora
    from tests.test_batch_assembly import DeviceArray
    d = SMOKE + "/"
    tasks = ora.create_tasks(d + "ref.fa", d + "exons.txt", 300, 30, 50, 50, ora.read_align_region_pairs(d + "regions.txt"))
    reads = {}
    ora.read_fastq(d + "reads.1.fastq", reads)
    ora.read_fastq(d + "reads.2.fastq", reads)
    names, regs = {}, []
    for t in tasks.values():
        for ce in (0, 1):
            for loc in t.mate_regions[ce]:
                regs.append((names.setdefault(loc["refName"], len(names)), loc["strand"], loc["start"], loc["end"], cand.cluster_id(t.fusion_id, ce)))
    als = cand.alignments([(names.get(rname, -1), strand, start, end, ora.lexical_cast_int(frag), rend)
                           for frag, rend, rname, strand, start, end in ora.sam_alignments(d + "improper.sam")])
    windows = {t.fusion_id: (t.seq[0], t.seq[1]) for t in tasks.values()}
    with cand.Table(cand.regions(regs)) as table, bat.Reads.from_dict(reads) as r, bat.Windows.from_dict(windows) as w, bat.Batch() as b, \
            pred.Tasks.from_oracle(w, tasks) as ptasks, pred.Context(ptasks) as P, table.session() as s, \
            ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T:
        ptr, n = s.enumerate_device(als, cand.ORDER_FUSION)
        gpu_ctx.upload_device(b.assemble_device(r, w, ptr, n))
        n_rec = gpu_ctx.run()
        with DeviceArray(np.zeros(n_rec, dtype=np.dtype("V40"))) as dev:
            assert gpu_ctx.records_to_device(dev.ptr, n_rec) == n_rec
            groups, _ = ectx.evaluate_device(dev.ptr, n_rec)
        P.predict_resident(ectx)
        T.format(P)
        seq_text, brk_text, lines = T.fetch()
        assert len(lines) == len(groups) == len(tasks) and (lines["status"] == 0).all()
        assert brk_text.decode() == open(d + "expected.break.txt").read()
        res, seq = P.fetch()
        assert seq_text == "".join(P.format_seq(row, seq) for row in res).encode("latin-1")


@pytest.mark.gpu
def test_config1_derived_chain_prints_all_three_files(bat, pred, ptext, ectx, tmp_path):
    """The records in a rec_store, the kept list of eval_groups_device, the prediction and its text: splitreads.seq,
    splitreads.break and splitreads.predalign of one run all come from the device."""
    from defuse_amd import rec as recmod
    from oracle import dosplitalign_oracle as ora
    from tests import config1_case
    case = config1_case.build(str(tmp_path / "case"))
    tasks = ora.create_tasks(case["fasta"], case["exons"], case["ufrag"], case["sfrag"], case["minread"], case["maxread"],
                             ora.read_align_region_pairs(case["regions_derived"]))
    rows = [tuple(int(x) for x in l.split()) for l in open(os.path.join(CONFIG1, "expected.derived.align.txt"))]
    rows.sort(key=lambda r: r[0])                                               # stable, by fusion id: the tool's input
    records = records_of([r + (0,) for r in rows])
    windows = {t.fusion_id: (t.seq[0], t.seq[1]) for t in tasks.values()}
    with bat.Windows.from_dict(windows) as w, pred.Tasks.from_oracle(w, tasks) as ptasks, pred.Context(ptasks) as P, recmod.Store(0) as store, \
            ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T:
        store.append(records)
        ptr, n = store.records_device()
        groups, kept = ectx.evaluate_device(ptr, n)
        P.predict_resident(ectx)
        T.format(P)
        seq_text, brk_text, lines = T.fetch()
        assert len(lines) == len(groups) > 0 and (lines["status"] == 0).all()
        assert seq_text.decode() == open(os.path.join(CONFIG1, "expected.derived.seq.txt")).read()
        assert brk_text.decode() == open(os.path.join(CONFIG1, "expected.derived.break.txt")).read()
        assert store.text(kept).decode() == open(os.path.join(CONFIG1, "expected.derived.predalign.txt")).read()
