"""splitreads.span.stats on the GPU (the "span statistics" section of include/defuse_ptext.h through defuse_amd/spanstats.py),
`defuse_glue calc_span_stats` and `defuse_glue span_stats`.

Yardstick: tests/spanstats_oracle.py, a restatement of the header's rules on bytes.  Without a GPU it is pinned to the
reference's Perl script (tests/golden/span/, compared order-free) and, byte for byte, to the host step of bin/defuse_glue on
every case; span_shared.hpp gives the oracle's per-line results and Python's "%.15g" in a host program under ASan + UBSan.  On
the GPU the result structs, the rows (the mean by its bits) and the text of every case equal the oracle's, the tables made from
a prediction equal the tables made from its printed texts, and the tool writes the host step's file.

SPAN_SUM_LIMIT needs |sum| > 2^53 with every term inside 2^30: more than six million cluster lines.  No case here reaches it
through the library; its bound is checked on span_shared.hpp's span_sum_ok in the host program."""
import ctypes
import math
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import abi
from tests import clusterregions_oracle as cora
from tests import spanstats_oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "span")
TOOL = os.path.join(ROOT, "bin", "defuse_glue")
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
BLOCK = 256                       # threads per workgroup of every span kernel (txt_shared.hpp's BLOCK)
INT_MIN, INT_MAX = ora.INT_MIN, ora.INT_MAX
FIXTURES = ("example", "random1", "random2")


@pytest.fixture(scope="module")
def sp(built):
    from defuse_amd import spanstats
    return spanstats


@pytest.fixture(scope="module")
def cr(built):
    from defuse_amd import clusterregions
    return clusterregions


@pytest.fixture(scope="module")
def glue(built):
    from defuse_amd import build
    build.build_tools()
    return TOOL


def golden(name, kind):
    return open(os.path.join(GOLDEN, "%s_%s.txt" % (name, kind)), "rb").read()


# ---------------------------------------------------------------------------------------------- cases
def _b(x):
    return x if isinstance(x, bytes) else b"%d" % x


def cl(cid, ce, frag, strand, start, end, *more, name=b"chr1", re=0):
    return b"\t".join(_b(c) for c in (cid, ce, frag, re, name, strand, start, end) + more) + b"\n"


def br(cid, ce, pos, *more, name=b"chr1", strand=b"+"):
    return b"\t".join(_b(c) for c in (cid, ce, name, strand, pos) + more) + b"\n"


def sq(cid, inter=0, *more, seq=b"ACGTACGT"):
    return b"\t".join(_b(c) for c in (cid, seq, inter) + more) + b"\n"


def simple(cid, n_frags=1, base=1000, inter=0):
    """A cluster of n_frags fragments with both ends, a plus end 0 and a minus end 1, its two breaks and its .seq line."""
    lines = b"".join(cl(cid, 0, f, b"+", base + f * f % 97, base + f + 49) + cl(cid, 1, f, b"-", 5 * base + 3 * f, 5 * base + 3 * f + 49) for f in range(n_frags))
    return lines, br(cid, 0, base + 70) + br(cid, 1, 5 * base - 20, strand=b"-"), sq(cid, inter)


def join(*parts):
    return tuple(b"".join(p[k] for p in parts) for k in range(3))


EXAMPLE = (cl(5, 0, 10, b"+", 100, 149) + cl(5, 1, 10, b"-", 300, 349) + cl(5, 0, 11, b"+", 90, 139) + cl(5, 0, 12, b"-", 95, 144) + cl(5, 1, 12, b"-", 310, 359),
           br(5, 0, 160) + br(5, 1, 290, strand=b"-"), sq(5, 0, 3, b"0.5", b"0.25"))
GROUPS = ["values", "keys", "sizes", "line stops", "id stops"]


def cases():
    """[dict(name, group, clusters, brk, seq)]"""
    C = []
    group = "values"

    def add(name, files):
        C.append(dict(name=name, group=group, clusters=files[0], brk=files[1], seq=files[2]))

    add("empty", (b"", b"", b""))
    add("example", EXAMPLE)
    add("no_newline", tuple(t[:-1] for t in join(simple(3, 2), EXAMPLE)))
    add("cr_strand", (cl(1, 0, 1, b"+\r", 100, 149) + cl(1, 1, 1, b"-", 300, 349), br(1, 0, 160) + br(1, 1, 290), sq(1)))
    add("five_e_minus_5", (cl(7, 0, 0, b"+", 1000, 1049) + b"".join(cl(7, 0, f, b"+", 1001, 1050) for f in range(1, 19999)) + cl(7, 1, 19999, b"-", 1900, 2000),
                           br(7, 0, 1000) + br(7, 1, 2001), sq(7)))
    add("negative_mean", (cl(3, 0, 1, b"+", 14, 60) + cl(3, 1, 2, b"+", 10, 60), br(3, 0, 10) + br(3, 1, 5), sq(3)))
    add("thirds_and_inter", join(simple(1, 3, inter=7), simple(2, 7, base=333, inter=-2), simple(4, 1, inter=40)))
    add("unused_position_is_garbage", (cl(6, 0, 1, b"+", 100, b"junk") + cl(6, 1, 1, b"-", b"", 349) + cl(6, 0, 2, b"+", 90, b"1e2") + cl(6, 1, 2, b"-", b" 7", 300),
                                       br(6, 0, 160) + br(6, 1, 290), sq(6)))
    add("more_fields", (cl(6, 0, 1, b"+", 100, 149, b"x", b"", b"12x") + cl(6, 1, 1, b"-", 300, 349, b""), br(6, 0, 160, b"more", b"") + br(6, 1, 290, b""),
                        sq(6, 0, b"", seq=b"A" * 5000)))
    group = "keys"
    add("int_extremes", join(simple(5), simple(INT_MAX, 2), simple(-1, 3), simple(INT_MIN, 2), simple(0)))
    add("id_without_break", (simple(3, 2)[0] + cl(8, 0, 1, b"?", b"x", b"y") + cl(-8, 4, 1, b"+", b"", b"") + simple(9)[0], simple(3)[1], simple(3)[2]))
    add("ends_0_2", (cl(2, 0, 1, b"+", 100, 149) + cl(2, 2, 1, b"-", 300, 349) + cl(2, 2, 2, b"-", 310, 359), br(2, 0, 160) + br(2, 2, 290) + br(2, 1, 5), sq(2)))
    add("negative_end_and_fragment", (cl(2, -1, -7, b"+", 100, 149) + cl(2, INT_MAX, -7, b"-", 300, 349) + cl(2, -1, INT_MIN, b"+", 90, 139) + cl(2, -1, INT_MAX, b"+", 95, 144),
                                      br(2, -1, 160) + br(2, INT_MAX, 290), sq(2)))
    add("duplicates_everywhere", (cl(4, 0, 1, b"+", 100, 149) + cl(4, 1, 1, b"-", 300, 349) + cl(4, 0, 1, b"+", 120, 169) + cl(4, 1, 2, b"+", 280, 350) + cl(4, 1, 1, b"-", 300, 351),
                                  br(4, 0, 999) + br(4, 1, 290) + br(4, 0, 160), sq(4, 50, seq=b"C" * 3000) + sq(4, 3) + sq(9, 1)))
    add("id_comes_back", (simple(4, 3)[0] + simple(1, 2)[0] + cl(4, 0, 7, b"-", 1, 1100) + cl(4, 1, 0, b"+", 4000, 1), simple(4)[1] + simple(1)[1], simple(4)[2] + simple(1)[2]))
    add("three_spellings", (cl(b"7", 0, 1, b"+", 100, 149) + cl(b"+7", 1, b"01", b"-", 300, 349) + cl(b"007", b"+0", b"1", b"+", 90, 139) + cl(7, b"-0", 2, b"+", 95, 144),
                            br(b"07", 0, 160) + br(7, b"+1", 290), sq(b"+7", b"-0")))
    group = "sizes"
    big = simple(5000, 600)
    for n in (BLOCK - 1, BLOCK, BLOCK + 1):
        # n one-line clusters without a break in front: the big cluster begins at element n of both sorted orders, and is id n
        add("big_cluster_at_%d" % n, (b"".join(cl(k, 0, 1, b"+", 1, 2) for k in range(n)) + big[0] + simple(6000, 2)[0], big[1] + simple(6000)[1], big[2] + simple(6000)[2]))
    for n in (BLOCK // 2 - 1, BLOCK // 2, BLOCK // 2 + 1):
        add("big_cluster_behind_%d_rows" % n, join(*[simple(k, 1, base=1000 + k) for k in range(n)], big, simple(6000, 2)))
    add("many_one_fragment_clusters", join(*[simple(k, 1, base=100 + 7 * k, inter=k % 3) for k in range(-700, 800)]))
    group = "line stops"
    good = join(simple(3, 3), simple(8, 2))
    for name, line in (("few", b"5\t0\t1\t0\tc\t+\t7\n"), ("empty_line", b"\n"), ("int0", cl(b"5x", 0, 1, b"+", 1, 2)), ("int1", cl(5, b"", 1, b"+", 1, 2)),
                       ("int2", cl(5, 0, b"1e2", b"+", 1, 2))):
        add("clusters_%s_first" % name, (line + good[0], good[1], good[2]))
        add("clusters_%s_last_no_newline" % name, (good[0] + line[:-1] if line != b"\n" else good[0] + b"\n\n", good[1], good[2]))
    for name, line in (("few", b"5\t0\tchr1\t+\n"), ("int0", br(b"", 0, 5)), ("int1", br(5, b" 1", 5)), ("int4", br(5, 0, b"12\r"))):
        add("break_%s" % name, (good[0], good[1] + line + br(3, 0, 1), good[2]))
    for name, line in (("few", b"5\tACGT\n"), ("int0", sq(b"5.0")), ("int2", sq(5, b"2147483648"))):
        add("seq_%s" % name, (good[0], good[1], line + good[2]))
    add("break_and_seq_stop", (good[0], good[1] + b"x\n", b"y\n" + good[2]))
    add("two_line_stops", (good[0] + cl(5, 0, b"", b"+", 1, 2) + b"\n", good[1], good[2]))
    add("line_stop_beats_id_stop", (cl(1, 0, 1, b"+", 1, 2) + good[0] + cl(9, b"x", 1, b"+", 1, 2), br(1, 0, 5) + good[1], good[2]))
    group = "id stops"
    add("one_end", join(good, (cl(9, 0, 1, b"+", 10, 59) + cl(9, 0, 2, b"+", 20, 69), br(9, 0, 100), sq(9))))
    add("three_ends", join((cl(2, 0, 1, b"+", 10, 59) + cl(2, 1, 1, b"+", 10, 59) + cl(2, 2, 1, b"+", 10, 59), br(2, 0, 100) + br(2, 1, 100) + br(2, 2, 100), sq(2)), good))
    add("no_break_end", join(good, (cl(9, 0, 1, b"+", 10, 59) + cl(9, 1, 1, b"+", 20, 69), br(9, 0, 100), sq(9))))
    add("bad_start", join(good, (cl(9, 0, 1, b"+", b"10.5", 59) + cl(9, 1, 1, b"+", 20, 69), br(9, 0, 100) + br(9, 1, 100), sq(9))))
    add("bad_end_and_start", join(good, (cl(9, 0, 1, b"-", 10, b"") + cl(9, 1, 1, b"+", b"x", 69), br(9, 0, 100) + br(9, 1, 100), sq(9))))
    add("bad_end", join(good, (cl(9, 0, 1, b"-", 10, b"59 ") + cl(9, 1, 1, b"+", 20, 69), br(9, 0, 100) + br(9, 1, 100), sq(9))))
    lim = ora.MAX_COORD
    add("coord_break", join(good, (cl(9, 0, 1, b"+", 10, 59) + cl(9, 1, 1, b"+", 20, 69), br(9, 0, lim + 1) + br(9, 1, 100), sq(9))))
    add("coord_position", join(good, (cl(9, 0, 1, b"+", 10, 59) + cl(9, 1, 1, b"-", 20, -lim - 1), br(9, 0, 100) + br(9, 1, 100), sq(9))))
    add("coord_inter", join(good, (cl(9, 0, 1, b"+", 10, 59) + cl(9, 1, 1, b"+", 20, 69), br(9, 0, 100) + br(9, 1, 100), sq(9, lim + 1))))
    add("coord_at_the_limit", join(good, (cl(9, 0, 1, b"+", -lim, 59) + cl(9, 1, 1, b"-", 20, lim), br(9, 0, lim) + br(9, 1, -lim), sq(9, -lim))))
    add("no_inter", join(good, (cl(9, 0, 1, b"+", 10, 59) + cl(9, 1, 1, b"+", 20, 69), br(9, 0, 100) + br(9, 1, 100), b"")))
    add("all_causes_in_one_id", (cl(9, 0, 1, b"+", b"x", 59) + cl(9, 1, 1, b"+", lim + 5, 69) + cl(9, 2, 1, b"+", 20, 69), br(9, 0, 100) + br(9, 1, 100), b""))
    add("break_end_before_integer", (cl(9, 0, 1, b"+", b"x", 59) + cl(9, 1, 1, b"+", lim + 5, 69), br(9, 0, 100), b""))
    add("integer_before_coord", (cl(9, 0, 1, b"+", b"x", 59) + cl(9, 1, 1, b"+", lim + 5, 69), br(9, 0, 100) + br(9, 1, 100), b""))
    add("coord_before_inter", (cl(9, 0, 1, b"+", 10, 59) + cl(9, 1, 1, b"+", lim + 5, 69), br(9, 0, 100) + br(9, 1, 100), b""))
    add("lowest_id_of_two", join((cl(9, 0, 1, b"+", 10, 59), br(9, 0, 100), sq(9)), good, (cl(-4, 0, 1, b"+", 10, 59) + cl(-4, 1, 1, b"+", 20, 69), br(-4, 0, 1) + br(-4, 1, 1), b"")))
    assert len({c["name"] for c in C}) == len(C) and {c["group"] for c in C} == set(GROUPS)
    assert all(len(c["clusters"]) < 600000 for c in C)
    return C


def random_files(seed, n_clusters=60):
    """Clusters of 1-20 fragments: one-end fragments, a (fragment, end) given again, strands that change inside an end, ids that
    come back, ids without a break entry, doubled lines in the two small files, inter lengths other than 0."""
    rng = random.Random(seed)
    ids = rng.sample(range(-20, 300), n_clusters)
    blocks, late, brk, seq = [], [], [], []
    for k, cid in enumerate(ids):
        base = [rng.randrange(-500, 90000), rng.randrange(1000, 90000)]
        strands = [rng.choice([b"+", b"-"]), rng.choice([b"+", b"-"])]
        lines = [cl(cid, 0, 5000, strands[0], base[0], base[0] + 49), cl(cid, 1, 5000, strands[1], base[1], base[1] + 49)]
        for frag in rng.sample(range(-50, 1000), rng.randrange(0, 20)):
            for e in (0, 1):
                if rng.random() < 0.1:
                    continue
                a = base[e] + rng.randrange(300)
                lines.append(cl(cid, e, frag, strands[e] if rng.random() < 0.9 else rng.choice([b"+", b"-", b""]), a, a + rng.randrange(30, 76), re=e))
                if rng.random() < 0.1:
                    lines.append(cl(cid, e, frag, rng.choice([b"+", b"-"]), a + 3, a + 60, name=b"chr7"))
        rng.shuffle(lines)
        half = len(lines) // 2 if k % 5 == 0 else len(lines)
        blocks.append(b"".join(lines[:half]))
        if half < len(lines):
            late.append(b"".join(lines[half:]))
        if k % 7 != 3:
            for e in (0, 1):
                if rng.random() < 0.2:
                    brk.append(br(cid, e, rng.randrange(1000, 90000), name=b"chr9"))
                brk.append(br(cid, e, base[e] + rng.randrange(-100, 400), strand=strands[e] or b"+"))
        if rng.random() < 0.2:
            seq.append(sq(cid, 7, seq=b"NNNN"))
        seq.append(sq(cid, 0 if k % 4 else rng.randrange(-5, 40), 3, b"0.5", seq=bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(20, 300)))))
    rng.shuffle(late)
    return b"".join(blocks + late), b"".join(brk), b"".join(seq)


def expect(case):
    """The oracle on a case: (tables result, tables, stats result, rows, text); the last three None where the tables stopped."""
    tres, tabs = ora.tables(case["brk"], case["seq"])
    if tabs is None:
        return tres, None, None, None, None
    return (tres, tabs) + ora.stats(case["clusters"], tabs)


def same_result(got, want):
    return all(got[k] == v for k, v in want.items() if v is not None) and set(got) == set(want)


# ---------------------------------------------------------------------------------------------- without a GPU
def test_header_and_binding_agree(sp):
    sizes, n = abi.check("defuse_ptext.h", sp, r"span_[a-z_]+", constants=sp.CONSTANTS, dtypes=[(sp.Row, sp.ROW_DTYPE)])
    assert sizes == [96, 40, 40, 48] and n == 10 == len(sp.EXPORTS) == len(sp.PROTOTYPES)
    assert (sp.FEW_FIELDS, sp.BAD_INTEGER, sp.NOT_TWO_ENDS, sp.NO_BREAK_END, sp.COORD_LIMIT, sp.NO_INTER, sp.SUM_LIMIT) == \
        (ora.FEW_FIELDS, ora.BAD_INTEGER, ora.NOT_TWO_ENDS, ora.NO_BREAK_END, ora.COORD_LIMIT, ora.NO_INTER, ora.SUM_LIMIT)
    assert (sp.FILE_CLUSTERS, sp.FILE_BREAKS, sp.FILE_SEQS) == (ora.FILE_CLUSTERS, ora.FILE_BREAKS, ora.FILE_SEQS)
    from defuse_amd import ptext
    assert not set(sp.EXPORTS) & set(ptext.EXPORTS) and len(ptext.EXPORTS) == 10


def test_argument_errors_need_no_device(sp):
    lib = sp.lib()
    err = lambda: lib.span_last_error().decode()
    h, one = ctypes.c_void_p(), ctypes.c_void_p(1)          # `one` stands for an object: argument errors come before it is looked at
    res = sp.SpanResult()
    text = np.frombuffer(b"abc", dtype=np.uint8)
    p = text.ctypes.data
    assert lib.span_create(0, None) == E_ARG and "no output" in err()
    assert lib.span_create(999, ctypes.byref(h)) == E_DEVICE and not h and "device" in err()
    assert lib.span_breaks_text(one, p, 3, p, 3, None) == E_ARG and "no result" in err()
    res.stop_field = 5
    assert lib.span_breaks_text(one, p, -1, p, 3, ctypes.byref(res)) == E_ARG and "negative" in err() and res.stop_field == -1
    assert lib.span_breaks_text(one, p, 3, p, -1, ctypes.byref(res)) == E_ARG and "negative" in err()
    assert lib.span_breaks_text(one, p, 2 ** 31, p, 3, ctypes.byref(res)) == E_LIMIT and "2^31 - 1" in err()
    assert lib.span_breaks_text(one, p, 3, p, 2 ** 31, ctypes.byref(res)) == E_LIMIT
    assert lib.span_breaks_text(one, None, 3, p, 3, ctypes.byref(res)) == E_ARG and "null pointer" in err()
    assert lib.span_breaks_text(one, p, 3, None, 3, ctypes.byref(res)) == E_ARG and "null pointer" in err()
    assert lib.span_breaks_text(None, p, 3, p, 3, ctypes.byref(res)) == E_ARG and "no ctx" in err()
    assert lib.span_breaks_pred(one, one, None) == E_ARG and "no result" in err()
    assert lib.span_breaks_pred(None, one, ctypes.byref(res)) == E_ARG and "no ctx" in err()
    assert lib.span_breaks_pred(one, None, ctypes.byref(res)) == E_ARG and "no pred ctx" in err()
    assert lib.span_stats(one, one, sp.INPUT, None) == E_ARG and "no result" in err()
    for source in (-1, 2, 7):
        assert lib.span_stats(one, one, source, ctypes.byref(res)) == E_ARG and "source" in err()
    assert lib.span_stats(None, one, sp.DEDUP, ctypes.byref(res)) == E_ARG and "no ctx" in err()
    assert lib.span_stats(one, None, sp.INPUT, ctypes.byref(res)) == E_ARG and "no cluster ctx" in err()
    view, timing = sp.View(), sp.SpanTiming()
    assert lib.span_view(None, ctypes.byref(view)) == E_ARG and lib.span_view(one, None) == E_ARG
    assert lib.span_fetch(None, None, 0, None, 0) == E_ARG and "no ctx" in err()
    assert lib.span_fetch(one, None, -1, None, 0) == E_ARG and "negative" in err()
    assert lib.span_fetch(one, None, 1, None, 0) == E_ARG and lib.span_fetch(one, None, 0, None, 1) == E_ARG and "without a buffer" in err()
    assert lib.span_get_timing(None, ctypes.byref(timing)) == E_ARG and lib.span_get_timing(one, None) == E_ARG
    lib.span_destroy(None)
    x, out, ln, total = np.array([1.5, 2.5]), np.zeros(64, np.uint8), np.zeros(2, np.int32), ctypes.c_int64(-1)
    fd = lambda n=2, cap=64, xp=x.ctypes.data, op=out.ctypes.data, lp=ln.ctypes.data, tp=ctypes.byref(total), device=0: \
        lib.span_format_doubles(device, xp, n, op, cap, lp, tp)
    assert fd(tp=None) == E_ARG
    assert fd(n=-1) == E_ARG and "negative" in err() and total.value == 0
    assert fd(cap=-1) == E_ARG and fd(xp=None) == E_ARG and fd(lp=None) == E_ARG and fd(op=None) == E_ARG and "null" in err()
    assert fd(n=2 ** 30) == E_LIMIT and fd(device=999) == E_DEVICE and "999" in err()
    assert not out.any() and not ln.any()


def rows_of(text):
    return sorted(text.splitlines())


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_agrees_with_the_perl_script(name):
    """Order-free: the script prints in hash order.  The fixtures' key fields are all plain decimal."""
    res, text = ora.run(golden(name, "clusters"), golden(name, "break"), golden(name, "seq"))
    perl = golden(name, "stats.perl")
    assert res["stop_kind"] == 0 and res["n_noncanonical"] == 0 and rows_of(text) == rows_of(perl) and len(perl) == res["out_bytes"] > 0
    ids = [int(l.split(b"\t")[0]) for l in text.splitlines()]
    assert ids == sorted(ids) and res["n_rows"] == len(ids)
    assert (name != "example") or text == b"5\t28.3333333333333\t3\n"
    assert (name == "example") or (res["n_rows"] < res["n_ids"] and any(b"." in l for l in text.splitlines()))


def test_oracle_stops_where_the_perl_script_dies():
    res, text = ora.run(golden("one_end", "clusters"), golden("one_end", "break"), golden("one_end", "seq"))
    assert text is None and (res["stop_kind"], res["stop_value"], res["stop_line"]) == (ora.NOT_TWO_ENDS, 9, 0)
    assert golden("one_end", "stderr.perl") == b"Error: Did not find 2 reference names for cluster 9\n" and int(golden("one_end", "status.perl")) != 0


def test_the_cases_reach_their_edges():
    """On the oracle alone: what the cases are named for."""
    C = {c["name"]: c for c in cases()}
    got = {n: expect(c) for n, c in C.items()}
    text = lambda n: got[n][4]
    rows = lambda n: got[n][3]
    stop = lambda n: (lambda r: (r["stop_file"], r["stop_line"], r["stop_kind"], r["stop_field"], r["stop_value"]))(got[n][2] if got[n][2] is not None else got[n][0])
    assert text("empty") == b"" and got["empty"][2]["n_rows"] == 0 and got["empty"][2]["out_bytes"] == 0
    # a one-end fragment (11), a strand taken from another fragment's line (end 0 is a minus end by fragment 12's line)
    assert text("example") == b"5\t28.3333333333333\t3\n" and rows("example") == [(5, 3, 85, 85 / 3)]
    assert text("no_newline") == text("example")[:0] + ora.stats(C["no_newline"]["clusters"] + b"\n", got["no_newline"][1])[2] and text("no_newline").endswith(text("example"))
    assert not any(c.endswith(b"\n") for c in (C["no_newline"]["clusters"], C["no_newline"]["brk"], C["no_newline"]["seq"]))
    assert text("cr_strand") == b"1\t50\t1\n"                                    # "+\r" is not "+": 149 - 160 + 1 + 349 - 290 + 1
    assert text("five_e_minus_5") == b"7\t5e-05\t20000\n" and rows("five_e_minus_5")[0][2] == 1
    assert text("negative_mean") == b"3\t-3.5\t2\n"
    assert text("thirds_and_inter").startswith(b"1\t149.333333333333\t3\n")       # fifteen significant digits
    assert got["thirds_and_inter"][1][1] == {1: 7, 2: -2, 4: 40}
    assert got["unused_position_is_garbage"][2]["stop_kind"] == 0 and len(rows("unused_position_is_garbage")) == 1
    assert got["more_fields"][2]["stop_kind"] == 0 and text("more_fields") == b"6\t121\t1\n"
    assert [r[0] for r in rows("int_extremes")] == [INT_MIN, -1, 0, 5, INT_MAX] and text("int_extremes").startswith(b"-2147483648\t")
    # an id without a break entry, malformed or not, and a negative id
    assert [r[0] for r in rows("id_without_break")] == [3] and got["id_without_break"][2]["n_ids"] == 4
    assert [r[0] for r in rows("ends_0_2")] == [2] and rows("ends_0_2")[0][1] == 2
    assert rows("negative_end_and_fragment")[0][1] == 3
    d = got["duplicates_everywhere"]
    assert d[0]["n_lines"] == 3 and d[0]["n_breaks"] == 2 and d[0]["n_seq_lines"] == 3 and d[0]["n_inters"] == 2 and d[1][0][(4, 0)] == 160 and d[1][1][4] == 3
    assert rows("duplicates_everywhere") == [(4, 2, (160 - 120 + 1) + (351 - 290 + 1) + 3 + (350 - 290 + 1) + 3, 85.0)]
    assert [r[0] for r in rows("id_comes_back")] == [1, 4] and rows("id_comes_back")[1][1] == 4
    t = got["three_spellings"]
    assert t[0]["n_noncanonical"] == 3 and t[2]["n_noncanonical"] == 5 and [r[:2] for r in rows("three_spellings")] == [(7, 2)]
    for n in (BLOCK - 1, BLOCK, BLOCK + 1):
        c = C["big_cluster_at_%d" % n]
        keys = sorted((int(l.split(b"\t")[0]), int(l.split(b"\t")[1])) for l in c["clusters"].splitlines())
        assert keys.index((5000, 0)) == n and [r[:2] for r in rows("big_cluster_at_%d" % n)] == [(5000, 600), (6000, 2)] and got["big_cluster_at_%d" % n][2]["n_ids"] == n + 2
    for n in (BLOCK // 2 - 1, BLOCK // 2, BLOCK // 2 + 1):
        assert len(rows("big_cluster_behind_%d_rows" % n)) == n + 2 and rows("big_cluster_behind_%d_rows" % n)[n][:2] == (5000, 600)
    assert len(rows("many_one_fragment_clusters")) == 1500 and C["many_one_fragment_clusters"]["clusters"].count(b"\n") == 3000
    F, B, I = ora.FEW_FIELDS, ora.BAD_INTEGER, -1
    n_good = 10
    for name, (kind, field) in {"few": (F, I), "empty_line": (F, I), "int0": (B, 0), "int1": (B, 1), "int2": (B, 2)}.items():
        assert stop("clusters_%s_first" % name) == (ora.FILE_CLUSTERS, 1, kind, field, 0), name
        assert stop("clusters_%s_last_no_newline" % name) == (ora.FILE_CLUSTERS, n_good + 1, kind, field, 0), name
    for name, (kind, field) in {"few": (F, I), "int0": (B, 0), "int1": (B, 1), "int4": (B, 4)}.items():
        assert stop("break_%s" % name) == (ora.FILE_BREAKS, 5, kind, field, 0) and got["break_%s" % name][1] is None, name
    for name, (kind, field) in {"few": (F, I), "int0": (B, 0), "int2": (B, 2)}.items():
        assert stop("seq_%s" % name) == (ora.FILE_SEQS, 1, kind, field, 0), name
    assert stop("break_and_seq_stop") == (ora.FILE_BREAKS, 5, F, I, 0)
    assert stop("two_line_stops") == (ora.FILE_CLUSTERS, n_good + 1, B, 2, 0)
    assert stop("line_stop_beats_id_stop") == (ora.FILE_CLUSTERS, n_good + 2, B, 1, 0)
    ID = lambda kind, cid=9, field=-1: (ora.FILE_CLUSTERS, 0, kind, field, cid)
    assert stop("one_end") == ID(ora.NOT_TWO_ENDS) and stop("three_ends") == ID(ora.NOT_TWO_ENDS, 2)
    assert stop("no_break_end") == ID(ora.NO_BREAK_END)
    assert stop("bad_start") == ID(B, field=6) and stop("bad_end") == ID(B, field=7) and stop("bad_end_and_start") == ID(B, field=6)
    assert stop("coord_break") == stop("coord_position") == stop("coord_inter") == ID(ora.COORD_LIMIT)
    assert got["coord_at_the_limit"][2]["stop_kind"] == 0 and rows("coord_at_the_limit")[-1] == (9, 1, 4 * ora.MAX_COORD + 2 - ora.MAX_COORD, float(3 * ora.MAX_COORD + 2))
    assert stop("no_inter") == ID(ora.NO_INTER)
    assert stop("all_causes_in_one_id") == ID(ora.NOT_TWO_ENDS) and stop("break_end_before_integer") == ID(ora.NO_BREAK_END)
    assert stop("integer_before_coord") == ID(B, field=6) and stop("coord_before_inter") == ID(ora.COORD_LIMIT)
    assert stop("lowest_id_of_two") == ID(ora.NO_INTER, -4)
    kinds = {stop(n)[2] for n in C}
    assert kinds == {0, F, B, ora.NOT_TWO_ENDS, ora.NO_BREAK_END, ora.COORD_LIMIT, ora.NO_INTER}     # (SUM_LIMIT: see the head of the file)
    for seed in (1, 2, 3):
        cl_, b_, s_ = random_files(seed)
        res, tabs = ora.tables(b_, s_)
        res2, rws, _ = ora.stats(cl_, tabs)
        assert res["n_breaks"] < res["n_lines"] and res["n_inters"] < res["n_seq_lines"] and 0 < res2["n_rows"] < res2["n_ids"] and res2["n_noncanonical"] == 0
        assert 900 < res2["n_lines"] < 3000 and any(r[3] != int(r[3]) for r in rws)


def all_files():
    out = [(c["name"], c["clusters"], c["brk"], c["seq"]) for c in cases()]
    out += [(n, golden(n, "clusters"), golden(n, "break"), golden(n, "seq")) for n in FIXTURES + ("one_end",)]
    return out + [("random_%d" % s,) + random_files(s) for s in (1, 2, 3)]


def write_files(tmp_path, clusters, brk, seq):
    paths = [tmp_path / "clusters.txt", tmp_path / "break.txt", tmp_path / "seq.txt"]
    for p, data in zip(paths, (clusters, brk, seq)):
        p.write_bytes(data)
    return ["-c", str(paths[0]), "-b", str(paths[1]), "-s", str(paths[2])]


def test_oracle_is_the_host_step(glue, tmp_path):
    """bin/defuse_glue calc_span_stats on every case, the fixtures and three random texts: the oracle's bytes where it does not
    stop; where it does, status 1, nothing on stdout, one line on stderr, and Perl's own words for a cluster without two ends."""
    n_stops = 0
    for name, clusters, brk, seq in all_files():
        res, text = ora.run(clusters, brk, seq)
        r = subprocess.run([glue, "calc_span_stats"] + write_files(tmp_path, clusters, brk, seq), capture_output=True, timeout=120)
        if text is None:
            n_stops += 1
            assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"Error: ") and r.stderr.count(b"\n") == 1, (name, r.stderr)
            if res["stop_kind"] == ora.NOT_TWO_ENDS:
                assert r.stderr == b"Error: Did not find 2 reference names for cluster %d\n" % res["stop_value"], name
            elif res["stop_line"]:
                which = ("clusters.txt", "break.txt", "seq.txt")[res["stop_file"]]
                assert ("/%s line %d: " % (which, res["stop_line"])).encode() in r.stderr, (name, r.stderr)
            else:
                assert b"/clusters.txt cluster %d: " % res["stop_value"] in r.stderr, (name, r.stderr)
        else:
            assert r.returncode == 0 and r.stdout == text and r.stderr == b"", (name, r.stderr)
    assert n_stops >= 35
    r = subprocess.run([glue, "calc_span_stats"] + write_files(tmp_path, *[golden("one_end", k) for k in ("clusters", "break", "seq")]), capture_output=True)
    assert r.stderr == golden("one_end", "stderr.perl") and r.stdout == b""
    # the long options, the binary's own name, the usage
    args = write_files(tmp_path, *EXAMPLE)
    link = tmp_path / "calc_span_stats.pl"
    os.symlink(glue, link)
    long_args = ["--clusters", args[1], "--breaks", args[3], "--seqs", args[5]]
    for cmd in ([glue, "calc_span_stats"] + long_args, [str(link)] + args):
        assert subprocess.run(cmd, capture_output=True, check=True).stdout == b"5\t28.3333333333333\t3\n"
    for bad in ([], args[:4], args + ["-x", "y"], args[:5]):
        r = subprocess.run([glue, "calc_span_stats"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("Usage: calc_span_stats") and r.stdout == ""
    usage = subprocess.run([glue], capture_output=True, text=True).stderr
    assert "calc_span_stats" in usage and "span_stats [args]" in usage


def g15_values():
    """(taken, declined): the doubles of the issue's list."""
    rng = np.random.default_rng(29)
    n = 4000
    bits = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) | (rng.integers(1023 - 64, 1023 + 64, n, dtype=np.uint64) << np.uint64(52)) | \
        rng.integers(0, 2 ** 52, n, dtype=np.uint64)
    xs = bits.view(np.float64).tolist()
    xs += [k / 3 for k in range(-40, 200)] + [k / 7 for k in range(-40, 200)] + [1 / 20000, 0.0, -0.0, 85 / 3, 50.0, -3.5, 1e15, 1e-5, 123456789012345.0, 0.0001, 0.00001234]
    xs += [1000000000000005.0, 1000000000000015.0, 100000000000000.5, 100000000000001.5, 999999999999999.5, 2.0 ** 53, -(2.0 ** 53), 2.0 ** -31, 2.0 ** -64,
           float(np.nextafter(2.0 ** 64, 0.0)), 999999999999999.4, 99999999999999.95, 9.999999999999995, 0.9999999999999995]
    declined = [float("nan"), float("inf"), -float("inf"), 5e-324, 2.2e-308 / 4, 2.0 ** 64, -(2.0 ** 64), 2.0 ** -65, 1e300]
    return xs, declined


def taken(x):
    return x == 0 or (math.isfinite(x) and 2.0 ** -64 <= abs(x) < 2.0 ** 64)


def test_g15_values_are_what_the_issue_lists():
    xs, declined = g15_values()
    assert all(taken(x) for x in xs) and not any(taken(x) for x in declined) and len(xs) > 4400
    fmt = lambda x: "%.15g" % x
    assert [fmt(x) for x in (1 / 3, 85 / 3, 1 / 20000, 50.0, -3.5, 1e15)] == ["0.333333333333333", "28.3333333333333", "5e-05", "50", "-3.5", "1e+15"]
    assert fmt(1000000000000005.0) == "1e+15" and fmt(1000000000000015.0) == "1.00000000000002e+15" and fmt(-0.0) == "-0"
    assert max(len(fmt(x)) for x in xs) == 21


HOST = r'''
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "%(root)s/tools_src/defuse_host.hpp"
#include "%(root)s/defuse_amd/csrc/span_shared.hpp"
struct HostInt {
    bool operator()(const uint8_t* p, int64_t n, int& v) const { return n >= 0 && defuse::field_int(reinterpret_cast<const char*>(p), (size_t)n, v); }
};
struct Tabs {
    const std::vector<int64_t>* at;
    int64_t operator()(int64_t k) const { return (*at)[(size_t)k]; }      // (.at would hide a read beyond the line's tabs from ASan, so: the heap vector)
};
static std::string slurp(const char* name)
{
    std::ifstream in(name, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string mode = argv[1], data = slurp(argv[2]);
    if (mode == "g") {                                      // one double per line as 16 hex digits: its text, or "-" where declined
        for (size_t s = 0; s + 16 <= data.size(); s += 17) {
            const uint64_t bits = strtoull(data.substr(s, 16).c_str(), nullptr, 16);
            double x;
            memcpy(&x, &bits, sizeof x);
            const span_g g = span_g_of(x);
            const int len = span_g_length(g);
            if (len < 0 || len > SPAN_G_MAX) return 3;
            std::vector<char> buf((size_t)len);             // exactly the promised room: a longer text is an overflow
            if (span_g_write(g, buf.data()) != len) return 4;
            printf("%%s\n", len ? std::string(buf.data(), (size_t)len).c_str() : "-");
        }
        // the rows, the term and the bounds
        const long long two53 = 1ll << 53;
        if (!span_sum_ok(two53) || !span_sum_ok(-two53) || span_sum_ok(two53 + 1) || span_sum_ok(-two53 - 1) || !span_sum_ok(0)) return 5;
        if (!span_coord_ok(TASK_MAX_COORD) || !span_coord_ok(-TASK_MAX_COORD) || span_coord_ok(TASK_MAX_COORD + 1) || span_coord_ok(-TASK_MAX_COORD - 1)) return 6;
        if (span_term(true, 160, 100) != 61 || span_term(false, 160, 144) != -15 || span_term(true, -TASK_MAX_COORD, TASK_MAX_COORD) != -2ll * TASK_MAX_COORD + 1) return 7;
        const int kinds[] = {SPAN_NOT_TWO_ENDS, SPAN_NO_BREAK_END, SPAN_BAD_INTEGER, SPAN_COORD_LIMIT, SPAN_NO_INTER, SPAN_SUM_LIMIT};
        for (int k = 0; k < 6; ++k)
            if (span_stop_rank(kinds[k]) != k + 1 || span_stop_kind(k + 1) != kinds[k]) return 8;
        const struct { int32_t id; long long sum, count; } rows[] = {{5, 85, 3}, {-2147483647 - 1, -7, 2}, {2147483647, two53, 2147483647}, {0, 0, 1}, {7, 1, 20000}};
        for (const auto& r : rows) {
            char want[96];
            const double mean = span_mean(r.sum, r.count);
            const int nw = snprintf(want, sizeof want, "%%d\t%%.15g\t%%lld\n", r.id, mean, r.count);
            const span_g g = span_g_of(mean);
            std::vector<uint8_t> line((size_t)span_row_length(r.id, g, r.count));
            if ((int)line.size() != nw || span_row_write(r.id, g, r.count, line.data()) != nw || memcmp(want, line.data(), (size_t)nw) != 0) return 9;
        }
        return 0;
    }
    int64_t s = 0;
    while (s < (int64_t)data.size()) {
        int64_t e = s;
        while (e < (int64_t)data.size() && data[(size_t)e] != '\n') ++e;
        // an exact copy of the line on the heap: a read beyond it is a report
        std::vector<uint8_t> line(data.begin() + s, data.begin() + e);
        const int64_t n = (int64_t)line.size();
        if (mode == "c") {
            const taskc_line r = taskc_parse_line(line.data(), 0, n, HostInt());
            int field = -1;
            const int kind = span_cluster_stop(r, field);
            int32_t nc = 0, v6 = 0, v7 = 0, f6 = 0, f7 = 0;
            int plus = 0, ok6 = 0, ok7 = 0;
            if (!kind) {
                nc = span_cluster_noncanonical(line.data(), 0, n, HostInt());
                plus = span_is_plus(r, line.data(), 0);
                ok6 = span_position(line.data(), 0, n, r, true, HostInt(), v6, f6);
                ok7 = span_position(line.data(), 0, n, r, false, HostInt(), v7, f7);
                if (f6 != 6 || f7 != 7) return 10;
            }
            printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", kind, field, r.id, r.ce, r.frag, nc, plus, ok6, v6, ok7, v7);
        } else {
            std::vector<int64_t> tabs;
            for (int64_t p = 0; p < n; ++p)
                if (line[(size_t)p] == '\t') tabs.push_back(p);
            const Tabs at{&tabs};
            const span_entry r = mode == "b" ? span_break_line(line.data(), 0, n, at, (int64_t)tabs.size(), HostInt()) : span_seq_line(line.data(), 0, n, at, (int64_t)tabs.size(), HostInt());
            printf("%%d %%d %%d %%d %%d %%d\n", r.kind, r.field, r.id, r.end, r.value, r.noncanonical);
        }
        s = e + 1;
    }
    return 0;
}
'''


def line_rows(kind, data):
    """What the host program prints for the lines of a text, by the oracle."""
    out = []
    for _, line in ora.lines_of(data):
        f = line.split(b"\t")
        nc = [0]
        if kind == "c":
            L = cora.parse_line(line)
            few = L["dkind"] == cora.FEW_FIELDS
            bad = L["dkind"] == cora.BAD_INTEGER and L["dfield"] <= 2
            row = [ora.FEW_FIELDS if few else ora.BAD_INTEGER if bad else 0, L["dfield"] if bad else -1, L["id"], L["ce"], L["frag"]]
            if few or bad:
                out.append(row + [0] * 6)
                continue
            for k in (0, 1, 2):
                ora.key_field(f[k], nc)
            v6, v7 = ora.field_int(f[6]), ora.field_int(f[7])
            out.append(row + [nc[0], int(f[5] == b"+"), int(v6 is not None), v6 or 0, int(v7 is not None), v7 or 0])
            continue
        need, keys, plain = (5, (0, 1), 4) if kind == "b" else (3, (0,), 2)
        if len(f) < need:
            out.append([ora.FEW_FIELDS, -1, 0, 0, 0, 0])
            continue
        vals, bad = [], -1
        for k in keys + (plain,):
            v = ora.key_field(f[k], nc) if k in keys else ora.field_int(f[k])
            if v is None:
                bad = k
                break
            vals.append(v)
        vals += [0] * (3 - len(vals)) if kind == "b" else []
        if kind == "s":
            vals = [vals[0] if vals else 0, 0, vals[1] if len(vals) > 1 else 0]
        out.append([ora.BAD_INTEGER if bad >= 0 else 0, bad] + vals + [nc[0]])
    return out


def test_shared_header_as_a_host_program(tmp_path):
    """span_shared.hpp compiled by g++ into a stand-alone program under ASan + UBSan, with the host's own field_int: the line
    rules on every line of every case give the oracle's per-line results, and the "%.15g" formatter prints what Python prints
    for every value of the list and declines the rest, without a report."""
    from tests.test_sanitizers import BAD, ENV
    src = tmp_path / "span_host.cpp"
    src.write_text(HOST % {"root": ROOT})
    exe = str(tmp_path / "span_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, str(src)])
    path = tmp_path / "case.txt"

    def run(mode, data):
        path.write_bytes(data)
        r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, env=dict(os.environ, LC_ALL="C", **ENV["asan"]), stdin=subprocess.DEVNULL, timeout=300)
        assert not any(b in r.stderr for b in BAD), r.stderr[-3000:]
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-2000:])
        return r.stdout.splitlines()

    n = 0
    for name, clusters, brk, seq in all_files():
        if name == "five_e_minus_5":
            clusters = clusters[:20000]                     # (one line twenty thousand times over)
            clusters = clusters[:clusters.rfind(b"\n") + 1]
        for mode, data in (("c", clusters), ("b", brk), ("s", seq)):
            rows = [[int(x) for x in l.split()] for l in run(mode, data)]
            assert rows == line_rows(mode, data), (name, mode)
            n += len(rows)
    assert n > 20000
    xs, declined = g15_values()
    got = run("g", b"".join(b"%016x\n" % struct.unpack("<Q", struct.pack("<d", x))[0] for x in xs + declined))
    want = ["%.15g" % x for x in xs] + ["-"] * len(declined)
    bad = [(x, w, g) for x, w, g in zip(xs + declined, want, got) if w != g]
    assert not bad and len(got) == len(want), bad[:10]


def test_tool_refuses_cleanly_without_a_gpu(glue, tmp_path):
    """Bad arguments print the usage; with arguments in order and no usable device the status is 1, nothing is on stdout and an
    existing OUT keeps its bytes.  (DEFUSE_GPU names a device no machine has, so this is the same run with and without a GPU.)"""
    args = write_files(tmp_path, *EXAMPLE)
    out = tmp_path / "stats.out"
    for bad in ([], args[:4], args + ["-o"], args + ["more"]):
        p = subprocess.run([glue, "span_stats"] + bad, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert p.returncode == 1 and p.stderr.startswith("Usage: span_stats"), bad
    link = tmp_path / "span_stats"
    os.symlink(glue, link)
    for exe in ([glue, "span_stats"], [str(link)]):
        for have in (False, True):
            if have:
                out.write_bytes(b"kept")
            p = subprocess.run(exe + args + ["-o", str(out)], capture_output=True, text=True, env=dict(os.environ, DEFUSE_GPU="999"))
            assert p.returncode == 1 and "_create" in p.stderr and p.stdout == "" and len(p.stderr.splitlines()) == 1
            assert out.read_bytes() == b"kept" if have else not out.exists()
        out.unlink()


# ---------------------------------------------------------------------------------------------- GPU
def refused(sp, call):
    with pytest.raises(sp.SpanStatsError) as e:
        call()
    assert e.value.code == E_ARG, str(e.value)


def check_output(ctx, res, rows, text):
    """The rows and the text of a ctx against the oracle's; the mean by its bits."""
    got_rows, got_text = ctx.fetch()
    assert got_text == text and len(got_rows) == len(rows) == res["n_rows"]
    assert got_rows["cluster_id"].tolist() == [r[0] for r in rows] and got_rows["count"].tolist() == [r[1] for r in rows]
    assert got_rows["sum"].tolist() == [r[2] for r in rows]
    assert got_rows["mean"].tobytes() == np.array([r[3] for r in rows], dtype=np.float64).tobytes()
    lens = [len(l) + 1 for l in text.splitlines()]
    assert got_rows["text_len"].tolist() == lens and got_rows["text_off"].tolist() == [sum(lens[:k]) for k in range(len(lens))] if len(lens) < 50 else \
        got_rows["text_off"].tolist() == np.concatenate(([0], np.cumsum(lens)[:-1])).tolist()
    v = ctx.view()
    assert (v.n_rows, v.text_len) == (len(rows), len(text)) and v.rows and v.text


def run_case(sp, ctx, tc, name, clusters, brk, seq, pieces=None):
    """Both steps of a case on a span ctx and a taskc ctx against the oracle."""
    want = expect(dict(clusters=clusters, brk=brk, seq=seq))
    tc.begin()
    tc.add_pieces(clusters, pieces)
    assert same_result(ctx.breaks_text(brk, seq), want[0]), name
    if want[1] is None:
        refused(sp, lambda: ctx.stats(tc, sp.INPUT))        # no tables after a stop
        return
    got = ctx.stats(tc, sp.INPUT)
    assert same_result(got, want[2]), (name, got, want[2])
    if want[3] is None:
        refused(sp, ctx.view)
        refused(sp, ctx.fetch)
        return
    check_output(ctx, want[2], want[3], want[4])
    t = ctx.timing()
    assert t["n_lines"] == want[2]["n_lines"] and t["n_rows"] == want[2]["n_rows"] and all(t[k] >= 0 for k in t)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_cases_on_the_gpu(sp, cr, group):
    """Result structs, rows and text of every case equal the oracle's; one pair of contexts for all cases of a group, so every
    case but the first also runs on used ones - after a stop as well, and a good case follows the last stop."""
    group_cases = [c for c in cases() if c["group"] == group]
    assert len(group_cases) >= 7
    with sp.Context() as ctx, cr.Context() as tc:
        refused(sp, ctx.view)
        refused(sp, lambda: ctx.stats(tc, sp.INPUT))
        for c in group_cases + [dict(name="example", clusters=EXAMPLE[0], brk=EXAMPLE[1], seq=EXAMPLE[2])]:
            run_case(sp, ctx, tc, c["name"], c["clusters"], c["brk"], c["seq"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES + ("one_end",))
def test_fixtures_on_the_gpu(sp, cr, name):
    with sp.Context() as ctx, cr.Context() as tc:
        run_case(sp, ctx, tc, name, golden(name, "clusters"), golden(name, "break"), golden(name, "seq"))
        if name != "one_end":
            assert rows_of(ctx.fetch()[1]) == rows_of(golden(name, "stats.perl"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_texts_in_one_piece_and_in_pieces(sp, cr, seed):
    clusters, brk, seq = random_files(seed)
    with sp.Context() as ctx, cr.Context() as tc:
        run_case(sp, ctx, tc, "random_%d" % seed, clusters, brk, seq)
        whole = ctx.fetch()
        run_case(sp, ctx, tc, "random_%d in pieces" % seed, clusters, brk, seq, pieces=64)
        again = ctx.fetch()
        assert whole[1] == again[1] and whole[0].tobytes() == again[0].tobytes() and tc.timing()["n_pieces"] > 100


@pytest.mark.gpu
def test_dedup_text_as_the_source(sp, cr):
    """After taskc_dedup, TASKC_DEDUP gives the oracle's result on the dedup text and TASKC_INPUT the one on the input."""
    from tests.test_cluster_regions import random_text
    text = random_text(7)
    _, dedup_text = cora.dedup(text, 2)
    ids = sorted({int(l.split(b"\t")[0]) for l in text.splitlines()})
    rng = random.Random(7)
    brk = b"".join(br(i, e, rng.randrange(0, 90000)) for i in ids if i % 5 for e in (0, 1))
    seq = b"".join(sq(i, i % 3) for i in ids)
    tabs = ora.tables(brk, seq)[1]
    with sp.Context() as ctx, cr.Context() as tc:
        tc.begin()
        tc.add_pieces(text, 64)
        ctx.breaks_text(brk, seq)
        refused(sp, lambda: ctx.stats(tc, sp.DEDUP))        # no dedup text yet
        for _ in (0, 1):
            want = ora.stats(text, tabs)                    # (the input has ids with a third cluster end: a stop)
            assert same_result(ctx.stats(tc, sp.INPUT), want[0]) and want[0]["stop_kind"] == ora.NOT_TWO_ENDS
            refused(sp, ctx.fetch)
            assert tc.dedup(2)["stop_kind"] == 0 and tc.fetch(cr.DEDUP) == dedup_text
            want = ora.stats(dedup_text, tabs)
            assert same_result(ctx.stats(tc, sp.DEDUP), want[0]) and 0 < want[0]["n_rows"] < want[0]["n_ids"] and want[0]["n_lines"] < text.count(b"\n")
            check_output(ctx, *want)


@pytest.mark.gpu
def test_reuse(sp, cr):
    """A second, smaller call on the same contexts; a call after span_breaks_text replaced the tables; the capacity protocol."""
    C = {c["name"]: c for c in cases()}
    with sp.Context() as ctx, cr.Context() as tc:
        for name in ("many_one_fragment_clusters", "example", "big_cluster_at_256", "one_end", "empty", "break_few", "thirds_and_inter", "five_e_minus_5", "negative_mean"):
            c = C[name]
            run_case(sp, ctx, tc, name, c["clusters"], c["brk"], c["seq"])
        # other tables under the same cluster text
        c = C["thirds_and_inter"]
        run_case(sp, ctx, tc, "thirds", c["clusters"], c["brk"], c["seq"])
        first = ctx.fetch()
        brk2, seq2 = simple(2, base=400)[1] + simple(4)[1], sq(2, 1) + sq(4, 2)
        res, tabs = ora.tables(brk2, seq2)
        assert same_result(ctx.breaks_text(brk2, seq2), res)
        assert ctx.fetch()[1] == first[1]                   # the output of the stats before is still there
        want = ora.stats(c["clusters"], tabs)
        assert same_result(ctx.stats(tc, sp.INPUT), want[0]) and [r[0] for r in want[1]] == [2, 4]
        check_output(ctx, *want)
        # span_fetch writes nothing where either does not fit
        rows, text = ctx.fetch()
        lib, h = ctx._lib, ctx.handle
        r2, t2 = np.zeros(len(rows), sp.ROW_DTYPE), np.full(len(text), 7, np.uint8)
        fetch = lambda rc, tcap: lib.span_fetch(h, r2.ctypes.data, rc, t2.ctypes.data, tcap)
        assert fetch(len(r2) - 1, len(t2)) == E_CAPACITY and fetch(len(r2), len(t2) - 1) == E_CAPACITY and lib.span_fetch(h, None, 0, None, 0) == E_CAPACITY
        assert str(len(r2)) in lib.span_last_error().decode() and not r2.view(np.uint8).any() and (t2 == 7).all()
        assert fetch(len(r2), len(t2)) == 0 and r2.tobytes() == rows.tobytes() and t2.tobytes() == text and ctx.timing()["download_ms"] > 0


@pytest.mark.gpu
def test_resident_tables_equal_the_tables_of_the_texts(sp, cr):
    """A prediction with a split, EVAL_NO_SPLIT, PRED_NO_TASK, PRED_OUT_OF_WINDOW and EVAL_HOST_STATS groups: span_breaks_pred on
    the pred_ctx and span_breaks_text on what ptext_format printed of it (the caller's .seq lines spliced in) give identical
    rows and bytes for one cluster text, and the oracle's."""
    from defuse_amd import bat, eval as ev, pred, ptext
    from tests.test_pred import Store
    from tests.test_ptext import EDGE_FIDS, HOST_SEQ, edge_tasks, groups_of, kind_row
    tasks = edge_tasks()
    kinds = ["plain", "no_split", "no_task", "out_of_window", "host_stats", "plain", "no_split", "plain"]
    fids = EDGE_FIDS[:len(kinds)]
    groups = groups_of(ev, [kind_row(kind, fid) for kind, fid in zip(kinds, fids)])
    no_task_fid = int(groups["fusion_id"][2])
    ids = [no_task_fid if k == "no_task" else f for k, f in zip(kinds, fids)]
    clusters = b"".join(simple(i, 1 + k % 3, base=50 + 10 * k)[0] for k, i in enumerate(ids))
    with Store(bat, pred, tasks) as P, ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T, sp.Context() as ctx, cr.Context() as tc:
        refused(sp, lambda: ctx.breaks_pred(P.ctx))         # no prediction yet
        P.predict(groups)
        res, _ = P.fetch()
        T.format(P.ctx)
        seq_text, brk_text, lines = T.fetch()
        status = lines["status"].tolist()
        assert [bool(s & HOST_SEQ) for s in status] == [k == "host_stats" for k in kinds] and [int(l) > 0 for l in lines["brk_len"]] == [k not in ("no_task", "out_of_window") for k in kinds]
        for k in reversed(range(len(kinds))):               # the caller's own .seq lines, at seq_off of their rows
            if status[k] & HOST_SEQ:
                off = int(lines["seq_off"][k])
                seq_text = seq_text[:off] + sq(int(res["fusion_id"][k]), 0, 2, b"nan", b"nan") + seq_text[off:]
        tc.begin()
        tc.add(clusters)
        want_t, tabs = ora.tables_of_pred(res)
        assert ora.tables(brk_text, seq_text)[1] == tabs and len(tabs[1]) == 6 and 0 in tabs[0].values()
        want = ora.stats(clusters, tabs)
        assert want[0]["stop_kind"] == 0 and want[0]["n_rows"] == 6 and want[0]["n_ids"] == 8
        got_t = ctx.breaks_text(brk_text, seq_text)
        assert (got_t["n_breaks"], got_t["n_inters"], got_t["stop_kind"]) == (12, 6, 0)
        assert same_result(ctx.stats(tc, sp.INPUT), want[0])
        check_output(ctx, *want)
        from_text = ctx.fetch()
        assert same_result(ctx.breaks_pred(P.ctx), want_t)
        assert same_result(ctx.stats(tc, sp.INPUT), want[0])
        check_output(ctx, *want)
        from_pred = ctx.fetch()
        assert from_pred[1] == from_text[1] and from_pred[0].tobytes() == from_text[0].tobytes()
        P.predict(groups[[2, 3]])                           # no group with lines: empty tables, every id skipped
        assert same_result(ctx.breaks_pred(P.ctx), ora.result(n_lines=2))
        assert ctx.stats(tc, sp.INPUT)["n_rows"] == 0 and ctx.fetch()[1] == b""


@pytest.mark.gpu
def test_format_doubles_against_python(sp):
    xs, declined = g15_values()
    both = np.array(xs[:1000] + declined + xs[1000:] + declined, dtype=np.float64)
    want = [("%.15g" % x).encode() if taken(x) else b"" for x in both.tolist()]
    got = sp.format_doubles(both)
    bad = [(k, both[k], want[k], got[k]) for k in range(len(both)) if got[k] != want[k]]
    assert not bad, bad[:10]
    assert sp.format_doubles(np.zeros(0)) == [] and sp.format_doubles(np.array(declined)) == [b""] * len(declined)


def run_tool(glue, tmp_path, files, out, env=None):
    return subprocess.run([glue, "span_stats"] + write_files(tmp_path, *files) + ["-o", str(out)], capture_output=True, text=True,
                          env=dict(os.environ, DEFUSE_GLUE_PIECE_BYTES="64", **(env or {})), timeout=120)


@pytest.mark.gpu
def test_tool_writes_the_host_steps_file(glue, tmp_path):
    """On the fixtures and one random text, the cluster file in pieces of 64 bytes: byte-identical to calc_span_stats."""
    out = tmp_path / "stats.out"
    texts = [tuple(golden(n, k) for k in ("clusters", "break", "seq")) for n in FIXTURES] + [random_files(5)]
    for k, files in enumerate(texts):
        p = run_tool(glue, tmp_path, files, out, env={"DEFUSE_TIMING": "1"} if k == 0 else None)
        assert p.returncode == 0 and p.stdout == "", p.stderr
        assert ("[span_stats] device: upload" in p.stderr) == (k == 0)
        host = subprocess.run([glue, "calc_span_stats"] + write_files(tmp_path, *files), capture_output=True, check=True).stdout
        assert out.read_bytes() == host and len(host) > 0
        out.unlink()
    p = subprocess.run([glue, "span_stats"] + write_files(tmp_path, *EXAMPLE), capture_output=True)       # without -o: stdout
    assert p.returncode == 0 and p.stdout == b"5\t28.3333333333333\t3\n"


@pytest.mark.gpu
def test_tool_declines_what_the_host_step_must_judge(glue, tmp_path):
    """A stopping text and a text with a "007" id: status 3, one line on stderr, and OUT keeps its bytes or stays absent."""
    C = {c["name"]: c for c in cases()}
    out = tmp_path / "stats.out"
    for name, words in (("one_end", ["clusters.txt cluster 9", "not two cluster ends"]), ("break_int4", ["break.txt line 5", "field 5"]),
                        ("seq_few", ["seq.txt line 1", "too few"]), ("clusters_int2_first", ["clusters.txt line 1", "field 3"]),
                        ("bad_end", ["cluster 9", "field 8"]), ("three_spellings", ["8 key field(s)"])):
        c = C[name]
        for have in (True, False):
            if have:
                out.write_bytes(b"kept")
            p = run_tool(glue, tmp_path, (c["clusters"], c["brk"], c["seq"]), out)
            assert p.returncode == 3 and p.stdout == "" and all(w in p.stderr for w in words) and len(p.stderr.splitlines()) == 1, (name, p.stderr)
            assert out.read_bytes() == b"kept" if have else not out.exists(), name
            if have:
                out.unlink()
