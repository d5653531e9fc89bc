"""The regions file and the exon table parsed and resolved on the GPU (the "region and exon text" section of
include/defuse_task.h through defuse_amd/tasktext.py).

Yardstick: tests/tasktext_oracle.py, a restatement of the header's rules on bytes.  Without a GPU it is pinned to the tools' own
readers (ReadAlignRegionPairs and ExonRegions::Read of tools_src/defuse_host.hpp, run by a small program on every shape case),
taskt_shared.hpp gives its per-line results in a host program under ASan + UBSan, and every shape case is shown to reach the
edge it is named for.  On the GPU the results, fetched tables and pairs equal the oracle's, and the store made from text is
byte for byte the store task_store_create makes from the oracle's pairs and tables."""
import ctypes
import os
import random
import subprocess
from collections import OrderedDict

import numpy as np
import pytest

from tests import abi
from tests import tasktext_oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "tests", "golden", "smoke")
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
SPAN = 256 * 16                   # the bytes one workgroup of the line tables reads


@pytest.fixture(scope="module")
def tt(built):
    from defuse_amd import tasktext
    return tasktext


# ---------------------------------------------------------------------------------------------- shape cases
def xline(gene, t, chrom, strand, *coords):
    return b"\t".join([gene, t, chrom, strand] + [c if isinstance(c, bytes) else b"%d" % c for c in coords]) + b"\n"


def rline(fid, end, name, strand, start, stop, *more):
    f = [fid, end, name, strand, start, stop] + list(more)
    return b"\t".join(c if isinstance(c, bytes) else b"%d" % c for c in f) + b"\n"


E0 = xline(b"G1", b"T1", b"chr1", b"+", 10, 20, 30, 40) + xline(b"G1", b"T0", b"chr2", b"-", 5, 9) + xline(b"G2", b"T2", b"chr1", b"-", 100, 200)
R0 = rline(7, 0, b"chr1", b"+", 12, 50) + rline(7, 1, b"G1|T0", b"-", 1, 4) + rline(3, 0, b"G2|T2", b"+", 2, 9) + rline(3, 1, b"chr2", b"-", 3, 8)
REF0 = [b"chr2", b"G1|T1", b"chr1", b"G2|T2"]            # G1|T0 is absent
SEQ0 = [b"chr1", b"chr2", b"G1|T0", b"G2|T2"]            # G1|T1 is absent
EXON_GOOD = [xline(b"G", b"A%d" % k, b"c", b"+", k, k + 5) for k in range(3)]
REGION_GOOD = [rline(k, k & 1, b"c", b"+", 1, 9) for k in range(3)]


def padded_to(text, size, filler):
    """`text` with a first line put in front so that the whole has `size` bytes; filler(n) is a line of n bytes."""
    return filler(size - len(text)) + text


def exon_filler(n):
    return xline(b"P" * (n - len(xline(b"", b"pad", b"c", b"+", 1, 2))), b"pad", b"c", b"+", 1, 2)


def region_filler(n):
    return rline(900, 0, b"c", b"+", 1, 2, b"p" * (n - len(rline(900, 0, b"c", b"+", 1, 2, b""))))


def shape_cases():
    """[dict(name, group, exons, regions, ref, seq)]: texts and the two name lists."""
    C = []
    group = "table edges"

    def add(name, exons=E0, regions=R0, ref=REF0, seq=SEQ0):
        C.append(dict(name=name, group=group, exons=exons, regions=regions, ref=list(ref), seq=list(seq)))

    def add_both(name, exons, regions):           # both texts stop: a case each, so that the regions are reached
        add(name + "_x", exons)
        add(name + "_r", E0, regions)

    add("plain")
    add("empty", b"", b"")
    add("one_byte", b"x", b"\n")
    add("no_last_newline", E0[:-1], R0[:-1])
    for size in (SPAN, SPAN + 1):
        add("bytes_%d" % size, padded_to(E0, size, exon_filler), padded_to(R0, size, region_filler))
    for n in (256, 257):
        add("lines_%d" % n, b"".join(xline(b"G", b"L%03d" % k, b"c%d" % (k % 5), b"+-"[k & 1:][:1], k, k + 3) for k in range(n)),
            b"".join(rline(k // 2, k & 1, b"G|L%03d" % (k % 300), b"+", k, k + 9) for k in range(n)))
    coords = [v for k in range(700) for v in (1000000 + 10 * k + 1, 1000000 + 10 * k + 6)]
    add("exon_700", xline(b"G", b"S0", b"c", b"+", 1, 2) + xline(b"G", b"BIG", b"c", b"-", *coords) + xline(b"G", b"S1", b"c", b"+", 3, 4),
        rline(1, 0, b"G|BIG", b"+", 1, 5) + rline(1, 1, b"c", b"-", 2, 6))
    for k in range(6):                                   # the span edge falls behind the first byte of field k of a regions line
        line = rline(123456, 1, b"G1|T1", b"+", 7654321, 7654399)
        at = sum(len(f) + 1 for f in line.split(b"\t")[:k]) + 1
        add("span_split_f%d" % k, E0, padded_to(line + R0, SPAN + len(line) - at + len(R0), region_filler))
    group = "line rules"          # every stop kind at the first, a middle and the last line
    bad_exon = {"exon_int": xline(b"G", b"B", b"c", b"+", 1, b"x9"), "exon_strand": xline(b"G", b"B", b"c", b"*", 1, 9),
                "exon_long": xline(b"G", b"B" * (ora.MAX_NAME + 1), b"c", b"+", 1, 9), "exon_dup": xline(b"H", b"A1", b"d", b"-", 4, 8)}
    for name, bad in bad_exon.items():
        for where in ("first", "middle", "last"):
            if name == "exon_dup" and where == "first":
                continue
            g = EXON_GOOD
            add("%s_%s" % (name, where), b"".join({"first": [bad] + g, "middle": g[:2] + [bad] + g[2:], "last": g + [bad]}[where]))
    bad_region = {"region_int": rline(5, 0, b"c", b"+", b"1x", 9), "region_end": rline(5, 2, b"c", b"+", 1, 9), "region_strand": rline(5, 0, b"c", b"", 1, 9)}
    for name, bad in bad_region.items():
        for where in ("first", "middle", "last"):
            g = REGION_GOOD
            add("%s_%s" % (name, where), E0, b"".join({"first": [bad] + g, "middle": g[:2] + [bad] + g[2:], "last": g + [bad]}[where]))
    add_both("two_causes", b"".join(EXON_GOOD[:1] + [bad_exon["exon_strand"]] + EXON_GOOD[1:] + [bad_exon["exon_int"]]),
        b"".join(REGION_GOOD[:1] + [bad_region["region_strand"]] + REGION_GOOD[1:] + [bad_region["region_int"]]))
    add_both("two_causes_one_line", xline(b"G", b"B", b"c", b"?", 1, b""), rline(b"x", 2, b"c", b"?", 1, 9))
    ten = [xline(b"G", b"Q%d" % k, b"c", b"+", k, k + 5) for k in range(12)]
    dup, bad = xline(b"H", b"Q2", b"d", b"-", 4, 8), xline(b"G", b"QB", b"c", b"*", 1, 9)
    add("dup_before_strand", b"".join(ten[:4] + [dup] + ten[4:8] + [bad] + ten[8:]))          # Q2 on lines 3 and 5, the strand on line 10
    add("strand_before_dup", b"".join(ten[:4] + [bad] + ten[4:8] + [dup] + ten[8:]))
    add("dup_before_int_first_lines", b"".join(ten[:1] + ten[:1] + [bad_exon["exon_int"]]))
    add("end_before_strand", E0, rline(1, 2, b"c", b"?", 1, 9))
    add("strand_before_int", E0, rline(1, 1, b"c", b"?", b"z", 9))
    add("unpaired_junk", xline(b"G", b"U", b"c", b"+", 1, 5, b"junk") + xline(b"G", b"V", b"c", b"-", 1, 5, 7, 9, b""))
    add("six_fields_empty_5", b"g\tt\tc\t+\t1\t\n")
    add("five_fields_exon", b"g\tt\tc\t+\t1\n" + E0)
    add("int_forms", xline(b"G", b"I", b"c", b"+", b"+007", b"-0", b"-12", b"+0"),
        rline(b"+007", 0, b"c", b"+", b"-0", b"+5") + rline(7, 1, b"c", b"-", b"2147483647", b"-2147483648") + rline(b"2147483647", b"+1", b"c", b"+", 1, 2))
    add_both("int_plus_alone", xline(b"G", b"I", b"c", b"+", b"+", 5), rline(1, 0, b"c", b"+", b"-", 5))
    add_both("int_2p31", xline(b"G", b"I", b"c", b"+", 1, b"2147483648"), rline(b"2147483648", 0, b"c", b"+", 1, 5))
    add_both("int_minus_2p31_less", xline(b"G", b"I", b"c", b"+", b"-2147483649", 1), rline(1, 0, b"c", b"+", 1, b"99999999999999999999"))
    add_both("cr_in_last_field", b"g\tt\tc\t+\t1\t5\r\n", b"1\t0\tc\t+\t5\t9\r\n")
    add("cr_in_ignored_field", b"g\tt\tc\t+\t1\t5\tx\r\n", b"1\t0\tc\t+\t5\t9\tx\r\n" + R0)
    add_both("cr_in_strand", b"g\tt\tc\t+\r\t1\t5\n", b"1\t0\tc\t-\r\t5\t9\n")
    add("region_fields", E0, b"4\t0\tchr1\t+\n" + b"\n" + rline(8, 0, b"chr1", b"+", 1, 2, b"a", b"b") + rline(6, 1, b"chr1", b"-", 3, 4))
    add("region_five_fields", E0, rline(6, 1, b"chr1", b"-", 3, 4) + b"5\t0\tchr1\t+\tjunk\n")
    group = "names"
    names = [b"ABCDEFGH" + b"x", b"ABCDEFGH" + b"w", b"ABCDEFGHIJKLMNOP" + b"b", b"ABCDEFGHIJKLMNOP" + b"a", b"ABCDEFGH", b"ABCDEFGHIJKLMNOP", b"AB", b"",
             b"\xff\x80", b"\x7f", b"a\x00b", b"a\x00", b"a", b"N" * ora.MAX_NAME, b"N" * (ora.MAX_NAME - 1)]
    chroms = [b"chrB", b"", b"chrA", b"chrB\x00", b"\xe9", b"C" * ora.MAX_NAME]
    ex = b"".join(xline(b"" if k == 3 else b"g%d" % (k % 4), t, chroms[k % len(chroms)], b"+-"[k & 1:][:1], k + 1, k + 9) for k, t in enumerate(names))
    regs = [b"g|t|x", b"|AB", b"g0|", b"g|", b"chrA", b"", b"g1|ABCDEFGHx", b"g1|ABCDEFGHx|", b"zz|\xff\x80|q", b"nobody", b"a\x00b", b"|", b"||", b"chrB\x00",
            b"x|" + b"N" * ora.MAX_NAME, b"g0|a\x00"]
    add("names", ex, b"".join(rline(k // 2, k & 1, n, b"+-"[k & 1:][:1], k, k + 20) for k, n in enumerate(regs)),
        ref=[b"chrA", b"g1|ABCDEFGHx", b"|", b"\xe9", b"g0|ABCDEFGH", b"g3|", b"g0|a", b"zzz"], seq=[b"chrA", b"", b"g|t|x", b"\xff", b"|AB", b"a\x00b"])
    add("name_max_plus_one_chrom", xline(b"G", b"T", b"C" * (ora.MAX_NAME + 1), b"+", 1, 2))
    many = [xline(b"G", b"D%03d" % k, b"c", b"+", k, k + 1) for k in range(320)]
    add("dup_300_lines_later", b"".join(many[:10] + many[10:310] + [xline(b"G2", b"D010", b"e", b"-", 1, 2)] + many[310:]))
    group = "pairs"
    rng = random.Random(11)
    ids = list(range(40, 0, -1))
    add("ids_descending", E0, b"".join(rline(i, e, b"chr1", b"+", i, i + 5) for i in ids for e in (1, 0)))
    rng.shuffle(ids)
    add("ids_shuffled", E0, b"".join(rline(i, rng.randint(0, 1), b"chr%d" % rng.randint(1, 3), b"-", i, i + 5) for i in ids + ids[:13]))
    filler = [rline(1000 + k, k & 1, b"chr2", b"+", k, k + 1) for k in range(600)]
    add("ends_600_apart", E0, rline(5, 1, b"chr1", b"+", 1, 2) + b"".join(filler) + rline(5, 0, b"G1|T1", b"-", 3, 4))
    add("last_line_wins", E0, rline(9, 0, b"chr1", b"+", 1, 2) + rline(4, 1, b"chr2", b"+", 5, 6) + rline(9, 0, b"chr2", b"-", 3, 4) + rline(b"+009", 0, b"G1|T1", b"+", 7, 8))
    add("end_1_only", E0, rline(2, 1, b"chr1", b"-", 4, 9))
    add("negative_id", E0, rline(3, 0, b"chr1", b"+", 1, 2) + rline(-5, 1, b"chr1", b"+", 1, 2) + rline(-2147483648, 0, b"chr1", b"+", 1, 2))
    add("coord_beyond", E0, rline(3, 0, b"chr1", b"+", 1, 2) + rline(2, 0, b"chr1", b"+", 1, 2) + rline(3, 1, b"chr1", b"+", ora.MAX_COORD - 2, ora.MAX_COORD + 1))
    add("span_beyond", E0, rline(2, 0, b"chr1", b"+", 1, 2) + rline(3, 0, b"chr1", b"+", -1, ora.MAX_REGION))
    assert len({c["name"] for c in C}) == len(C) and {c["group"] for c in C} == set(GROUPS)
    return C


def oracle_of(case):
    eres, T = ora.parse_exons(case["exons"], case["ref"])
    if T is None:
        return eres, None, None, None, None
    rres, pairs, plines = ora.parse_regions(case["regions"], case["seq"], T)
    return eres, T, rres, pairs, plines


# ---------------------------------------------------------------------------------------------- without a GPU
def test_header_and_binding_agree(tt):
    sizes, n = abi.check("defuse_task.h", tt, r"taskt_[a-z_]+", constants=tt.CONSTANTS)
    assert sizes == [80, 40] and n == 12 == len(tt.EXPORTS)
    assert (ora.MAX_NAME, ora.EXON_LONG_NAME, ora.EXON_DUPLICATE) == (tt.MAX_NAME, tt.EXON_LONG_NAME, tt.EXON_DUPLICATE)
    assert tt.EXON_LONG_NAME >= tt.LIBRARY_LIMIT > tt.REGION_BAD_STRAND


def test_argument_errors_need_no_device(tt):
    lib = tt.lib()
    err = lambda: lib.taskt_last_error().decode()
    h, one = ctypes.c_void_p(), ctypes.c_void_p(1)        # `one` stands for an object: argument errors come before it is looked at
    res = tt.TasktResult()
    text = np.frombuffer(b"abc", dtype=np.uint8)
    off = np.array([0, 2, 1], dtype=np.int64)
    assert lib.taskt_names_create(0, None, 0, None, 0, None) == E_ARG and "no output" in err()
    assert lib.taskt_names_create(0, None, -1, None, 0, ctypes.byref(h)) == E_ARG and "negative" in err()
    assert lib.taskt_names_create(0, None, 0, None, 1, ctypes.byref(h)) == E_ARG and "null pointer" in err()
    assert lib.taskt_names_create(0, text.ctypes.data, 3, off.ctypes.data, 2, ctypes.byref(h)) == E_ARG and "name 1" in err()
    off[:] = [0, 1, 9]
    assert lib.taskt_names_create(0, text.ctypes.data, 3, off.ctypes.data, 2, ctypes.byref(h)) == E_ARG and "ends outside" in err()
    dup = np.frombuffer(b"abab", dtype=np.uint8)
    off[:] = [0, 2, 4]
    assert lib.taskt_names_create(0, dup.ctypes.data, 4, off.ctypes.data, 2, ctypes.byref(h)) == E_ARG and "names 0 and 1 are equal" in err()
    assert lib.taskt_names_create(0, None, 0, None, 2 ** 31, ctypes.byref(h)) == E_LIMIT
    assert lib.taskt_create(0, None) == E_ARG
    for fn in (lib.taskt_parse_exons, lib.taskt_parse_regions):
        assert fn(one, one, text.ctypes.data, 3, None) == E_ARG and "no result" in err()
        assert fn(one, one, text.ctypes.data, -1, ctypes.byref(res)) == E_ARG and "negative length" in err() and res.stop_field == -1
        assert fn(one, one, text.ctypes.data, 2 ** 31, ctypes.byref(res)) == E_LIMIT and "2^31 - 1" in err()
        assert fn(one, one, None, 3, ctypes.byref(res)) == E_ARG and "null pointer" in err()
        assert fn(None, one, text.ctypes.data, 3, ctypes.byref(res)) == E_ARG and "no ctx" in err()
        assert fn(one, None, text.ctypes.data, 3, ctypes.byref(res)) == E_ARG and "no names" in err()
    assert lib.taskt_exons(None) is None
    assert lib.taskt_exons_fetch(one, None, -1, None, 0, None, 0, None, 0, None, 0) == E_ARG and "negative capacity" in err()
    assert lib.taskt_exons_fetch(one, None, 1, None, 0, None, 0, None, 0, None, 0) == E_ARG and "capacity without a buffer" in err()
    assert lib.taskt_exons_fetch(None, None, 0, None, 0, None, 0, None, 0, None, 0) == E_ARG and "no ctx" in err()
    assert lib.taskt_pairs_fetch(one, None, 0, None, -1) == E_ARG and lib.taskt_pairs_fetch(one, None, 2, None, 0) == E_ARG
    assert lib.taskt_pairs_fetch(None, None, 0, None, 0) == E_ARG and "no ctx" in err()
    prm = tt.task.Params(70, 130, 20, 30)
    assert lib.taskt_store_create(one, one, ctypes.byref(prm), None) == E_ARG and "no output" in err()
    assert lib.taskt_store_create(None, one, ctypes.byref(prm), ctypes.byref(h)) == E_ARG and "no ctx" in err()
    assert lib.taskt_store_create(one, None, ctypes.byref(prm), ctypes.byref(h)) == E_ARG and "no reference" in err()
    assert lib.taskt_store_create(one, one, None, ctypes.byref(h)) == E_ARG and "no params" in err()
    assert lib.taskt_get_timing(None, None) == E_ARG
    lib.taskt_destroy(None)
    lib.taskt_names_destroy(None)
    # without a GPU the objects cannot be made; with one they can
    rc = lib.taskt_create(999, ctypes.byref(h))
    assert rc == E_DEVICE and not h and "device" in err()
    rc = lib.taskt_names_create(999, None, 0, None, 0, ctypes.byref(h))
    assert rc == E_DEVICE and not h


def test_the_cases_reach_their_edges():
    """On the oracle alone: what every shape case is named for."""
    got = {c["name"]: (c,) + oracle_of(c) for c in shape_cases()}
    stop = lambda r: (r["stop_line"], r["stop_kind"], r["stop_field"])
    for name, (c, eres, T, rres, pairs, plines) in got.items():
        assert (T is None) == (eres["stop_line"] > 0) and (T is None or (pairs is None) == (rres["stop_line"] > 0)), name
    c, eres, T, rres, pairs, _ = got["plain"]
    assert T.names == [b"T0", b"T1", b"T2"] and T.chroms == [b"chr1", b"chr2"] and T.chrom_ref == [2, 0]
    assert [t[4] for t in T.transcripts] == [4 + 2 + 0, 1, 3] and [t[2] for t in T.transcripts] == [2, 0, 3]
    assert pairs == [(3, (3, 2, -1, 0, 2, 9), (1, -1, 1, 1, 3, 8)), (7, (0, -1, 0, 0, 12, 50), (2, 0, -1, 1, 1, 4))]
    assert got["empty"][1]["n_lines"] == 0 and got["empty"][3]["n_lines"] == 0 and got["empty"][4] == []
    assert (got["one_byte"][1]["n_lines"], got["one_byte"][1]["n_skipped"], got["one_byte"][3]["n_skipped"]) == (1, 1, 1)
    assert got["no_last_newline"][4] == got["plain"][4] and got["no_last_newline"][2].transcripts == T.transcripts
    for size in (SPAN, SPAN + 1):
        c = got["bytes_%d" % size][0]
        assert len(c["exons"]) == len(c["regions"]) == size and [p[0] for p in got["bytes_%d" % size][4]] == [3, 7, 900]
    for n in (256, 257):
        assert got["lines_%d" % n][1]["n_items"] == n and got["lines_%d" % n][3]["n_lines"] == n
    c, eres, T = got["exon_700"][:3]
    big = c["exons"].index(b"BIG")
    assert eres["n_exons"] == 702 and big < SPAN and len(c["exons"]) > 2 * SPAN and T.transcripts[0][2:4] == (1, 700)
    for k in range(6):
        c, _, _, rres, pairs, plines = got["span_split_f%d" % k]
        line = c["regions"].split(b"\n")[1]
        start = c["regions"].index(line)
        fields, at = line.split(b"\t"), start
        for f in fields[:k]:
            at += len(f) + 1
        assert at < SPAN <= at + len(fields[k]) and (len(fields[k]) == 1 or SPAN < at + len(fields[k])) and rres["stop_line"] == 0 and plines[-1] == [0, 2], k
    for name in ("exon_int", "exon_strand", "exon_long", "exon_dup"):
        kind, field = {"exon_int": (ora.EXON_BAD_INTEGER, 5), "exon_strand": (ora.EXON_BAD_STRAND, 3), "exon_long": (ora.EXON_LONG_NAME, 1),
                       "exon_dup": (ora.EXON_DUPLICATE, 1)}[name]
        for where, line in (("first", 1), ("middle", 3), ("last", 4)):
            if name + "_" + where in got:
                assert stop(got[name + "_" + where][1]) == (line, kind, field), (name, where)
    for name, (kind, field) in {"region_int": (ora.REGION_BAD_INTEGER, 4), "region_end": (ora.REGION_BAD_END, 1), "region_strand": (ora.REGION_BAD_STRAND, 3)}.items():
        for where, line in (("first", 1), ("middle", 3), ("last", 4)):
            assert stop(got[name + "_" + where][3]) == (line, kind, field), (name, where)
    assert stop(got["two_causes_x"][1]) == (2, ora.EXON_BAD_STRAND, 3) and stop(got["two_causes_r"][3]) == (2, ora.REGION_BAD_STRAND, 3)
    assert stop(got["two_causes_one_line_x"][1]) == (1, ora.EXON_BAD_INTEGER, 5) and stop(got["two_causes_one_line_r"][3]) == (1, ora.REGION_BAD_INTEGER, 0)
    assert stop(got["dup_before_strand"][1]) == (5, ora.EXON_DUPLICATE, 1) and stop(got["strand_before_dup"][1]) == (5, ora.EXON_BAD_STRAND, 3)
    assert got["dup_before_strand"][0]["exons"].split(b"\n")[9].split(b"\t")[3] == b"*" and got["strand_before_dup"][0]["exons"].split(b"\n")[9].startswith(b"H\tQ2")
    assert stop(got["dup_before_int_first_lines"][1]) == (2, ora.EXON_DUPLICATE, 1)
    assert stop(got["end_before_strand"][3]) == (1, ora.REGION_BAD_END, 1) and stop(got["strand_before_int"][3]) == (1, ora.REGION_BAD_STRAND, 3)
    assert got["unpaired_junk"][1]["n_exons"] == 3 and got["unpaired_junk"][1]["stop_line"] == 0
    assert stop(got["six_fields_empty_5"][1]) == (1, ora.EXON_BAD_INTEGER, 5)
    assert got["five_fields_exon"][1]["n_skipped"] == 1 and got["five_fields_exon"][1]["n_items"] == 3
    assert got["int_forms"][2].exons == [(7, 0), (-12, 0)]
    assert got["int_forms"][4] == [(7, (-1, -1, 0, 0, 0, 5), (-1, -1, 0, 1, 2147483647, -2147483648)), (2147483647, (-1, -1, -1, 0, 0, 0), (-1, -1, 0, 0, 1, 2))]
    for name, xfield, rfield in (("int_plus_alone", 4, 4), ("int_2p31", 5, 0), ("int_minus_2p31_less", 4, 5), ("cr_in_last_field", 5, 5)):
        assert stop(got[name + "_x"][1]) == (1, ora.EXON_BAD_INTEGER, xfield) and stop(got[name + "_r"][3]) == (1, ora.REGION_BAD_INTEGER, rfield), name
    assert got["cr_in_ignored_field"][1]["n_items"] == 1 and got["cr_in_ignored_field"][3]["n_items"] == 3
    assert stop(got["cr_in_strand_x"][1]) == (1, ora.EXON_BAD_STRAND, 3) and stop(got["cr_in_strand_r"][3]) == (1, ora.REGION_BAD_STRAND, 3)
    r = got["region_fields"][3]
    assert (r["n_lines"], r["n_skipped"], r["n_items"], r["stop_line"]) == (4, 2, 2, 0)
    assert stop(got["region_five_fields"][3]) == (2, ora.REGION_BAD_INTEGER, 5)
    c, eres, T, rres, pairs, _ = got["names"]
    assert eres["stop_line"] == 0 and T.names[0] == b"" and T.names.index(b"ABCDEFGH") + 1 == T.names.index(b"ABCDEFGHIJKLMNOP")
    assert T.names.index(b"ABCDEFGHw") + 1 == T.names.index(b"ABCDEFGHx") and T.names.index(b"ABCDEFGHIJKLMNOPa") + 1 == T.names.index(b"ABCDEFGHIJKLMNOPb")
    assert T.names.index(b"a") < T.names.index(b"a\x00") < T.names.index(b"a\x00b") and T.names[-1] == b"\xff\x80" and b"" in T.chroms
    assert len(T.names[T.names.index(b"N" * ora.MAX_NAME)]) == ora.MAX_NAME and T.chroms == [b"chrB", b"", b"chrA", b"chrB\x00", b"\xe9", b"C" * ora.MAX_NAME]
    n_ref = len(c["ref"])
    refs = [t[4] for t in T.transcripts]
    assert sum(r < n_ref for r in refs) == 3 and sum(r >= n_ref + len(T.chroms) for r in refs) == len(refs) - 3 and sorted(T.chrom_ref)[:2] == [0, 3]
    ends = {n: e for (fid, e0, e1) in pairs for n, e in zip(c["regions"].split(b"\n")[2 * pairs.index((fid, e0, e1)):][:2], (e0, e1))}
    by = {l.split(b"\t")[2]: e for l, e in ends.items()}
    t_of = lambda n: T.tindex[n]
    assert by[b"g|t|x"][:3] == (2, -1, -1) and by[b"|AB"][:3] == (4, t_of(b"AB"), -1) and by[b"g0|"][:3] == (-1, t_of(b""), -1) and by[b"g|"][1] == t_of(b"")
    assert by[b"chrA"][:3] == (0, -1, T.cindex[b"chrA"]) and by[b""][:3] == (1, -1, T.cindex[b""]) and by[b"g1|ABCDEFGHx|"][1] == t_of(b"ABCDEFGHx")
    assert by[b"zz|\xff\x80|q"][1] == t_of(b"\xff\x80") and by[b"nobody"][:3] == (-1, -1, -1) and by[b"a\x00b"][:3] == (5, -1, -1)
    assert by[b"|"][1] == t_of(b"") and by[b"||"][1] == t_of(b"") and by[b"chrB\x00"][2] == 3 and by[b"x|" + b"N" * ora.MAX_NAME][1] >= 0 and by[b"g0|a\x00"][1] >= 0
    assert stop(got["name_max_plus_one_chrom"][1]) == (1, ora.EXON_LONG_NAME, 2)
    assert stop(got["dup_300_lines_later"][1]) == (311, ora.EXON_DUPLICATE, 1)
    assert [p[0] for p in got["ids_descending"][4]] == list(range(1, 41)) and [p[0] for p in got["ids_shuffled"][4]] == list(range(1, 41))
    assert got["ends_600_apart"][5][0] == [602, 1] and got["ends_600_apart"][4][0][1][1] == 1
    assert got["last_line_wins"][5] == [[0, 2], [4, 0]] and got["last_line_wins"][4][1][1][:3] == (-1, 1, -1)
    assert got["end_1_only"][4] == [(2, (-1, -1, -1, 0, 0, 0), (0, -1, 0, 1, 4, 9))]
    assert ora.check_pairs(got["negative_id"][4]) == (E_ARG, 0, None) and got["negative_id"][4][0][0] == -2147483648
    assert ora.check_pairs(got["coord_beyond"][4]) == (E_LIMIT, 1, 1) and ora.check_pairs(got["span_beyond"][4]) == (E_LIMIT, 1, 0)
    assert ora.check_pairs(got["plain"][4]) is None


READERS = r'''
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include "%(root)s/tools_src/defuse_host.hpp"
static std::string hex(const std::string& s)
{
    std::string out = "x";
    char b[3];
    for (unsigned char c : s) { snprintf(b, sizeof b, "%%02x", c); out += b; }
    return out;
}
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[2], std::ios::binary);
    if (std::string(argv[1]) == "exons") {
        defuse::ExonRegions E;
        E.Read(in);
        E.ForEachTranscript([&](const std::string& t, const std::string& gene, const std::string& chrom, int strand, const std::vector<defuse::Region>& ex) {
            std::cout << hex(t) << ' ' << hex(gene) << ' ' << hex(chrom) << ' ' << strand;
            for (const auto& r : ex) std::cout << ' ' << r.start << ' ' << r.end;
            std::cout << '\n';
        });
    } else {
        for (const auto& kv : defuse::ReadAlignRegionPairs(in)) {
            std::cout << kv.first;
            for (const auto& l : kv.second) std::cout << ' ' << hex(l.refName) << ' ' << l.strand << ' ' << l.start << ' ' << l.end;
            std::cout << '\n';
        }
    }
    return 0;
}
'''
LIBRARY_LIMIT_CASES = ("exon_long", "exon_dup", "name_max_plus_one_chrom", "dup_300_lines_later", "dup_before_")


def test_the_oracle_is_the_tools_readers(tmp_path):
    """ReadAlignRegionPairs and ExonRegions::Read of tools_src/defuse_host.hpp on every shape case: the oracle's tables and
    pairs, or the reference's message, stream and exit status at the oracle's stop line.  (The duplicate-transcript and
    long-name cases are limits of the library: the readers read on there.)"""
    src = tmp_path / "readers.cpp"
    src.write_text(READERS % {"root": ROOT})
    exe = str(tmp_path / "readers")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src)])
    unhex = lambda h: bytes.fromhex(h[1:])
    path = tmp_path / "case.txt"

    def run(mode, data):
        path.write_bytes(data)
        return subprocess.run([exe, mode, str(path)], capture_output=True, stdin=subprocess.DEVNULL, timeout=60)

    def check_stop(r, res, data, what):
        line = data[res["stop_off"]:res["stop_off"] + res["stop_len"]]
        assert r.returncode == 1
        if res["stop_kind"] in (ora.EXON_BAD_INTEGER, ora.REGION_BAD_INTEGER):
            assert r.stdout == b"Failed to interpret %s:\n" % what + line + b"\n" and r.stderr == b""
        elif res["stop_kind"] == ora.REGION_BAD_END:
            assert r.stdout == b"" and r.stderr == b"Error: DebugCheck pairEnd == 0 || pairEnd == 1 failed\n"
        else:
            assert r.stdout == b"" and r.stderr == b"Error: Unable to intepret strand " + line.split(b"\t")[3] + b"\n"

    n_stops = 0
    for c in shape_cases():
        if not c["name"].startswith(LIBRARY_LIMIT_CASES):
            eres, T = ora.parse_exons(c["exons"], c["ref"])
            r = run("exons", c["exons"])
            if T is None:
                check_stop(r, eres, c["exons"], b"exon")
                n_stops += 1
            else:
                assert r.returncode == 0 and r.stderr == b"", c["name"]
                rows = [l.split(b" ") for l in r.stdout.splitlines()]
                theirs = {unhex(f[0].decode()): (unhex(f[1].decode()), unhex(f[2].decode()), int(f[3]), [(int(a), int(b)) for a, b in zip(f[4::2], f[5::2])])
                          for f in rows}
                assert theirs == T.table, c["name"]
        stop, ends, _, _ = ora.read_regions(c["regions"])
        r = run("regions", c["regions"])
        if stop is not None:
            check_stop(r, ora.result(stop=stop), c["regions"], b"region")
            n_stops += 1
        else:
            assert r.returncode == 0 and r.stderr == b"", c["name"]
            theirs = {}
            for l in r.stdout.splitlines():
                f = l.split(b" ")
                theirs[int(f[0])] = [(unhex(f[k].decode()), int(f[k + 1]), int(f[k + 2]), int(f[k + 3])) for k in (1, 5)]
            mine = {fid: [got[e][:4] if e in got else (b"", 0, 0, 0) for e in (0, 1)] for fid, got in ends.items()}
            assert theirs == mine, c["name"]
    assert n_stops >= 30


HOST = r'''
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>
#include "%(root)s/tools_src/defuse_host.hpp"
#include "%(root)s/defuse_amd/csrc/taskt_shared.hpp"
struct HostInt {
    bool operator()(const uint8_t* p, int64_t n, int& v) const { return n >= 0 && defuse::field_int(reinterpret_cast<const char*>(p), (size_t)n, v); }
};
struct TabAt {
    const int64_t* tabs;
    int64_t operator()(int64_t k) const { return tabs[k]; }
};
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[2], std::ios::binary);
    const std::string data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    // an exact copy on the heap: a read beyond the text is a report
    std::vector<uint8_t> text(data.begin(), data.end());
    const bool exons = std::string(argv[1]) == "exons";
    int64_t s = 0;
    while (s < (int64_t)text.size()) {
        int64_t e = s;
        std::vector<int64_t> tabs;
        for (; e < (int64_t)text.size() && text[(size_t)e] != '\n'; ++e)
            if (text[(size_t)e] == '\t') tabs.push_back(e);
        if (exons) {
            const taskt_exon_line r = taskt_parse_exon_line(text.data(), s, e, (int64_t)tabs.size(), TabAt{tabs.data()}, HostInt());
            printf("%%d %%d %%d %%d\n", r.kind, r.field, r.n_exons, r.strand);
        } else {
            const taskt_region_line r = taskt_parse_region_line(text.data(), s, e, (int64_t)tabs.size(), TabAt{tabs.data()}, HostInt());
            printf("%%d %%d %%d %%d %%d %%d %%d %%lld %%d\n", r.kind, r.field, r.id, r.end, r.strand, r.start, r.stop, (long long)(r.kind ? 0 : r.name_off - s),
                   r.name_len);
        }
        s = e + 1;
    }
    task_pair p = {5, {{0, 0, 0, 0, 1, 2}, {0, 0, 0, 0, TASK_MAX_COORD, TASK_MAX_COORD}}};
    int e = -1;
    if (taskt_pair_fault(p, &e) != 0) return 3;
    p.end[1].end = TASK_MAX_COORD + 1;
    if (taskt_pair_fault(p, &e) != 2 || e != 1) return 4;
    p.end[1] = task_end{0, 0, 0, 0, INT32_MIN, INT32_MAX};
    if (taskt_pair_fault(p, &e) != 2 || e != 1) return 5;
    p.end[1] = task_end{0, 0, 0, 0, 0, TASK_MAX_REGION};
    if (taskt_pair_fault(p, &e) != 3 || e != 1) return 6;
    p.end[0] = task_end{0, 0, 0, 0, TASK_MAX_REGION, -2};
    if (taskt_pair_fault(p, &e) != 3 || e != 0) return 7;
    p.fusion_id = -1;
    if (taskt_pair_fault(p, &e) != 1) return 8;
    return 0;
}
'''


def test_shared_header_as_a_host_program(tmp_path):
    """taskt_shared.hpp compiled by g++ into a stand-alone program under ASan + UBSan, with the host's own field_int: on every
    line of every shape case it gives the oracle's per-line result, without a report."""
    from tests.test_sanitizers import BAD, ENV
    src = tmp_path / "taskt_host.cpp"
    src.write_text(HOST % {"root": ROOT})
    exe = str(tmp_path / "taskt_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, str(src)])
    path = tmp_path / "case.txt"
    n = 0
    for c in shape_cases():
        for mode, data in (("exons", c["exons"]), ("regions", c["regions"])):
            path.write_bytes(data)
            r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV["asan"]), stdin=subprocess.DEVNULL, timeout=120)
            assert not any(b in r.stderr for b in BAD), (c["name"], r.stderr[-3000:])
            assert r.returncode == 0, (c["name"], mode, r.returncode, r.stderr[-2000:])
            rows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
            want = []
            for _, line in ora.lines_of(data):
                if mode == "exons":
                    kind, field, row = ora.exon_line(line)
                    want.append([kind, field, len(row[4]), row[3]] if kind == 0 else [kind, field] + rows[len(want)][2:])
                    assert kind == 0 or rows[len(want) - 1][3] in (0, 1)
                else:
                    kind, field, row = ora.region_line(line)
                    name_off = sum(len(f) + 1 for f in line.split(b"\t")[:2])
                    want.append([kind, field, row[0], row[1], row[3], row[4], row[5], name_off, len(row[2])] if kind == 0 else [kind, field] + rows[len(want)][2:])
            assert [w[:2] for w in want] == [g[:2] for g in rows] and want == rows, (c["name"], mode)
            n += len(rows)
    assert n > 2000


# ---------------------------------------------------------------------------------------------- GPU
def pairs_array(tt, pairs):
    out = np.zeros(len(pairs), dtype=tt.task.PAIR_DTYPE)
    for k, (fid, e0, e1) in enumerate(pairs):
        out[k]["fusion_id"] = fid
        out[k]["end"][0], out[k]["end"][1] = e0, e1
    return out


def refused(tt, call, name):
    """A call that needs a table the ctx does not hold: DSA_E_ARG."""
    with pytest.raises(tt.TaskTextError) as e:
        call()
    assert e.value.code == E_ARG, (name, str(e.value))
    return str(e.value)


def run_case(tt, ctx, case):
    """Both parses of a case on `ctx` against the oracle; returns the oracle's (eres, T, rres, pairs, plines)."""
    eres, T, rres, pairs, plines = want = oracle_of(case)
    name = case["name"]
    tiny = lambda: tt.task.Reference(OrderedDict((n.decode("latin-1"), b"ACGT") for n in case["seq"]))
    with tt.Names(case["ref"]) as ref, tt.Names(case["seq"]) as seq:
        assert ctx.parse_exons(ref, case["exons"]) == eres, name
        if T is None:
            assert ctx.exons_handle() is None, name
            assert "no exon table" in refused(tt, lambda: ctx.parse_regions(seq, case["regions"]), name)
            refused(tt, ctx.exons, name)
            with tiny() as ref3:
                assert "no exon table" in refused(tt, lambda: ctx.store(ref3, (70, 130, 20, 30)), name)
            return want
        assert ctx.exons_handle(), name
        tx, ex, cref, names = ctx.exons()
        assert names == T.names, name
        assert [tuple(int(v) for v in t) for t in tx.tolist()] == T.transcripts, name
        assert [tuple(int(v) for v in e) for e in ex.tolist()] == T.exons and cref.tolist() == T.chrom_ref, name
        assert ctx.parse_regions(seq, case["regions"]) == rres, name
        if pairs is None:
            refused(tt, ctx.pairs, name)
            with tiny() as ref3:
                assert "no pairs" in refused(tt, lambda: ctx.store(ref3, (70, 130, 20, 30)), name)
            return want
        got, lines = ctx.pairs()
        assert got.tobytes() == pairs_array(tt, pairs).tobytes(), (name, got.tolist(), pairs)
        assert lines.tolist() == plines, name
    return want


GROUPS = ["table edges", "line rules", "names", "pairs"]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_shape_cases_on_the_gpu(tt, group):
    """Results, fetched tables and pairs of every shape case equal the oracle's; one ctx for all cases of a group."""
    cases = [c for c in shape_cases() if c["group"] == group]
    assert len(cases) >= 3
    with tt.Context() as ctx:
        for case in cases:
            run_case(tt, ctx, case)
        t = ctx.timing()
        assert t["exon_bytes"] > 0 and t["region_bytes"] > 0 and t["exon_device_ms"] >= 0


@pytest.mark.gpu
def test_exon_coordinate_beyond_the_table_limit(tt):
    """2^31 - 1 is an integer of the text and a coordinate task_exons_create refuses: its code and message come through."""
    with tt.Context() as ctx, tt.Names([]) as ref:
        with pytest.raises(tt.TaskTextError) as e:
            ctx.parse_exons(ref, xline(b"G", b"T", b"c", b"+", 1, b"2147483647"))
        assert e.value.code == E_LIMIT and "transcript 0" in str(e.value) and ctx.exons_handle() is None
        assert ctx.parse_exons(ref, E0)["n_items"] == 3


@pytest.mark.gpu
def test_store_checks_on_the_device(tt):
    """A negative id and a coordinate or span beyond the limits parse, and taskt_store_create refuses them with check_pairs'
    code, naming the lowest pair, its id and its line."""
    cases = {c["name"]: c for c in shape_cases()}
    with tt.Context() as ctx, tt.task.Reference(OrderedDict((n.decode(), b"ACGT" * 30) for n in SEQ0)) as ref:
        for name, code, words in (("negative_id", E_ARG, ["pair 0 ", "lines 3 and 0", "fusion_id -2147483648"]),
                                  ("coord_beyond", E_LIMIT, ["pair 1 ", "fusion_id 3", "line 3", "end[1]", "coordinate"]),
                                  ("span_beyond", E_LIMIT, ["pair 1 ", "fusion_id 3", "line 2", "end[0]", "spans"])):
            _, _, _, pairs, _ = run_case(tt, ctx, cases[name])
            assert ora.check_pairs(pairs)[0] == code
            with pytest.raises(tt.TaskTextError) as e:
                ctx.store(ref, (70, 130, 20, 30))
            assert e.value.code == code and all(w in str(e.value) for w in words), (name, str(e.value))
        run_case(tt, ctx, cases["plain"])
        with pytest.raises(tt.TaskTextError) as e:
            ctx.store(ref, (70, 2 ** 30, 20, 30))
        assert e.value.code == E_LIMIT and "params" in str(e.value)
        with tt.task.Reference(OrderedDict([("chr1", b"ACGT")])) as short, pytest.raises(tt.TaskTextError) as e:
            ctx.store(short, (70, 130, 20, 30))
        assert e.value.code == E_ARG and "sequences" in str(e.value)
        with ctx.store(ref, (70, 130, 20, 30)) as st:
            assert st.counts().n_tasks == 2


def texts_of(seqs, table, regions):
    """The exon table and a regions file of tests/test_task_store.py's worlds, written out as the tools read them."""
    exons = b"".join(xline(gene.encode(), t.encode(), chrom.encode(), b"+-"[strand:][:1], *[v for e in ex for v in e]) for t, (gene, chrom, strand, ex) in table.items())
    regs = b"".join(rline(fid, e, a["refName"].encode(), b"+-"[a["strand"]:][:1], a["start"], a["end"]) for fid, pair in regions.items() for e, a in enumerate(pair))
    return exons, regs


def oracle_exons(tt, T):
    """task_exons_create over the oracle's table, as arrays."""
    lib = tt.task.lib()
    tx = np.array(T.transcripts, dtype=np.int32).reshape(-1, 5).view(tt.task.TRANSCRIPT_DTYPE).reshape(-1)
    ex = np.array(T.exons, dtype=np.int32).reshape(-1, 2).view(tt.task.EXON_DTYPE).reshape(-1)
    cref = np.array(T.chrom_ref, dtype=np.int32)
    h = ctypes.c_void_p()
    rc = lib.task_exons_create(0, cref.ctypes.data, len(cref), tx.ctypes.data, len(tx), ex.ctypes.data, len(ex), ctypes.byref(h))
    assert rc == 0, lib.task_last_error()

    class Handle:
        handle = h
    return Handle, lambda: lib.task_exons_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_store_from_text(tt, seed):
    """The generator of test_task_store.py's random_case written out as text: the store made from text equals, byte for byte,
    the store task_store_create makes from the oracle's pairs and tables."""
    from tests.test_task_store import int_params, random_case
    seqs, table, cases = random_case(seed)
    rng = random.Random(seed)
    every = [c.encode() for c in seqs]
    ref_names = [n for n in every if rng.random() < 0.6] + [b"unused"]
    rng.shuffle(ref_names)
    with tt.Context() as ctx, tt.task.Reference(seqs) as ref, tt.Names(ref_names) as rn, tt.Names(every) as sn:
        for params, regions in cases:
            exons, regs = texts_of(seqs, table, regions)
            eres, T = ora.parse_exons(exons, ref_names)
            rres, pairs, _ = ora.parse_regions(regs, every, T)
            assert ctx.parse_exons(rn, exons) == eres and ctx.parse_regions(sn, regs) == rres and rres["n_items"] == len(regions) == 75
            assert any(r >= len(ref_names) for r in T.chrom_ref + [t[4] for t in T.transcripts]) and any(t[4] < len(ref_names) for t in T.transcripts)
            theirs_exons, destroy = oracle_exons(tt, T)
            try:
                with ctx.store(ref, int_params(params)) as mine, tt.task.Store(ref, theirs_exons, int_params(params), pairs_array(tt, pairs)) as theirs:
                    a, b = mine.fetch(), theirs.fetch()
                    assert len(a[0]) == 75 and len(a[3]) >= 150
                    for x, y in zip(a, b):
                        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
                    assert (a[0]["fusion_id"] == sorted(regions)).all()
            finally:
                destroy()


@pytest.mark.gpu
def test_smoke_vector_through_the_whole_chain_from_the_texts(tt, gpu_ctx):
    """tests/test_task_store.py::test_smoke_vector_through_the_whole_chain_from_the_store with the store made from the two
    texts: the same final files."""
    from defuse_amd import bat, cand, pred
    from defuse_amd import eval as ev
    from oracle import dosplitalign_oracle as dora
    from tests.test_batch_assembly import DeviceArray
    from tests.test_pred import check as check_pred, expected
    from tests.test_task_store import int_params
    d = SMOKE + "/"
    regions = dora.read_align_region_pairs(d + "regions.txt")
    tasks = dora.create_tasks(d + "ref.fa", d + "exons.txt", 300, 30, 50, 50, regions)         # for the expected records only
    exon_text, region_text = open(d + "exons.txt", "rb").read(), open(d + "regions.txt", "rb").read()
    seqs = OrderedDict(dora.FastaIndex(d + "ref.fa").seqs)
    _, T = ora.parse_exons(exon_text, [])
    ref_names = T.chroms + [T.table[t][0] + b"|" + t for t in T.names]
    names = {n.decode(): k for k, n in enumerate(ref_names)}
    reads = {}
    dora.read_fastq(d + "reads.1.fastq", reads)
    dora.read_fastq(d + "reads.2.fastq", reads)
    with tt.Context() as ctx, tt.task.Reference(seqs) as ref, tt.Names(ref_names) as rn, tt.Names(list(seqs)) as sn:
        assert ctx.parse_exons(rn, exon_text)["stop_line"] == 0 and ctx.parse_regions(sn, region_text)["n_items"] == len(regions)
        with ctx.store(ref, int_params((300, 30, 50, 50))) as st:
            rec, _, _, regs = st.fetch()
            assert (rec["status"] == 0).all()
            als = cand.alignments([(names.get(rname, -1), strand, start, end, dora.lexical_cast_int(frag), rend)
                                   for frag, rend, rname, strand, start, end in dora.sam_alignments(d + "improper.sam")])
            with cand.Table(regs) as table_, bat.Reads.from_dict(reads) as r, bat.Batch() as b, pred.Context(st.tasks) as P, table_.session() as s, \
                    ev.Context(0) as ectx:
                ptr, n = s.enumerate_device(als, cand.ORDER_FUSION)
                gpu_ctx.upload_device(b.assemble_device(r, st.windows, ptr, n))
                n_rec = gpu_ctx.run()
                with DeviceArray(np.zeros(n_rec, dtype=np.dtype("V40"))) as dev:
                    assert gpu_ctx.records_to_device(dev.ptr, n_rec) == n_rec
                    groups, _ = ectx.evaluate_device(dev.ptr, n_rec)
                P.predict_resident(ectx)
                res, seq = P.fetch()
                assert len(res) == len(groups) == len(tasks) and (res["status"] == 0).all()
                lines = "".join(P.format_break(row, [a["refName"] for a in regions[int(row["fusion_id"])]], [a["strand"] for a in regions[int(row["fusion_id"])]])
                                for row in res)
                assert lines == open(d + "expected.break.txt").read()
                check_pred(res, seq, expected(tasks, gpu_ctx.download()))


@pytest.mark.gpu
def test_reuse(tt):
    """A ctx used for a second exon table and regions file, larger and then smaller, and after a stop, gives each problem's own."""
    cases = {c["name"]: c for c in shape_cases()}
    with tt.Context() as ctx:
        for name in ("plain", "lines_257", "names", "exon_strand_middle", "plain", "region_end_last", "ids_shuffled", "empty", "exon_700"):
            run_case(tt, ctx, cases[name])
        _, _, _, pairs, _ = run_case(tt, ctx, cases["plain"])
        with tt.task.Reference(OrderedDict((n.decode(), b"ACGT" * 30) for n in SEQ0)) as ref, ctx.store(ref, (70, 130, 20, 30)) as st:
            assert st.fetch()[0]["fusion_id"].tolist() == [p[0] for p in pairs]
