"""remove_duplicates and get_align_regions on cluster text in device memory (the "cluster text" section of
include/defuse_task.h through defuse_amd/clusterregions.py) and `defuse_glue cluster_regions`.

Yardstick: tests/clusterregions_oracle.py, a restatement of the header's rules on bytes.  Without a GPU it is pinned to the
reference's Perl scripts (tests/golden/glue/ and tests/golden/cluster_regions/, compared order-free as tests/test_glue.py
compares) and, byte for byte, to the host steps of bin/defuse_glue on every shape case; taskc_shared.hpp gives the oracle's
per-line results in a host program under ASan + UBSan.  On the GPU the result structs, both texts and the stop fields of every
shape case equal the oracle's, the chain from sct_cover to taskt_store_create equals the host route, and the tool writes the two
host steps' files."""
import ctypes
import os
import random
import subprocess
from collections import OrderedDict, defaultdict

import numpy as np
import pytest

from tests import abi
from tests import clusterregions_oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SMOKE = os.path.join(GOLDEN, "smoke")
TOOL = os.path.join(ROOT, "bin", "defuse_glue")
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
BLOCK = 256                       # threads per workgroup of every taskc kernel (txt_shared.hpp's BLOCK)
INT_MIN, INT_MAX = ora.INT_MIN, ora.INT_MAX


@pytest.fixture(scope="module")
def cr(built):
    from defuse_amd import clusterregions
    return clusterregions


@pytest.fixture(scope="module")
def glue(built):
    from defuse_amd import build
    build.build_tools()
    return TOOL


# ---------------------------------------------------------------------------------------------- shape cases
def cl(cid, ce, frag, name, strand, start, end, *more, re=0):
    f = [cid, ce, frag, re, name, strand, start, end] + list(more)
    return b"\t".join(c if isinstance(c, bytes) else b"%d" % c for c in f) + b"\n"


def frag2(cid, frag, p0, p1, s0=b"+", s1=b"-", n0=b"chr1", n1=b"G2|T9"):
    """Both lines of a fragment whose positions (start on "+", end on "-") are p0 and p1."""
    def line(e, p, s, n):
        return cl(cid, e, frag, n, s, p, p + 49) if s == b"+" else cl(cid, e, frag, n, s, p - 49, p)
    return line(0, p0, s0, n0) + line(1, p1, s1, n1)


def run_of(cid, n, frag0=100, dups=True):
    """A run of n fragments; with dups every third repeats the pair of the one in front."""
    out = []
    for k in range(n):
        same = dups and k % 3 == 2
        out.append(frag2(cid, frag0 + k, 1000 + (k - 1 if same else k), 5000 + 7 * (k - 1 if same else k)))
    return b"".join(out)


TEXT40 = b"".join(run_of(cid, 4, 10 * cid) for cid in (5, 2, 9, 2, 7))          # 40 lines, id 2 comes back
GOOD = run_of(3, 3) + run_of(8, 2)
GROUPS = ["sizes", "pieces", "ids", "order", "cluster ends", "stops", "bytes"]


def shape_cases():
    """[dict(name, group, text, min, pieces)]; pieces: None (one piece), "lines" (a line per piece), an int (pieces of that
    many bytes, cut anywhere) or a list of offsets where pieces given with final = 0 end."""
    C = []
    group = "sizes"

    def add(name, text, min_size=1, pieces=None):
        C.append(dict(name=name, group=group, text=text, min=min_size, pieces=pieces))

    add("empty", b"")
    add("one_line_no_newline", cl(4, 2, 1, b"c", b"+", 1, 2)[:-1])
    add("one_fragment_no_newline", frag2(4, 1, 10, 20)[:-1])
    add("run_of_1", frag2(4, 1, 10, 20))
    for n in (63, 64, 65, 129):
        add("run_of_%d" % n, run_of(1, 2) + run_of(6, n) + run_of(2, 2), 2)
    add("run_over_two_workgroups", run_of(6, 2 * BLOCK + 88) + run_of(2, 3), 2)
    group = "pieces"
    add("one_line_per_piece", TEXT40, 2, "lines")
    add("cut_mid_line", TEXT40, 2, [len(TEXT40) // 4 + 3, len(TEXT40) // 2 + 1, 3 * len(TEXT40) // 4 + 5])
    lines30 = run_of(1, 2) + run_of(6, 15) + run_of(2, 2)
    at = [sum(len(l) + 1 for l in lines30.split(b"\n")[:k]) for k in (12, 22)]
    add("run_spans_three_pieces", lines30, 2, at)
    add("stop_in_second_piece", run_of(3, 4) + run_of(8, 2) + b"8\t0\tx\n" + run_of(9, 2), 1, [len(run_of(3, 4))])
    add("no_newline_in_a_piece", TEXT40, 2, 16)
    group = "ids"
    add("one_value_three_spellings", frag2(b"7", 1, 10, 20) + frag2(b"+7", 2, 11, 20) + frag2(b"007", 3, 10, 20) + frag2(b"8", 3, 10, 20), 3)
    add("id_comes_back", run_of(4, 3) + run_of(1, 2) + run_of(4, 3, 200), 2)
    add("negative_ids", run_of(-3, 3) + run_of(INT_MIN, 2) + run_of(5, 2) + run_of(-1, 2) + run_of(INT_MAX, 2), 2)
    group = "order"
    edge = [INT_MIN, -1, 0, INT_MAX]
    add("extreme_fragments_and_positions",
        b"".join(cl(1, 0, f, b"c", b"+", p, 0) + cl(1, 1, f, b"d", b"-", 0, edge[(k + 1) % 4]) for k, (f, p) in enumerate(zip(edge, reversed(edge)))) +
        b"".join(cl(2, 0, f, b"c", b"+", INT_MAX, 0) + cl(2, 1, f, b"d", b"-", 0, INT_MIN) for f in reversed(edge)), 1)
    add("duplicates_differ_in_fragment", b"".join(frag2(1, f, 500, 900) for f in (9, -4, 7, 300)) + frag2(1, 8, 500, 901), 2)
    add("equal_in_one_position", frag2(1, 5, 500, 900) + frag2(1, 4, 500, 901) + frag2(1, 3, 499, 900) + frag2(1, 2, 500, 900), 3)
    add("all_on_one_pair", b"".join(frag2(1, f, 77, 88) for f in range(40, 0, -1)) + run_of(2, 2), 1)
    add("fragment_end_twice", frag2(1, 5, 500, 900) + frag2(1, 6, 600, 950) + cl(1, 0, 5, b"later", b"-", 1, 600) + frag2(1, 7, 1, 2) + cl(1, 1, 6, b"z", b"+", 901, 1), 1)
    group = "cluster ends"
    add("other_ends", cl(1, 2, 0, b"c", b"+", b"x", b"y") + run_of(1, 2) + cl(1, -1, 5, b"c", b"?", b"", b"") + frag2(1, 50, 1, 2) + cl(3, 2, 0, b"c", b"+", 1, 2) +
        run_of(1, 2, 300) + cl(1, 7, 0, b"c", b"+", 1, 2), 2)
    add("one_end_and_three", cl(9, 0, 1, b"c", b"+", 1, 2) + cl(9, 1, 1, b"c", b"+", 1, 2) + cl(9, 2, 1, b"c", b"+", 1, 2) + cl(4, 1, 1, b"c", b"+", 1, 2) +
        cl(6, 0, 1, b"c", b"+", 1, 2) + cl(6, 1, 1, b"c", b"+", 1, 2))
    for m in (3, 4, 0, -5, 2 ** 40):                      # run 3 keeps 3 fragments, run 8 keeps 2
        add("min_%d" % m, run_of(3, 4) + run_of(8, 2), m)
    group = "stops"
    bad = {"few": b"5\t0\t1\t0\tc\t+\t7\n", "empty": b"\n", "int0": cl(b"5x", 0, 1, b"c", b"+", 1, 2), "int1": cl(5, b"", 1, b"c", b"+", 1, 2),
           "int2": cl(5, 0, b"-", b"c", b"+", 1, 2), "int6": cl(8, 0, 9, b"c", b"+", b"1.5", 2), "int7": cl(8, 1, 9, b"c", b"-", 1, b"2147483648")}
    for name, line in bad.items():
        add("%s_first" % name, line + GOOD)
        add("%s_last" % name, GOOD + line)
        add("%s_last_no_newline" % name, GOOD + line[:-1])
    add("empty_line_middle", run_of(3, 3) + b"\n" + run_of(8, 2))
    add("missing_end_first_run", cl(3, 0, 5, b"c", b"+", 1, 2) + cl(3, 1, 4, b"c", b"+", 1, 2) + run_of(8, 2))
    add("missing_end_last_run", GOOD + cl(9, 1, 5, b"c", b"+", 1, 2))
    add("two_stops", run_of(3, 2) + cl(4, 0, 5, b"c", b"+", 1, 2) + run_of(8, 2) + bad["int2"] + run_of(9, 2))
    add("two_line_stops", run_of(3, 2) + bad["int6"] + bad["few"] + run_of(9, 2))
    add("bad_line_and_missing_end_in_one_run", run_of(3, 2) + cl(8, 0, 4, b"c", b"+", 1, 2) + bad["int6"] + cl(8, 1, 9, b"c", b"+", 1, 2))
    add("bad_id_behind_a_missing_end", run_of(3, 2) + cl(8, 0, 4, b"c", b"+", 1, 2) + bad["int0"] + run_of(9, 2))
    add("bad_position_opens_a_new_run", run_of(3, 2) + cl(5, 0, 4, b"c", b"+", 1, 2) + bad["int6"])
    add("cr_on_plus_line", cl(1, 0, 1, b"c", b"+", 5, b"12\r") + cl(1, 1, 1, b"c", b"+", 6, 9))
    add("cr_on_minus_line", cl(1, 0, 1, b"c", b"+", 5, 9) + cl(1, 1, 1, b"c", b"-", 6, b"12\r"))
    add("cr_newlines", frag2(1, 1, 5, 9).replace(b"\n", b"\tx\r\n"))
    add("eight_and_twelve_fields", frag2(1, 1, 5, 9) + cl(1, 0, 2, b"c", b"+", 7, 8, b"a", b"b", b"", b"12x") + cl(1, 1, 2, b"c", b"+", b"+07", b"-0", b""))
    add("ignored_position_field", cl(1, 0, 1, b"c", b"+", 5, b"junk") + cl(1, 1, 1, b"c", b"-", b"", 9))
    group = "bytes"
    add("long_name", frag2(1, 1, 5, 9, n0=b"N" * 300) + frag2(1, 2, 6, 9, n1=bytes(range(32, 256)) * 2))
    add("long_line", frag2(1, 1, 5, 9) + cl(1, 0, 2, b"c", b"+", 7, 8, b"q" * 5000) + cl(1, 1, 2, b"L" * 5000, b"-", 1, 8) + frag2(2, 1, 5, 9))
    add("empty_name_and_odd_strands", cl(1, 0, 1, b"", b"x", 5, 9) + cl(1, 1, 1, b"c", b"", 6, 9) + cl(1, 0, 2, b"", b"+-", 5, 10) + cl(1, 1, 2, b"\x00\xff", b"\x00", 6, 11))
    assert len({c["name"] for c in C}) == len(C) and {c["group"] for c in C} == set(GROUPS)
    assert all(len(c["text"]) < 200000 for c in C)
    return C


def random_text(seed, n_lines=2000):
    """Runs of 1-30 fragments with duplicates, ids that come back, (fragment, end) given again, now and then another end."""
    rng = random.Random(seed)
    out, n = [], 0
    while n < n_lines:
        cid = rng.randrange(-5, 60)
        base = [rng.randrange(-1000, 90000), rng.randrange(1000, 90000)]
        frags, lines = [], []
        for k in range(rng.randrange(1, 31)):
            fr = rng.randrange(-50, 400)
            p = [base[0] + rng.randrange(4), base[1] + rng.randrange(3)]
            frags.append(fr)
            lines.append(frag2(cid, fr, p[0], p[1], rng.choice([b"+", b"-"]), rng.choice([b"+", b"-"]), rng.choice([b"chr1", b"chr1_alt"]), rng.choice([b"G|T", b"chrX"])))
        if rng.random() < 0.2:
            lines.append(cl(cid, rng.choice([2, -1]), 0, b"c", b"+", 1, 2))
        rng.shuffle(lines)
        out += lines
        n += 2 * len(lines)
    return b"".join(out)


def feed(ctx, text, pieces):
    ctx.begin()
    if pieces is None:
        assert ctx.add(text) == len(text)
    elif pieces == "lines":
        lines = text.split(b"\n")
        for l in lines[:-1]:
            assert ctx.add(l + b"\n", final=False) == len(l) + 1
        ctx.add(lines[-1], final=True)
    elif isinstance(pieces, int):
        ctx.add_pieces(text, pieces)
    else:
        pos = 0
        for cut in pieces:
            used = ctx.add(text[pos:cut], final=False)
            assert 0 <= used <= cut - pos and (used == 0 or text[pos + used - 1:pos + used] == b"\n")
            pos += used
        assert ctx.add(text[pos:], final=True) == len(text) - pos


# ---------------------------------------------------------------------------------------------- without a GPU
def test_header_and_binding_agree(cr):
    from defuse_amd import task, tasktext
    sizes, n = abi.check("defuse_task.h", cr, r"taskc_[a-z_]+", constants=cr.CONSTANTS)
    assert sizes == [96, 48] and n == 11 == len(cr.EXPORTS)
    assert abi.check_functions("defuse_task.h", task, r"task_[a-z_]+") == 12 and abi.check_functions("defuse_task.h", tasktext, r"taskt_[a-z_]+") == 12
    assert (cr.FEW_FIELDS, cr.BAD_INTEGER, cr.MISSING_END, cr.NOT_TWO_ENDS) == (ora.FEW_FIELDS, ora.BAD_INTEGER, ora.MISSING_END, ora.NOT_TWO_ENDS)


def test_argument_errors_need_no_device(cr):
    lib = cr.lib()
    err = lambda: lib.taskc_last_error().decode()
    h, one = ctypes.c_void_p(), ctypes.c_void_p(1)        # `one` stands for an object: argument errors come before it is looked at
    res, used = cr.TaskcResult(), ctypes.c_int64(5)
    text = np.frombuffer(b"abc", dtype=np.uint8)
    assert lib.taskc_create(0, None) == E_ARG and "no output" in err()
    assert lib.taskc_begin(None) == E_ARG
    assert lib.taskc_add(one, text.ctypes.data, 3, 1, None) == E_ARG and "consumed" in err()
    assert lib.taskc_add(one, text.ctypes.data, -1, 1, ctypes.byref(used)) == E_ARG and "negative" in err() and used.value == 0
    assert lib.taskc_add(one, text.ctypes.data, 2 ** 31, 1, ctypes.byref(used)) == E_LIMIT and "2^31 - 1" in err()
    assert lib.taskc_add(one, None, 3, 1, ctypes.byref(used)) == E_ARG and "null pointer" in err()
    assert lib.taskc_add(one, text.ctypes.data, 3, 2, ctypes.byref(used)) == E_ARG and "final" in err()
    assert lib.taskc_add(None, text.ctypes.data, 3, 1, ctypes.byref(used)) == E_ARG and "no ctx" in err()
    assert lib.taskc_add_cover(None, one) == E_ARG and "no ctx" in err() and lib.taskc_add_cover(one, None) == E_ARG and "no cover" in err()
    assert lib.taskc_dedup(one, 1, None) == E_ARG and "no result" in err()
    assert lib.taskc_dedup(None, 1, ctypes.byref(res)) == E_ARG and "no ctx" in err() and res.stop_field == -1
    assert lib.taskc_regions(one, 0, None) == E_ARG and "no result" in err()
    for source in (-1, 2, 7):
        assert lib.taskc_regions(one, source, ctypes.byref(res)) == E_ARG and "source" in err()
    assert lib.taskc_regions(None, cr.DEDUP, ctypes.byref(res)) == E_ARG and "no ctx" in err()
    for which in (-1, 0, 3):
        assert lib.taskc_fetch(one, which, 0, None, 0) == E_ARG and "which" in err()
    assert lib.taskc_fetch(None, cr.REGIONS, 0, None, 0) == E_ARG and "no ctx" in err()
    assert lib.taskc_parse_regions(None, one, one, None) == E_ARG and "no ctx" in err()
    assert lib.taskc_get_timing(None, None) == E_ARG
    lib.taskc_destroy(None)
    rc = lib.taskc_create(999, ctypes.byref(h))
    assert rc == E_DEVICE and not h and "device" in err()


def _by_cluster(text):
    d = defaultdict(list)
    for l in text.splitlines():
        d[int(l.split(b"\t")[0])].append(l)
    return d


def _pos(line):
    f = line.split(b"\t")
    return int(f[6]) if f[5] == b"+" else int(f[7])


def _pairs(lines):
    frag = defaultdict(dict)
    for l in lines:
        f = l.split(b"\t")
        frag[int(f[2])][f[1]] = _pos(l)
    return sorted((v[b"0"], v[b"1"]) for v in frag.values())


@pytest.mark.parametrize("inp,min_size,dedup,regions", [("glue/dups_in.txt", 3, "glue/dups_out.perl.txt", None), ("glue/regions_in.txt", 1, None, "glue/regions_out.perl.txt"),
                                                        ("cluster_regions/clusters1_in.txt", 2, "cluster_regions/clusters1_dedup.perl.txt", "cluster_regions/clusters1_regions.perl.txt"),
                                                        ("cluster_regions/clusters2_in.txt", 2, "cluster_regions/clusters2_dedup.perl.txt", "cluster_regions/clusters2_regions.perl.txt")])
def test_oracle_agrees_with_the_perl_scripts(inp, min_size, dedup, regions):
    """Order-free, as tests/test_glue.py compares: the same clusters survive with as many lines and the same position pairs
    (which duplicate stays is hash order in the script); the regions are the same set of lines."""
    read = lambda name: open(os.path.join(GOLDEN, name), "rb").read()
    data = read(inp)
    if dedup:
        res, got = ora.dedup(data, min_size)
        g, e, src = _by_cluster(got), _by_cluster(read(dedup)), set(data.splitlines())
        assert res["stop_kind"] == 0 and sorted(g) == sorted(e)
        for cid in g:
            assert len(g[cid]) == len(e[cid]) and all(l in src for l in g[cid])
            assert _pairs(g[cid]) == _pairs(e[cid])
    if regions:
        res, got = ora.regions(data)
        assert res["stop_kind"] == 0 and sorted(got.splitlines()) == sorted(read(regions).splitlines())
        keys = [tuple(int(v) for v in l.split(b"\t")[:2]) for l in got.splitlines()]
        assert keys == sorted(keys)


def test_new_goldens_have_what_the_old_ones_lack():
    for seed in (1, 2):
        lines = [l.split(b"\t") for l in open(os.path.join(GOLDEN, "cluster_regions", "clusters%d_in.txt" % seed), "rb").read().splitlines()]
        runs, seen_twice, names = [], False, defaultdict(set)
        for k, f in enumerate(lines):
            if k == 0 or f[0] != lines[k - 1][0]:
                runs.append((f[0], set()))
            seen_twice |= (f[2], f[1]) in runs[-1][1]
            runs[-1][1].add((f[2], f[1]))
            names[(f[0], f[1])].add((f[4], f[5]))
        ids = [r[0] for r in runs]
        assert seen_twice and len(set(ids)) < len(ids) and any(len({n for n, _ in v}) > 1 for v in names.values()) and any(len({s for _, s in v}) > 1 for v in names.values())


def test_the_cases_reach_their_edges():
    """On the oracle alone: what the shape cases are named for."""
    got = {c["name"]: (c, ora.dedup(c["text"], c["min"]), ora.regions(c["text"])) for c in shape_cases()}
    d = lambda name: got[name][1][0]
    r = lambda name: got[name][2][0]
    stop = lambda res: (res["stop_line"], res["stop_kind"], res["stop_field"], res["stop_value"])
    assert d("empty")["n_lines"] == 0 and got["empty"][1][1] == b"" and got["empty"][2][1] == b""
    assert d("one_line_no_newline")["n_runs"] == 1 and stop(r("one_line_no_newline")) == (0, ora.NOT_TWO_ENDS, -1, 4)
    assert got["one_fragment_no_newline"][1][1] == got["run_of_1"][1][1] == frag2(4, 1, 10, 20)
    for n in (63, 64, 65, 129):
        assert d("run_of_%d" % n)["n_fragments"] == n + 4 and d("run_of_%d" % n)["n_kept_fragments"] == n - n // 3 + 4
    assert d("run_over_two_workgroups")["n_fragments"] > 2 * BLOCK + 3 and d("run_over_two_workgroups")["n_runs"] == 2
    assert TEXT40.count(b"\n") == 40 and d("one_line_per_piece") == d("cut_mid_line") and d("one_line_per_piece")["n_runs"] == 5 and r("cut_mid_line")["n_clusters"] == 4
    assert all(TEXT40[c - 1:c] != b"\n" for c in got["cut_mid_line"][0]["pieces"])
    c = got["run_spans_three_pieces"][0]
    assert all(c["text"][p - 1:p] == b"\n" and c["text"][p:p + 2] == b"6\t" for p in c["pieces"])
    c = got["stop_in_second_piece"][0]
    assert stop(d("stop_in_second_piece")) == (13, ora.FEW_FIELDS, -1, 0) and d("stop_in_second_piece")["stop_off"] > c["pieces"][0]
    assert d("one_value_three_spellings")["n_runs"] == 2 and d("one_value_three_spellings")["n_kept_runs"] == 0 and d("one_value_three_spellings")["n_fragments"] == 4
    assert d("id_comes_back")["n_runs"] == 3 and r("id_comes_back")["n_clusters"] == 2
    assert got["negative_ids"][2][1].startswith(b"-2147483648\t0\t") and r("negative_ids")["n_clusters"] == 5
    out = got["extreme_fragments_and_positions"][1][1].splitlines()
    assert [int(l.split(b"\t")[2]) for l in out[::2]] == [INT_MIN, -1, 0, INT_MAX, INT_MIN] and d("extreme_fragments_and_positions")["n_kept_fragments"] == 5
    assert [int(l.split(b"\t")[2]) for l in got["duplicates_differ_in_fragment"][1][1].splitlines()[::2]] == [-4, 8]
    assert d("equal_in_one_position")["n_kept_fragments"] == 3 and [int(l.split(b"\t")[2]) for l in got["equal_in_one_position"][1][1].splitlines()[::2]] == [2, 3, 4]
    assert d("all_on_one_pair")["n_kept_fragments"] == 1 + 2 and got["all_on_one_pair"][1][1].startswith(b"1\t0\t1\t")
    out = got["fragment_end_twice"][1][1]
    assert b"later" in out and b"\tz\t" in out and d("fragment_end_twice")["n_fragments"] == 3
    assert d("other_ends")["n_runs"] == 3 and d("other_ends")["stop_kind"] == 0 and stop(r("other_ends")) == (1, ora.BAD_INTEGER, 6, 0)
    assert stop(r("one_end_and_three")) == (0, ora.NOT_TWO_ENDS, -1, 4) and stop(d("one_end_and_three")) == (4, ora.MISSING_END, -1, 1)
    assert [d("min_%d" % m)["n_kept_runs"] for m in (3, 4, 0, -5, 2 ** 40)] == [1, 0, 2, 2, 0] and d("min_3")["n_kept_fragments"] == 3
    n_good = GOOD.count(b"\n")
    for name, (kind, dfield, rfield) in {"few": (ora.FEW_FIELDS, -1, -1), "empty": (ora.FEW_FIELDS, -1, -1), "int0": (ora.BAD_INTEGER, 0, 0), "int1": (ora.BAD_INTEGER, 1, 1),
                                         "int2": (ora.BAD_INTEGER, 2, None), "int6": (ora.BAD_INTEGER, 6, 6), "int7": (ora.BAD_INTEGER, 7, 7)}.items():
        for where, line in (("first", 1), ("last", n_good + 1), ("last_no_newline", n_good + 1)):
            if name == "empty" and where == "last_no_newline":
                assert d("empty_last_no_newline")["stop_kind"] == 0          # (no line at all)
                continue
            assert stop(d("%s_%s" % (name, where))) == (line, kind, dfield, 0), (name, where)
            if rfield is not None:
                assert stop(r("%s_%s" % (name, where))) == (line, kind, rfield, 0), (name, where)
    assert stop(d("empty_line_middle")) == (7, ora.FEW_FIELDS, -1, 0)
    assert stop(d("missing_end_first_run")) == (2, ora.MISSING_END, -1, 4) and stop(d("missing_end_last_run")) == (n_good + 1, ora.MISSING_END, -1, 5)
    assert stop(d("two_stops")) == (5, ora.MISSING_END, -1, 5) and stop(d("two_line_stops")) == (5, ora.BAD_INTEGER, 6, 0)
    assert stop(d("bad_line_and_missing_end_in_one_run")) == (6, ora.BAD_INTEGER, 6, 0)
    assert stop(d("bad_id_behind_a_missing_end")) == (5, ora.MISSING_END, -1, 4)
    assert stop(d("bad_position_opens_a_new_run")) == (5, ora.MISSING_END, -1, 4)
    assert d("cr_on_plus_line")["stop_kind"] == 0 and stop(r("cr_on_plus_line")) == (1, ora.BAD_INTEGER, 7, 0)
    assert stop(d("cr_on_minus_line")) == (2, ora.BAD_INTEGER, 7, 0) and stop(r("cr_on_minus_line")) == (2, ora.BAD_INTEGER, 7, 0)
    assert d("cr_newlines")["stop_kind"] == 0 and got["cr_newlines"][1][1].count(b"\r\n") == 2 and r("cr_newlines")["stop_kind"] == 0
    assert d("eight_and_twelve_fields")["n_kept_fragments"] == 2 and got["eight_and_twelve_fields"][2][1].endswith(b"1\t1\tc\t+\t-40\t9\n")
    assert d("ignored_position_field")["stop_kind"] == 0 and r("ignored_position_field")["stop_kind"] == ora.BAD_INTEGER
    assert b"N" * 300 in got["long_name"][1][1] and bytes(range(32, 256)) * 2 in got["long_name"][2][1] and max(len(l) for l in got["long_line"][0]["text"].split(b"\n")) >= 5000
    assert got["empty_name_and_odd_strands"][2][1] == b"1\t0\t\t+-\t5\t10\n1\t1\t\x00\xff\t\x00\t6\t11\n"


def test_oracle_is_the_host_tool(glue, tmp_path):
    """bin/defuse_glue remove_duplicates and get_align_regions on every shape case and two random texts: the oracle's bytes
    where it does not stop, a non-zero status where it does."""
    path = tmp_path / "in.txt"

    def tool(args, data):
        path.write_bytes(data)
        with open(path, "rb") as fh:
            return subprocess.run([glue] + args, stdin=fh, capture_output=True, timeout=120)

    cases = shape_cases() + [dict(name="random_%d" % s, text=random_text(s), min=2) for s in (1, 2)]
    n_stops = 0
    for c in cases:
        if not INT_MIN <= c["min"] <= INT_MAX:            # the tool reads its threshold as an int
            continue
        res, text = ora.dedup(c["text"], c["min"])
        r = tool(["remove_duplicates", str(c["min"])], c["text"])
        if text is None:
            assert r.returncode != 0 and r.stdout == b"", c["name"]
            n_stops += 1
        else:
            assert r.returncode == 0 and r.stdout == text, c["name"]
        for source in (c["text"], text):
            if source is None:
                continue
            res, rtext = ora.regions(source)
            r = tool(["get_align_regions"], source)
            if rtext is None:
                assert r.returncode != 0 and r.stdout == b"", c["name"]
                n_stops += 1
            else:
                assert r.returncode == 0 and r.stdout == rtext, c["name"]
    assert n_stops >= 40


HOST = r'''
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "%(root)s/tools_src/defuse_host.hpp"
#include "%(root)s/defuse_amd/csrc/taskc_shared.hpp"
struct HostInt {
    bool operator()(const uint8_t* p, int64_t n, int& v) const { return n >= 0 && defuse::field_int(reinterpret_cast<const char*>(p), (size_t)n, v); }
};
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::string data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    int64_t s = 0;
    while (s < (int64_t)data.size()) {
        int64_t e = s;
        while (e < (int64_t)data.size() && data[(size_t)e] != '\n') ++e;
        // an exact copy of the line on the heap: a read beyond it is a report
        std::vector<uint8_t> line(data.begin() + s, data.begin() + e);
        const taskc_line r = taskc_parse_line(line.data(), 0, (int64_t)line.size(), HostInt());
        printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", r.dkind, r.dfield, r.rkind, r.rfield, r.id, r.ce, r.frag, r.pos, r.start, r.end, r.name_off,
               r.name_len, r.strand_off, r.strand_len);
        s = e + 1;
    }
    uint8_t buf[12];
    const int32_t vals[] = {0, 7, -7, 10, 99, 100, -100, 2147483647, (int32_t)-2147483648LL, 1000000000, 999999999};
    for (int32_t v : vals) {
        const int n = taskc_dec_put(v, buf);
        if (n != taskc_dec_len(v) || std::string((const char*)buf, (size_t)n) != std::to_string(v)) return 3;
    }
    return 0;
}
'''


def test_shared_header_as_a_host_program(tmp_path):
    """taskc_shared.hpp compiled by g++ into a stand-alone program under ASan + UBSan, with the host's own field_int: on every
    line of every shape case it gives the oracle's per-line result, without a report."""
    from tests.test_sanitizers import BAD, ENV
    src = tmp_path / "taskc_host.cpp"
    src.write_text(HOST % {"root": ROOT})
    exe = str(tmp_path / "taskc_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, str(src)])
    path = tmp_path / "case.txt"
    n = 0
    keys = ("dkind", "dfield", "rkind", "rfield", "id", "ce", "frag", "pos", "start", "end", "name_off", "name_len", "strand_off", "strand_len")
    for c in shape_cases() + [dict(name="random", text=random_text(3, 400))]:
        path.write_bytes(c["text"])
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV["asan"]), stdin=subprocess.DEVNULL, timeout=120)
        assert not any(b in r.stderr for b in BAD), (c["name"], r.stderr[-3000:])
        assert r.returncode == 0, (c["name"], r.returncode, r.stderr[-2000:])
        rows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        want = [[ora.parse_line(line)[k] for k in keys] for _, line in ora.lines_of(c["text"])]
        assert rows == want, c["name"]
        n += len(rows)
    assert n > 3000


def test_tool_refuses_cleanly_without_a_gpu(glue, tmp_path):
    """Bad arguments print the usage; with arguments in order and no usable device the status is 1 and neither file exists.
    (DEFUSE_GPU names a device no machine has, so this is the same run with and without a GPU.)"""
    c, r = tmp_path / "c.out", tmp_path / "r.out"
    inp = os.path.join(GOLDEN, "cluster_regions", "clusters1_in.txt")
    for args in ([], ["3"], ["x", "-c", str(c), "-r", str(r)], ["3", "-c", str(c)], ["3", "-c", str(c), "-r"], ["3", "-c", str(c), "-r", str(r), inp, "more"]):
        p = subprocess.run([glue, "cluster_regions"] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        assert p.returncode == 1 and p.stderr.startswith("Usage: cluster_regions"), args
    assert "cluster_regions" in subprocess.run([glue], capture_output=True, text=True).stderr
    link = tmp_path / "cluster_regions.pl"
    os.symlink(glue, link)
    for exe in ([glue, "cluster_regions"], [str(link)]):
        p = subprocess.run(exe + ["3", "-c", str(c), "-r", str(r), inp], capture_output=True, text=True, env=dict(os.environ, DEFUSE_GPU="999"))
        assert p.returncode == 1 and "taskc_create" in p.stderr and p.stdout == "" and not c.exists() and not r.exists()


# ---------------------------------------------------------------------------------------------- GPU
def refused(cr, call):
    with pytest.raises(cr.ClusterRegionsError) as e:
        call()
    assert e.value.code == E_ARG, str(e.value)


def run_case(cr, ctx, case):
    """The input's regions, the dedup and the dedup text's regions of a case on `ctx` against the oracle."""
    name, text = case["name"], case["text"]
    feed(ctx, text, case.get("pieces"))
    for source, data in ((cr.INPUT, text), (cr.DEDUP, None)):
        if source == cr.DEDUP:
            want, data = ora.dedup(text, case["min"])
            assert ctx.dedup(case["min"]) == want, name
            refused(cr, lambda: ctx.fetch(cr.REGIONS))                   # a dedup drops the regions text
            if data is None:
                refused(cr, lambda: ctx.fetch(cr.DEDUP))
                refused(cr, lambda: ctx.regions(cr.DEDUP))
                return
            assert ctx.fetch(cr.DEDUP) == data, name
            if len(data) > 10:
                assert ctx.fetch(cr.DEDUP, 3, 7) == data[3:10]
        want, rtext = ora.regions(data)
        assert ctx.regions(source) == want, (name, source)
        if rtext is None:
            refused(cr, lambda: ctx.fetch(cr.REGIONS))
        else:
            assert ctx.fetch(cr.REGIONS) == rtext, (name, source)
    t = ctx.timing()
    assert t["text_bytes"] == len(text) and all(t[k] >= 0 for k in t)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_shape_cases_on_the_gpu(cr, group):
    """Result structs, dedup bytes, regions bytes and stop fields of every shape case equal the oracle's; one ctx for all cases
    of a group, so every case but the first also runs on a used ctx."""
    cases = [c for c in shape_cases() if c["group"] == group]
    assert len(cases) >= 3
    with cr.Context() as ctx:
        for case in cases:
            run_case(cr, ctx, case)


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [None, 64])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_texts_on_the_gpu(cr, seed, pieces):
    text = random_text(seed)
    res, _ = ora.dedup(text, 2)
    assert 1900 <= text.count(b"\n") < 2100 and len(text) < 200000 and res["n_kept_fragments"] < res["n_fragments"] and 0 < res["n_kept_runs"] < res["n_runs"]
    with cr.Context() as ctx:
        run_case(cr, ctx, dict(name="random_%d" % seed, text=text, min=2, pieces=pieces))


@pytest.mark.gpu
def test_reuse(cr):
    """One ctx through begin, add, dedup and regions several times, larger and smaller texts, after stops, and dedup twice."""
    cases = {c["name"]: c for c in shape_cases()}
    with cr.Context() as ctx:
        refused(cr, lambda: ctx.regions(cr.DEDUP))
        for name in ("run_of_129", "run_of_1", "int6_last", "one_line_per_piece", "missing_end_first_run", "empty", "cr_on_plus_line", "run_over_two_workgroups", "min_3"):
            run_case(cr, ctx, cases[name])
        text = cases["min_3"]["text"]
        for m, kept in ((4, 0), (0, 5), (3, 3)):
            assert ctx.dedup(m)["n_kept_fragments"] == kept and ctx.fetch(cr.DEDUP) == ora.dedup(text, m)[1]
        assert ctx.regions(cr.DEDUP)["n_clusters"] == 1 and ctx.regions(cr.INPUT)["n_clusters"] == 2


def chain_clusters():
    """A cluster file over the smoke regions: per region pair one cluster the set cover keeps, whose extent is the region's, with
    PCR duplicates and a (fragment, end) given twice; and clusters of the same fragments that the set cover drops."""
    regs = defaultdict(dict)
    for l in open(os.path.join(SMOKE, "regions.txt"), "rb").read().splitlines():
        f = l.split(b"\t")
        regs[int(f[0])][int(f[1])] = (f[2], f[3], int(f[4]), int(f[5]))
    lines, frag = [], 0
    for cid, ends in sorted(regs.items()):
        frags = list(range(frag, frag + 6))
        frag += 6
        for k, fr in enumerate(frags):
            for e in (0, 1):
                name, strand, start, end = ends[e]
                a = start + max(k - 2, 0)                                            # 0, 1 and 2 are duplicates, and have the region's extent
                b = end - max(k - 2, 0)
                lines.append(cl(cid, e, fr, name, strand, a, b, re=e))
        lines.append(cl(cid, 0, frags[3], ends[0][0], ends[0][1], ends[0][2] + 2, ends[0][3] - 2))          # fragment 3's end 0 again
        other = 1000 + cid                                                            # a smaller cluster of the same fragments: dropped by the cover
        for fr in frags[:2]:
            for e in (0, 1):
                lines.append(cl(other, e, fr, b"chrA", b"+", 1, 50, re=e))
    return b"".join(lines)


@pytest.mark.gpu
def test_chain_from_cover_to_store(cr):
    """sct_add / sct_cover, taskc_add_cover, taskc_dedup, taskc_regions(TASKC_DEDUP), taskc_parse_regions, taskt_store_create
    against the host route on the fetched bytes: sct_fetch, the oracle's two steps, taskt_parse_regions, taskt_store_create."""
    from defuse_amd import sctext, tasktext as tt
    from oracle import dosplitalign_oracle as dora
    from tests import tasktext_oracle as tora
    from tests.test_task_store import int_params
    d = SMOKE + "/"
    exon_text = open(d + "exons.txt", "rb").read()
    seqs = OrderedDict(dora.FastaIndex(d + "ref.fa").seqs)
    _, T = tora.parse_exons(exon_text, [])
    ref_names = T.chroms + [T.table[t][0] + b"|" + t for t in T.names]
    clusters = chain_clusters()
    with sctext.SctContext() as cover, cr.Context() as ctx, tt.Context() as mine, tt.Context() as theirs, tt.task.Reference(seqs) as ref, tt.Names(ref_names) as rn, \
            tt.Names(list(seqs)) as sn:
        cover.begin()
        refused(cr, lambda: ctx.add_cover(cover))                        # no cover yet
        cover.add(clusters)
        refused(cr, lambda: ctx.add_cover(cover))
        res = cover.cover(3)
        covered = cover.fetch()
        assert res["status"] == sctext.OK and 0 < len(covered) < len(clusters)
        ctx.begin()
        ctx.add_cover(cover)
        cover.begin()                                                    # the cover may be reused: the text was copied
        want_d, dedup_text = ora.dedup(covered, 3)
        assert ctx.dedup(3) == want_d and want_d["n_kept_fragments"] < want_d["n_fragments"] and ctx.fetch(cr.DEDUP) == dedup_text
        want_r, region_text = ora.regions(dedup_text)
        assert ctx.regions(cr.DEDUP) == want_r and ctx.fetch(cr.REGIONS) == region_text
        assert sorted(region_text.splitlines()) == sorted(open(d + "regions.txt", "rb").read().splitlines())
        for t in (mine, theirs):
            assert t.parse_exons(rn, exon_text)["stop_line"] == 0
        got = ctx.parse_regions(mine, sn)
        assert got == theirs.parse_regions(sn, region_text) and got["n_items"] == want_r["n_clusters"] > 0
        (pa, la), (pb, lb) = mine.pairs(), theirs.pairs()
        assert pa.tobytes() == pb.tobytes() and la.tolist() == lb.tolist()
        with mine.store(ref, int_params((300, 30, 50, 50))) as a, theirs.store(ref, int_params((300, 30, 50, 50))) as b:
            for x, y in zip(a.fetch(), b.fetch()):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes() and len(x) > 0
        with sctext.SctContext() as none:
            refused(cr, lambda: ctx.add_cover(none))


def run_tool(glue, tmp_path, data, min_size, env=None):
    inp, c, r = tmp_path / "in.txt", tmp_path / "c.out", tmp_path / "r.out"
    for f in (c, r):
        if f.exists():
            f.unlink()
    inp.write_bytes(data)
    p = subprocess.run([glue, "cluster_regions", str(min_size), "-c", str(c), "-r", str(r), str(inp)], capture_output=True, text=True,
                       env=dict(os.environ, DEFUSE_GLUE_PIECE_BYTES="64", **(env or {})), timeout=120)
    return p, c, r


@pytest.mark.gpu
def test_tool_writes_the_two_host_steps_files(glue, tmp_path):
    """On the goldens and one random text, in pieces of 64 bytes: byte-identical to remove_duplicates | get_align_regions."""
    texts = [(open(os.path.join(GOLDEN, name), "rb").read(), m) for name, m in (("glue/dups_in.txt", 3), ("cluster_regions/clusters1_in.txt", 2),
                                                                                ("cluster_regions/clusters2_in.txt", 2))] + [(random_text(5), 2)]
    for k, (data, m) in enumerate(texts):
        p, c, r = run_tool(glue, tmp_path, data, m, env={"DEFUSE_TIMING": "1"} if k == 0 else None)
        assert p.returncode == 0 and p.stdout == "", p.stderr
        assert ("[cluster_regions] device: upload" in p.stderr) == (k == 0)
        host_c = subprocess.run([glue, "remove_duplicates", str(m)], input=data, capture_output=True, check=True).stdout
        host_r = subprocess.run([glue, "get_align_regions"], input=host_c, capture_output=True, check=True).stdout
        assert c.read_bytes() == host_c and r.read_bytes() == host_r and len(host_r) > 0
    p, c, r = run_tool(glue, tmp_path, b"", 2)                           # stdin would be read without FILE; an empty file: two empty files
    assert p.returncode == 0 and c.read_bytes() == b"" and r.read_bytes() == b""
    with open(os.path.join(GOLDEN, "cluster_regions", "clusters1_in.txt"), "rb") as fh:
        p = subprocess.run([glue, "cluster_regions", "2", "-c", str(c), "-r", str(r)], stdin=fh, capture_output=True, text=True)
    assert p.returncode == 0 and c.read_bytes() == ora.dedup(texts[1][0], 2)[1]


@pytest.mark.gpu
def test_tool_declines_a_stopping_text(glue, tmp_path):
    cases = {c["name"]: c for c in shape_cases()}
    for name, words in (("int6_last", ["clusters line 11", "field 7"]), ("missing_end_first_run", ["clusters line 2", "fragment 4"]),
                        ("cr_on_plus_line", ["kept clusters line 1", "field 8"]), ("few_first", ["clusters line 1", "fewer than eight"])):
        p, c, r = run_tool(glue, tmp_path, cases[name]["text"], 1)
        assert p.returncode == 3 and p.stdout == "" and all(w in p.stderr for w in words) and len(p.stderr.splitlines()) == 1, (name, p.stderr)
        assert not c.exists() and not r.exists(), name
