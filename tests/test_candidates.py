"""The candidate loop of DoAlignment on the GPU (include/defuse_cand.h through defuse_amd/cand.py) against
oracle/dosplitalign_oracle.py: BinnedLocations(2000).overlapping for the ids of an alignment, visited ascending as signed
int, and the first-come de-duplication on (fusion, fragment, read_end, revcomp) restated below.  Every comparison is exact
equality of the candidate tuples (alignment, fusion, fragment, cluster_end, read_end, revcomp, first), in order."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "tests", "golden", "smoke")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4


@pytest.fixture(scope="module")
def cand(built):
    from defuse_amd import cand as c
    return c


@pytest.fixture(scope="module")
def ora(built):
    from oracle import dosplitalign_oracle as o
    return o


def cid(fusion, end):
    from oracle import dosplitalign_oracle as o
    return o.cluster_id(fusion, end)


def oracle_table(regs, spacing=2000):
    """Rows (ref, strand, start, end, id) in the oracle's BinnedLocations."""
    from oracle import dosplitalign_oracle as o
    binned = o.BinnedLocations(spacing)
    for ref, strand, start, end, i in regs:
        binned.add(int(i), dict(refName=int(ref), strand=int(strand), start=int(start), end=int(end)))
    return binned


def oracle_candidates(binned, als, seen, base=0, visited=None):
    """tools/SplitAlignment.cpp:266-303 on rows (ref, strand, start, end, fragment, read_end): ids ascending as signed int,
    first come, first kept in `seen` (which it extends).  `visited` (a list) receives the number of ids of each alignment."""
    out = []
    for k, (ref, strand, start, end, frag, rend) in enumerate(als):
        first = 1
        ids = binned.overlapping(int(ref), int(strand), int(start), int(end))
        if visited is not None:
            visited.append(len(ids))
        for i in sorted(ids):
            cend = 1 if i < 0 else 0
            key = (i & 0x7FFFFFFF, int(frag), 1 if rend == 0 else 0, 1 if cend == 0 else 0)
            if key in seen:
                continue
            seen.add(key)
            out.append((base + k, key[0], key[1], cend, key[2], key[3], first))
            first = 0
    return out


def tuples(recs):
    return [(int(r["alignment"]), int(r["fusion_id"]), int(r["fragment"]), int(r["cluster_end"]), int(r["read_end"]), int(r["revcomp"]),
             int(r["first"])) for r in recs]


def by_fusion(exp):
    return sorted(exp, key=lambda t: t[1])          # stable: visiting order inside a fusion


# ---------------------------------------------------------------------------------------------- CPU
def test_struct_layouts_match_header(cand):
    """sizeof and offsetof of every struct of the header, as a C++ and a C compiler see them, against the ctypes structs."""
    sizes, _ = abi.check("defuse_cand.h", cand, r"cand_[a-z_]+")
    assert sizes == [20, 24, 24, 48]
    assert (cand.REGION_DTYPE.itemsize, cand.ALIGNMENT_DTYPE.itemsize, cand.RECORD_DTYPE.itemsize) == (20, 24, 24)
    assert ctypes.sizeof(cand.CandTiming) == 48


def test_library_exports_cand(cand):
    assert abi.check_functions("defuse_cand.h", cand, r"cand_[a-z_]+") == 8


def test_argument_errors_need_no_device(cand):
    """Every argument error is found before a device is touched: the code is DSA_E_ARG with or without a GPU."""
    lib = cand.lib()
    err = lambda: lib.cand_last_error().decode()
    table = ctypes.c_void_p()
    one = cand.regions([(0, 0, 100, 200, 5)])

    def create(regs, n, spacing):
        return lib.cand_table_create(0, regs.ctypes.data if len(regs) else None, n, spacing, ctypes.byref(table))
    for spacing in (0, -2000, INT_MIN):
        assert create(one, 1, spacing) == E_ARG and "bin_spacing" in err() and not table
    assert create(one, -1, 2000) == E_ARG and "negative" in err()
    assert create(cand.regions([(0, 2, 100, 200, 5)]), 1, 2000) == E_ARG and "strand" in err()
    assert create(cand.regions([(0, 0, 1, 2, 5), (0, -1, 100, 200, 5)]), 2, 2000) == E_ARG and "region 1" in err()
    assert create(cand.regions([(-1, 0, 100, 200, 5)]), 1, 2000) == E_ARG and "reference" in err()
    # fusion ids: where a caller packs one into a ClusterID
    out = ctypes.c_int32()
    for fusion in (-1, 2 ** 31, 2 ** 40):
        assert lib.cand_cluster_id(fusion, 0, ctypes.byref(out)) == E_ARG and "fusion id" in err()
        with pytest.raises(cand.CandError) as e:
            cand.cluster_id(fusion, 1)
        assert e.value.code == E_ARG
    assert lib.cand_cluster_id(7, 2, ctypes.byref(out)) == E_ARG and "cluster end" in err()
    for fusion, end in ((0, 0), (0, 1), (INT_MAX, 0), (INT_MAX, 1), (12345, 1)):
        assert cand.cluster_id(fusion, end) == cid(fusion, end)
    # alignments are checked before the session is looked at
    n_out = ctypes.c_int64(-7)

    def enum(als, n, order=0):
        return lib.cand_enumerate(None, als.ctypes.data if len(als) else None, n, order, None, 0, ctypes.byref(n_out), None)
    good = (0, 0, 100, 200, 9, 0)
    assert enum(cand.alignments([good, (0, 0, 100, 200, -1, 0)]), 2) == E_ARG and "fragment" in err() and "alignment 1" in err()
    assert n_out.value == 0
    assert enum(cand.alignments([(0, 0, 100, 200, INT_MIN, 0)]), 1) == E_ARG and "fragment" in err()
    assert enum(cand.alignments([(0, 2, 100, 200, 9, 0)]), 1) == E_ARG and "strand" in err()
    assert enum(cand.alignments([(0, -1, 100, 200, 9, 0)]), 1) == E_ARG and "strand" in err()
    assert enum(cand.alignments([(0, 0, 100, 200, 9, 2)]), 1) == E_ARG and "read_end" in err()
    assert enum(cand.alignments([good]), -1) == E_ARG and "negative" in err()
    assert enum(cand.alignments([good]), 1, order=2) == E_ARG and "order" in err()
    assert enum(cand.alignments([good]), 1) == E_ARG and "session" in err()
    assert enum(cand.alignments([]), 2 ** 31) == E_LIMIT
    assert lib.cand_session_create(None, ctypes.byref(table)) == E_ARG and lib.cand_session_reset(None) == E_ARG


def too_many_entries(cand):
    """Three regions over the whole int range at spacing 1: 3 * 2^32 (region, bin) entries."""
    lib = cand.lib()
    table = ctypes.c_void_p()
    regs = cand.regions([(0, 0, INT_MIN, INT_MAX, 1), (0, 1, INT_MIN, INT_MAX, 2), (1, 0, INT_MIN, INT_MAX, 3)])
    rc = lib.cand_table_create(0, regs.ctypes.data, len(regs), 1, ctypes.byref(table))
    assert rc == E_LIMIT and not table and str(3 * 2 ** 32) in lib.cand_last_error().decode()
    # one entry above the limit: 2^31 bins
    regs = cand.regions([(0, 0, 0, INT_MAX, 1)])
    assert lib.cand_table_create(0, regs.ctypes.data, 1, 1, ctypes.byref(table)) == E_LIMIT and not table


def test_entry_total_is_formed_in_64_bits(cand):
    too_many_entries(cand)


# ---------------------------------------------------------------------------------------------- GPU
def check(cand, regs, als, spacing=2000):
    """One table, one session, both orders against the oracle; returns the expected tuples in visiting order."""
    exp = oracle_candidates(oracle_table(regs, spacing), als, set())
    with cand.Table(cand.regions(regs), spacing) as table:
        for order, want in ((cand.ORDER_VISIT, exp), (cand.ORDER_FUSION, by_fusion(exp))):
            with table.session() as s:
                got = s.enumerate(cand.alignments(als), order)
                assert tuples(got) == want
                assert (s.timing.n_alignments, s.timing.n_kept) == (len(als), len(exp))
                assert s.timing.n_hits >= s.timing.n_visited >= s.timing.n_kept
    return exp


@pytest.mark.gpu
def test_rules_one_by_one(cand):
    A, B = cid(3, 0), cid(3, 1)
    # (a) an alignment over two bins finds a region that sits in both of them once
    exp = check(cand, [(0, 0, 1900, 2100, A)], [(0, 0, 1950, 2050, 7, 0)])
    assert exp == [(0, 3, 7, 0, 1, 1, 1)]
    # (b) two regions with one id both hit: the id comes once
    assert len(check(cand, [(0, 0, 100, 300, A), (0, 0, 200, 400, A)], [(0, 0, 250, 260, 7, 1)])) == 1
    # (c) both cluster ends: the negative ids (end 1) are visited first.  Inside one alignment two ids never share a key
    # (another end is another revcomp), so the collision comes from a second alignment of the same read: the end-1
    # candidate of fusion 3 was kept for alignment 0 and is dropped there, the end-0 candidate of fusion 5 is new
    regs = [(0, 0, 100, 300, A), (0, 0, 100, 300, B), (0, 0, 100, 300, cid(4, 1)), (0, 0, 5000, 5100, cid(3, 1)), (0, 0, 5000, 5100, cid(5, 0))]
    exp = check(cand, regs, [(0, 0, 150, 160, 7, 0), (0, 0, 5050, 5060, 7, 0)])
    assert [(t[0], t[1], t[3]) for t in exp] == [(0, 3, 1), (0, 4, 1), (0, 3, 0), (1, 5, 0)]
    assert [t[6] for t in exp] == [1, 0, 0, 1]
    # (d) start > end inside one bin is found
    assert len(check(cand, [(0, 0, 1500, 1400, A)], [(0, 0, 1300, 1600, 7, 0)])) == 1
    # (e) an empty bin range is never found, although the coordinates pass the overlap test
    assert check(cand, [(0, 0, 2100, 1900, A)], [(0, 0, 1800, 2200, 7, 0)]) == []
    # (f) truncating division: [100, -100] is in bin 0..0, [-150, 120] looks into bin 0..0; floor division would look into -1..0
    # for the alignment but enter the region nowhere (0 > -1)
    assert len(check(cand, [(0, 0, 100, -100, A)], [(0, 0, -150, 120, 7, 0)])) == 1
    # (g) alignments with end < start: bin range empty (2100 -> 1900), and non-empty (1600 -> 1300: bin 0..0)
    regs = [(0, 0, 1000, 3000, A)]
    assert check(cand, regs, [(0, 0, 2100, 1900, 7, 0)]) == []
    assert len(check(cand, regs, [(0, 0, 1600, 1300, 7, 0)])) == 1
    assert check(cand, [(0, 0, 1700, 1800, A)], [(0, 0, 1600, 1300, 7, 0)]) == []           # same bin, fails the overlap test
    # (h) a name the table lacks, a ref present on the other strand only, bins outside the ref's bins on either side
    regs = [(0, 0, 4000, 9000, A), (1, 1, 4000, 9000, B), (2, 0, 100, 200, cid(9, 0))]
    als = [(-1, 0, 4500, 4600, 7, 0), (1, 0, 4500, 4600, 7, 0), (0, 1, 4500, 4600, 7, 0), (0, 0, 100, 1999, 7, 0), (0, 0, 10000, 20000, 7, 0),
           (3, 0, 100, 200, 7, 0), (0, 0, -9000, -2000, 7, 0), (0, 0, 3999, 4000, 8, 0), (1, 1, 9000, 9001, 8, 0)]
    exp = check(cand, regs, als)
    assert [(t[0], t[1]) for t in exp] == [(7, 3), (8, 3)]
    # (i) a huge range on a small table: clamped to the bins the table has
    regs = [(0, 0, 100, 300, A), (0, 0, -5000, -4000, B), (0, 0, 900000, 900100, cid(4, 0)), (0, 1, 100, 300, cid(5, 0))]
    exp = check(cand, regs, [(0, 0, INT_MIN // 2, INT_MAX // 2, 7, 0), (0, 0, INT_MIN, INT_MAX, 8, 0)])
    assert [(t[0], t[1], t[3]) for t in exp] == [(0, 3, 1), (0, 3, 0), (0, 4, 0), (1, 3, 1), (1, 3, 0), (1, 4, 0)]
    # (j) an empty table, n = 0, and a table whose only region is in no bin
    assert check(cand, [], [(0, 0, 100, 200, 7, 0)]) == []
    assert check(cand, [(0, 0, 100, 300, A)], []) == []
    assert check(cand, [], []) == []


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """300 regions on 3 refs x 2 strands, ids of 40 fusions x 2 ends, about 5 % with start > end; 4000 alignments of length
    1-4500 of 200 fragments x 2 read ends.  Returns (regions, alignments, the oracle's candidates in visiting order)."""
    rng = np.random.default_rng(seed)
    regs = []
    for _ in range(300):
        a, b = sorted(int(x) for x in rng.integers(-6000, 12001, size=2))
        if rng.random() < 0.6:
            b = min(b, a + int(rng.integers(0, 3000)))
        if rng.random() < 0.05:
            a, b = b, a
        regs.append((int(rng.integers(0, 3)), int(rng.integers(0, 2)), a, b, cid(int(rng.integers(0, 40)), int(rng.integers(0, 2)))))
    als = []
    for _ in range(4000):
        length = int(rng.integers(1, 4501))
        start = int(rng.integers(-6000, 12001 - length + 1))
        als.append((int(rng.integers(0, 3)), int(rng.integers(0, 2)), start, start + length - 1, int(rng.integers(0, 200)), int(rng.integers(0, 2))))
    visited = []
    exp = oracle_candidates(oracle_table(regs), als, set(), visited=visited)
    return tuple(regs), tuple(als), tuple(exp), sum(visited)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_against_oracle(cand, seed):
    regs, als, exp, n_visited = random_case(seed)
    assert any(a > b for _, _, a, b, _ in regs) and any(t[3] for t in exp) and any(not t[3] for t in exp)
    assert n_visited > 2 * len(exp) > 1000                    # the de-duplication drops most visited hits
    with cand.Table(cand.regions(regs)) as table:
        with table.session() as s:
            got = tuples(s.enumerate(cand.alignments(als), cand.ORDER_VISIT))
            assert (s.timing.n_visited, s.timing.n_kept) == (n_visited, len(exp)) and s.timing.n_hits > n_visited
        with table.session() as s:
            got_f = tuples(s.enumerate(cand.alignments(als), cand.ORDER_FUSION))
    assert got == list(exp)
    assert got_f == by_fusion(exp) and got_f != got


@pytest.mark.gpu
def test_sessions(cand):
    regs, als, exp, _ = random_case(1)
    a = cand.alignments(als)
    with cand.Table(cand.regions(regs)) as table:
        s, other = table.session(), table.session()
        parts = [a[:1300], a[1300:1300], a[1300:1777], a[1777:]]
        got = [t for p in parts for t in tuples(s.enumerate(p))]
        assert got == list(exp)
        assert len(s.enumerate(a)) == 0                          # everything was kept before
        s.reset()
        assert tuples(s.enumerate(a)) == list(exp)               # the count starts at 0 again too
        # the other session has seen nothing of this; by fusion in pieces = each piece's candidates by fusion
        seen, want = set(), []
        binned = oracle_table(regs)
        for lo, hi in ((0, 2500), (2500, 4000)):
            want += by_fusion(oracle_candidates(binned, als[lo:hi], seen, base=lo))
        assert [t for lo, hi in ((0, 2500), (2500, 4000)) for t in tuples(other.enumerate(a[lo:hi], cand.ORDER_FUSION))] == want
        other.close()
        s.close()


@pytest.mark.gpu
def test_capacity_protocol(cand):
    regs, als, _, _ = random_case(2)
    binned, seen = oracle_table(regs), set()
    first = oracle_candidates(binned, als[:2000], seen)
    second = oracle_candidates(binned, als[2000:], seen, base=2000)
    assert len(first) > 100 and len(second) > 10
    a = cand.alignments(als)
    with cand.Table(cand.regions(regs)) as table, table.session() as s:
        rc, n = s.count(a[:2000])                                # cap = 0, out = NULL
        assert (rc, n) == (E_CAPACITY, len(first))
        buf = np.frombuffer(bytearray(b"\x55" * ((n - 1) * cand.RECORD_DTYPE.itemsize)), dtype=cand.RECORD_DTYPE)
        assert s.enumerate_into(a[:2000], buf) == (E_CAPACITY, n)
        assert len(buf) == n - 1 and buf.tobytes() == b"\x55" * buf.nbytes          # nothing else was written
        out = np.zeros(n, dtype=cand.RECORD_DTYPE)
        assert s.enumerate_into(a[:2000], out) == (0, n)
        assert tuples(out) == first                              # alignment indices from 0: the refused calls counted nothing
        assert tuples(s.enumerate(a[2000:])) == second           # and this one de-duplicates against what the successful one kept


@pytest.mark.gpu
def test_entry_limit_on_device(cand):
    """DSA_E_LIMIT before anything of that size is allocated (3 * 2^32 entries would be 48 GiB of keys alone), and the
    device is usable afterwards."""
    too_many_entries(cand)
    assert len(check(cand, [(0, 0, -3, 3, 1)], [(0, 0, 0, 0, 7, 0)], spacing=1)) == 1


@pytest.mark.gpu
def test_smoke_vector_through_the_library(cand, ora, gpu_ctx):
    """SAM records -> candidates (cand) -> DP records (dsa) on the reference's known-answer vector."""
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
    als = [(names.get(rname, -1), strand, start, end, ora.lexical_cast_int(frag), rend)
           for frag, rend, rname, strand, start, end in ora.sam_alignments(d + "improper.sam")]
    windows = {t.fusion_id: (t.seq[0], t.seq[1]) for t in tasks.values()}
    want = [(t.fusion_id, frag, rend, revcomp) for t, frag, rend, revcomp, _ in ora.enumerate_candidates(tasks, reads, d + "improper.sam")]
    exp = [tuple(int(x) for x in l.split()) for l in open(d + "expected.split.align.txt")]
    assert len(want) > 5
    with cand.Table(cand.regions(regs)) as table:
        for order in (cand.ORDER_VISIT, cand.ORDER_FUSION):
            with table.session() as s:
                cands = s.enumerate(cand.alignments(als), order)
            got = [(int(c["fusion_id"]), int(c["fragment"]), int(c["read_end"]), int(c["revcomp"])) for c in cands]
            assert got == (want if order == cand.ORDER_VISIT else sorted(want, key=lambda t: t[0]))
            recs = gpu_ctx.align_batch(*cand.dsa_batch(cands, reads, windows))
            lines = [tuple(int(r[f]) for f in recs.dtype.names[:9]) for r in recs]
            if order == cand.ORDER_VISIT:
                assert lines == exp                               # the reference's own order, no sort needed
            assert sorted(lines) == sorted(exp)
