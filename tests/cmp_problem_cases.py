"""The checker and the inputs of tests/test_cmp_problems.py (test infrastructure).

`problems_of` restates the host stages of clustermatepairs between the bin pairs and MatePairEM the way the oracle runs them
inline (oracle/clustermatepairs_oracle.py:581-624: the two size checks, FilterUnmatched, FilterOverlapping, GetAlignPairs,
strand_remap) and adds what the tool hands to the EM with them: x, y, u and the two ranks (stable sorts, descending).  It
takes the map of bin pairs of tests/test_cmp_bins.py:oracle_bin_pairs — {(id1, id2): ([(fragment, read end, relative start,
relative end), ...], [...])} — or one written by hand.  `select_rows` is the rule by which the tool picks the lines of a
cluster (:630-643).  Nothing here touches a GPU."""
import os
import struct
import subprocess

import numpy as np

from oracle import clustermatepairs_oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "clustermatepairs")
BIN_LENGTH = ora.BIN_LENGTH
PACKED = np.dtype([("fragment", "<i4"), ("read_end", "<i4"), ("rel_start", "<u2"), ("rel_end", "<u2")])
PAIR = np.dtype([("first", "<i4"), ("second", "<i4")])


def unpack(pid, packed):
    ref, strand, b = pid & 0x3FFFF, (pid >> 18) & 1, pid >> 19
    return [dict(frag=f, readEnd=e, ref=ref, strand=strand, region=(rs + b * BIN_LENGTH - BIN_LENGTH // 2, re_ + b * BIN_LENGTH - BIN_LENGTH // 2))
            for (f, e, rs, re_) in packed]


def ranks_desc(v):
    """rank of every element when sorted descending, ties by index ascending"""
    order = sorted(range(len(v)), key=lambda i: -v[i])            # sorted() is stable
    r = [0] * len(v)
    for k, i in enumerate(order):
        r[i] = k
    return r


def problems_of(bin_pairs, min_fusion_range, min_cluster_size, fragment_mean):
    """-> dict: prob_off, x, y, u, to_xo, to_yo, pairs, bin_pair (numpy, the dtypes of cmp_problems_fetch), n_candidates, and
    per problem the unpacked alignment lists (`als`) and the fragment of every mate pair (`frags`)."""
    prob_off, xs, ys, us, txo, tyo, pairs_all, bin_pair, als, frags = [0], [], [], [], [], [], [], [], [], []
    n_candidates = 0
    for k, (b1, b2) in enumerate(sorted(bin_pairs)):
        p1, p2 = bin_pairs[(b1, b2)]
        if len(p1) < min_cluster_size or len(p2) < min_cluster_size:
            continue
        n_candidates += 1
        a1, a2 = unpack(b1, p1), unpack(b2, p2)
        fr1, fr2 = {}, {}
        for i, a in enumerate(a1):
            fr1.setdefault(a["frag"], []).append(i)
        for i, a in enumerate(a2):
            fr2.setdefault(a["frag"], []).append(i)
        fr2 = {f: v for f, v in fr2.items() if f in fr1}          # FilterUnmatched x2
        fr1 = {f: v for f, v in fr1.items() if f in fr2}

        def filter_overlapping(frs, al):                           # :316-358
            for f in frs:
                bins = [set(), set()]
                kept = []
                for idx in frs[f]:
                    a = al[idx]
                    rid = a["ref"] + (a["strand"] << 31)
                    rb = [(rid, b) for b in ora.get_bins(a["region"], min_fusion_range, 0)]
                    if not any(x in bins[a["readEnd"]] for x in rb):
                        bins[a["readEnd"]].update(rb)
                        kept.append(idx)
                frs[f] = kept
        filter_overlapping(fr1, a1)
        filter_overlapping(fr2, a2)
        if len(fr1) < min_cluster_size or len(fr2) < min_cluster_size:
            continue
        pairs = [(i1, i2) for f in sorted(fr1) for i1 in fr1[f] for i2 in fr2[f]]      # GetAlignPairs, ascending fragment
        x, y, u = [], [], []
        for i1, i2 in pairs:
            r1 = ora.MatePairEM.strand_remap(a1[i1]["region"], a1[i1]["strand"])
            r2 = ora.MatePairEM.strand_remap(a2[i2]["region"], a2[i2]["strand"])
            x.append(float(r1[1]))
            y.append(float(r2[1]))
            u.append(fragment_mean - (r1[1] - r1[0] + 1) - (r2[1] - r2[0] + 1))       # left to right, the lengths as ints
        xs += x
        ys += y
        us += u
        txo += ranks_desc(x)
        tyo += ranks_desc(y)
        pairs_all += pairs
        prob_off.append(prob_off[-1] + len(pairs))
        bin_pair.append(k)
        als.append((a1, a2))
        frags.append([a1[i1]["frag"] for i1, _ in pairs])
    return dict(prob_off=np.array(prob_off, dtype=np.int64), x=np.array(xs, dtype=np.float64), y=np.array(ys, dtype=np.float64),
                u=np.array(us, dtype=np.float64), to_xo=np.array(txo, dtype=np.int32), to_yo=np.array(tyo, dtype=np.int32),
                pairs=np.array(pairs_all, dtype=PAIR), bin_pair=np.array(bin_pair, dtype=np.int32), n_candidates=n_candidates, als=als, frags=frags)


ARRAYS = ("prob_off", "x", "y", "u", "to_xo", "to_yo", "pairs", "bin_pair")


def assert_same_problems(got, want):
    """every array of cmp_problems_fetch against the restatement, byte for byte"""
    for name in ARRAYS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and len(g) == len(w), (name, len(g), len(w))
        assert g.tobytes() == w.tobytes(), name


def lists_of(bin_pairs):
    """the map as the five arrays of cmp_bin_fetch"""
    keys, off1, off2, p1, p2 = [], [0], [0], [], []
    for (b1, b2) in sorted(bin_pairs):
        keys.append((b1 << 32) | b2)
        p1 += bin_pairs[(b1, b2)][0]
        p2 += bin_pairs[(b1, b2)][1]
        off1.append(len(p1))
        off2.append(len(p2))
    return (np.array(keys, dtype=np.uint64), np.array(off1, dtype=np.int64), np.array(off2, dtype=np.int64),
            np.array(p1, dtype=PACKED).reshape(len(p1)), np.array(p2, dtype=PACKED).reshape(len(p2)))


def select_rows(want, p0, p1, n_clusters, member, cluster_base=0):
    """The rows of problems [p0, p1) of a problems_of() result: n_clusters[q] and member[] are relative to p0 and to its first
    mate pair.  Per cluster j < n_clusters the first member mate pair of every fragment, in mate pair order (:630-643)."""
    rows = []
    base = int(want["prob_off"][p0])
    cid = cluster_base
    for p in range(p0, p1):
        lo, hi = int(want["prob_off"][p]) - base, int(want["prob_off"][p + 1]) - base
        a1, a2 = want["als"][p]
        for j in range(int(n_clusters[p - p0])):
            used = set()
            for i in range(lo, hi):
                if not (int(member[i]) >> j) & 1:
                    continue
                i1, i2 = (int(v) for v in want["pairs"][base + i])
                if a1[i1]["frag"] in used:
                    continue
                used.add(a1[i1]["frag"])
                rows.append((cid + j,) + tuple((a["frag"], a["readEnd"], a["ref"], a["strand"], a["region"][0], a["region"][1]) for a in (a1[i1], a2[i2])))
        cid += int(n_clusters[p - p0])
    return rows


def rows_as_tuples(rows):
    """cmp.ROW_DTYPE rows in the form of select_rows"""
    return [(int(r["cluster_id"]),) + tuple(tuple(int(r[f][s]) for f in ("fragment", "read_end", "ref", "strand", "start", "end")) for s in (0, 1))
            for r in rows]


# ------------------------------------------------------------------------------------------------------ hand-made lists
def pid(ref, strand, b):
    return ora.pack_id(ref, strand, b)


def ent(frag, read_end, start, end, b):
    """an entry of a list of bin b from absolute coordinates"""
    rs, re_ = start - b * BIN_LENGTH + BIN_LENGTH // 2, end - b * BIN_LENGTH + BIN_LENGTH // 2
    assert 0 <= rs < 65536 and 0 <= re_ < 65536
    return (frag, read_end, rs, re_)


def edge_cases():
    """[(name, bin pairs, min_fusion_range, min_cluster_size, fragment_mean, expected problem sizes or None)], one property each."""
    K = (pid(0, 0, 1), pid(1, 0, 3))                     # bin 1 holds 16384..81919, bin 3 holds 81920..147455
    other = lambda *frs: [ent(f, 1, 100000 + 10 * n, 100049 + 10 * n, 3) for n, f in enumerate(frs)]
    cases = []

    def add(name, bp, mfr=600, mcs=1, mean=300.0, sizes=None):
        cases.append((name, bp, mfr, mcs, mean, sizes))

    add("fragment_on_one_side_only", {K: ([ent(1, 0, 40000, 40049, 1), ent(2, 0, 40100, 40149, 1), ent(3, 0, 40200, 40249, 1)], other(1, 9, 3))},
        mcs=2, sizes=[2])
    add("both_read_ends_in_one_list", {K: ([ent(1, 0, 40000, 40049, 1), ent(1, 1, 40010, 40059, 1)], other(1))}, sizes=[2])
    add("same_read_end_same_bin", {K: ([ent(1, 0, 40000, 40049, 1), ent(1, 0, 40010, 40059, 1)], other(1))}, sizes=[1])
    add("same_read_end_adjacent_bins", {K: ([ent(1, 0, 40000, 40049, 1), ent(1, 0, 40200, 40249, 1)], other(1))}, sizes=[2])   # 40000/600 = 66, 40200/600 = 67
    add("straddler_collides_through_its_second_bin", {K: ([ent(1, 0, 40250, 40300, 1), ent(1, 0, 40150, 40210, 1)], other(1))}, sizes=[1])
    add("kept_straddler_blocks_both_bins", {K: ([ent(1, 0, 40150, 40210, 1), ent(1, 0, 39700, 39750, 1), ent(1, 0, 40300, 40350, 1)], other(1))}, sizes=[1])
    add("overlap_with_a_dropped_one_only", {K: ([ent(1, 0, 40000, 40049, 1), ent(1, 0, 40150, 40210, 1), ent(1, 0, 40300, 40350, 1)], other(1))}, sizes=[2])
    # bin 0: relative starts below 16384 are negative coordinates; -300 / 600 and 100 / 600 are both 0 in C++ (floor gives -1 and 0)
    K0 = (pid(0, 0, 0), pid(1, 0, 3))
    add("negative_start_in_bin_0", {K0: ([ent(1, 0, -300, -250, 0), ent(1, 0, 100, 150, 0), ent(2, 0, -900, -850, 0), ent(2, 0, -300, -250, 0)],
                                         other(1, 2))}, sizes=[3])
    add("fragment_in_two_runs", {K: ([ent(1, 0, 40000, 40049, 1), ent(2, 0, 41000, 41049, 1), ent(1, 0, 42000, 42049, 1), ent(-5, 0, 43000, 43049, 1),
                                      ent(2, 0, 41010, 41059, 1), ent(1, 0, 40010, 40059, 1)], other(2, 1, -5, 1))}, sizes=[2 + 1 + 1])
    rng = np.random.default_rng(4)
    for n in (1, 64, 65, 200):                            # one fragment group of n alignments: kept and dropped ones, both read ends
        first = [ent(7, int(rng.integers(0, 2)), s, s + int(rng.integers(30, 300)), 1) for s in (int(v) for v in rng.integers(16384, 81000, size=n))]
        add("group_of_%d" % n, {K: (first + [ent(8, 0, 50000, 50049, 1)], other(7, 8, 7) + [ent(7, 1, 120000, 120049, 3)])}, mfr=250)
    three = lambda f0: [ent(f0 + n, 0, 40000 + 1000 * n, 40049 + 1000 * n, 1) for n in range(3)]
    KB = (pid(0, 0, 1), pid(1, 0, 4))
    far = lambda *frs: [ent(f, 1, 140000 + 10 * n, 140049 + 10 * n, 4) for n, f in enumerate(frs)]
    add("list_lengths_at_the_threshold", {K: (three(1)[:2], other(1, 2, 3)), KB: (three(1), far(1, 2, 3))}, mcs=3, sizes=[3])
    add("matched_fragments_at_the_threshold", {K: (three(1) + [ent(4, 0, 44000, 44049, 1)], other(1, 2, 5, 6)),
                                               KB: (three(1) + [ent(7, 0, 44000, 44049, 1)], far(1, 2, 3, 8))}, mcs=3, sizes=[3])
    add("two_by_three_product", {K: ([ent(1, 0, 40000, 40049, 1), ent(1, 0, 41000, 41049, 1)],
                                     [ent(1, 1, 100000, 100049, 3), ent(1, 1, 101000, 101049, 3), ent(1, 1, 102000, 102049, 3)])}, sizes=[6])
    for s1, s2 in ((1, 0), (0, 1), (1, 1)):
        add("minus_strand_%d%d" % (s1, s2), {(pid(0, s1, 1), pid(1, s2, 3)): (three(1), other(3, 1, 2))}, sizes=[3])
    add("tied_x_and_y", {K: ([ent(f, 0, 40000, 40049 + (f % 2), 1) for f in range(1, 8)], [ent(f, 1, 100000, 100049 + (f % 3 == 0), 3) for f in range(1, 8)])},
        sizes=[7])
    many = {}
    for k in range(300):                                  # problems and groups across workgroup boundaries
        many[(pid(k % 7, 0, 1 + k // 7), pid(7 + k % 5, 1, 2 + k // 5))] = (
            [ent(2 * k, 0, 32768 * (1 + k // 7) + 5 * k, 32768 * (1 + k // 7) + 5 * k + 49, 1 + k // 7), ent(2 * k + 1, 0, 32768 * (1 + k // 7) + 100, 32768 * (1 + k // 7) + 180, 1 + k // 7)],
            [ent(2 * k + 1, 1, 32768 * (2 + k // 5) + 3 * k, 32768 * (2 + k // 5) + 3 * k + 59, 2 + k // 5), ent(2 * k, 1, 32768 * (2 + k // 5) + 200, 32768 * (2 + k // 5) + 270, 2 + k // 5)])
    add("300_bin_pairs_of_two_fragments", many, mcs=2, sizes=[2] * 300)
    add("fragment_mean_with_a_fraction", {K: (three(1), other(1, 2, 3))}, mean=301.7, sizes=[3])
    add("no_surviving_problem", {K: (three(1), other(1, 2, 3)), KB: (three(1)[:1], far(1))}, mcs=5, sizes=[])
    add("no_bin_pairs", {}, sizes=[])
    return cases


# -------------------------------------------------------------------------------------------------------------- the tool
def bin_pairs_of_lines(lines, min_fusion_range):
    """the oracle's map of bin pairs of a compact alignment input, and the reference names in order of appearance"""
    ref_names, ref_index, bp = [], {}, {}
    for raws in ora.read_fragments(lines):
        als = []
        for r in raws:
            if r["reference"] not in ref_index:
                ref_index[r["reference"]] = len(ref_names)
                ref_names.append(r["reference"])
            als.append(dict(frag=int(r["fragment"]), readEnd=r["readEnd"], ref=ref_index[r["reference"]], strand=r["strand"], region=r["region"]))
        ora.add_fragment(als, min_fusion_range, bp)
    return bp, ref_names


def run_tool(path, out, m=5, env=None):
    """clustermatepairs -u 300 -s 30 -p 0.95 on the file at `path`"""
    args = [TOOL, "-a", str(path), "-c", str(out), "-u", "300", "-s", "30", "-p", "0.95", "-m", str(m)]
    return subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **env) if env else None)


def parse_em_dump(data):
    """DEFUSE_CMP_DUMP_EM: two int64 (problems, mate pairs), mpe_params (32 bytes), probOff, X, Y, U, toXO, toYO"""
    n_prob, n_mp = struct.unpack_from("<qq", data, 0)
    at = 16 + 32
    out = {}
    for name, dtype, n in (("prob_off", np.int64, n_prob + 1), ("x", np.float64, n_mp), ("y", np.float64, n_mp), ("u", np.float64, n_mp),
                           ("to_xo", np.int32, n_mp), ("to_yo", np.int32, n_mp)):
        out[name] = np.frombuffer(data, dtype=dtype, count=n, offset=at)
        at += n * np.dtype(dtype).itemsize
    assert at == len(data)
    return out
