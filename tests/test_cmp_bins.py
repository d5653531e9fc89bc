"""The bin-pair builder of clustermatepairs (defuse_amd/csrc/cmp_api.hip, include/defuse_cmp.h).

Without a GPU: the per-fragment logic of the kernels — concordance, the reference's stop conditions, the entries a fragment
adds and the order it writes them in — is __host__ __device__ code; a host program compiled from the same source walks the
fragments in file order, sorts stably by key as the device does, and must give the oracle's map of bin pairs, list by list
(fragments with many alignments per end, both ends in the same bins, alignments over several bins, concordant pairs).
With a GPU (-m gpu): the C ABI itself against the oracle on the same inputs, and the tool with device binning against the
tool with the host cross-check path, dump for dump."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype([("fragment", "<i4"), ("start", "<i4"), ("end", "<i4"), ("meta", "<u4")])
PACKED = np.dtype([("fragment", "<i4"), ("read_end", "<i4"), ("rel_start", "<u2"), ("rel_end", "<u2")])


def random_fragments(seed, n_fragments, heavy_every=17):
    """Fragments as lists of alignment dicts (oracle form) and as cmp_record rows + fragment starts."""
    rng = np.random.default_rng(seed)
    frs = []
    for f in range(n_fragments):
        als = []
        heavy = f % heavy_every == 0
        n0 = int(rng.integers(1, 40 if heavy else 3))
        n1 = int(rng.integers(0 if f % 29 == 0 else 1, 40 if heavy else 3))
        # a few loci shared by all fragments: lists with entries of many fragments.  An end-0 alignment lies 6-12 kb below a
        # locus and an end-1 alignment 6-12 kb above one — often in one 32 kb bin (the symmetric combinations, when both ends have
        # alignments at both loci) and never close enough to make the fragment concordant; some alignments lie anywhere.
        loci = [(k % 5, 50000 + 90000 * k) for k in range(12)]
        anchor = [loci[int(rng.integers(0, len(loci)))] for _ in range(2)]
        for end, n in ((0, n0), (1, n1)):
            for _ in range(n):
                ref, pos = anchor[int(rng.integers(0, 2))]
                near = pos + (1 if end else -1) * int(rng.integers(6000, 12000))
                start = max(1, near if rng.random() < 0.85 else int(rng.integers(1, 600000)))
                if rng.random() < 0.15:
                    start = (start // 32768) * 32768 + int(rng.integers(-700, 700))      # near a bin edge: two or three bins
                    start = max(1, start)
                length = int(rng.integers(30, 151))
                als.append(dict(frag=1000 + f, readEnd=end, ref=ref, strand=int(rng.integers(0, 2)), region=(start, start + length - 1)))
        order = rng.permutation(len(als))                       # the ends interleaved, as an aligner's output may be
        frs.append([als[k] for k in order])
    return frs


def to_records(frs):
    rows, starts = [], [0]
    for als in frs:
        for a in als:
            rows.append((a["frag"], a["region"][0], a["region"][1], a["ref"] | (a["strand"] << 28) | (a["readEnd"] << 29)))
        starts.append(len(rows))
    return np.array(rows, dtype=REC), np.array(starts, dtype=np.uint32)


HEAVY_MFR = 600
# (alignments on end 0, on end 1); an end of n alignments has n + n // 10 entries (below): 256 | 3, 257 | 3 (the entry past the
# bitmap is the id seen for the first time), 258 | 259 (both ends past it, ids seen again there), 3 | 264.  No larger: beyond
# the bitmap one lane scans an end again for every pair of entries, about 1.6 us per entry scanned on an MI355X — ends of
# 282 and 330 entries took 28 s of device time, these take about a second together.
HEAVY_CASES = [(233, 3), (234, 3), (235, 236), (3, 240)]


def heavy_fragments(seed, n0, n1):
    """Six fragments with n0 / n1 alignments on their two ends, for the far side of Distinct's bitmap (entry 256 of an end).
    End 0 lies on references 0-2 and end 1 on references 3-5, so no fragment is concordant.  Of an end's n alignments n // 10
    lie across a bin edge and cover two bins with HEAVY_MFR, the others lie inside one bin: the end has n + n // 10 entries.
    All but one start in twelve (reference, bin) places, so ids repeat all along the list; the last alignment of an end lies
    in a bin of its own, an id whose first entry comes last.  The order of the others, and of the two ends, is shuffled."""
    rng = np.random.default_rng(seed)
    frs = []
    for f in range(6):
        ends = []
        for end, n in ((0, n0), (1, n1)):
            places = [(3 * end + k % 3, 3 + 5 * (k // 3)) for k in range(12)]
            als = []
            for j in range(n):
                ref, b = places[int(rng.integers(0, 12))]
                if j < n // 10:
                    start = b * 32768 + int(rng.integers(-300, 300))                 # bins b - 1 and b
                elif j == n - 1:
                    start = 40 * 32768 + int(rng.integers(4000, 28000))              # nobody else's bin
                else:
                    start = b * 32768 + int(rng.integers(4000, 28000))               # bin b alone
                length = int(rng.integers(30, 151))
                als.append(dict(frag=1000 + f, readEnd=end, ref=ref, strand=int(rng.integers(0, 2)), region=(start, start + length - 1)))
            order = list(rng.permutation(n - 1)) + [n - 1]
            ends.append([als[k] for k in order])
        take = [0] * n0 + [1] * n1                                                    # the ends interleaved, each in its order
        rng.shuffle(take)
        at = [0, 0]
        out = []
        for e in take:
            out.append(ends[e][at[e]])
            at[e] += 1
        frs.append(out)
    return frs


def end_entries(als, end, mfr):
    """The ids of the (alignment, bin) entries of one read end in arrival order (end_list of cmp_api.hip)."""
    from oracle import clustermatepairs_oracle as ora
    return [ora.pack_id(a["ref"], a["strand"], b) for a in als if a["readEnd"] == end for b in ora.get_bins(a["region"], 32768, mfr)]


def heavy_coverage(cases):
    """What the heavy cases reach of Distinct::first, computed from the inputs: the lengths of the ends' entry lists, whether
    some id has its first entry at position >= 256, and whether some id first seen below 256 comes again at or beyond it."""
    lengths, late_first, seen_again = set(), False, False
    for frs in cases:
        for als in frs:
            for end in (0, 1):
                ids = end_entries(als, end, HEAVY_MFR)
                lengths.add(len(ids))
                first = {}
                for k, i in enumerate(ids):
                    first.setdefault(i, k)
                late_first |= any(k >= 256 for k in first.values())
                seen_again |= any(first[i] < 256 for i in ids[256:])
    return lengths, late_first, seen_again


def test_heavy_cases_reach_both_sides_of_the_bitmap():
    lengths, late_first, seen_again = heavy_coverage([heavy_fragments(20 + k, n0, n1) for k, (n0, n1) in enumerate(HEAVY_CASES)])
    assert {3, 256, 257, 258, 259, 264} == lengths
    assert late_first and seen_again


def oracle_bin_pairs(frs, mfr):
    from oracle import clustermatepairs_oracle as ora
    bp = {}
    conc = 0
    for als in frs:
        before = sum(len(v[0]) + len(v[1]) for v in bp.values())
        c = [set(), set()]
        for a in als:
            for b in ora.get_bins(a["region"], mfr, mfr):
                c[a["readEnd"]].add((a["ref"], b))
        conc += 1 if c[0] & c[1] else 0
        ora.add_fragment(als, mfr, bp)
    return bp, conc


def as_lists(keys, off1, off2, p1, p2):
    out = {}
    for k, key in enumerate(keys):
        key = int(key)
        f = [tuple(int(x) for x in r) for r in p1[off1[k]:off1[k + 1]]]
        s = [tuple(int(x) for x in r) for r in p2[off2[k]:off2[k + 1]]]
        out[(key >> 32, key & 0xFFFFFFFF)] = (f, s)
    return out


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("cmpwalk")
    src = d / "walk.hip"
    src.write_text(r'''
#include "%s/defuse_amd/csrc/cmp_api.hip"
#include <algorithm>
#include <cstdio>
// the kernels' per-fragment code on the host, fragments in file order, then the device's stable sort by key
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    long long n, nf; int mfr;
    if (fread(&n, 8, 1, in) != 1 || fread(&nf, 8, 1, in) != 1 || fread(&mfr, 4, 1, in) != 1) return 2;
    std::vector<cmp_record> recs(n); std::vector<uint32_t> fs(nf + 1);
    if (n && fread(recs.data(), sizeof(cmp_record), n, in) != (size_t)n) return 2;
    if (fread(fs.data(), 4, nf + 1, in) != (size_t)(nf + 1)) return 2;
    struct E { unsigned long long key; cmp_packed p; };
    std::vector<E> side[2];
    long long conc = 0;
    for (long long f = 0; f < nf; ++f) {
        const cmp_record* r = recs.data() + fs[f]; const int m = (int)(fs[f + 1] - fs[f]);
        if (fragment_concordant(r, m, mfr)) { ++conc; continue; }
        int bad, value; const int kind = fragment_error(r, m, mfr, bad, value);
        if (kind) { printf("error %%d %%lld %%d\n", kind, (long long)fs[f] + bad, value); return 0; }
        // as k_cmp_count + k_cmp_emit place them: `first` lists end 0 then end 1, `second` lists end 1 then end 0
        std::vector<E> part[2][2];
        fragment_entries(r, m, mfr, [&](int s, int ea, unsigned long long key, int ia, int b) {
            cmp_packed p; p.fragment = r[ia].fragment; p.read_end = rec_end(r[ia]);
            p.rel_start = (uint16_t)(r[ia].start - b * BIN_LENGTH + BIN_LENGTH / 2); p.rel_end = (uint16_t)(r[ia].end - b * BIN_LENGTH + BIN_LENGTH / 2);
            part[s][ea].push_back(E{key, p});
        });
        for (const E& e : part[0][0]) side[0].push_back(e);
        for (const E& e : part[0][1]) side[0].push_back(e);
        for (const E& e : part[1][1]) side[1].push_back(e);
        for (const E& e : part[1][0]) side[1].push_back(e);
    }
    printf("concordant %%lld\n", conc);
    for (int s = 0; s < 2; ++s) {
        std::stable_sort(side[s].begin(), side[s].end(), [](const E& a, const E& b) { return a.key < b.key; });
        for (const E& e : side[s]) printf("%%d %%llu %%d %%d %%d %%d\n", s, e.key, e.p.fragment, e.p.read_end, (int)e.p.rel_start, (int)e.p.rel_end);
    }
    return 0;
}
''' % ROOT)
    exe = d / "walk"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-result", "-o", str(exe), str(src)])
    return str(exe), d


def write_input(path, recs, starts, mfr):
    with open(path, "wb") as f:
        f.write(struct.pack("<qqi", len(recs), len(starts) - 1, mfr))
        f.write(recs.tobytes())
        f.write(starts.tobytes())


def walk(host_walk, frs, mfr):
    """The host walk's first line and its lists by bin pair."""
    exe, d = host_walk
    recs, starts = to_records(frs)
    write_input(d / "in.bin", recs, starts, mfr)
    out = subprocess.run([exe, str(d / "in.bin")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = {}
    for line in out[1:]:
        s, key, fr, e, rs, re_ = (int(x) for x in line.split())
        got.setdefault((key >> 32, key & 0xFFFFFFFF), ([], []))[s].append((fr, e, rs, re_))
    return out[0], got


@pytest.mark.parametrize("seed,mfr", [(1, 600), (2, 600), (3, 1500), (4, 250)])
def test_fragment_walk_equals_the_oracle(host_walk, seed, mfr):
    frs = random_fragments(seed, 400)
    head, got = walk(host_walk, frs, mfr)
    exp, conc = oracle_bin_pairs(frs, mfr)
    assert head == "concordant %d" % conc and conc > 5
    assert set(got) == set(exp) and len(exp) > 300
    multi = 0
    for key in exp:
        assert got[key][0] == exp[key][0] and got[key][1] == exp[key][1], key
        multi += 1 if len(exp[key][0]) > 3 else 0
    assert multi > 20                                             # lists with several entries: their order is what is being tested


@pytest.mark.parametrize("case", range(len(HEAVY_CASES)))
def test_fragment_walk_equals_the_oracle_on_heavy_ends(host_walk, case):
    """Ends of 256 entries and more: beyond its bitmap Distinct::first looks an id up by scanning the end again."""
    n0, n1 = HEAVY_CASES[case]
    frs = heavy_fragments(20 + case, n0, n1)
    head, got = walk(host_walk, frs, HEAVY_MFR)
    exp, conc = oracle_bin_pairs(frs, HEAVY_MFR)
    assert head == "concordant 0" and conc == 0
    assert set(got) == set(exp) and len(exp) > 100
    for key in exp:
        assert got[key][0] == exp[key][0] and got[key][1] == exp[key][1], key


def test_stop_conditions_in_file_order(host_walk):
    """The first alignment on which the reference stops is reported with its kind and value: too many reference sequences,
    chromosome too large.  (A relative position outside 16 bits needs a minFusionRange of more than half a bin: the
    test below.)"""
    exe, d = host_walk
    frs = random_fragments(9, 50)
    frs[20][0]["ref"] = (1 << 18) + 5
    frs[30][0]["region"] = ((1 << 13) * 32768 + 10, (1 << 13) * 32768 + 80)
    recs, starts = to_records(frs)
    write_input(d / "err.bin", recs, starts, 600)
    out = subprocess.run([exe, str(d / "err.bin")], capture_output=True, text=True, check=True).stdout.splitlines()
    from oracle import clustermatepairs_oracle as ora
    # fragment 20 may be concordant (then nothing stops there)
    first = None
    for k, als in enumerate(frs):
        try:
            ora.add_fragment(als, 600, {})
        except SystemExit as e:
            first = (k, str(e))
            break
    assert first is not None
    kind = 2 if "too many reference" in first[1] else 3
    assert out[0].startswith("error %d " % kind), (out[0], first)
    assert int(out[0].split()[2]) in range(int(starts[first[0]]), int(starts[first[0] + 1]))


STOP_MFR = 20000
BIN = 32768
# offender -> (reference, region, kind, the reference's message up to the file name).  With a minFusionRange above half a bin
# an alignment reaches bins in which its relative position does not fit 16 bits (tools/clustermatepairs.cpp:183-186); the
# RefBinPacked of the same (alignment, bin) is built first (:258 before :260), so its two limits win where both are broken.
STOP_OFFENDERS = {
    # start - 20000 lies 30000 into bin 5: relative start in bin 5 is 50000 + 16384
    "start_high": (1, (5 * BIN + 50000, 5 * BIN + 50049), 1, "Error: relativeStart < (1<<16) failed on line: 185 of "),
    # bins 7..9; fits bins 7 and 8; in bin 9 the start lies 18049 below the bin: -18049 + 16384
    "start_low": (1, (9 * BIN - 18049, 9 * BIN - 18000), 1, "Error: relativeStart >= 0 failed on line: 183 of "),
    # relative start 65500, relative end 65549 in the first bin
    "end_high": (1, (5 * BIN + 49116, 5 * BIN + 49165), 1, "Error: relativeEnd < (1 << 16) failed on line: 186 of "),
    "reference": ((1 << 18) + 5, (5 * BIN + 50000, 5 * BIN + 50049), 2, "Packing failed, too many reference sequences"),
    "bin": (1, ((1 << 13) * BIN + 25000, (1 << 13) * BIN + 25049), 3, "Packing failed, chromosome too large"),
}


def stop_fragments(offender):
    """Eight fragments that fit with STOP_MFR (starts 20000-30000 into a bin: bins b and b + 1, both relative positions
    inside 16 bits), the ends on references 0 and 1; alignment 1 of fragment 5 is the offender, fragment 7 holds another
    kind of offender that is never reached.  Returns (fragments, index of the offending record)."""
    frs = []
    for f in range(8):
        als = []
        for k in range(4):
            start = (3 + f + 2 * k) * BIN + 20000 + 1111 * k + 97 * f
            als.append(dict(frag=1000 + f, readEnd=k % 2, ref=k % 2, strand=(f + k) % 2, region=(start, start + 49)))
        frs.append(als)
    ref, region, _, _ = STOP_OFFENDERS[offender]
    frs[5][1].update(ref=ref, region=region)
    later = "bin" if offender != "bin" else "start_high"
    frs[7][0].update(ref=STOP_OFFENDERS[later][0], region=STOP_OFFENDERS[later][1])
    return frs, 5 * 4 + 1


def oracle_stop_kind(frs, mfr):
    """(fragment, kind) of the first fragment on which the oracle stops."""
    from oracle import clustermatepairs_oracle as ora
    for k, als in enumerate(frs):
        try:
            ora.add_fragment(als, mfr, {})
        except SystemExit as e:
            return k, 2 if "too many reference" in str(e) else 3 if "chromosome too large" in str(e) else 1
    return None


@pytest.mark.parametrize("offender", sorted(STOP_OFFENDERS))
def test_stop_conditions_with_a_wide_fusion_range(host_walk, offender):
    """fragment_error against the oracle's SystemExit, each kind as the first offender of an input of its own; an alignment
    on a reference >= 2^18 that also breaks a relative-position check stops as the reference limit."""
    exe, d = host_walk
    frs, record = stop_fragments(offender)
    assert oracle_stop_kind(frs, STOP_MFR) == (5, STOP_OFFENDERS[offender][2])
    clean = [als for k, als in enumerate(frs) if k not in (5, 7)]
    assert oracle_stop_kind(clean, STOP_MFR) is None
    recs, starts = to_records(frs)
    write_input(d / "stop.bin", recs, starts, STOP_MFR)
    out = subprocess.run([exe, str(d / "stop.bin")], capture_output=True, text=True, check=True).stdout.splitlines()
    kind = STOP_OFFENDERS[offender][2]
    assert out[0].split()[:3] == ["error", str(kind), str(record)], out[0]
    if kind == 2:
        assert out[0].split()[3] == str((1 << 18) + 5)
    if kind == 3:
        assert out[0].split()[3] == str(1 << 13)
