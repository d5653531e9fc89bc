"""The concordant-cluster filter on the GPU (include/defuse_task.h, section "concordant clusters", through defuse_amd/concfilter.py): prep_local_alignment_seqs.pl,
localalign and `filter_column.pl VALUES 0 1` over cluster text in device memory.

Yardstick: tests/concfilter_oracle.py, the scripts restated on Fractions.  Without a GPU it is pinned to what the reference's
Perl scripts printed on the fixtures of tests/golden/conc/ (tests/golden/make_conc.py; target lines as multisets, the filtered
file byte for byte, the two inputs the script dies on), and conc_shared.hpp gives the oracle's targets, positions and slices in a
host program under ASan + UBSan.  On the GPU the descriptors, the scores of the printed targets, both texts and the dedup that
follows equal the oracle's."""
import ctypes
import os
import random
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import abi
from tests import clusterregions_oracle as cora
from tests import concfilter_cases as cases
from tests import concfilter_oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conc")
E_DEVICE, E_ARG, E_LIMIT = -2, -3, -4
SCORES = dict(match=10, mismatch=-5, gap=-5, threshold=0.8)          # scripts/defuse_run.pl:497
PERL = (("edges", 40), ("edges", 130), ("random1", 40))


@pytest.fixture(scope="module")
def cf(built):
    from defuse_amd import concfilter
    return concfilter


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def fixture_case(name):
    """one_end and missing_other are cluster files over the FASTA and the GTF of edges."""
    inputs = "edges" if name in ("one_end", "missing_other") else name
    return dict(fa=golden(inputs + ".fa"), gtf=golden(inputs + ".gtf"), clusters=golden(name + ".clusters"))


_worlds = {}


def world(key, case, seq_range):
    """The case read by the host readers and, computed once, the oracle's whole answer (or its Stop)."""
    from defuse_amd import concfilter
    if (key, seq_range) not in _worlds:
        models, fasta = concfilter.read_gene_models(case["gtf"]), concfilter.read_fasta(case["fa"])
        try:
            want = ora.run(models, fasta, case["clusters"], seq_range, **SCORES)
        except (ora.Stop, ValueError, IndexError, KeyError, AssertionError) as stop:      # (a case made to stop the library)
            want = stop
        _worlds[(key, seq_range)] = dict(case=case, models=models, fasta=fasta, want=want)
    return _worlds[(key, seq_range)]


def named_world(name, seq_range):
    if name in ("edges", "random1", "one_end", "missing_other"):
        return world(name, fixture_case(name), seq_range)
    if name == "r2000":
        return world(name, cases.r2000_case(), seq_range)
    return world(name, cases.random_case(int(name[6:])), seq_range)


# ---------------------------------------------------------------------------------------------- without a GPU
def test_fixtures_are_what_the_generator_writes():
    """The committed inputs are the case builders' (the Perl outputs were recorded from exactly these bytes)."""
    for name, case in (("edges", cases.edges_case()), ("random1", cases.random_case(1)), ("one_end", cases.one_end_case()),
                       ("missing_other", cases.missing_other_case())):
        assert fixture_case(name) == case, name


@pytest.mark.parametrize("name,seq_range", PERL)
def test_oracle_targets_equal_perl(cf, name, seq_range):
    """Every line prep_local_alignment_seqs.pl printed, and no other, as multisets."""
    w = named_world(name, seq_range)
    perl = golden("%s.R%d.seq.perl.txt" % (name, seq_range))
    assert sorted(ora.target_lines(w["want"]["targets"])) == [l + b"\n" for l in perl.split(b"\n")[:-1]]
    assert len(w["want"]["targets"]) > 40


@pytest.mark.parametrize("name,seq_range", PERL)
def test_oracle_filtered_equals_perl(cf, name, seq_range):
    w = named_world(name, seq_range)
    assert w["want"]["align_text"] == golden("%s.R%d.align.txt" % (name, seq_range))
    assert w["want"]["filtered"] == golden("%s.R%d.filtered.perl.txt" % (name, seq_range))
    assert 0 < w["want"]["filtered"].count(b"\n") < w["case"]["clusters"].count(b"\n")


def test_oracle_stops_where_perl_dies(cf):
    for name, kind, cid in (("one_end", ora.ONE_END, "2"), ("missing_other", ora.NO_OTHER_SEQ, "2")):
        assert int(golden(name + ".status.perl.txt")) != 0 and golden(name + ".stderr.perl.txt").startswith(b"Use of uninitialized value")
        stop = named_world(name, 40)["want"]
        assert isinstance(stop, ora.Stop) and (stop.kind, stop.cluster_id) == (kind, cid), name


def test_edges_fixture_holds_the_branches(cf):
    """What the issue asks the fixtures to hold, read off the oracle's targets at R = 40."""
    w = named_world("edges", 40)
    tg, models = w["want"]["targets"], w["models"]
    by = {}
    for t in tg:
        by.setdefault((t["cluster_id"], t["cluster_end"]), []).append(t)
    names = lambda key: [t["name"] for t in by.get(key, [])]
    assert names((1, 0)) == ["chr1", "G1|T1", "G1|T2", "G1|T3"]                                           # T4 is skipped
    assert names((1, 1)) == ["chr1", "G1|T1", "G1|T2", "G1|T3", "G2|T1", "G2|T2"]              # two overlapping genes, both expressed at 135
    assert ora.overlapping_genes(models, "chr1", (101, 130)) == ["G1", "G2"]
    assert [(t["start"], t["len"]) for t in by[(2, 0)][:1]] == [(0, 12)] and [(t["start"], t["len"]) for t in by[(3, 0)][:1]] == [(391, 9)]
    assert [t["len"] for t in by[(4, 0)][:1]] == [1] and [t["len"] for t in by[(4, 1)][:1]] == [1]
    assert by[(5, 0)][0]["other_rev"] == 1 and by[(5, 0)][0]["other_len"] == 21
    assert ora.overlapping_genes(models, "G5|T1", (20, 51)) == ["G5"] and ora.overlapping_genes(models, "chr2", (21, 161)) == ["G4", "G5"]
    assert names((7, 0)) == ["chr1", "G1|T1", "G1|T2", "G1|T3"]
    assert names((8, 0)) == ["chr1"] and names((8, 1)) == ["chr1", "G3|T1"]                                     # the elsif quirk
    assert names((11, 0)) == ["G6|T1"]                                                                           # chr3 is not in the FASTA
    assert models.transcripts["G1|T2"]["cds"] is None and not ora.expressed(models, "G7", 75)
    for tx, pos, want in (("G1|T2", Fraction(231, 2), 41), ("G1|T3", Fraction(231, 2), 1), ("G1|T3", Fraction(461, 2), 11), ("G2|T2", 150, 21)):
        assert ora.transcript_position(models, tx, pos) == want                                                 # intron, before the first exon, past the last
    hit = {int(l.split(b"\t")[0]) for l in w["want"]["align_text"].split(b"\n")[:-1]}
    printed = {(t["cluster_id"], t["kind"]) for t, k in zip(tg, w["want"]["kept"]) if k}
    assert 10 not in hit and 9 in hit and (9, 0) not in printed and (9, 1) in printed and (1, 0) in printed
    assert any((t["other_start"] + t["other_len"]) % 2 for t in tg)


def test_abi(cf):
    sizes, n = abi.check("defuse_task.h", cf, r"conc_[a-z_]+", constants=cf.CONSTANTS, dtypes=[(cf.Target, cf.TARGET_DTYPE)])
    assert sizes == [160, 96, 56, 48] and n == 13 == len(cf.EXPORTS)
    assert abi.layout("defuse_task.h", {}, ["sizeof(conc_gene)", "sizeof(conc_transcript)", "sizeof(conc_interval)", "sizeof(conc_name)"]) == \
        ["sizeof(conc_gene) 16", "sizeof(conc_transcript) 32", "sizeof(conc_interval) 8", "sizeof(conc_name) 16"]
    assert (cf.GENE_DTYPE.itemsize, cf.TRANSCRIPT_DTYPE.itemsize, cf.INTERVAL_DTYPE.itemsize, cf.NAME_DTYPE.itemsize) == (16, 32, 8, 16)


def test_argument_errors_need_no_device(cf):
    """Every argument error is found before a device is touched."""
    lib = cf.lib()
    h, res = ctypes.c_void_p(), cf.ConcResult()
    assert lib.conc_create(0, None) == E_ARG and lib.conc_models_create(0, None, ctypes.byref(h)) == E_ARG
    flat = cf.read_gene_models(fixture_case("edges")["gtf"]).flatten()

    def create(names=("chr1",), mutate=None):
        pool = bytearray()
        f = {k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in flat.items()}
        if mutate:
            mutate(f)
        cn, tn, sn = cf._names(pool, f["chrom_names"]), cf._names(pool, f["transcript_names"]), cf._names(pool, list(names))
        pool = np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8)
        p = cf._ptr
        d = cf.ModelsDesc(p(f["genes"]), p(f["gene_tx"]), p(f["transcripts"]), p(f["exons"]), p(f["expressed"]), p(f["chrom_gene_first"]), p(f["chrom_genes"]),
                          p(pool), p(cn), p(tn), p(sn), len(f["genes"]), len(f["gene_tx"]), len(f["transcripts"]), len(f["exons"]), len(f["expressed"]),
                          len(f["chrom_genes"]), len(pool) - 1, len(cn), len(sn))
        return lib.conc_models_create(0, ctypes.byref(d), ctypes.byref(h)), lib.conc_last_error().decode()

    def swap_names(f):
        f["chrom_names"][0], f["chrom_names"][1] = f["chrom_names"][1], f["chrom_names"][0]

    def bad_tx(f):
        f["gene_tx"][0] = len(f["transcripts"])

    def far(f):
        f["exons"]["end"][0] = 2 ** 28 + 1

    assert create(mutate=swap_names)[0] == E_ARG and "ascend" in create(mutate=swap_names)[1]
    assert create(mutate=bad_tx)[0] == E_ARG and create(mutate=far)[0] == E_LIMIT
    assert create(names=("chr1:5-9",))[0] == E_LIMIT and create(names=("a", "a"))[0] == E_ARG
    assert lib.conc_targets(None, None, None, None, 40, ctypes.byref(res)) == E_ARG and lib.conc_targets(None, None, None, None, 40, None) == E_ARG
    assert lib.conc_align(None, None, 10, -5, -5, 0.8, ctypes.byref(res)) == E_ARG and lib.conc_filter(None, ctypes.byref(res)) == E_ARG
    assert lib.conc_fetch(None, 0, 0, None, 0) == E_ARG and lib.conc_fetch(None, 7, 0, None, 0) == E_ARG
    assert lib.conc_fetch_targets(None, None, 0) == E_ARG and lib.conc_fetch_scores(None, None, 0) == E_ARG
    assert lib.conc_into_taskc(None, None) == E_ARG and lib.conc_get_timing(None, None) == E_ARG
    lib.conc_destroy(None)
    lib.conc_models_destroy(None)


HOST = r'''
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "%(root)s/defuse_amd/csrc/conc_shared.hpp"

static FILE* in;
static long long num() { long long v; if (fscanf(in, "%%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static char g_word[1 << 20];
static std::string word() { if (fscanf(in, "%%1048575s", g_word) != 1) exit(2); return std::string(g_word); }
static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> out;
    for (size_t k = 1; k + 1 < h.size(); k += 2) out.push_back((uint8_t)strtol(h.substr(k, 2).c_str(), nullptr, 16));      // (a leading "x")
    return out;
}
template <class T> static std::vector<T> table(int fields)
{
    std::vector<T> v((size_t)num());
    for (auto& e : v) { int32_t* p = reinterpret_cast<int32_t*>(&e); for (int k = 0; k < fields; ++k) p[k] = (int32_t)num(); }
    return v;
}
static std::vector<conc_name> names()
{
    std::vector<conc_name> v((size_t)num());
    for (auto& e : v) { e.off = num(); e.len = (int32_t)num(); e.pad_ = 0; }
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 2 || !(in = fopen(argv[1], "r"))) return 2;
    auto genes = table<conc_gene>(4);
    auto gene_tx = table<int32_t>(1);
    auto tx = table<conc_transcript>(7);
    auto exons = table<conc_interval>(2);
    auto expr = table<conc_interval>(2);
    auto first = table<int32_t>(1);
    auto cg = table<int32_t>(1);
    auto pool = unhex(word());
    auto cn = names(), tn = names(), sn = names();
    std::vector<task_seq> seqs(sn.size());
    for (auto& s : seqs) { s.off = 0; s.len = num(); }
    // the tables conc_models_create derives
    std::vector<int32_t> sorted(sn.size()), chrom_seq(cn.size()), tx_seq(tn.size()), premax(cg.size());
    for (size_t k = 0; k < sorted.size(); ++k) sorted[k] = (int32_t)k;
    std::sort(sorted.begin(), sorted.end(), [&](int32_t a, int32_t b) { return conc_name_cmp(pool.data() + sn[a].off, sn[a].len, pool.data() + sn[b].off, sn[b].len) < 0; });
    for (size_t c = 0; c < cn.size(); ++c) chrom_seq[c] = conc_find_name(pool.data(), sn.data(), sorted.data(), (int32_t)sn.size(), pool.data() + cn[c].off, cn[c].len);
    for (size_t t = 0; t < tn.size(); ++t) tx_seq[t] = conc_find_name(pool.data(), sn.data(), sorted.data(), (int32_t)sn.size(), pool.data() + tn[t].off, tn[t].len);
    for (size_t c = 0; c + 1 < first.size(); ++c)
        for (int32_t k = first[c]; k < first[c + 1]; ++k) premax[k] = k > first[c] ? std::max(premax[k - 1], genes[cg[k]].end) : genes[cg[k]].end;
    conc_view V{genes.data(), gene_tx.data(), tx.data(), exons.data(), expr.data(), first.data(), cg.data(), premax.data(), pool.data(), cn.data(), tn.data(),
                sn.data(), sorted.data(), chrom_seq.data(), tx_seq.data(), seqs.data(), (int32_t)cn.size(), (int32_t)tn.size(), (int32_t)sn.size(), 0};
    for (long long q = num(); q > 0; --q) {
        const std::string op = word();
        if (op == "G") { const int t = (int)num(); const long long p = num(); printf("%%lld\n", (long long)conc_genomic_position2(V, t, p)); }
        else if (op == "T") { const int t = (int)num(); const long long p = num(); printf("%%lld\n", (long long)conc_transcript_position2(V, t, p)); }
        else if (op == "S") {
            const long long a = num(), b = num(), L = num();
            const conc_slice s = conc_subseq(a, b, L);
            printf("%%d %%d %%d\n", s.start, s.len, s.rev);
        } else if (op == "R") { const auto n = unhex(word()); printf("%%d\n", conc_name_is_range(n.data(), (int64_t)n.size()) ? 1 : 0); }
        else if (op == "E") {
            std::vector<uint8_t> nm[2];
            conc_end e[2];
            for (int k = 0; k < 2; ++k) {
                nm[k] = unhex(word());
                nm[k].push_back(0);
                e[k] = conc_end{nm[k].data(), (int32_t)nm[k].size() - 1, (int32_t)num(), 0, 0};
                e[k].start = (int32_t)num();
                e[k].end = (int32_t)num();
            }
            const long long range = num();
            const conc_end_plan P = conc_plan_end(V, e[0], e[1]);
            int32_t limit = P.limit;
            std::vector<std::pair<long long, conc_target>> got;
            if (!P.stop && !limit) conc_end_targets(V, P, e[0], 7, 0, range, limit, [&](const conc_target& T, int64_t rank) { got.push_back({(long long)rank, T}); });
            std::sort(got.begin(), got.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
            printf("%%d %%d %%zu", P.stop, limit, got.size());
            for (const auto& g : got)
                printf(" | %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", g.second.kind, g.second.name, g.second.seq, g.second.start, g.second.len, g.second.revcomp,
                       g.second.other_seq, g.second.other_start, g.second.other_len, g.second.other_rev);
            printf("\n");
        } else return 3;
    }
    return 0;
}
'''


def _hex(name):
    return "x" + name.encode("latin-1").hex()


def _host_input(cf, w, queries):
    """The flattened models, the names and the sequence lengths as the host program reads them, then the queries."""
    flat, fasta = w["models"].flatten(), w["fasta"]
    pool = bytearray()
    tabs = [cf._names(pool, flat["chrom_names"]), cf._names(pool, flat["transcript_names"]), cf._names(pool, list(fasta))]
    out = []
    for key, fields in (("genes", GENE), ("gene_tx", None), ("transcripts", TX), ("exons", IV), ("expressed", IV), ("chrom_gene_first", None), ("chrom_genes", None)):
        arr = flat[key]
        out.append("%d" % len(arr))
        out += [" ".join(str(int(x)) for x in (row if fields is None else [row[f] for f in fields])) for row in (arr.reshape(-1, 1) if fields is None else arr)]
    out.append("x" + bytes(pool).hex())
    for t in tabs:
        out.append("%d" % len(t))
        out += ["%d %d" % (int(r["off"]), int(r["len"])) for r in t]
    out += ["%d" % len(s) for s in fasta.values()]
    out.append("%d" % len(queries))
    return "\n".join(out + queries) + "\n"


GENE, IV = ("start", "end", "tx_first", "tx_count"), ("start", "end")
TX = ("gene", "chrom", "strand", "exon_first", "exon_count", "expr_first", "expr_count")


def _end_queries(w, seq_range):
    """One query per cluster end of the case, and what the oracle's targets say it must print."""
    flat, fasta = w["models"].flatten(), w["fasta"]
    cidx, tidx, sidx = ({n: k for k, n in enumerate(v)} for v in (flat["chrom_names"], flat["transcript_names"], list(fasta)))
    clusters = ora.read_clusters(w["case"]["clusters"])
    by = {}
    for t in w["want"]["targets"]:
        by.setdefault((t["cluster_id"], t["cluster_end"]), []).append(t)
    queries, want = [], []
    for cid in clusters:
        for end in ("0", "1"):
            me, other = clusters[cid][end], clusters[cid]["1" if end == "0" else "0"]
            queries.append("E " + " ".join("%s %d %d %d" % (_hex(e["ref_name"]), "+-".index(e["strand"]), e["start"], e["end"]) for e in (me, other)) + " %d" % seq_range)
            mine = by.get((int(cid), int(end)), [])
            want.append("0 0 %d" % len(mine) + "".join(" | %d %d %d %d %d %d %d %d %d %d" % (
                t["kind"], tidx[t["name"]] if t["kind"] else cidx.get(t["name"], -1), sidx[t["seq_name"]], t["start"], t["len"], t["revcomp"], sidx[t["other_name"]],
                t["other_start"], t["other_len"], t["other_rev"]) for t in mine))
    return queries, want


def test_shared_header_as_a_host_program(cf, tmp_path):
    """conc_shared.hpp compiled by g++ into a stand-alone program under ASan + UBSan: every cluster end of the fixtures and of a
    random case gives the oracle's targets in canonical order; calc_genomic_position, calc_transcript_position and subseq agree
    with the oracle at every half-unit position from -2 to L + 2, every transcript of the fixtures' models; the name:a-b rule
    agrees with the regex."""
    from tests.test_sanitizers import BAD, ENV
    src = tmp_path / "conc_host.cpp"
    src.write_text(HOST % {"root": ROOT})
    exe = str(tmp_path / "conc_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-o", exe, str(src)])
    rng = random.Random(5)
    for name, seq_range in PERL + (("random2", 130), ("r2000", 2000)):
        w = named_world(name, seq_range)
        queries, want = _end_queries(w, seq_range)
        models, flat = w["models"], w["models"].flatten()
        for t, tx in enumerate(flat["transcript_names"]):
            length = ora.regions_length(models.transcripts[tx]["exons"])
            lo, hi = min(e[0] for e in models.transcripts[tx]["exons"]), max(e[1] for e in models.transcripts[tx]["exons"])
            for p2 in range(-4, 2 * length + 5):
                queries.append("G %d %d" % (t, p2))
                want.append("%d" % int(2 * ora.genomic_position(models, tx, Fraction(p2, 2))))
            for p2 in list(range(2 * lo - 4, 2 * hi + 5)) if name == "edges" else [rng.randrange(2 * lo - 4, 2 * hi + 5) for _ in range(20)]:
                queries.append("T %d %d" % (t, p2))
                want.append("%d" % int(2 * ora.transcript_position(models, tx, Fraction(p2, 2))))
        for length in (1, 2, 7):
            for a2 in range(-4, 2 * length + 5):
                for b2 in range(-4, 2 * length + 5):
                    queries.append("S %d %d %d" % (a2, b2, length))
                    a, b, rev = ora.subseq_bounds(Fraction(a2, 2), Fraction(b2, 2), length)
                    want.append("%d %d %d" % (a, b - a + 1, int(rev)))
        for text in ("chr1", "chr1:5-9", "a:1_0..2", "a:1,2", ":1-2", "a:1-", "a:-2", "a:1.2", "a:b:3-4", "chr1:5-9x", "1-2", "a:1-2-3", "a::1-2", "_:_-_"):
            queries.append("R " + _hex(text))
            want.append("%d" % bool(ora._RANGE_NAME.match(text)))
        path = tmp_path / (name + ".txt")
        path.write_text(_host_input(cf, w, queries))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV["asan"]), stdin=subprocess.DEVNULL, timeout=300)
        assert not any(b in r.stderr for b in BAD), (name, r.stderr[-3000:])
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        got = r.stdout.splitlines()
        assert len(got) == len(want)
        bad = [(q, g, x) for q, g, x in zip(queries, got, want) if g != x]
        assert not bad, (name, len(bad), bad[:5])
    # the two ends Perl dies on: the missing other sequence is seen by the rule itself
    w = named_world("edges", 40)
    path = tmp_path / "stops.txt"
    path.write_text(_host_input(cf, w, ["E %s 0 45 60 %s 1 10 40 40" % (_hex("chr1"), _hex("chrQ")), "E %s 0 45 60 %s 1 10 40 40" % (_hex(""), _hex("chr1"))]))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV["asan"]), stdin=subprocess.DEVNULL, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines() == ["%d 0 0" % cf.NO_OTHER_SEQ, "%d 0 0" % cf.EMPTY_NAME], (r.stdout, r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- on the GPU
def device_run(cf, w, seq_range, piece=None, extra_seqs=None, scores=SCORES):
    """The whole call sequence; dict(stages' results, targets, scores, align_text, filtered, dedup) or, on a stop, the result."""
    from defuse_amd import clusterregions, task
    fasta = dict(w["fasta"], **(extra_seqs or {}))
    with task.Reference(fasta) as ref, cf.Models(w["models"], list(fasta)) as models, clusterregions.Context() as cl, cf.Context() as ctx, \
            clusterregions.Context() as nxt:
        cl.begin()
        cl.add_pieces(w["case"]["clusters"], piece)
        r_targets = ctx.targets(cl, models, ref, seq_range)
        if r_targets["stop_kind"]:
            for call in (ctx.fetch_targets, lambda: ctx.align(ref, **scores), ctx.filter, lambda: ctx.fetch(cf.FILTERED)):
                with pytest.raises(cf.ConcFilterError) as err:      # a stop leaves no output
                    call()
                assert err.value.code == E_ARG
            return r_targets
        tg = ctx.fetch_targets()
        r_align = ctx.align(ref, **scores)
        got_scores = ctx.fetch_scores()
        r_filter = ctx.filter()
        align_text, filtered = ctx.fetch(cf.ALIGN_TEXT), ctx.fetch(cf.FILTERED)
        timing = ctx.timing()
        nxt.begin()
        cf.add_conc(nxt, ctx)
        r_dedup = nxt.dedup(1)
        dedup = None if r_dedup["stop_kind"] else nxt.fetch(clusterregions.DEDUP)
        return dict(targets=r_targets, align=r_align, filter=r_filter, tg=tg, scores=got_scores, align_text=align_text, filtered=filtered, dedup=dedup,
                    timing=timing, seq_names=list(fasta), fasta=fasta, flat=models.flat)


def check_against_oracle(cf, w, got):
    want = w["want"]
    flat, names, fasta = got["flat"], got["seq_names"], got["fasta"]
    assert got["targets"]["stop_kind"] == 0 and got["targets"]["n_targets"] == len(want["targets"]) == len(got["tg"])
    assert got["targets"]["n_lines"] == w["case"]["clusters"].count(b"\n")
    for k, (t, x) in enumerate(zip(got["tg"], want["targets"])):
        name = flat["transcript_names"][t["name"]] if t["kind"] else (flat["chrom_names"][t["name"]] if t["name"] >= 0 else names[t["seq"]])
        assert (int(t["cluster_id"]), int(t["cluster_end"]), int(t["kind"]), name, names[t["seq"]]) == (x["cluster_id"], x["cluster_end"], x["kind"], x["name"], x["seq_name"]), k
        seq = fasta[names[t["seq"]]][t["start"]:t["start"] + t["len"]]
        other = fasta[names[t["other_seq"]]][t["other_start"]:t["other_start"] + t["other_len"]]
        assert (ora.revcomp(seq) if t["revcomp"] else seq) == x["sequence"] and len(seq) == t["len"], (k, x["name"])
        assert (ora.revcomp(other) if t["other_rev"] else other) == x["other"] and len(other) == t["other_len"], (k, x["name"])
    kept = np.array(want["kept"], dtype=bool)
    assert np.array_equal(got["scores"][kept], np.array(want["scores"], dtype=np.int32)[kept])
    assert np.all(got["scores"][~kept] <= np.array(want["scores"], dtype=np.int32)[~kept])          # (below the minimum a score need not be exact)
    assert got["align_text"] == want["align_text"]
    assert got["filtered"] == want["filtered"]
    f = got["filter"]
    assert (f["n_kept_targets"], f["align_bytes"], f["out_bytes"], f["n_kept_lines"], f["n_noncanonical"], f["stop_kind"]) == \
        (int(kept.sum()), len(want["align_text"]), len(want["filtered"]), want["filtered"].count(b"\n"), 0, 0)
    assert f["n_hit_clusters"] == len({l.split(b"\t")[0] for l in want["align_text"].split(b"\n")[:-1]})
    host = cora.dedup(want["filtered"], 1)
    assert got["dedup"] == host[1]


GPU_CASES = (("edges", 40), ("edges", 130), ("random1", 40), ("random2", 40), ("random3", 130), ("random4", 40))


@pytest.mark.gpu
@pytest.mark.parametrize("name,seq_range", GPU_CASES)
def test_device_equals_the_oracle(cf, name, seq_range):
    """Descriptors, scores of the printed targets, both texts and the dedup that follows, on the fixtures and on three seeded
    random cases of 50 clusters over 5 contigs and 20 genes; R = 40 is one 64-column tile, R = 130 windows of up to 131."""
    w = named_world(name, seq_range)
    got = device_run(cf, w, seq_range)
    check_against_oracle(cf, w, got)
    assert got["timing"]["n_packed16"] == len(w["want"]["targets"]) and got["timing"]["cells"] > 0


@pytest.mark.gpu
def test_tile_boundary_windows(cf):
    """R = 130 clipped to windows of 64 and of 65 columns: ends 64 and 65 bases before a contig's end."""
    base = fixture_case("edges")
    case = cases.with_clusters(base, [cases.cl(1, 0, 1, "chr1", "+", 330, 344), cases.cl(1, 1, 1, "chr1", "-", 350, 380),       # midpoint 337: [337, 400]
                                      cases.cl(2, 0, 1, "chr1", "+", 330, 342), cases.cl(2, 1, 1, "chr1", "-", 350, 380)])      # midpoint 336: [336, 400]
    w = world("tiles", case, 130)
    got = device_run(cf, w, 130)
    check_against_oracle(cf, w, got)
    assert sorted(int(t["len"]) for t in got["tg"] if t["kind"] == 0 and t["cluster_end"] == 0) == [64, 65]


@pytest.mark.gpu
def test_pipeline_range_and_both_kernels(cf):
    """R = 2000 with six clusters and other ends of 18, 64, 65, 300 and 1900 bases: the 1900-row pairs go to the int32 kernel,
    the others to the packed one, in one call."""
    w = named_world("r2000", 2000)
    got = device_run(cf, w, 2000)
    check_against_oracle(cf, w, got)
    assert sorted({int(t["other_len"]) for t in got["tg"]}) == [18, 31, 41, 61, 64, 65, 300, 1900]
    assert got["timing"]["n_int32"] == sum(1 for t in got["tg"] if t["other_len"] == 1900) > 0 and got["timing"]["n_packed16"] > 0
    assert max(int(t["len"]) for t in got["tg"]) == 2001


@pytest.mark.gpu
@pytest.mark.parametrize("piece", (1, 37, 4096))
def test_text_in_pieces(cf, piece):
    """The cluster text added in pieces cut inside a line (a piece of one byte sends every line up on its own)."""
    w = named_world("edges", 40)
    check_against_oracle(cf, w, device_run(cf, w, 40, piece=piece))


@pytest.mark.gpu
def test_no_targets_no_kept_lines_no_lines(cf):
    base = fixture_case("edges")
    none = world("no_targets", cases.with_clusters(base, [cases.cl(4, 0, 1, "G7|T1", "+", 5, 20), cases.cl(4, 1, 1, "G7|T1", "-", 8, 25)]), 40)
    got = device_run(cf, none, 40)
    check_against_oracle(cf, none, got)
    assert got["targets"]["n_targets"] == 0 and got["align_text"] == b"" and got["filtered"] == none["case"]["clusters"]
    lines = fixture_case("edges")["clusters"].split(b"\n")
    all_hit = world("all_hit", dict(base, clusters=b"".join(l + b"\n" for l in lines if l.split(b"\t")[0] in (b"1", b"9"))), 40)
    got = device_run(cf, all_hit, 40)
    check_against_oracle(cf, all_hit, got)
    assert got["filtered"] == b"" and got["filter"]["n_hit_clusters"] == 2 and got["dedup"] == b""
    empty = world("empty", dict(base, clusters=b""), 40)
    got = device_run(cf, empty, 40)
    assert (got["targets"]["n_targets"], got["align_text"], got["filtered"], got["dedup"]) == (0, b"", b"", b"")


@pytest.mark.gpu
def test_noncanonical_ids_are_counted(cf):
    base = fixture_case("edges")
    text = (cases.cl(7, 0, 1, "chr1", "+", 250, 270) + "007\t1\t1\t0\tchr2\t-\t250\t280\n" + cases.cl(8, 0, 1, "chr1", "+", 101, 130) +
            "+8\t1\t2\t0\tchr1\t-\t120\t149\n").encode()
    w = world("odd_ids", dict(base, clusters=text), 40)
    got = device_run(cf, w, 40)
    assert got["filter"]["n_noncanonical"] == 2 and got["filter"]["n_hit_clusters"] == 1
    assert got["filtered"] == b"".join(l + b"\n" for l in text.split(b"\n")[:2])          # ids compare by value: "+8" goes with 8


@pytest.mark.gpu
def test_every_stop_leaves_no_output(cf):
    base = fixture_case("edges")
    good = cases.cl(1, 0, 1, "chr1", "+", 101, 130) + cases.cl(1, 1, 1, "chr1", "-", 120, 149)
    stops = (
        (good + "2\t0\t1\t0\tchr1\t+\t45\n", cf.FEW_FIELDS, dict(stop_line=3)),
        (good + "2\t0\t1\t0\tchr1\t+\t45\tx\n", cf.BAD_INTEGER, dict(stop_line=3, stop_field=7)),
        (good + cases.cl(2, 0, 1, "chr1", "+", 45, 60), cf.NOT_TWO_ENDS, dict(stop_value=2)),
        (good + cases.cl(2, 0, 1, "chr1", "+", 45, 60) + cases.cl(2, 2, 1, "chr1", "-", 105, 135), cf.NOT_TWO_ENDS, dict(stop_value=2)),
        (good + cases.cl(2, 0, 1, "chr1", "*", 45, 60) + cases.cl(2, 1, 1, "chr1", "-", 105, 135), cf.BAD_STRAND, dict(stop_value=2)),
        (good + cases.cl(2, 0, 1, "", "+", 45, 60) + cases.cl(2, 1, 1, "chr1", "-", 105, 135), cf.EMPTY_NAME, dict(stop_value=2)),
        (good + cases.cl(3, 0, 1, "chr1", "+", 45, 60) + cases.cl(3, 1, 1, "chrQ", "-", 10, 40), cf.NO_OTHER_SEQ, dict(stop_value=3)),
        (good + cases.cl(3, 0, 1, "chr1", "+", 45, 60) + cases.cl(3, 1, 1, "void", "-", 10, 40), cf.EMPTY_OTHER, dict(stop_value=3)),
    )
    for k, (text, kind, more) in enumerate(stops):
        w = world("stop%d" % k, dict(base, clusters=text.encode()), 40)
        got = device_run(cf, w, 40, extra_seqs={"void": b""})
        assert got["stop_kind"] == kind and all(got[f] == v for f, v in more.items()), (k, got)
        assert got["n_targets"] == 0 and got["out_bytes"] == 0
    assert isinstance(named_world("one_end", 40)["want"], ora.Stop) and isinstance(named_world("missing_other", 40)["want"], ora.Stop)
    for text, code in ((good + cases.cl(2, 0, 1, "chr1:5-9", "+", 45, 60) + cases.cl(2, 1, 1, "chr1", "-", 105, 135), E_LIMIT),
                       (good + cases.cl(2, 0, 1, "chr1", "+", 45, 2 ** 28 + 1) + cases.cl(2, 1, 1, "chr1", "-", 105, 135), E_LIMIT)):
        with pytest.raises(cf.ConcFilterError) as err:
            device_run(cf, world("limit%d" % len(text), dict(base, clusters=text.encode()), 40), 40)
        assert err.value.code == code
    with pytest.raises(cf.ConcFilterError) as err:
        device_run(cf, named_world("edges", 40), 2 ** 20 + 1)
    assert err.value.code == E_LIMIT
