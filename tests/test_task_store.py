"""The tasks of the split-read chain made on the GPU (include/defuse_task.h through defuse_amd/task.py).

Yardstick: oracle/dosplitalign_oracle.py:make_task on the same inputs, which restates tools/SplitAlignment.cpp:31-175 with
FastaIndex::Get and ExonRegions; every field, every byte of both pools and every mate region is compared, without tolerance.
The case builders below run without a GPU; each GPU test first asserts, on the oracle's own results, that its cases reach the
edges it is about."""
import ctypes
import os
import random
import subprocess
from collections import OrderedDict

import numpy as np
import pytest

from tests import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "tests", "golden", "smoke")
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
PLUS, MINUS = 0, 1
ODD_BYTES = b"ACGTNacgtn.\x00\xff*"


@pytest.fixture(scope="module")
def task(built):
    from defuse_amd import task as t
    return t


# ---------------------------------------------------------------------------------------------- worlds and the checker
def text(rng, n, alphabet=ODD_BYTES):
    return bytes(alphabet[rng.randrange(len(alphabet))] for _ in range(int(n)))


def loc(name, strand, start, end):
    return dict(refName=name, strand=strand, start=start, end=end)


class World:
    """One reference and one exon table, for the oracle and (device=True) on the GPU.  seqs: {name: bytes};
    table: {transcript: (gene, chromosome, strand, [(start, end)])}."""

    def __init__(self, seqs, table, tmp, task=None):
        from oracle import dosplitalign_oracle as ora
        self.ora, self.seqs, self.table = ora, seqs, table
        self.fasta = ora.FastaIndex.__new__(ora.FastaIndex)
        self.fasta.seqs = dict(seqs)
        path = os.path.join(str(tmp), "exons.%d.txt" % id(self))
        with open(path, "w") as f:
            for t, (gene, chrom, strand, exons) in table.items():
                f.write("\t".join([gene, t, chrom, "+-"[strand]] + [str(v) for e in exons for v in e]) + "\n")
        self.oexons = ora.ExonRegions(path)
        self.names = {}
        self.ref = self.exons = None
        if task is not None:
            self.ref = task.Reference(seqs)
            self.exons = task.Exons(table, self.names)

    def close(self):
        for h in (self.ref, self.exons):
            if h is not None:
                h.close()

    def want(self, params, regions):
        """Per task the oracle's Task, or the message it exits with."""
        u, s, minr, maxr = params
        out = []
        for fid, pair in regions.items():
            try:
                out.append(self.ora.make_task(fid, pair, self.fasta, self.oexons, u, s, minr, maxr))
            except SystemExit as e:
                out.append(str(e))
        return out


def int_params(params):
    u, s, minr, maxr = params
    return (int(u - 3 * s), int(u + 3 * s), minr, maxr)


def check(W, regions, want, fetched):
    """Every record, both pools and the regions of a fetched store against the oracle's tasks."""
    from defuse_amd import cand
    rec, win, rem, reg = fetched
    assert len(rec) == len(want) == len(regions)
    R = {k: rec[k].tolist() for k in rec.dtype.names}
    G = [tuple(int(v) for v in r) for r in reg.tolist()]
    woff = roff = goff = 0
    clean = all(not isinstance(t, str) for t in want)
    for k, ((fid, pair), t) in enumerate(zip(regions.items(), want)):
        assert R["fusion_id"][k] == fid
        if isinstance(t, str):
            low = R["status"][k] & -R["status"][k]
            assert low in (1, 2, 4, 8), (k, t, R["status"][k])
            e = 0 if low < 4 else 1
            msg = ("Error: Unable to find sequence for " if low in (1, 4) else "Error: Data mismatch, invalid chromosome ") + pair[e]["refName"]
            assert msg == t, (k, R["status"][k])
            continue
        assert R["status"][k] == 0, (k, R["status"][k])
        assert (R["seq_start"][k], R["seq_len"][k], R["seq_strand"][k]) == (t.seq_start, t.seq_len, t.seq_strand), (k, pair)
        assert R["rem_len"][k] == [len(t.remainder[0]), len(t.remainder[1])], (k, pair)
        assert R["n_regions"][k] == [len(t.mate_regions[0]), len(t.mate_regions[1])], (k, pair, R["n_regions"][k])
        g = R["region_off"][k]
        for e in (0, 1):
            o = R["win_off"][k][e]
            assert win[o:o + len(t.seq[e])].tobytes() == t.seq[e] and len(t.seq[e]) == max(t.seq_len[e], 0), (k, e, pair)
            o = R["rem_off"][k][e]
            assert rem[o:o + len(t.remainder[e])].tobytes() == t.remainder[e], (k, e, pair)
            exp = [(W.names[m["refName"]], m["strand"], m["start"], m["end"], cand.cluster_id(fid, e)) for m in t.mate_regions[e]]
            assert G[g:g + len(exp)] == exp, (k, e, pair, G[g:g + len(exp)], exp)
            g += len(exp)
        if clean:           # the pools are plain concatenations in input order: no byte and no region belongs to nobody
            assert (R["win_off"][k], R["rem_off"][k], R["region_off"][k]) == ([woff, woff + len(t.seq[0])], [roff, roff + len(t.remainder[0])], goff), k
            woff += len(t.seq[0]) + len(t.seq[1])
            roff += len(t.remainder[0]) + len(t.remainder[1])
            goff += len(t.mate_regions[0]) + len(t.mate_regions[1])
    if clean:
        assert (len(win), len(rem), len(reg)) == (woff, roff, goff)
        assert win.tobytes() == b"".join(t.seq[0] + t.seq[1] for t in want)
        assert rem.tobytes() == b"".join(t.remainder[0] + t.remainder[1] for t in want)


def run(task, W, params, regions):
    want = W.want(params, regions)
    pairs = task.pairs_from_regions(regions, W.ref, W.exons)
    with task.Store(W.ref, W.exons, int_params(params), pairs) as st:
        fetched = st.fetch()
        c, tm = st.counts(), st.timing()
        assert (c.n_tasks, c.window_bytes, c.rem_bytes, c.n_regions) == (len(pairs), len(fetched[1]), len(fetched[2]), len(fetched[3]))
        assert (tm["n_tasks"], tm["window_bytes"], tm["rem_bytes"], tm["n_regions"]) == (c.n_tasks, c.window_bytes, c.rem_bytes, c.n_regions)
    check(W, regions, want, fetched)
    return want, fetched


def window_request(W, params, a):
    """(s0, l0): what Initialize asks FastaIndex::Get for."""
    u, s, minr, maxr = params
    bstart, blen = W.ora.calculate_break_region(minr, maxr, int(u + 3 * s), a["start"], a["end"], a["strand"])
    return (bstart - maxr if a["strand"] == PLUS else bstart - blen + 1), blen + maxr


def pair_up(ends, shift):
    """End k with end k + shift as the two ends of task k: every end is met as end 0 and as end 1."""
    return OrderedDict((k, [ends[k], ends[(k + shift) % len(ends)]]) for k in range(len(ends)))


# ---------------------------------------------------------------------------------------------- the cases (no GPU needed)
def cut_edge_cases():
    rng = random.Random(11)
    seqs = OrderedDict([("pad", b"xyz"), ("chrA", text(rng, 83))])
    table = {"tA": ("gA", "chrA", PLUS, [(10, 30)]), "tX": ("gX", "chrX", MINUS, [(5, 9)])}
    params = (40, 0, 5, 8)
    ends = [loc("chrA", strand, start, start + n - 1) for strand in (PLUS, MINUS) for start in range(-45, 126, 2) for n in (1, 2, 3, 7, 17, 18, 20, 41, 62, 75)]
    # maxFragment < minRead: the window is asked for with a length below 0 and no remainder is asked for; chrX is a chromosome
    # of the exon table that the FASTA does not have
    odd_params = (10, 0, 20, 4)
    odd = [loc(name, strand, start, start + n - 1) for name in ("chrX", "chrA") for strand in (PLUS, MINUS) for start in (-3, 1, 40) for n in (1, 2, 5)]
    return seqs, table, [(params, pair_up(ends, 397)), (odd_params, pair_up(odd, 7))]


def cut_edge_coverage(W, cases):
    seen = set()
    for params, regions in cases:
        for pair, t in zip(regions.values(), W.want(params, regions)):
            assert not isinstance(t, str), t
            for e in (0, 1):
                a = pair[e]
                L = len(W.seqs.get(a["refName"], b""))
                s0, l0 = window_request(W, params, a)
                if l0 < 0:
                    assert (t.seq_start[e], t.seq_len[e], t.seq[e]) == (s0, l0, b"")
                    seen.add("negative length" + (", no such sequence" if a["refName"] not in W.seqs else ""))
                    continue
                if s0 < 1:
                    seen.add("start below 1")
                    assert t.seq_start[e] == 1
                end = t.seq_start[e] + (l0 - (1 - s0 if s0 < 1 else 0)) - 1
                if end > L and t.seq_len[e] > 0:
                    seen.add("end beyond the sequence")
                if end < 0:
                    assert t.seq_len[e] == L
                    seen.add("wholly in front")
                if s0 > L:
                    assert t.seq_len[e] == 0
                    seen.add("start beyond the end")
                n = len(t.remainder[e])
                strand = "plus" if a["strand"] == PLUS else "minus"
                asked = a["start"] < t.seq_start[e] if a["strand"] == PLUS else a["end"] > t.seq_start[e] + t.seq_len[e] - 1
                if asked:
                    seen.add("remainder on %s, %s" % (strand, "0" if n == 0 else "1" if n == 1 else "several"))
    need = {"negative length", "negative length, no such sequence", "start below 1", "end beyond the sequence", "wholly in front", "start beyond the end"}
    need |= {"remainder on %s, %s" % (s, n) for s in ("plus", "minus") for n in ("0", "1", "several")}
    assert need <= seen, need - seen


def word_edge_cases():
    rng = random.Random(12)
    # the sequences end at byte offsets 42, 87, 128 and 173 of the reference: every phase of a window clipped at its end
    seqs = OrderedDict([("p", b"#"), ("chrA", text(rng, 41)), ("q", b"##"), ("chrB", text(rng, 43)), ("chrC", text(rng, 41)), ("chrD", text(rng, 45))])
    table = {"t" + c: ("g", "chr" + c, k & 1, [(10, 30)]) for k, c in enumerate("ABCD")}
    params = (12, 0, 3, 8)                      # windows of 17 or 16 bytes before clipping, remainders of region length - 16
    ends = [loc(name, strand, start, start + n - 1) for name in ("chrA", "chrB", "chrC", "chrD") for strand in (PLUS, MINUS) for start in range(-20, 52)
            for n in (1, 2, 17, 18, 19, 21, 23, 24, 25, 31, 32, 33)]
    return seqs, table, [(params, pair_up(ends, 1231))]


def word_edge_coverage(W, want, fetched):
    rec = fetched[0]
    off = {}
    o = 0
    for name, s in W.seqs.items():
        off[name] = o
        o += len(s)
    wins, rems = set(), set()
    for k, t in enumerate(want):
        for e in (0, 1):
            rev = t.seq_strand[e]
            # the window's first source byte: start - 1 of its sequence (an empty window has none)
            if t.seq[e]:
                wins.add((len(t.seq[e]), (off[t.ref_name[e]] + t.seq_start[e] - 1) % 4, int(rec["win_off"][k][e]) % 4, rev))
            else:
                wins.add((0, None, None, rev))
            rems.add((len(t.remainder[e]), int(rec["rem_off"][k][e]) % 4, rev))
    lens = set(range(0, 10)) | {15, 16, 17}
    for rev in (0, 1):
        assert lens <= {w[0] for w in wins if w[3] == rev}, (rev, sorted({w[0] for w in wins if w[3] == rev}))
        assert lens <= {r[0] for r in rems if r[2] == rev}, (rev, sorted({r[0] for r in rems if r[2] == rev}))
        for n in lens - {0}:
            assert {w[1] for w in wins if w[0] == n and w[3] == rev} == {0, 1, 2, 3}, (n, rev)
            assert {w[2] for w in wins if w[0] == n and w[3] == rev} == {0, 1, 2, 3}, (n, rev)
            assert {r[1] for r in rems if r[0] == n and r[2] == rev} == {0, 1, 2, 3}, (n, rev)


def exon_cases():
    rng = random.Random(13)
    table = {
        "t1p": ("g1", "chr1", PLUS, [(100, 200)]),
        "t1m": ("g1", "chr1", MINUS, [(300, 420)]),
        "t2p": ("g2", "chr1", PLUS, [(500, 560), (700, 790)]),
        "t2m": ("g2", "chr1", MINUS, [(520, 600), (640, 700)]),         # overlaps t2p
        "t3p": ("g3", "chr1", PLUS, [(900, 950), (1000, 1040), (1100, 1180)]),
        "t3m": ("g3", "chr1", MINUS, [(920, 960), (1010, 1050), (1120, 1170)]),
        "t3x": ("g4", "chr1", PLUS, [(940, 1000), (1150, 1400)]),
        # around a bin border of 100000; the names interleave the bins: ua (bin 0), ub (bin 1), uc (bin 0), ud (both), ue (bin 1)
        "ua": ("h", "chr2", PLUS, [(99800, 99900)]),
        "ub": ("h", "chr2", MINUS, [(100020, 100090)]),
        "uc": ("h", "chr2", PLUS, [(99930, 99990)]),
        "ud": ("h", "chr2", MINUS, [(99950, 99999), (100000, 100060)]),
        "ue": ("h", "chr2", PLUS, [(100100, 100200), (100300, 100400)]),
    }
    seqs = OrderedDict([("chr1", text(rng, 1500, b"ACGTNacgtn")), ("chr2", text(rng, 300, b"ACGTNacgtn"))])
    for t, (gene, _, _, exons) in table.items():
        seqs[gene + "|" + t] = text(rng, sum(e - b + 1 for b, e in exons), b"ACGTNacgtn")
    cases = []
    # ends that name a transcript: every break position along it and beyond its end
    params = (100, 10, 20, 30)
    ends = []
    for t, (gene, _, _, exons) in table.items():
        tlen = sum(e - b + 1 for b, e in exons)
        step = 1 if t[0] == "t" else 7
        ends += [loc(gene + "|" + t, strand, start, start + n - 1) for strand in (PLUS, MINUS) for start in range(-5, tlen + 40, step) for n in (1, 24)]
    cases.append((params, pair_up(ends, 911)))
    # genomic ends base by base past the transcripts of chr1 (a short mate region: 25 bases) and over the bin border of chr2
    short = (40, 1, 30, 36)
    ends = [loc("chr1", strand, start, start + 9) for strand in (PLUS, MINUS) for start in list(range(-20, 130)) + list(range(380, 620)) + list(range(850, 1500))]
    cases.append((short, pair_up(ends, 577)))
    ends = [loc("chr2", strand, start, start + n - 1) for strand in (PLUS, MINUS) for start in range(99700, 100500, 3) for n in (10, 300)]
    cases.append((params, pair_up(ends, 311)))
    # long align regions: mateMin far above 0 (the third way out of RemapThroughTranscript)
    ends = [loc("chr1", strand, start, start + n - 1) for strand in (PLUS, MINUS) for start in range(0, 1300, 5) for n in (180, 260)]
    cases.append((params, pair_up(ends, 211)))
    return seqs, table, cases


def classify_remap(ex, transcript, position, strand, ext_min, ext_max):
    """The way RemapThroughTranscript (oracle.remap_through_transcript) leaves, and what it met on the way."""
    exons = ex.exons_str[strand][transcript]
    tlen, tstrand = ex.length[transcript], ex.strand[transcript]
    sp = position if strand == PLUS else -position
    if sp > exons[-1][1]:
        return {"out: beyond the last exon"}
    off = 0
    for k, (b, e) in enumerate(exons):
        if sp <= e:
            rs, re_ = sp - b + ext_min + 1, sp - b + ext_max + 1
            if re_ < 1:
                return {"out: end below 1"}
            tags = {"found in exon %d of %d" % (k + 1, len(exons))}
            if rs < 1:
                tags.add("start clamped")
            if max(1, rs) + off > tlen:
                return tags | {"out: start beyond the transcript"}
            tags.add("swapped" if strand != tstrand else "not swapped")
            return tags | {"remapped"}
        off += e - b + 1
    raise AssertionError("unreachable")


def exon_coverage(W, cases):
    ex, seen = W.oexons, set()
    for params, regions in cases:
        u, s, minr, maxr = params
        for pair, t in zip(regions.values(), W.want(params, regions)):
            assert not isinstance(t, str), t
            for e in (0, 1):
                a = pair[e]
                bstart, blen = W.ora.calculate_break_region(minr, maxr, int(u + 3 * s), a["start"], a["end"], a["strand"])
                parts = a["refName"].split("|")
                if len(parts) == 2:
                    tr = parts[1]
                    pos = bstart if ex.strand[tr] == PLUS else ex.length[tr] - bstart + 1
                    off, where = 0, "past the last exon"
                    for k, (b, en) in enumerate(ex.exons[tr]):
                        n = en - b + 1
                        if pos <= off + n:
                            where = "exon %d of %d" % (k + 1, len(ex.exons[tr]))
                            if pos == off + 1:
                                seen.add("break at an exon's first base")
                            if pos == off + n:
                                seen.add("break at an exon's last base")
                            break
                        off += n
                    seen.add("break in " + where + " on " + "+-"[ex.strand[tr]])
                g = t.mate_regions[e][0]
                q0, q1 = g["start"], g["end"]
                if q0 < 0:
                    seen.add("negative start")
                if q0 > q1:
                    seen.add("inverted mate region" + (", two bins" if q0 // 100000 != q1 // 100000 else ""))
                mate_min, mate_max = int(u - 3 * s) - blen - maxr + 1, int(u + 3 * s) - minr
                gb = q0 + mate_max if g["strand"] == PLUS else q0 - mate_min
                hits = ex.region_transcripts(g["refName"], (q0, q1))
                seen.add("overlaps %s" % ("none" if not hits else "one" if len(hits) == 1 else "several"))
                if q0 // 100000 != q1 // 100000 and q0 >= 0:
                    seen.add("two bins, %d transcripts" % len(hits))
                for tr, (r0, r1) in ex.region.items():
                    if ex.chromosome[tr] == g["refName"] and q0 <= q1:
                        for tag, cond in (("touches on the left", r1 == q0), ("touches on the right", r0 == q1), ("one short on the left", r1 == q0 - 1),
                                          ("one short on the right", r0 == q1 + 1)):
                            if cond:
                                seen.add(tag)
                                assert (tr in hits) == tag.startswith("touches")
                n_ok = 0
                for tr in hits:
                    tags = classify_remap(ex, tr, gb, 1 - g["strand"], mate_min, mate_max)
                    n_ok += "remapped" in tags
                    seen |= tags
                assert n_ok == len(t.mate_regions[e]) - 1
                seen.add("regions per end: %s" % min(len(t.mate_regions[e]), 4))
    need = {"break at an exon's first base", "break at an exon's last base", "negative start", "overlaps none", "overlaps one", "overlaps several",
            "touches on the left", "touches on the right", "one short on the left", "one short on the right", "out: beyond the last exon",
            "out: end below 1", "out: start beyond the transcript", "start clamped", "swapped", "not swapped", "two bins, 3 transcripts",
            "regions per end: 1", "regions per end: 2", "regions per end: 3"}
    need |= {"break in exon %d of %d on %s" % (k, n, s) for n in (1, 2, 3) for k in range(1, n + 1) for s in "+-"}
    need |= {"break in past the last exon on +", "break in past the last exon on -"}
    need |= {"found in exon %d of %d" % (k, n) for n in (1, 2, 3) for k in range(1, n + 1)}
    assert need <= seen, sorted(need - seen)


def random_case(seed):
    rng = random.Random(seed)
    seqs, table = OrderedDict(), {}
    chroms = ["chr%d" % c for c in range(4)]
    for c in chroms:
        seqs[c] = text(rng, rng.randint(300, 3000), b"ACGTNacgtn")
    for k in range(30):
        c = chroms[k] if k < 4 else rng.choice(chroms)           # every chromosome has a transcript
        L = len(seqs[c])
        cuts = sorted(rng.sample(range(1, L), 2 * rng.randint(1, 4)))
        table["T%02d" % k] = ("G%d" % (k // 2), c, rng.randint(0, 1), [(cuts[2 * j], cuts[2 * j + 1]) for j in range(len(cuts) // 2)])
    for t, (gene, _, _, exons) in table.items():
        seqs[gene + "|" + t] = text(rng, sum(e - b + 1 for b, e in exons), b"ACGTNacgtn")
    names = list(seqs)
    cases = []
    fids = rng.sample(range(2 ** 31), 300)
    for k, params in enumerate([(100, 10, 20, 30), (60, 5, 25, 25), (300, 30, 50, 50), (40, 0, 30, 36)]):
        regions = OrderedDict()
        for fid in fids[75 * k:75 * (k + 1)]:
            pair = []
            for e in (0, 1):
                name = rng.choice(names)
                start = rng.randint(-40, len(seqs[name]) + 40)
                pair.append(loc(name, rng.randint(0, 1), start, start + rng.randint(1, 120) - 1))
            regions[fid] = pair
        cases.append((params, regions))
    return seqs, table, cases


# ---------------------------------------------------------------------------------------------- without a GPU
def test_task_header_and_binding_agree(task):
    """sizeof and offsetof of every struct of the header, as g++ and gcc -std=c99 see them, against the ctypes structs and
    the numpy dtypes; the constants; every declared function bound and exported."""
    consts = {"TASK_NO_SEQUENCE_0": task.NO_SEQUENCE_0, "TASK_BAD_CHROMOSOME_0": task.BAD_CHROMOSOME_0, "TASK_NO_SEQUENCE_1": task.NO_SEQUENCE_1,
              "TASK_BAD_CHROMOSOME_1": task.BAD_CHROMOSOME_1, "TASK_MAX_COORD": task.MAX_COORD, "TASK_MAX_REGION": task.MAX_REGION,
              "TASK_MAX_PARAM": task.MAX_PARAM, "TASK_MAX_SEQ_LEN": task.MAX_SEQ_LEN, "TASK_EXON_BIN": task.EXON_BIN}
    pairs = ((task.Pair, task.PAIR_DTYPE, 52), (task.Record, task.RECORD_DTYPE, 80), (task.End, task.END_DTYPE, 24), (task.Seq, task.SEQ_DTYPE, 16),
             (task.Transcript, task.TRANSCRIPT_DTYPE, 20), (task.Exon, task.EXON_DTYPE, 8))
    sizes, n = abi.check("defuse_task.h", task, r"task_[a-z_]+", constants=consts, dtypes=[(st, dt) for st, dt, _ in pairs])
    assert "%d %d %d %d " % tuple(consts.values())[:4] == "1 2 4 8 "
    for st, dt, size in pairs:
        assert ctypes.sizeof(st) == dt.itemsize == size
    assert (ctypes.sizeof(task.Params), ctypes.sizeof(task.Counts), ctypes.sizeof(task.TaskTiming)) == (16, 32, 64)
    assert len(sizes) == 9 and n == 12


def test_task_argument_errors_need_no_device(task):
    lib = task.lib()
    err = lambda: lib.task_last_error().decode()
    h = ctypes.c_void_p()
    one = ctypes.c_void_p(1)           # stands for an object: the argument errors are found before any is looked at
    ptr = lambda a: a.ctypes.data if len(a) else None

    # ---- task_reference_create
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)

    def reference(seqs, n=None, nbytes=len(data), out=h, device=0):
        s = np.array(seqs, dtype=task.SEQ_DTYPE).reshape(-1)
        return lib.task_reference_create(device, data.ctypes.data if nbytes else None, nbytes, ptr(s), len(s) if n is None else n,
                                         ctypes.byref(out) if out is not None else None)
    assert reference([(0, 4)], out=None) == E_ARG
    assert reference([(0, 4)], n=-1) == E_ARG and "negative" in err()
    assert reference([(0, 4)], nbytes=-1) == E_ARG and "negative" in err()
    assert reference([], n=1) == E_ARG and "null" in err()
    assert reference([], n=2 ** 31) == E_LIMIT
    assert reference([(0, 4), (4, 7)]) == E_ARG and "sequence 1" in err() and "outside" in err()
    assert reference([(-1, 2)]) == E_ARG and "sequence 0" in err()
    assert reference([(0, 10), (2 ** 62, 2 ** 62)]) == E_ARG and "sequence 1" in err()            # no overflow of off + len
    assert reference([(0, -1)]) == E_ARG and "sequence 0" in err()
    assert lib.task_reference_create(0, one, 2 ** 40, ptr(np.array([(0, 4), (5, 2 ** 30 + 1)], dtype=task.SEQ_DTYPE)), 2, ctypes.byref(h)) == E_LIMIT \
        and "sequence 1" in err()
    assert reference([(0, 4)], device=999) == E_DEVICE and "999" in err() and not h

    # ---- task_exons_create
    def exons(tx, ex, chrom_ref=(3, 4), out=h, device=0, n_ex=None):
        c = np.array(chrom_ref, dtype=np.int32)
        t = np.array(tx, dtype=task.TRANSCRIPT_DTYPE).reshape(-1)
        e = np.array(ex, dtype=task.EXON_DTYPE).reshape(-1)
        return lib.task_exons_create(device, ptr(c), len(c), ptr(t), len(t), ptr(e), len(e) if n_ex is None else n_ex, ctypes.byref(out) if out is not None else None)
    good_tx, good_ex = [(0, 0, 0, 2, 7), (1, 1, 2, 1, 8)], [(10, 20), (30, 40), (5, 9)]
    assert exons(good_tx, good_ex, out=None) == E_ARG
    assert exons(good_tx, good_ex, n_ex=-1) == E_ARG and "negative" in err()
    assert exons(good_tx, [], n_ex=3) == E_ARG and "null" in err()
    assert exons(good_tx, good_ex, chrom_ref=(3, -4)) == E_ARG and "chromosome 1" in err()
    assert exons([(0, 0, 0, 2, 7), (1, 1, 2, 0, 8)], good_ex) == E_ARG and "transcript 1" in err() and "no exons" in err()
    assert exons([(0, 0, 0, 2, 7), (1, 1, 2, 2, 8)], good_ex) == E_ARG and "transcript 1" in err() and "outside" in err()
    assert exons([(0, 0, -1, 2, 7)], good_ex) == E_ARG and "transcript 0" in err()
    assert exons([(2, 0, 0, 2, 7)], good_ex) == E_ARG and "transcript 0" in err() and "chromosome 2" in err()
    assert exons([(-1, 0, 0, 2, 7)], good_ex) == E_ARG and "chromosome -1" in err()
    assert exons([(0, 2, 0, 2, 7)], good_ex) == E_ARG and "strand 2" in err()
    assert exons([(0, 0, 0, 2, -7)], good_ex) == E_ARG and "name_ref" in err()
    assert exons(good_tx, [(10, 20), (30, 2 ** 28 + 1), (5, 9)]) == E_LIMIT and "transcript 0" in err() and "exon 1" in err()
    assert exons(good_tx, [(10, 20), (30, 40), (-2 ** 28 - 1, 9)]) == E_LIMIT and "transcript 1" in err() and "exon 0" in err()
    assert exons(good_tx, [(-2 ** 27, 2 ** 27), (30, 40), (5, 9)]) == E_LIMIT and "transcript 0" in err() and "cover" in err()
    assert exons(good_tx, [(2 ** 27, -2 ** 27), (30, 40), (5, 9)]) == E_LIMIT and "transcript 0" in err()          # a negative length counts as its size
    assert exons(good_tx, good_ex, device=999) == E_DEVICE and "999" in err() and not h

    # ---- task_store_create
    def pair(fid=5, e0=(0, -1, 0, 0, 100, 150), e1=(1, 0, -1, 1, 30, 60)):
        p = np.zeros(1, dtype=task.PAIR_DTYPE)
        p["fusion_id"] = fid
        p["end"][0][0], p["end"][0][1] = e0, e1
        return p

    def store(pairs, params=(70, 130, 20, 30), n=None, ref=one, ex=one, out=h):
        p = np.concatenate(pairs) if pairs else np.zeros(0, dtype=task.PAIR_DTYPE)
        prm = task.Params(*params) if params is not None else None
        return lib.task_store_create(ref, ex, ctypes.byref(prm) if prm is not None else None, ptr(p), len(p) if n is None else n,
                                     ctypes.byref(out) if out is not None else None)
    good = pair()
    assert store([good], out=None) == E_ARG
    assert store([good], params=None) == E_ARG and "no params" in err()
    assert store([good], params=(70, 130, -1, 30)) == E_ARG and "negative read length" in err()
    assert store([good], params=(70, 130, 20, -30)) == E_ARG and "negative read length" in err()
    for bad in ((70, 130, 20, 2 ** 20 + 1), (70, 130, 2 ** 20 + 1, 30), (70, 2 ** 20 + 1, 20, 30), (-2 ** 20 - 1, 130, 20, 30), (70, -2 ** 20 - 1, 20, 30)):
        assert store([good], params=bad) == E_LIMIT and "params" in err(), bad
    assert store([good], n=-1) == E_ARG and "negative" in err()
    assert store([], n=1) == E_ARG and "null" in err()
    assert store([], n=2 ** 30) == E_LIMIT
    assert store([good, pair(-1)]) == E_ARG and "pair 1" in err() and "fusion_id -1" in err()
    assert store([good, pair(6), pair(5)]) == E_ARG and "pairs 0 and 2" in err() and "fusion_id 5" in err()
    assert store([pair(9), pair(2 ** 31 - 1), pair(3), pair(2 ** 31 - 1)]) == E_ARG and "pairs 1 and 3" in err()
    assert store([good, pair(6, e1=(1, 0, -1, 2, 30, 60))]) == E_ARG and "pair 1" in err() and "end[1].strand 2" in err()
    assert store([pair(e0=(0, -1, 0, -1, 100, 150))]) == E_ARG and "pair 0" in err() and "end[0].strand -1" in err()
    for bad in ((-2, -1, 0, 0, 100, 150), (0, -2, 0, 0, 100, 150), (0, -1, -2, 0, 100, 150)):
        assert store([good, pair(6, e0=bad)]) == E_ARG and "pair 1" in err() and "below -1" in err(), bad
    assert store([good, pair(6, e1=(1, 0, -1, 1, 30, 2 ** 28 + 1))]) == E_LIMIT and "pair 1" in err() and "end[1]" in err() and "coordinate" in err()
    assert store([pair(e0=(0, -1, 0, 0, -2 ** 28 - 1, -2 ** 28))]) == E_LIMIT and "pair 0" in err() and "end[0]" in err()
    assert store([pair(e0=(0, -1, 0, 0, 100, 100 + 2 ** 24))]) == E_LIMIT and "pair 0" in err() and "spans" in err()
    assert store([pair(e0=(0, -1, 0, 0, 100 + 2 ** 24 + 2, 100))]) == E_LIMIT and "spans" in err()
    assert store([pair(e0=(0, -1, 0, 0, 100, 99 + 2 ** 24))], ref=None) == E_ARG and "no reference" in err()     # the longest region that passes
    assert store([good], ref=None) == E_ARG and "no reference" in err()
    assert store([good], ex=None) == E_ARG and "no exons" in err()
    assert not h

    # ---- the rest
    assert lib.task_store_windows(None) is None and lib.task_store_pred_tasks(None) is None
    counts, timing = task.Counts(), task.TaskTiming()
    assert lib.task_store_counts(None, ctypes.byref(counts)) == E_ARG and lib.task_store_counts(one, None) == E_ARG
    assert lib.task_store_get_timing(None, ctypes.byref(timing)) == E_ARG and lib.task_store_get_timing(one, None) == E_ARG
    assert lib.task_store_fetch(None, None, 0, None, 0, None, 0, None, 0) == E_ARG and "no store" in err()
    assert lib.task_store_fetch(one, None, -1, None, 0, None, 0, None, 0) == E_ARG and "negative" in err()
    assert lib.task_store_fetch(one, None, 0, None, 0, None, 1, None, 0) == E_ARG and "without a buffer" in err()
    lib.task_store_destroy(None)
    lib.task_exons_destroy(None)
    lib.task_reference_destroy(None)
    # good arguments get as far as the device: no CPU path
    rc = reference([(0, 4), (4, 6)])
    assert rc in (0, E_DEVICE)
    if rc == 0:
        lib.task_reference_destroy(h)
    else:
        assert not h and "device" in err()


def test_the_cases_reach_their_edges(built, tmp_path):
    """The coverage of the GPU tests' cases, on the oracle alone."""
    seqs, table, cases = cut_edge_cases()
    cut_edge_coverage(World(seqs, table, tmp_path), cases)
    seqs, table, cases = exon_cases()
    exon_coverage(World(seqs, table, tmp_path), cases)


def test_host_checks_under_sanitizers(built, tmp_path):
    """task_check.hpp (everything task_api.hip does before a device call) in a host program under ASan and UBSan: the
    argument errors again, and the bins of a table against ExonRegions' own rule."""
    src = tmp_path / "check.cpp"
    src.write_text(r'''
#include <cassert>
#include <cstring>
#include <set>
#include "%s/defuse_amd/csrc/task_check.hpp"
using namespace taskhost;
int main()
{
    std::string err;
    // a table whose transcripts straddle bins, lie below zero and are inverted
    std::vector<int32_t> chrom_ref = {4, 9, 2};
    std::vector<task_exon> ex = {{99990, 100010}, {250000, 250100}, {-150000, -99999}, {5, 9}, {300000, 100}, {120000, 130000}, {7, 7}};
    std::vector<task_transcript> tx = {{0, 0, 0, 2, 1}, {1, 1, 2, 1, 2}, {1, 0, 3, 1, 3}, {0, 1, 4, 1, 5}, {0, 0, 5, 1, 6}, {0, 0, 6, 1, 7}};
    ExonIndex ix;
    assert(build_exons(chrom_ref.data(), 3, tx.data(), (int32_t)tx.size(), ex.data(), (int64_t)ex.size(), ix, err) == DSA_OK);
    assert(ix.chrom_bins[2] == 0 && ix.tx_len[0] == 21 + 101 && ix.tx_reg[0] == 99990 && ix.tx_reg[1] == 250100);
    for (int c = 0; c < 3; ++c)
        for (int b = -3; b <= 4; ++b) {
            std::set<int32_t> want, got;
            for (size_t t = 0; t < tx.size(); ++t)
                if (tx[t].chrom == c && ix.tx_reg[2 * t] / TASK_EXON_BIN <= b && b <= ix.tx_reg[2 * t + 1] / TASK_EXON_BIN) want.insert((int32_t)t);
            const int r = b - ix.chrom_bin_lo[c];
            if (r >= 0 && r < ix.chrom_bins[c]) {
                int32_t prev = -1;
                for (int32_t j = ix.row_first[ix.chrom_row[c] + r]; j < ix.row_first[ix.chrom_row[c] + r + 1]; ++j) {
                    assert(ix.row_tx[j] > prev);
                    prev = ix.row_tx[j];
                    got.insert(prev);
                }
            }
            assert(want == got);
        }
    assert(build_exons(nullptr, 0, nullptr, 0, nullptr, 0, ix, err) == DSA_OK && ix.row_first.size() == 1);
    tx[1].n_exons = 0;
    assert(build_exons(chrom_ref.data(), 3, tx.data(), (int32_t)tx.size(), ex.data(), (int64_t)ex.size(), ix, err) == DSA_E_ARG && err.find("transcript 1") != std::string::npos);
    // pairs
    std::vector<task_pair> p(3);
    for (int k = 0; k < 3; ++k) p[k] = task_pair{10 - k, {{0, -1, 0, 0, 5, 50}, {-1, 2, -1, 1, -7, 3}}};
    assert(check_pairs(p.data(), 3, err) == DSA_OK && check_pairs(nullptr, 0, err) == DSA_OK);
    assert(check_pair_indices(p.data(), 3, 1, 3, 1, err) == DSA_OK);
    assert(check_pair_indices(p.data(), 3, 1, 2, 1, err) == DSA_E_ARG && err.find("transcript 2") != std::string::npos);
    p[2].fusion_id = 10;
    assert(check_pairs(p.data(), 3, err) == DSA_E_ARG && err.find("pairs 0 and 2") != std::string::npos);
    p[2].fusion_id = INT32_MAX;
    p[1].end[1].end = INT32_MIN;
    assert(check_pairs(p.data(), 3, err) == DSA_E_LIMIT && err.find("pair 1") != std::string::npos);
    p[1].end[1].end = TASK_MAX_COORD;
    p[1].end[1].start = -TASK_MAX_COORD;
    assert(check_pairs(p.data(), 3, err) == DSA_E_LIMIT && err.find("spans") != std::string::npos);
    task_params prm = {70, 130, 20, 30};
    assert(check_params(&prm, err) == DSA_OK && check_params(nullptr, err) == DSA_E_ARG);
    prm.max_fragment = INT32_MAX;
    assert(check_params(&prm, err) == DSA_E_LIMIT);
    // reference
    const uint8_t bytes[8] = {0};
    task_seq seqs[2] = {{0, 8}, {8, 0}};
    assert(check_reference(bytes, 8, seqs, 2, err) == DSA_OK);
    seqs[1].off = INT64_MAX;
    seqs[1].len = INT64_MAX;
    assert(check_reference(bytes, 8, seqs, 2, err) == DSA_E_ARG && err.find("sequence 1") != std::string::npos);
    return 0;
}
''' % ROOT)
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, str(src)])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_cut_edges(task, tmp_path):
    seqs, table, cases = cut_edge_cases()
    W = World(seqs, table, tmp_path, task)
    cut_edge_coverage(W, cases)
    for params, regions in cases:
        run(task, W, params, regions)
    W.close()


@pytest.mark.gpu
def test_gather_word_edges(task, tmp_path):
    seqs, table, cases = word_edge_cases()
    W = World(seqs, table, tmp_path, task)
    for params, regions in cases:
        want, fetched = run(task, W, params, regions)
        word_edge_coverage(W, want, fetched)
    W.close()


@pytest.mark.gpu
def test_exon_logic(task, tmp_path):
    seqs, table, cases = exon_cases()
    W = World(seqs, table, tmp_path, task)
    exon_coverage(W, cases)
    for params, regions in cases:
        run(task, W, params, regions)
    W.close()


@pytest.mark.gpu
def test_status(task, tmp_path):
    """chrX: in the exon table, not in the FASTA; lonely: in the FASTA, not in the exon table; nope: in neither."""
    rng = random.Random(14)
    seqs = OrderedDict([("chrA", text(rng, 400)), ("lonely", text(rng, 300)), ("gA|tA", text(rng, 150))])
    table = {"tA": ("gA", "chrA", PLUS, [(10, 159)]), "tX": ("gX", "chrX", MINUS, [(50, 90)])}
    W = World(seqs, table, tmp_path, task)
    good = [loc("chrA", PLUS, 100, 150), loc("gA|tA", MINUS, 30, 80), loc("chrA", MINUS, 200, 260)]
    rows = [("chrX", 1), ("lonely", 2), ("nope", 3)]
    regions, expect = OrderedDict(), {}
    fid = 100
    for name, bits in rows:
        for strand in (PLUS, MINUS):
            bad = loc(name, strand, 120, 170)
            for pair, status in (([bad, good[0]], bits), ([good[1], bad], bits << 2), ([bad, loc(name, 1 - strand, 60, 90)], bits | (bits << 2))):
                regions[fid - 1], regions[fid], regions[fid + 1] = [good[2], good[0]], pair, [good[0], good[1]]
                expect[fid] = status
                fid += 10
    want, (rec, _, _, _) = run(task, W, (100, 10, 20, 30), regions)
    got = dict(zip(rec["fusion_id"].tolist(), rec["status"].tolist()))
    assert {f: got[f] for f in expect} == expect
    assert set(expect.values()) == {1, 2, 3, 4, 8, 12, 5, 10, 15}
    assert all(got[f] == 0 for f in got if f not in expect) and sum(isinstance(t, str) for t in want) == len(expect)
    W.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_against_the_oracle(task, tmp_path, seed):
    seqs, table, cases = random_case(seed)
    W = World(seqs, table, tmp_path, task)
    tally = dict(rem=[0, 0], clipped=0, empty=0, negative=0, regions=set())
    for params, regions in cases:
        want, _ = run(task, W, params, regions)
        for t in want:
            for e in (0, 1):
                tally["rem"][t.seq_strand[e]] += len(t.remainder[e]) > 0
                tally["clipped"] += t.seq_start[e] == 1
                tally["empty"] += t.seq_len[e] == 0
                tally["negative"] += t.seq_len[e] < 0
                tally["regions"].add(min(len(t.mate_regions[e]), 4))
    print(seed, tally)
    assert min(tally["rem"]) >= 40 and tally["clipped"] >= 50 and tally["empty"] >= 15 and tally["regions"] >= {1, 2, 3}
    W.close()


@pytest.mark.gpu
def test_the_stores_are_the_real_ones(task, tmp_path):
    """bat_assemble over the store's windows, pred_predict over its tasks and a cand table from its regions give what the same
    calls give over bat.Windows.from_dict, pred.Tasks.from_oracle and the oracle's regions."""
    from defuse_amd import bat, cand, dsa, pred
    from defuse_amd import eval as ev
    from tests.test_batch_assembly import assert_same_batch
    seqs, table, cases = random_case(4)
    W = World(seqs, table, tmp_path, task)
    params, regions = cases[0]
    want = W.want(params, regions)
    rng = random.Random(5)
    reads = {cand.read_id(k, k & 1): text(rng, rng.randint(20, 60), b"ACGTN") for k in range(len(want))}
    cands = np.zeros(len(want), dtype=cand.RECORD_DTYPE)
    order = sorted(range(len(want)), key=lambda k: want[k].fusion_id)
    rows, names, oregs = [], dict(W.names), []
    for n, k in enumerate(order):
        t = want[k]
        cands[n]["alignment"], cands[n]["fusion_id"], cands[n]["fragment"] = n, t.fusion_id, k
        cands[n]["cluster_end"], cands[n]["read_end"], cands[n]["revcomp"], cands[n]["first"] = k & 1, k & 1, 1 - (k & 1), 1
        if len(t.seq[1]) >= 2:
            rows.append((t.fusion_id, 0, 0, 0, min(3, len(t.seq[0])), min(5, len(t.seq[1]) - 2), 30, 46, 10, 0))
    for t in want:
        for e in (0, 1):
            oregs += [(names[m["refName"]], m["strand"], m["start"], m["end"], cand.cluster_id(t.fusion_id, e)) for m in t.mate_regions[e]]
    records = np.array(rows, dtype=dsa.RECORD_DTYPE).reshape(-1)
    als = cand.alignments([(r[0], r[1], r[2] + d, r[2] + d + 30, 7 * k + d, k & 1) for k, r in enumerate(oregs) for d in (0, 40)])
    windows = {t.fusion_id: (t.seq[0], t.seq[1]) for t in want}
    pairs = task.pairs_from_regions(regions, W.ref, W.exons)
    with task.Store(W.ref, W.exons, int_params(params), pairs) as st, bat.Reads.from_dict(reads) as r, bat.Windows.from_dict(windows) as w, \
            bat.Batch() as b, pred.Tasks.from_oracle(w, want) as ptasks, pred.Context() as P, ev.Context(0) as ectx:
        b.assemble(r, w, cands)
        theirs = b.fetch()
        b.assemble(r, st.windows, cands)
        assert_same_batch(b.fetch(), theirs)
        assert len(theirs[1]) == len(want) and len(theirs[3]) == len(want)
        groups, _ = ectx.evaluate(records)
        P.predict(groups, ptasks)
        res, seq = P.fetch()
        assert len(res) == len(rows) > 50 and (res["status"] == 0).all() and (res["seq_len"] > 0).all()
        P.predict(groups, st.tasks)
        res2, seq2 = P.fetch()
        assert res2.tobytes() == res.tobytes() and seq2.tobytes() == seq.tobytes()
        regs = st.fetch()[3]
        assert regs.tobytes() == cand.regions(oregs).tobytes()
        with cand.Table(regs) as mine, cand.Table(cand.regions(oregs)) as other, mine.session() as s1, other.session() as s2:
            c1, c2 = s1.enumerate(als, cand.ORDER_FUSION), s2.enumerate(als, cand.ORDER_FUSION)
            assert len(c1) >= len(oregs) and c1.tobytes() == c2.tobytes()
    W.close()


@pytest.mark.gpu
def test_smoke_vector_through_the_whole_chain_from_the_store(task, gpu_ctx):
    """tests/test_pred.py::test_smoke_vector_through_the_whole_resident_chain with the host's tasks, windows, prediction tasks
    and region list replaced by the store."""
    from defuse_amd import bat, cand, pred
    from defuse_amd import eval as ev
    from oracle import dosplitalign_oracle as ora
    from tests.test_batch_assembly import DeviceArray
    from tests.test_pred import check as check_pred, expected
    d = SMOKE + "/"
    regions = ora.read_align_region_pairs(d + "regions.txt")
    tasks = ora.create_tasks(d + "ref.fa", d + "exons.txt", 300, 30, 50, 50, regions)         # for the expected records only
    E = ora.ExonRegions(d + "exons.txt")
    table = {t: (E.transcript_gene[t], E.chromosome[t], E.strand[t], E.exons[t]) for t in E.exons}
    reads = {}
    ora.read_fastq(d + "reads.1.fastq", reads)
    ora.read_fastq(d + "reads.2.fastq", reads)
    names = {}
    with task.Reference(OrderedDict(ora.FastaIndex(d + "ref.fa").seqs)) as ref, task.Exons(table, names) as ex, \
            task.Store(ref, ex, int_params((300, 30, 50, 50)), task.pairs_from_regions(regions, ref, ex)) as st:
        rec, _, _, regs = st.fetch()
        assert (rec["status"] == 0).all()
        als = cand.alignments([(names.get(rname, -1), strand, start, end, ora.lexical_cast_int(frag), rend)
                               for frag, rend, rname, strand, start, end in ora.sam_alignments(d + "improper.sam")])
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
def test_window_beyond_the_dp_limit(task, gpu_ctx, tmp_path):
    """A region wholly in front of a sequence gets the whole sequence (the faidx quirk): beyond dsa_limits.max_ref_len that is
    DSA_E_LIMIT naming the first such pair, and one base shorter it is a task."""
    lim = gpu_ctx.limits().max_ref_len
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(15).integers(0, 4, size=2 * lim + 1)].tobytes()
    seqs = OrderedDict([("chrA", acgt[:lim]), ("chrB", acgt[lim:])])
    table = {"tA": ("g", "chrA", PLUS, [(10, 30)]), "tB": ("g", "chrB", MINUS, [(10, 30)])}
    W = World(seqs, table, tmp_path, task)
    params = (100, 10, 20, 30)
    front = lambda name: loc(name, PLUS, -400, -350)
    regions = OrderedDict([(7, [front("chrA"), loc("chrA", MINUS, 50, 90)]), (3, [loc("chrB", PLUS, 50, 90), front("chrA")])])
    want, _ = run(task, W, params, regions)
    assert [t.seq_len for t in want] == [[lim, want[0].seq_len[1]], [want[1].seq_len[0], lim]]
    regions[5] = [loc("chrA", PLUS, 10, 60), front("chrB")]
    regions[6] = [front("chrB"), front("chrB")]
    with pytest.raises(task.TaskError) as e:
        task.Store(W.ref, W.exons, int_params(params), task.pairs_from_regions(regions, W.ref, W.exons))
    assert e.value.code == E_LIMIT and "pair 2" in str(e.value) and str(lim) in str(e.value)
    W.close()


@pytest.mark.gpu
def test_reuse(task, tmp_path):
    """Two stores from one reference and one exon table at a time; store and bat_batch / pred_ctx destroyed in either order;
    no tasks at all; the capacity protocol of the fetch."""
    from defuse_amd import bat, cand, pred
    from defuse_amd import eval as ev
    seqs, table, cases = random_case(6)
    W = World(seqs, table, tmp_path, task)
    (p1, r1), (p2, r2) = cases[0], cases[2]
    s1 = task.Store(W.ref, W.exons, int_params(p1), task.pairs_from_regions(r1, W.ref, W.exons))
    s2 = task.Store(W.ref, W.exons, int_params(p2), task.pairs_from_regions(r2, W.ref, W.exons))
    check(W, r2, W.want(p2, r2), s2.fetch())
    check(W, r1, W.want(p1, r1), s1.fetch())
    # capacities: nothing is written, the counts say what is needed
    lib, c = s1._lib, s1.counts()
    rec = np.zeros(c.n_tasks, dtype=task.RECORD_DTYPE)
    buf = np.zeros(max(c.window_bytes, c.rem_bytes), dtype=np.uint8)
    reg = np.zeros(c.n_regions, dtype=cand.REGION_DTYPE)
    full = (c.n_tasks, c.window_bytes, c.rem_bytes, c.n_regions)
    for short in range(4):
        caps = [v - (k == short) for k, v in enumerate(full)]
        assert lib.task_store_fetch(s1.handle, rec.ctypes.data, caps[0], buf.ctypes.data, caps[1], buf.ctypes.data, caps[2], reg.ctypes.data, caps[3]) == E_CAPACITY
        assert str(full[short]) in lib.task_last_error().decode() and not rec.view(np.uint8).any() and not buf.any() and not reg.view(np.uint8).any()
    # a part without a buffer stays on the device
    assert lib.task_store_fetch(s1.handle, None, 0, None, 0, None, 0, reg.ctypes.data, len(reg)) == 0
    assert reg.tobytes() == s1.fetch()[3].tobytes() and not rec.view(np.uint8).any() and not buf.any()
    # the first store goes before the objects that used it, the second after them
    fid = next(iter(r1))
    cands = np.zeros(1, dtype=cand.RECORD_DTYPE)
    cands[0]["fusion_id"], cands[0]["first"] = fid, 1
    r = bat.Reads.from_dict({cand.read_id(0, 0): b"ACGTACGTAC"})
    b1, P1 = bat.Batch(), pred.Context()
    v = b1.assemble(r, s1.windows, cands)
    assert v.n_pairs == 1 and v.n_fusions == 1
    assert P1.predict(np.zeros(0, dtype=ev.GROUP_DTYPE), s1.tasks).n_results == 0
    s1.close()
    b1.close()
    P1.close()
    b2, P2 = bat.Batch(), pred.Context()
    cands[0]["fusion_id"] = next(iter(r2))
    assert b2.assemble(r, s2.windows, cands).n_pairs == 1
    b2.close()
    P2.close()
    s2.close()
    # no tasks
    with task.Store(W.ref, W.exons, int_params(p1), np.zeros(0, dtype=task.PAIR_DTYPE)) as s0:
        rec, win, rem, reg = s0.fetch()
        assert (len(rec), len(win), len(rem), len(reg)) == (0, 0, 0, 0) and s0.windows.handle and s0.tasks.handle
        with bat.Batch() as b0:
            assert b0.assemble(r, s0.windows, cands[:0]).n_pairs == 0
    r.close()
    W.close()
