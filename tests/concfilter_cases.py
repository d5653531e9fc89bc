"""The synthetic inputs of the concordant-cluster filter's tests (tests/test_conc_filter.py) and fixtures
(tests/golden/make_conc.py): every case is dict(fa, gtf, clusters), the bytes of the three files."""
import random

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _fasta(seqs, width=60):
    out = []
    for name, s in seqs.items():
        out.append(b">" + name.encode() + b"\n" + b"".join(s[k:k + width] + b"\n" for k in range(0, len(s), width)))
    return b"".join(out)


def _gtf(rows):
    """rows: (chromosome, type, start, end, strand, gene, transcript)."""
    return "".join('%s\tsrc\t%s\t%d\t%d\t.\t%s\t.\tgene_id "%s"; transcript_id "%s"; gene_name "%s";\n' % (c, t, s, e, st, g, tx, "N" + g)
                   for c, t, s, e, st, g, tx in rows).encode()


def _spliced(contig, exons, strand):
    s = b"".join(contig[a - 1:b] for a, b in sorted(exons))
    return s[::-1].translate(_COMP) if strand == "-" else s


def cl(cid, ce, frag, name, strand, start, end, read_end=0):
    return "%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (cid, ce, frag, read_end, name, strand, start, end)


EDGE_MODEL = [  # gene, chromosome, strand, {transcript: (exons, cds or None, in the FASTA)}
    ("G1", "chr1", "+", {"T1": ([(21, 60), (101, 140), (201, 240)], [(41, 60), (101, 140), (201, 220)], True),
                         "T2": ([(21, 60), (201, 240)], None, True),
                         "T3": ([(150, 160)], None, True),
                         "T4": ([(30, 50)], None, False)}),
    ("G2", "chr1", "-", {"T1": ([(130, 170), (260, 300)], [(140, 170), (260, 280)], True),
                         "T2": ([(200, 220)], None, True)}),
    ("G3", "chr1", "+", {"T1": ([(320, 380)], [(340, 360)], True)}),          # one exon around the CDS: no right-hand UTR piece
    ("G4", "chr2", "+", {"T1": ([(80, 120)], [(90, 110)], True)}),            # inside the intron of G5
    ("G5", "chr2", "-", {"T1": ([(10, 40), (150, 180)], [(20, 40), (150, 170)], True)}),
    ("G6", "chr3", "+", {"T1": ([(10, 50)], [(10, 50)], True)}),              # chr3 is not in the FASTA
    ("G7", "chr3", "-", {"T1": ([(60, 90)], None, True)}),                    # an end on it has no target at all
]


def _model_files(rng, contigs, model, extra_seqs=()):
    seqs, rows = dict(contigs), []
    for gene, chrom, strand, txs in model:
        for tx, (exons, cds, in_fasta) in txs.items():
            rows += [(chrom, "exon", a, b, strand, gene, tx) for a, b in exons]
            rows += [(chrom, "CDS", a, b, strand, gene, tx) for a, b in (cds or [])]
            if in_fasta:
                seqs[gene + "|" + tx] = _spliced(contigs[chrom], exons, strand) if chrom in contigs else _bases(rng, sum(b - a + 1 for a, b in exons))
    rng.shuffle(rows)                                            # exon lines come unsorted
    rows.insert(0, ("chr1", "gene", 1, 400, "+", "Gx", "Tx"))    # a type the reader skips
    for name, s in extra_seqs:
        seqs[name] = s
    return _fasta(seqs), _gtf(rows)


def edges_case():
    """Every branch the issue lists, by hand (R = 40 in mind; see the comments)."""
    rng = random.Random(7)
    contigs = {"chr1": _bases(rng, 400), "chr2": _bases(rng, 300), "chrM": _bases(rng, 90)}
    fa, gtf = _model_files(rng, contigs, EDGE_MODEL)
    c = [
        # 1: both ends in G1 and G2 (two overlapping genes share end 0); the genomic window of end 0 reaches end 1: dropped.
        #    midpoint 115.5 (odd sum on a chromosome): T2 is in an intron there, T3 lies behind it, T4 is not in the FASTA;
        #    end 1 at 150: G2|T2 (minus strand) lies behind it.  An earlier line of end 0 names another strand and sequence
        cl(1, 0, 5, "chr2", "-", 110, 120), cl(1, 1, 5, "chr1", "-", 125, 150), cl(1, 0, 6, "chr1", "+", 101, 130), cl(1, 1, 6, "chr1", "-", 120, 149),
        # 2: window clipped at the contig start, on a minus end with an odd sum
        cl(2, 0, 1, "chr1", "-", 5, 20), cl(2, 1, 1, "chr2", "+", 200, 230),
        # 3: window clipped at the contig end; the other end on a contig the models do not know
        cl(3, 0, 1, "chr1", "+", 385, 399), cl(3, 1, 1, "chrM", "-", 10, 30),
        # 4: windows wholly past either end of a contig: one base each
        cl(4, 0, 1, "chr2", "+", 310, 330), cl(4, 1, 1, "chr1", "-", -30, -10),
        # 5: an extent with start > end: the reversed subseq
        cl(5, 0, 1, "chr2", "-", 60, 90), cl(5, 1, 1, "chr2", "+", 120, 100),
        # 6: transcript ends with odd sums on either strand; G5|T1 [20, 51] spans the intron G4 lies in: G4 does not count
        cl(6, 0, 1, "G1|T1", "+", 10, 25), cl(6, 1, 1, "G5|T1", "-", 20, 51),
        # 7: midpoint 230.5 in the 3' UTR of G1|T1: past the last exon of T3
        cl(7, 0, 1, "chr1", "+", 225, 236), cl(7, 1, 1, "chr2", "-", 30, 60),
        # 8: G3: 370.5 lies in the piece the elsif never makes (no transcript target), 327.5 in the 5' UTR
        cl(8, 0, 1, "chr1", "+", 365, 376), cl(8, 1, 1, "chr1", "-", 322, 333),
        # 9: ends in neighbouring exons of G1|T1, 45 bases of intron apart: only the transcript windows reach: dropped
        cl(9, 0, 1, "chr1", "+", 45, 60), cl(9, 0, 2, "chr1", "+", 47, 58), cl(9, 1, 1, "chr1", "-", 105, 135),
        # 10: nothing reaches: kept
        cl(10, 0, 1, "chr1", "+", 250, 270), cl(10, 1, 1, "chr2", "-", 250, 280), cl(10, 1, 2, "chr2", "-", 255, 285),
        # 11: a transcript end whose chromosome the FASTA lacks (the genomic target is skipped), transcript ends past both ends
        cl(11, 0, 1, "G6|T1", "+", 30, 41), cl(11, 1, 1, "G5|T1", "+", 60, 75),
        cl(12, 0, 1, "G5|T1", "-", -9, 0), cl(12, 1, 1, "G1|T1", "-", 118, 131),
        # 13: midpoint 0 on a plus end and on a minus end: `start ||= 1`, `stop ||= length`
        cl(13, 0, 1, "chrM", "+", -5, 5), cl(13, 1, 1, "chrM", "-", -7, 7),
    ]
    return dict(fa=fa, gtf=gtf, clusters="".join(c).encode())


def one_end_case():
    d = edges_case()
    d["clusters"] = (cl(1, 0, 1, "chr1", "+", 101, 130) + cl(1, 1, 1, "chr1", "-", 120, 149) + cl(2, 0, 1, "chr1", "+", 45, 60)).encode()
    return d


def missing_other_case():
    d = edges_case()
    d["clusters"] = (cl(1, 0, 1, "chr1", "+", 101, 130) + cl(1, 1, 1, "chr1", "-", 120, 149) + cl(2, 0, 1, "chr1", "+", 45, 60) +
                     cl(2, 1, 1, "chrQ", "-", 10, 40)).encode()
    return d


def random_case(seed, n_clusters=50, n_contigs=5, n_genes=20, contig_len=(1500, 3000), zero_ok=True):
    """About n_clusters clusters over n_contigs contigs and n_genes genes: concordant pairs a few bases or an intron apart,
    ends on transcripts, ends at and past contig ends, lines of one end that disagree.  zero_ok false: a coordinate 0 becomes 1 (an extent that ends at 0 is
    the whole sequence to subseq: `stop ||= length`)."""
    rng = random.Random(seed)
    contigs = {"c%d" % k: _bases(rng, rng.randrange(*contig_len)) for k in range(n_contigs)}
    model = []
    for g in range(n_genes):
        chrom = rng.choice(sorted(contigs))
        strand = rng.choice("+-")
        a = rng.randrange(50, len(contigs[chrom]) - 700)
        txs = {}
        for t in range(rng.randrange(1, 4)):
            exons, p = [], a + rng.randrange(0, 40)
            for _ in range(rng.randrange(1, 5)):
                e = p + rng.randrange(20, 90)
                exons.append((p, e))
                p = e + rng.randrange(30, 120)
            cds = None
            if rng.random() < 0.7:
                lo, hi = exons[0][0] + rng.randrange(0, 15), exons[-1][1] - rng.randrange(0, 15)
                cds = [(max(s, lo), min(e, hi)) for s, e in exons if max(s, lo) <= min(e, hi)] or None
            txs["T%d" % t] = (exons, cds, rng.random() < 0.85)
        model.append(("G%02d" % g, chrom, strand, txs))
    fa, gtf = _model_files(rng, contigs, model, extra_seqs=[("lone", _bases(rng, 200))])
    present = [(g, t, sum(e - s + 1 for s, e in ex)) for g, _c, _s, txs in model for t, (ex, _cds, inf) in txs.items() if inf]
    lines = []
    for cid in rng.sample(range(1, 10 * n_clusters), n_clusters):
        kind = rng.random()
        if kind < 0.5:                                           # a pair on one contig, often inside a gene
            gene = rng.choice(model)
            chrom = gene[1]
            ex = rng.choice(list(gene[3].values()))[0]
            a = rng.choice(ex)[0] + rng.randrange(-20, 30)
            b = a + rng.choice([rng.randrange(0, 40), rng.randrange(20, 160)])
            ends = [(chrom, "+", a, a + rng.randrange(18, 60)), (chrom, "-", b, b + rng.randrange(18, 60))]
        elif kind < 0.75:                                        # transcript ends
            ends = []
            for _ in range(2):
                g, t, n = rng.choice(present)
                a = rng.randrange(-10, n)
                ends.append(("%s|%s" % (g, t), rng.choice("+-"), a, a + rng.randrange(18, 70)))
        else:                                                    # anywhere, contig ends included
            ends = []
            for _ in range(2):
                chrom = rng.choice(sorted(contigs) + ["lone"])
                n = len(contigs.get(chrom, b"x" * 200))
                a = rng.choice([rng.randrange(1, n), rng.randrange(-30, 30), n - rng.randrange(0, 60)])
                ends.append((chrom, rng.choice("+-"), a, a + rng.randrange(18, 64)))
        rng.shuffle(ends)
        for frag in range(rng.randrange(1, 4)):
            for ce, (name, strand, s, e) in enumerate(ends):
                lines.append((rng.random(), cl(cid, ce, frag, name, strand, (s + rng.randrange(-3, 4)) or int(not zero_ok), (e + rng.randrange(-3, 4)) or int(not zero_ok), ce)))
    if seed % 2:                                                 # now and then the lines of the clusters are interleaved
        lines.sort()
    return dict(fa=fa, gtf=gtf, clusters="".join(l for _k, l in lines).encode())


def r2000_case():
    """Six clusters for the pipeline's R = 2000: other ends of 18, 64, 65 and 300 bases, one of 1900 (the int32 kernel takes a
    pair with more than 1863 rows at -m 10 -g -5) and one that nothing reaches; a gene with two transcripts under the first ends."""
    rng = random.Random(2000)
    contigs = {"chrA": _bases(rng, 9000), "chrB": _bases(rng, 2500)}
    model = [("GA", "chrA", "+", {"T1": ([(900, 1250), (1500, 1700)], [(950, 1250), (1500, 1650)], True), "T2": ([(1000, 1100)], None, True)})]
    fa, gtf = _model_files(rng, contigs, model)
    c = []
    for k, n in enumerate((18, 64, 65, 300, 1900)):
        a = 1000 + 40 * k
        c += [cl(k + 1, 0, 1, "chrA", "+", a, a + 30), cl(k + 1, 1, 1, "chrA", "-", a + 90, a + 90 + n - 1)]
    c += [cl(9, 0, 1, "chrA", "+", 6000, 6040), cl(9, 1, 1, "chrB", "-", 100, 160)]
    return dict(fa=fa, gtf=gtf, clusters="".join(c).encode())


def with_clusters(case, lines):
    return dict(case, clusters="".join(lines).encode())
