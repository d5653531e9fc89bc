"""What prep_local_alignment_seqs.pl, localalign and `filter_column.pl VALUES 0 1` compute, restated on the host as the
scripts are written (scripts/prep_local_alignment_seqs.pl, scripts/gene_models.pm:248-587, Bio::DB::Fasta::subseq and
caloffset) — TEST INFRASTRUCTURE ONLY.  Positions are Fractions, so a midpoint that ends in .5 is exact.

Perl's order of clusters, genes and transcripts is hash order; `targets` returns the canonical order of include/defuse_task.h, section "concordant clusters":
cluster id ascending, end 0 then 1, the genomic target, then genes by id bytes, then transcripts by name bytes."""
import os
import re
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

ONE_END, NO_OTHER_SEQ = "one_end", "no_other_seq"
_RANGE_NAME = re.compile(r"^(.+):([\d_]+)(?:,|-|\.\.)([\d_]+)$", re.S)


class Stop(Exception):
    """Where Perl dies: .kind, .cluster_id."""

    def __init__(self, kind, cluster_id):
        super().__init__("%s at cluster %s" % (kind, cluster_id))
        self.kind, self.cluster_id = kind, cluster_id


def read_clusters(text):
    """prep_local_alignment_seqs.pl:158-188: {id: {end: dict(ref_name, strand, start, end)}}, keys as the file writes them."""
    clusters = {}
    for line in text.decode("latin-1").split("\n")[:-1] if text.endswith(b"\n") else text.decode("latin-1").split("\n"):
        f = line.split("\t")
        c = clusters.setdefault(f[0], {}).setdefault(f[1], {})
        c["ref_name"], c["strand"] = f[4], f[5]
        c["start"] = min(int(f[6]), c.get("start", int(f[6])))
        c["end"] = max(int(f[7]), c.get("end", int(f[7])))
    return clusters


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def subseq_bounds(start, stop, length):
    """Fasta.pm:903-967 on one sequence of `length` bytes: (first byte, last byte, reversed), 0-based and inclusive."""
    start = start or 1
    stop = stop or length
    reversed_ = start > stop
    if reversed_:
        start, stop = stop, start

    def caloffset(a):
        a -= 1
        if a < 0:
            a = 0
        if a >= length:
            a = length - 1
        return int(a)                                           # int($a / n) and $a % n both drop the fraction of a >= 0
    return caloffset(start), caloffset(stop), reversed_


def subseq(fasta, name, start, stop):
    """The bytes, or None for a name the FASTA lacks."""
    assert not _RANGE_NAME.match(name), name
    if name not in fasta:
        return None
    a, b, reversed_ = subseq_bounds(start, stop, len(fasta[name]))
    data = fasta[name][a:b + 1]
    return data[::-1].translate(bytes.maketrans(b"gatcGATC", b"ctagCTAG")) if reversed_ else data


def regions_length(exons):
    return sum(e - s + 1 for s, e in exons)


def genomic_position(models, name, position):
    if name not in models.transcripts:
        return position
    tr = models.transcripts[name]
    exons = tr["exons"]
    if tr["strand"] == "-":
        position = regions_length(exons) - position + 1
    if position < 1:
        return exons[0][0] + position - 1
    offset = 0
    for s, e in exons:
        size = e - s + 1
        if position <= offset + size:
            return position - offset - 1 + s
        offset += size
    return position - offset + exons[-1][1]


def genomic_regions(models, name, region):
    if name not in models.transcripts:
        return [region]
    tr = models.transcripts[name]
    exons = tr["exons"]
    length = regions_length(exons)
    if tr["strand"] == "-":
        region = (length - region[1] + 1, length - region[0] + 1)
    if region[0] < 1:
        region = (1, region[1])
    if region[1] > length:
        region = (region[0], length)
    out, offset = [], 0
    for s, e in exons:
        size = e - s + 1
        a = max(1, region[0] - offset) + s - 1
        b = min(size, region[1] - offset) + s - 1
        if a <= b:
            out.append((a, b))
        offset += size
    return out


def transcript_position(models, name, position):
    tr = models.transcripts[name]
    exons = tr["exons"]
    offset, found = 0, None
    for s, e in exons:
        if position <= e:
            found = offset + 1 if position < s else offset + position - s + 1
            break
        offset += e - s + 1
    if found is None:
        found = regions_length(exons)
    if tr["strand"] == "-":
        found = regions_length(exons) - found + 1
    return found


def overlapping_genes(models, name, region, spacing=10000):
    """calc_overlapping_genes with its bins: the genes of the bins the region touches whose region overlaps it."""
    if name not in models.chromosomes and name not in models.transcripts:
        return []
    chromosome = models.transcripts[name]["chromosome"] if name in models.transcripts else name
    found = set()
    for r in genomic_regions(models, name, region):
        bins = set(range(int(r[0] / spacing), int(r[1] / spacing) + 1))
        for g in models.chromosomes.get(chromosome, {}):
            gr = models.genes[g]["region"]
            if bins & set(range(int(gr[0] / spacing), int(gr[1] / spacing) + 1)) and not (r[1] < gr[0] or r[0] > gr[1]):
                found.add(g)
    return sorted(found)


def expressed(models, gene, position):
    """calc_gene_location is coding, utr5p or utr3p."""
    g = models.genes[gene]
    if position < g["region"][0] or position > g["region"][1]:
        return False
    for t in g["transcripts"]:
        tr = models.transcripts[t]
        if any(s <= position <= e for s, e in (tr["cds"] or []) + tr["utr5p"] + tr["utr3p"]):
            return True
    return False


def targets(models, fasta, clusters_text, seq_range):
    """The lines of clusters.sc.local.seq in canonical order, as dicts: cluster_id, cluster_end, kind (0 genomic, 1 transcript),
    name, sequence, other (the bytes of fields 1 and 2), and where they come from (seq_name, start, len, revcomp, other_*)."""
    clusters = read_clusters(clusters_text)
    out = []
    for cid in sorted(clusters, key=int):
        for end, other_end in (("0", "1"), ("1", "0")):
            if other_end not in clusters[cid] or end not in clusters[cid]:
                raise Stop(ONE_END, cid)
            me, other = clusters[cid][end], clusters[cid][other_end]
            other_seq = subseq(fasta, other["ref_name"], other["start"], other["end"])
            name, strand = me["ref_name"], me["strand"]
            midpoint = Fraction(me["start"] + me["end"], 2)
            is_tx = name in models.transcripts
            chromosome = models.transcripts[name]["chromosome"] if is_tx else name
            genomic_mid = genomic_position(models, name, midpoint)
            genomic_strand = strand if not is_tx else "+" if models.transcripts[name]["strand"] == strand else "-"
            mine = [(0, chromosome, genomic_mid, genomic_strand)]
            for g in overlapping_genes(models, name, (me["start"], me["end"])):
                if expressed(models, g, genomic_mid):
                    for t in sorted(models.genes[g]["transcripts"]):
                        mine.append((1, t, transcript_position(models, t, genomic_mid), "+" if models.transcripts[t]["strand"] == genomic_strand else "-"))
            for kind, tname, mid, tstrand in mine:
                start, stop = (mid, mid + seq_range) if tstrand == "+" else (mid - seq_range, mid)
                sequence = subseq(fasta, tname, start, stop)
                if sequence is None:
                    continue
                if other_seq is None:
                    raise Stop(NO_OTHER_SEQ, cid)               # (Perl dies on the undefined value at its first print)
                a, b, rev = subseq_bounds(start, stop, len(fasta[tname]))
                oa, ob, orev = subseq_bounds(other["start"], other["end"], len(fasta[other["ref_name"]]))
                flip = tstrand == other["strand"]
                out.append(dict(cluster_id=int(cid), cluster_end=int(end), kind=kind, name=tname, sequence=revcomp(sequence) if flip else sequence,
                                other=other_seq, seq_name=tname, start=a, len=b - a + 1, revcomp=int(rev != flip), other_name=other["ref_name"],
                                other_start=oa, other_len=ob - oa + 1, other_rev=int(orev)))
            if other_seq is None and any(fasta.get(t[1]) is not None for t in mine):
                raise Stop(NO_OTHER_SEQ, cid)
    return out


def target_lines(tg):
    return [b"%d\t%s\t%s\n" % (t["cluster_id"], t["sequence"], t["other"]) for t in tg]


def local_align(tg, match, mismatch, gap, threshold):
    """(text, scores, kept): oracle/localalign_oracle.py over the target lines; every target's score, and which printed."""
    import localalign_oracle
    text, scores, kept = [], [], []
    for t in tg:
        score = localalign_oracle.simple_align(match, mismatch, gap, t["sequence"], t["other"])
        out, _err, status = localalign_oracle.run([target_lines([t])[0].decode("latin-1")], match, mismatch, gap, threshold)
        assert status == 0
        scores.append(score)
        kept.append(out != "")
        text.append(out)
    return "".join(text).encode(), scores, kept


def filter_clusters(clusters_text, align_text):
    """filter_column.pl ALIGN 0 1 over the cluster text: string keys, as Perl's."""
    hit = {line.split(b"\t")[0] for line in align_text.split(b"\n")[:-1]}
    lines = clusters_text.split(b"\n")
    if clusters_text.endswith(b"\n"):
        lines.pop()
    return b"".join(l + b"\n" for l in lines if l.split(b"\t")[0] not in hit)


def run(models, fasta, clusters_text, seq_range, match=10, mismatch=-5, gap=-5, threshold=0.8):
    """dict(targets, align_text, scores, kept, filtered) of the whole step."""
    tg = targets(models, fasta, clusters_text, seq_range)
    text, scores, kept = local_align(tg, match, mismatch, gap, threshold)
    return dict(targets=tg, align_text=text, scores=scores, kept=kept, filtered=filter_clusters(clusters_text, text))
