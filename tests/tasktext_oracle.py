"""The rules of the "region and exon text" section of include/defuse_task.h, restated on bytes: what taskt_parse_exons and
taskt_parse_regions give for a text.  (oracle/dosplitalign_oracle.py decodes its text and differs at the five-field and
empty-strand edges; tests/test_task_text.py pins this file to the tools' own readers instead.)"""
MAX_NAME = 64
EXON_BAD_INTEGER, EXON_BAD_STRAND, REGION_BAD_INTEGER, REGION_BAD_END, REGION_BAD_STRAND = 1, 2, 3, 4, 5
EXON_LONG_NAME, EXON_DUPLICATE = 16, 17
SKIPPED = -1
MAX_COORD, MAX_REGION = 1 << 28, 1 << 24
E_ARG, E_LIMIT = -3, -4


def lexical_int(f):
    """boost::lexical_cast<int> of a field (bytes): the int, or None."""
    body = f[1:] if f[:1] in (b"+", b"-") else f
    if not body or any(c < 0x30 or c > 0x39 for c in body):
        return None
    v = int(body)
    if f[:1] == b"-":
        v = -v
    return v if -2 ** 31 <= v <= 2 ** 31 - 1 else None


def lines_of(text):
    """[(offset, line bytes without the newline)]: a last line without a newline is a line, empty text has none."""
    out, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end = len(text) if nl < 0 else nl
        out.append((at, text[at:end]))
        at = end + 1
    return out


def exon_line(line):
    """(kind, field, transcript line or None) without the duplicate rule; a transcript line is
    (gene, transcript, chromosome, strand, [(start, end)])."""
    f = line.split(b"\t")
    if not line or len(f) < 6:
        return SKIPPED, -1, None
    exons = []
    for k in range(5, len(f), 2):
        pair = []
        for j in (k - 1, k):
            v = lexical_int(f[j])
            if v is None:
                return EXON_BAD_INTEGER, j, None
            pair.append(v)
        exons.append(tuple(pair))
    if f[3] not in (b"+", b"-"):
        return EXON_BAD_STRAND, 3, None
    for k in (1, 2):
        if len(f[k]) > MAX_NAME:
            return EXON_LONG_NAME, k, None
    return 0, -1, (f[0], f[1], f[2], 0 if f[3] == b"+" else 1, exons)


def region_line(line):
    """(kind, field, (id, end, name, strand, start, stop) or None)."""
    f = line.split(b"\t")
    if not line or len(f) < 5:
        return SKIPPED, -1, None
    v = []
    for k in (0, 1):
        v.append(lexical_int(f[k]))
        if v[k] is None:
            return REGION_BAD_INTEGER, k, None
    if v[1] not in (0, 1):
        return REGION_BAD_END, 1, None
    if f[3] not in (b"+", b"-"):
        return REGION_BAD_STRAND, 3, None
    if len(f) == 5:
        return REGION_BAD_INTEGER, 5, None
    for k in (4, 5):
        v.append(lexical_int(f[k]))
        if v[-1] is None:
            return REGION_BAD_INTEGER, k, None
    return 0, -1, (v[0], v[1], f[2], 0 if f[3] == b"+" else 1, v[2], v[3])


def result(n_lines=0, n_skipped=0, n_items=0, n_exons=0, n_chroms=0, name_bytes=0, stop=None):
    r = dict(n_lines=n_lines, n_skipped=n_skipped, n_items=n_items, n_exons=n_exons, n_chroms=n_chroms, name_bytes=name_bytes, stop_line=0, stop_off=0,
             stop_len=0, stop_kind=0, stop_field=-1)
    if stop is not None:
        k, (off, line), kind, field = stop
        r.update(n_lines=k, stop_line=k + 1, stop_off=off, stop_len=len(line), stop_kind=kind, stop_field=field)
    return r


class ExonTable:
    """The parsed table: .transcripts [(chrom, strand, first_exon, n_exons, name_ref)] in ascending name order, .names their
    names, .exons [(start, end)] in file order, .chrom_ref, .chroms the chromosome names by first appearance, and the
    {transcript: (gene, chromosome, strand, exons)} table task.Exons takes."""

    def __init__(self, rows, ref_names):
        ref = {n: k for k, n in enumerate(ref_names)}
        self.chroms, self.exons = [], []
        first = {}
        for gene, t, chrom, strand, exons in rows:
            if chrom not in self.chroms:
                self.chroms.append(chrom)
            first[t] = len(self.exons)
            self.exons += exons
        self.cindex = {c: k for k, c in enumerate(self.chroms)}
        self.chrom_ref = [ref.get(c, len(ref) + k) for k, c in enumerate(self.chroms)]
        self.names = sorted(r[1] for r in rows)                 # bytes sort as unsigned bytes, a prefix first
        self.tindex = {t: k for k, t in enumerate(self.names)}
        by_name = {r[1]: r for r in rows}
        self.transcripts = []
        for k, t in enumerate(self.names):
            gene, _, chrom, strand, exons = by_name[t]
            self.transcripts.append((self.cindex[chrom], strand, first[t], len(exons), ref.get(gene + b"|" + t, len(ref) + len(self.chroms) + k)))
        self.table = {r[1]: (r[0], r[2], r[3], r[4]) for r in rows}


def parse_exons(text, ref_names):
    """(taskt_result as a dict, ExonTable or None after a stop)."""
    rows, seen, skipped = [], set(), 0
    lines = lines_of(text)
    for k, (off, line) in enumerate(lines):
        kind, field, row = exon_line(line)
        if kind == 0 and row[1] in seen:
            kind, field = EXON_DUPLICATE, 1
        if kind > 0:
            return result(stop=(k, (off, line), kind, field)), None
        if kind == SKIPPED:
            skipped += 1
        else:
            seen.add(row[1])
            rows.append(row)
    T = ExonTable(rows, ref_names)
    return result(len(lines), skipped, len(rows), len(T.exons), len(T.chroms), sum(len(t) for t in T.names)), T


def resolve(name, seq_index, T):
    """(seq, transcript, chrom) of a region's name (defuse_amd/task.py:pairs_from_regions, on bytes)."""
    parts = name.split(b"|")
    return seq_index.get(name, -1), (T.tindex.get(parts[1], -1) if len(parts) >= 2 else -1), T.cindex.get(name, -1)


def read_regions(text):
    """ReadAlignRegionPairs on bytes: (stop or None, {id: {end: (name, strand, start, stop, 1-based line)}}, skipped lines,
    lines); a stop is the argument of result()."""
    ends, skipped = {}, 0
    lines = lines_of(text)
    for k, (off, line) in enumerate(lines):
        kind, field, row = region_line(line)
        if kind > 0:
            return (k, (off, line), kind, field), None, 0, k
        if kind == SKIPPED:
            skipped += 1
            continue
        fid, end, name, strand, start, stop = row
        ends.setdefault(fid, {})[end] = (name, strand, start, stop, k + 1)
    return None, ends, skipped, len(lines)


def parse_regions(text, seq_names, T):
    """(taskt_result as a dict, pairs or None after a stop, lines); a pair is (id, end0, end1), an end
    (seq, transcript, chrom, strand, start, end); lines[k] = the two 1-based lines that gave pair k its ends, 0: default."""
    seq_index = {n: k for k, n in enumerate(seq_names)}
    stop, ends, skipped, n_lines = read_regions(text)
    if stop is not None:
        return result(stop=stop), None, None
    default = resolve(b"", seq_index, T) + (0, 0, 0)
    pairs, plines = [], []
    for fid in sorted(ends):
        got = ends[fid]
        pairs.append((fid,) + tuple(resolve(got[e][0], seq_index, T) + got[e][1:4] if e in got else default for e in (0, 1)))
        plines.append([got[e][4] if e in got else 0 for e in (0, 1)])
    return result(n_lines, skipped, len(pairs)), pairs, plines


def check_pairs(pairs):
    """None, or (code, pair index, end or None) of the first pair taskt_store_create refuses."""
    for k, (fid, e0, e1) in enumerate(pairs):
        if fid < 0:
            return E_ARG, k, None
        for e, (_, _, _, _, start, end) in enumerate((e0, e1)):
            if abs(start) > MAX_COORD or abs(end) > MAX_COORD or abs(end - start + 1) > MAX_REGION:
                return E_LIMIT, k, e
    return None
