"""CPU restatement of the reference `estislands` tool (tools/estislands.cpp, tools/EstCatalog.cpp) — TEST INFRASTRUCTURE ONLY,
and generators of its inputs.

Parity unpinned: the reference holds no test or golden vector for estislands, and it cannot be compiled here (Boost).  The
restatement, line by line:

  * Lines as std::getline returns them (split on '\\n', a last line without one included, '\\r' kept).  Empty lines and lines
    whose first byte is not 0-9 are skipped; so are lines with fewer than 18 fields when split on every tab.
  * EST rows (ReadEsts, :20-63): chromosome = field 14, start = int(field 16) + 1, end = int(field 17).  Break rows
    (FilterContainedInEstIslands, :103-173): chromosome = field 13, start = int(field 15) + 1, end = int(field 16).  A leading
    `chr` is removed, then `M` becomes `MT`.  Integers as boost::lexical_cast<int> (start first, then end).
  * Islands (SortAndMergeSegments, :72-101): per chromosome, sorted by start — STABLY, the canonical order of the drop-in
    (chromosome, start, file order) where the reference's std::sort leaves ties to chance — then the sequential merge.
  * Lookup: lower_bound by start, one step back unless first, walk while island.start <= q.end, contained if some visited
    island has start - 300 <= q.start and end + 300 >= q.end.
  * Output: every contained break line, as read, with '\\n', in input order.  A bad integer: in the EST file `Error: ...`,
    exit 1, no output file; in the breaks file the contained lines before it, then `Error: ...`, exit 1 (the drop-in's rule
    where the reference dies of an uncaught bad_lexical_cast).
"""
import bisect

import numpy as np

PAD = 300
EST_FIELDS = (14, 16, 17)
BREAK_FIELDS = (13, 15, 16)


def lexical_int(s):
    """boost::lexical_cast<int> of a byte string; None where it throws."""
    body = s[1:] if s[:1] in (b"+", b"-") else s
    if not body or not body.isdigit() or not body.isascii():
        return None
    v = int(s)
    return v if -2 ** 31 <= v < 2 ** 31 else None


def i32(v):
    """C++ int arithmetic (wraps modulo 2^32)."""
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def lines(data):
    """std::getline over the bytes of a file."""
    parts = data.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return parts


def chrom_key(name):
    if name[:3] == b"chr":
        name = name[3:]
    return b"MT" if name == b"M" else name


class BadInteger(Exception):
    def __init__(self, field, line_no):
        super().__init__(field)
        self.field, self.line_no = field, line_no


def rows(data, fields):
    """(line number, line, chromosome key, start, end) of every used row; raises BadInteger at the first bad one."""
    fc, fs, fe = fields
    for no, line in enumerate(lines(data), 1):
        if not line or not (48 <= line[0] <= 57):
            continue
        f = line.split(b"\t")
        if len(f) < 18:
            continue
        s = lexical_int(f[fs])
        if s is None:
            raise BadInteger(f[fs], no)
        e = lexical_int(f[fe])
        if e is None:
            raise BadInteger(f[fe], no)
        yield no, line, chrom_key(f[fc]), i32(s + 1), e


def merge(segments):
    """SortAndMergeSegments on a list of (start, end) in file order: the islands, a list of (start, end)."""
    if not segments:
        return []
    segs = sorted(segments, key=lambda x: x[0])          # stable: ties keep file order
    merged = []
    cs, ce = segs[0]
    for s, e in segs:
        if s > ce:
            merged.append((cs, ce))
            cs, ce = s, e
        else:
            ce = max(ce, e)
    merged.append((cs, ce))
    return merged


def catalog(segments_by_chrom):
    """{chromosome: [(start, end), ...] in file order} -> {chromosome: (island starts, island ends)}."""
    out = {}
    for c, segs in segments_by_chrom.items():
        isl = merge(segs)
        out[c] = ([s for s, _ in isl], [e for _, e in isl])
    return out


def contained(islands, s, e):
    """The reference's lookup (:141-167) on (starts, ends) of one chromosome."""
    starts, ends = islands
    k = bisect.bisect_left(starts, s)
    if k != 0:
        k -= 1
    hit = False
    while k < len(starts) and starts[k] <= e:
        if starts[k] - PAD <= s and ends[k] + PAD >= e:
            hit = True
        k += 1
    return hit


def read_ests(data):
    """{chromosome: [(start, end), ...]} in file order and in order of first appearance."""
    segs = {}
    for _, _, c, s, e in rows(data, EST_FIELDS):
        segs.setdefault(c, []).append((s, e))
    return segs


def run(est_data, break_data):
    """(output bytes or None when no output file is created, stderr text, exit status) of the tool on the two inputs'
    bytes (None: cannot be opened).  Names in messages are 'EST' / 'BREAKS' / 'OUT'."""
    if est_data is None:
        return None, "Error: Unable to open est file EST\n", 1
    try:
        cat = catalog(read_ests(est_data))
    except BadInteger as x:
        return None, "Error: bad integer '%s' in est file EST line %d\n" % (x.field.decode("latin-1"), x.line_no), 1
    if break_data is None:
        return None, "Error: Unable to open break alignments file BREAKS\n", 1
    out = []
    try:
        for _, line, c, s, e in rows(break_data, BREAK_FIELDS):
            if c in cat and contained(cat[c], s, e):
                out.append(line + b"\n")
    except BadInteger as x:
        return b"".join(out), "Error: bad integer '%s' in break alignments file BREAKS line %d\n" % (x.field.decode("latin-1"), x.line_no), 1
    return b"".join(out), "", 0


# ---------------------------------------------------------------------------------------------- generators
CHROMS = [b"chr1", b"chr2", b"chr3", b"chrX", b"chrY", b"chrM", b"chr7_random", b"chrUn_gl000220", b"chr6_cox_hap2", b"4", b"M", b"MT",
          b"chr17"]


def segment_columns(rng, n, n_chroms=len(CHROMS), span=2_000_000, degenerate=0.0):
    """n EST segments: (chromosome index, tStart, tEnd) as int arrays, clustered so that islands touch, nest and chain."""
    c = rng.integers(0, n_chroms, size=n)
    centre = rng.integers(0, span, size=n)
    # cluster centres on a coarse grid so that many segments pile up
    centre = (centre // 20000) * 20000 + rng.integers(-800, 800, size=n)
    length = rng.choice(np.array([1, 30, 200, 600, 1500, 4000]), size=n) + rng.integers(0, 300, size=n)
    ts = np.maximum(centre, 0)
    te = ts + length
    # touching: a segment that starts one past the end of the one before it (tStart = tEnd: a new island) or at its end
    touch = np.nonzero(rng.random(n) < 0.04)[0]
    touch = touch[touch > 0]
    c[touch] = c[touch - 1]
    ts[touch] = te[touch - 1] - (rng.random(len(touch)) < 0.5)
    te[touch] = ts[touch] + length[touch]
    if degenerate:
        deg = rng.random(n) < degenerate
        te[deg] = ts[deg] - rng.integers(0, 50, size=int(deg.sum()))
    return c, ts, te


def est_table(rng, c, ts, te, crlf=False, junk=True, chroms=CHROMS):
    """An intronEst-shaped table (bin + 21 PSL columns) of the segments, with header, comment, short and blank lines."""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    if junk:
        out.append(b"#bin\tmatches\tmisMatches\trepMatches\tnCount\tqNumInsert\tqBaseInsert\ttNumInsert\ttBaseInsert\tstrand\tqName\tqSize"
                   b"\tqStart\tqEnd\ttName\ttSize\ttStart\ttEnd\tblockCount\tblockSizes\tqStarts\ttStarts")
    for k in range(len(c)):
        ln = int(te[k]) - int(ts[k])
        out.append(b"%d\t%d\t0\t0\t0\t0\t0\t1\t%d\t+\tBX%07d\t%d\t0\t%d\t%s\t250000000\t%d\t%d\t2\t10,20,\t0,10,\t%d,%d," % (
            585 + k % 7, max(ln, 0), max(ln - 30, 0), k, max(ln, 1), max(ln, 1), chroms[int(c[k])], int(ts[k]), int(te[k]), int(ts[k]),
            int(te[k]) - 20))
        if junk and k % 997 == 3:
            out.append(b"")
        if junk and k % 1511 == 5:
            out.append(b"12\tshort\tline")
        if junk and k % 2003 == 7:
            out.append(b"# comment\t" * 20)
    return nl.join(out) + nl


def break_psl(rng, c, ts, te, crlf=False, junk=True, chroms=CHROMS):
    """A blat -noHead PSL (21 columns) of break alignments, with junk lines as est_table."""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for k in range(len(c)):
        name = chroms[int(c[k])] if c[k] >= 0 else b"chrNotThere"
        ln = int(te[k]) - int(ts[k])
        out.append(b"%d\t1\t0\t0\t0\t0\t0\t0\t+\tbreak%d\t%d\t0\t%d\t%s\t250000000\t%d\t%d\t1\t%d,\t0,\t%d," % (
            max(ln, 0), k, max(ln, 1), max(ln, 1), name, int(ts[k]), int(te[k]), max(ln, 1), int(ts[k])))
        if junk and k % 331 == 2:
            out.append(b"")
        if junk and k % 557 == 9:
            out.append(b"psLayout version 3")
    return nl.join(out) + nl


def queries_near(rng, islands_by_chrom, chroms, n, span=2_000_000):
    """n break segments (chromosome index or -1, tStart, tEnd): most at or across the padded edges of islands, exactly +-300
    among them, the rest random."""
    names = [chrom_key(x) for x in chroms]
    qc = rng.integers(-1, len(chroms), size=n)
    qs = np.zeros(n, dtype=np.int64)
    qe = np.zeros(n, dtype=np.int64)
    for k in range(n):
        isl = islands_by_chrom.get(names[qc[k]]) if qc[k] >= 0 else None
        if not isl or not isl[0] or rng.random() < 0.15:
            s = int(rng.integers(0, span))
            qs[k], qe[k] = s - 1, s + int(rng.integers(0, 3000))
            continue
        j = int(rng.integers(0, len(isl[0])))
        a, b = isl[0][j], isl[1][j]
        r = rng.random()
        d1, d2 = (int(rng.integers(-2, 3)) for _ in range(2))
        if r < 0.4:                                           # padded edges, exactly and one off
            s, e = a - PAD + d1, b + PAD + d2
        elif r < 0.7:
            s = int(rng.integers(a - PAD - 5, b + 1))
            e = s + int(rng.integers(0, max(1, b + PAD + 5 - s)))
        else:
            s, e = a + int(rng.integers(-1000, 1000)), b + int(rng.integers(-1000, 1000))
        qs[k], qe[k] = s - 1, e                              # tStart = start - 1
    return qc, qs, qe
