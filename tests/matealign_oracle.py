"""CPU restatement of the reference `matealign` tool (tools/matealign.cpp:39-205) — TEST INFRASTRUCTURE ONLY.

Parity unpinned: the reference holds no test or golden vector for matealign, and the tool cannot be compiled here (Common.h pulls
in Boost headers the image lacks).  Scores come from oracle.localalign_oracle.simple_align (ora_simple_align,
SimpleAligner.cpp:24-64) and numbers are printed with its format_double; this module restates the protocol around them:

  * SAM on stdin, per line in this order: an empty line ends the run (`Error: Empty alignment line N`); `@` lines are skipped;
    fewer than ten tab-separated fields is `Format error for alignment line N`; flag and pos must be ints; only then a line
    with rname `*` is skipped; the qname must split on `/` into exactly two parts, the second `1` or `2`; the first must be an
    int.  Strand from flag 0x10; anchor pos (plus) or pos + len(SEQ) - 1 (minus).  Alignments keyed by ReadID
    (fragment & 0x7fffffff | end << 31), kept in SAM order.
  * `Read alignments`, then the FASTA (Sequences::Read: whole header line as name, empty lines skipped, last contig of a name
    wins; a file that cannot be opened is `Error: unable to open file X`), then `Read reference fasta`.
  * Both FASTQ files are opened (IReadStream::Create: extension fastq / fq, else `Error: unrecognized extension X`; a file
    that cannot be opened is `Error: unable to open file X`); if either failed, `Error: unable to read sequences` on stdout,
    exit 1.  Records of four lines; a bad name or end prints its message and ends that file quietly.
  * Every record of file 1, then of file 2: fragment as int (not an int: `Error: bad integer 'X' in read name NAME`, exit 1 —
    the reference dies of an uncaught bad_lexical_cast there), then for every alignment of the other end the window
    [pos, pos+s] reverse-complemented (plus) or [anchor-s, anchor] (minus) through Sequences::Get (unknown name: `Error:
    Unable to find sequence X`, exit 1; a start beyond the contig, where substr throws: an `Error: window start` line, exit
    1), score, maxScore = len(read) * match, percent, line `fragment \\t score \\t percent` unless percent < threshold.
"""
import math

import numpy as np

from oracle.localalign_oracle import format_double, simple_align

_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


class _Exit(Exception):
    def __init__(self, code):
        self.code = code


def lexical_int(s):
    """boost::lexical_cast<int> of a byte or text string; None where it throws."""
    if isinstance(s, bytes):
        s = s.decode("latin-1")
    body = s[1:] if s[:1] in ("+", "-") else s
    if not body or not all("0" <= c <= "9" for c in body):
        return None
    v = int(s)
    return v if -2 ** 31 <= v < 2 ** 31 else None


def i32(v):
    """C++ int conversion of an integer (wraps modulo 2^32)."""
    return int(np.int64(v).astype(np.int32)) if -2 ** 63 <= v < 2 ** 63 else int(np.int64(v & 0xFFFFFFFF).astype(np.int32))


def read_fasta(data):
    """Sequences::Read on the bytes of a FASTA file: {name bytes: sequence bytes}."""
    seqs, name, parts = {}, b"", []
    for line in _lines(data):
        if not line:
            continue
        if line[:1] == b">":
            if name:
                seqs[name] = b"".join(parts)
            name, parts = line[1:], []
        else:
            parts.append(line)
    if name:
        seqs[name] = b"".join(parts)
    return seqs


def get_parts(full_len, start, end):
    """Sequences::Get's int arithmetic: (slice start 0-based, slice length, pad_left, pad_right), or None where substr throws."""
    seq_start = max(1, start)
    prepend = seq_start - start
    seq_end = min(full_len, end)
    append = end - seq_end
    length = seq_end - seq_start + 1
    if seq_start - 1 > full_len:
        return None
    return seq_start - 1, (length if length >= 0 else full_len - (seq_start - 1)), prepend, append


def get(full, start, end):
    """Sequences::Get of [start, end] (1-based) on a contig: N padding, substr taking the tail for a negative length."""
    p = get_parts(len(full), start, end)
    if p is None:
        return None
    off, n, pl, pr = p
    return b"N" * pl + full[off:off + n] + b"N" * pr


def reverse_complement(s):
    return s[::-1].translate(_COMPLEMENT)


def window(full, strand, anchor, s):
    """The reference string the tool aligns a read against, for a mate at `anchor` on `strand` (0 plus, 1 minus)."""
    if strand == 0:
        w = get(full, anchor, i32(anchor + s))
        return None if w is None else reverse_complement(w)
    return get(full, i32(anchor - s), anchor)


def _lines(data):
    """std::getline over bytes: lines without their newline, a last line without one kept."""
    if not data:
        return []
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def fastq_records(path, err):
    """IReadStream::Create + FastqReadStream::GetNextRead: None if the stream is not created, else a list of (fragment text,
    end, sequence) in file order up to the first record that ends the file (its message appended to err)."""
    ext = path[path.rfind(".") + 1:]
    if ext not in ("fastq", "fq"):
        err.append("Error: unrecognized extension %s\n" % ext)
        return None
    try:
        data = open(path, "rb").read()
    except OSError:
        err.append("Error: unable to open file %s\n" % path)
        return None
    lines, out = _lines(data), []
    for k in range(0, len(lines) - 3, 4):
        name, seq = lines[k], lines[k + 1]
        if name[:1] != b"@":
            out.append(("msg", "Error: Unable to interpret read name %s\n" % name.decode("latin-1")))
            break
        slash = name.find(b"/")
        endc = name[slash + 1:slash + 2] if slash >= 0 else b""
        if endc not in (b"1", b"2"):
            out.append(("msg", "Error: Unable to interpret read end %s\n" % name.decode("latin-1")))
            break
        out.append((name[1:slash], 0 if endc == b"1" else 1, seq, name))
    return out


def run(sam_lines, fasta, fq1, fq2, match, mismatch, gap, search, threshold=0.0):
    """(stdout, stderr, exit status) of `matealign -m -x -g -s -r fasta -1 fq1 -2 fq2 [-t]` fed with `sam_lines` (text lines)."""
    out, err = [], []
    try:
        _run(sam_lines, fasta, fq1, fq2, match, mismatch, gap, search, threshold, out, err)
        code = 0
    except _Exit as e:
        code = e.code
    return "".join(out), "".join(err), code


def _die(err, msg):
    err.append(msg + "\n")
    raise _Exit(1)


def _run(sam_lines, fasta, fq1, fq2, match, mismatch, gap, search, threshold, out, err):
    alignments = {}
    for n, line in enumerate(sam_lines, 1):
        line = line.rstrip("\n")
        if not line:
            _die(err, "Error: Empty alignment line %d" % n)
        if line[0] == "@":
            continue
        f = line.split("\t")
        if len(f) < 10:
            _die(err, "Error: Format error for alignment line %d" % n)
        flag, pos = lexical_int(f[1]), lexical_int(f[3])
        if flag is None or pos is None:
            _die(err, "Error: bad integer in sam line %d" % n)
        if f[2] == "*":
            continue
        strand = 1 if flag & 0x10 else 0
        q = f[0].split("/")
        if len(q) != 2 or q[1] not in ("1", "2"):
            _die(err, "Error: Unable to interpret qname for alignment line %d" % n)
        end = i32(pos + len(f[9].encode("latin-1")) - 1)
        frag = lexical_int(q[0])
        if frag is None:
            _die(err, "Error: bad integer in sam line %d" % n)
        key = (frag & 0x7FFFFFFF, 0 if q[1] == "1" else 1)
        alignments.setdefault(key, []).append((f[2].encode("latin-1"), strand, pos if strand == 0 else end))
    err.append("Read alignments\n")
    try:
        seqs = read_fasta(open(fasta, "rb").read())
    except OSError:
        _die(err, "Error: unable to open file %s" % fasta)
    err.append("Read reference fasta\n")
    files = [fastq_records(p, err) for p in (fq1, fq2)]
    if files[0] is None or files[1] is None:
        out.append("Error: unable to read sequences\n")
        raise _Exit(1)
    for records in files:
        for rec in records:
            if rec[0] == "msg":
                err.append(rec[1])
                break
            frag_text, read_end, seq, name = rec
            frag = lexical_int(frag_text)
            if frag is None:
                _die(err, "Error: bad integer '%s' in read name %s" % (frag_text.decode("latin-1"), name.decode("latin-1")))
            for rname, strand, anchor in alignments.get((frag & 0x7FFFFFFF, 1 - read_end), []):
                if rname not in seqs:
                    _die(err, "Error: Unable to find sequence %s" % rname.decode("latin-1"))
                ref = window(seqs[rname], strand, anchor, search)
                if ref is None:
                    start = anchor if strand == 0 else i32(anchor - search)
                    _die(err, "Error: window start %d lies beyond the end of sequence %s (length %d)" %
                         (start, rname.decode("latin-1"), len(seqs[rname])))
                score = simple_align(match, mismatch, gap, ref, seq)
                max_score = i32(len(seq) * match)
                if max_score == 0:
                    percent = -math.nan if score == 0 else math.copysign(math.inf, score)     # x86: 0.0/0.0 is -nan
                else:
                    percent = float(score) / float(max_score)
                if percent < threshold:
                    continue
                out.append("%d\t%d\t%s\n" % (frag & 0x7FFFFFFF, score, format_double(percent)))
