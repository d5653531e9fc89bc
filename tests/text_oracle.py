"""The SAM and FASTQ contracts of include/defuse_text.h restated in Python: the yardstick of tests/test_text_parse.py.

tests/test_text_parse.py pins this file to the tools' host parser (ParseSamLine, FastqReader::next and field_int of
tools_src/defuse_host.hpp), which the tool tests pin to the reference."""

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def field_int(b):
    """boost::lexical_cast<int> on a field: an optional sign, digits only, at least one, int range.  None if it fails."""
    if not b:
        return None
    digits = b[1:] if b[:1] in (b"+", b"-") else b
    if not digits or any(c < 0x30 or c > 0x39 for c in digits):
        return None
    v = int(digits)                                      # (Python's integers do not overflow: twenty digits are fine)
    if b[:1] == b"-":
        v = -v
    return v if INT_MIN <= v <= INT_MAX else None


def split_lines(text, final):
    """[(start, end)] of the lines: they end at b"\\n"; a last line without one is a line only with final."""
    lines, s = [], 0
    while True:
        e = text.find(b"\n", s)
        if e < 0:
            break
        lines.append((s, e))
        s = e + 1
    if final and s < len(text):
        lines.append((s, len(text)))
    return lines


def sam_line(line, names):
    """One SAM line -> (kind, alignment): kind 0 = a record, 1 = skipped, 2 .. 5 = a stop.  The alignment is
    [ref, strand, start, end, fragment, read_end] with read_end None where it is carried."""
    if len(line) == 0:
        return 2, None
    if line[:1] == b"@":
        return 1, None
    f = line.split(b"\t")
    if len(f) < 10:
        return 3, None
    flag, pos = field_int(f[1]), field_int(f[3])
    if flag is None or pos is None:
        return 4, None
    if f[2] == b"*":
        return 1, None
    qname, read_end = f[0], None
    if qname.count(b"/") == 1:
        frag, tail = qname.split(b"/")
        if tail not in (b"1", b"2"):
            return 5, None
        read_end = 0 if tail == b"1" else 1
    else:
        frag = qname
        if flag & 0x40:
            read_end = 0
        elif flag & 0x80:
            read_end = 1
    end = (pos + len(f[9]) - 1 + 2 ** 31) % 2 ** 32 - 2 ** 31          # 64-bit sum truncated to int32
    fragment = field_int(frag)
    if fragment is None or fragment < 0:
        fragment = -1
    return 0, [names.get(f[2], -1), 1 if flag & 0x10 else 0, pos, end, fragment, read_end]


def parse_sam(text, names, final=True, carry_in=0):
    """txt_parse_sam: `names` is a sequence of bytes names (index = position).  Returns a dict with the fields of
    txt_sam_result, `alignments` (a list of 6-tuples) and `line_of` (their 1-based line numbers)."""
    index = {n: k for k, n in enumerate(names)}
    res = dict(consumed=0, n_lines=0, n_alignments=0, stop_line=0, n_bad_fragment=0, stop_kind=0, carry_out=carry_in, alignments=[], line_of=[])
    carry = carry_in
    for k, (s, e) in enumerate(split_lines(text, final)):
        kind, a = sam_line(text[s:e], index)
        if kind >= 2:
            res["stop_kind"], res["stop_line"] = kind, k + 1
            break
        res["n_lines"] = k + 1
        res["consumed"] = min(e + 1, len(text))
        if kind == 0:
            if a[5] is None:
                a[5] = carry
            carry = a[5]
            res["alignments"].append(tuple(a))
            res["line_of"].append(k + 1)
            res["n_bad_fragment"] += a[4] < 0
    res["n_alignments"] = len(res["alignments"])
    res["carry_out"] = carry
    return res


def parse_fastq(text, final=True, max_read_len=1 << 24, lines_before=0):
    """txt_fastq_add on one piece of a file of which `lines_before` lines were consumed by earlier pieces.  Returns a dict
    with the fields of txt_fastq_result and `records`: (fragment, read_end, sequence, skipped) in file order, the skipped
    ones (negative fragment) included and marked."""
    lines = split_lines(text, final)
    res = dict(consumed=0, n_records=0, n_skipped=0, stop_line=0, stop_kind=0, records=[])
    n_groups = len(lines) // 4
    for g in range(n_groups):
        name = text[lines[4 * g][0]:lines[4 * g][1]]
        seq = text[lines[4 * g + 1][0]:lines[4 * g + 1][1]]
        kind = 0
        slash = name.find(b"/")
        endc = name[slash + 1:slash + 2] if slash >= 0 else b""
        if name[:1] != b"@":
            kind = 1
        elif endc not in (b"1", b"2"):
            kind = 2
        else:
            fragment = field_int(name[1:slash])
            if fragment is None:
                kind = 3
            elif len(seq) >= max_read_len:
                kind = 4
        if kind:
            res["stop_kind"], res["stop_line"], res["consumed"] = kind, lines_before + 4 * g + 1, len(text)
            break
        res["records"].append((fragment, 0 if endc == b"1" else 1, seq, fragment < 0))
        res["consumed"] = min(lines[4 * g + 3][1] + 1, len(text))
    if final:
        res["consumed"] = len(text)
    res["n_skipped"] = sum(1 for r in res["records"] if r[3])
    res["n_records"] = len(res["records"]) - res["n_skipped"]
    return res


def read_store(records):
    """The kept records of parse_fastq (of one piece or of several, concatenated) -> (bytes, [(off, len, fragment,
    read_end, 0)]): what txt_fastq_fetch returns."""
    data, recs = bytearray(), []
    for fragment, read_end, seq, skipped in records:
        if not skipped:
            recs.append((len(data), len(seq), fragment, read_end, 0))
            data += seq
    return bytes(data), recs
