"""The "alignment and cluster text" section of include/defuse_cmp.h on bytes, in plain Python.  TEST INFRASTRUCTURE ONLY.

Restates CompactAlignmentStream and FragmentAlignmentStream (tools/AlignmentStream.cpp:156-221), the reference-name numbering of
the tool's main loop (tools/clustermatepairs.cpp:430-446) and OutputClusterMember (:376-387) as the header words them:

  lines        std::getline: a line ends at '\\n', a last line without one is a line (with final = 1), empty text has none;
               a '\\r' belongs to its field
  kind 1       the line has length 0
  kind 2       fewer than six fields split at '\\t'
  kind 3       field 0 is no integer (lexical_cast<int>: optional sign, digits only, int range)
  kind 4       field 4 or field 5 is none
  record       (fragment, start, end, ref | strand << 28 | read_end << 29), read_end = 0 iff field 1 is "1", strand = 1 iff
               field 3 is "-", ref = the index of field 2 among the distinct names in order of first appearance, as bytes
  fragments    a line starts one when the BYTES of its field 0 differ from those of the line before it
  a stop       ends the stream: records, fragments and names are those of the lines before it
  pieces       with final = 0 an open last line is not consumed; state (names, the last field 0, counts) carries over

Stream.add mirrors cmpt_add and returns the dict cmpt_result becomes in defuse_amd/cmptext.py; print_rows is the printer.
"""
from tests.sctext_oracle import lexical_int, lines_of

EMPTY_LINE, FORMAT, BAD_FRAGMENT, BAD_POSITION = 1, 2, 3, 4


def parse_line(line):
    """(kind, fields): the kind of stop (0 = none) and the line's fields."""
    if len(line) == 0:
        return EMPTY_LINE, None
    f = line.split(b"\t")
    if len(f) < 6:
        return FORMAT, None
    if lexical_int(f[0]) is None:
        return BAD_FRAGMENT, None
    if lexical_int(f[4]) is None or lexical_int(f[5]) is None:
        return BAD_POSITION, None
    return 0, f


def meta(ref, strand, read_end):
    return ref | (strand << 28) | (read_end << 29)


class Stream:
    """One alignment stream: records as (fragment, start, end, meta) tuples, frag_start closed by the number of records,
    names as bytes in their numbering."""

    def __init__(self, max_names=None):
        self.max_names = max_names
        self.records, self.starts, self.names, self.index = [], [], [], {}
        self.last_field0 = None
        self.n_lines = self.n_bytes = 0
        self.stop = None                        # (kind, 1-based line, offset in the stream, length)
        self.too_many_names = False

    @property
    def frag_start(self):
        return self.starts + [len(self.records)]

    def add(self, text, final=True):
        if not final:
            text = text[:text.rfind(b"\n") + 1]
        if self.stop is None:
            offset = self.n_bytes
            for line in lines_of(text):
                self.n_lines += 1
                kind, f = parse_line(line)
                if kind:
                    self.stop = (kind, self.n_lines, offset, len(line))
                    break
                if f[2] not in self.index:
                    if self.max_names is not None and len(self.names) == self.max_names:
                        self.too_many_names = True      # the library refuses the piece (DSA_E_LIMIT)
                        return None
                    self.index[f[2]] = len(self.names)
                    self.names.append(f[2])
                if f[0] != self.last_field0:
                    self.starts.append(len(self.records))
                self.last_field0 = f[0]
                self.records.append((lexical_int(f[0]), lexical_int(f[4]), lexical_int(f[5]),
                                     meta(self.index[f[2]], 1 if f[3] == b"-" else 0, 0 if f[1] == b"1" else 1)))
                offset += len(line) + 1
            self.n_bytes += len(text)
        kind, line, off, length = self.stop or (0, 0, 0, 0)
        return {"consumed": len(text), "n_lines": self.n_lines, "n_records": len(self.records), "n_fragments": len(self.starts),
                "n_names": len(self.names), "stop_line": line, "stop_offset": off, "stop_len": length, "stop_kind": kind}


def parse(data, cuts=(), max_names=None):
    """The stream of `data` given in pieces cut at `cuts` (as defuse_amd.cmptext.parse_pieces gives them): (Stream, last result)."""
    s = Stream(max_names)
    pos = 0
    for cut in cuts:
        res = s.add(data[pos:cut], final=False)
        if res is None:                         # too many names: the stream is over
            return s, None
        pos += res["consumed"]
    return s, s.add(data[pos:], final=True)


def print_rows(rows, names):
    """Two lines per row (anything indexable like cmp_row: cluster_id, and fragment, read_end, ref, strand, start, end per
    end).  Returns (text, None), or (b"", the lowest row with a ref outside `names`)."""
    out = []
    for k, r in enumerate(rows):
        for ce in (0, 1):
            ref = int(r["ref"][ce])
            if not 0 <= ref < len(names):
                return b"", k
            out.append(b"%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (int(r["cluster_id"]), ce, int(r["fragment"][ce]), int(r["read_end"][ce]), names[ref],
                                                              b"+" if int(r["strand"][ce]) == 0 else b"-", int(r["start"][ce]), int(r["end"][ce])))
    return b"".join(out), None
