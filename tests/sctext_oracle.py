"""The setcover tool on the bytes of a cluster file, in plain Python.  TEST INFRASTRUCTURE ONLY.

Restates ReadClusters and WriteClusters of the reference (tools/Parsers.cpp:23-170) as include/defuse_sc.h's "cluster text"
section words them, around oracle/setcover_oracle.set_cover for the greedy:

  lines          std::getline (:36, :125): a line ends at '\\n', a last line without one is a line, empty text has none
  kind 1         line.length() == 0                                  (:42-46, :131-135)
  kind 2         fewer than three fields split at '\\t'               (:48-55, :137-144)
  kind 3         lexical_cast<int> of field 0, 1 or 2 throws         (:57-59, :76-80; the writer casts 0 and 2 only, :146-147,
                                                                      but a line that fails there has stopped the reader)
  kind 4         reader: clusterEnd == 0 and clusterID < 0 (:61-71); writer: clusterID < 0 on any line (:149-153)
  clusters       clusters[clusterID].push_back(fragmentIndex) of the end-0 lines in file order (:73-74)
  negative       "Error: negative elements not permitted" of tools/setcover.cpp's SetCover, between the two passes
  kept           the line's fragment is in the solution of the line's cluster, and that holds at least minClusterSize
                 fragments (:93-104, :156-159); a cluster id beyond the table is passed over (the reference indexes past
                 the vector there)

Returns (status, stop_kind, stop_line, output bytes) with the SCT_* numbers of the header.
"""
from oracle import setcover_oracle

OK, READ_STOP, NEGATIVE_ELEMENT, WRITE_STOP = 0, 1, 2, 3
EMPTY_LINE, FEW_FIELDS, BAD_INTEGER, BAD_CLUSTER_ID = 1, 2, 3, 4


def lexical_int(field):
    """boost::lexical_cast<int> of bytes: an optional sign, digits only, inside the int range; None where it throws."""
    digits = field[1:] if field[:1] in (b"+", b"-") else field
    if not digits or any(not 48 <= b <= 57 for b in digits):
        return None
    v = int(digits) * (-1 if field[:1] == b"-" else 1)
    return v if -2 ** 31 <= v <= 2 ** 31 - 1 else None


def lines_of(data):
    lines = data.split(b"\n")
    if lines[-1] == b"":            # behind the last newline (or in empty text) there is no line
        lines.pop()
    return lines


def parse(line):
    """(kind, clusterID, clusterEnd, fragmentIndex) by the checks both passes share."""
    if len(line) == 0:
        return EMPTY_LINE, 0, 0, 0
    fields = line.split(b"\t")
    if len(fields) < 3:
        return FEW_FIELDS, 0, 0, 0
    v = [lexical_int(f) for f in fields[:3]]
    if None in v:
        return BAD_INTEGER, 0, 0, 0
    return 0, v[0], v[1], v[2]


def setcover_text(data, min_cluster_size):
    lines = lines_of(data)
    parsed = [parse(l) for l in lines]
    clusters = []
    for n, (kind, cid, end, frag) in enumerate(parsed, 1):                  # ReadClusters
        if kind == 0 and end == 0 and cid < 0:
            kind = BAD_CLUSTER_ID
        if kind:
            return READ_STOP, kind, n, b""
        if end != 0:
            continue
        while len(clusters) <= cid:
            clusters.append([])
        clusters[cid].append(frag)
    if any(e < 0 for c in clusters for e in c):
        return NEGATIVE_ELEMENT, 0, 0, b""
    solution = setcover_oracle.set_cover(clusters)
    keep = [set(s) if len(s) >= min_cluster_size else set() for s in solution]
    out = []
    for n, (line, (kind, cid, end, frag)) in enumerate(zip(lines, parsed), 1):      # WriteClusters
        if cid < 0:
            return WRITE_STOP, BAD_CLUSTER_ID, n, b"".join(out)
        if cid < len(keep) and frag in keep[cid]:
            out.append(line + b"\n")
    return OK, 0, 0, b"".join(out)
