"""The "span statistics" section of include/defuse_ptext.h restated on bytes: what `defuse_glue calc_span_stats` prints for a
cluster file, a .break file and a .seq file, and where and why it stops.  No GPU, no library: plain Python over the bytes."""
from tests.clusterregions_oracle import INT_MAX, INT_MIN, field_int, lines_of     # noqa: F401  (the same integer rule and lines)

FEW_FIELDS, BAD_INTEGER, NOT_TWO_ENDS, NO_BREAK_END, COORD_LIMIT, NO_INTER, SUM_LIMIT = 1, 2, 3, 4, 5, 6, 7
FILE_CLUSTERS, FILE_BREAKS, FILE_SEQS = 0, 1, 2
MAX_COORD = 1 << 28                # TASK_MAX_COORD
SUM_MAX = 1 << 53
# the order in which an id's stops are looked for
RANK = {NOT_TWO_ENDS: 1, NO_BREAK_END: 2, BAD_INTEGER: 3, COORD_LIMIT: 4, NO_INTER: 5, SUM_LIMIT: 6}


def result(**kw):
    """A span_result as a dict.  n_noncanonical is None after a line stop: the library counts on all lines of the text, not on
    those in front of the stop, and the count of a text that stopped is not compared."""
    r = dict(n_lines=0, n_seq_lines=0, n_breaks=0, n_inters=0, n_ids=0, n_rows=0, out_bytes=0, n_noncanonical=0, stop_line=0, stop_value=0, stop_kind=0,
             stop_field=-1, stop_file=0)
    r.update(kw)
    return r


def key_field(b, counter):
    """A key field: its int or None; counter[0] grows where the bytes are not the "%d" of the value."""
    v = field_int(b)
    if v is not None and b != b"%d" % v:
        counter[0] += 1
    return v


def file_lines(data, n_fields, keys, plain):
    """The lines of a .break or .seq text: ([(key ints..., value)], noncanonical, stop) with stop None or (line, kind, field)."""
    out, nc = [], [0]
    for n, (_, line) in enumerate(lines_of(data)):
        f = line.split(b"\t")
        if len(f) < n_fields:
            return out, nc[0], (n + 1, FEW_FIELDS, -1)
        vals = []
        for k in keys:
            v = key_field(f[k], nc)
            if v is None:
                return out, nc[0], (n + 1, BAD_INTEGER, k)
            vals.append(v)
        v = field_int(f[plain])
        if v is None:
            return out, nc[0], (n + 1, BAD_INTEGER, plain)
        out.append(tuple(vals) + (v,))
    return out, nc[0], None


def tables(brk, seq):
    """span_breaks_text: (result, (break, inter)) with break {(id, end): position} and inter {id: length}; the tables are None
    after a stop.  The .break text is looked at first."""
    res = result(n_lines=len(lines_of(brk)))
    rows, nc, stop = file_lines(brk, 5, (0, 1), 4)
    res["n_noncanonical"] += nc
    if stop:
        res.update(stop_line=stop[0], stop_kind=stop[1], stop_field=stop[2], stop_file=FILE_BREAKS, n_noncanonical=None)
        return res, None
    res["n_seq_lines"] = len(lines_of(seq))
    srows, nc, stop = file_lines(seq, 3, (0,), 2)
    res["n_noncanonical"] += nc
    if stop:
        res.update(stop_line=stop[0], stop_kind=stop[1], stop_field=stop[2], stop_file=FILE_SEQS, n_noncanonical=None)
        return res, None
    brk_map = {(i, e): v for i, e, v in rows}
    inter = {i: v for i, v in srows}
    res.update(n_breaks=len(brk_map), n_inters=len(inter))
    return res, (brk_map, inter)


def tables_of_pred(rows):
    """span_breaks_pred on the rows of pred_fetch: groups with PRED_NO_TASK (4) or PRED_OUT_OF_WINDOW (8) give nothing, a group
    with EVAL_NO_SPLIT (1) break positions 0."""
    brk_map, inter = {}, {}
    for row in rows:
        fid, st = int(row["fusion_id"]), int(row["status"])
        if st & (4 | 8):
            continue
        for e in (0, 1):
            brk_map[(fid, e)] = 0 if st & 1 else int(row["break_pos"][e])
        inter[fid] = 0
    return result(n_lines=len(rows), n_breaks=len(brk_map), n_inters=len(inter)), (brk_map, inter)


def g15(x):
    """What Perl prints for a number: "%.15g"."""
    return b"%.15g" % x


def stats(clusters, tabs):
    """span_stats: (result, rows, text) with rows [(id, count, sum, mean)]; rows and text are None after a stop."""
    brk_map, inter = tabs
    with_break = {i for i, _ in brk_map}
    lines = lines_of(clusters)
    res = result(n_lines=len(lines))
    nc = [0]
    strand, winner, ends, ids = {}, {}, {}, []
    for n, (_, line) in enumerate(lines):
        f = line.split(b"\t")
        if len(f) < 8:
            res.update(stop_line=n + 1, stop_kind=FEW_FIELDS, stop_file=FILE_CLUSTERS, n_noncanonical=None)
            return res, None, None
        v = [key_field(f[k], nc) for k in (0, 1, 2)]
        if None in v:
            res.update(stop_line=n + 1, stop_kind=BAD_INTEGER, stop_field=v.index(None), stop_file=FILE_CLUSTERS, n_noncanonical=None)
            return res, None, None
        cid, ce, frag = v
        strand[(cid, ce)] = f[5]
        winner.setdefault(cid, {})[(frag, ce)] = (f[6], f[7])
        ends.setdefault(cid, set()).add(ce)
        ids.append(cid)
    res["n_noncanonical"] = nc[0]
    res["n_ids"] = len(set(ids))
    rows = []
    for cid in sorted(set(ids)):
        if cid not in with_break:
            continue
        stops = []                                          # (rank, field)
        if len(ends[cid]) != 2:
            stops.append((RANK[NOT_TWO_ENDS], -1))
        total, frags = 0, set()
        for (frag, ce), (start, end) in winner[cid].items():
            frags.add(frag)
            plus = strand[(cid, ce)] == b"+"
            b = brk_map.get((cid, ce))
            if b is None:
                stops.append((RANK[NO_BREAK_END], -1))
            elif abs(b) > MAX_COORD:
                stops.append((RANK[COORD_LIMIT], -1))
            p = field_int(start if plus else end)
            if p is None:
                stops.append((RANK[BAD_INTEGER], 6 if plus else 7))
            elif abs(p) > MAX_COORD:
                stops.append((RANK[COORD_LIMIT], -1))
            if b is not None and p is not None:
                total += b - p + 1 if plus else p - b + 1
        if cid not in inter:
            stops.append((RANK[NO_INTER], -1))
        elif abs(inter[cid]) > MAX_COORD:
            stops.append((RANK[COORD_LIMIT], -1))
        else:
            total += inter[cid] * len(frags)
        if not stops and abs(total) > SUM_MAX:
            stops.append((RANK[SUM_LIMIT], -1))
        if stops:
            rank, field = min(stops)
            kind = {v: k for k, v in RANK.items()}[rank]
            res.update(stop_kind=kind, stop_field=field if kind == BAD_INTEGER else -1, stop_value=cid, stop_file=FILE_CLUSTERS)
            return res, None, None
        rows.append((cid, len(frags), total, float(total) / float(len(frags))))
    text = b"".join(b"%d\t%s\t%d\n" % (cid, g15(mean), count) for cid, count, _, mean in rows)
    res.update(n_rows=len(rows), out_bytes=len(text))
    return res, rows, text


def run(clusters, brk, seq):
    """The three files through both steps, as the tools do: (result of the step that stopped or of stats, text or None)."""
    res, tabs = tables(brk, seq)
    if tabs is None:
        return res, None
    res2, _, text = stats(clusters, tabs)
    res2["n_noncanonical"] = None if res2["n_noncanonical"] is None else res2["n_noncanonical"] + res["n_noncanonical"]
    return res2, text
