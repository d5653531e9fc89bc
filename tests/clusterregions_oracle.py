"""The "cluster text" section of include/defuse_task.h restated on bytes: what `defuse_glue remove_duplicates MIN` and
`defuse_glue get_align_regions` print, and where and why they stop.  No GPU, no library: plain Python over the input's bytes."""
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
FEW_FIELDS, BAD_INTEGER, MISSING_END, NOT_TWO_ENDS = 1, 2, 3, 4


def field_int(b):
    """An optional sign, digits only, inside int: the value or None."""
    digits = b[1:] if b[:1] in (b"+", b"-") else b
    if not digits or not all(48 <= c <= 57 for c in digits):
        return None
    v = int(digits) * (-1 if b[:1] == b"-" else 1)
    return v if INT_MIN <= v <= INT_MAX else None


def lines_of(data):
    """[(offset, line without its newline)]: a last line without a newline is a line, empty text has none."""
    out, pos = [], 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl
        out.append((pos, data[pos:end]))
        pos = end + 1
    return out


def parse_line(line):
    """One line by both steps' rules, as taskc_shared.hpp's taskc_line: a dict of its fields."""
    L = dict(id=0, ce=0, frag=0, pos=0, start=0, end=0, name_off=0, name_len=0, strand_off=0, strand_len=0, dkind=0, dfield=-1, rkind=0, rfield=-1,
             name=b"", strand=b"")
    f = line.split(b"\t")
    if len(f) < 8:
        L["dkind"] = L["rkind"] = FEW_FIELDS
        return L
    v = {k: field_int(f[k]) for k in (0, 1, 2, 6, 7)}
    L["id"], L["ce"], L["frag"] = (v[k] if v[k] is not None else 0 for k in (0, 1, 2))
    L["name"], L["strand"] = f[4], f[5]
    L["name_off"] = sum(len(x) + 1 for x in f[:4])
    L["name_len"] = len(f[4])
    L["strand_off"] = L["name_off"] + len(f[4]) + 1
    L["strand_len"] = len(f[5])
    bad3 = [k for k in (0, 1, 2) if v[k] is None]
    if bad3:
        L["dkind"], L["dfield"] = BAD_INTEGER, bad3[0]
    elif v[1] in (0, 1):
        pf = 6 if f[5] == b"+" else 7
        if v[pf] is None:
            L["dkind"], L["dfield"] = BAD_INTEGER, pf
        else:
            L["pos"] = v[pf]
    bad4 = [k for k in (0, 1, 6, 7) if v[k] is None]
    if bad4:
        L["rkind"], L["rfield"] = BAD_INTEGER, bad4[0]
    else:
        L["start"], L["end"] = v[6], v[7]
    return L


def result(n_lines=0, stop=None, **counts):
    """A taskc_result as a dict; stop = (line index or None, offset, length, kind, field, value)."""
    r = dict(n_lines=n_lines, n_runs=0, n_clusters=0, n_fragments=0, n_kept_fragments=0, n_kept_runs=0, out_bytes=0, stop_line=0, stop_off=0, stop_len=0,
             stop_value=0, stop_kind=0, stop_field=-1)
    if stop is not None:
        line, off, length, kind, field, value = stop
        r.update(stop_line=0 if line is None else line + 1, stop_off=off, stop_len=length, stop_kind=kind, stop_field=field, stop_value=value)
    else:
        r.update(counts)
    return r


def dedup(data, min_cluster_size):
    """(result, the de-duplicated text or None with a stop)."""
    lines = lines_of(data)
    recs = [parse_line(l) for _, l in lines]
    n = len(lines)
    first = next((i for i, r in enumerate(recs) if r["dkind"]), None)
    m = n if first is None else first
    # a line that stops on its position field belongs to its run: the run of the line in front of it, if they share the id, is open
    open_tail = first is not None and first > 0 and recs[first]["dkind"] == BAD_INTEGER and recs[first]["dfield"] >= 6 and recs[first]["id"] == recs[first - 1]["id"]
    runs = []                                   # [first line, one past the last]
    for i in range(m):
        if i == 0 or recs[i]["id"] != recs[i - 1]["id"]:
            runs.append([i, i + 1])
        else:
            runs[-1][1] = i + 1
    frags_of = []
    for k, (a, b) in enumerate(runs):
        frags = {}
        for i in range(a, b):
            if recs[i]["ce"] in (0, 1):
                frags.setdefault(recs[i]["frag"], {})[recs[i]["ce"]] = i          # the last line wins
        frags_of.append(frags)
        missing = sorted(fr for fr, ends in frags.items() if len(ends) != 2)
        if missing and not (open_tail and k == len(runs) - 1):
            off, line = lines[b - 1]
            return result(n, (b - 1, off, len(line), MISSING_END, -1, missing[0])), None
    if first is not None:
        off, line = lines[first]
        return result(n, (first, off, len(line), recs[first]["dkind"], recs[first]["dfield"], 0)), None
    out, n_frag, n_kept, n_kept_runs = [], 0, 0, 0
    for frags in frags_of:
        n_frag += len(frags)
        seen, kept = set(), []
        for fr in sorted(frags, key=lambda fr: (recs[frags[fr][0]]["pos"], recs[frags[fr][1]]["pos"], fr)):
            pair = (recs[frags[fr][0]]["pos"], recs[frags[fr][1]]["pos"])
            if pair not in seen:
                seen.add(pair)
                kept.append(fr)
        if len(kept) >= min_cluster_size:
            n_kept_runs += 1
            n_kept += len(kept)
            for fr in sorted(kept):
                out += [lines[frags[fr][0]][1] + b"\n", lines[frags[fr][1]][1] + b"\n"]
    text = b"".join(out)
    return result(n, n_runs=len(runs), n_fragments=n_frag, n_kept_fragments=n_kept, n_kept_runs=n_kept_runs, out_bytes=len(text)), text


def regions(data):
    """(result, the regions text or None with a stop)."""
    lines = lines_of(data)
    n = len(lines)
    groups = {}
    for i, (off, line) in enumerate(lines):
        r = parse_line(line)
        if r["rkind"]:
            return result(n, (i, off, len(line), r["rkind"], r["rfield"], 0)), None
        g = groups.setdefault((r["id"], r["ce"]), [b"", b"", r["start"], r["end"]])
        g[0], g[1], g[2], g[3] = r["name"], r["strand"], min(g[2], r["start"]), max(g[3], r["end"])
    ends = {}
    for cid, ce in groups:
        ends[cid] = ends.get(cid, 0) + 1
    bad = sorted(cid for cid, k in ends.items() if k != 2)
    if bad:
        return result(n, (None, 0, 0, NOT_TWO_ENDS, -1, bad[0])), None
    text = b"".join(b"%d\t%d\t%s\t%s\t%d\t%d\n" % (cid, ce, g[0], g[1], g[2], g[3]) for (cid, ce), g in sorted(groups.items()))
    return result(n, n_clusters=len(ends), out_bytes=len(text)), text
