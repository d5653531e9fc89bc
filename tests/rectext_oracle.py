"""The rules of the "alignment text" section of include/defuse_rec.h restated in plain Python: the checker of
tests/test_rectext.py.  Lines, the integer rule, the stop with its kind, field and id, plain-ness, the records, and the
expected sorted text through rec_case.expected_text."""
import numpy as np

from defuse_amd.dsa import RECORD_DTYPE
from tests import rec_case

FEW_FIELDS, BAD_INTEGER, BAD_BOOL = 1, 2, 3
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
DIGITS = frozenset(b"0123456789")


def lines_of(data, final=True):
    """(the lines without their newlines, the bytes they take up).  Only b"\\n" ends a line; with final a last line without
    one is a line, without final it is left for the next piece."""
    parts = data.split(b"\n")
    last = parts.pop()
    used = len(data) - len(last)
    if final and last:
        parts.append(last)
        used = len(data)
    return parts, used


def field_int(f):
    """The int of a field, or None: an optional sign, then digits only, at least one, and a value in the int range."""
    body = f[1:] if f[:1] in (b"+", b"-") else f
    if not body or not set(body) <= DIGITS:
        return None
    v = int(body) * (-1 if f[:1] == b"-" else 1)
    return v if INT_MIN <= v <= INT_MAX else None


def parse_line(line):
    """dict(kind, field, id_read, id, values, plain) of one line (no newline)."""
    f = line.split(b"\t")
    out = dict(kind=0, field=-1, id_read=0, id=0, values=None, plain=False)
    if len(f) >= 7 and field_int(f[0]) is not None:
        out.update(id_read=1, id=field_int(f[0]))
    if len(f) < 9:
        out["kind"] = FEW_FIELDS
        return out
    values = []
    for k in range(9):
        if k == 3:
            if f[k] not in (b"0", b"1"):
                out.update(kind=BAD_BOOL, field=k)
                return out
            values.append(int(f[k]))
        else:
            v = field_int(f[k])
            if v is None:
                out.update(kind=BAD_INTEGER, field=k)
                return out
            values.append(v)
    out["values"] = tuple(values)
    out["plain"] = line == b"%d\t" * 9 % tuple(values)
    return out


def records_of(rows):
    r = np.zeros(len(rows), RECORD_DTYPE)
    for k, name in enumerate(rec_case.FIELDS):
        r[name] = [row[k] for row in rows]
    return r


def parse(data, final=True):
    """What rect_add reports for one piece, and the records it appends: (result dict, records)."""
    lines, used = lines_of(data, final)
    res = dict(consumed=used, n_lines=len(lines), n_records=len(lines), stop_line=0, n_other=0, first_other=0, stop_kind=0, stop_field=-1,
               stop_id_read=0, stop_id=0)
    rows, pos = [], 0
    for k, line in enumerate(lines):
        p = parse_line(line)
        if p["kind"]:
            res.update(consumed=pos, n_lines=k, n_records=k, stop_line=k + 1, stop_kind=p["kind"], stop_field=p["field"], stop_id_read=p["id_read"],
                       stop_id=p["id"])
            break
        if not p["plain"]:
            res["n_other"] += 1
            res["first_other"] = res["first_other"] or k + 1
        rows.append(p["values"])
        pos += len(line) + 1
    return res, records_of(rows)


def sorted_text(files):
    """`LC_ALL=C sort -n -k 1 FILE...` for files of plain lines: a file without a final newline ends its own last line."""
    lines = []
    for data in files:
        got, _ = lines_of(data, True)
        lines += [l + b"\n" for l in got]
    return rec_case.expected_text(lines)
