"""Inputs and the expected order for tests/test_records.py (include/defuse_rec.h).

The expected order is, everywhere, the Python expression of expected_text(): numeric fusion id, then the bytes of the line.
test_records.py pins that expression against GNU sort once, without a GPU."""
import numpy as np

from defuse_amd.dsa import RECORD_DTYPE

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
EDGE = [0, 1, 9, 10, 11, 99, 100, 101, 999, 1000, -1, -9, -10, -11, -100, 1999999999, 200000000, INT_MAX, INT_MIN]
FIELDS = RECORD_DTYPE.names[:9]
FMT = b"%d\t" * 9 + b"\n"


def lines_of(records):
    """SplitAlignment::WriteAlignment of every record: nine "%d\\t" and a newline."""
    return [FMT % t for t in zip(*(records[f].tolist() for f in FIELDS))]


def expected_text(lines):
    return b"".join(sorted(lines, key=lambda l: (int(l.split(b"\t")[0]), l)))


def expected_order(records, lines=None):
    """The indices of the records in the expected order; equal lines keep their input order (sorted() is stable)."""
    lines = lines_of(records) if lines is None else lines
    fid = records["fusion_id"].tolist()
    return np.array(sorted(range(len(lines)), key=lambda i: (fid[i], lines[i])), dtype=np.int64)


def numeric_order(records):
    """What a sort by the numeric values of the nine fields gives: the wrong order every test must be able to tell."""
    return np.lexsort(tuple(records[f] for f in reversed(FIELDS)))


def text_of(lines, order):
    return b"".join(lines[i] for i in order)


def draw(rng, n, flags01=False, fusion_ids=None):
    """n records.  A third of them draw every field from the edge set, a third from small ranges (so that records agree in
    many leading fields and a late field decides), a third from the full int32 range; fusion ids of both signs from a short
    list, so that fusions have many records.  flags01: read_end and revcomp are 0 or 1, as in every record dsa_* produces."""
    r = np.zeros(n, RECORD_DTYPE)
    edge = np.array(EDGE, dtype=np.int64)
    kind = rng.integers(0, 3, n)
    for f in FIELDS[1:]:
        v = np.where(kind == 0, edge[rng.integers(0, len(edge), n)],
                     np.where(kind == 1, rng.integers(-2, 3, n) * rng.choice(np.array([1, 5, 50]), n), rng.integers(INT_MIN, INT_MAX + 1, n)))
        r[f] = v.astype(np.int32)
    ids = np.array([-100, -11, -10, -9, -1, 0, 1, 9, 10, 11, 99, 100, INT_MAX, INT_MIN] if fusion_ids is None else fusion_ids, dtype=np.int64)
    r["fusion_id"] = ids[rng.integers(0, len(ids), n)].astype(np.int32)
    if flags01:
        r["read_end"] = rng.integers(0, 2, n)
        r["revcomp"] = rng.integers(0, 2, n)
    r["pair_idx"] = np.arange(n) % 1000003
    return r


def parts_of(records, cuts):
    """The records as consecutive pieces ending at the given cuts (an empty piece where two cuts are equal)."""
    edges = [0] + [min(c, len(records)) for c in cuts] + [len(records)]
    return [records[a:b] for a, b in zip(edges[:-1], edges[1:])]
