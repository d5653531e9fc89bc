"""Each fusion's predicted sequence and break positions on the GPU (include/defuse_pred.h through defuse_amd/pred.py).

Yardstick: oracle/dosplitalign_oracle.py:evaluate on each group's rows, which restates tools/SplitAlignment.cpp:545-591,
with the status rules of the header (no task, no split, the two DebugChecks) applied around it by `expected` below; for the
chains the golden break and sequence files.  The averages are compared as bit patterns."""
import ctypes
import os
import struct
import types

import numpy as np
import pytest

from tests import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "tests", "golden", "smoke")
CONFIG1 = os.path.join(ROOT, "tests", "golden", "config1")
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
NO_SPLIT, HOST_STATS, NO_TASK, OUT_OF_WINDOW = 1, 2, 4, 8
ODD_BYTES = b"ACGTNacgtn.\x00\xff*"


@pytest.fixture(scope="module")
def pred(built):
    from defuse_amd import pred as p
    return p


@pytest.fixture(scope="module")
def bat(built):
    from defuse_amd import bat as b
    return b


@pytest.fixture(scope="module")
def ectx(built):
    from defuse_amd import eval as ev
    ctx = ev.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------- the checker
def bits(x):
    return struct.pack("<d", x)


def make_task(fid, seq0, seq1, rem0=b"", rem1=b"", start=(100, 200), strand=(0, 0), name=("chrA", "chrB"), seq_len=None):
    """What oracle.evaluate and pred.pack_tasks read of a task."""
    return types.SimpleNamespace(fusion_id=fid, seq=[bytes(seq0), bytes(seq1)], remainder=[bytes(rem0), bytes(rem1)], seq_start=list(start),
                                 seq_len=list(seq_len or (len(seq0), len(seq1))), seq_strand=list(strand), ref_name=list(name), strand=list(strand))


def rec(fid, first, second, score=10, left=30, right=46):
    return (fid, 0, 0, 0, first, second, left, right, score, 0)


def records_of(rows):
    from defuse_amd import dsa
    return np.array([tuple(r) for r in rows], dtype=dsa.RECORD_DTYPE).reshape(-1)


def expected(tasks, records):
    """Per maximal run of equal fusion ids: dict(fusion_id, status, seq, break_pos, count, pos_avg, min_avg).  seq is None for
    a group without a sequence; the averages are None for a group whose statistics are the caller's."""
    from oracle import dosplitalign_oracle as ora
    cols = [records[k].tolist() for k in records.dtype.names[:9]]
    rows = list(zip(*cols))
    out, k = [], 0
    while k < len(rows):
        e = k
        while e < len(rows) and rows[e][0] == rows[k][0]:
            e += 1
        group, k = rows[k:e], e
        fid = group[0][0]
        sums = {}
        for r in group:
            sums[(r[4], r[5])] = sums.get((r[4], r[5]), 0) + r[8]
        g = dict(fusion_id=fid, status=0, seq=None, break_pos=(0, 0), count=0, pos_avg=None, min_avg=None)
        if max(sums.values()) <= -1:
            g["status"] |= NO_SPLIT
        if fid not in tasks:
            g["status"] |= NO_TASK
        if g["status"] == 0 or g["status"] == NO_TASK:
            best = min((s for s in sums if sums[s] == max(sums.values())))        # ascending keys, strict '>'
            kept = [r for r in group if (r[4], r[5]) == best]
            g["count"] = len(kept)
            flagged = any(r[6] + r[7] - 8 <= 1 for r in kept)
            if flagged:
                g["status"] |= HOST_STATS
        if (g["status"] & ~HOST_STATS) == 0:
            t = tasks[fid]
            first, cut = best[0], best[1] + 1
            if first < 0 or first > len(t.seq[0]) or cut < 0 or cut >= len(t.seq[1]):      # the two DebugChecks, on the strings
                g["status"] |= OUT_OF_WINDOW
            else:
                safe = [r[:6] + (30, 46) + r[8:] for r in group] if flagged else group      # (the oracle divides by zero there)
                p = ora.evaluate(t, safe)
                assert p["count"] == g["count"] and (p["kept"][0][4], p["kept"][0][5]) == best
                g.update(seq=p["seq"], break_pos=p["break_pos"])
                if not flagged:
                    g.update(pos_avg=p["pos_avg"], min_avg=p["min_avg"])
        out.append(g)
    return out


def check(res, seq, exp):
    """Every result row and the whole of seq_bytes against `exp`."""
    assert len(res) == len(exp)
    R = {k: res[k].tolist() for k in res.dtype.names}
    off = 0
    for k, g in enumerate(exp):
        assert (R["fusion_id"][k], R["status"][k], R["count"][k], R["seq_off"][k]) == (g["fusion_id"], g["status"], g["count"], off), (k, g)
        if g["seq"] is None:
            assert R["seq_len"][k] == 0, k
            continue
        assert R["seq_len"][k] == len(g["seq"]) and tuple(R["break_pos"][k]) == tuple(g["break_pos"]), (k, g, R["break_pos"][k])
        off += len(g["seq"])
        if g["pos_avg"] is not None:
            assert (bits(R["pos_avg"][k]), bits(R["min_avg"][k])) == (bits(g["pos_avg"]), bits(g["min_avg"])), (k, g)
    want = b"".join(g["seq"] for g in exp if g["seq"] is not None)
    assert len(seq) == len(want) == off
    assert seq.tobytes() == want


def predict_both(P, ectx, records, exp=None, tasks=None):
    """eval_groups -> pred_predict and eval_groups_device -> pred_predict_resident on `records`: both checked against the
    oracle and equal to each other as whole arrays.  Returns (groups, results, seq_bytes)."""
    from tests.test_batch_assembly import DeviceArray
    tasks = tasks if tasks is not None else P.oracle_tasks
    exp = expected(tasks, records) if exp is None else exp
    groups, _ = ectx.evaluate(records)
    v = P.predict(groups)
    assert v.n_results == len(exp) and v.results and v.seq_bytes
    res, seq = P.fetch()
    check(res, seq, exp)
    assert v.seq_bytes_len == len(seq) == P.timing()["seq_bytes"] and P.timing()["n_groups"] == len(exp)
    with DeviceArray(records) as dev:
        groups2, _ = ectx.evaluate_device(dev.ptr, len(records))
    P.predict(groups[:0])                                                       # nothing of the first call is left to find
    P.predict_resident(ectx)
    res2, seq2 = P.fetch()
    assert groups2.tobytes() == groups.tobytes() and res2.tobytes() == res.tobytes() and seq2.tobytes() == seq.tobytes()
    assert P.timing()["upload_ms"] == 0
    return groups, res, seq


class Store:
    """bat.Windows, pred.Tasks and a pred.Context over oracle-style tasks.  `gaps`: filler bytes in front of each window in
    the pool (two per task), so that windows begin at chosen byte phases."""

    def __init__(self, bat, pred, tasks, gaps=None):
        from defuse_amd import dsa
        self.oracle_tasks = {t.fusion_id: t for t in tasks}
        pool, fus = bytearray(), np.zeros(len(tasks), dtype=dsa.FUSION_DTYPE)
        for k, t in enumerate(tasks):
            offs = []
            for e in (0, 1):
                pool += b"#" * (gaps[2 * k + e] if gaps is not None else 0)
                offs.append(len(pool))
                pool += t.seq[e]
            fus[k] = (t.fusion_id, offs[0], len(t.seq[0]), offs[1], len(t.seq[1]))
        self.fusions = fus
        self.windows = bat.Windows(np.frombuffer(bytes(pool), dtype=np.uint8), fus)
        self.tasks = pred.Tasks.from_oracle(self.windows, tasks)
        self.ctx = pred.Context(self.tasks)
        for name in ("predict", "predict_resident", "fetch", "view", "timing"):
            setattr(self, name, getattr(self.ctx, name))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()
        self.tasks.close()
        self.windows.close()


# ---------------------------------------------------------------------------------------------- without a GPU
def test_pred_header_and_binding_agree(pred):
    """sizeof and offsetof of every struct of the header, as g++ and gcc -std=c99 see them, against the ctypes structs and the
    numpy dtypes; the PRED_* values; every declared function bound and exported."""
    sizes, n = abi.check("defuse_pred.h", pred, r"pred_[a-z_]+", constants={"PRED_NO_TASK": pred.NO_TASK, "PRED_OUT_OF_WINDOW": pred.OUT_OF_WINDOW},
                         dtypes=[(pred.Task, pred.TASK_DTYPE), (pred.Result, pred.RESULT_DTYPE)])
    assert (pred.NO_TASK, pred.OUT_OF_WINDOW) == (4, 8)
    assert sizes == [56, 56, 40, 40] and n == 10
    assert pred.TASK_DTYPE.itemsize == pred.RESULT_DTYPE.itemsize == 56
    assert (ctypes.sizeof(pred.View), ctypes.sizeof(pred.PredTiming)) == (40, 40)


def test_pred_argument_errors_need_no_device(pred):
    from defuse_amd import eval as ev
    lib = pred.lib()
    err = lambda: lib.pred_last_error().decode()
    h = ctypes.c_void_p()
    one = ctypes.c_void_p(1)           # stands for an object: the argument errors are found before any is looked at
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)

    def task(fid=5, start=(1, 1), length=(4, 4), strand=(0, 1), rem_len=(2, 3), rem_off=(0, 2)):
        t = np.zeros(1, dtype=pred.TASK_DTYPE)
        t["fusion_id"], t["seq_start"], t["seq_len"], t["seq_strand"], t["rem_len"], t["rem_off"] = fid, start, length, strand, rem_len, rem_off
        return t

    def create(tasks, n=None, nbytes=len(data), windows=one, out=h, device=0):
        t = np.concatenate(tasks) if tasks else np.zeros(0, dtype=pred.TASK_DTYPE)
        return lib.pred_tasks_create(device, windows, data.ctypes.data if nbytes else None, nbytes, t.ctypes.data if len(t) else None,
                                     len(t) if n is None else n, ctypes.byref(out) if out is not None else None)
    good = task()
    assert create([good], out=None) == E_ARG
    assert create([good], n=-1) == E_ARG and "negative" in err()
    assert create([good], nbytes=-1) == E_ARG and "negative" in err()
    assert create([], n=1) == E_ARG and "null" in err()
    assert create([task(rem_len=(0, 0))], nbytes=0, windows=None) == E_ARG and "no windows" in err()
    assert create([], n=2 ** 31) == E_LIMIT
    assert create([good, task(6, strand=(0, 2))]) == E_ARG and "task 1" in err() and "seq_strand[1]" in err()
    assert create([task(strand=(-1, 0))]) == E_ARG and "task 0" in err() and "seq_strand[0]" in err()
    assert create([good, task(6), task(7, rem_len=(2, -3))]) == E_ARG and "task 2" in err() and "negative length" in err() and "rem_len[1]" in err()
    assert create([task(rem_len=(-1, 0))]) == E_ARG and "task 0" in err() and "negative length" in err()
    assert create([good, task(6, rem_off=(0, 8))]) == E_ARG and "task 1" in err() and "remainder 1" in err() and "outside" in err()   # one byte beyond
    assert create([task(rem_off=(-1, 0))]) == E_ARG and "remainder 0" in err()
    assert create([task(rem_off=(11, 0), rem_len=(0, 0))]) == E_ARG and "outside" in err()
    assert create([task(rem_off=(2 ** 62, 0), rem_len=(2 ** 31 - 1, 0))]) == E_ARG and "outside" in err()      # no overflow of off + len
    assert create([good, task(6), task(5, start=(9, 9))]) == E_ARG and "fusion_id 5" in err() and "tasks 0 and 2" in err()
    assert create([task(-1), task(2 ** 31 - 1), task(-1)]) == E_ARG and "fusion_id -1" in err()
    assert create([good], device=999, windows=one) == E_DEVICE and "999" in err()          # (the windows are not looked at before the device)
    assert not h

    g = np.zeros(2, dtype=ev.GROUP_DTYPE)
    assert lib.pred_create(0, None) == E_ARG
    assert lib.pred_create(999, ctypes.byref(h)) == E_DEVICE and "999" in err() and not h
    assert lib.pred_create(-1, ctypes.byref(h)) == E_DEVICE and not h
    assert lib.pred_predict(None, one, g.ctypes.data, 2) == E_ARG and "no ctx" in err()
    assert lib.pred_predict(one, None, g.ctypes.data, 2) == E_ARG and "no tasks" in err()
    assert lib.pred_predict_resident(None, one, one) == E_ARG and "no ctx" in err()
    assert lib.pred_predict_resident(one, None, one) == E_ARG and "no tasks" in err()
    assert lib.pred_predict_resident(one, one, None) == E_ARG and "no eval ctx" in err()
    view, timing = pred.View(), pred.PredTiming()
    assert lib.pred_view(None, ctypes.byref(view)) == E_ARG and lib.pred_get_timing(None, ctypes.byref(timing)) == E_ARG
    assert lib.pred_fetch(None, None, 0, None, 0) == E_ARG
    lib.pred_destroy(None)
    lib.pred_tasks_destroy(None)
    # good arguments get as far as the device: no CPU path
    rc = lib.pred_create(0, ctypes.byref(h))
    assert rc in (0, E_DEVICE)
    if rc == 0:
        view.n_results = -1
        assert lib.pred_predict(h, one, g.ctypes.data, -1) == E_ARG and "negative" in err()
        assert lib.pred_view(h, ctypes.byref(view)) == 0 and view.n_results == 0 and lib.pred_view(h, None) == E_ARG
        assert lib.pred_fetch(h, None, -1, None, 0) == E_ARG and lib.pred_fetch(h, None, 1, None, 0) == E_ARG
        lib.pred_destroy(h)
    else:
        assert not h and "device" in err()


# ---------------------------------------------------------------------------------------------- GPU: by hand
def text(rng, n):
    alphabet = np.frombuffer(ODD_BYTES, dtype=np.uint8)
    return alphabet[rng.integers(0, len(alphabet), size=int(n))].tobytes()


@pytest.mark.gpu
def test_word_edges_of_the_sequence_gather(bat, pred, ectx):
    """Remainders of 0-5 bytes, left parts of 0-5 bytes and the whole window, right parts of 1-5 bytes, one task per
    combination; windows at every byte phase of the pool, remainders at every phase of theirs, and - the groups shuffled -
    every part beginning at every phase of the output.  One stray or missing edge byte anywhere breaks the equality of the
    whole of seq_bytes."""
    rng = np.random.default_rng(5)
    tasks, specs = [], []
    for rem0 in range(6):
        for rem1 in range(6):
            for f in (0, 1, 2, 3, 4, 5, -1):
                for right in range(1, 6):
                    len0, len1 = int(rng.integers(5, 10)), int(rng.integers(right, right + 8))
                    fid = 1000 + len(tasks)
                    tasks.append(make_task(fid, text(rng, len0), text(rng, len1), text(rng, rem0), text(rng, rem1)))
                    specs.append((fid, len0 if f < 0 else f, len1 - right - 1))
    gaps = rng.integers(0, 4, 2 * len(tasks)).tolist()
    order = rng.permutation(len(specs))
    records = records_of([rec(*specs[i]) for i in order])
    assert len(tasks) == 6 * 6 * 7 * 5
    with Store(bat, pred, tasks, gaps) as P:
        assert {int(o) % 4 for o in P.fusions["ref0_off"]} == {0, 1, 2, 3} == {int(o) % 4 for o in P.fusions["ref1_off"]}
        groups, res, seq = predict_both(P, ectx, records)
        # every part is empty somewhere and begins at every phase of the output somewhere
        phases = {name: set() for name in ("rem0", "left", "bar", "right", "rem1")}
        for r, i in zip(res, order):
            t, (_, first, second) = tasks[i], specs[i]
            o = int(r["seq_off"])
            lens = (len(t.remainder[0]), first, 1, t.seq_len[1] - second - 1, len(t.remainder[1]))
            assert sum(lens) == r["seq_len"]
            for name, n in zip(phases, lens):
                if n:
                    phases[name].add(o % 4)
                o += n
        assert all(p == {0, 1, 2, 3} for p in phases.values()), phases
        assert (res["status"] == 0).all() and len(seq) == int(res["seq_len"].sum()) > 10000
        # each part empty in turn, alone and together, on one task (the right part always has a byte: second + 1 < seq_len[1])
        t = make_task(7, b"ACGTN", b"acgtn")
        e = make_task(8, b"", b"g", b"", b"")
        r = make_task(9, b"", b"t", b"AC", b"GTN")
        with Store(bat, pred, [t, e, r]) as Q:
            _, res, seq = predict_both(Q, ectx, records_of([rec(7, 0, 3), rec(8, 0, -1), rec(7, 5, -1), rec(9, 0, -1), rec(7, 0, -1), rec(8, 0, -1)]))
            assert seq.tobytes() == b"|n" + b"|g" + b"ACGTN|acgtn" + b"AC|tGTN" + b"|acgtn" + b"|g"


@pytest.mark.gpu
def test_break_positions(bat, pred, ectx):
    """The four strand combinations; a window clipped at the start of its sequence (seq_start 1, shorter than asked);
    first = 0 and second + 1 = seq_len[1] - 1, the two ends of what the DebugChecks allow; first = seq_len[0]."""
    rng = np.random.default_rng(9)
    tasks = []
    for k, strand in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        tasks.append(make_task(10 + k, text(rng, 61), text(rng, 47), text(rng, 3), text(rng, 2), start=(1000 + k, 5000 + k), strand=strand))
        tasks.append(make_task(20 + k, text(rng, 33), text(rng, 90), b"", text(rng, 7), start=(1, 1), strand=strand))        # clipped at the start
    splits = lambda t: ((0, t.seq_len[1] - 2), (t.seq_len[0], -1), (17, 5), (1, 0))
    rows = [(t.fusion_id,) + splits(t)[pick] for pick in range(4) for t in tasks]       # (no two neighbours with one id: they would be one group)
    with Store(bat, pred, tasks) as P:
        _, res, _ = predict_both(P, ectx, records_of([rec(*r) for r in rows]))
    assert (res["status"] == 0).all() and len(res) == 32
    # by hand, from the header: plus start + first - 1 / start + second + 1, minus start + len - first / start + len - second - 2
    for row, (fid, first, second) in zip(res, rows):
        t = P.oracle_tasks[fid]
        bp0 = t.seq_start[0] + first - 1 if t.seq_strand[0] == 0 else t.seq_start[0] + t.seq_len[0] - first
        bp1 = t.seq_start[1] + second + 1 if t.seq_strand[1] == 0 else t.seq_start[1] + t.seq_len[1] - second - 2
        assert row["break_pos"].tolist() == [bp0, bp1], (fid, first, second)
    assert rows[0] == (10, 0, 45) and res["break_pos"][0].tolist() == [999, 5046]           # plus, plus
    assert rows[1] == (20, 0, 88) and res["break_pos"][1].tolist() == [0, 90]               # clipped at 1
    assert rows[-1] == (23, 1, 0) and res["break_pos"][-1].tolist() == [33, 89]             # minus, minus, clipped


@pytest.mark.gpu
def test_status_rules(bat, pred, ectx):
    tasks = [make_task(10, b"ACGTACGTAC", b"ttttgggg", b"NN", b"n"), make_task(20, b"GATTACA", b"catcat", b"", b"*."),
             make_task(30, b"CCCCC", b"aaaaaaaaaaaa", b"\x00\xff", b""),
             # a window asked for with a negative length: FastaIndex::Get leaves the length as it is and the string empty
             make_task(40, b"", b"acgt", b"ACG", b"T", start=(5000, 7), strand=(1, 0), seq_len=(-939, 4))]
    rows = [rec(10, 3, 2), rec(10, 3, 2),
            rec(20, 1, 1, score=-3),                              # EVAL_NO_SPLIT
            rec(30, 5, 0),
            rec(99, 1, 1), rec(99, 1, 1),                         # no task
            rec(10, 10, 6),
            rec(20, -1, 2),                                       # first < 0
            rec(30, 0, 10),
            rec(20, 8, 2),                                        # first > seq_len[0]
            rec(10, 0, -1),
            rec(30, 2, -2),                                       # second + 1 < 0
            rec(20, 7, 4),
            rec(10, 2, 7),                                        # second + 1 >= seq_len[1]
            rec(30, 1, 1),
            rec(20, 2, 2, left=4, right=5), rec(20, 2, 2),        # EVAL_HOST_STATS: sequence and positions, no averages
            rec(10, 1, 1),
            rec(98, 1, 1, score=-1),                              # no task and no split
            rec(30, 4, 3),
            rec(20, -2 ** 31, 2 ** 31 - 1),                       # the far corners of the coordinates
            rec(10, 2 ** 31 - 1, -2 ** 31),
            rec(40, 1, 1),                                        # first > the empty window
            rec(30, 3, 3),
            rec(40, 0, 1)]                                        # the break position comes from the negative length
    records = records_of(rows)
    exp = expected({t.fusion_id: t for t in tasks}, records)
    assert [g["status"] for g in exp] == [0, NO_SPLIT, 0, NO_TASK, 0, OUT_OF_WINDOW, 0, OUT_OF_WINDOW, 0, OUT_OF_WINDOW, 0, OUT_OF_WINDOW, 0,
                                           HOST_STATS, 0, NO_SPLIT | NO_TASK, 0, OUT_OF_WINDOW, OUT_OF_WINDOW, OUT_OF_WINDOW, 0, 0]
    assert exp[-1]["seq"] == b"ACG|gtT" and exp[-1]["break_pos"] == (5000 - 939, 7 + 2)
    assert exp[13]["seq"] == b"GA|cat*." and exp[13]["pos_avg"] is None and exp[0]["seq"] == b"NNACG|tggggn"
    with Store(bat, pred, tasks) as P:
        groups, res, seq = predict_both(P, ectx, records, exp)
        # the neighbours are unaffected and the offsets stay contiguous: the same groups without the refused ones
        keep = [k for k, g in enumerate(exp) if g["seq"] is not None]
        assert len(keep) == 12
        P.predict(groups[keep])
        res2, seq2 = P.fetch()
        assert seq2.tobytes() == seq.tobytes() and res2["seq_off"].tolist() == res["seq_off"][keep].tolist()
        assert res2["seq_len"].tolist() == res["seq_len"][keep].tolist()
        # a group without a sequence has zeros in the fields that mean nothing
        for k, g in enumerate(exp):
            if g["seq"] is None:
                assert (res["seq_len"][k], res["break_pos"][k].tolist(), res["pos_avg"][k], res["min_avg"][k]) == (0, [0, 0], 0.0, 0.0)
        # a fusion_id the windows do not have, and a seq_len that is not its window's
        extra = make_task(77, b"AC", b"GT")
        with pytest.raises(pred.PredError) as e:
            pred.Tasks.from_oracle(P.windows, tasks + [extra])
        assert e.value.code == E_ARG and "task 4" in str(e.value) and "fusion_id 77" in str(e.value)
        wrong = make_task(20, b"GATTACA", b"catca")
        with pytest.raises(pred.PredError) as e:
            pred.Tasks.from_oracle(P.windows, [tasks[0], wrong])
        assert e.value.code == E_ARG and "task 1" in str(e.value) and "seq_len" in str(e.value)
        # a store of some of the windows' tasks, and an empty one
        with pred.Tasks.from_oracle(P.windows, tasks[1:2]) as some, pred.Tasks.from_oracle(P.windows, []) as none:
            P.predict(groups, tasks=some)
            check(*P.fetch(), expected({20: tasks[1]}, records))
            P.predict(groups, tasks=none)
            res3, seq3 = P.fetch()
            assert len(seq3) == 0 and (res3["status"] & NO_TASK).all() and res3["count"].tolist() == res["count"].tolist()


# ---------------------------------------------------------------------------------------------- GPU: random
def random_case(seed, n_tasks=2000):
    """n_tasks tasks with windows of 1-700 bases and remainders of 0-300 (half of them none); per group 1-8 records on a
    few splits, mostly inside the windows, with few distinct scores (ties); about 3 % of the groups name no task, some
    have no split, some a kept record that flags the statistics."""
    rng = np.random.default_rng(seed)
    fids = rng.choice(10 ** 6, size=n_tasks + 60, replace=False)
    tasks = []
    for fid in fids[:n_tasks].tolist():
        rem = [int(rng.integers(0, 301)) if rng.random() < 0.5 else 0 for _ in (0, 1)]
        tasks.append(make_task(fid, text(rng, rng.integers(1, 701)), text(rng, rng.integers(1, 701)), text(rng, rem[0]), text(rng, rem[1]),
                               start=(int(rng.integers(1, 10 ** 6)), int(rng.integers(1, 10 ** 6))), strand=(int(rng.integers(0, 2)), int(rng.integers(0, 2)))))
    rows = []
    for i in rng.permutation(n_tasks + 60).tolist():
        fid = int(fids[i])
        l0, l1 = (tasks[i].seq_len if i < n_tasks else (50, 50))
        firsts = rng.integers(-1, l0 + 2, 3)
        seconds = rng.integers(-2, l1 + 1, 2)
        for _ in range(int(rng.integers(1, 9))):
            left = int(rng.integers(0, 77)) if rng.random() > 0.01 else 4
            right = 76 - left if left != 4 else 5
            rows.append(rec(fid, int(rng.choice(firsts)), int(rng.choice(seconds)), score=int(rng.choice((8, 9, 9, 30, -40))), left=left, right=right))
    return tasks, records_of(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_against_the_oracle(bat, pred, ectx, seed):
    tasks, records = random_case(seed)
    gaps = np.random.default_rng(seed).integers(0, 4, 2 * len(tasks)).tolist()
    with Store(bat, pred, tasks, gaps) as P:
        exp = expected(P.oracle_tasks, records)
        status = [g["status"] for g in exp]
        assert len(exp) == 2060 and status.count(0) > 1000 and sum(1 for s in status if s & NO_TASK) == 60
        assert status.count(OUT_OF_WINDOW) > 20 and status.count(NO_SPLIT) > 20 and status.count(HOST_STATS) > 3
        _, res, seq = predict_both(P, ectx, records, exp)
        assert len(seq) > 500000


@pytest.mark.gpu
def test_context_reuse_and_capacities(bat, pred, ectx):
    from defuse_amd import dsa
    from defuse_amd import eval as ev
    tasks, records = random_case(4, n_tasks=300)
    fid = records["fusion_id"]
    heads = np.flatnonzero(np.concatenate(([True], fid[1:] != fid[:-1])))
    cut = lambda a, b: records[heads[a]:heads[b]]
    with Store(bat, pred, tasks) as P:
        # growing, then shrinking, then nothing: nothing of an earlier call may show
        for part in (cut(0, 20), cut(20, 200), cut(0, 359), cut(100, 103), records[:0], cut(5, 6)):
            predict_both(P, ectx, part)
        lib, h = P.ctx._lib, P.ctx.handle
        groups, _ = ectx.evaluate(cut(0, 50))
        P.predict(groups)
        res, seq = P.fetch()
        # the capacity protocol of pred_fetch: nothing is written when either does not fit
        r2, s2 = np.zeros(len(res), pred.RESULT_DTYPE), np.full(len(seq), 7, np.uint8)
        assert lib.pred_fetch(h, r2.ctypes.data, len(res) - 1, s2.ctypes.data, len(seq)) == E_CAPACITY
        assert str(len(res)) in lib.pred_last_error().decode() and str(len(seq)) in lib.pred_last_error().decode()
        assert lib.pred_fetch(h, r2.ctypes.data, len(res), s2.ctypes.data, len(seq) - 1) == E_CAPACITY
        assert lib.pred_fetch(h, None, 0, None, 0) == E_CAPACITY
        assert not r2.view(np.uint8).any() and (s2 == 7).all()
        assert lib.pred_fetch(h, r2.ctypes.data, len(res), None, len(seq)) == E_ARG
        assert lib.pred_fetch(h, r2.ctypes.data, len(res), s2.ctypes.data, len(seq)) == 0
        assert r2.tobytes() == res.tobytes() and s2.tobytes() == seq.tobytes() and P.timing()["download_ms"] > 0
        P.predict(groups[:0])
        assert lib.pred_fetch(h, None, 0, None, 0) == 0                      # empty results: both buffers may be NULL
        # pred_predict_resident needs a completed evaluation in the eval ctx
        def refused(e):
            with pytest.raises(pred.PredError) as err:
                P.predict_resident(e)
            assert err.value.code == E_ARG and "completed evaluation" in str(err.value)
            assert P.view().n_results == 0
        with ev.Context(0) as fresh:
            refused(fresh)
            fresh.evaluate(cut(0, 3))
            P.predict_resident(fresh)
            check(*P.fetch(), expected(P.oracle_tasks, cut(0, 3)))
            with pytest.raises(dsa.DsaError) as err:                         # refused for capacity
                fresh.evaluate(cut(0, 3), group_cap=2, kept_cap=100)
            assert err.value.code == E_CAPACITY
            refused(fresh)
            fresh.evaluate(cut(3, 9))
            P.predict_resident(fresh)
            check(*P.fetch(), expected(P.oracle_tasks, cut(3, 9)))
            ng, nk = ctypes.c_int64(), ctypes.c_int64()
            assert fresh.lib.eval_groups(fresh.h, None, -1, None, 0, ctypes.byref(ng), None, 0, ctypes.byref(nk)) == E_ARG      # failed
            refused(fresh)
            big = records_of([rec(1, 1, 1, score=2 ** 31 - 1), rec(1, 1, 1, score=2 ** 31 - 1)])
            with pytest.raises(dsa.DsaError) as err:
                fresh.evaluate(big)
            assert err.value.code == E_LIMIT
            refused(fresh)
            fresh.evaluate(records[:0])                                      # a completed evaluation of nothing
            assert P.predict_resident(fresh).n_results == 0
        predict_both(P, ectx, cut(7, 30))


@pytest.mark.gpu
def test_sequence_total_is_formed_in_64_bits(bat, pred):
    """300 groups that all name one task with a window of 2^24 bases and first = seq_len[0]: 5.03e9 sequence bytes.  The
    offset of the last result and the total pass 2^32; the last sequence, and the one that lies across byte 2^32, are read
    back from the device alone."""
    from defuse_amd import eval as ev
    from tests.test_batch_assembly import from_device
    n0, n_groups = 2 ** 24, 300
    rng = np.random.default_rng(3)
    w0 = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n0)].tobytes()
    t = make_task(5, w0, b"acgtn", b"NN", b"n.")
    groups = np.zeros(n_groups, dtype=ev.GROUP_DTYPE)
    groups["fusion_id"], groups["best_first"], groups["best_second"], groups["count"] = 5, n0, 1, 3
    groups["pos_sum"], groups["min_sum"] = 1.0, 2.0
    want = b"NN" + w0 + b"|gtnn."
    with Store(bat, pred, [t]) as P:
        try:
            v = P.predict(groups)
        except pred.PredError as e:
            if not (e.code == E_DEVICE and "memory" in str(e).lower()):
                raise
            pytest.skip("the device refused %d sequence bytes: %s" % (n_groups * len(want), e))
        assert v.n_results == n_groups and v.seq_bytes_len == n_groups * len(want) > 2 ** 32
        print("%d sequence bytes: the gathers took %.1f ms" % (v.seq_bytes_len, P.timing()["gather_ms"]))
        res = from_device(v.results, n_groups, pred.RESULT_DTYPE)
        assert res["seq_off"].tolist() == [k * len(want) for k in range(n_groups)] and res["seq_off"][-1] > 2 ** 32
        assert (res["seq_len"] == len(want)).all() and (res["status"] == 0).all()
        assert bits(res["pos_avg"][7]) == bits(1.0 / 3.0) and bits(res["min_avg"][7]) == bits(2.0 / 3.0)
        across = 2 ** 32 // len(want)
        assert res["seq_off"][across] < 2 ** 32 < res["seq_off"][across] + len(want)
        for k in (n_groups - 1, across, 0):
            got = from_device(v.seq_bytes + int(res["seq_off"][k]), len(want), np.uint8)
            assert got.tobytes() == want, k


# ---------------------------------------------------------------------------------------------- GPU: the chains
@pytest.mark.gpu
def test_smoke_vector_through_the_whole_resident_chain(bat, pred, gpu_ctx, ectx):
    """SAM records up; candidates, batch, DP records and groups stay on the device; the break positions come down.  Set up
    as test_batch_assembly.test_smoke_vector_resident_chain."""
    from defuse_amd import cand
    from oracle import dosplitalign_oracle as ora
    from tests.test_batch_assembly import DeviceArray
    d = SMOKE + "/"
    tasks = ora.create_tasks(d + "ref.fa", d + "exons.txt", 300, 30, 50, 50, ora.read_align_region_pairs(d + "regions.txt"))
    reads = {}
    ora.read_fastq(d + "reads.1.fastq", reads)
    ora.read_fastq(d + "reads.2.fastq", reads)
    names, regs = {}, []
    for t in tasks.values():
        for ce in (0, 1):
            for loc in t.mate_regions[ce]:
                regs.append((names.setdefault(loc["refName"], len(names)), loc["strand"], loc["start"], loc["end"], cand.cluster_id(t.fusion_id, ce)))
    als = cand.alignments([(names.get(rname, -1), strand, start, end, ora.lexical_cast_int(frag), rend)
                           for frag, rend, rname, strand, start, end in ora.sam_alignments(d + "improper.sam")])
    windows = {t.fusion_id: (t.seq[0], t.seq[1]) for t in tasks.values()}
    with cand.Table(cand.regions(regs)) as table, bat.Reads.from_dict(reads) as r, bat.Windows.from_dict(windows) as w, bat.Batch() as b, \
            pred.Tasks.from_oracle(w, tasks) as ptasks, pred.Context(ptasks) as P, table.session() as s:
        ptr, n = s.enumerate_device(als, cand.ORDER_FUSION)
        gpu_ctx.upload_device(b.assemble_device(r, w, ptr, n))
        n_rec = gpu_ctx.run()
        with DeviceArray(np.zeros(n_rec, dtype=np.dtype("V40"))) as dev:
            assert gpu_ctx.records_to_device(dev.ptr, n_rec) == n_rec
            groups, _ = ectx.evaluate_device(dev.ptr, n_rec)
        P.predict_resident(ectx)
        res, seq = P.fetch()
        assert len(res) == len(groups) == len(tasks) and (res["status"] == 0).all()
        lines = "".join(P.format_break(row, tasks[int(row["fusion_id"])].ref_name, tasks[int(row["fusion_id"])].strand) for row in res)
        assert lines == open(d + "expected.break.txt").read()
        check(res, seq, expected(tasks, gpu_ctx.download()))


@pytest.mark.gpu
def test_config1_derived_chain(bat, pred, ectx, tmp_path):
    from oracle import dosplitalign_oracle as ora
    from tests import config1_case
    case = config1_case.build(str(tmp_path / "case"))
    tasks = ora.create_tasks(case["fasta"], case["exons"], case["ufrag"], case["sfrag"], case["minread"], case["maxread"],
                             ora.read_align_region_pairs(case["regions_derived"]))
    rows = [tuple(int(x) for x in l.split()) for l in open(os.path.join(CONFIG1, "expected.derived.align.txt"))]
    rows.sort(key=lambda r: r[0])                                               # stable, by fusion id: the tool's input
    records = records_of([r + (0,) for r in rows])
    windows = {t.fusion_id: (t.seq[0], t.seq[1]) for t in tasks.values()}
    with bat.Windows.from_dict(windows) as w, pred.Tasks.from_oracle(w, tasks) as ptasks, pred.Context(ptasks) as P:
        P.oracle_tasks = tasks
        _, res, seq = predict_both(P, ectx, records)
        assert len(res) > 0 and (res["status"] == 0).all()
        seq_lines = "".join(P.format_seq(row, seq) for row in res)
        brk_lines = "".join(P.format_break(row, tasks[int(row["fusion_id"])].ref_name, tasks[int(row["fusion_id"])].strand) for row in res)
    assert seq_lines == open(os.path.join(CONFIG1, "expected.derived.seq.txt")).read()
    assert brk_lines == open(os.path.join(CONFIG1, "expected.derived.break.txt")).read()
