"""include/defuse_eval.h: per fusion the best supported breakpoint on the GPU (defuse_amd/csrc/eval_api.hip through
defuse_amd/eval.py), and evalsplitalign's opt-in use of it (DEFUSE_EVAL_GPU=1).

The checker is oracle/dosplitalign_oracle.py: evaluate() per group for the best split, the support and the kept records,
evalsplitalign() for the tool's three files.  The two FP64 sums are compared BIT FOR BIT with a Python loop that adds the same
quotients in the same serial order (a Python float is an IEEE double).  Groups flagged EVAL_HOST_STATS leave their sums out of
that comparison, so the flag is capped: every generated case but the one about the flag uses reads of at least ten bases
and must come back with zero flagged groups."""
import ctypes
import math
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

from tests import abi
from tests import config1_case as c1
from tests import pipeline_case
from tests.eval_case import generated_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL = os.path.join(ROOT, "bin", "evalsplitalign")
HEADER = os.path.join(ROOT, "include", "defuse_eval.h")
DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = -1, -2, -3, -4
NO_GPU = {"DEFUSE_EVAL_GPU": "1", "DEFUSE_GPU": "999"}          # a device ordinal no machine has: the library finds no device


@pytest.fixture(scope="module")
def tools(built):
    from defuse_amd import build
    build.build_tools()
    return True


# ---------------------------------------------------------------------------------------------- the checker
def bits(x):
    return struct.pack("<d", x)


def serial_sums(kept_reads):
    """tools/SplitAlignment.cpp:571-587 over (left, right) in order; None where a range is zero (EVAL_HOST_STATS territory)."""
    pos = mn = 0.0
    for left, right in kept_reads:
        pos_range = float(left + right - 8)
        min_range = float(math.floor(0.5 * float(left + right - 8)))
        if pos_range == 0.0 or min_range == 0.0:
            return None
        pos += float(max(0, left - 4)) / pos_range
        mn += float(max(0, min(left - 4, right - 4))) / min_range
    return pos, mn


def oracle_groups(records):
    """Per maximal run of equal fusion ids: dict(fusion_id, first, n, best, score, kept indices, sums, pos_avg, min_avg) from
    oracle.evaluate on the run; best is None where no split has a sum above -1 (the oracle itself has no such branch)."""
    from oracle import dosplitalign_oracle as ora
    task = types.SimpleNamespace(remainder=(b"", b""), seq=(b"", b""), seq_strand=(ora.PLUS, ora.PLUS), seq_start=(0, 0), seq_len=(0, 0))
    fid = records["fusion_id"]
    n = len(records)
    heads = np.flatnonzero(np.concatenate(([True], fid[1:] != fid[:-1]))) if n else np.zeros(0, np.int64)
    ends = np.concatenate((heads[1:], [n])) if n else heads
    cols = [records[k].tolist() for k in ("ref_first", "ref_second", "read_first", "read_second", "score")]
    fids = fid.tolist()
    out = []
    for a, b in zip(heads.tolist(), ends.tolist()):
        rows = [(fids[i], i, 0, 0, cols[0][i], cols[1][i], cols[2][i], cols[3][i], cols[4][i]) for i in range(a, b)]   # frag = the index
        sums = {}
        for r in rows:
            sums[(r[4], r[5])] = sums.get((r[4], r[5]), 0) + r[8]
        g = dict(fusion_id=fids[a], first=a, n=b - a, best=None, splits=len(sums))
        if max(sums.values()) > -1:
            p = ora.evaluate(task, rows)
            kept = p["kept"]
            g.update(best=(kept[0][4], kept[0][5]), score=sum(r[8] for r in kept), count=p["count"], kept=[r[1] for r in kept],
                     sums=serial_sums([(r[6], r[7]) for r in kept]), pos_avg=p["pos_avg"], min_avg=p["min_avg"])
        out.append(g)
    return out


def check(records, groups, kept, exp=None, flagged_allowed=False):
    """Every field of every group and the whole kept list against the oracle; returns the number of flagged groups."""
    from defuse_amd import eval as ev
    exp = oracle_groups(records) if exp is None else exp
    assert len(groups) == len(exp)
    want_kept = [i for g in exp if g["best"] is not None for i in g["kept"]]
    assert kept.tolist() == want_kept
    off = flagged = 0
    G = {k: groups[k].tolist() for k in groups.dtype.names}
    for k, g in enumerate(exp):
        assert (G["fusion_id"][k], G["first_record"][k], G["n_records"][k]) == (g["fusion_id"], g["first"], g["n"]), k
        if g["best"] is None:
            assert G["status"][k] == ev.NO_SPLIT, k
            continue
        assert (G["best_first"][k], G["best_second"][k]) == g["best"], (k, g)
        assert (G["best_score"][k], G["count"][k], G["kept_off"][k]) == (g["score"], g["count"], off), k
        off += g["count"]
        if g["sums"] is None:
            assert G["status"][k] == ev.HOST_STATS, k
            flagged += 1
            continue
        assert G["status"][k] == 0, k
        assert (bits(G["pos_sum"][k]), bits(G["min_sum"][k])) == (bits(g["sums"][0]), bits(g["sums"][1])), (k, G["pos_sum"][k], g["sums"])
        # what the tool prints: the oracle's averages are these sums over the count
        assert bits(G["pos_sum"][k] / g["count"]) == bits(g["pos_avg"]) and bits(G["min_sum"][k] / g["count"]) == bits(g["min_avg"]), k
    assert flagged_allowed or flagged == 0
    return flagged


def make_records(rng, sizes, ids=None, n_first=5, n_second=3, scores=(8, 9, 10, 30), lq=76):
    """Groups of the given sizes; few distinct splits (some negative) and few distinct scores, so that equal sums are common
    in small groups; reads of lq >= 10 bases."""
    from defuse_amd import dsa
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    r = np.zeros(n, dsa.RECORD_DTYPE)
    ids = np.arange(len(sizes)) * 3 + 7 if ids is None else np.asarray(ids)
    r["fusion_id"] = np.repeat(ids, sizes)
    r["frag"] = np.arange(n) % 1000003
    r["read_end"] = rng.integers(0, 2, n)
    r["revcomp"] = rng.integers(0, 2, n)
    r["ref_first"] = rng.integers(-2, n_first - 2, n) * 37
    r["ref_second"] = rng.integers(-1, n_second - 1, n) * 11
    r["read_first"] = rng.integers(0, lq + 1, n)
    r["read_second"] = lq - r["read_first"]
    r["score"] = rng.choice(np.asarray(scores), n)
    r["pair_idx"] = np.arange(n)
    return r


def rec(fid, first, second, score, left=30, right=46):
    return (fid, 0, 0, 0, first, second, left, right, score, 0)


# ---------------------------------------------------------------------------------------------- CPU
def _c_struct(name):
    """[(field, ctype-name)] of a typedef struct in the header."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(n, t) for t, n in re.findall(r"(int32_t|int64_t|float|double)\s+(\w+);", body)]


def test_header_and_binding_agree(built):
    """eval_group and eval_timing: the binding's fields are the header's, in order, with its types, sizes and offsets; the
    library exports every function the header declares."""
    from defuse_amd import eval as ev
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    for name, struct_ in (("eval_group", ev.EvalGroup), ("eval_timing", ev.EvalTiming)):
        assert [(n, ctype[t]) for n, t in _c_struct(name)] == list(struct_._fields_), name
    sizes, n = abi.check("defuse_eval.h", ev, r"eval_\w+", constants={"EVAL_NO_SPLIT": ev.NO_SPLIT, "EVAL_HOST_STATS": ev.HOST_STATS},
                         dtypes=[(ev.EvalGroup, ev.GROUP_DTYPE)])
    assert sizes == [72, 56] and n == 6
    assert ev.GROUP_DTYPE.itemsize == 72


def test_argument_errors_without_a_device(built):
    from defuse_amd import dsa
    from defuse_amd import eval as ev
    lib = ev.lib()
    h = ctypes.c_void_p()
    devices = [999] + ([0] if lib.dsa_device_count() == 0 else [])
    for d in devices:
        assert lib.eval_create(d, ctypes.byref(h)) == DSA_E_DEVICE and not h.value
        assert len(lib.eval_last_error()) > 0
    with pytest.raises(dsa.DsaError) as e:
        ev.Context(999)
    assert e.value.code == DSA_E_DEVICE
    assert lib.eval_create(0, None) == DSA_E_ARG
    ng, nk = ctypes.c_int64(), ctypes.c_int64()
    r = np.zeros(4, dsa.RECORD_DTYPE)
    for fn in (lib.eval_groups, lib.eval_groups_device):
        assert fn(None, r.ctypes.data, 4, None, 0, ctypes.byref(ng), None, 0, ctypes.byref(nk)) == DSA_E_ARG      # no context
        assert fn(None, r.ctypes.data, -1, None, 0, ctypes.byref(ng), None, 0, ctypes.byref(nk)) == DSA_E_ARG
    assert lib.eval_get_timing(None, None) == DSA_E_ARG
    lib.eval_destroy(None)                                          # a no-op


def config1_align(tmp_path):
    """The config-1 chain's alignment file (the committed golden, sorted by fusion id as the pipeline does) and its case."""
    case = c1.build(str(tmp_path / "config1"))
    rows = sorted(open(os.path.join(c1.DATA, "expected.derived.align.txt")).read().splitlines(True), key=lambda l: int(l.split("\t")[0]))
    assert len(rows) == 41
    align = tmp_path / "config1.sorted.align"
    align.write_text("".join(rows))
    case = dict(case, regions=case["regions_derived"])
    return case, str(align)


def eval_args(case, align, out):
    return ["-f", case["fasta"], "-e", case["exons"], "-u", str(case["ufrag"]), "-s", str(case["sfrag"]),
            "-n", str(case["minread"]), "-x", str(case["maxread"]), "-r", case["regions"], "-a", align,
            "-q", out + ".seq", "-b", out + ".break", "-p", out + ".predalign"]


def run_eval(case, align, out, env=None, tool=EVAL):
    e = {k: v for k, v in os.environ.items() if k != "DEFUSE_EVAL_GPU"}
    e.update(env or {})
    r = subprocess.run([tool] + eval_args(case, align, out), capture_output=True, text=True, env=e, timeout=900, stdin=subprocess.DEVNULL)
    files = tuple(open(out + "." + x).read() if os.path.exists(out + "." + x) else None for x in ("seq", "break", "predalign"))
    return r, files


def config1_expected():
    return tuple(open(os.path.join(c1.DATA, "expected.derived.%s.txt" % x)).read() for x in ("seq", "break", "predalign"))


def test_tool_with_the_variable_and_no_device(tools, tmp_path):
    """DEFUSE_EVAL_GPU=1 without a usable device: groups to evaluate end the run with an Error line and exit 1; an alignment
    file without lines needs no device and gives three empty files; without the variable the files are today's."""
    case, align = config1_align(tmp_path)
    r, files = run_eval(case, align, str(tmp_path / "host"), env={"DEFUSE_GPU": "999"})
    assert r.returncode == 0 and files == config1_expected(), r.stderr
    r, files = run_eval(case, align, str(tmp_path / "nogpu"), env=NO_GPU)
    assert r.returncode == 1 and r.stderr.startswith("Error: GPU evaluation failed: ") and len(r.stderr.strip().splitlines()) == 1, r.stderr
    empty = tmp_path / "empty.align"
    empty.write_text("")
    r, files = run_eval(case, str(empty), str(tmp_path / "empty"), env=NO_GPU)
    assert (r.returncode, r.stderr, files) == (0, "", ("", "", ""))
    # a malformed first line: nothing to evaluate, the reader's message, and still no device
    bad = tmp_path / "bad.align"
    bad.write_text("short\tline\n" + open(align).read())
    r, files = run_eval(case, str(bad), str(tmp_path / "bad"), env=NO_GPU)
    assert r.returncode == 1 and r.stderr.startswith("Error: Format error for candidate reads line:") and files == ("", "", "")
    assert (r.returncode, r.stderr, files) == run_flat(case, str(bad), str(tmp_path / "bad_host"), {})


def prime(case, tmp_path):
    """One run on an empty alignment file, so that the FASTA index exists and no later run reports building it on stderr."""
    empty = tmp_path / "prime.align"
    empty.write_text("")
    r, files = run_eval(case, str(empty), str(tmp_path / "prime"), env={"DEFUSE_GPU": "999"})
    assert r.returncode == 0 and files == ("", "", ""), r.stderr


def run_flat(case, align, out, env):
    r, files = run_eval(case, align, out, env=env)
    return r.returncode, r.stderr, files


def test_host_code_under_asan(tools, tmp_path):
    """The opt-in path's host stages (parsing into records, the reader's rules about malformed lines, the exit through the
    library's error) and the refactored host evaluator under ASan + UBSan; no GPU is used."""
    from defuse_amd import build
    from tests.test_sanitizers import BAD, ENV
    tool = build.build_sanitized("asan")["evalsplitalign"]
    case, align = config1_align(tmp_path)
    for threads in ("1", "5"):
        r, files = run_eval(case, align, str(tmp_path / "asan"), env=dict(ENV["asan"], DEFUSE_THREADS=threads, DEFUSE_GPU="999"), tool=tool)
        assert not any(b in r.stderr for b in BAD), r.stderr[-3000:]
        assert r.returncode == 0 and files == config1_expected()
        r, files = run_eval(case, align, str(tmp_path / "asan_gpu"), env=dict(ENV["asan"], DEFUSE_THREADS=threads, **NO_GPU), tool=tool)
        assert not any(b in r.stderr for b in BAD), r.stderr[-3000:]
        assert r.returncode == 1 and "Error: GPU evaluation failed: " in r.stderr


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ectx(built):
    from defuse_amd import eval as ev
    ctx = ev.Context(0)                 # raises without a GPU: no fallback
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_group_sizes_against_the_oracle(ectx):
    rng = np.random.default_rng(1)
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 5000] * 3 + [1] * 40 + [2] * 40
    r = make_records(rng, sizes)
    groups, kept = ectx.evaluate(r)
    check(r, groups, kept)
    t = ectx.timing()
    exp = oracle_groups(r)
    assert (t["n_records"], t["n_groups"], t["n_kept"], t["n_flagged"]) == (len(r), len(sizes), len(kept), 0)
    assert t["n_runs"] == sum(g["splits"] for g in exp)
    assert t["device_ms"] > 0 and t["upload_ms"] > 0
    # many splits per group: the run scan over long groups
    r = make_records(rng, [5000, 1, 257, 64], n_first=400, n_second=7, scores=(8, 20, 21, 150))
    check(r, *ectx.evaluate(r))
    assert ectx.timing()["n_flagged"] == 0
    groups, kept = ectx.evaluate(r[:0])                              # n == 0: zero groups
    assert len(groups) == 0 and len(kept) == 0


@pytest.mark.gpu
def test_one_group_of_300000_records(ectx):
    rng = np.random.default_rng(2)
    r = make_records(rng, [300000], n_first=9, n_second=4)
    groups, kept = ectx.evaluate(r)
    assert len(groups) == 1 and groups["count"][0] == len(kept) > 5000
    check(r, groups, kept)
    assert ectx.timing()["n_flagged"] == 0


@pytest.mark.gpu
def test_200000_small_groups(ectx):
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 4, 200000)
    ids = rng.integers(-50, 50, 200000)
    ids[1::2] += 1000                                                # neighbours differ: every run is one group; ids repeat and are unsorted
    r = make_records(rng, sizes, ids=ids, n_first=2, n_second=2, scores=(8, 9))
    groups, kept = ectx.evaluate(r)
    assert len(groups) == 200000
    check(r, groups, kept)
    assert ectx.timing()["n_flagged"] == 0


@pytest.mark.gpu
def test_ties_and_order_by_hand(ectx):
    from defuse_amd import dsa
    from defuse_amd import eval as ev
    big = 2 ** 30
    rows = [
        # group 0 (id 5): two splits with equal sums that differ only in second: the smaller second wins
        rec(5, 10, 7, 20), rec(5, 10, 3, 8), rec(5, 10, 3, 12), rec(5, 10, 9, 19),
        # group 1 (id 6): three splits with equal sums: (-4, 50) < (2, -9) < (2, 0), a negative first beats a positive one
        rec(6, 2, 0, 30), rec(6, 2, -9, 30), rec(6, -4, 50, 10), rec(6, -4, 50, 20),
        # group 2 (id 5 again): a separated run of an id is a group of its own; the larger sum wins whatever the order
        rec(5, 1, 1, 8), rec(5, 0, 0, 9),
        # group 3 (id 9): every sum negative: no split
        rec(9, 3, 3, -5), rec(9, 4, 4, -1), rec(9, 3, 3, -2),
        # group 4 (id 10): a sum of exactly -1 is not above -1 either, but 0 is
        rec(10, 8, 8, -1), rec(10, 9, 9, 5), rec(10, 9, 9, -5),
        # group 5 (id 11): a sum of exactly 2^31 - 1
        rec(11, 1, 2, big), rec(11, 1, 2, big - 1), rec(11, 7, 7, 100), rec(11, 1, 2, 0, left=4, right=72),
        # group 6 (id -3): negative ids and a tie between (INT_MIN, 5) and (INT_MAX, 5)
        rec(-3, 2 ** 31 - 1, 5, 40), rec(-3, -2 ** 31, 5, 40),
    ]
    r = np.array(rows, dtype=dsa.RECORD_DTYPE)
    groups, kept = ectx.evaluate(r)
    check(r, groups, kept)
    assert groups["fusion_id"].tolist() == [5, 6, 5, 9, 10, 11, -3]
    assert list(zip(groups["best_first"].tolist(), groups["best_second"].tolist()))[:3] == [(10, 3), (-4, 50), (0, 0)]
    assert groups["status"].tolist() == [0, 0, 0, ev.NO_SPLIT, 0, 0, 0]
    assert (groups["best_first"][4], groups["best_score"][4], groups["count"][4]) == (9, 0, 2)
    assert (groups["best_score"][5], groups["count"][5]) == (2 ** 31 - 1, 3)
    assert (groups["best_first"][6], groups["best_second"][6]) == (-2 ** 31, 5)
    assert kept.tolist() == [1, 2, 6, 7, 9, 14, 15, 16, 17, 19, 21]
    assert groups["kept_off"].tolist()[:3] == [0, 2, 4] and groups["n_records"].tolist() == [4, 4, 2, 3, 3, 4, 2]
    # one above 2^31 - 1: the call fails
    over = r.copy()
    over["score"][19] = 1
    with pytest.raises(dsa.DsaError) as e:
        ectx.evaluate(over)
    assert e.value.code == DSA_E_LIMIT
    under = np.array([rec(1, 0, 0, -2 ** 31), rec(1, 0, 0, -1), rec(1, 5, 5, 9)], dtype=dsa.RECORD_DTYPE)
    with pytest.raises(dsa.DsaError) as e:
        ectx.evaluate(under)
    assert e.value.code == DSA_E_LIMIT
    under["score"][1] = 0                                           # exactly INT_MIN is a sum the reference can hold
    groups, kept = ectx.evaluate(under)
    check(under, groups, kept)
    assert (groups["best_first"][0], groups["count"][0], kept.tolist()) == (5, 1, [2])


@pytest.mark.gpu
def test_host_stats_flag(ectx):
    """Kept records with read_first + read_second of 8 and 9 flag exactly their groups; such a record that is not kept does
    not."""
    from defuse_amd import dsa
    from defuse_amd import eval as ev
    rng = np.random.default_rng(4)
    r = make_records(rng, [40, 1, 70, 3, 200, 2, 5])
    g = np.repeat(np.arange(7), [40, 1, 70, 3, 200, 2, 5])
    first = oracle_groups(r)
    kept_of = {k: first[k]["kept"] for k in range(7)}

    def shorten(i, total):
        r["read_first"][i] = total // 2
        r["read_second"][i] = total - total // 2
    shorten(kept_of[0][-1], 8)                                      # group 0: posRange 0
    shorten(kept_of[2][0], 9)                                       # group 2: minRange 0
    not_kept = [i for i in np.flatnonzero(g == 4).tolist() if i not in kept_of[4]]
    shorten(not_kept[0], 8)                                         # group 4: such a record exists but is not kept
    shorten(not_kept[-1], 9)
    shorten(kept_of[6][0], 10)                                      # group 6: ten bases are fine (ranges 2 and 1)
    groups, kept = ectx.evaluate(r)
    flagged = check(r, groups, kept, flagged_allowed=True)
    assert groups["status"].tolist() == [ev.HOST_STATS, 0, ev.HOST_STATS, 0, 0, 0, 0] and flagged == 2
    assert ectx.timing()["n_flagged"] == 2
    assert [first[k]["kept"] for k in range(7)] == [x["kept"] for x in oracle_groups(r)]      # the read splits do not move the choice


@pytest.mark.gpu
def test_capacity_protocol(ectx):
    from defuse_amd import dsa
    rng = np.random.default_rng(5)
    r = make_records(rng, [30, 2, 500, 1])
    exp = oracle_groups(r)
    n_kept = sum(g["count"] for g in exp)
    for gc, kc in ((3, n_kept), (4, n_kept - 1), (0, 0)):
        with pytest.raises(dsa.DsaError) as e:
            ectx.evaluate(r, group_cap=gc, kept_cap=kc)
        assert (e.value.code, e.value.n_groups, e.value.n_kept) == (DSA_E_CAPACITY, 4, n_kept)
    # nothing else is written
    from defuse_amd import eval as ev
    groups = np.full(4, 0x55, np.uint8).repeat(72).view(ev.GROUP_DTYPE)
    keptbuf = np.full(n_kept, -7, np.int64)
    ng, nk = ctypes.c_int64(), ctypes.c_int64()
    rc = ectx.lib.eval_groups(ectx.h, r.ctypes.data, len(r), groups.ctypes.data, 3, ctypes.byref(ng), keptbuf.ctypes.data, n_kept, ctypes.byref(nk))
    assert (rc, ng.value, nk.value) == (DSA_E_CAPACITY, 4, n_kept)
    assert (groups.view(np.uint8) == 0x55).all() and (keptbuf == -7).all()
    # argument errors on a live context: negative n, no records for n > 0, no place for the counts, negative capacities
    lib, h, rp = ectx.lib, ectx.h, r.ctypes.data
    for fn in (lib.eval_groups, lib.eval_groups_device):
        assert fn(h, rp, -1, groups.ctypes.data, 4, ctypes.byref(ng), keptbuf.ctypes.data, n_kept, ctypes.byref(nk)) == DSA_E_ARG
        assert fn(h, None, len(r), groups.ctypes.data, 4, ctypes.byref(ng), keptbuf.ctypes.data, n_kept, ctypes.byref(nk)) == DSA_E_ARG
        assert fn(h, rp, len(r), groups.ctypes.data, 4, None, keptbuf.ctypes.data, n_kept, ctypes.byref(nk)) == DSA_E_ARG
        assert fn(h, rp, len(r), groups.ctypes.data, 4, ctypes.byref(ng), keptbuf.ctypes.data, n_kept, None) == DSA_E_ARG
        assert fn(h, rp, len(r), groups.ctypes.data, -1, ctypes.byref(ng), keptbuf.ctypes.data, n_kept, ctypes.byref(nk)) == DSA_E_ARG
        assert len(lib.eval_last_error()) > 0
    assert lib.eval_groups(h, rp, len(r), None, 4, ctypes.byref(ng), keptbuf.ctypes.data, n_kept, ctypes.byref(nk)) == DSA_E_ARG   # room, but nowhere to put it
    assert (groups.view(np.uint8) == 0x55).all() and (keptbuf == -7).all()
    got = ectx.evaluate(r, group_cap=4, kept_cap=n_kept)           # a second call with room succeeds
    check(r, *got, exp=exp)
    check(r, *ectx.evaluate(r, group_cap=100, kept_cap=len(r)), exp=exp)


@pytest.mark.gpu
def test_deterministic(ectx):
    rng = np.random.default_rng(6)
    r = make_records(rng, rng.integers(1, 400, 3000))
    a = ectx.evaluate(r)
    b = ectx.evaluate(r)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) == 3000


def _hip_runtime():
    """The HIP runtime the library has loaded, for a device allocation of the test's own."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


@pytest.mark.gpu
def test_resident_records_of_the_headline_batch(gpu_ctx, ectx):
    """BASELINE configs[1] (10k fusions x 100 reads, 2x76) through dsa_upload / dsa_plan / dsa_run; the records go on with
    dsa_copy_records_device and are evaluated from the device pointer: all groups against the oracle on the downloaded
    records, and the host-pointer entry gives identical bytes."""
    from defuse_amd import synth
    ref, fus, reads, pairs = synth.make_batch(10000, 100, lq=76, lr=389, seed=2)
    gpu_ctx.upload(ref, fus, reads, pairs)
    gpu_ctx.plan()
    n = gpu_ctx.run()
    assert n > 1_500_000
    hip = _hip_runtime()
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), n * 40) == 0
    try:
        assert gpu_ctx.records_to_device(dev.value, n) == n
        groups, kept = ectx.evaluate_device(dev.value, n)
        t = ectx.timing()
    finally:
        assert hip.hipFree(dev) == 0
    assert t["upload_ms"] == 0 and t["n_records"] == n and t["n_flagged"] == 0
    got = gpu_ctx.download()
    assert len(got) == n and len(groups) == 10000
    check(got, groups, kept)
    host = ectx.evaluate(got)
    assert host[0].tobytes() == groups.tobytes() and host[1].tobytes() == kept.tobytes()
    print("resident batch: %d records, %d groups, %d splits, %d kept; device %.3f ms" % (n, len(groups), t["n_runs"], len(kept), t["device_ms"]))


def oracle_files(case, align):
    from oracle import dosplitalign_oracle as ora
    return tuple(ora.evalsplitalign(case["fasta"], case["exons"], case["ufrag"], case["sfrag"], case["minread"], case["maxread"], case["regions"], align))


@pytest.mark.gpu
def test_tool_on_the_config1_chain(tools, tmp_path):
    case, align = config1_align(tmp_path)
    prime(case, tmp_path)
    exp = config1_expected()
    assert oracle_files(case, align) == exp
    for threads in ("1", "16"):
        host = run_flat(case, align, str(tmp_path / ("host" + threads)), {"DEFUSE_THREADS": threads})
        gpu = run_flat(case, align, str(tmp_path / ("gpu" + threads)), {"DEFUSE_THREADS": threads, "DEFUSE_EVAL_GPU": "1"})
        assert (host[0], host[2]) == (0, exp) and gpu == host, threads
    # the variable really routes into the library: its timing line names the 41 records, the groups and the kept lines, and only with the variable
    timed = run_flat(case, align, str(tmp_path / "timed"), {"DEFUSE_TIMING": "1", "DEFUSE_EVAL_GPU": "1"})
    assert timed[0] == 0 and timed[2] == exp and "[evalsplitalign] eval gpu:" in timed[1] and " 41 records, %d groups, " % (len(exp[1].splitlines()) // 2) in timed[1] \
        and " %d kept, 0 flagged" % len(exp[2].splitlines()) in timed[1], timed[1]
    plain = run_flat(case, align, str(tmp_path / "timed_host"), {"DEFUSE_TIMING": "1"})
    assert plain[0] == 0 and "eval gpu" not in plain[1] and "parse+evaluate" in plain[1]


@pytest.mark.gpu
def test_tool_on_a_generated_file(tools, tmp_path):
    """At least 500 k lines: the files with DEFUSE_EVAL_GPU=1 are the host path's and the oracle's, on 1 and on 16 threads."""
    case, lines = generated_case(tmp_path, 2700)
    prime(case, tmp_path)
    assert len(lines) >= 500_000
    align = str(tmp_path / "big.align")
    open(align, "w").write("".join(lines))
    exp = oracle_files(case, align)
    assert len(exp[1].splitlines()) == 2 * len(lines) // 2700
    for threads in ("1", "16"):
        host = run_flat(case, align, str(tmp_path / ("host" + threads)), {"DEFUSE_THREADS": threads})
        gpu = run_flat(case, align, str(tmp_path / ("gpu" + threads)), {"DEFUSE_THREADS": threads, "DEFUSE_EVAL_GPU": "1"})
        assert (host[0], host[2]) == (0, exp), threads
        assert gpu == host, threads
    timed = run_flat(case, align, str(tmp_path / "timed"), {"DEFUSE_TIMING": "1", "DEFUSE_EVAL_GPU": "1", "DEFUSE_THREADS": "16"})
    assert timed[0] == 0 and timed[2] == exp and "eval gpu:" in timed[1] and " %d records, %d groups" % (len(lines), len(lines) // 2700) in timed[1], timed[1]


@pytest.mark.gpu
def test_tool_flagged_and_no_split_groups(tools, tmp_path):
    """The two kinds of group the library leaves to the tool: all scores negative (the reference's message and the N line) and
    kept records of 8 or 9 read bases (a zero range: the host's own NaN and infinity, printed with their signs).  The files,
    stderr and exit status are the host path's.  The oracle has no branch for the first kind and prints a NaN without its
    sign, so it checks the other groups, with the sign of the tool's NaN removed."""
    case, lines = generated_case(tmp_path, 40, n_fusions=12, seed=23)
    prime(case, tmp_path)
    ids = sorted({int(l.split("\t", 1)[0]) for l in lines})
    assert len(ids) >= 8
    edits = {ids[1]: "negative", ids[2]: (4, 4), ids[4]: (5, 4), ids[5]: (8, 0), ids[6]: (0, 9)}
    out = []
    for l in lines:
        f = l.split("\t")
        e = edits.get(int(f[0]))
        if e == "negative":
            f[8] = str(-int(f[8]))
        elif e:
            f[6], f[7] = str(e[0]), str(e[1])
        out.append("\t".join(f))
    align = str(tmp_path / "flags.align")
    open(align, "w").write("".join(out))
    for threads in ("1", "4"):
        host = run_flat(case, align, str(tmp_path / ("host" + threads)), {"DEFUSE_THREADS": threads})
        gpu = run_flat(case, align, str(tmp_path / ("gpu" + threads)), {"DEFUSE_THREADS": threads, "DEFUSE_EVAL_GPU": "1"})
        assert gpu == host, threads
        assert host[0] == 0 and host[1].count("Error: Unable to find max score split") == 1
    seq = {int(l.split("\t", 1)[0]): l.rstrip("\n").split("\t") for l in host[2][0].splitlines()}
    assert seq[ids[1]][1:] == ["N", "0", "0", "-1", "-1"]
    assert "nan" in seq[ids[2]][5] and "nan" in seq[ids[4]][5] and seq[ids[5]][4] == "inf" and "nan" in seq[ids[6]][5]
    assert not any(l.startswith("%d\t" % ids[1]) for l in host[2][2].splitlines())          # no kept lines for the N group
    timed = run_flat(case, align, str(tmp_path / "timed"), {"DEFUSE_TIMING": "1", "DEFUSE_EVAL_GPU": "1"})
    assert timed[2] == host[2] and " 4 flagged" in timed[1], timed[1]
    rest = str(tmp_path / "rest.align")
    open(rest, "w").write("".join(l for l in out if int(l.split("\t", 1)[0]) != ids[1]))
    exp = oracle_files(case, rest)
    drop = lambda text: "".join(l for l in text.splitlines(True) if int(l.split("\t", 1)[0]) != ids[1])
    assert (drop(host[2][0]).replace("-nan", "nan"), drop(host[2][1]), host[2][2]) == exp


@pytest.mark.gpu
def test_tool_malformed_lines_like_the_host_path(tools, tmp_path):
    """A malformed line in the middle of a piece, and one that is the first line of a piece: the same three files, stderr
    and exit status as without the variable."""
    case, lines = generated_case(tmp_path, 300, n_fusions=40, seed=22)
    prime(case, tmp_path)
    ids = [int(l.split("\t", 1)[0]) for l in lines]
    heads = [k for k in range(1, len(lines)) if ids[k] != ids[k - 1]]
    assert len(heads) >= 20

    def both(text, threads, tag):
        align = str(tmp_path / (tag + ".align"))
        open(align, "w").write(text)
        host = run_flat(case, align, str(tmp_path / (tag + ".host")), {"DEFUSE_THREADS": threads})
        gpu = run_flat(case, align, str(tmp_path / (tag + ".gpu")), {"DEFUSE_THREADS": threads, "DEFUSE_EVAL_GPU": "1"})
        assert gpu == host, tag
        assert host[0] == 1 and host[1].startswith("Error: ") and len(host[2][0]) > 0
        return host

    # in the middle of a group in the middle of a piece: the group it sits in is not written
    k = heads[7] + 100
    bad = lines[k].split("\t")
    bad[5] = "x7"
    for threads in ("1", "3", "16"):
        h = both("".join(lines[:k] + ["\t".join(bad)] + lines[k + 1:]), threads, "mid" + threads)
        assert len(h[2][0].splitlines()) == 8 and "bad integer 'x7'" in h[1]      # groups 0..7; heads[7] opens group 8
    # opens a new group with a readable id: the running group is written first
    bad = lines[heads[7]].split("\t")
    bad[8] = ""
    h = both("".join(lines[:heads[7]] + ["\t".join(bad)] + lines[heads[7] + 1:]), "4", "opens")
    assert len(h[2][0].splitlines()) == 8
    # the first line of the second of two pieces: the cut moves forward from the middle of the file to the next change of the
    # id column, and a line whose id cannot be read is such a change
    middle = sum(len(l) for l in lines) // 2
    at, k = 0, 0
    while at <= middle + 16:                                         # the first group boundary past the middle (of the longer file too)
        at += len(lines[k])
        k += 1
    k = next(h for h in heads if h >= k)
    text = "".join(lines[:k] + ["short\tline\n"] + lines[k:])
    off = sum(len(l) for l in lines[:k])
    mid = len(text) // 2
    prev_head = heads[heads.index(k) - 1]
    assert mid < off and text.count("\n", mid, off) + 2 < k - prev_head      # only lines of one group between the middle and it: the cut lands on it
    h = both(text, "2", "cut")
    assert "Format error for candidate reads line" in h[1]
    assert len(h[2][0].splitlines()) == heads.index(k)              # the group before it is cancelled: the reader was still collecting it
