"""include/defuse_rec.h: the record store (defuse_amd/csrc/rec_api.hip through defuse_amd/rec.py) — the split-alignment
records of several batches sorted on the GPU into the order of the pipeline's `LC_ALL=C sort -n -k 1`, and their lines.

The expected order is rec_case.expected_text everywhere: numeric fusion id, then the bytes of the line.  One test without
a GPU pins it, and the __host__ __device__ code of rec_shared.hpp, against GNU sort.  A sort by the numeric values of the
fields is the mistake to catch (100 sorts before 99, -1 before -10 before -9): check_sorted asserts, for every input of 64
records or more, that such a sort gives another text than the expected one, so no case that goes through it can pass on it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import abi
from tests import rec_case as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "defuse_rec.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "config1", "expected.derived.align.txt")
DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = -1, -2, -3, -4


# ---------------------------------------------------------------------------------------------- CPU
def test_header_and_binding_agree(built):
    """rec_timing: the binding's fields are the header's, in order, with its types and offsets; every prototype of the header
    is in rec.EXPORTS, bound and exported by the library."""
    from defuse_amd import rec
    body = re.search(r"typedef struct rec_timing \{(.*?)\} rec_timing;", open(HEADER).read(), re.S).group(1)
    fields = [(n, t) for t, n in re.findall(r"(int32_t|int64_t|float|double)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))]
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    assert [(n, ctype[t]) for n, t in fields] == list(rec.RecTiming._fields_)
    sizes, n = abi.check("defuse_rec.h", rec, r"rec_[a-z_]+")
    assert sizes == [56] and n == 14
    assert rec.FIELDS == rc.FIELDS and rec.MAX_LINE == 9 * 12 + 1


def test_argument_errors_without_a_device(built):
    from defuse_amd import dsa, rec
    lib = rec.lib()
    h = ctypes.c_void_p()
    for d in [999] + ([0] if lib.dsa_device_count() == 0 else []):
        assert lib.rec_create(d, ctypes.byref(h)) == DSA_E_DEVICE and not h.value
        assert len(lib.rec_last_error()) > 0
    with pytest.raises(dsa.DsaError) as e:
        rec.Store(999)
    assert e.value.code == DSA_E_DEVICE
    assert lib.rec_create(0, None) == DSA_E_ARG
    r = np.zeros(4, dsa.RECORD_DTYPE)
    n, p = ctypes.c_int64(), ctypes.c_void_p()
    calls = [lambda: lib.rec_clear(None), lambda: lib.rec_append(None, r.ctypes.data, 4), lambda: lib.rec_append(None, r.ctypes.data, -1),
             lambda: lib.rec_append_device(None, r.ctypes.data, 4), lambda: lib.rec_tail(None, 4, ctypes.byref(p)), lambda: lib.rec_tail(None, -1, None),
             lambda: lib.rec_commit(None, 1), lambda: lib.rec_sort(None), lambda: lib.rec_count(None, ctypes.byref(n)),
             lambda: lib.rec_records_device(None, ctypes.byref(p), ctypes.byref(n)), lambda: lib.rec_download(None, r.ctypes.data, 4, ctypes.byref(n)),
             lambda: lib.rec_text(None, None, 0, None, 0, ctypes.byref(n)), lambda: lib.rec_get_timing(None, None)]
    for call in calls:
        assert call() == DSA_E_ARG
        assert len(lib.rec_last_error()) > 0
    lib.rec_destroy(None)                                           # a no-op


WALK = r'''
#include "%s/defuse_amd/csrc/rec_shared.hpp"
#include <algorithm>
#include <cstdio>
#include <vector>
// argv[1]: records (40 bytes each).  argv[2] receives every record's line in input order, argv[3] the input indices in the
// order of (fusion key, field keys 2-9), equal keys in input order.
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<dsa_record> recs;
    dsa_record r;
    while (fread(&r, sizeof r, 1, in) == 1) recs.push_back(r);
    fclose(in);
    FILE* text = fopen(argv[2], "wb");
    for (const dsa_record& x : recs) {
        std::vector<char> line(rec_line_length(x));              // exactly the promised length: a longer line is an overflow
        if (rec_write_line(x, line.data()) != (int)line.size() || line.size() > (size_t)REC_MAX_LINE) return 3;
        fwrite(line.data(), 1, line.size(), text);
    }
    fclose(text);
    struct K { uint32_t fusion; uint64_t f[REC_FIELDS - 1]; };
    std::vector<K> keys(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) {
        keys[i].fusion = rec_fusion_key(recs[i].fusion_id);
        for (int k = 1; k < REC_FIELDS; ++k) {
            keys[i].f[k - 1] = rec_field_key(rec_fields(recs[i])[k]);
            if (keys[i].f[k - 1] >> REC_FIELD_KEY_BITS) return 4;
        }
    }
    if (rec_field_key(0) != REC_KEY_OF_0 || rec_field_key(1) != REC_KEY_OF_1) return 5;
    std::vector<long long> order(recs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (long long)i;
    std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) {
        if (keys[a].fusion != keys[b].fusion) return keys[a].fusion < keys[b].fusion;
        return std::lexicographical_compare(keys[a].f, keys[a].f + REC_FIELDS - 1, keys[b].f, keys[b].f + REC_FIELDS - 1);
    });
    FILE* out = fopen(argv[3], "w");
    for (long long i : order) fprintf(out, "%%lld\n", i);
    fclose(out);
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    """The shared code as a host program: plain, and as a stand-alone executable under ASan + UBSan."""
    d = tmp_path_factory.mktemp("recwalk")
    src = d / "walk.hip"
    src.write_text(WALK % ROOT)
    base = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17"]
    subprocess.check_call(base + ["-O1", "-o", str(d / "walk"), str(src)])
    subprocess.check_call(base + ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                                  "-Xarch_host", "-fno-omit-frame-pointer", "-o", str(d / "walk_asan"), str(src)])
    return d


def golden_records():
    from defuse_amd import dsa
    rows = [tuple(int(x) for x in l.split("\t")[:9]) + (k,) for k, l in enumerate(open(GOLDEN).read().splitlines())]
    assert len(rows) == 41
    return np.array(rows, dtype=dsa.RECORD_DTYPE)


@pytest.mark.parametrize("case", ["golden", "generated", "generated01"])
def test_shared_code_against_gnu_sort(host_walk, case):
    """rec_write_line prints "%d\\t" * 9 + "\\n"; the order of (fusion key, field keys) is GNU sort's on those lines and the
    Python expression's; a numeric sort is not.  The same program under ASan + UBSan gives the same files and no report."""
    from tests.test_sanitizers import BAD, ENV
    d = host_walk
    records = golden_records() if case == "golden" else rc.draw(np.random.default_rng(11), 5000, flags01=case == "generated01")
    lines = rc.lines_of(records)
    (d / "in.bin").write_bytes(records.tobytes())
    (d / "in.txt").write_bytes(b"".join(lines))
    gnu = subprocess.run(["sort", "-n", "-k", "1", str(d / "in.txt")], capture_output=True, check=True, env=dict(os.environ, LC_ALL="C")).stdout
    exp = rc.expected_text(lines)
    assert gnu == exp                                               # the expression every other test uses
    assert rc.text_of(lines, rc.numeric_order(records)) != exp      # a sort by numeric fields cannot pass
    outs = {}
    for exe, env in (("walk", {}), ("walk_asan", ENV["asan"])):
        r = subprocess.run([str(d / exe), str(d / "in.bin"), str(d / (exe + ".txt")), str(d / (exe + ".order"))], capture_output=True, text=True,
                           env=dict(os.environ, **env), stdin=subprocess.DEVNULL, timeout=300)
        assert not any(b in r.stderr for b in BAD), r.stderr[-3000:]
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        outs[exe] = ((d / (exe + ".txt")).read_bytes(), [int(x) for x in (d / (exe + ".order")).read_text().split()])
    text, order = outs["walk"]
    assert text == b"".join(lines)
    assert rc.text_of(lines, order) == exp
    assert order == rc.expected_order(records, lines).tolist()      # ties in input order
    assert outs["walk_asan"] == outs["walk"]


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def store(built):
    from defuse_amd import rec
    s = rec.Store(0)                    # raises without a GPU: no fallback
    yield s
    s.close()


@pytest.fixture(scope="module")
def ectx(built):
    from defuse_amd import eval as ev
    ctx = ev.Context(0)
    yield ctx
    ctx.close()


def printed(records):
    """The nine printed fields as an (n, 9) array."""
    return np.ascontiguousarray(records).view(np.int32).reshape(-1, 10)[:, :9]


def check_sorted(s, records, full=False, numeric_differs=True):
    """The store holds `records` (appended in that order) sorted: the downloaded array and the text against the expected
    order; full: pair_idx as well, which pins the order of equal lines.  Returns (expected records, their lines)."""
    lines = rc.lines_of(records)
    order = rc.expected_order(records, lines)
    exp_text = rc.expected_text(lines)
    assert rc.text_of(lines, order) == exp_text
    if numeric_differs:
        assert rc.text_of(lines, rc.numeric_order(records)) != exp_text
    got = s.download()
    exp = records[order]
    assert len(s) == len(got) == len(exp)
    assert np.array_equal(printed(got), printed(exp))
    if full:
        assert got.tobytes() == exp.tobytes()
    assert s.text() == exp_text
    return exp, [lines[i] for i in order]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 70001])
def test_sizes_at_the_kernels_edges(store, n):
    """Three uneven appends, one of them empty; with read_end / revcomp of any value (nine sorts) and of 0 or 1 (seven)."""
    for flags01 in (False, True):
        records = rc.draw(np.random.default_rng(100 + n), n, flags01=flags01)
        store.clear()
        for part in rc.parts_of(records, [n // 5, n // 5]):
            store.append(part)
        store.sort()
        check_sorted(store, records, numeric_differs=n >= 64)
        t = store.timing()
        assert t["n_records"] == n and t["n_sorts"] == (0 if n <= 1 else 7 if flags01 else 9)
        assert n <= 1 or (t["keys_ms"] > 0 and t["sort_ms"] > 0 and t["gather_ms"] > 0 and t["format_ms"] > t["write_ms"] > 0)
        assert t["text_bytes"] == sum(len(l) for l in rc.lines_of(records))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one_fusion", "small_fusions", "descending"])
def test_group_shapes(store, shape):
    rng = np.random.default_rng(7)
    if shape == "one_fusion":
        records = rc.draw(rng, 300000, flags01=True, fusion_ids=[-42])
    elif shape == "small_fusions":
        sizes = rng.integers(1, 3, 200000)
        records = rc.draw(rng, int(sizes.sum()), flags01=True)
        ids = rng.permutation(np.arange(-100000, 100000))
        records["fusion_id"] = np.repeat(ids, sizes)
    else:
        records = rc.draw(rng, 50000, flags01=True)
        records["fusion_id"] = np.repeat(np.arange(5000, -5000, -1), 5)      # five records each: their order is the lines'
    store.clear()
    store.append(records)
    store.sort()
    check_sorted(store, records)


@pytest.mark.gpu
def test_ties_stability_repetition(store):
    from defuse_amd import rec
    rng = np.random.default_rng(8)
    records = rc.draw(rng, 1000, flags01=True)
    records[600:] = records[rng.integers(0, 600, 400)]              # 400 exact nine-field duplicates ...
    records["pair_idx"] = np.arange(1000)                           # ... that only pair_idx tells apart
    records = records[rng.permutation(1000)]
    store.clear()
    store.append(records)
    store.sort()
    once, _ = check_sorted(store, records, full=True)
    store.sort()                                                    # a second sort changes nothing
    assert store.download().tobytes() == once.tobytes()
    # sort, append a chunk that interleaves with the first, sort: one sort of both
    more = rc.draw(rng, 700, flags01=True)
    more[300:] = records[rng.integers(0, 1000, 400)]
    more["pair_idx"] = 5000 + np.arange(700)
    store.append(more)
    store.sort()
    both = np.concatenate((records, more))
    check_sorted(store, both, full=True)
    merged = store.download()
    assert (np.diff(np.flatnonzero(merged["pair_idx"] >= 5000)) > 1).any()      # the chunks do interleave
    # clear and reuse: what a fresh store gives
    store.clear()
    assert len(store) == 0 and store.text() == b""
    store.append(more)
    store.sort()
    with rec.Store(0) as fresh:
        fresh.append(more)
        fresh.sort()
        assert fresh.download().tobytes() == store.download().tobytes() and fresh.text() == store.text()
    check_sorted(store, more, full=True)


@pytest.mark.gpu
def test_growth_keeps_the_records(built):
    """A store grown by 50 appends of 1 000 records, some handed over through rec_tail / rec_commit; the buffer is reallocated
    right after a tail was committed.  Equal to the store that received everything in one append."""
    from defuse_amd import rec
    from tests.test_eval import _hip_runtime
    records = rc.draw(np.random.default_rng(9), 50000)
    with rec.Store(0) as grown, rec.Store(0) as whole:
        hip = _hip_runtime()                                        # the runtime the library has loaded, for a copy of the test's own
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        moved_after_commit = 0
        for k in range(50):
            part = np.ascontiguousarray(records[1000 * k:1000 * (k + 1)])
            before = grown.records_device()[0]
            if k in (1, 10, 30):
                tail = grown.tail(1500)                             # more room than is used
                assert hip.hipMemcpy(tail, part.ctypes.data, part.nbytes, 1) == 0     # host to device
                grown.commit(1000)
            else:
                grown.append(part)
                moved_after_commit += 1 if k in (2, 11, 31) and grown.records_device()[0] != before else 0
            assert len(grown) == 1000 * (k + 1)
        assert moved_after_commit >= 1                              # 1 000 -> tail of 1 500 -> 2 000 records in room for 2 876: the next append moves them
        assert grown.download().tobytes() == records.tobytes()      # unsorted: append order
        whole.append(records)
        assert grown.text() == whole.text() == b"".join(rc.lines_of(records))
        grown.sort()
        whole.sort()
        assert grown.download().tobytes() == whole.download().tobytes()
        check_sorted(grown, records)
        # tail / commit misuse
        lib, h, p = grown.lib, grown.h, ctypes.c_void_p()
        assert lib.rec_commit(h, 1) == DSA_E_ARG                    # no tail
        assert lib.rec_tail(h, -1, ctypes.byref(p)) == DSA_E_ARG and lib.rec_tail(h, 4, None) == DSA_E_ARG
        assert lib.rec_tail(h, 4, ctypes.byref(p)) == 0 and p.value
        assert lib.rec_commit(h, 5) == DSA_E_ARG and lib.rec_commit(h, -1) == DSA_E_ARG
        assert lib.rec_commit(h, 0) == 0 and lib.rec_commit(h, 0) == DSA_E_ARG      # one commit per tail
        assert lib.rec_tail(h, 4, ctypes.byref(p)) == 0
        grown.append(records[:1])                                   # an append takes the tail back
        assert lib.rec_commit(h, 1) == DSA_E_ARG and len(lib.rec_last_error()) > 0
        assert len(grown) == 50001
        # the size limit is checked before anything is touched
        q = ctypes.c_void_p()
        for n in (2 ** 31 - 2 - 50001, 2 ** 31):
            assert lib.rec_append_device(h, p, n) == DSA_E_LIMIT and lib.rec_tail(h, n, ctypes.byref(q)) == DSA_E_LIMIT and not q.value
        assert len(grown) == 50001


@pytest.mark.gpu
def test_text_protocol(store):
    from defuse_amd import dsa
    rng = np.random.default_rng(10)
    records = rc.draw(rng, 3000)
    store.clear()
    store.append(records)
    store.sort()
    exp, lines = check_sorted(store, records)
    total = sum(len(l) for l in lines)
    # capacity: too small leaves out untouched and reports the size; exact succeeds
    buf = np.full(total, 0x55, np.uint8)
    got = ctypes.c_int64()
    for cap in (0, total - 1):
        assert store.lib.rec_text(store.h, None, 0, buf.ctypes.data, cap, ctypes.byref(got)) == DSA_E_CAPACITY
        assert got.value == total and (buf == 0x55).all()
    assert store.lib.rec_text(store.h, None, 0, None, 0, ctypes.byref(got)) == DSA_E_CAPACITY and got.value == total
    with pytest.raises(dsa.DsaError) as e:
        store.text(cap=total - 1)
    assert (e.value.code, e.value.bytes) == (DSA_E_CAPACITY, total)
    assert store.text(cap=total) == b"".join(lines)
    assert store.lib.rec_text(store.h, None, 0, buf.ctypes.data, total, None) == DSA_E_ARG
    assert store.lib.rec_text(store.h, None, 0, buf.ctypes.data, -1, ctypes.byref(got)) == DSA_E_ARG
    # a kept list: any order, indices may repeat
    kept = rng.integers(0, 3000, 1500)
    kept[700:710] = kept[0]
    assert store.text(kept) == b"".join(lines[i] for i in kept.tolist())
    assert store.text(kept[:1]) == lines[int(kept[0])]
    assert store.text(np.zeros(0, np.int64)) == b""
    buf[:] = 0x55
    for bad in (3000, -1):
        k = kept.copy()
        k[1499] = bad
        assert store.lib.rec_text(store.h, k.ctypes.data, 1500, buf.ctypes.data, total, ctypes.byref(got)) == DSA_E_ARG
        assert (buf == 0x55).all()
    assert store.lib.rec_text(store.h, kept.ctypes.data, -1, buf.ctypes.data, total, ctypes.byref(got)) == DSA_E_ARG


@pytest.mark.gpu
def test_longest_lines(store):
    """A record of nine INT_MIN prints 109 bytes.  A workgroup's 256 such lines are the largest span there is, and it begins
    15 bytes past a multiple of 16 when the text before it is 255 such lines and one of 28 bytes."""
    from defuse_amd import dsa
    records = np.zeros(700, dsa.RECORD_DTYPE)
    for f in rc.FIELDS:
        records[f] = rc.INT_MIN
    records[0] = (10,) * 10
    lines = rc.lines_of(records)
    assert len(lines[0]) == 28 and len(lines[1]) == 109 and (28 + 255 * 109) % 16 == 15
    store.clear()
    store.append(records[1:2])
    assert store.text() == lines[1]
    store.clear()
    store.append(records)
    assert store.text() == b"".join(lines)                          # unsorted: append order
    assert store.text(np.arange(1, 700)) == b"".join(lines[1:])    # aligned spans
    store.sort()
    assert store.text() == b"".join(lines[1:] + lines[:1])


@pytest.mark.gpu
def test_chain_over_three_uploads(gpu_ctx, ectx):
    """dsa_run on three uploads that each hold a third of every fusion's reads -> dsa_copy_records_device into rec_tail ->
    rec_commit -> rec_sort -> eval_groups_device on rec_records_device: the records, groups, kept list and FP64 sums of the
    one-upload run evaluated on the host in the expected order; the kept lines; and, unsorted, other groups."""
    from defuse_amd import rec, synth
    from tests import test_eval as te
    ref, fus, reads, pairs = synth.make_batch(40, 12, lq=50, lr=260, seed=5)
    gpu_ctx.upload(ref, fus, reads, pairs)
    gpu_ctx.plan()
    assert gpu_ctx.run() > 0
    whole = gpu_ctx.download()
    lines = rc.lines_of(whole)
    exp = whole[rc.expected_order(whole, lines)]
    exp_lines = rc.lines_of(exp)
    assert rc.text_of(lines, rc.numeric_order(whole)) != b"".join(exp_lines)
    parts = []
    with rec.Store(0) as s:
        for k in range(3):
            gpu_ctx.upload(ref, fus, reads, np.ascontiguousarray(pairs[k::3]))      # every fusion is in every upload
            gpu_ctx.plan()
            n = gpu_ctx.run()
            tail = s.tail(n)
            assert gpu_ctx.records_to_device(tail, n) == n
            s.commit(n)
            parts.append(gpu_ctx.download())
        assert len(s) == len(whole) and min(len(p) for p in parts) > 0
        assert all(len(set(p["fusion_id"].tolist())) > 30 for p in parts)
        s.sort()
        assert s.timing()["n_sorts"] == 7                           # dsa records: read_end and revcomp are 0 or 1
        got = s.download()
        assert np.array_equal(printed(got), printed(exp))
        ptr, n = s.records_device()
        groups, kept = ectx.evaluate_device(ptr, n)
        te.check(exp, groups, kept)                                 # bit patterns of pos_sum / min_sum included
        assert len(groups) == len(set(whole["fusion_id"].tolist())) and len(kept) > 0
        assert s.text(kept) == b"".join(exp_lines[i] for i in kept.tolist())
        assert s.text() == b"".join(exp_lines)
    unsorted_groups, _ = ectx.evaluate(np.concatenate(parts))
    assert len(unsorted_groups) > len(groups)                       # a fusion's records come back in every batch: what the store is for


@pytest.mark.gpu
def test_deterministic(built):
    from defuse_amd import rec
    records = rc.draw(np.random.default_rng(12), 20000, flags01=True)
    records[5000:9000] = records[:4000]
    out = []
    for _ in range(2):
        with rec.Store(0) as s:
            for part in rc.parts_of(records, [7000, 7001, 15000]):
                s.append(part)
            s.sort()
            out.append((s.download().tobytes(), s.text()))
    assert out[0] == out[1]
