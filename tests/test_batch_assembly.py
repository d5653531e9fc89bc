"""The batch assembly on the GPU (include/defuse_bat.h through defuse_amd/bat.py), dsa_upload_device and
cand_enumerate_device.

Yardsticks, none of them the new path itself: for the assembly defuse_amd.cand.dsa_batch (the host loop the assembly
replaces), compared byte for byte on all four arrays; for dsa_upload_device the records, tile width and kernel counts of
dsa_upload on the same arrays; for the chain tests/golden/smoke/expected.split.align.txt and eval_groups on the records of
the host chain."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOKE = os.path.join(ROOT, "tests", "golden", "smoke")
E_CAPACITY, E_DEVICE, E_ARG, E_LIMIT = -1, -2, -3, -4
ODD_BYTES = b"ACGTNacgtn.\x00\xff*"
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 150)


@pytest.fixture(scope="module")
def bat(built):
    from defuse_amd import bat as b
    return b


@pytest.fixture(scope="module")
def cand(built):
    from defuse_amd import cand as c
    return c


@pytest.fixture(scope="module")
def ectx(built):
    from defuse_amd import eval as ev
    ctx = ev.Context(0)
    yield ctx
    ctx.close()


def cands_of(cand, rows):
    """Rows (fusion_id, fragment, read_end, revcomp) -> cand.RECORD_DTYPE, the other fields as cand_enumerate sets them."""
    out = np.zeros(len(rows), dtype=cand.RECORD_DTYPE)
    for k, (fid, frag, rend, rc) in enumerate(rows):
        out[k] = (k, fid, frag, 1 - rc, rend, rc, 1, (0, 0, 0, 0))
    return out


def reads_dict(cand, reads):
    """(fragment, read_end, bytes) in the order given -> the dict cand.dsa_batch takes: the last of a key wins."""
    return {cand.read_id(frag, rend): bytes(seq) for frag, rend, seq in reads}


# ---------------------------------------------------------------------------------------------- device memory of the tests
def hip_runtime():
    """The HIP runtime the library has loaded, for device allocations of the tests' own."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = ctypes.CDLL(line.split()[-1])
            hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            hip.hipFree.argtypes = [ctypes.c_void_p]
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            return hip
    raise RuntimeError("libamdhip64 is not loaded")


class DeviceArray:
    """A copy of a numpy array in device memory (hipMalloc / hipMemcpy); .ptr is never 0."""

    def __init__(self, a):
        self.hip = hip_runtime()
        a = np.ascontiguousarray(a)
        self.nbytes = a.nbytes
        dev = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(dev), max(a.nbytes, 16)) == 0
        self.ptr = dev.value
        if a.nbytes:
            assert self.hip.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        assert self.hip.hipFree(self.ptr) == 0


def from_device(ptr, n, dtype):
    out = np.zeros(n, dtype=dtype)
    if n:
        assert hip_runtime().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def assert_same_batch(got, want):
    for g, w, name in zip(got, want, ("ref_bytes", "fusions", "read_bytes", "pairs")):
        assert g.dtype == w.dtype and len(g) == len(w), name
        assert g.tobytes() == w.tobytes(), name


def check_both_entries(bat, cand, batch, reads, windows, cands, rdict, wdict):
    """bat_assemble and bat_assemble_device of `cands` against cand.dsa_batch; returns the expected tuple."""
    want = cand.dsa_batch(cands, rdict, wdict)
    v = batch.assemble(reads, windows, cands)
    assert (v.n_pairs, v.n_fusions, v.read_bytes_len, v.ref_bytes_len) == (len(want[3]), len(want[1]), len(want[2]), len(want[0]))
    assert v.ref_bytes and v.fusions and v.read_bytes and v.pairs
    assert_same_batch(batch.fetch(), want)
    with DeviceArray(cands) as dev:
        batch.assemble_device(reads, windows, dev.ptr, len(cands))
        assert_same_batch(batch.fetch(), want)
    return want


# ---------------------------------------------------------------------------------------------- without a GPU
def test_bat_struct_layouts_match_header(bat):
    """sizeof and offsetof of every struct of the header, as a C++ and a C compiler see them, against the ctypes structs."""
    sizes, _ = abi.check("defuse_bat.h", bat, r"(?:bat|cand)_[a-z_]+")
    assert sizes == [24, 64, 48]
    assert (bat.READ_DTYPE.itemsize, ctypes.sizeof(bat.View), ctypes.sizeof(bat.BatTiming)) == (24, 64, 48)


def test_library_exports_bat(bat, cand):
    from defuse_amd import dsa
    assert abi.check_functions("defuse_bat.h", bat, r"(?:bat|cand)_[a-z_]+") == 14
    assert ctypes.CDLL(dsa.LIB_PATH).dsa_upload_device is not None
    assert "dsa_upload_device" in dsa.EXPORTS
    assert hasattr(dsa.Context, "upload_device") and hasattr(cand.Session, "enumerate_device")


def test_bat_argument_errors_need_no_device(bat, cand):
    """Every argument error that can be told from the arguments alone comes back with its code before a device is touched.
    (The errors of bat_assemble that need its objects - an unknown fusion_id, the byte totals, two devices - need a device
    to make the objects on: a store cannot be created without one.  They are in the GPU tests below.)"""
    from defuse_amd import dsa
    lib = bat.lib()
    err = lambda: lib.bat_last_error().decode()
    h = ctypes.c_void_p()
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)

    def reads(rows, n=None, nbytes=len(data), out=h):
        r = np.array([tuple(x) for x in rows], dtype=bat.READ_DTYPE).reshape(-1)
        return lib.bat_reads_create(0, data.ctypes.data if nbytes else None, nbytes, r.ctypes.data if len(r) else None, len(r) if n is None else n,
                                    ctypes.byref(out) if out is not None else None)
    good = (0, 4, 7, 0, 0)
    assert reads([good], out=None) == E_ARG
    assert reads([good], n=-1) == E_ARG and "negative" in err()
    assert reads([good], nbytes=-1) == E_ARG and "negative" in err()
    assert reads([], n=1) == E_ARG and "null" in err()
    assert reads([], n=2 ** 31) == E_LIMIT
    assert reads([good, (0, 4, -1, 0, 0)]) == E_ARG and "read 1" in err() and "fragment" in err()
    assert reads([good, good, (0, 4, 7, 2, 0)]) == E_ARG and "read 2" in err() and "read_end" in err()
    assert reads([(0, -1, 7, 0, 0)]) == E_ARG and "read 0" in err() and "length" in err()
    assert reads([good, (7, 4, 7, 0, 0)]) == E_ARG and "read 1" in err() and "outside" in err()       # one byte beyond
    assert reads([(-1, 4, 7, 0, 0)]) == E_ARG and "outside" in err()
    assert reads([(11, 0, 7, 0, 0)]) == E_ARG and "outside" in err()
    assert reads([(2 ** 62, 2 ** 31 - 1, 7, 0, 0)]) == E_ARG and "outside" in err()                   # no overflow of off + len
    assert not h

    def windows(rows, n=None, nbytes=len(data), out=h):
        f = np.array([tuple(x) for x in rows], dtype=dsa.FUSION_DTYPE).reshape(-1)
        return lib.bat_windows_create(0, data.ctypes.data if nbytes else None, nbytes, f.ctypes.data if len(f) else None, len(f) if n is None else n,
                                      ctypes.byref(out) if out is not None else None)
    w = (5, 0, 4, 4, 6)
    assert windows([w], out=None) == E_ARG
    assert windows([w], n=-1) == E_ARG and "negative" in err()
    assert windows([], n=1) == E_ARG and "null" in err()
    assert windows([w, (6, 0, 4, 4, 7)]) == E_ARG and "fusion 1" in err() and "outside" in err()
    assert windows([(6, -1, 4, 4, 6)]) == E_ARG and "fusion 0" in err()
    assert windows([(6, 0, -4, 4, 6)]) == E_ARG and "fusion 0" in err()
    assert windows([w, (6, 0, 1, 1, 1), (5, 1, 2, 3, 4)]) == E_ARG and "fusion_id 5" in err() and "fusions 0 and 2" in err()
    assert windows([w], nbytes=2 ** 31) == E_LIMIT
    assert not h

    c = cands_of(cand, [(5, 7, 0, 0)])
    one = ctypes.c_void_p(1)           # stands for an object: the missing one is found before any is looked at
    for fn in (lib.bat_assemble, lib.bat_assemble_device):
        assert fn(None, one, c.ctypes.data, 1, one) == E_ARG and "no reads" in err()
        assert fn(one, None, c.ctypes.data, 1, one) == E_ARG and "no windows" in err()
        assert fn(one, one, c.ctypes.data, 1, None) == E_ARG and "no batch" in err()
    view, timing = bat.View(), bat.BatTiming()
    assert lib.bat_batch_view(None, ctypes.byref(view)) == E_ARG and lib.bat_get_timing(None, ctypes.byref(timing)) == E_ARG
    assert lib.bat_batch_fetch(None, None, 0, None, 0, None, 0, None, 0) == E_ARG
    assert lib.bat_batch_create(0, None) == E_ARG
    # the device twins: the alignments are checked before the session is looked at, as cand_enumerate checks them
    n_out = ctypes.c_int64(-7)
    bad = cand.alignments([(0, 0, 100, 200, 9, 0), (0, 0, 100, 200, -1, 0)])
    assert lib.cand_enumerate_device(None, bad.ctypes.data, 2, 0, ctypes.byref(n_out), None) == E_ARG
    assert "alignment 1" in lib.cand_last_error().decode() and n_out.value == 0
    assert lib.cand_enumerate_device(None, bad.ctypes.data, 1, 0, ctypes.byref(n_out), None) == E_ARG and "session" in lib.cand_last_error().decode()
    assert lib.cand_enumerate_device(None, bad.ctypes.data, 1, 2, ctypes.byref(n_out), None) == E_ARG and "order" in lib.cand_last_error().decode()
    dev, n = ctypes.c_void_p(), ctypes.c_int64()
    assert lib.cand_records_device(None, ctypes.byref(dev), ctypes.byref(n)) == E_ARG
    assert dsa.load_library().dsa_upload_device(None, None, 0, None, 0, None, 0, None, 0) == E_ARG
    # good arguments get as far as the device: no CPU path
    rc = reads([good])
    assert rc in (0, E_DEVICE)
    if rc == 0:
        lib.bat_reads_destroy(h)
    else:
        assert not h and "device" in err()


# ---------------------------------------------------------------------------------------------- GPU: assembly
def word_edge_case(cand):
    """Reads of LENGTHS at odd offsets of the store with other bytes between them; candidates in both orientations, the
    1-, 2-, 3- and 5-byte reads next to each other at every phase of the output dword."""
    store, recs, reads = bytearray(b"#"), [], []
    for i, n in enumerate(LENGTHS):
        seq = bytes(ODD_BYTES[(i * 5 + j * (1 + i % 3)) % len(ODD_BYTES)] for j in range(n))
        assert len(store) % 2 == 1
        recs.append((len(store), n, 100 + i, i & 1, 0))
        reads.append((100 + i, i & 1, seq))
        store += seq + (b"%" if (len(store) + n) % 2 == 0 else b"$!")
    assert set(b"".join(s for _, _, s in reads)) == set(ODD_BYTES)
    idx = {n: i for i, n in enumerate(LENGTHS)}
    small = [1, 2, 3, 5, 1, 1, 2, 5, 3, 3, 2, 1, 0, 1, 5, 5, 2, 2, 3, 1, 1, 1, 1, 5, 3, 2, 1]
    order = [(idx[n], k & 1) for k, n in enumerate(small)] + [(idx[n], 1 - (k & 1)) for k, n in enumerate(small)]
    order += [(i, rc) for i in range(len(LENGTHS)) for rc in (0, 1)] + [(idx[n], 1) for n in (3, 150, 1, 64, 2, 65, 5, 63)]
    rows = [(3, 100 + i, i & 1, rc) for i, rc in order]
    assert {(i, rc) for i, rc in order} == {(i, rc) for i in range(len(LENGTHS)) for rc in (0, 1)}
    return np.frombuffer(bytes(store), dtype=np.uint8), recs, reads, rows


@pytest.mark.gpu
def test_word_edges_of_the_gather(bat, cand):
    store, recs, reads, rows = word_edge_case(cand)
    recs = np.array(recs, dtype=bat.READ_DTYPE)
    assert all(o % 2 == 1 for o in recs["off"].tolist())
    wdict = {3: (b"ACGTN", b"acg")}
    with bat.Reads(store, recs) as r, bat.Windows.from_dict(wdict) as w, bat.Batch() as b:
        want = check_both_entries(bat, cand, b, r, w, cands_of(cand, rows), reads_dict(cand, reads), wdict)
        t = b.timing()
    assert len(want[2]) == sum(p[2] for p in want[3].tolist()) > 1000
    assert (t.n_candidates, t.n_fusions, t.read_bytes, t.ref_bytes) == (len(rows), 1, len(want[2]), 8) and t.upload_ms == 0
    # the yardstick itself on one read: reversed, ACGTacgt -> TGCAtgca, everything else as it is
    assert bytes(cand.reverse_complement(b"ACGTNacgtn.\x00\xff*")) == b"*\xff\x00.nacgtNACGT"


@pytest.mark.gpu
def test_lookup_rules(bat, cand):
    top = 2 ** 31 - 1
    reads = [(5, 0, b"AAAA"), (5, 0, b"CCCCC"), (9, 1, b"G"), (0, 0, b"ACGTNN"), (top, 1, b"TTGCA"), (0, 1, b"cg"), (top, 0, b"NNNNNNNNN"),
             (5, 0, b"ACGTTTT"), (21, 0, b"GATTACAGATTACAGATTACA")]
    rdict = reads_dict(cand, reads)
    assert rdict[cand.read_id(5, 0)] == b"ACGTTTT" and cand.read_id(top, 1) == -1 and cand.read_id(0, 1) == -2 ** 31
    wdict = {1: (b"ACGT", b"TTTT"), 2: (b"GG", b"CCCCC"), 3: (b"A", b"C")}
    rows = [(1, 5, 0, 0), (1, 5, 0, 1),                      # a key given three times: the last wins
            (2, 77, 0, 0), (2, 77, 1, 1), (1, 9, 0, 0),      # no such read (9 has read end 1 only): length 0, the offsets go on
            (2, 0, 0, 1), (2, top, 1, 0), (3, 0, 1, 1), (3, top, 0, 0), (1, top, 1, 1), (1, 9, 1, 1),
            (1, 21, 0, 0), (2, 21, 0, 1), (3, 21, 0, 0), (1, 21, 0, 1), (2, 21, 0, 0), (3, 21, 0, 1)]      # one read, three fusions, both ways
    cands = cands_of(cand, rows)
    with bat.Reads.from_dict(rdict) as r, bat.Windows.from_dict(wdict) as w, bat.Batch() as b:
        want = check_both_entries(bat, cand, b, r, w, cands, rdict, wdict)
        assert want[3]["read_len"].tolist()[:5] == [7, 7, 0, 0, 0] and want[3]["read_off"].tolist()[:6] == [0, 7, 14, 14, 14, 14]
        # the same store given record by record, duplicates and all, in device order of arrival
        with bat.Reads(*bat.pack_reads(reads)) as r2:
            check_both_entries(bat, cand, b, r2, w, cands, rdict, wdict)
        # an empty store: every read is the empty string
        with bat.Reads(np.zeros(0, np.uint8), np.zeros(0, bat.READ_DTYPE)) as empty:
            none = check_both_entries(bat, cand, b, empty, w, cands, {}, wdict)
            assert len(none[2]) == 0 and not none[3]["read_len"].any() and len(none[1]) == 3
        # no candidates: an empty batch, whatever the batch held before
        nothing = check_both_entries(bat, cand, b, r, w, cands[:0], rdict, wdict)
        assert [len(a) for a in nothing] == [0, 0, 0, 0]
        check_both_entries(bat, cand, b, r, w, cands[3:9], rdict, wdict)


@pytest.mark.gpu
def test_fusion_numbering(bat, cand):
    wdict = {40: (b"ACGTACGTAC", b"GGG"), 7: (b"T", b"CCCCCCC"), 1000: (b"NNNN", b"NNNN"), 99: (b"ACACACACACACACACA", b"GT"), 3: (b"GATTACA", b"TGTAATC"),
             8: (b"", b"ACGTA"), 15: (b"CCGG", b"AATTCCGGA"), 2: (b"AC", b"GT"), 11: (b"", b""), 2 ** 31 - 1: (b"TTT", b"A")}
    rdict = {cand.read_id(f, e): bytes(ODD_BYTES[(f + j) % len(ODD_BYTES)] for j in range(3 + f % 11)) for f in range(40) for e in (0, 1)}
    # in visiting order a read's candidates come together, so the fusions interleave: first seen 15, 3, 99, 7, 40, then 8, 11, 2^31 - 1
    rows = []
    for k, fids in enumerate([(15, 3), (15, 99), (3, 7, 99), (40, 15), (7,), (40, 3, 15, 99, 7), (8, 40), (11, 8, 3), (2 ** 31 - 1, 15), (99,)] * 3):
        rows += [(fid, k, k & 1, (k + j) & 1) for j, fid in enumerate(fids)]
    cands = cands_of(cand, rows)
    with bat.Reads.from_dict(rdict) as r, bat.Windows.from_dict(wdict) as w, bat.Batch() as b:
        want = check_both_entries(bat, cand, b, r, w, cands, rdict, wdict)
        assert want[1]["fusion_id"].tolist() == [15, 3, 99, 7, 40, 8, 11, 2 ** 31 - 1]          # neither by id nor as `windows` has them
        assert want[1]["ref0_len"].tolist()[5:7] == [0, 0] and want[1]["ref1_len"].tolist()[6] == 0
        check_both_entries(bat, cand, b, r, w, cands[::-1].copy(), rdict, wdict)
        check_both_entries(bat, cand, b, r, w, cands[5:6], rdict, wdict)
        # an unknown fusion_id in records 7 and 3: the lowest is named, by both entries, and the batch is empty afterwards
        bad = cands.copy()
        bad["fusion_id"][7] = 12
        bad["fusion_id"][3] = 41
        with pytest.raises(bat.BatError) as e:
            b.assemble(r, w, bad)
        assert e.value.code == E_ARG and "record 3:" in str(e.value)
        with DeviceArray(bad) as dev:
            with pytest.raises(bat.BatError) as e:
                b.assemble_device(r, w, dev.ptr, len(bad))
        assert e.value.code == E_ARG and "record 3:" in str(e.value)
        assert b.view().n_pairs == 0 and [len(a) for a in b.fetch()] == [0, 0, 0, 0]
        with bat.Windows.from_dict({}) as no_windows:
            with pytest.raises(bat.BatError) as e:
                b.assemble(r, no_windows, cands)
            assert e.value.code == E_ARG and "record 0:" in str(e.value)
        check_both_entries(bat, cand, b, r, w, cands, rdict, wdict)                              # and is usable again


def random_case(cand, seed):
    """300 windows of 0..400 bases of which 200 are used, 1500 reads of 0..160 bytes over all byte values of ODD_BYTES (40
    of them given twice), 5000 candidates of which about 5 % name a read that was not given."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(ODD_BYTES, dtype=np.uint8)
    text = lambda n: alphabet[rng.integers(0, len(alphabet), size=int(n))].tobytes()
    fids = rng.choice(100000, size=300, replace=False)
    wdict = {int(f): (text(rng.integers(0, 401)), text(rng.integers(0, 401))) for f in fids}
    keys = [(int(f), int(e)) for f, e in zip(rng.choice(3000, size=1500, replace=False), rng.integers(0, 2, size=1500))]
    reads = [(f, e, text(rng.integers(0, 161))) for f, e in keys]
    reads += [(f, e, text(rng.integers(0, 161))) for f, e in keys[:40]]
    used = fids[:200]
    rows = []
    for _ in range(5000):
        f, e = keys[int(rng.integers(0, len(keys)))]
        if rng.random() < 0.05:
            f += 5000
        rows.append((int(used[int(rng.integers(0, len(used)))]), f, e, int(rng.integers(0, 2))))
    return wdict, reads, cands_of(cand, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_against_dsa_batch(bat, cand, seed):
    wdict, reads, cands = random_case(cand, seed)
    rdict = reads_dict(cand, reads)
    with bat.Reads(*bat.pack_reads(reads)) as r, bat.Windows.from_dict(wdict) as w, bat.Batch() as b:
        # one batch object: a call, a smaller one, a larger one - nothing of an earlier batch may show
        for part in (cands[:3000], cands[3000:3400], cands):
            want = check_both_entries(bat, cand, b, r, w, part, rdict, wdict)
        assert len(want[1]) == 200 and len(want[2]) > 300000 and (want[3]["read_len"] == 0).sum() > 100


@pytest.mark.gpu
def test_byte_totals_are_formed_in_64_bits(bat, cand):
    """One 7600-byte read and 300 000 candidates that name it: 2.28e9 read bytes are DSA_E_LIMIT, by both entries, before
    anything of that size is allocated, and the batch object works afterwards.  The total depends on the lookup in a store,
    and a store exists only on a device (bat_reads_create has no CPU path), so this is a GPU test."""
    rdict = {cand.read_id(1, 0): b"ACGT" * 1900}
    wdict = {9: (b"ACGT", b"TTTT")}
    cands = cands_of(cand, [(9, 1, 0, k & 1) for k in range(300000)])
    assert 7600 * len(cands) > 2 ** 31 - 1
    with bat.Reads.from_dict(rdict) as r, bat.Windows.from_dict(wdict) as w, bat.Batch() as b:
        with pytest.raises(bat.BatError) as e:
            b.assemble(r, w, cands)
        assert e.value.code == E_LIMIT and str(7600 * len(cands)) in str(e.value)
        with DeviceArray(cands) as dev:
            with pytest.raises(bat.BatError) as e:
                b.assemble_device(r, w, dev.ptr, len(cands))
        assert e.value.code == E_LIMIT and str(7600 * len(cands)) in str(e.value)
        assert b.view().n_pairs == 0
        check_both_entries(bat, cand, b, r, w, cands[:1000], rdict, wdict)


# ---------------------------------------------------------------------------------------------- GPU: dsa_upload_device
def thinned_batch(n_fusions, seed):
    """synth.make_batch with 5 reads per fusion of which 1-5 are kept (the read bytes of the others stay where they are)."""
    from defuse_amd import synth
    ref, fus, reads, pairs = synth.make_batch(n_fusions, 5, lq=76, lr=389, seed=seed)
    rng = np.random.default_rng(seed)
    keep = (np.arange(len(pairs)) % 5 == 0) | (rng.random(len(pairs)) < 0.5)
    return ref, fus, reads, pairs[keep].copy()


class DeviceBatch:
    """The four arrays of a batch in device memory, with the fields dsa.Context.upload_device reads."""

    def __init__(self, ref, fus, reads, pairs):
        self.arrays = [DeviceArray(a) for a in (ref, fus, reads, pairs)]
        self.ref_bytes, self.fusions, self.read_bytes, self.pairs = (a.ptr for a in self.arrays)
        self.ref_bytes_len, self.n_fusions, self.read_bytes_len, self.n_pairs = len(ref), len(fus), len(reads), len(pairs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for a in self.arrays:
            a.__exit__()


@pytest.mark.gpu
def test_upload_device_equals_upload(gpu_ctx):
    a, other = thinned_batch(300, 2), thinned_batch(120, 3)
    assert 300 < len(a[3]) < 1500

    def run_again():                   # the counts of a run depend on the run before it: both sides follow a run of `a`
        n = gpu_ctx.run()
        gpu_ctx.plan()
        assert gpu_ctx.run() == n
        return gpu_ctx.download(), gpu_ctx.tile_cols_in_use(), gpu_ctx.kernel_counts()
    gpu_ctx.upload(*a)
    want = run_again()
    assert len(want[0]) > len(a[3])
    with DeviceBatch(*a) as dev:
        gpu_ctx.upload_device(dev)
        got = run_again()
        assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:]
        assert len(np.unique(got[0]["pair_idx"])) > 0.5 * len(a[3])
        gpu_ctx.upload(*other)                                                  # a host upload in between
        gpu_ctx.run()
        other_want = gpu_ctx.download()
        gpu_ctx.upload_device(dev)
        assert gpu_ctx.run() == len(want[0]) and gpu_ctx.download().tobytes() == want[0].tobytes()
    with DeviceBatch(*other) as dev:                                            # the first copy is freed: the ctx has its own
        gpu_ctx.upload_device(dev)
    assert gpu_ctx.run() == len(other_want) and gpu_ctx.download().tobytes() == other_want.tobytes()
    empty = (np.zeros(0, np.uint8), a[1][:0], np.zeros(0, np.uint8), a[3][:0])
    with DeviceBatch(*empty) as dev:
        gpu_ctx.upload_device(dev)
        assert gpu_ctx.run() == 0 and len(gpu_ctx.download()) == 0


@pytest.mark.gpu
def test_upload_device_refusals(gpu_ctx):
    from defuse_amd import dsa, synth
    ref, fus, reads, pairs = synth.make_batch(40, 3, lq=76, lr=389, seed=5)
    assert len(reads) > 7601
    gpu_ctx.upload(ref, fus, reads, pairs)
    gpu_ctx.run()
    want = gpu_ctx.download()

    def refused(fus2, pairs2, device):
        with pytest.raises(dsa.DsaError) as e:
            if device:
                with DeviceBatch(ref, fus2, reads, pairs2) as dev:
                    gpu_ctx.upload_device(dev)
            else:
                gpu_ctx.upload(ref, fus2, reads, pairs2)
        m = re.search(r"(pair|fusion) (\d+):", str(e.value))
        return e.value.code, m.group(1), int(m.group(2))

    def both(fus2, pairs2, expect):
        assert refused(fus2, pairs2, False) == expect                          # the host entry is the yardstick
        assert refused(fus2, pairs2, True) == expect
        with DeviceBatch(ref, fus, reads, pairs) as dev:                        # and the ctx aligns a good batch afterwards
            gpu_ctx.upload_device(dev)
        assert gpu_ctx.run() == len(want) and gpu_ctx.download().tobytes() == want.tobytes()

    p = pairs.copy()
    p["fusion_idx"][17] = -1
    both(fus, p, (E_ARG, "pair", 17))
    p = pairs.copy()
    p["fusion_idx"][88] = len(fus)
    p["fusion_idx"][31] = len(fus)
    both(fus, p, (E_ARG, "pair", 31))
    p = pairs.copy()
    p["read_off"][[60, 119]] = len(reads) - 76 + 1                               # one byte beyond reads_len
    both(fus, p, (E_ARG, "pair", 60))
    f = fus.copy()
    f["ref1_len"][39] += 1                                                      # the last window: one byte beyond ref_len
    f["ref0_off"][12] = len(ref)
    both(f, pairs, (E_ARG, "fusion", 12))
    p = pairs.copy()
    p["fusion_idx"][3] = -1                                                     # a bad fusion comes before any pair
    both(f, p, (E_ARG, "fusion", 12))
    # beyond the 16-bit kernels: the host entry takes the 32-bit path, the device entry says where such a batch goes
    p = pairs.copy()
    p["read_off"][[5, 70]] = 0
    p["read_len"][[5, 70]] = 7601
    code, what, k = refused(fus, p, True)
    assert (code, what, k) == (E_LIMIT, "pair", 5)
    assert "dsa_upload" in gpu_ctx.lib.dsa_last_error(gpu_ctx.h).decode()
    p["read_len"][[5, 70]] = 7600                                              # the longest read they take
    with DeviceBatch(ref, fus, reads, p) as dev:
        gpu_ctx.upload_device(dev)
    n = gpu_ctx.run()
    got = gpu_ctx.download()
    gpu_ctx.upload(ref, fus, reads, p)
    assert gpu_ctx.run() == n and gpu_ctx.download().tobytes() == got.tobytes()
    with DeviceBatch(ref, fus, reads, pairs) as dev:
        gpu_ctx.upload_device(dev)
    assert gpu_ctx.run() == len(want) and gpu_ctx.download().tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- GPU: the chain
@pytest.mark.gpu
def test_smoke_vector_resident_chain(bat, cand, gpu_ctx, ectx):
    """SAM records up; candidates, batch and DP records stay on the device; groups and kept records (and, for the check,
    the records) come down.  Set up as test_candidates.test_smoke_vector_through_the_library."""
    from oracle import dosplitalign_oracle as ora
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
    exp = [tuple(int(x) for x in l.split()) for l in open(d + "expected.split.align.txt")]
    lines_of = lambda recs: [tuple(int(r[f]) for f in recs.dtype.names[:9]) for r in recs]

    def resident(session, part, order, b, r, w):
        """One batch through the resident chain: (candidates as downloaded for the check, records, groups, kept)."""
        ptr, n = session.enumerate_device(part, order)
        assert session.timing.download_ms == 0 and session.timing.n_kept == n
        cands = from_device(ptr, n, cand.RECORD_DTYPE)
        view = b.assemble_device(r, w, ptr, n)
        assert_same_batch(b.fetch(), cand.dsa_batch(cands, reads, windows))
        gpu_ctx.upload_device(view)
        n_rec = gpu_ctx.run()
        with DeviceArray(np.zeros(n_rec, dtype=np.dtype("V40"))) as dev:
            assert gpu_ctx.records_to_device(dev.ptr, n_rec) == n_rec
            groups, kept = ectx.evaluate_device(dev.ptr, n_rec)
        return cands, gpu_ctx.download(), groups, kept

    with cand.Table(cand.regions(regs)) as table, bat.Reads.from_dict(reads) as r, bat.Windows.from_dict(windows) as w, bat.Batch() as b:
        for order in (cand.ORDER_VISIT, cand.ORDER_FUSION):
            with table.session() as s:
                host_cands = s.enumerate(als, order)
            assert len(host_cands) > 5
            host_recs = gpu_ctx.align_batch(*cand.dsa_batch(host_cands, reads, windows))
            host_groups, host_kept = ectx.evaluate(host_recs)
            with table.session() as s:
                cands, recs, groups, kept = resident(s, als, order, b, r, w)
            assert cands.tobytes() == host_cands.tobytes()
            if order == cand.ORDER_VISIT:
                assert lines_of(recs) == exp                                     # the reference's own order, no sort needed
            assert sorted(lines_of(recs)) == sorted(exp)
            assert recs.tobytes() == host_recs.tobytes()
            assert groups.tobytes() == host_groups.tobytes() and kept.tobytes() == host_kept.tobytes() and len(groups) > 0
            # the alignments in two calls of one session, each a batch of its own: the union of the records is the same
            half = len(als) // 2
            with table.session() as s:
                parts = [resident(s, als[lo:hi], order, b, r, w) for lo, hi in ((0, half), (half, len(als)))]
            assert len(parts[0][0]) and len(parts[1][0]) and len(parts[0][0]) + len(parts[1][0]) == len(host_cands)
            assert sorted(lines_of(parts[0][1]) + lines_of(parts[1][1])) == sorted(exp)
