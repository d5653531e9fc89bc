"""ctypes binding of include/defuse_cand.h (the candidate loop of DoAlignment on the GPU); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi, dsa
from .capi import ptr as _ptr
from .dsa import load_library

BIN_SPACING = 2000              # CAND_BIN_SPACING
ORDER_VISIT, ORDER_FUSION = 0, 1
DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT


class Region(ctypes.Structure):
    _fields_ = [("ref", ctypes.c_int32), ("strand", ctypes.c_int32), ("start", ctypes.c_int32), ("end", ctypes.c_int32),
                ("id", ctypes.c_int32)]


class Alignment(ctypes.Structure):
    _fields_ = [("ref", ctypes.c_int32), ("strand", ctypes.c_int32), ("start", ctypes.c_int32), ("end", ctypes.c_int32),
                ("fragment", ctypes.c_int32), ("read_end", ctypes.c_int32)]


class Record(ctypes.Structure):
    _fields_ = [("alignment", ctypes.c_int64), ("fusion_id", ctypes.c_int32), ("fragment", ctypes.c_int32),
                ("cluster_end", ctypes.c_uint8), ("read_end", ctypes.c_uint8), ("revcomp", ctypes.c_uint8),
                ("first", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 4)]


class CandTiming(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_float), ("device_ms", ctypes.c_float), ("download_ms", ctypes.c_float),
                ("pad_", ctypes.c_float), ("n_alignments", ctypes.c_int64), ("n_hits", ctypes.c_int64),
                ("n_visited", ctypes.c_int64), ("n_kept", ctypes.c_int64)]


STRUCTS = {"cand_region": Region, "cand_alignment": Alignment, "cand_record": Record, "cand_timing": CandTiming}
REGION_DTYPE = np.dtype(Region)
ALIGNMENT_DTYPE = np.dtype(Alignment)
RECORD_DTYPE = np.dtype(Record)

EXPORTS = ["cand_cluster_id", "cand_table_create", "cand_table_destroy", "cand_session_create", "cand_session_reset",
           "cand_session_destroy", "cand_enumerate", "cand_last_error"]


class CandError(capi.ApiError):
    prefix = "cand"


p, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "cand_cluster_id": (cint, [i64, i32, ctypes.POINTER(i32)]),
    "cand_table_create": (cint, [cint, p, i64, i32, ctypes.POINTER(p)]),
    "cand_table_destroy": (None, [p]),
    "cand_session_create": (cint, [p, ctypes.POINTER(p)]),
    "cand_session_reset": (cint, [p]),
    "cand_session_destroy": (None, [p]),
    "cand_enumerate": (cint, [p, p, i64, i32, p, i64, ctypes.POINTER(i64), ctypes.POINTER(CandTiming)]),
    "cand_last_error": (ctypes.c_char_p, []),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_cand.h bound."""
    return _bind(load_library())


def _fail(lib, what, rc):
    raise CandError(rc, "%s: %s" % (what, lib.cand_last_error().decode()))


def cluster_id(fusion_id, cluster_end):
    """ClusterID.id of (fusion, cluster end) (cand_cluster_id); raises CandError(DSA_E_ARG) for a fusion id outside [0, 2^31)."""
    out = ctypes.c_int32()
    rc = lib().cand_cluster_id(int(fusion_id), int(cluster_end), ctypes.byref(out))
    if rc != 0:
        _fail(lib(), "cand_cluster_id", rc)
    return out.value


def read_id(fragment, read_end):
    """ReadID.id, the key of the reference's read map: fragment in bits 0-30, read end in bit 31, as a signed int."""
    v = (int(fragment) & 0x7FFFFFFF) | (int(read_end) << 31)
    return v - (1 << 32) if v >= (1 << 31) else v


def regions(rows):
    """Rows (ref, strand, start, end, id) -> REGION_DTYPE array."""
    return np.array([tuple(r) for r in rows], dtype=REGION_DTYPE).reshape(-1)


def alignments(rows):
    """Rows (ref, strand, start, end, fragment, read_end) -> ALIGNMENT_DTYPE array."""
    return np.array([tuple(r) for r in rows], dtype=ALIGNMENT_DTYPE).reshape(-1)


class Table(capi.Owned):
    """The binned mate regions on one device (cand_table_create); close() or a with-block frees them, after the sessions."""
    _destroy = "cand_table_destroy"

    def __init__(self, regs, bin_spacing=BIN_SPACING, device=0):
        super().__init__(lib())
        r = np.ascontiguousarray(regs, dtype=REGION_DTYPE)
        rc = self._lib.cand_table_create(device, _ptr(r), len(r), int(bin_spacing), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "cand_table_create", rc)

    def session(self):
        return Session(self)


class Session(capi.Owned):
    """What one DoAlignment run has kept so far (cand_session_create)."""
    _destroy = "cand_session_destroy"

    def __init__(self, table):
        super().__init__(table._lib)
        self._table = table                                  # the table outlives its sessions
        rc = self._lib.cand_session_create(table.handle, ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "cand_session_create", rc)
        self.timing = CandTiming()

    def count(self, als, order=ORDER_VISIT):
        """The number of candidates cand_enumerate would keep; the session is left as it was (cap = 0, out = NULL)."""
        a = np.ascontiguousarray(als, dtype=ALIGNMENT_DTYPE)
        n = ctypes.c_int64()
        rc = self._lib.cand_enumerate(self.handle, _ptr(a), len(a), order, None, 0, ctypes.byref(n), ctypes.byref(self.timing))
        if rc not in (0, DSA_E_CAPACITY):
            _fail(self._lib, "cand_enumerate", rc)
        return rc, n.value

    def enumerate_into(self, als, out, order=ORDER_VISIT):
        """cand_enumerate into the RECORD_DTYPE array `out`: (return code, count).  Raises only on codes other than
        DSA_E_CAPACITY."""
        a = np.ascontiguousarray(als, dtype=ALIGNMENT_DTYPE)
        assert out.dtype == RECORD_DTYPE and out.flags.c_contiguous
        n = ctypes.c_int64()
        rc = self._lib.cand_enumerate(self.handle, _ptr(a), len(a), order, _ptr(out), len(out), ctypes.byref(n), ctypes.byref(self.timing))
        if rc not in (0, DSA_E_CAPACITY):
            _fail(self._lib, "cand_enumerate", rc)
        return rc, n.value

    def enumerate(self, als, order=ORDER_VISIT):
        """The kept candidates of the alignments as a RECORD_DTYPE array (a counting call, then one with room); the timing
        of the second call is in self.timing."""
        rc, n = self.count(als, order)
        out = np.zeros(n, dtype=RECORD_DTYPE)
        if rc == 0 and n == 0:
            return out                                       # already committed: nothing was kept
        rc, n2 = self.enumerate_into(als, out, order)
        if rc != 0 or n2 != n:
            _fail(self._lib, "cand_enumerate", rc)
        return out

    def enumerate_device(self, als, order=ORDER_VISIT):
        """cand_enumerate_device: the kept candidates stay in the session's device buffer.  Returns (device pointer, count)
        from cand_records_device, valid until the next call on this session; the timing is in self.timing."""
        from . import bat                                    # (bat imports this module: its header declares the two device twins)
        bat.lib()
        a = np.ascontiguousarray(als, dtype=ALIGNMENT_DTYPE)
        n = ctypes.c_int64()
        rc = self._lib.cand_enumerate_device(self.handle, _ptr(a), len(a), order, ctypes.byref(n), ctypes.byref(self.timing))
        if rc != 0:
            _fail(self._lib, "cand_enumerate_device", rc)
        dev, m = ctypes.c_void_p(), ctypes.c_int64()
        rc = self._lib.cand_records_device(self.handle, ctypes.byref(dev), ctypes.byref(m))
        if rc != 0 or m.value != n.value:
            _fail(self._lib, "cand_records_device", rc)
        return dev.value or 0, n.value

    def reset(self):
        rc = self._lib.cand_session_reset(self.handle)
        if rc != 0:
            _fail(self._lib, "cand_session_reset", rc)


_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACTGactg", b"TGACtgac"):                 # tools/Common.cpp:32-54: every other byte stays
    _COMPLEMENT[_a] = _b


def reverse_complement(seq):
    """uint8 array of the reverse complement of the bytes `seq`."""
    return _COMPLEMENT[np.frombuffer(seq, dtype=np.uint8)[::-1]]


def dsa_batch(cands, reads, windows):
    """Kept candidates -> (ref_bytes, fusions, read_bytes, pairs) of defuse_amd.dsa, pairs in the order of `cands`.

    reads: {read_id(fragment, read_end): bytes}; a read that is missing aligns as the empty string, as the reference's map
    lookup gives it (tools/SplitAlignment.cpp:286).  windows: {fusion_id: (mSplitAlignSeq[0], mSplitAlignSeq[1])}.  A
    fusion enters `fusions` when its first candidate is met; the reads are reverse-complemented where revcomp is set."""
    ref, fusions, fidx = [], [], {}
    seqs, pairs = [], []
    ref_off = read_off = 0
    for c in cands:
        fid = int(c["fusion_id"])
        if fid not in fidx:
            w0, w1 = windows[fid]
            fidx[fid] = len(fusions)
            fusions.append((fid, ref_off, len(w0), ref_off + len(w0), len(w1)))
            ref += [np.frombuffer(w0, dtype=np.uint8), np.frombuffer(w1, dtype=np.uint8)]
            ref_off += len(w0) + len(w1)
        seq = reads.get(read_id(c["fragment"], c["read_end"]), b"")
        s = reverse_complement(seq) if c["revcomp"] else np.frombuffer(seq, dtype=np.uint8)
        pairs.append((fidx[fid], read_off, len(s), int(c["fragment"]), int(c["read_end"]), int(c["revcomp"]), (0, 0)))
        seqs.append(s)
        read_off += len(s)
    cat = lambda parts: np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, dtype=np.uint8)
    return cat(ref), np.array(fusions, dtype=dsa.FUSION_DTYPE).reshape(-1), cat(seqs), np.array(pairs, dtype=dsa.PAIR_DTYPE).reshape(-1)
