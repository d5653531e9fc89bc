"""ctypes binding of include/defuse_bat.h (the batch assembly between cand and dsa on the GPU); test/bench plumbing only."""
import ctypes

import numpy as np

from . import cand, capi, dsa
from .capi import ptr as _ptr
from .dsa import load_library      # noqa: F401  (bat.load_library() is what callers of _bind pass)

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT


class Read(ctypes.Structure):
    _fields_ = [("off", ctypes.c_int64), ("len", ctypes.c_int32), ("fragment", ctypes.c_int32), ("read_end", ctypes.c_int32),
                ("pad_", ctypes.c_int32)]


class View(ctypes.Structure):
    """bat_view: the assembled batch on the device, the arguments of dsa_upload_device in its order."""
    _fields_ = [("ref_bytes", ctypes.c_void_p), ("fusions", ctypes.c_void_p), ("read_bytes", ctypes.c_void_p), ("pairs", ctypes.c_void_p),
                ("ref_bytes_len", ctypes.c_int64), ("read_bytes_len", ctypes.c_int64), ("n_pairs", ctypes.c_int64),
                ("n_fusions", ctypes.c_int32), ("device", ctypes.c_int32)]


class BatTiming(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_float), ("lookup_ms", ctypes.c_float), ("scan_ms", ctypes.c_float), ("gather_ms", ctypes.c_float),
                ("n_candidates", ctypes.c_int64), ("n_fusions", ctypes.c_int64), ("read_bytes", ctypes.c_int64), ("ref_bytes", ctypes.c_int64)]


STRUCTS = {"bat_read": Read, "bat_view": View, "bat_timing": BatTiming}
READ_DTYPE = np.dtype(Read)

# every function include/defuse_bat.h declares: its own, and the device twins of cand_enumerate
EXPORTS = ["bat_reads_create", "bat_reads_destroy", "bat_windows_create", "bat_windows_destroy", "bat_batch_create", "bat_batch_destroy",
           "bat_assemble", "bat_assemble_device", "bat_batch_view", "bat_batch_fetch", "bat_get_timing", "bat_last_error",
           "cand_enumerate_device", "cand_records_device"]


class BatError(capi.ApiError):
    prefix = "bat"


p, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "bat_reads_create": (cint, [cint, p, i64, p, i64, ctypes.POINTER(p)]),
    "bat_reads_destroy": (None, [p]),
    "bat_windows_create": (cint, [cint, p, i64, p, i32, ctypes.POINTER(p)]),
    "bat_windows_destroy": (None, [p]),
    "bat_batch_create": (cint, [cint, ctypes.POINTER(p)]),
    "bat_batch_destroy": (None, [p]),
    "bat_assemble": (cint, [p, p, p, i64, p]),
    "bat_assemble_device": (cint, [p, p, p, i64, p]),
    "bat_batch_view": (cint, [p, ctypes.POINTER(View)]),
    "bat_batch_fetch": (cint, [p, p, i64, p, i64, p, i64, p, i64]),
    "bat_get_timing": (cint, [p, ctypes.POINTER(BatTiming)]),
    "bat_last_error": (ctypes.c_char_p, []),
    "cand_enumerate_device": (cint, [p, p, i64, i32, ctypes.POINTER(i64), ctypes.POINTER(cand.CandTiming)]),
    "cand_records_device": (cint, [p, ctypes.POINTER(p), ctypes.POINTER(i64)]),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_bat.h, and of defuse_cand.h before it, bound."""
    return _bind(cand.lib())


def _fail(lib, what, rc):
    raise BatError(rc, "%s: %s" % (what, lib.bat_last_error().decode()))


def pack_reads(reads):
    """{cand.read_id(fragment, read_end): bytes} or a sequence of (fragment, read_end, bytes) -> (bytes, READ_DTYPE array), one
    record per entry in its order, the sequences back to back."""
    if isinstance(reads, dict):
        reads = [(k & 0x7FFFFFFF, 1 if k < 0 else 0, v) for k, v in reads.items()]
    recs = np.zeros(len(reads), dtype=READ_DTYPE)
    off = 0
    for k, (frag, rend, seq) in enumerate(reads):
        recs[k] = (off, len(seq), frag, rend, 0)
        off += len(seq)
    return np.frombuffer(b"".join(bytes(seq) for _, _, seq in reads), dtype=np.uint8), recs


def pack_windows(windows):
    """{fusion_id: (window 0, window 1)} -> (ref_bytes, dsa.FUSION_DTYPE array), in the order of the dict."""
    fus = np.zeros(len(windows), dtype=dsa.FUSION_DTYPE)
    off = 0
    for k, (fid, (w0, w1)) in enumerate(windows.items()):
        fus[k] = (fid, off, len(w0), off + len(w0), len(w1))
        off += len(w0) + len(w1)
    return np.frombuffer(b"".join(bytes(w0) + bytes(w1) for w0, w1 in windows.values()), dtype=np.uint8), fus


class Reads(capi.Owned):
    """The reads of a run on one device (bat_reads_create): `data` uint8, `recs` READ_DTYPE, or see from_dict."""
    _destroy = "bat_reads_destroy"

    def __init__(self, data, recs, device=0):
        super().__init__(lib())
        data = np.ascontiguousarray(data, dtype=np.uint8)
        recs = np.ascontiguousarray(recs, dtype=READ_DTYPE)
        rc = self._lib.bat_reads_create(device, _ptr(data), data.size, _ptr(recs), len(recs), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "bat_reads_create", rc)

    @classmethod
    def from_dict(cls, reads, device=0):
        return cls(*pack_reads(reads), device=device)


class Windows(capi.Owned):
    """Both windows of every task on one device (bat_windows_create): `ref_bytes` uint8, `fusions` dsa.FUSION_DTYPE."""
    _destroy = "bat_windows_destroy"

    def __init__(self, ref_bytes, fusions, device=0):
        super().__init__(lib())
        ref_bytes = np.ascontiguousarray(ref_bytes, dtype=np.uint8)
        fusions = np.ascontiguousarray(fusions, dtype=dsa.FUSION_DTYPE)
        rc = self._lib.bat_windows_create(device, _ptr(ref_bytes), ref_bytes.size, _ptr(fusions), len(fusions), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "bat_windows_create", rc)

    @classmethod
    def from_dict(cls, windows, device=0):
        return cls(*pack_windows(windows), device=device)


class Batch(capi.Owned):
    """The device buffers of an assembled batch (bat_batch_create), reused call after call."""
    _destroy = "bat_batch_destroy"

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.bat_batch_create(device, ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "bat_batch_create", rc)

    def assemble(self, reads, windows, cands):
        """bat_assemble of a cand.RECORD_DTYPE array in host memory; returns the view."""
        c = np.ascontiguousarray(cands, dtype=cand.RECORD_DTYPE)
        rc = self._lib.bat_assemble(reads.handle, windows.handle, _ptr(c), len(c), self.handle)
        if rc != 0:
            _fail(self._lib, "bat_assemble", rc)
        return self.view()

    def assemble_device(self, reads, windows, cands_ptr, n):
        """bat_assemble_device of n records at a device pointer (cand.Session.enumerate_device); returns the view."""
        rc = self._lib.bat_assemble_device(reads.handle, windows.handle, ctypes.c_void_p(cands_ptr), int(n), self.handle)
        if rc != 0:
            _fail(self._lib, "bat_assemble_device", rc)
        return self.view()

    def view(self):
        v = View()
        rc = self._lib.bat_batch_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "bat_batch_view", rc)
        return v

    def fetch(self):
        """(ref_bytes, fusions, read_bytes, pairs) as numpy arrays: the tuple cand.dsa_batch returns."""
        v = self.view()
        ref = np.zeros(v.ref_bytes_len, dtype=np.uint8)
        fus = np.zeros(v.n_fusions, dtype=dsa.FUSION_DTYPE)
        reads = np.zeros(v.read_bytes_len, dtype=np.uint8)
        pairs = np.zeros(v.n_pairs, dtype=dsa.PAIR_DTYPE)
        rc = self._lib.bat_batch_fetch(self.handle, _ptr(ref), len(ref), _ptr(fus), len(fus), _ptr(reads), len(reads), _ptr(pairs), len(pairs))
        if rc != 0:
            _fail(self._lib, "bat_batch_fetch", rc)
        return ref, fus, reads, pairs

    def timing(self):
        t = BatTiming()
        self._lib.bat_get_timing(self.handle, ctypes.byref(t))
        return t
