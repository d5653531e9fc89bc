"""ctypes binding of include/defuse_text.h (the improper-mate SAM text and the reads' FASTQ text parsed on the GPU, and the
device-pointer twins of cand_enumerate and bat_reads_create); test/bench plumbing only."""
import ctypes

import numpy as np

from . import bat, cand, capi
from .capi import ptr as _ptr
from .dsa import load_library      # noqa: F401  (text.load_library() is what callers of _bind pass)

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
MAX_READ_LEN = 1 << 24                                  # TXT_MAX_READ_LEN
SAM_EMPTY_LINE, SAM_FEW_FIELDS, SAM_BAD_INTEGER, SAM_BAD_QNAME = 2, 3, 4, 5
FASTQ_BAD_NAME, FASTQ_BAD_END, FASTQ_BAD_FRAGMENT, FASTQ_LONG_READ = 1, 2, 3, 4

ALIGNMENT_DTYPE = cand.ALIGNMENT_DTYPE
READ_DTYPE = bat.READ_DTYPE


class SamResult(ctypes.Structure):
    _fields_ = [("consumed", ctypes.c_int64), ("n_lines", ctypes.c_int64), ("n_alignments", ctypes.c_int64), ("stop_line", ctypes.c_int64),
                ("n_bad_fragment", ctypes.c_int64), ("stop_kind", ctypes.c_int32), ("carry_out", ctypes.c_int32)]


class SamView(ctypes.Structure):
    _fields_ = [("alignments", ctypes.c_void_p), ("line_of", ctypes.c_void_p), ("n", ctypes.c_int64), ("device", ctypes.c_int32),
                ("pad_", ctypes.c_int32)]


class FastqResult(ctypes.Structure):
    _fields_ = [("consumed", ctypes.c_int64), ("n_records", ctypes.c_int64), ("n_skipped", ctypes.c_int64), ("stop_line", ctypes.c_int64),
                ("stop_kind", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class FastqView(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_void_p), ("reads", ctypes.c_void_p), ("bytes_len", ctypes.c_int64), ("n_reads", ctypes.c_int64),
                ("device", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class TxtTiming(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_float), ("device_ms", ctypes.c_float), ("download_ms", ctypes.c_float), ("pad_", ctypes.c_float),
                ("text_bytes", ctypes.c_int64), ("n_lines", ctypes.c_int64), ("n_records", ctypes.c_int64), ("gather_bytes", ctypes.c_int64)]


STRUCTS = {"txt_sam_result": SamResult, "txt_sam_device_view": SamView, "txt_fastq_result": FastqResult, "txt_fastq_device_view": FastqView,
           "txt_timing": TxtTiming}
SAM_RESULT_DTYPE = np.dtype(SamResult)
FASTQ_RESULT_DTYPE = np.dtype(FastqResult)

# every function include/defuse_text.h declares: its own, and the device-pointer twins of the two consumers
EXPORTS = ["txt_names_create", "txt_names_destroy", "txt_create", "txt_destroy", "txt_set_max_read_len", "txt_parse_sam", "txt_parse_sam_device",
           "txt_sam_view", "txt_sam_fetch", "txt_fastq_begin", "txt_fastq_add", "txt_fastq_view", "txt_fastq_fetch", "txt_get_timing",
           "txt_last_error", "cand_enumerate_resident", "bat_reads_create_device"]


class TextError(capi.ApiError):
    prefix = "text"


p, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "txt_names_create": (cint, [cint, p, i64, p, i64, ctypes.POINTER(p)]),
    "txt_names_destroy": (None, [p]),
    "txt_create": (cint, [cint, ctypes.POINTER(p)]),
    "txt_destroy": (None, [p]),
    "txt_set_max_read_len": (cint, [p, i32]),
    "txt_parse_sam": (cint, [p, p, p, i64, i32, i32, ctypes.POINTER(SamResult)]),
    "txt_parse_sam_device": (cint, [p, p, p, i64, i32, i32, ctypes.POINTER(SamResult)]),
    "txt_sam_view": (cint, [p, ctypes.POINTER(SamView)]),
    "txt_sam_fetch": (cint, [p, p, i64, p, i64]),
    "txt_fastq_begin": (cint, [p]),
    "txt_fastq_add": (cint, [p, p, i64, i32, ctypes.POINTER(FastqResult)]),
    "txt_fastq_view": (cint, [p, ctypes.POINTER(FastqView)]),
    "txt_fastq_fetch": (cint, [p, p, i64, p, i64]),
    "txt_get_timing": (cint, [p, ctypes.POINTER(TxtTiming)]),
    "txt_last_error": (ctypes.c_char_p, []),
    "cand_enumerate_resident": (cint, [p, p, i64, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(cand.CandTiming)]),
    "bat_reads_create_device": (cint, [cint, p, i64, p, i64, ctypes.POINTER(p)]),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_text.h, and of defuse_bat.h and defuse_cand.h before it, bound."""
    return _bind(bat.lib())


def _fail(lib, what, rc):
    raise TextError(rc, "%s: %s" % (what, lib.txt_last_error().decode()))


def _text(text):
    """bytes or a uint8 array -> a contiguous uint8 array (no copy of an array that already is one)."""
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


def pack_names(names):
    """A sequence of names (bytes or str), index = position -> (name_bytes, name_off)."""
    names = [n if isinstance(n, bytes) else str(n).encode("latin-1") for n in names]
    off = np.zeros(len(names) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(n) for n in names])
    return np.frombuffer(b"".join(names), dtype=np.uint8), off


class Names(capi.Owned):
    """The reference names of a run on one device (txt_names_create): a sequence of names, index = position, the numbering
    of cand_region.ref."""
    _destroy = "txt_names_destroy"

    def __init__(self, names, device=0):
        super().__init__(lib())
        data, off = pack_names(names)
        rc = self._lib.txt_names_create(device, _ptr(data), data.size, off.ctypes.data, len(off) - 1, ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "txt_names_create", rc)


class Context(capi.Owned):
    """One txt_ctx (one device): the alignments of the latest SAM parse and the read store of the FASTQ pieces.  `names` is
    the Names the parses use unless one names another."""
    _destroy = "txt_destroy"

    def __init__(self, names=None, device=0):
        super().__init__(lib())
        self.names = names
        rc = self._lib.txt_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "txt_create", rc)

    # ---- SAM
    def parse_sam(self, text, final=True, carry_in=0, names=None):
        """txt_parse_sam of bytes or a uint8 array; returns the SamResult."""
        t = _text(text)
        res = SamResult()
        rc = self._lib.txt_parse_sam(self.handle, (names or self.names).handle, _ptr(t), len(t), int(final), int(carry_in), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "txt_parse_sam", rc)
        return res

    def parse_sam_device(self, ptr, n, final=True, carry_in=0, names=None):
        """txt_parse_sam_device of n bytes at a device pointer; returns the SamResult."""
        res = SamResult()
        rc = self._lib.txt_parse_sam_device(self.handle, (names or self.names).handle, ctypes.c_void_p(ptr), int(n), int(final), int(carry_in),
                                            ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "txt_parse_sam_device", rc)
        return res

    def sam_view(self):
        v = SamView()
        rc = self._lib.txt_sam_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "txt_sam_view", rc)
        return v

    def sam_alignments(self, lines=False):
        """The alignments of the latest parse as an ALIGNMENT_DTYPE array (txt_sam_fetch); with lines=True also every
        record's 1-based line number."""
        n = self.sam_view().n
        als = np.zeros(n, dtype=ALIGNMENT_DTYPE)
        line_of = np.zeros(n if lines else 0, dtype=np.int32)
        rc = self._lib.txt_sam_fetch(self.handle, _ptr(als), len(als), _ptr(line_of), len(line_of))
        if rc != 0:
            _fail(self._lib, "txt_sam_fetch", rc)
        return (als, line_of) if lines else als

    # ---- FASTQ
    def fastq_begin(self):
        rc = self._lib.txt_fastq_begin(self.handle)
        if rc != 0:
            _fail(self._lib, "txt_fastq_begin", rc)

    def fastq_add(self, text, final=True):
        """txt_fastq_add of one piece of a file; returns the FastqResult."""
        t = _text(text)
        res = FastqResult()
        rc = self._lib.txt_fastq_add(self.handle, _ptr(t), len(t), int(final), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "txt_fastq_add", rc)
        return res

    def set_max_read_len(self, n):
        rc = self._lib.txt_set_max_read_len(self.handle, int(n))
        if rc != 0:
            _fail(self._lib, "txt_set_max_read_len", rc)

    def fastq_view(self):
        v = FastqView()
        rc = self._lib.txt_fastq_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "txt_fastq_view", rc)
        return v

    def fastq_fetch(self):
        """(bytes, reads): the sequences back to back as a uint8 array and a READ_DTYPE array - bat.pack_reads' pair."""
        v = self.fastq_view()
        data = np.zeros(v.bytes_len, dtype=np.uint8)
        reads = np.zeros(v.n_reads, dtype=READ_DTYPE)
        rc = self._lib.txt_fastq_fetch(self.handle, _ptr(data), len(data), _ptr(reads), len(reads))
        if rc != 0:
            _fail(self._lib, "txt_fastq_fetch", rc)
        return data, reads

    def reads_store(self):
        """A bat.Reads made of the store in place (bat_reads_create_device); it copies, so the ctx can be reused."""
        v = self.fastq_view()
        return reads_from_device(v.bytes, v.bytes_len, v.reads, v.n_reads, v.device)

    def timing(self):
        t = TxtTiming()
        rc = self._lib.txt_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "txt_get_timing", rc)
        return capi.as_dict(t)


def reads_from_device(bytes_ptr, bytes_len, reads_ptr, n, device=0):
    """bat_reads_create_device -> a bat.Reads; raises bat.BatError."""
    bound = lib()
    r = bat.Reads.__new__(bat.Reads)
    capi.Owned.__init__(r, bound)
    rc = bound.bat_reads_create_device(int(device), ctypes.c_void_p(bytes_ptr), int(bytes_len), ctypes.c_void_p(reads_ptr), int(n), ctypes.byref(r.handle))
    if rc != 0:
        bat._fail(bound, "bat_reads_create_device", rc)
    return r


def enumerate_resident(session, alignments_ptr, n, order=cand.ORDER_VISIT):
    """cand_enumerate_resident on a cand.Session: n alignments at a device pointer (Context.sam_view).  Returns (device
    pointer, count) of the records as Session.enumerate_device does; a bad alignment raises cand.CandError, whose first_bad
    is the index the call reports (-1: none)."""
    bound = lib()
    n_out, first_bad = ctypes.c_int64(), ctypes.c_int64()
    rc = bound.cand_enumerate_resident(session.handle, ctypes.c_void_p(alignments_ptr), int(n), int(order), ctypes.byref(n_out), ctypes.byref(first_bad),
                                       ctypes.byref(session.timing))
    if rc != 0:
        e = cand.CandError(rc, "cand_enumerate_resident: " + bound.cand_last_error().decode())
        e.first_bad = first_bad.value
        raise e
    dev, m = ctypes.c_void_p(), ctypes.c_int64()
    rc = bound.cand_records_device(session.handle, ctypes.byref(dev), ctypes.byref(m))
    if rc != 0 or m.value != n_out.value:
        cand._fail(bound, "cand_records_device", rc)
    return dev.value or 0, n_out.value
