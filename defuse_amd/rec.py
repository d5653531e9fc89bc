"""ctypes binding of include/defuse_rec.h (the record store: the records of many batches sorted on the GPU into the order of
the pipeline's `sort -n -k 1`, and their lines printed); test/bench plumbing only.

In a process that also uses PyTorch-ROCm, import torch and let it touch the GPU before this module loads the library
(README)."""
import ctypes

import numpy as np

from . import capi
from .capi import ptr as _ptr
from .dsa import RECORD_DTYPE, DsaError, load_library

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
FIELDS = RECORD_DTYPE.names[:9]      # the printed fields, in print order (pair_idx is not printed)
MAX_LINE = 109

EXPORTS = ["rec_create", "rec_destroy", "rec_clear", "rec_append", "rec_append_device", "rec_tail", "rec_commit", "rec_sort", "rec_count",
           "rec_records_device", "rec_download", "rec_text", "rec_get_timing", "rec_last_error"]


class RecTiming(ctypes.Structure):
    _fields_ = [("append_ms", ctypes.c_float), ("keys_ms", ctypes.c_float), ("sort_ms", ctypes.c_float), ("gather_ms", ctypes.c_float),
                ("format_ms", ctypes.c_float), ("write_ms", ctypes.c_float), ("download_ms", ctypes.c_float), ("pad_", ctypes.c_float),
                ("n_records", ctypes.c_int64), ("n_sorts", ctypes.c_int64), ("text_bytes", ctypes.c_int64)]


STRUCTS = {"rec_timing": RecTiming}

p, i64, cint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "rec_create": (cint, [cint, ctypes.POINTER(p)]),
    "rec_destroy": (None, [p]),
    "rec_clear": (cint, [p]),
    "rec_append": (cint, [p, p, i64]),
    "rec_append_device": (cint, [p, p, i64]),
    "rec_tail": (cint, [p, i64, ctypes.POINTER(p)]),
    "rec_commit": (cint, [p, i64]),
    "rec_sort": (cint, [p]),
    "rec_count": (cint, [p, ctypes.POINTER(i64)]),
    "rec_records_device": (cint, [p, ctypes.POINTER(p), ctypes.POINTER(i64)]),
    "rec_download": (cint, [p, p, i64, ctypes.POINTER(i64)]),
    "rec_text": (cint, [p, p, i64, p, i64, ctypes.POINTER(i64)]),
    "rec_get_timing": (cint, [p, ctypes.POINTER(RecTiming)]),
    "rec_last_error": (ctypes.c_char_p, []),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_rec.h bound."""
    return _bind(load_library())


class Store(capi.Owned):
    """One rec_store (one device); close() or a with-block frees its device buffers.  No CPU path: raises without a GPU."""
    _destroy = "rec_destroy"
    h = property(lambda self: self.handle)      # the older spelling of .handle and ._lib
    lib = property(lambda self: self._lib)

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.rec_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            raise DsaError(rc, "rec_create: " + self._lib.rec_last_error().decode())

    def _check(self, rc):
        if rc != 0:
            raise DsaError(rc, self._lib.rec_last_error().decode())

    def clear(self):
        self._check(self._lib.rec_clear(self.handle))

    def append(self, records):
        """rec_append of a structured array with the layout of dsa_record (dsa.RECORD_DTYPE)."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        self._check(self._lib.rec_append(self.handle, _ptr(records), len(records)))

    def append_device(self, ptr, n):
        """rec_append_device: n records at a device pointer (an int) of the store's device, their producer completed."""
        self._check(self._lib.rec_append_device(self.handle, ctypes.c_void_p(ptr), int(n)))

    def tail(self, room):
        """rec_tail: the device pointer (an int) of room for `room` records behind the last one; commit(n) adds n of them."""
        p = ctypes.c_void_p()
        self._check(self._lib.rec_tail(self.handle, int(room), ctypes.byref(p)))
        return p.value

    def commit(self, n):
        self._check(self._lib.rec_commit(self.handle, int(n)))

    def sort(self):
        self._check(self._lib.rec_sort(self.handle))

    def __len__(self):
        n = ctypes.c_int64()
        self._check(self._lib.rec_count(self.handle, ctypes.byref(n)))
        return n.value

    def records_device(self):
        """(device pointer as an int, n): what eval.Context.evaluate_device takes."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self._lib.rec_records_device(self.handle, ctypes.byref(p), ctypes.byref(n)))
        return p.value or 0, n.value

    def download(self):
        n = ctypes.c_int64()
        out = np.zeros(len(self), RECORD_DTYPE)
        self._check(self._lib.rec_download(self.handle, _ptr(out), len(out), ctypes.byref(n)))
        return out

    def text(self, kept=None, cap=None):
        """rec_text as bytes: every record's line in store order, or the lines of the records kept[...] in the list's order.
        Without cap the buffer has room for the longest possible text, so the device prints once; with it the call is made
        as given and a DsaError carries the code and, for DSA_E_CAPACITY, the required size (bytes)."""
        kp, nk, m = None, 0, len(self)
        if kept is not None:
            kept = np.ascontiguousarray(kept, dtype=np.int64)
            hold = kept if len(kept) else np.zeros(1, np.int64)      # an empty list is still a list: a pointer that is not NULL
            kp, nk, m = hold.ctypes.data, len(kept), len(kept)
        size = m * MAX_LINE if cap is None else int(cap)
        buf = np.empty(max(size, 1), np.uint8)
        got = ctypes.c_int64()
        rc = self._lib.rec_text(self.handle, kp, nk, buf.ctypes.data, size, ctypes.byref(got))
        if rc != 0:
            e = DsaError(rc, self._lib.rec_last_error().decode())
            e.bytes = got.value
            raise e
        return buf[:got.value].tobytes()

    def timing(self):
        t = RecTiming()
        self._check(self._lib.rec_get_timing(self.handle, ctypes.byref(t)))
        return capi.as_dict(t)
