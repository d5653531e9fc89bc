"""ctypes binding of include/defuse_rec.h (the record store: the records of many batches sorted on the GPU into the order of
the pipeline's `sort -n -k 1`, and their lines printed); test/bench plumbing only.

In a process that also uses PyTorch-ROCm, import torch and let it touch the GPU before this module loads the library
(README)."""
import ctypes

import numpy as np

from .dsa import DSA_E_CAPACITY, RECORD_DTYPE, DsaError, load_library

DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = -2, -3, -4
FIELDS = RECORD_DTYPE.names[:9]      # the printed fields, in print order (pair_idx is not printed)
MAX_LINE = 109

EXPORTS = ["rec_create", "rec_destroy", "rec_clear", "rec_append", "rec_append_device", "rec_tail", "rec_commit", "rec_sort", "rec_count",
           "rec_records_device", "rec_download", "rec_text", "rec_get_timing", "rec_last_error"]


class RecTiming(ctypes.Structure):
    _fields_ = [("append_ms", ctypes.c_float), ("keys_ms", ctypes.c_float), ("sort_ms", ctypes.c_float), ("gather_ms", ctypes.c_float),
                ("format_ms", ctypes.c_float), ("write_ms", ctypes.c_float), ("download_ms", ctypes.c_float), ("pad_", ctypes.c_float),
                ("n_records", ctypes.c_int64), ("n_sorts", ctypes.c_int64), ("text_bytes", ctypes.c_int64)]


def _bind(lib):
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.rec_create.argtypes = [ctypes.c_int, ctypes.POINTER(p)]
    lib.rec_destroy.argtypes = [p]
    lib.rec_destroy.restype = None
    lib.rec_clear.argtypes = [p]
    lib.rec_append.argtypes = [p, p, i64]
    lib.rec_append_device.argtypes = [p, p, i64]
    lib.rec_tail.argtypes = [p, i64, ctypes.POINTER(p)]
    lib.rec_commit.argtypes = [p, i64]
    lib.rec_sort.argtypes = [p]
    lib.rec_count.argtypes = [p, ctypes.POINTER(i64)]
    lib.rec_records_device.argtypes = [p, ctypes.POINTER(p), ctypes.POINTER(i64)]
    lib.rec_download.argtypes = [p, p, i64, ctypes.POINTER(i64)]
    lib.rec_text.argtypes = [p, p, i64, p, i64, ctypes.POINTER(i64)]
    lib.rec_get_timing.argtypes = [p, ctypes.POINTER(RecTiming)]
    lib.rec_last_error.restype = ctypes.c_char_p
    return lib


class Store:
    """One rec_store (one device); close() or a with-block frees its device buffers.  No CPU path: raises without a GPU."""

    def __init__(self, device=0):
        self.lib = _bind(load_library())
        self.h = ctypes.c_void_p()
        rc = self.lib.rec_create(int(device), ctypes.byref(self.h))
        if rc != 0:
            raise DsaError(rc, "rec_create: " + self.lib.rec_last_error().decode())

    def _check(self, rc):
        if rc != 0:
            raise DsaError(rc, self.lib.rec_last_error().decode())

    def clear(self):
        self._check(self.lib.rec_clear(self.h))

    def append(self, records):
        """rec_append of a structured array with the layout of dsa_record (dsa.RECORD_DTYPE)."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        self._check(self.lib.rec_append(self.h, records.ctypes.data if len(records) else None, len(records)))

    def append_device(self, ptr, n):
        """rec_append_device: n records at a device pointer (an int) of the store's device, their producer completed."""
        self._check(self.lib.rec_append_device(self.h, ctypes.c_void_p(ptr), int(n)))

    def tail(self, room):
        """rec_tail: the device pointer (an int) of room for `room` records behind the last one; commit(n) adds n of them."""
        p = ctypes.c_void_p()
        self._check(self.lib.rec_tail(self.h, int(room), ctypes.byref(p)))
        return p.value

    def commit(self, n):
        self._check(self.lib.rec_commit(self.h, int(n)))

    def sort(self):
        self._check(self.lib.rec_sort(self.h))

    def __len__(self):
        n = ctypes.c_int64()
        self._check(self.lib.rec_count(self.h, ctypes.byref(n)))
        return n.value

    def records_device(self):
        """(device pointer as an int, n): what eval.Context.evaluate_device takes."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._check(self.lib.rec_records_device(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value or 0, n.value

    def download(self):
        n = ctypes.c_int64()
        out = np.zeros(len(self), RECORD_DTYPE)
        self._check(self.lib.rec_download(self.h, out.ctypes.data if len(out) else None, len(out), ctypes.byref(n)))
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
        rc = self.lib.rec_text(self.h, kp, nk, buf.ctypes.data, size, ctypes.byref(got))
        if rc != 0:
            e = DsaError(rc, self.lib.rec_last_error().decode())
            e.bytes = got.value
            raise e
        return buf[:got.value].tobytes()

    def timing(self):
        t = RecTiming()
        self._check(self.lib.rec_get_timing(self.h, ctypes.byref(t)))
        return {name: getattr(t, name) for name, _ in RecTiming._fields_ if name != "pad_"}

    def close(self):
        if self.h:
            self.lib.rec_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
