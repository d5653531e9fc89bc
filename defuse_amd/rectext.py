"""ctypes binding of the "alignment text" section of include/defuse_rec.h (an alignment file parsed on the GPU straight into
a record store, so that the store's sort and print give the sorted file); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi, rec
from .capi import ptr as _ptr
from .dsa import load_library

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
FEW_FIELDS, BAD_INTEGER, BAD_BOOL = 1, 2, 3                                   # RECT_FEW_FIELDS ...
CONSTANTS = {"RECT_FEW_FIELDS": FEW_FIELDS, "RECT_BAD_INTEGER": BAD_INTEGER, "RECT_BAD_BOOL": BAD_BOOL}


class RectResult(ctypes.Structure):
    _fields_ = [("consumed", ctypes.c_int64), ("n_lines", ctypes.c_int64), ("n_records", ctypes.c_int64), ("stop_line", ctypes.c_int64),
                ("n_other", ctypes.c_int64), ("first_other", ctypes.c_int64), ("stop_kind", ctypes.c_int32), ("stop_field", ctypes.c_int32),
                ("stop_id_read", ctypes.c_int32), ("stop_id", ctypes.c_int32)]


class RectTiming(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_float), ("device_ms", ctypes.c_float), ("text_bytes", ctypes.c_int64), ("n_lines", ctypes.c_int64),
                ("n_records", ctypes.c_int64)]


STRUCTS = {"rect_result": RectResult, "rect_timing": RectTiming}


class RectError(capi.ApiError):
    prefix = "rect"


p, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "rect_create": (cint, [cint, ctypes.POINTER(p)]),
    "rect_destroy": (None, [p]),
    "rect_add": (cint, [p, p, p, i64, i32, ctypes.POINTER(RectResult)]),
    "rect_get_timing": (cint, [p, ctypes.POINTER(RectTiming)]),
    "rect_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the rect_ functions of include/defuse_rec.h bound."""
    return capi.bind(load_library(), PROTOTYPES)


def _fail(lib, what, rc):
    raise RectError(rc, "%s: %s" % (what, lib.rect_last_error().decode()))


def _text(text):
    """bytes or a uint8 array -> a contiguous uint8 array (no copy of an array that already is one)."""
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


class RectContext(capi.Owned):
    """One rect_ctx (one device): the text buffers and tables the pieces of any number of files pass through."""
    _destroy = "rect_destroy"

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.rect_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "rect_create", rc)

    def add(self, store, data, final=True):
        """rect_add of one piece (bytes or a uint8 array) into a rec.Store; returns the rect_result as a dict."""
        t = _text(data)
        res = RectResult()
        rc = self._lib.rect_add(self.handle, store.handle, _ptr(t), len(t), int(final), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "rect_add", rc)
        return capi.as_dict(res)

    def timing(self):
        t = RectTiming()
        rc = self._lib.rect_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "rect_get_timing", rc)
        return capi.as_dict(t)


def sort_text(pieces, device=0):
    """`LC_ALL=C sort -n -k 1` of the concatenation of `pieces` (each a whole file's bytes: a piece without a final newline
    ends its own last line) as bytes.  Raises ValueError for a stop or a line that is not plain, as the tool declines them."""
    with RectContext(device) as ctx, rec.Store(device) as store:
        for k, data in enumerate(pieces):
            r = ctx.add(store, data, final=True)
            if r["stop_line"] or r["n_other"]:
                raise ValueError("piece %d, line %d: not a plain alignment line" % (k, r["stop_line"] or r["first_other"]))
        store.sort()
        return store.text()
