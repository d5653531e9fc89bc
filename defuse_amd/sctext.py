"""ctypes binding of the "cluster text" section of include/defuse_sc.h (setcover's cluster file parsed, covered, filtered and
printed on the GPU); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi
from .capi import ptr as _ptr
from .dsa import load_library

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
EMPTY_LINE, FEW_FIELDS, BAD_INTEGER, BAD_CLUSTER_ID = 1, 2, 3, 4            # SCT_EMPTY_LINE ...
OK, READ_STOP, NEGATIVE_ELEMENT, WRITE_STOP = 0, 1, 2, 3                     # SCT_OK ...
CONSTANTS = {"SCT_EMPTY_LINE": EMPTY_LINE, "SCT_FEW_FIELDS": FEW_FIELDS, "SCT_BAD_INTEGER": BAD_INTEGER, "SCT_BAD_CLUSTER_ID": BAD_CLUSTER_ID,
             "SCT_OK": OK, "SCT_READ_STOP": READ_STOP, "SCT_NEGATIVE_ELEMENT": NEGATIVE_ELEMENT, "SCT_WRITE_STOP": WRITE_STOP}


class SctResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("stop_kind", ctypes.c_int32), ("stop_line", ctypes.c_int64), ("stop_offset", ctypes.c_int64),
                ("stop_len", ctypes.c_int64), ("n_lines", ctypes.c_int64), ("n_members", ctypes.c_int64), ("n_clusters", ctypes.c_int64),
                ("max_element", ctypes.c_int64), ("n_kept_lines", ctypes.c_int64), ("out_bytes", ctypes.c_int64)]


class SctTiming(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_float), ("tables_ms", ctypes.c_float), ("parse_ms", ctypes.c_float), ("layout_ms", ctypes.c_float),
                ("cover_ms", ctypes.c_float), ("select_ms", ctypes.c_float), ("gather_ms", ctypes.c_float), ("download_ms", ctypes.c_float),
                ("text_bytes", ctypes.c_int64), ("gather_bytes", ctypes.c_int64), ("n_runs", ctypes.c_int64), ("n_pieces", ctypes.c_int32),
                ("n_components", ctypes.c_int32), ("n_large", ctypes.c_int32), ("cc_iterations", ctypes.c_int32)]


STRUCTS = {"sct_result": SctResult, "sct_timing": SctTiming}


class SctError(capi.ApiError):
    prefix = "sct"


p, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "sct_create": (cint, [cint, ctypes.POINTER(p)]),
    "sct_destroy": (None, [p]),
    "sct_begin": (cint, [p]),
    "sct_add": (cint, [p, p, i64, i32, ctypes.POINTER(i64)]),
    "sct_cover": (cint, [p, i64, ctypes.POINTER(SctResult)]),
    "sct_fetch": (cint, [p, i64, p, i64]),
    "sct_fetch_owner": (cint, [p, p, i64]),
    "sct_get_timing": (cint, [p, ctypes.POINTER(SctTiming)]),
    "sct_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the sct_ functions of include/defuse_sc.h bound."""
    return capi.bind(load_library(), PROTOTYPES)


def _fail(lib, what, rc):
    raise SctError(rc, "%s: %s" % (what, lib.sct_last_error().decode()))


def _text(text):
    """bytes or a uint8 array -> a contiguous uint8 array (no copy of an array that already is one)."""
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


class SctContext(capi.Owned):
    """One sct_ctx (one device): the pieces of one cluster file on the device, and the output of the latest cover."""
    _destroy = "sct_destroy"
    result = None

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.sct_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "sct_create", rc)

    def begin(self):
        rc = self._lib.sct_begin(self.handle)
        if rc != 0:
            _fail(self._lib, "sct_begin", rc)

    def add(self, text, final=True):
        """sct_add of one piece (bytes or a uint8 array); returns the number of bytes consumed."""
        t = _text(text)
        consumed = ctypes.c_int64()
        rc = self._lib.sct_add(self.handle, _ptr(t), len(t), int(final), ctypes.byref(consumed))
        if rc != 0:
            _fail(self._lib, "sct_add", rc)
        return consumed.value

    def cover(self, min_cluster_size):
        """sct_cover; returns the sct_result as a dict."""
        res = SctResult()
        rc = self._lib.sct_cover(self.handle, int(min_cluster_size), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "sct_cover", rc)
        self.result = capi.as_dict(res)
        return self.result

    def fetch(self, offset=0, n=None):
        """n output bytes from `offset` (all that follow it by default) as a bytes object."""
        n = self.result["out_bytes"] - offset if n is None else n
        buf = np.zeros(max(n, 0), dtype=np.uint8)
        rc = self._lib.sct_fetch(self.handle, int(offset), _ptr(buf), int(n))
        if rc != 0:
            _fail(self._lib, "sct_fetch", rc)
        return buf.tobytes()

    def owner(self):
        """owner[0 .. max_element] of the latest cover as an int32 array (empty if the set cover did not run)."""
        ran = self.result["status"] in (OK, WRITE_STOP)
        owner = np.full(self.result["max_element"] + 1 if ran else 0, -1, dtype=np.int32)
        rc = self._lib.sct_fetch_owner(self.handle, _ptr(owner), len(owner))
        if rc != 0:
            _fail(self._lib, "sct_fetch_owner", rc)
        return owner

    def timing(self):
        t = SctTiming()
        rc = self._lib.sct_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "sct_get_timing", rc)
        return capi.as_dict(t)


def setcover_text(data, min_cluster_size, piece=None, device=0):
    """The whole tool on bytes: (result dict, output bytes).  `piece`: the file goes up in pieces of that many bytes, cut
    wherever they fall (final = 0, the unconsumed rest given again), and one final piece; None: in one piece."""
    with SctContext(device) as ctx:
        ctx.begin()
        pos = 0
        if piece:
            while len(data) - pos > piece:
                used = ctx.add(data[pos:pos + piece], final=False)
                if used == 0:                                   # no newline in the piece: a longer one, up to the line's end
                    nl = data.find(b"\n", pos + piece)
                    if nl < 0:
                        break
                    used = ctx.add(data[pos:nl + 1], final=False)
                pos += used
        ctx.add(data[pos:], final=True)
        res = ctx.cover(min_cluster_size)
        return res, ctx.fetch()
