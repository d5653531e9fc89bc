"""ctypes binding of the "span statistics" section of include/defuse_ptext.h (splitreads.span.stats from cluster text and
break positions in device memory); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi, clusterregions, tasktext
from .capi import ptr as _ptr
from .dsa import load_library

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
FEW_FIELDS, BAD_INTEGER, NOT_TWO_ENDS, NO_BREAK_END, COORD_LIMIT, NO_INTER, SUM_LIMIT = 1, 2, 3, 4, 5, 6, 7
FILE_CLUSTERS, FILE_BREAKS, FILE_SEQS = 0, 1, 2
INPUT, DEDUP = clusterregions.INPUT, clusterregions.DEDUP
G_MAX = 21                         # SPAN_G_MAX of span_shared.hpp: the longest "%.15g" text
CONSTANTS = {"SPAN_FEW_FIELDS": FEW_FIELDS, "SPAN_BAD_INTEGER": BAD_INTEGER, "SPAN_NOT_TWO_ENDS": NOT_TWO_ENDS, "SPAN_NO_BREAK_END": NO_BREAK_END,
             "SPAN_COORD_LIMIT": COORD_LIMIT, "SPAN_NO_INTER": NO_INTER, "SPAN_SUM_LIMIT": SUM_LIMIT, "SPAN_FILE_CLUSTERS": FILE_CLUSTERS,
             "SPAN_FILE_BREAKS": FILE_BREAKS, "SPAN_FILE_SEQS": FILE_SEQS, "TASKC_INPUT": INPUT, "TASKC_DEDUP": DEDUP}

ROW_DTYPE = np.dtype([("cluster_id", "<i4"), ("text_len", "<i4"), ("text_off", "<i8"), ("count", "<i8"), ("sum", "<i8"), ("mean", "<f8")])
assert ROW_DTYPE.itemsize == 40

i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float


class SpanResult(ctypes.Structure):
    _fields_ = [("n_lines", i64), ("n_seq_lines", i64), ("n_breaks", i64), ("n_inters", i64), ("n_ids", i64), ("n_rows", i64), ("out_bytes", i64),
                ("n_noncanonical", i64), ("stop_line", i64), ("stop_value", i64), ("stop_kind", i32), ("stop_field", i32), ("stop_file", i32), ("pad_", i32)]


class Row(ctypes.Structure):
    """span_row, field for field (ROW_DTYPE is the same layout for arrays)."""
    _fields_ = [("cluster_id", i32), ("text_len", i32), ("text_off", i64), ("count", i64), ("sum", i64), ("mean", ctypes.c_double)]


class View(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_void_p), ("text", ctypes.c_void_p), ("n_rows", i64), ("text_len", i64), ("device", i32), ("pad_", i32)]


class SpanTiming(ctypes.Structure):
    _fields_ = [("upload_ms", f32), ("lines_ms", f32), ("tables_ms", f32), ("sorts_ms", f32), ("terms_ms", f32), ("print_ms", f32), ("download_ms", f32),
                ("pad_", f32), ("n_lines", i64), ("n_rows", i64)]


STRUCTS = {"span_result": SpanResult, "span_row": Row, "span_device_view": View, "span_timing": SpanTiming}


class SpanStatsError(capi.ApiError):
    prefix = "spanstats"


p, cint = ctypes.c_void_p, ctypes.c_int
PROTOTYPES = {
    "span_create": (cint, [cint, ctypes.POINTER(p)]),
    "span_destroy": (None, [p]),
    "span_breaks_text": (cint, [p, p, i64, p, i64, ctypes.POINTER(SpanResult)]),
    "span_breaks_pred": (cint, [p, p, ctypes.POINTER(SpanResult)]),
    "span_stats": (cint, [p, p, i32, ctypes.POINTER(SpanResult)]),
    "span_view": (cint, [p, ctypes.POINTER(View)]),
    "span_fetch": (cint, [p, p, i64, p, i64]),
    "span_get_timing": (cint, [p, ctypes.POINTER(SpanTiming)]),
    "span_format_doubles": (cint, [cint, p, i64, p, i64, p, ctypes.POINTER(i64)]),
    "span_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the span_ functions of include/defuse_ptext.h bound."""
    return capi.bind(load_library(), PROTOTYPES)


def _fail(lib, what, rc):
    raise SpanStatsError(rc, "%s: %s" % (what, lib.span_last_error().decode()))


def _result(res):
    d = capi.as_dict(res)
    return d


class Context(capi.Owned):
    """One span_ctx (one device): the break and inter tables last made, and the rows and text of the last span_stats."""
    _destroy = "span_destroy"

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.span_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "span_create", rc)

    def breaks_text(self, brk, seq):
        """span_breaks_text of the two files' bytes; the span_result as a dict."""
        b, s = tasktext._text(brk), tasktext._text(seq)
        res = SpanResult()
        rc = self._lib.span_breaks_text(self.handle, _ptr(b), len(b), _ptr(s), len(s), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "span_breaks_text", rc)
        return _result(res)

    def breaks_pred(self, pred_ctx):
        """span_breaks_pred of the latest prediction of a pred.Context."""
        res = SpanResult()
        rc = self._lib.span_breaks_pred(self.handle, pred_ctx.handle, ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "span_breaks_pred", rc)
        return _result(res)

    def stats(self, clusters, source=DEDUP):
        """span_stats over the cluster text of a clusterregions.Context."""
        res = SpanResult()
        rc = self._lib.span_stats(self.handle, clusters.handle, int(source), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "span_stats", rc)
        return _result(res)

    def view(self):
        v = View()
        rc = self._lib.span_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "span_view", rc)
        return v

    def fetch(self):
        """(rows, text): a ROW_DTYPE array and a bytes object."""
        v = self.view()
        rows = np.zeros(v.n_rows, dtype=ROW_DTYPE)
        text = np.zeros(v.text_len, dtype=np.uint8)
        rc = self._lib.span_fetch(self.handle, _ptr(rows), len(rows), _ptr(text), len(text))
        if rc != 0:
            _fail(self._lib, "span_fetch", rc)
        return rows, text.tobytes()

    def timing(self):
        t = SpanTiming()
        rc = self._lib.span_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "span_get_timing", rc)
        return capi.as_dict(t)


def format_doubles(x, device=0):
    """span_format_doubles: the "%.15g" text of every double of x as the device prints it, a list of bytes objects (b"" where
    the formatter declines)."""
    bound = lib()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(max(len(x) * G_MAX, 1), dtype=np.uint8)
    lens = np.zeros(max(len(x), 1), dtype=np.int32)
    total = ctypes.c_int64()
    rc = bound.span_format_doubles(device, _ptr(x), len(x), out.ctypes.data, len(x) * G_MAX, lens.ctypes.data, ctypes.byref(total))
    if rc != 0:
        _fail(bound, "span_format_doubles", rc)
    ends = np.cumsum(lens[:len(x)].astype(np.int64))
    assert (ends[-1] if len(x) else 0) == total.value
    text = out[:total.value].tobytes()
    return [text[e - l:e] for e, l in zip(ends.tolist(), lens[:len(x)].tolist())]
