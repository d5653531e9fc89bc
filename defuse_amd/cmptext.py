"""ctypes binding of the "alignment and cluster text" section of include/defuse_cmp.h (clustermatepairs' alignment file parsed
and its cluster file printed on the GPU, defuse_amd/csrc/cmpt_api.hip); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi, cmp
from .capi import ptr as _ptr
from .cmp import RECORD_DTYPE, ROW_DTYPE

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
EMPTY_LINE, FORMAT, BAD_FRAGMENT, BAD_POSITION = 1, 2, 3, 4                  # CMPT_EMPTY_LINE ...
CONSTANTS = {"CMPT_EMPTY_LINE": EMPTY_LINE, "CMPT_FORMAT": FORMAT, "CMPT_BAD_FRAGMENT": BAD_FRAGMENT, "CMPT_BAD_POSITION": BAD_POSITION}

i32, i64, f32, vp, cint = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int


class CmptResult(ctypes.Structure):
    _fields_ = [("consumed", i64), ("n_lines", i64), ("n_records", i64), ("n_fragments", i64), ("n_names", i64), ("stop_line", i64),
                ("stop_offset", i64), ("stop_len", i64), ("stop_kind", i32), ("pad_", i32)]


class CmptDevice(ctypes.Structure):
    _fields_ = [("records", vp), ("frag_start", vp), ("name_bytes", vp), ("name_off", vp), ("n_records", i64), ("n_fragments", i64),
                ("n_names", i64), ("n_name_bytes", i64), ("device", i32), ("pad_", i32)]


class CmptPrintResult(ctypes.Structure):
    _fields_ = [("n_rows", i64), ("text_bytes", i64), ("bad_row", i64)]


class CmptTiming(ctypes.Structure):
    _fields_ = [("upload_ms", f32), ("tables_ms", f32), ("lines_ms", f32), ("names_ms", f32), ("layout_ms", f32), ("lengths_ms", f32),
                ("write_ms", f32), ("download_ms", f32), ("text_bytes", i64), ("out_bytes", i64), ("n_pieces", i32), ("pad_", i32)]


STRUCTS = {"cmpt_result": CmptResult, "cmpt_device": CmptDevice, "cmpt_print_result": CmptPrintResult, "cmpt_timing": CmptTiming}


class CmptError(capi.ApiError):
    prefix = "cmpt"


P = ctypes.POINTER
PROTOTYPES = {
    "cmpt_create": (cint, [cint, i64, P(vp)]),
    "cmpt_destroy": (None, [vp]),
    "cmpt_begin": (cint, [vp]),
    "cmpt_add": (cint, [vp, vp, i64, i32, P(CmptResult)]),
    "cmpt_add_device": (cint, [vp, vp, i64, i32, P(CmptResult)]),
    "cmpt_view": (cint, [vp, P(CmptDevice)]),
    "cmpt_fetch": (cint, [vp, vp, i64, vp, i64]),
    "cmpt_names_fetch": (cint, [vp, vp, i64, vp, i64]),
    "cmpt_bin_upload_records_device": (cint, [vp, vp, i64, i64]),
    "cmpt_bin_upload_fragments_device": (cint, [vp, vp, i64, i64]),
    "cmpt_problems_rows_view": (cint, [vp, P(vp), P(i64)]),
    "cmpt_print_rows": (cint, [vp, vp, i64, P(CmptPrintResult)]),
    "cmpt_print_rows_device": (cint, [vp, vp, i64, P(CmptPrintResult)]),
    "cmpt_text_fetch": (cint, [vp, vp, i64, P(i64)]),
    "cmpt_get_timing": (cint, [vp, P(CmptTiming)]),
    "cmpt_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the cmpt_ functions (and those of cmp.lib()) bound."""
    return capi.bind(cmp.lib(), PROTOTYPES)


def _fail(lib, what, rc, sink="cmpt_last_error"):
    raise CmptError(rc, "%s: %s" % (what, getattr(lib, sink)().decode()))


def _text(text):
    """bytes or a uint8 array -> a contiguous uint8 array (no copy of an array that already is one)."""
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


class CmptContext(capi.Owned):
    """One cmpt_ctx (one device): the records, fragment starts and names of one alignment stream, and the latest printed text."""
    _destroy = "cmpt_destroy"
    result = None
    printed = None

    def __init__(self, max_names=1 << 16, device=0):
        super().__init__(lib())
        rc = self._lib.cmpt_create(int(device), int(max_names), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "cmpt_create", rc)

    def begin(self):
        rc = self._lib.cmpt_begin(self.handle)
        if rc != 0:
            _fail(self._lib, "cmpt_begin", rc)
        self.result = self.printed = None

    def add(self, text, final=True):
        """cmpt_add of one piece (bytes or a uint8 array); returns the cmpt_result as a dict."""
        t = _text(text)
        res = CmptResult()
        rc = self._lib.cmpt_add(self.handle, _ptr(t), len(t), int(final), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "cmpt_add", rc)
        self.result = capi.as_dict(res)
        return self.result

    def add_device(self, ptr, n, final=True):
        """cmpt_add_device of n bytes at the device address `ptr`."""
        res = CmptResult()
        rc = self._lib.cmpt_add_device(self.handle, vp(ptr), int(n), int(final), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "cmpt_add_device", rc)
        self.result = capi.as_dict(res)
        return self.result

    def view(self):
        v = CmptDevice()
        rc = self._lib.cmpt_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "cmpt_view", rc)
        return v

    def fetch(self):
        """(records as RECORD_DTYPE, fragment starts as uint32 with their closing entry) of the stream so far."""
        v = self.view()
        recs, starts = np.zeros(v.n_records, dtype=RECORD_DTYPE), np.zeros(v.n_fragments + 1, dtype=np.uint32)
        rc = self._lib.cmpt_fetch(self.handle, _ptr(recs), len(recs), starts.ctypes.data, len(starts))
        if rc != 0:
            _fail(self._lib, "cmpt_fetch", rc)
        return recs, starts

    def names(self):
        """The names of the stream so far, in their numbering, as a list of bytes objects."""
        v = self.view()
        data, off = np.zeros(v.n_name_bytes, dtype=np.uint8), np.zeros(v.n_names + 1, dtype=np.int64)
        rc = self._lib.cmpt_names_fetch(self.handle, _ptr(data), len(data), off.ctypes.data, len(off))
        if rc != 0:
            _fail(self._lib, "cmpt_names_fetch", rc)
        raw = data.tobytes()
        return [raw[off[k]:off[k + 1]] for k in range(v.n_names)]

    def hand_over(self, binner):
        """cmp_bin_reserve and the two device-pointer uploads: the stream's records and fragments into a cmp.Binner."""
        v = self.view()
        for what, rc in (("cmp_bin_reserve", self._lib.cmp_bin_reserve(binner.handle, v.n_records, v.n_fragments)),
                         ("cmpt_bin_upload_records_device", self._lib.cmpt_bin_upload_records_device(binner.handle, v.records, v.n_records, 0)),
                         ("cmpt_bin_upload_fragments_device", self._lib.cmpt_bin_upload_fragments_device(binner.handle, v.frag_start, v.n_fragments + 1, 0))):
            if rc != 0:
                _fail(self._lib, what, rc, "cmp_last_error")

    def print_rows(self, rows):
        """cmpt_print_rows of host rows (ROW_DTYPE); returns the text."""
        rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        return self._print("cmpt_print_rows", _ptr(rows), len(rows))

    def print_rows_device(self, ptr, n_rows):
        return self._print("cmpt_print_rows_device", vp(ptr), n_rows)

    def print_problems(self, problems):
        """The rows of the last select of a cmp.Problems, printed where they are."""
        rows, n = vp(), i64()
        rc = self._lib.cmpt_problems_rows_view(problems.handle, ctypes.byref(rows), ctypes.byref(n))
        if rc != 0:
            _fail(self._lib, "cmpt_problems_rows_view", rc, "cmp_last_error")
        return self.print_rows_device(rows.value, n.value)

    def _print(self, fn, rows, n_rows):
        res = CmptPrintResult()
        rc = getattr(self._lib, fn)(self.handle, rows, int(n_rows), ctypes.byref(res))
        self.printed = capi.as_dict(res)
        if rc != 0:
            e = CmptError(rc, "%s: %s" % (fn, self._lib.cmpt_last_error().decode()))
            e.bad_row = res.bad_row
            raise e
        return self.text()

    def text(self, cap=None):
        """The text of the last print; with cap, the buffer has that many bytes and a short one raises CmptError
        (code DSA_E_CAPACITY, .needed = the size)."""
        n = i64()
        rc = self._lib.cmpt_text_fetch(self.handle, None, 0, ctypes.byref(n))
        if rc not in (0, DSA_E_CAPACITY):
            _fail(self._lib, "cmpt_text_fetch", rc)
        buf = np.zeros(n.value if cap is None else cap, dtype=np.uint8)
        rc = self._lib.cmpt_text_fetch(self.handle, _ptr(buf), len(buf), ctypes.byref(n))
        if rc != 0:
            e = CmptError(rc, "cmpt_text_fetch: " + self._lib.cmpt_last_error().decode())
            e.needed = n.value
            raise e
        return buf[:n.value].tobytes()

    def timing(self):
        t = CmptTiming()
        rc = self._lib.cmpt_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "cmpt_get_timing", rc)
        return capi.as_dict(t)


def parse_pieces(ctx, data, cuts=()):
    """`data` through ctx.add in pieces cut at the ascending byte offsets `cuts` (final = 0; what a piece leaves unconsumed
    is given again in front of the next) and one final piece.  Returns the last result."""
    ctx.begin()
    pos = 0
    for cut in cuts:
        pos += ctx.add(data[pos:cut], final=False)["consumed"]
    return ctx.add(data[pos:], final=True)
