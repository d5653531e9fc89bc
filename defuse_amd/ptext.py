"""ctypes binding of include/defuse_ptext.h (splitreads.seq and splitreads.break printed on the GPU from a prediction);
test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi
from .capi import ptr as _ptr
from .dsa import load_library

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
HOST_SEQ = 16                      # PTEXT_HOST_SEQ
G_MAX = 12                         # PTEXT_G_MAX of ptext_shared.hpp: the longest "%g" text

END_DTYPE = np.dtype([("fusion_id", "<i4"), ("cluster_end", "<i4"), ("name", "<i4"), ("strand", "<i4")])
LINE_DTYPE = np.dtype([("seq_off", "<i8"), ("seq_len", "<i8"), ("brk_off", "<i8"), ("brk_len", "<i8"), ("status", "<i4"), ("pad_", "<i4")])
assert END_DTYPE.itemsize == 16 and LINE_DTYPE.itemsize == 40


class End(ctypes.Structure):
    """ptext_end, field for field (END_DTYPE is the same layout for arrays)."""
    _fields_ = [("fusion_id", ctypes.c_int32), ("cluster_end", ctypes.c_int32), ("name", ctypes.c_int32), ("strand", ctypes.c_int32)]


class Line(ctypes.Structure):
    """ptext_line, field for field (LINE_DTYPE is the same layout for arrays)."""
    _fields_ = [("seq_off", ctypes.c_int64), ("seq_len", ctypes.c_int64), ("brk_off", ctypes.c_int64), ("brk_len", ctypes.c_int64),
                ("status", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class View(ctypes.Structure):
    """ptext_device_view: the texts of the latest ptext_format on the device."""
    _fields_ = [("seq_text", ctypes.c_void_p), ("brk_text", ctypes.c_void_p), ("lines", ctypes.c_void_p), ("seq_text_len", ctypes.c_int64),
                ("brk_text_len", ctypes.c_int64), ("n_lines", ctypes.c_int64), ("device", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class PtextTiming(ctypes.Structure):
    _fields_ = [("lengths_ms", ctypes.c_float), ("write_ms", ctypes.c_float), ("gather_ms", ctypes.c_float), ("download_ms", ctypes.c_float),
                ("n_groups", ctypes.c_int64), ("seq_text_bytes", ctypes.c_int64), ("brk_text_bytes", ctypes.c_int64), ("gather_bytes", ctypes.c_int64)]


STRUCTS = {"ptext_end": End, "ptext_line": Line, "ptext_device_view": View, "ptext_timing": PtextTiming}

# every function include/defuse_ptext.h declares
EXPORTS = ["ptext_names_create", "ptext_names_destroy", "ptext_create", "ptext_destroy", "ptext_format", "ptext_view", "ptext_fetch",
           "ptext_get_timing", "ptext_format_doubles", "ptext_last_error"]


class PtextError(capi.ApiError):
    prefix = "ptext"


p, i64, cint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "ptext_names_create": (cint, [cint, p, i64, p, i64, p, i64, ctypes.POINTER(p)]),
    "ptext_names_destroy": (None, [p]),
    "ptext_create": (cint, [cint, ctypes.POINTER(p)]),
    "ptext_destroy": (None, [p]),
    "ptext_format": (cint, [p, p, p]),
    "ptext_view": (cint, [p, ctypes.POINTER(View)]),
    "ptext_fetch": (cint, [p, p, i64, p, i64, p, i64]),
    "ptext_get_timing": (cint, [p, ctypes.POINTER(PtextTiming)]),
    "ptext_format_doubles": (cint, [cint, p, i64, p, i64, p, ctypes.POINTER(i64)]),
    "ptext_last_error": (ctypes.c_char_p, []),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_ptext.h bound."""
    return _bind(load_library())


def _fail(lib, what, rc):
    raise PtextError(rc, "%s: %s" % (what, lib.ptext_last_error().decode()))


def pack_names(tasks):
    """The oracle's Task objects (fusion_id, ref_name, strand; a dict's values or a sequence) -> (name_bytes, name_off,
    END_DTYPE array): one name per distinct reference name, two ends per task."""
    tasks = list(tasks.values()) if isinstance(tasks, dict) else list(tasks)
    index, ends = {}, np.zeros(2 * len(tasks), dtype=END_DTYPE)
    for k, t in enumerate(tasks):
        for e in (0, 1):
            name = t.ref_name[e] if isinstance(t.ref_name[e], bytes) else str(t.ref_name[e]).encode("latin-1")
            ends[2 * k + e] = (t.fusion_id, e, index.setdefault(name, len(index)), t.strand[e])
    off = np.zeros(len(index) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(n) for n in index])
    return np.frombuffer(b"".join(index), dtype=np.uint8), off, ends


class Names(capi.Owned):
    """The reference names and align strands of a run on one device (ptext_names_create): `name_bytes` uint8, `name_off`
    int64 with one entry more than there are names, `ends` END_DTYPE; or see from_oracle."""
    _destroy = "ptext_names_destroy"

    def __init__(self, name_bytes, name_off, ends, device=0):
        super().__init__(lib())
        name_bytes = np.ascontiguousarray(name_bytes, dtype=np.uint8)
        name_off = np.ascontiguousarray(name_off, dtype=np.int64)
        ends = np.ascontiguousarray(ends, dtype=END_DTYPE)
        rc = self._lib.ptext_names_create(device, _ptr(name_bytes), name_bytes.size, _ptr(name_off), max(len(name_off) - 1, 0), _ptr(ends), len(ends),
                                          ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "ptext_names_create", rc)

    @classmethod
    def from_oracle(cls, tasks, device=0):
        return cls(*pack_names(tasks), device=device)


class Context(capi.Owned):
    """One ptext_ctx (one device): the two texts and the line table, reused call after call.  `names` is the Names the
    calls use unless one names another."""
    _destroy = "ptext_destroy"

    def __init__(self, names=None, device=0):
        super().__init__(lib())
        self.names = names
        rc = self._lib.ptext_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "ptext_create", rc)

    def format(self, pred_ctx, names=None):
        """ptext_format of the latest prediction of a pred.Context; returns the view."""
        rc = self._lib.ptext_format(self.handle, pred_ctx.handle, (names or self.names).handle)
        if rc != 0:
            _fail(self._lib, "ptext_format", rc)
        return self.view()

    def view(self):
        v = View()
        rc = self._lib.ptext_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "ptext_view", rc)
        return v

    def fetch(self):
        """(seq_text, brk_text, lines): two bytes objects and a LINE_DTYPE array."""
        v = self.view()
        seq = np.zeros(v.seq_text_len, dtype=np.uint8)
        brk = np.zeros(v.brk_text_len, dtype=np.uint8)
        lines = np.zeros(v.n_lines, dtype=LINE_DTYPE)
        rc = self._lib.ptext_fetch(self.handle, _ptr(seq), len(seq), _ptr(brk), len(brk), _ptr(lines), len(lines))
        if rc != 0:
            _fail(self._lib, "ptext_fetch", rc)
        return seq.tobytes(), brk.tobytes(), lines

    def timing(self):
        t = PtextTiming()
        rc = self._lib.ptext_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "ptext_get_timing", rc)
        return capi.as_dict(t)


def format_doubles(x, device=0, cap=None):
    """ptext_format_doubles: the "%g" text of every double of x as the device prints it, a list of bytes objects (b"" where
    the formatter declines)."""
    bound = lib()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(max(len(x) * G_MAX if cap is None else int(cap), 1), dtype=np.uint8)
    lens = np.zeros(max(len(x), 1), dtype=np.int32)
    total = ctypes.c_int64()
    rc = bound.ptext_format_doubles(device, _ptr(x), len(x), out.ctypes.data, len(x) * G_MAX if cap is None else int(cap), lens.ctypes.data, ctypes.byref(total))
    if rc != 0:
        e = PtextError(rc, "ptext_format_doubles: " + bound.ptext_last_error().decode())
        e.bytes = total.value
        raise e
    ends = np.cumsum(lens[:len(x)].astype(np.int64))
    assert (ends[-1] if len(x) else 0) == total.value
    text = out[:total.value].tobytes()
    return [text[e - l:e] for e, l in zip(ends.tolist(), lens[:len(x)].tolist())]
