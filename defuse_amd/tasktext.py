"""ctypes binding of the "region and exon text" section of include/defuse_task.h (the regions file and the exon table parsed
and resolved on the GPU, and the task store made from the pairs where they are); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi, task
from .capi import ptr as _ptr
from .text import pack_names

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
MAX_NAME = 64
EXON_BAD_INTEGER, EXON_BAD_STRAND, REGION_BAD_INTEGER, REGION_BAD_END, REGION_BAD_STRAND = 1, 2, 3, 4, 5
LIBRARY_LIMIT, EXON_LONG_NAME, EXON_DUPLICATE = 16, 16, 17
CONSTANTS = {"TASKT_MAX_NAME": MAX_NAME, "TASKT_EXON_BAD_INTEGER": EXON_BAD_INTEGER, "TASKT_EXON_BAD_STRAND": EXON_BAD_STRAND,
             "TASKT_REGION_BAD_INTEGER": REGION_BAD_INTEGER, "TASKT_REGION_BAD_END": REGION_BAD_END, "TASKT_REGION_BAD_STRAND": REGION_BAD_STRAND,
             "TASKT_LIBRARY_LIMIT": LIBRARY_LIMIT, "TASKT_EXON_LONG_NAME": EXON_LONG_NAME, "TASKT_EXON_DUPLICATE": EXON_DUPLICATE}

i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float


class TasktResult(ctypes.Structure):
    _fields_ = [("n_lines", i64), ("n_skipped", i64), ("n_items", i64), ("n_exons", i64), ("n_chroms", i64), ("name_bytes", i64), ("stop_line", i64),
                ("stop_off", i64), ("stop_len", i64), ("stop_kind", i32), ("stop_field", i32)]


class TasktTiming(ctypes.Structure):
    _fields_ = [("exon_upload_ms", f32), ("exon_device_ms", f32), ("exon_table_ms", f32), ("region_upload_ms", f32), ("region_device_ms", f32),
                ("check_ms", f32), ("exon_bytes", i64), ("region_bytes", i64)]


STRUCTS = {"taskt_result": TasktResult, "taskt_timing": TasktTiming}


class TaskTextError(capi.ApiError):
    prefix = "tasktext"


p, cint = ctypes.c_void_p, ctypes.c_int
PROTOTYPES = {
    "taskt_names_create": (cint, [cint, p, i64, p, i64, ctypes.POINTER(p)]),
    "taskt_names_destroy": (None, [p]),
    "taskt_create": (cint, [cint, ctypes.POINTER(p)]),
    "taskt_destroy": (None, [p]),
    "taskt_parse_exons": (cint, [p, p, p, i64, ctypes.POINTER(TasktResult)]),
    "taskt_parse_regions": (cint, [p, p, p, i64, ctypes.POINTER(TasktResult)]),
    "taskt_exons": (p, [p]),
    "taskt_exons_fetch": (cint, [p, p, i64, p, i64, p, i64, p, i64, p, i64]),
    "taskt_pairs_fetch": (cint, [p, p, i64, p, i64]),
    "taskt_store_create": (cint, [p, p, ctypes.POINTER(task.Params), ctypes.POINTER(p)]),
    "taskt_get_timing": (cint, [p, ctypes.POINTER(TasktTiming)]),
    "taskt_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the taskt_ functions of include/defuse_task.h, and the store's own, bound."""
    return capi.bind(task.lib(), PROTOTYPES)


def _fail(lib, what, rc):
    raise TaskTextError(rc, "%s: %s" % (what, lib.taskt_last_error().decode()))


def _text(text):
    """bytes or a uint8 array -> a contiguous uint8 array (no copy of an array that already is one)."""
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


class Names(capi.Owned):
    """A list of names on one device (taskt_names_create): a sequence of names (bytes or str), index = position."""
    _destroy = "taskt_names_destroy"

    def __init__(self, names, device=0):
        super().__init__(lib())
        data, off = pack_names(names)
        rc = self._lib.taskt_names_create(device, _ptr(data), data.size, off.ctypes.data, len(off) - 1, ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "taskt_names_create", rc)


class Store(task.Store):
    """A task_store made by taskt_store_create: everything of task.Store but the constructor."""

    def __init__(self, lib_, handle):
        capi.Owned.__init__(self, lib_)
        self.handle.value = handle
        self.windows = task._Borrowed(self._lib.task_store_windows(self.handle), self)
        self.tasks = task._Borrowed(self._lib.task_store_pred_tasks(self.handle), self)
        self.tasks.windows = self.windows


class Context(capi.Owned):
    """One taskt_ctx (one device): the exon table and the pairs of the texts last parsed."""
    _destroy = "taskt_destroy"

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.taskt_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "taskt_create", rc)

    def _parse(self, what, names, data):
        t = _text(data)
        res = TasktResult()
        rc = getattr(self._lib, what)(self.handle, names.handle, _ptr(t), len(t), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, what, rc)
        return capi.as_dict(res)

    def parse_exons(self, ref_names, data):
        """taskt_parse_exons of the whole exon table (bytes or a uint8 array); the taskt_result as a dict."""
        self.exon_result = self._parse("taskt_parse_exons", ref_names, data)
        return self.exon_result

    def parse_regions(self, seq_names, data):
        self.region_result = self._parse("taskt_parse_regions", seq_names, data)
        return self.region_result

    def exons_handle(self):
        return self._lib.taskt_exons(self.handle)

    def exons(self):
        """(transcripts, exons, chrom_ref, [transcript names]): task.TRANSCRIPT_DTYPE, task.EXON_DTYPE, int32, bytes."""
        r = self.exon_result
        tx = np.zeros(r["n_items"], dtype=task.TRANSCRIPT_DTYPE)
        ex = np.zeros(r["n_exons"], dtype=task.EXON_DTYPE)
        cref = np.zeros(r["n_chroms"], dtype=np.int32)
        off = np.zeros(r["n_items"] + 1, dtype=np.int64)
        data = np.zeros(r["name_bytes"], dtype=np.uint8)
        rc = self._lib.taskt_exons_fetch(self.handle, _ptr(tx), len(tx), _ptr(ex), len(ex), _ptr(cref), len(cref), _ptr(off), len(off), _ptr(data), len(data))
        if rc != 0:
            _fail(self._lib, "taskt_exons_fetch", rc)
        raw = data.tobytes()
        return tx, ex, cref, [raw[off[k]:off[k + 1]] for k in range(len(tx))]

    def pairs(self):
        """(pairs, lines): task.PAIR_DTYPE and the (n, 2) int64 lines that gave the ends."""
        n = self.region_result["n_items"]
        pairs = np.zeros(n, dtype=task.PAIR_DTYPE)
        lines = np.zeros((n, 2), dtype=np.int64)
        rc = self._lib.taskt_pairs_fetch(self.handle, _ptr(pairs), n, _ptr(lines.reshape(-1)), 2 * n)
        if rc != 0:
            _fail(self._lib, "taskt_pairs_fetch", rc)
        return pairs, lines

    def store(self, reference, params):
        """taskt_store_create over the parsed table and pairs: a Store."""
        prm = task.Params(*[int(v) for v in params])
        h = ctypes.c_void_p()
        rc = self._lib.taskt_store_create(self.handle, reference.handle, ctypes.byref(prm), ctypes.byref(h))
        if rc != 0:
            _fail(self._lib, "taskt_store_create", rc)
        return Store(self._lib, h.value)

    def timing(self):
        t = TasktTiming()
        rc = self._lib.taskt_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "taskt_get_timing", rc)
        return capi.as_dict(t)
