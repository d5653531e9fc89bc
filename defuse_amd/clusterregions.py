"""ctypes binding of the "cluster text" section of include/defuse_task.h (remove_duplicates and get_align_regions on cluster
text in device memory, and the regions parse over their output where it lies); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi, task, tasktext
from .capi import ptr as _ptr

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
FEW_FIELDS, BAD_INTEGER, MISSING_END, NOT_TWO_ENDS = 1, 2, 3, 4
INPUT, DEDUP, REGIONS = 0, 1, 2
CONSTANTS = {"TASKC_FEW_FIELDS": FEW_FIELDS, "TASKC_BAD_INTEGER": BAD_INTEGER, "TASKC_MISSING_END": MISSING_END, "TASKC_NOT_TWO_ENDS": NOT_TWO_ENDS,
             "TASKC_INPUT": INPUT, "TASKC_DEDUP": DEDUP, "TASKC_REGIONS": REGIONS}

i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float


class TaskcResult(ctypes.Structure):
    _fields_ = [("n_lines", i64), ("n_runs", i64), ("n_clusters", i64), ("n_fragments", i64), ("n_kept_fragments", i64), ("n_kept_runs", i64),
                ("out_bytes", i64), ("stop_line", i64), ("stop_off", i64), ("stop_len", i64), ("stop_value", i64), ("stop_kind", i32), ("stop_field", i32)]


class TaskcTiming(ctypes.Structure):
    _fields_ = [("upload_ms", f32), ("tables_ms", f32), ("parse_ms", f32), ("sorts_ms", f32), ("select_ms", f32), ("gather_ms", f32), ("regions_ms", f32),
                ("print_ms", f32), ("text_bytes", i64), ("n_pieces", i64)]


STRUCTS = {"taskc_result": TaskcResult, "taskc_timing": TaskcTiming}


class ClusterRegionsError(capi.ApiError):
    prefix = "clusterregions"


p, cint = ctypes.c_void_p, ctypes.c_int
PROTOTYPES = {
    "taskc_create": (cint, [cint, ctypes.POINTER(p)]),
    "taskc_destroy": (None, [p]),
    "taskc_begin": (cint, [p]),
    "taskc_add": (cint, [p, p, i64, i32, ctypes.POINTER(i64)]),
    "taskc_add_cover": (cint, [p, p]),
    "taskc_dedup": (cint, [p, i64, ctypes.POINTER(TaskcResult)]),
    "taskc_regions": (cint, [p, i32, ctypes.POINTER(TaskcResult)]),
    "taskc_fetch": (cint, [p, i32, i64, p, i64]),
    "taskc_parse_regions": (cint, [p, p, p, ctypes.POINTER(tasktext.TasktResult)]),
    "taskc_get_timing": (cint, [p, ctypes.POINTER(TaskcTiming)]),
    "taskc_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the taskc_ functions of include/defuse_task.h bound."""
    return capi.bind(task.lib(), PROTOTYPES)


def _fail(lib, what, rc):
    raise ClusterRegionsError(rc, "%s: %s" % (what, lib.taskc_last_error().decode()))


class Context(capi.Owned):
    """One taskc_ctx (one device): the cluster text, and the dedup text and regions text last made from it."""
    _destroy = "taskc_destroy"
    dedup_result = regions_result = None

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.taskc_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "taskc_create", rc)

    def begin(self):
        rc = self._lib.taskc_begin(self.handle)
        if rc != 0:
            _fail(self._lib, "taskc_begin", rc)

    def add(self, text, final=True):
        """taskc_add of one piece (bytes or a uint8 array); returns the number of bytes consumed."""
        t = tasktext._text(text)
        consumed = ctypes.c_int64()
        rc = self._lib.taskc_add(self.handle, _ptr(t), len(t), int(final), ctypes.byref(consumed))
        if rc != 0:
            _fail(self._lib, "taskc_add", rc)
        return consumed.value

    def add_pieces(self, data, piece=None):
        """The whole text: in one piece, or in pieces of `piece` bytes cut wherever they fall (final = 0, the unconsumed rest
        given again; a line longer than a piece goes up whole) and one final piece."""
        pos = 0
        if piece:
            while len(data) - pos > piece:
                used = self.add(data[pos:pos + piece], final=False)
                if used == 0:
                    nl = data.find(b"\n", pos + piece)
                    if nl < 0:
                        break
                    used = self.add(data[pos:nl + 1], final=False)
                pos += used
        self.add(data[pos:], final=True)

    def add_cover(self, cover):
        """taskc_add_cover: the output of an sctext.SctContext's last cover, from device memory."""
        rc = self._lib.taskc_add_cover(self.handle, cover.handle)
        if rc != 0:
            _fail(self._lib, "taskc_add_cover", rc)

    def dedup(self, min_cluster_size):
        res = TaskcResult()
        rc = self._lib.taskc_dedup(self.handle, int(min_cluster_size), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "taskc_dedup", rc)
        self.dedup_result = capi.as_dict(res)
        return self.dedup_result

    def regions(self, source=DEDUP):
        res = TaskcResult()
        rc = self._lib.taskc_regions(self.handle, int(source), ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "taskc_regions", rc)
        self.regions_result = capi.as_dict(res)
        return self.regions_result

    def fetch(self, which, offset=0, n=None):
        """n bytes from `offset` (all that follow it by default) of the dedup text (DEDUP) or the regions text (REGIONS)."""
        total = (self.dedup_result if which == DEDUP else self.regions_result)["out_bytes"]
        n = total - offset if n is None else n
        buf = np.zeros(max(n, 0), dtype=np.uint8)
        rc = self._lib.taskc_fetch(self.handle, int(which), int(offset), _ptr(buf), int(n))
        if rc != 0:
            _fail(self._lib, "taskc_fetch", rc)
        return buf.tobytes()

    def parse_regions(self, into, seq_names):
        """taskc_parse_regions into a tasktext.Context, which then holds the pairs; the taskt_result as a dict."""
        res = tasktext.TasktResult()
        rc = self._lib.taskc_parse_regions(self.handle, into.handle, seq_names.handle, ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, "taskc_parse_regions", rc)
        into.region_result = capi.as_dict(res)
        return into.region_result

    def timing(self):
        t = TaskcTiming()
        rc = self._lib.taskc_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "taskc_get_timing", rc)
        return capi.as_dict(t)
