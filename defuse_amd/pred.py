"""ctypes binding of include/defuse_pred.h (each fusion's predicted sequence and break positions on the GPU); test/bench
plumbing only."""
import ctypes

import numpy as np

from . import capi
from . import eval as ev
from .capi import ptr as _ptr
from .dsa import load_library

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
NO_TASK, OUT_OF_WINDOW = 4, 8      # PRED_NO_TASK, PRED_OUT_OF_WINDOW

TASK_DTYPE = np.dtype([("fusion_id", "<i4"), ("pad_", "<i4"), ("seq_start", "<i4", (2,)), ("seq_len", "<i4", (2,)),
                       ("seq_strand", "<i4", (2,)), ("rem_len", "<i4", (2,)), ("rem_off", "<i8", (2,))])
RESULT_DTYPE = np.dtype([("fusion_id", "<i4"), ("status", "<i4"), ("seq_off", "<i8"), ("seq_len", "<i4"), ("break_pos", "<i4", (2,)),
                         ("pad_", "<i4"), ("count", "<i8"), ("pos_avg", "<f8"), ("min_avg", "<f8")])
assert TASK_DTYPE.itemsize == 56 and RESULT_DTYPE.itemsize == 56


class Task(ctypes.Structure):
    """pred_task, field for field (TASK_DTYPE is the same layout for arrays)."""
    _fields_ = [("fusion_id", ctypes.c_int32), ("pad_", ctypes.c_int32), ("seq_start", ctypes.c_int32 * 2), ("seq_len", ctypes.c_int32 * 2),
                ("seq_strand", ctypes.c_int32 * 2), ("rem_len", ctypes.c_int32 * 2), ("rem_off", ctypes.c_int64 * 2)]


class Result(ctypes.Structure):
    """pred_result, field for field (RESULT_DTYPE is the same layout for arrays)."""
    _fields_ = [("fusion_id", ctypes.c_int32), ("status", ctypes.c_int32), ("seq_off", ctypes.c_int64), ("seq_len", ctypes.c_int32),
                ("break_pos", ctypes.c_int32 * 2), ("pad_", ctypes.c_int32), ("count", ctypes.c_int64), ("pos_avg", ctypes.c_double),
                ("min_avg", ctypes.c_double)]


class View(ctypes.Structure):
    """pred_device_view: the results of the latest prediction on the device."""
    _fields_ = [("results", ctypes.c_void_p), ("seq_bytes", ctypes.c_void_p), ("n_results", ctypes.c_int64), ("seq_bytes_len", ctypes.c_int64),
                ("device", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class PredTiming(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_float), ("plan_ms", ctypes.c_float), ("scan_ms", ctypes.c_float), ("gather_ms", ctypes.c_float),
                ("download_ms", ctypes.c_float), ("pad_", ctypes.c_float), ("n_groups", ctypes.c_int64), ("seq_bytes", ctypes.c_int64)]


STRUCTS = {"pred_task": Task, "pred_result": Result, "pred_device_view": View, "pred_timing": PredTiming}

# every function include/defuse_pred.h declares
EXPORTS = ["pred_tasks_create", "pred_tasks_destroy", "pred_create", "pred_destroy", "pred_predict", "pred_predict_resident", "pred_view",
           "pred_fetch", "pred_get_timing", "pred_last_error"]


class PredError(capi.ApiError):
    prefix = "pred"


p, i64, cint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "pred_tasks_create": (cint, [cint, p, p, i64, p, i64, ctypes.POINTER(p)]),
    "pred_tasks_destroy": (None, [p]),
    "pred_create": (cint, [cint, ctypes.POINTER(p)]),
    "pred_destroy": (None, [p]),
    "pred_predict": (cint, [p, p, p, i64]),
    "pred_predict_resident": (cint, [p, p, p]),
    "pred_view": (cint, [p, ctypes.POINTER(View)]),
    "pred_fetch": (cint, [p, p, i64, p, i64]),
    "pred_get_timing": (cint, [p, ctypes.POINTER(PredTiming)]),
    "pred_last_error": (ctypes.c_char_p, []),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_pred.h bound."""
    return _bind(load_library())


def _fail(lib, what, rc):
    raise PredError(rc, "%s: %s" % (what, lib.pred_last_error().decode()))


def pack_tasks(tasks):
    """The oracle's Task objects (fusion_id, seq_start, seq_len, seq_strand, remainder; a dict's values or a sequence) ->
    (rem_bytes, TASK_DTYPE array), one record per task in its order, the remainders back to back."""
    tasks = list(tasks.values()) if isinstance(tasks, dict) else list(tasks)
    recs = np.zeros(len(tasks), dtype=TASK_DTYPE)
    off = 0
    for k, t in enumerate(tasks):
        recs[k]["fusion_id"] = t.fusion_id
        for e in (0, 1):
            recs[k]["seq_start"][e], recs[k]["seq_len"][e], recs[k]["seq_strand"][e] = t.seq_start[e], t.seq_len[e], t.seq_strand[e]
            recs[k]["rem_off"][e], recs[k]["rem_len"][e] = off, len(t.remainder[e])
            off += len(t.remainder[e])
    return np.frombuffer(b"".join(bytes(t.remainder[0]) + bytes(t.remainder[1]) for t in tasks), dtype=np.uint8), recs


class Tasks(capi.Owned):
    """The tasks of a run on one device (pred_tasks_create) over a bat.Windows, which it keeps alive: `rem_bytes` uint8,
    `recs` TASK_DTYPE, or see from_oracle."""
    _destroy = "pred_tasks_destroy"

    def __init__(self, windows, rem_bytes, recs, device=0):
        super().__init__(lib())
        self.windows = windows
        rem_bytes = np.ascontiguousarray(rem_bytes, dtype=np.uint8)
        recs = np.ascontiguousarray(recs, dtype=TASK_DTYPE)
        rc = self._lib.pred_tasks_create(device, windows.handle, _ptr(rem_bytes), rem_bytes.size, _ptr(recs), len(recs), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "pred_tasks_create", rc)

    @classmethod
    def from_oracle(cls, windows, tasks, device=0):
        return cls(windows, *pack_tasks(tasks), device=device)


class Context(capi.Owned):
    """One pred_ctx (one device): the output buffers of the predictions, reused call after call.  `tasks` is the Tasks the
    predictions use unless a call names another."""
    _destroy = "pred_destroy"

    def __init__(self, tasks=None, device=0):
        super().__init__(lib())
        self.tasks = tasks
        rc = self._lib.pred_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "pred_create", rc)

    def predict(self, groups, tasks=None):
        """pred_predict of an eval.GROUP_DTYPE array in host memory; returns the view."""
        g = np.ascontiguousarray(groups, dtype=ev.GROUP_DTYPE)
        rc = self._lib.pred_predict(self.handle, (tasks or self.tasks).handle, _ptr(g), len(g))
        if rc != 0:
            _fail(self._lib, "pred_predict", rc)
        return self.view()

    def predict_resident(self, eval_ctx, tasks=None):
        """pred_predict_resident on the groups an eval.Context left on the device; returns the view."""
        rc = self._lib.pred_predict_resident(self.handle, (tasks or self.tasks).handle, eval_ctx.handle)
        if rc != 0:
            _fail(self._lib, "pred_predict_resident", rc)
        return self.view()

    def view(self):
        v = View()
        rc = self._lib.pred_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "pred_view", rc)
        return v

    def fetch(self):
        """(results, seq_bytes): a RESULT_DTYPE array and the uint8 sequences."""
        v = self.view()
        res = np.zeros(v.n_results, dtype=RESULT_DTYPE)
        seq = np.zeros(v.seq_bytes_len, dtype=np.uint8)
        rc = self._lib.pred_fetch(self.handle, _ptr(res), len(res), _ptr(seq), len(seq))
        if rc != 0:
            _fail(self._lib, "pred_fetch", rc)
        return res, seq

    def timing(self):
        t = PredTiming()
        rc = self._lib.pred_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "pred_get_timing", rc)
        return capi.as_dict(t)

    @staticmethod
    def format_seq(row, seq_bytes):
        """The line of WriteSequence (tools/SplitAlignment.cpp:596-605) for a result row with a sequence: "%g" for the
        two doubles, as an ostream prints them."""
        s = bytes(seq_bytes[int(row["seq_off"]):int(row["seq_off"]) + int(row["seq_len"])])
        return "%d\t%s\t0\t%d\t%s\t%s\n" % (row["fusion_id"], s.decode("latin-1"), row["count"], "%g" % row["pos_avg"], "%g" % row["min_avg"])

    @staticmethod
    def format_break(row, names, strands):
        """The two lines of WriteBreak (:607-615): names and strands (0 = plus) are the task's mAlignRefName / mAlignStrand
        of the two cluster ends."""
        return "".join("%d\t%d\t%s\t%s\t%d\n" % (row["fusion_id"], ce, names[ce], "+" if strands[ce] == 0 else "-", row["break_pos"][ce])
                       for ce in (0, 1))
