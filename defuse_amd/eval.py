"""ctypes binding of include/defuse_eval.h (per fusion the best supported breakpoint, on the GPU); test/bench plumbing only.

In a process that also uses PyTorch-ROCm, import torch and let it touch the GPU before this module loads the library
(README)."""
import ctypes

import numpy as np

from . import capi
from .capi import ptr as _ptr
from .dsa import RECORD_DTYPE, DsaError, load_library

NO_SPLIT, HOST_STATS = 1, 2      # EVAL_NO_SPLIT, EVAL_HOST_STATS
DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_LIMIT

GROUP_DTYPE = np.dtype([("fusion_id", "<i4"), ("status", "<i4"), ("first_record", "<i8"), ("n_records", "<i8"),
                        ("best_first", "<i4"), ("best_second", "<i4"), ("best_score", "<i4"), ("pad_", "<i4"),
                        ("count", "<i8"), ("kept_off", "<i8"), ("pos_sum", "<f8"), ("min_sum", "<f8")])
assert GROUP_DTYPE.itemsize == 72

EXPORTS = ["eval_create", "eval_destroy", "eval_groups", "eval_groups_device", "eval_get_timing", "eval_last_error"]


class EvalGroup(ctypes.Structure):
    """eval_group, field for field (GROUP_DTYPE is the same layout for arrays)."""
    _fields_ = [("fusion_id", ctypes.c_int32), ("status", ctypes.c_int32), ("first_record", ctypes.c_int64),
                ("n_records", ctypes.c_int64), ("best_first", ctypes.c_int32), ("best_second", ctypes.c_int32),
                ("best_score", ctypes.c_int32), ("pad_", ctypes.c_int32), ("count", ctypes.c_int64), ("kept_off", ctypes.c_int64),
                ("pos_sum", ctypes.c_double), ("min_sum", ctypes.c_double)]


class EvalTiming(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_float), ("device_ms", ctypes.c_float), ("download_ms", ctypes.c_float), ("pad_", ctypes.c_float),
                ("n_records", ctypes.c_int64), ("n_groups", ctypes.c_int64), ("n_runs", ctypes.c_int64), ("n_kept", ctypes.c_int64),
                ("n_flagged", ctypes.c_int64)]


STRUCTS = {"eval_group": EvalGroup, "eval_timing": EvalTiming}

p, i64, cint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
call = [p, p, i64, p, i64, ctypes.POINTER(i64), p, i64, ctypes.POINTER(i64)]
PROTOTYPES = {
    "eval_create": (cint, [cint, ctypes.POINTER(p)]),
    "eval_destroy": (None, [p]),
    "eval_groups": (cint, call),
    "eval_groups_device": (cint, call),
    "eval_get_timing": (cint, [p, ctypes.POINTER(EvalTiming)]),
    "eval_last_error": (ctypes.c_char_p, []),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_eval.h bound."""
    return _bind(load_library())


class Context(capi.Owned):
    """One eval_ctx (one device); close() or a with-block frees its device buffers.  No CPU path: raises without a GPU."""
    _destroy = "eval_destroy"
    h = property(lambda self: self.handle)      # the older spelling of .handle and ._lib
    lib = property(lambda self: self._lib)

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.eval_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            raise DsaError(rc, "eval_create: " + self._lib.eval_last_error().decode())

    def _call(self, fn, ptr, n, group_cap=None, kept_cap=None):
        """(groups, kept): a GROUP_DTYPE array and the int64 kept list.  Without capacities the arrays have room for n groups
        and n kept records, which always suffices, so the device pipeline runs once; with them the call is made as given and a
        DsaError carries the code and, for DSA_E_CAPACITY, the required counts (n_groups, n_kept)."""
        ng, nk = ctypes.c_int64(), ctypes.c_int64()
        sized = group_cap is not None and kept_cap is not None
        if not sized:
            group_cap = kept_cap = n
        groups = np.zeros(group_cap, GROUP_DTYPE)
        kept = np.zeros(kept_cap, np.int64)
        rc = fn(self.handle, ptr, n, groups.ctypes.data if group_cap else None, group_cap, ctypes.byref(ng),
                kept.ctypes.data if kept_cap else None, kept_cap, ctypes.byref(nk))
        if rc != 0:
            e = DsaError(rc, self._lib.eval_last_error().decode())
            e.n_groups, e.n_kept = ng.value, nk.value
            raise e
        if sized:
            return groups[:ng.value], kept[:nk.value]
        return groups[:ng.value].copy(), kept[:nk.value].copy()      # (lets go of the n-sized arrays)

    def evaluate(self, records, group_cap=None, kept_cap=None):
        """eval_groups on a structured array with the layout of dsa_record (dsa.RECORD_DTYPE)."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        return self._call(self._lib.eval_groups, _ptr(records), len(records), group_cap, kept_cap)

    def evaluate_device(self, ptr, n, group_cap=None, kept_cap=None):
        """eval_groups_device: n records at a device pointer (an int, e.g. what dsa.Context.records_to_device filled)."""
        return self._call(self._lib.eval_groups_device, ctypes.c_void_p(ptr), int(n), group_cap, kept_cap)

    def timing(self):
        t = EvalTiming()
        rc = self._lib.eval_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            raise DsaError(rc, self._lib.eval_last_error().decode())
        return capi.as_dict(t)
