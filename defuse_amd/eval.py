"""ctypes binding of include/defuse_eval.h (per fusion the best supported breakpoint, on the GPU); test/bench plumbing only.

In a process that also uses PyTorch-ROCm, import torch and let it touch the GPU before this module loads the library
(README)."""
import ctypes

import numpy as np

from .dsa import DSA_E_CAPACITY, RECORD_DTYPE, DsaError, load_library

NO_SPLIT, HOST_STATS = 1, 2      # EVAL_NO_SPLIT, EVAL_HOST_STATS
DSA_E_DEVICE, DSA_E_LIMIT = -2, -4

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


def _bind(lib):
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.eval_create.argtypes = [ctypes.c_int, ctypes.POINTER(p)]
    lib.eval_destroy.argtypes = [p]
    lib.eval_destroy.restype = None
    call = [p, p, i64, p, i64, ctypes.POINTER(i64), p, i64, ctypes.POINTER(i64)]
    lib.eval_groups.argtypes = call
    lib.eval_groups_device.argtypes = call
    lib.eval_get_timing.argtypes = [p, ctypes.POINTER(EvalTiming)]
    lib.eval_last_error.restype = ctypes.c_char_p
    return lib


class Context:
    """One eval_ctx (one device); close() or a with-block frees its device buffers.  No CPU path: raises without a GPU."""

    def __init__(self, device=0):
        self.lib = _bind(load_library())
        self.h = ctypes.c_void_p()
        rc = self.lib.eval_create(int(device), ctypes.byref(self.h))
        if rc != 0:
            raise DsaError(rc, "eval_create: " + self.lib.eval_last_error().decode())

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
        rc = fn(self.h, ptr, n, groups.ctypes.data if group_cap else None, group_cap, ctypes.byref(ng),
                kept.ctypes.data if kept_cap else None, kept_cap, ctypes.byref(nk))
        if rc != 0:
            e = DsaError(rc, self.lib.eval_last_error().decode())
            e.n_groups, e.n_kept = ng.value, nk.value
            raise e
        if sized:
            return groups[:ng.value], kept[:nk.value]
        return groups[:ng.value].copy(), kept[:nk.value].copy()      # (lets go of the n-sized arrays)

    def evaluate(self, records, group_cap=None, kept_cap=None):
        """eval_groups on a structured array with the layout of dsa_record (dsa.RECORD_DTYPE)."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        return self._call(self.lib.eval_groups, records.ctypes.data if len(records) else None, len(records), group_cap, kept_cap)

    def evaluate_device(self, ptr, n, group_cap=None, kept_cap=None):
        """eval_groups_device: n records at a device pointer (an int, e.g. what dsa.Context.records_to_device filled)."""
        return self._call(self.lib.eval_groups_device, ctypes.c_void_p(ptr), int(n), group_cap, kept_cap)

    def timing(self):
        t = EvalTiming()
        rc = self.lib.eval_get_timing(self.h, ctypes.byref(t))
        if rc != 0:
            raise DsaError(rc, self.lib.eval_last_error().decode())
        return {name: getattr(t, name) for name, _ in EvalTiming._fields_ if name != "pad_"}

    def close(self):
        if self.h:
            self.lib.eval_destroy(self.h)
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
