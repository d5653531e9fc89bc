"""ctypes binding of include/defuse_cov.h (the sampling kernel of calccov); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi
from .capi import E_CAPACITY as DSA_E_CAPACITY
from .dsa import load_library

FRAGMENT_DTYPE = np.dtype([("ref", "<i4"), ("start", "<i4", (2,)), ("end", "<i4", (2,))])
assert FRAGMENT_DTYPE.itemsize == 20


class CovTiming(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_float), ("pad_", ctypes.c_int32), ("n_length_samples", ctypes.c_int64),
                ("n_split_samples", ctypes.c_int64)]


class CovError(capi.ApiError):
    prefix = "cov"


vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
PROTOTYPES = {
    "cov_sample_batch": (ctypes.c_int, [ctypes.c_int, vp, i32, vp, vp, i64, i32, i32, vp, vp, i64, ctypes.POINTER(i64),
                                        vp, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(CovTiming)]),
    "cov_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_cov.h bound."""
    return capi.bind(load_library(), PROTOTYPES)


def fragments_array(fragments):
    """[(ref, (start0, end0), (start1, end1)), ...] -> cov_fragment rows."""
    a = np.zeros(len(fragments), dtype=FRAGMENT_DTYPE)
    for k, (r, (s0, e0), (s1, e1)) in enumerate(fragments):
        a[k] = (r, (s0, s1), (e0, e1))
    return a


def sample_batch_raw(sample_off, sample_pos, fragments, trim, anchor, length_idx, length_val, split_idx, split_pos, split_min, device=0):
    """One call of cov_sample_batch into the caller's arrays (their sizes are the capacities): (return code, n_length,
    n_split, timing)."""
    off = np.ascontiguousarray(sample_off, dtype=np.int64)
    pos = np.ascontiguousarray(sample_pos, dtype=np.int32)
    fr = np.ascontiguousarray(fragments, dtype=FRAGMENT_DTYPE)
    assert len(length_idx) == len(length_val) and len(split_idx) == len(split_pos) == len(split_min)
    ptr = capi.ptr
    nl, ns, t = ctypes.c_int64(-1), ctypes.c_int64(-1), CovTiming()
    rc = lib().cov_sample_batch(device, off.ctypes.data, len(off) - 1, ptr(pos), ptr(fr), len(fr), trim, anchor,
                                ptr(length_idx), ptr(length_val), len(length_idx), ctypes.byref(nl),
                                ptr(split_idx), ptr(split_pos), ptr(split_min), len(split_idx), ctypes.byref(ns), ctypes.byref(t))
    return rc, nl.value, ns.value, t


def sample_batch(sample_off, sample_pos, fragments, trim, anchor, device=0):
    """The two-call protocol: ask for the counts with no room, then fetch.  fragments: cov_fragment rows (fragments_array).
    Returns (length_idx, length_val, split_idx, split_pos, split_min, timing)."""
    def room(nl, ns):
        return (np.zeros(nl, np.int32), np.zeros(nl, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.float64), np.zeros(ns, np.float64))
    out = room(0, 0)
    rc, nl, ns, t = sample_batch_raw(sample_off, sample_pos, fragments, trim, anchor, *out, device=device)
    if rc == DSA_E_CAPACITY:
        out = room(nl, ns)
        rc, nl, ns, t = sample_batch_raw(sample_off, sample_pos, fragments, trim, anchor, *out, device=device)
    if rc != 0:
        raise CovError(rc, lib().cov_last_error().decode())
    return out + (t,)
