"""ctypes binding of include/defuse_est.h (EST islands on the GPU); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi
from .capi import ptr as _ptr
from .dsa import load_library

PAD = 300                       # EST_ISLAND_PAD


class EstTiming(ctypes.Structure):
    _fields_ = [("build_ms", ctypes.c_float), ("lookup_ms", ctypes.c_float), ("n_segments", ctypes.c_int64),
                ("n_degenerate", ctypes.c_int64), ("n_islands", ctypes.c_int64), ("n_queries", ctypes.c_int64),
                ("n_contained", ctypes.c_int64)]


p, i64, cint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "est_catalog_create": (cint, [cint, p, p, p, i64, ctypes.c_int32, ctypes.POINTER(p)]),
    "est_catalog_islands": (cint, [p, p, p, i64, ctypes.POINTER(i64), p]),
    "est_catalog_contained": (cint, [p, p, p, p, i64, p, ctypes.POINTER(EstTiming)]),
    "est_catalog_destroy": (None, [p]),
    "est_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_est.h bound."""
    return _bind(load_library())


def _col(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Catalog(capi.Owned):
    """The islands of EST segments (dense chromosome ids in [0, n_chrom), start, end) on one device
    (est_catalog_create); close() or a with-block frees them."""
    _destroy = "est_catalog_destroy"

    def __init__(self, chrom, start, end, n_chrom, device=0):
        super().__init__(lib())
        c, s, e = _col(chrom), _col(start), _col(end)
        assert len(c) == len(s) == len(e)
        self.n_chrom = int(n_chrom)
        rc = self._lib.est_catalog_create(device, _ptr(c), _ptr(s), _ptr(e), len(c), self.n_chrom, ctypes.byref(self.handle))
        if rc != 0:
            raise RuntimeError("est_catalog_create failed (%d): %s" % (rc, self._lib.est_last_error().decode()))

    def islands(self):
        """(starts, ends, chrom_off): int32 arrays of the islands in order and the n_chrom + 1 offsets of each chromosome's."""
        n = ctypes.c_int64()
        off = np.zeros(self.n_chrom + 1, dtype=np.int64)
        rc = self._lib.est_catalog_islands(self.handle, None, None, 0, ctypes.byref(n), off.ctypes.data)
        if rc not in (0, -1):
            raise RuntimeError("est_catalog_islands failed (%d): %s" % (rc, self._lib.est_last_error().decode()))
        s = np.zeros(n.value, dtype=np.int32)
        e = np.zeros(n.value, dtype=np.int32)
        rc = self._lib.est_catalog_islands(self.handle, _ptr(s), _ptr(e), n.value, ctypes.byref(n), off.ctypes.data)
        if rc != 0:
            raise RuntimeError("est_catalog_islands failed (%d): %s" % (rc, self._lib.est_last_error().decode()))
        return s, e, off

    def contained(self, chrom, start, end):
        """(uint8 array, EstTiming): 1 where the query lies in a padded island of its chromosome."""
        c, s, e = _col(chrom), _col(start), _col(end)
        out = np.zeros(len(c), dtype=np.uint8)
        t = EstTiming()
        rc = self._lib.est_catalog_contained(self.handle, _ptr(c), _ptr(s), _ptr(e), len(c), _ptr(out), ctypes.byref(t))
        if rc != 0:
            raise RuntimeError("est_catalog_contained failed (%d): %s" % (rc, self._lib.est_last_error().decode()))
        return out, t


def catalog(chrom, start, end, n_chrom, device=0):
    return Catalog(chrom, start, end, n_chrom, device)
