"""ctypes binding of include/defuse_est.h (EST islands on the GPU); test/bench plumbing only."""
import ctypes

import numpy as np

from .dsa import load_library

PAD = 300                       # EST_ISLAND_PAD


class EstTiming(ctypes.Structure):
    _fields_ = [("build_ms", ctypes.c_float), ("lookup_ms", ctypes.c_float), ("n_segments", ctypes.c_int64),
                ("n_degenerate", ctypes.c_int64), ("n_islands", ctypes.c_int64), ("n_queries", ctypes.c_int64),
                ("n_contained", ctypes.c_int64)]


def _bind(lib):
    p = ctypes.c_void_p
    lib.est_catalog_create.argtypes = [ctypes.c_int, p, p, p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.est_catalog_islands.argtypes = [p, p, p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), p]
    lib.est_catalog_contained.argtypes = [p, p, p, p, ctypes.c_int64, p, ctypes.POINTER(EstTiming)]
    lib.est_catalog_destroy.argtypes = [p]
    lib.est_catalog_destroy.restype = None
    lib.est_last_error.restype = ctypes.c_char_p
    return lib


def _col(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a):
    return a.ctypes.data if len(a) else None


class Catalog:
    """The islands of EST segments (dense chromosome ids in [0, n_chrom), start, end) on one device
    (est_catalog_create); close() or a with-block frees them."""

    def __init__(self, chrom, start, end, n_chrom, device=0):
        self._lib = _bind(load_library())
        c, s, e = _col(chrom), _col(start), _col(end)
        assert len(c) == len(s) == len(e)
        self.n_chrom = int(n_chrom)
        self.handle = ctypes.c_void_p()
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

    def close(self):
        if self.handle:
            self._lib.est_catalog_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def catalog(chrom, start, end, n_chrom, device=0):
    return Catalog(chrom, start, end, n_chrom, device)
