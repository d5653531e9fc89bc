"""ctypes binding of include/defuse_cmp.h (the bin pairs of clustermatepairs and the EM problems built from them on the GPU)
and of the two batch entries of include/defuse_mpe.h; test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi, mpe
from .capi import ptr as _ptr
from .mpe import MpeParams, MpeTiming      # noqa: F401  (cmp.MpeParams is what callers of cluster_batch build)

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT

i32, i64, u16, u32, f32, f64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_float, ctypes.c_double, ctypes.c_void_p


class Record(ctypes.Structure):
    _fields_ = [("fragment", i32), ("start", i32), ("end", i32), ("meta", u32)]


class Packed(ctypes.Structure):
    _fields_ = [("fragment", i32), ("read_end", i32), ("rel_start", u16), ("rel_end", u16)]


class Stats(ctypes.Structure):
    _fields_ = [("n_fragments", i64), ("n_concordant", i64), ("n_keys", i64), ("n_first", i64), ("n_second", i64), ("err_record", i64),
                ("err_kind", i32), ("err_value", i32), ("device_ms", f32), ("pad_", f32)]


class ProblemCounts(ctypes.Structure):
    _fields_ = [("n_candidates", i64), ("n_problems", i64), ("n_mate_pairs", i64), ("device_ms", f32), ("pad_", f32)]


class Pair(ctypes.Structure):
    _fields_ = [("first", i32), ("second", i32)]


class Row(ctypes.Structure):
    _fields_ = [("cluster_id", i32), ("fragment", i32 * 2), ("read_end", i32 * 2), ("ref", i32 * 2), ("strand", i32 * 2), ("start", i32 * 2),
                ("end", i32 * 2)]


class ProblemsDevice(ctypes.Structure):
    """cmp_problems_device: the arrays on the device, in the argument order of mpe_cluster_batch_device."""
    _fields_ = [("prob_off", vp), ("x", vp), ("y", vp), ("u", vp), ("to_xo", vp), ("to_yo", vp), ("pairs", vp), ("bin_pair", vp), ("member", vp),
                ("n_problems", i64), ("n_mate_pairs", i64), ("device", i32), ("pad_", i32)]


STRUCTS = {"cmp_record": Record, "cmp_packed": Packed, "cmp_stats": Stats, "cmp_problem_counts": ProblemCounts, "cmp_pair": Pair, "cmp_row": Row,
           "cmp_problems_device": ProblemsDevice}
MPE_STRUCTS = mpe.STRUCTS
RECORD_DTYPE = np.dtype([("fragment", "<i4"), ("start", "<i4"), ("end", "<i4"), ("meta", "<u4")])
PACKED_DTYPE = np.dtype([("fragment", "<i4"), ("read_end", "<i4"), ("rel_start", "<u2"), ("rel_end", "<u2")])
PAIR_DTYPE = np.dtype([("first", "<i4"), ("second", "<i4")])
ROW_DTYPE = np.dtype([("cluster_id", "<i4"), ("fragment", "<i4", (2,)), ("read_end", "<i4", (2,)), ("ref", "<i4", (2,)), ("strand", "<i4", (2,)),
                      ("start", "<i4", (2,)), ("end", "<i4", (2,))])
DTYPES = {"cmp_record": RECORD_DTYPE, "cmp_packed": PACKED_DTYPE, "cmp_pair": PAIR_DTYPE, "cmp_row": ROW_DTYPE}
assert (RECORD_DTYPE.itemsize, PACKED_DTYPE.itemsize, PAIR_DTYPE.itemsize, ROW_DTYPE.itemsize) == (16, 12, 8, 52)

# every function include/defuse_cmp.h declares
EXPORTS = ["cmp_bin_create", "cmp_bin_destroy", "cmp_bin_reserve", "cmp_bin_upload_records", "cmp_bin_upload_fragments", "cmp_bin_run",
           "cmp_bin_fetch", "cmp_bin_fetch_part", "cmp_last_error", "cmp_problems_create", "cmp_problems_destroy", "cmp_problems_build",
           "cmp_problems_build_lists", "cmp_problems_fetch", "cmp_problems_view", "cmp_problems_select", "cmp_problems_rows"]
MPE_EXPORTS = mpe.EXPORTS


class CmpError(capi.ApiError):
    prefix = "cmp"


P, cint = ctypes.POINTER, ctypes.c_int
PROTOTYPES = {
    "cmp_bin_create": (cint, [P(vp), cint]),
    "cmp_bin_destroy": (None, [vp]),
    "cmp_bin_reserve": (cint, [vp, i64, i64]),
    "cmp_bin_upload_records": (cint, [vp, vp, i64, i64]),
    "cmp_bin_upload_fragments": (cint, [vp, vp, i64, i64]),
    "cmp_bin_run": (cint, [vp, i32, P(Stats)]),
    "cmp_bin_fetch": (cint, [vp, vp, vp, vp, vp, vp]),
    "cmp_bin_fetch_part": (cint, [vp, cint, i64, i64, vp]),
    "cmp_last_error": (ctypes.c_char_p, []),
    "cmp_problems_create": (cint, [P(vp), cint]),
    "cmp_problems_destroy": (None, [vp]),
    "cmp_problems_build": (cint, [vp, vp, i32, i32, f64, P(ProblemCounts)]),
    "cmp_problems_build_lists": (cint, [vp, vp, vp, vp, vp, vp, i64, i32, i32, f64, P(ProblemCounts)]),
    "cmp_problems_fetch": (cint, [vp] + [vp] * 8),
    "cmp_problems_view": (cint, [vp, P(ProblemsDevice)]),
    "cmp_problems_select": (cint, [vp, i64, i64, vp, vp, i32, P(i64)]),
    "cmp_problems_rows": (cint, [vp, vp, i64, P(i64)]),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_cmp.h and defuse_mpe.h bound."""
    return _bind(mpe.lib())


def _fail(lib, what, rc):
    raise CmpError(rc, "%s: %s" % (what, lib.cmp_last_error().decode()))


class Binner(capi.Owned):
    """cmp_bin_*: records (RECORD_DTYPE) and fragment starts (uint32, one more entry = the number of records) -> bin pairs."""
    _destroy = "cmp_bin_destroy"

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.cmp_bin_create(ctypes.byref(self.handle), device)
        if rc != 0:
            _fail(self._lib, "cmp_bin_create", rc)
        self.stats = None

    def run(self, recs, starts, min_fusion_range):
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        for what, rc in (("cmp_bin_reserve", self._lib.cmp_bin_reserve(self.handle, len(recs), len(starts) - 1)),
                         ("cmp_bin_upload_records", self._lib.cmp_bin_upload_records(self.handle, _ptr(recs), len(recs), 0)),
                         ("cmp_bin_upload_fragments", self._lib.cmp_bin_upload_fragments(self.handle, _ptr(starts), len(starts), 0))):
            if rc != 0:
                _fail(self._lib, what, rc)
        st = Stats()
        rc = self._lib.cmp_bin_run(self.handle, min_fusion_range, ctypes.byref(st))
        if rc != 0:
            _fail(self._lib, "cmp_bin_run", rc)
        self.stats = st
        return st

    def fetch(self):
        """(keys, off_first, off_second, first, second) of the last run."""
        st = self.stats
        keys = np.zeros(st.n_keys, dtype=np.uint64)
        off1, off2 = np.zeros(st.n_keys + 1, dtype=np.int64), np.zeros(st.n_keys + 1, dtype=np.int64)
        p1, p2 = np.zeros(st.n_first, dtype=PACKED_DTYPE), np.zeros(st.n_second, dtype=PACKED_DTYPE)
        rc = self._lib.cmp_bin_fetch(self.handle, _ptr(keys), off1.ctypes.data, off2.ctypes.data, _ptr(p1), _ptr(p2))
        if rc != 0:
            _fail(self._lib, "cmp_bin_fetch", rc)
        return keys, off1, off2, p1, p2


ARRAYS = ("prob_off", "x", "y", "u", "to_xo", "to_yo", "pairs", "bin_pair")


class Problems(capi.Owned):
    """cmp_problems_*: the EM problems of the bin pairs, built and kept on the device."""
    _destroy = "cmp_problems_destroy"

    def __init__(self, device=0):
        super().__init__(lib())
        self.device = device
        rc = self._lib.cmp_problems_create(ctypes.byref(self.handle), device)
        if rc != 0:
            _fail(self._lib, "cmp_problems_create", rc)
        self.counts = None
        self._keep = None

    def build(self, binner, min_fusion_range, min_cluster_size, fragment_mean):
        c = ProblemCounts()
        self._keep = binner                    # its lists are read in place
        rc = self._lib.cmp_problems_build(self.handle, binner.handle, min_fusion_range, min_cluster_size, fragment_mean, ctypes.byref(c))
        if rc != 0:
            _fail(self._lib, "cmp_problems_build", rc)
        self.counts = c
        return c

    def build_lists(self, keys, off_first, off_second, first, second, min_fusion_range, min_cluster_size, fragment_mean):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        off1, off2 = np.ascontiguousarray(off_first, dtype=np.int64), np.ascontiguousarray(off_second, dtype=np.int64)
        p1, p2 = np.ascontiguousarray(first, dtype=PACKED_DTYPE), np.ascontiguousarray(second, dtype=PACKED_DTYPE)
        c = ProblemCounts()
        rc = self._lib.cmp_problems_build_lists(self.handle, _ptr(keys), off1.ctypes.data, off2.ctypes.data, _ptr(p1), _ptr(p2), len(keys),
                                                min_fusion_range, min_cluster_size, fragment_mean, ctypes.byref(c))
        if rc != 0:
            _fail(self._lib, "cmp_problems_build_lists", rc)
        self.counts = c
        return c

    def fetch(self, names=ARRAYS):
        """dict of the named arrays (any subset of ARRAYS) as numpy arrays."""
        c = self.counts
        shape = {"prob_off": (c.n_problems + 1, np.int64), "x": (c.n_mate_pairs, np.float64), "y": (c.n_mate_pairs, np.float64),
                 "u": (c.n_mate_pairs, np.float64), "to_xo": (c.n_mate_pairs, np.int32), "to_yo": (c.n_mate_pairs, np.int32),
                 "pairs": (c.n_mate_pairs, PAIR_DTYPE), "bin_pair": (c.n_problems, np.int32)}
        out = {n: np.zeros(shape[n][0], dtype=shape[n][1]) for n in names}
        rc = self._lib.cmp_problems_fetch(self.handle, *[out[n].ctypes.data if n in out else None for n in ARRAYS])
        if rc != 0:
            _fail(self._lib, "cmp_problems_fetch", rc)
        return out

    def view(self):
        v = ProblemsDevice()
        rc = self._lib.cmp_problems_view(self.handle, ctypes.byref(v))
        if rc != 0:
            _fail(self._lib, "cmp_problems_view", rc)
        return v

    def select(self, p0, p1, n_clusters, member_ptr, cluster_base=0):
        """cmp_problems_select of problems [p0, p1): n_clusters a host array of p1 - p0 counts, member_ptr a device pointer to the
        mask of mate pair prob_off[p0]; returns the number of rows."""
        ncl = np.ascontiguousarray(n_clusters, dtype=np.int32)
        assert len(ncl) == p1 - p0
        n = i64()
        rc = self._lib.cmp_problems_select(self.handle, p0, p1, _ptr(ncl), vp(member_ptr), cluster_base, ctypes.byref(n))
        if rc != 0:
            _fail(self._lib, "cmp_problems_select", rc)
        return n.value

    def rows(self, cap=None):
        """The rows of the last select (ROW_DTYPE); with cap, the buffer has that many rows and a short one raises CmpError
        (code DSA_E_CAPACITY, .needed = the count)."""
        n = i64()
        rc = self._lib.cmp_problems_rows(self.handle, None, 0, ctypes.byref(n))
        if rc not in (0, DSA_E_CAPACITY):
            _fail(self._lib, "cmp_problems_rows", rc)
        out = np.zeros(n.value if cap is None else cap, dtype=ROW_DTYPE)
        rc = self._lib.cmp_problems_rows(self.handle, _ptr(out), len(out), ctypes.byref(n))
        if rc != 0:
            e = CmpError(rc, "cmp_problems_rows: " + self._lib.cmp_last_error().decode())
            e.needed = n.value
            raise e
        return out[:n.value]


def cluster_batch(params, prob_off, x, y, u, to_xo, to_yo, device=0, on_device=None):
    """mpe_cluster_batch of host arrays -> (n_clusters, member, status).  With on_device = (x, y, u, to_xo, to_yo, member) device
    pointers, mpe_cluster_batch_device: member stays on the device and None is returned in its place."""
    bound = lib()
    prob_off = np.ascontiguousarray(prob_off, dtype=np.int64)
    n = len(prob_off) - 1
    ncl, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    t = MpeTiming()
    if on_device is None:
        member = np.zeros(int(prob_off[-1]), dtype=np.uint16)
        arrs = [np.ascontiguousarray(a, dtype=d) for a, d in ((x, np.float64), (y, np.float64), (u, np.float64), (to_xo, np.int32), (to_yo, np.int32))]
        rc = bound.mpe_cluster_batch(device, ctypes.byref(params), prob_off.ctypes.data, n, *[a.ctypes.data for a in arrs], ncl.ctypes.data,
                                     member.ctypes.data, status.ctypes.data, ctypes.byref(t))
    else:
        member = None
        rc = bound.mpe_cluster_batch_device(device, ctypes.byref(params), prob_off.ctypes.data, n, *[vp(a) for a in on_device[:5]], ncl.ctypes.data,
                                            vp(on_device[5]), status.ctypes.data, ctypes.byref(t))
    if rc != 0:
        raise CmpError(rc, "mpe_cluster_batch: " + bound.mpe_last_error().decode())
    return ncl, member, status
