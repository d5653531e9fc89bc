"""ctypes binding of include/defuse_la.h (batched SimpleAligner scores on the GPU); test/bench plumbing only."""
import ctypes

import numpy as np

from . import capi
from .dsa import load_library

LA_ITEM = np.dtype([("ref_off", np.int64), ("seq_off", np.int64), ("ref_len", np.int32), ("seq_len", np.int32)])


class LaTiming(ctypes.Structure):
    _fields_ = [("pack_ms", ctypes.c_float), ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                ("n_packed16", ctypes.c_int32), ("n_int32", ctypes.c_int32), ("row_groups16", ctypes.c_int32),
                ("cells", ctypes.c_int64)]


p, i32, i64, cint = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
PROTOTYPES = {
    "la_align_batch": (cint, [cint, i32, i32, i32, p, i64, p, i64, p, ctypes.POINTER(LaTiming)]),
    "la_align_batch_min": (cint, [cint, i32, i32, i32, p, i64, p, i64, p, p, ctypes.POINTER(LaTiming)]),
    "la_genome_create": (cint, [cint, p, i64, ctypes.POINTER(p)]),
    "la_genome_destroy": (None, [p]),
    "la_align_windows_min": (cint, [p, i32, i32, i32, p, i64, p, i64, p, p, ctypes.POINTER(LaTiming)]),
    "la_last_error": (ctypes.c_char_p, []),
}
EXPORTS = list(PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_la.h bound."""
    return capi.bind(load_library(), PROTOTYPES)


def align_batch(pairs, match, mismatch, gap, device=0, min_score=None):
    """pairs: list of (reference bytes, sequence bytes).  Returns (int32 scores, timing).  With min_score (one
    int per pair) a score below its minimum is only guaranteed to be below it (la_align_batch_min)."""
    bound = lib()
    items = np.zeros(len(pairs), dtype=LA_ITEM)
    chunks, off = [], 0
    for k, (r, s) in enumerate(pairs):
        items[k] = (off, off + len(r), len(r), len(s))
        chunks += [bytes(r), bytes(s)]
        off += len(r) + len(s)
    pool = np.frombuffer(b"".join(chunks) + b"\0", dtype=np.uint8)
    scores = np.zeros(len(pairs), dtype=np.int32)
    t = LaTiming()
    need = None if min_score is None else np.ascontiguousarray(min_score, dtype=np.int32)
    rc = bound.la_align_batch_min(device, match, mismatch, gap, pool.ctypes.data, off, items.ctypes.data if len(pairs) else None,
                                  len(pairs), need.ctypes.data if need is not None and len(pairs) else None,
                                  scores.ctypes.data if len(pairs) else None, ctypes.byref(t))
    if rc != 0:
        raise RuntimeError("la_align_batch_min failed (%d): %s" % (rc, bound.la_last_error().decode()))
    return scores, t


LA_WINDOW = np.dtype([("slice_off", np.int64), ("seq_off", np.int64), ("slice_len", np.int32), ("pad_left", np.int32),
                      ("pad_right", np.int32), ("seq_len", np.int32), ("revcomp", np.int32), ("pad_", np.int32)])


class Genome(capi.Owned):
    """Contig bytes in HBM (la_genome_create); close() or a with-block frees them."""
    _destroy = "la_genome_destroy"

    def __init__(self, data, device=0):
        super().__init__(lib())
        buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
        self.len = len(buf) - 1
        rc = self._lib.la_genome_create(device, buf.ctypes.data, self.len, ctypes.byref(self.handle))
        if rc != 0:
            raise RuntimeError("la_genome_create failed (%d): %s" % (rc, self._lib.la_last_error().decode()))


def genome(data, device=0):
    """The bytes of a genome (contigs concatenated) on the device."""
    return Genome(data, device)


def align_windows(gen, reads, windows, match, mismatch, gap, min_score=None):
    """la_align_windows_min.  reads: list of byte strings; windows: one (read index, slice_off, slice_len, pad_left,
    pad_right, revcomp) per pair, or an LA_WINDOW array whose seq_off / seq_len index the concatenated reads.
    Returns (int32 scores, timing)."""
    bound = gen._lib
    pool = b"".join(bytes(r) for r in reads)
    if isinstance(windows, np.ndarray) and windows.dtype == LA_WINDOW:
        items = np.ascontiguousarray(windows)
    else:
        offs = np.cumsum([0] + [len(r) for r in reads])
        items = np.zeros(len(windows), dtype=LA_WINDOW)
        for k, (ri, so, sl, pl, pr, rc) in enumerate(windows):
            items[k] = (so, offs[ri], sl, pl, pr, len(reads[ri]), rc, 0)
    n = len(items)
    buf = np.frombuffer(pool + b"\0", dtype=np.uint8)
    scores = np.zeros(n, dtype=np.int32)
    t = LaTiming()
    need = None if min_score is None else np.ascontiguousarray(min_score, dtype=np.int32)
    rc = bound.la_align_windows_min(gen.handle, match, mismatch, gap, buf.ctypes.data, len(pool), items.ctypes.data if n else None, n,
                                    need.ctypes.data if need is not None and n else None, scores.ctypes.data if n else None, ctypes.byref(t))
    if rc != 0:
        raise RuntimeError("la_align_windows_min failed (%d): %s" % (rc, bound.la_last_error().decode()))
    return scores, t


def window_bytes(data, slice_off, slice_len, pad_left, pad_right, revcomp):
    """The reference a window stands for, built on the host (the semantics of include/defuse_la.h's la_window)."""
    w = b"N" * pad_left + bytes(data[slice_off:slice_off + slice_len]) + b"N" * pad_right
    return w[::-1].translate(_COMPLEMENT) if revcomp else w


_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
