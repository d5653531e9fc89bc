"""ctypes binding of include/defuse_task.h (the tasks of the split-read chain made on the GPU from regions, reference and
exons); test/bench plumbing only."""
import ctypes

import numpy as np

from . import cand, capi
from .capi import ptr as _ptr
from .dsa import load_library

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
NO_SEQUENCE_0, BAD_CHROMOSOME_0, NO_SEQUENCE_1, BAD_CHROMOSOME_1 = 1, 2, 4, 8      # TASK_* status bits
MAX_COORD, MAX_REGION, MAX_PARAM, MAX_SEQ_LEN, EXON_BIN = 1 << 28, 1 << 24, 1 << 20, 1 << 30, 100000

i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float


class Seq(ctypes.Structure):
    _fields_ = [("off", i64), ("len", i64)]


class Transcript(ctypes.Structure):
    _fields_ = [("chrom", i32), ("strand", i32), ("first_exon", i32), ("n_exons", i32), ("name_ref", i32)]


class Exon(ctypes.Structure):
    _fields_ = [("start", i32), ("end", i32)]


class Params(ctypes.Structure):
    _fields_ = [("min_fragment", i32), ("max_fragment", i32), ("min_read", i32), ("max_read", i32)]


class End(ctypes.Structure):
    _fields_ = [("seq", i32), ("transcript", i32), ("chrom", i32), ("strand", i32), ("start", i32), ("end", i32)]


class Pair(ctypes.Structure):
    _fields_ = [("fusion_id", i32), ("end", End * 2)]


class Record(ctypes.Structure):
    _fields_ = [("fusion_id", i32), ("status", i32), ("seq_start", i32 * 2), ("seq_len", i32 * 2), ("seq_strand", i32 * 2), ("win_off", i32 * 2),
                ("rem_len", i32 * 2), ("rem_off", i64 * 2), ("n_regions", i32 * 2), ("region_off", i64)]


class Counts(ctypes.Structure):
    _fields_ = [("n_tasks", i64), ("window_bytes", i64), ("rem_bytes", i64), ("n_regions", i64)]


class TaskTiming(ctypes.Structure):
    _fields_ = [("upload_ms", f32), ("plan_ms", f32), ("count_ms", f32), ("scan_ms", f32), ("region_ms", f32), ("gather_ms", f32), ("sort_ms", f32),
                ("download_ms", f32), ("n_tasks", i64), ("n_regions", i64), ("window_bytes", i64), ("rem_bytes", i64)]


STRUCTS = {"task_seq": Seq, "task_transcript": Transcript, "task_exon": Exon, "task_params": Params, "task_end": End, "task_pair": Pair,
           "task_record": Record, "task_counts": Counts, "task_timing": TaskTiming}
SEQ_DTYPE, TRANSCRIPT_DTYPE, EXON_DTYPE = np.dtype(Seq), np.dtype(Transcript), np.dtype(Exon)
END_DTYPE = np.dtype(End)
PAIR_DTYPE = np.dtype([("fusion_id", "<i4"), ("end", END_DTYPE, (2,))])
RECORD_DTYPE = np.dtype([("fusion_id", "<i4"), ("status", "<i4"), ("seq_start", "<i4", (2,)), ("seq_len", "<i4", (2,)), ("seq_strand", "<i4", (2,)),
                         ("win_off", "<i4", (2,)), ("rem_len", "<i4", (2,)), ("rem_off", "<i8", (2,)), ("n_regions", "<i4", (2,)), ("region_off", "<i8")])
assert PAIR_DTYPE.itemsize == 52 and RECORD_DTYPE.itemsize == 80

# every function include/defuse_task.h declares
EXPORTS = ["task_reference_create", "task_reference_destroy", "task_exons_create", "task_exons_destroy", "task_store_create", "task_store_destroy",
           "task_store_windows", "task_store_pred_tasks", "task_store_counts", "task_store_fetch", "task_store_get_timing", "task_last_error"]


class TaskError(capi.ApiError):
    prefix = "task"


p, cint = ctypes.c_void_p, ctypes.c_int
PROTOTYPES = {
    "task_reference_create": (cint, [cint, p, i64, p, i64, ctypes.POINTER(p)]),
    "task_reference_destroy": (None, [p]),
    "task_exons_create": (cint, [cint, p, i32, p, i32, p, i64, ctypes.POINTER(p)]),
    "task_exons_destroy": (None, [p]),
    "task_store_create": (cint, [p, p, ctypes.POINTER(Params), p, i64, ctypes.POINTER(p)]),
    "task_store_destroy": (None, [p]),
    "task_store_windows": (p, [p]),
    "task_store_pred_tasks": (p, [p]),
    "task_store_counts": (cint, [p, ctypes.POINTER(Counts)]),
    "task_store_fetch": (cint, [p, p, i64, p, i64, p, i64, p, i64]),
    "task_store_get_timing": (cint, [p, ctypes.POINTER(TaskTiming)]),
    "task_last_error": (ctypes.c_char_p, []),
}


def _bind(lib):
    return capi.bind(lib, PROTOTYPES)


def lib():
    """The library with the functions of include/defuse_task.h bound."""
    return _bind(load_library())


def _fail(lib, what, rc):
    raise TaskError(rc, "%s: %s" % (what, lib.task_last_error().decode()))


class Reference(capi.Owned):
    """The sequences of a FASTA on one device (task_reference_create): {name: bytes} in the caller's order; .index maps a
    name to its sequence index."""
    _destroy = "task_reference_destroy"

    def __init__(self, seqs, device=0):
        super().__init__(lib())
        self.index = {name: k for k, name in enumerate(seqs)}
        recs = np.zeros(len(seqs), dtype=SEQ_DTYPE)
        off = 0
        for k, s in enumerate(seqs.values()):
            recs[k] = (off, len(s))
            off += len(s)
        data = np.frombuffer(b"".join(bytes(s) for s in seqs.values()), dtype=np.uint8)
        rc = self._lib.task_reference_create(device, _ptr(data), data.size, _ptr(recs), len(recs), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "task_reference_create", rc)


class Exons(capi.Owned):
    """The exon table on one device (task_exons_create).  `table`: {transcript: (gene, chromosome, strand, [(start, end)])};
    transcripts are numbered in ascending name order, the order of the reference's output.  `names`: the dense reference
    numbering ({name: index}), extended here by every chromosome and every "gene|transcript" it does not have yet."""
    _destroy = "task_exons_destroy"

    def __init__(self, table, names, device=0):
        super().__init__(lib())
        self.transcripts = sorted(table)
        self.tindex = {t: k for k, t in enumerate(self.transcripts)}
        self.cindex = {}
        tx = np.zeros(len(table), dtype=TRANSCRIPT_DTYPE)
        exons = []
        for k, t in enumerate(self.transcripts):
            gene, chrom, strand, ex = table[t]
            c = self.cindex.setdefault(chrom, len(self.cindex))
            names.setdefault(chrom, len(names))
            tx[k] = (c, strand, len(exons), len(ex), names.setdefault(gene + "|" + t, len(names)))
            exons.extend(ex)
        chrom_ref = np.array([names[c] for c in self.cindex], dtype=np.int32)
        ex = np.array(exons, dtype=np.int32).reshape(-1, 2).view(EXON_DTYPE).reshape(-1)
        rc = self._lib.task_exons_create(device, _ptr(chrom_ref), len(chrom_ref), _ptr(tx), len(tx), _ptr(ex), len(ex), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "task_exons_create", rc)


class _Borrowed:
    """A bat_windows / pred_tasks owned by a Store: quacks like bat.Windows / pred.Tasks (.handle), never destroyed here."""

    def __init__(self, handle, owner):
        self.handle = ctypes.c_void_p(handle)
        self.owner = owner


def pairs_from_regions(regions, reference, exons):
    """{fusion_id: [loc0, loc1]} with loc = dict(refName, strand, start, end) (oracle.read_align_region_pairs) -> PAIR_DTYPE
    array: the names resolved as SplitAlignmentTask::Initialize reads them (ParseTranscriptID: the second field of a name with
    '|', if the exon table has it)."""
    out = np.zeros(len(regions), dtype=PAIR_DTYPE)
    for k, (fid, pair) in enumerate(regions.items()):
        out[k]["fusion_id"] = fid
        for e in (0, 1):
            loc = pair[e]
            parts = loc["refName"].split("|")
            tr = exons.tindex.get(parts[1], -1) if len(parts) >= 2 else -1
            out[k]["end"][e] = (reference.index.get(loc["refName"], -1), tr, exons.cindex.get(loc["refName"], -1), loc["strand"], loc["start"], loc["end"])
    return out


class Store(capi.Owned):
    """All tasks of a run on one device (task_store_create).  .windows / .tasks stand where a bat.Windows / pred.Tasks do."""
    _destroy = "task_store_destroy"

    def __init__(self, reference, exons, params, pairs):
        super().__init__(lib())
        pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        prm = Params(*[int(v) for v in params])
        rc = self._lib.task_store_create(reference.handle, exons.handle, ctypes.byref(prm), _ptr(pairs), len(pairs), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "task_store_create", rc)
        self.windows = _Borrowed(self._lib.task_store_windows(self.handle), self)
        self.tasks = _Borrowed(self._lib.task_store_pred_tasks(self.handle), self)
        self.tasks.windows = self.windows

    def counts(self):
        c = Counts()
        rc = self._lib.task_store_counts(self.handle, ctypes.byref(c))
        if rc != 0:
            _fail(self._lib, "task_store_counts", rc)
        return c

    def fetch(self):
        """(records, window_bytes, rem_bytes, regions): RECORD_DTYPE, uint8, uint8, cand.REGION_DTYPE."""
        c = self.counts()
        rec = np.zeros(c.n_tasks, dtype=RECORD_DTYPE)
        win = np.zeros(c.window_bytes, dtype=np.uint8)
        rem = np.zeros(c.rem_bytes, dtype=np.uint8)
        reg = np.zeros(c.n_regions, dtype=cand.REGION_DTYPE)
        rc = self._lib.task_store_fetch(self.handle, _ptr(rec), len(rec), _ptr(win), len(win), _ptr(rem), len(rem), _ptr(reg), len(reg))
        if rc != 0:
            _fail(self._lib, "task_store_fetch", rc)
        return rec, win, rem, reg

    def timing(self):
        t = TaskTiming()
        rc = self._lib.task_store_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "task_store_get_timing", rc)
        return capi.as_dict(t)
