"""The host reader of the gene models (GTF) and the ctypes binding of the section "concordant clusters" of include/defuse_task.h: the concordant-cluster filter
(prep_local_alignment_seqs.pl, localalign and `filter_column.pl VALUES 0 1`) on cluster text in device memory; test/bench
plumbing only.

read_gene_models restates gene_models::new (scripts/gene_models.pm:10-186) as far as the filter reads it; GeneModels.flatten
turns it into the arrays conc_models_create takes."""
import ctypes
import re

import numpy as np

from . import capi, clusterregions
from .capi import ptr as _ptr

DSA_E_CAPACITY, DSA_E_DEVICE, DSA_E_ARG, DSA_E_LIMIT = capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT
FEW_FIELDS, BAD_INTEGER, NOT_TWO_ENDS, BAD_STRAND, EMPTY_NAME, NO_OTHER_SEQ, EMPTY_OTHER = 1, 2, 3, 4, 5, 6, 7
ALIGN_TEXT, FILTERED = 0, 1
KIND_GENOMIC, KIND_TRANSCRIPT = 0, 1
CONSTANTS = {"CONC_FEW_FIELDS": FEW_FIELDS, "CONC_BAD_INTEGER": BAD_INTEGER, "CONC_NOT_TWO_ENDS": NOT_TWO_ENDS, "CONC_BAD_STRAND": BAD_STRAND,
             "CONC_EMPTY_NAME": EMPTY_NAME, "CONC_NO_OTHER_SEQ": NO_OTHER_SEQ, "CONC_EMPTY_OTHER": EMPTY_OTHER, "CONC_ALIGN_TEXT": ALIGN_TEXT,
             "CONC_FILTERED": FILTERED, "CONC_KIND_GENOMIC": KIND_GENOMIC, "CONC_KIND_TRANSCRIPT": KIND_TRANSCRIPT}

ACCEPTED = ("CDS", "exon", "start_codon", "stop_codon")

GENE_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("tx_first", "<i4"), ("tx_count", "<i4")])
TRANSCRIPT_DTYPE = np.dtype([("gene", "<i4"), ("chrom", "<i4"), ("strand", "<i4"), ("exon_first", "<i4"), ("exon_count", "<i4"), ("expr_first", "<i4"),
                             ("expr_count", "<i4"), ("pad_", "<i4")])
INTERVAL_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4")])
NAME_DTYPE = np.dtype([("off", "<i8"), ("len", "<i4"), ("pad_", "<i4")])
TARGET_DTYPE = np.dtype([("cluster_id", "<i4"), ("cluster_end", "<i4"), ("kind", "<i4"), ("name", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("len", "<i4"),
                         ("revcomp", "<i4"), ("other_seq", "<i4"), ("other_start", "<i4"), ("other_len", "<i4"), ("other_rev", "<i4")])
assert TARGET_DTYPE.itemsize == 48


class GeneModels:
    """What gene_models::new keeps of a GTF, as far as prep_local_alignment_seqs.pl reads it.  Names are str with one
    character per byte (latin-1), so that str order is byte order."""

    def __init__(self):
        self.transcripts = {}       # "gene|transcript" -> dict(gene, chromosome, strand, exons, cds (or None), utr5p, utr3p)
        self.genes = {}             # gene id -> dict(chromosome, strand, transcripts {name: 1}, region)
        self.chromosomes = {}       # name -> {gene id: 1}: a chromosome is known iff an accepted line names it

    def flatten(self):
        """The arrays of conc_models_desc: chromosomes and transcripts in ascending order of their name bytes, genes in ascending
        order of their id bytes, every gene's transcripts in ascending order of their names, every chromosome's genes in
        ascending order of (region start, gene index)."""
        chroms, txs, genes = sorted(self.chromosomes), sorted(self.transcripts), sorted(self.genes)
        cidx, tidx, gidx = ({n: k for k, n in enumerate(v)} for v in (chroms, txs, genes))
        g_arr, gene_tx = np.zeros(len(genes), dtype=GENE_DTYPE), []
        for k, g in enumerate(genes):
            mine = sorted(self.genes[g]["transcripts"])
            g_arr[k] = (self.genes[g]["region"][0], self.genes[g]["region"][1], len(gene_tx), len(mine))
            gene_tx += [tidx[t] for t in mine]
        t_arr, exons, expr = np.zeros(len(txs), dtype=TRANSCRIPT_DTYPE), [], []
        for k, t in enumerate(txs):
            tr = self.transcripts[t]
            mine = (tr["cds"] or []) + tr["utr5p"] + tr["utr3p"]
            t_arr[k] = (gidx[tr["gene"]], cidx[tr["chromosome"]], {"+": 0, "-": 1}.get(tr["strand"], 2), len(exons), len(tr["exons"]), len(expr), len(mine), 0)
            exons += tr["exons"]
            expr += mine
        first, cg = [0], []
        for c in chroms:
            cg += sorted((gidx[g] for g in self.chromosomes[c]), key=lambda i: (int(g_arr[i]["start"]), i))
            first.append(len(cg))
        return dict(chrom_names=chroms, transcript_names=txs, gene_names=genes, genes=g_arr, gene_tx=np.array(gene_tx, dtype=np.int32), transcripts=t_arr,
                    exons=np.array(exons, dtype=np.int64).reshape(-1, 2).astype(np.int32).view(INTERVAL_DTYPE).reshape(-1),
                    expressed=np.array(expr, dtype=np.int64).reshape(-1, 2).astype(np.int32).view(INTERVAL_DTYPE).reshape(-1),
                    chrom_gene_first=np.array(first, dtype=np.int32), chrom_genes=np.array(cg, dtype=np.int32))


def read_gene_models(text):
    """gene_models::new over the bytes of a GTF.  ValueError where the script dies: a short line, a line without gene_id,
    transcript_id or gene_name, a coordinate that is no integer, a transcript without an exon line."""
    m = GeneModels()
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    for n, line in enumerate(text.split("\n"), 1):
        if line.startswith("#") or (line == "" and n == text.count("\n") + 1):
            continue
        f = line.split("\t")
        if len(f) < 9:
            raise ValueError("gtf line %d has %d fields" % (n, len(f)))
        chromosome, ftype, strand = f[0], f[2], f[6]
        if ftype not in ACCEPTED:
            continue
        try:
            start, end = int(f[3]), int(f[4])
        except ValueError:
            raise ValueError("gtf line %d: a coordinate that is no integer" % n)
        attr = {}
        for feature in f[8].split(";"):
            hit = re.search(r"(\S+)\s+(.*)", feature)
            if hit:
                attr[hit.group(1)] = hit.group(2).replace('"', "")
        for key in ("gene_id", "transcript_id", "gene_name"):
            if key not in attr:
                raise ValueError("gtf line %d has no %s" % (n, key))
        gene, name = attr["gene_id"], attr["gene_id"] + "|" + attr["transcript_id"]
        tr = m.transcripts.setdefault(name, dict(exons=[], cds=None, utr5p=[], utr3p=[]))
        tr.update(gene=gene, chromosome=chromosome, strand=strand)
        if ftype == "exon":
            tr["exons"].append((start, end))
        if ftype == "CDS":
            tr["cds"] = (tr["cds"] or []) + [(start, end)]
        g = m.genes.setdefault(gene, dict(transcripts={}))
        g.update(chromosome=chromosome, strand=strand)
        g["transcripts"][name] = 1
        m.chromosomes.setdefault(chromosome, {})[gene] = 1
    for name, tr in m.transcripts.items():
        if not tr["exons"]:
            raise ValueError("transcript %s has no exon line" % name)
        tr["exons"].sort(key=lambda e: e[0])                    # (stable, as Perl's merge sort)
        if tr["cds"] is not None:
            tr["cds"].sort(key=lambda e: e[0])
    for g in m.genes.values():
        mine = [m.transcripts[t]["exons"] for t in g["transcripts"]]
        g["region"] = (min(e[0][0] for e in mine), max(e[-1][1] for e in mine))     # the end of the LAST-SORTED exon
    for tr in m.transcripts.values():                           # gene_models.pm:139-182
        if tr["cds"] is None:
            continue
        coding_start, coding_end = tr["cds"][0][0], tr["cds"][-1][1]
        plus = tr["strand"] == "+"
        for s, e in tr["exons"]:
            if s < coding_start:
                tr["utr5p" if plus else "utr3p"].append((s, min(e, coding_start - 1)))
            elif e > coding_end:                                # (an exon that starts before the coding start never gets here)
                tr["utr3p" if plus else "utr5p"].append((max(s, coding_end + 1), e))
    return m


def read_fasta(text):
    """{name: bytes} of a FASTA in file order; the name is the header up to the first white space, as Bio::DB::Fasta keys it."""
    seqs, name = {}, None
    for line in bytes(text).split(b"\n"):
        line = line.rstrip(b"\r")
        if line.startswith(b">"):
            name = line[1:].split()[0].decode("latin-1") if line[1:].split() else ""
            seqs[name] = []
        elif name is not None:
            seqs[name].append(line)
    return {n: b"".join(v) for n, v in seqs.items()}


i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
p, cint = ctypes.c_void_p, ctypes.c_int


class ModelsDesc(ctypes.Structure):
    _fields_ = [("genes", p), ("gene_tx", p), ("transcripts", p), ("exons", p), ("expressed", p), ("chrom_gene_first", p), ("chrom_genes", p), ("names", p),
                ("chrom_names", p), ("transcript_names", p), ("seq_names", p), ("n_genes", i64), ("n_gene_tx", i64), ("n_transcripts", i64), ("n_exons", i64),
                ("n_expressed", i64), ("n_chrom_genes", i64), ("names_len", i64), ("n_chroms", i64), ("n_seqs", i64)]


class ConcResult(ctypes.Structure):
    _fields_ = [("n_lines", i64), ("n_clusters", i64), ("n_targets", i64), ("n_kept_targets", i64), ("align_bytes", i64), ("n_hit_clusters", i64),
                ("n_kept_lines", i64), ("out_bytes", i64), ("n_noncanonical", i64), ("stop_line", i64), ("stop_value", i64), ("stop_kind", i32),
                ("stop_field", i32)]


class ConcTiming(ctypes.Structure):
    _fields_ = [("targets_ms", f32), ("sort_ms", f32), ("download_ms", f32), ("pack_ms", f32), ("dp_ms", f32), ("print_ms", f32), ("filter_ms", f32),
                ("pad_", f32), ("cells", i64), ("n_packed16", i64), ("n_int32", i64)]


class Target(ctypes.Structure):
    _fields_ = [(n, i32) for n in TARGET_DTYPE.names]


STRUCTS = {"conc_models_desc": ModelsDesc, "conc_result": ConcResult, "conc_timing": ConcTiming, "conc_target": Target}

PROTOTYPES = {
    "conc_models_create": (cint, [cint, ctypes.POINTER(ModelsDesc), ctypes.POINTER(p)]),
    "conc_models_destroy": (None, [p]),
    "conc_create": (cint, [cint, ctypes.POINTER(p)]),
    "conc_destroy": (None, [p]),
    "conc_targets": (cint, [p, p, p, p, i32, ctypes.POINTER(ConcResult)]),
    "conc_fetch_targets": (cint, [p, p, i64]),
    "conc_align": (cint, [p, p, i32, i32, i32, ctypes.c_double, ctypes.POINTER(ConcResult)]),
    "conc_fetch_scores": (cint, [p, p, i64]),
    "conc_filter": (cint, [p, ctypes.POINTER(ConcResult)]),
    "conc_fetch": (cint, [p, i32, i64, p, i64]),
    "conc_get_timing": (cint, [p, ctypes.POINTER(ConcTiming)]),
    "conc_last_error": (ctypes.c_char_p, []),
    "conc_into_taskc": (cint, [p, p]),
}
EXPORTS = list(PROTOTYPES)


class ConcFilterError(capi.ApiError):
    prefix = "concfilter"


def lib():
    """The library with the conc_ functions of include/defuse_task.h bound."""
    return capi.bind(clusterregions.lib(), PROTOTYPES)


def _fail(lib, what, rc):
    raise ConcFilterError(rc, "%s: %s" % (what, lib.conc_last_error().decode()))


def _names(pool, names):
    arr = np.zeros(len(names), dtype=NAME_DTYPE)
    for k, n in enumerate(names):
        b = n.encode("latin-1")
        arr[k] = (len(pool), len(b), 0)
        pool += b
    return arr


class Models(capi.Owned):
    """conc_models_create: the flattened gene models and the names of the reference's sequences on one device.  `models` is a
    GeneModels, `seq_names` the names of a task.Reference in its order."""
    _destroy = "conc_models_destroy"

    def __init__(self, models, seq_names, device=0):
        super().__init__(lib())
        self.flat = f = models.flatten()
        self.seq_names = list(seq_names)
        pool = bytearray()
        cn, tn, sn = _names(pool, f["chrom_names"]), _names(pool, f["transcript_names"]), _names(pool, self.seq_names)
        pool = np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8)
        d = ModelsDesc(_ptr(f["genes"]), _ptr(f["gene_tx"]), _ptr(f["transcripts"]), _ptr(f["exons"]), _ptr(f["expressed"]), _ptr(f["chrom_gene_first"]),
                       _ptr(f["chrom_genes"]), _ptr(pool), _ptr(cn), _ptr(tn), _ptr(sn), len(f["genes"]), len(f["gene_tx"]), len(f["transcripts"]),
                       len(f["exons"]), len(f["expressed"]), len(f["chrom_genes"]), len(pool) - 1, len(cn), len(sn))
        rc = self._lib.conc_models_create(int(device), ctypes.byref(d), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "conc_models_create", rc)


class Context(capi.Owned):
    """One conc_ctx (one device): the targets, scores, local.align text and filtered cluster text of the last call sequence."""
    _destroy = "conc_destroy"
    result = None

    def __init__(self, device=0):
        super().__init__(lib())
        rc = self._lib.conc_create(int(device), ctypes.byref(self.handle))
        if rc != 0:
            _fail(self._lib, "conc_create", rc)

    def _call(self, name, *args):
        res = ConcResult()
        rc = getattr(self._lib, name)(self.handle, *args, ctypes.byref(res))
        if rc != 0:
            _fail(self._lib, name, rc)
        self.result = capi.as_dict(res)
        return self.result

    def targets(self, clusters, models, reference, seq_range):
        """conc_targets over the cluster text of a clusterregions.Context."""
        return self._call("conc_targets", clusters.handle, models.handle, reference.handle, int(seq_range))

    def fetch_targets(self):
        out = np.zeros(self.result["n_targets"], dtype=TARGET_DTYPE)
        rc = self._lib.conc_fetch_targets(self.handle, _ptr(out), len(out))
        if rc != 0:
            _fail(self._lib, "conc_fetch_targets", rc)
        return out

    def align(self, reference, match, mismatch, gap, threshold):
        return self._call("conc_align", reference.handle, int(match), int(mismatch), int(gap), float(threshold))

    def fetch_scores(self):
        out = np.zeros(self.result["n_targets"], dtype=np.int32)
        rc = self._lib.conc_fetch_scores(self.handle, _ptr(out), len(out))
        if rc != 0:
            _fail(self._lib, "conc_fetch_scores", rc)
        return out

    def filter(self):
        return self._call("conc_filter")

    def fetch(self, which):
        """The local.align text (ALIGN_TEXT) or the filtered cluster text (FILTERED) of the last conc_filter."""
        n = self.result["align_bytes" if which == ALIGN_TEXT else "out_bytes"]
        buf = np.zeros(max(n, 0), dtype=np.uint8)
        rc = self._lib.conc_fetch(self.handle, int(which), 0, _ptr(buf), int(n))
        if rc != 0:
            _fail(self._lib, "conc_fetch", rc)
        return buf.tobytes()

    def timing(self):
        t = ConcTiming()
        rc = self._lib.conc_get_timing(self.handle, ctypes.byref(t))
        if rc != 0:
            _fail(self._lib, "conc_get_timing", rc)
        return capi.as_dict(t)


def add_conc(clusters, conc):
    """conc_into_taskc: the filtered text of a Context behind the text of a clusterregions.Context, device to device."""
    bound = lib()
    rc = bound.conc_into_taskc(conc.handle, clusters.handle)
    if rc != 0:
        raise ConcFilterError(rc, "conc_into_taskc: %s" % bound.conc_last_error().decode())
