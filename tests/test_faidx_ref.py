"""FASTA index and region fetch: the oracle's FastaIndex (oracle/dosplitalign_oracle.py) and the index file the tools write
against the REFERENCE'S OWN code — faidx.c of the vendored samtools 0.1.8 (external/samtools-0.1.8), which tools/FastaIndex.cpp
wraps, compiled as it lies (oracle/Makefile: oracle/_ref/libfaidx_ref.so).  The window and remainder sequences of every
fusion, and the clipped start / length values the break positions are computed from (SURVEY a-5), come through this call.
Its answers on the inputs below are recorded by tests/golden/make_ref_answers.py into tests/golden/ref_answers/ (faidx.npz:
the fetches, ref.fa.fai: fai_build's index)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_answers")


@pytest.fixture(scope="module")
def faidx(built):
    """The reference's recorded fetches: (name, start, length) -> (sequence, start, length), in fetch_cases() order."""
    d = np.load(os.path.join(GOLDEN, "faidx.npz"))
    ends = np.cumsum(d["seq_len"])
    seq = d["seq"].tobytes()
    names = [str(n) for n in d["names"]]
    cases = []
    for i in range(len(d["start"])):
        s = seq[ends[i] - d["seq_len"][i]:ends[i]]
        cases.append(((names[d["name_idx"][i]], int(d["start"][i]), int(d["length"][i])), (s, int(d["ref_start"][i]), int(d["ref_length"][i]))))
    return {"fasta_sha256": str(d["fasta_sha256"]), "cases": cases}


def load_faidx(path):
    """ctypes bindings of the reference's faidx (tests/golden/make_ref_answers.py records its answers with them)."""
    lib = C.CDLL(path)
    lib.fai_load.restype = C.c_void_p
    lib.fai_load.argtypes = [C.c_char_p]
    lib.fai_fetch.restype = C.c_void_p
    lib.fai_fetch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.fai_build.argtypes = [C.c_char_p]
    lib.fai_destroy.argtypes = [C.c_void_p]
    return lib


def write_fasta(path, seed=5):
    """The FASTA of both tests; returns name -> sequence.  Its bytes must be those faidx.npz was recorded on."""
    rng = np.random.default_rng(seed)
    seqs = {}
    with open(path, "wb") as f:
        for k, (name, n, width) in enumerate((("chr1", 1000, 60), ("ENSG01|ENST01", 333, 70), ("short", 7, 60), ("chrM", 601, 50),
                                               ("lower", 240, 60), ("oneline", 95, 200))):
            s = bytes(rng.choice(np.frombuffer(b"ACGTN" if k != 4 else b"acgtn", dtype=np.uint8), size=n))
            seqs[name] = s
            f.write(b">" + name.encode() + (b" description text\n" if k % 2 else b"\n"))
            for o in range(0, n, width):
                f.write(s[o:o + width] + b"\n")
    return seqs


def ref_get(lib, fai, reference, start, length):
    """FastaIndex::Get (tools/FastaIndex.cpp:23-61) around the reference's fai_fetch, plus strand."""
    if length < 0:
        return b"", start, length
    if start < 1:
        length -= 1 - start
        start = 1
    end = start + length - 1
    n = C.c_int(length)
    p = lib.fai_fetch(fai, ("%s:%d-%d" % (reference, start, end)).encode(), C.byref(n))
    assert p
    s = C.string_at(p)
    C.CDLL("libc.so.6").free(C.c_void_p(p))
    return s, start, n.value


def fetch_cases(seqs):
    """(name, start, length) of every fetch the test makes, clipped and out-of-range ones included."""
    rng = np.random.default_rng(9)
    for name, s in seqs.items():
        L = len(s)
        cases = [(1, L), (1, 1), (L, 1), (L, 5), (L + 1, 3), (L + 50, 10), (0, 10), (-5, 3), (-5, 20), (-100, 50), (5, 0), (5, -1),
                 (1, L + 100), (2, L - 2)]
        cases += [(int(rng.integers(-30, L + 30)), int(rng.integers(-2, L + 40))) for _ in range(300)]
        for start, length in cases:
            yield name, start, length


def check_fasta(path, faidx):
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == faidx["fasta_sha256"], \
        "the test FASTA changed since faidx.npz was recorded: tests/golden/make_ref_answers.py"


def test_region_fetch_equals_the_reference(faidx, tmp_path):
    from oracle import dosplitalign_oracle as ora
    fa = str(tmp_path / "ref.fa")
    seqs = write_fasta(fa)
    check_fasta(fa, faidx)
    o = ora.FastaIndex(fa)
    assert [c for c, _ in faidx["cases"]] == list(fetch_cases(seqs))
    n_checked = 0
    for (name, start, length), exp in faidx["cases"]:
        got = o.get(name, ora.PLUS, start, length)
        assert (got[0], got[1], got[2]) == exp, (name, start, length)
        n_checked += 1
        rc = o.get(name, ora.MINUS, start, length)
        assert rc[0] == ora.reverse_complement(exp[0]) and rc[1:] == exp[1:]
    assert n_checked > 1500


def test_index_file_of_the_tools_equals_the_reference(faidx, tmp_path):
    """bin/dosplitalign builds <fasta>.fai when it is missing, as fai_load does; the bytes must be fai_build's."""
    from defuse_amd import build
    build.build_tools()
    b = tmp_path / "b"
    os.makedirs(b)
    write_fasta(str(b / "ref.fa"))
    check_fasta(str(b / "ref.fa"), faidx)
    (b / "exons.txt").write_text("g\tt\tchr1\t+\t1\t900\t\n")
    (b / "regions.txt").write_text("0\t0\tchr1\t+\t300\t400\n0\t1\tchr1\t-\t700\t800\n")
    (b / "improper.sam").write_text("@HD\tVN:1.0\n")
    for e in (1, 2):
        (b / ("reads.%d.fastq" % e)).write_text("@0/%d\nACGT\n+\nIIII\n" % e)
    r = subprocess.run([os.path.join(ROOT, "bin", "dosplitalign"), "-f", str(b / "ref.fa"), "-e", str(b / "exons.txt"), "-u", "200", "-s", "30",
                        "-n", "50", "-x", "50", "-r", str(b / "regions.txt"), "-i", str(b / "improper.sam"), "-1", str(b / "reads.1.fastq"),
                        "-2", str(b / "reads.2.fastq"), "-a", str(b / "out.align")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "[fai_load] build FASTA index." in r.stderr
    with open(os.path.join(GOLDEN, "ref.fa.fai"), "rb") as f:
        assert (b / "ref.fa.fai").read_bytes() == f.read()
