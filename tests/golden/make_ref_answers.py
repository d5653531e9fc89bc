"""Generates tests/golden/ref_answers/: the answers of the reference's own code on the inputs of tests/test_asa_ref.py,
tests/test_faidx_ref.py and tests/test_cli_ref.py, so that those tests run from the repository alone.  The reference's code is
what oracle/Makefile compiles into oracle/_ref/ where the reference sources are present (AS 136 / AS 241, samtools' faidx,
TCLAP); run this where that was done, after `make -C oracle`.  The fixtures it writes are what travels.

    python tests/golden/make_ref_answers.py

asa.npz     kmns (AS 136) on every case of kmns_cases() plus the ifault-3 calls, r8_normal_01_cdf_inverse (AS 241) on
            cdf_points(), and the known-answer table asa241.C carries (normal_01_cdf_values)
faidx.npz   fai_fetch through FastaIndex::Get on every case of fetch_cases(), the FASTA they were taken from
ref.fa.fai  fai_build's index of that FASTA
tclap.json  return code, stdout and stderr of TCLAP on every command line the CLI tests hold the tools against
Every file records a digest of the inputs it was made from; the tests check it, so that inputs which no longer match the
recording are reported as such."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ref_answers")
REF = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, ROOT)

from oracle import mpe_c  # noqa: E402
from tests import test_asa_ref as ta, test_cli_ref as tc, test_faidx_ref as tf  # noqa: E402


def asa():
    assert mpe_c.ref() is not None, "oracle/_ref/libasa_ref.so is not built"
    d = {k: [] for k in ("m", "k", "fault", "ic1", "nc", "wss", "c")}
    for m, k, pts, seeds in ta.kmns_cases():
        a = np.concatenate([pts[:, 0], pts[:, 1]])
        c = np.concatenate([seeds[:, 0], seeds[:, 1]])
        ic1, nc, wss, cc, fault = mpe_c.ref_kmns(a, m, 2, c, k)
        for key, v in (("m", [m]), ("k", [k]), ("fault", [fault]), ("ic1", ic1), ("nc", nc), ("wss", wss), ("c", cc)):
            d[key].append(np.asarray(v))
    out = {key: np.concatenate(v) for key, v in d.items()}
    out["fault_small"] = np.array([mpe_c.ref_kmns(*args)[4] for args in ta.SMALL_KMNS], dtype=np.int32)
    ps = ta.cdf_points()
    out["cdf_p"] = ps
    out["cdf_inverse"] = np.array([mpe_c.ref()._Z24r8_normal_01_cdf_inversed(float(p)) for p in ps])
    n, x, fx = C.c_int(0), C.c_double(0), C.c_double(0)
    tx, tfx = [], []
    while True:
        mpe_c.ref()._Z20normal_01_cdf_valuesPiPdS0_(C.byref(n), C.byref(x), C.byref(fx))
        if n.value == 0:
            break
        tx.append(x.value)
        tfx.append(fx.value)
    out["table_x"], out["table_fx"] = np.array(tx), np.array(tfx)
    out["inputs_sha256"] = np.array(ta.inputs_digest())
    np.savez_compressed(os.path.join(OUT, "asa.npz"), **out)


def faidx():
    lib = tf.load_faidx(os.path.join(REF, "libfaidx_ref.so"))
    d = tempfile.mkdtemp()
    try:
        fa = os.path.join(d, "ref.fa")
        seqs = tf.write_fasta(fa)
        fai = lib.fai_load(fa.encode())
        assert fai
        shutil.copy(fa + ".fai", os.path.join(OUT, "ref.fa.fai"))
        names, starts, lengths, got_start, got_len, blob = [], [], [], [], [], []
        for name, start, length in tf.fetch_cases(seqs):
            s, st, ln = tf.ref_get(lib, fai, name, start, length)
            names.append(list(seqs).index(name))
            starts.append(start)
            lengths.append(length)
            got_start.append(st)
            got_len.append(ln)
            blob.append(s)
        lib.fai_destroy(fai)
        fasta = open(fa, "rb").read()
    finally:
        shutil.rmtree(d)
    seq_len = [len(s) for s in blob]
    np.savez_compressed(os.path.join(OUT, "faidx.npz"), names=np.array(list(seqs)), name_idx=np.array(names, dtype=np.int32),
                        start=np.array(starts, dtype=np.int64), length=np.array(lengths, dtype=np.int64),
                        ref_start=np.array(got_start, dtype=np.int64), ref_length=np.array(got_len, dtype=np.int64),
                        seq_len=np.array(seq_len, dtype=np.int64), seq=np.frombuffer(b"".join(blob), dtype=np.uint8),
                        fasta_sha256=np.array(hashlib.sha256(fasta).hexdigest()))


def tclap():
    driver = os.path.join(REF, "tclap_ref")
    assert os.path.exists(driver), "oracle/_ref/tclap_ref is not built"

    def run(tool, args):
        message, spec = tc.SPECS[tool]
        cmd = [driver, tool, message, str(len(spec))]
        for (flag, name, desc, typ, req) in spec:
            cmd += [flag, name, desc, typ, str(req)]
        r = subprocess.run(cmd + ["--"] + args, capture_output=True, text=True)
        return {"args": args, "returncode": r.returncode, "stdout": r.stdout, "stderr": r.stderr}
    lines = [(tool, args) for tool in sorted(tc.SPECS) for args in tc.failing_lines(tool)]
    lines += [("dosplitalign", args) for args in tc.FUSED_LINES] + [("localalign", args) for args in tc.PARSED_LINES]
    out = {"specs_sha256": tc.specs_digest(), "answers": {}}
    for tool, args in lines:
        out["answers"].setdefault(tool, []).append(run(tool, args))
    with open(os.path.join(OUT, "tclap.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    asa()
    faidx()
    tclap()
    print("wrote", OUT)
