"""txt_parse_sam and txt_fastq_add of include/defuse_text.h on the text of one chunk, and the tools' host parsers over the
same bytes on 16 threads (profiles/microbench/text_host.cpp).

    g++ -std=c++17 -O2 -pthread -o profiles/microbench/text_host profiles/microbench/text_host.cpp
    python profiles/microbench/text_throughput.py [--fragments 1000000] [--alignments 1300000] [--out profiles/text/result.json]

The chunk has the shape of e2e_scale.py's chunks (its fixed-width lines, written by its text_rows): 1 M fragments of 2x150 bp
in two FASTQ files of 317-byte records, and improper-mate SAM records of 348 bytes with qnames "<fragment>/<end>", on 24
reference names.

What is timed.  Device: the three HIP-event times of txt_get_timing per call - upload (the pageable host text to the device),
device (every kernel and scan of the call, the waits for its two small counts included), download (txt_sam_fetch of the
alignments) - and the wall time of the call (time.perf_counter around the ctypes call).  One warm-up call of each kind, then
the median of --repeats.  Host: text_host's steady_clock around 16 threads, the median of its repeats after one warm-up."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
RL, THREADS = 150, 16


def make_chunk(n_fragments, n_alignments, seed=3):
    from e2e_scale import digits, text_rows
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    qual = np.full((1, RL), ord("I"), dtype=np.uint8)
    frag = np.arange(n_fragments)
    fastq = []
    for e in (1, 2):
        reads = acgt[rng.integers(0, 4, size=(n_fragments, RL), dtype=np.uint8)]
        fastq.append(text_rows(n_fragments, [b"@", digits(frag, 9), b"/%d\n" % e, reads, b"\n+\n", np.broadcast_to(qual, (n_fragments, RL)), b"\n"]))
    a_frag = np.sort(rng.integers(0, n_fragments, size=n_alignments))
    seq = np.full((1, RL), ord("A"), dtype=np.uint8)
    sam = text_rows(n_alignments, [digits(a_frag, 9), b"/", digits(rng.integers(1, 3, size=n_alignments), 1), b"\t", digits(16 * rng.integers(0, 2, size=n_alignments), 2),
                                   b"\tchr", digits(rng.integers(1, 25, size=n_alignments), 2), b"\t", digits(rng.integers(1, 60_000_000, size=n_alignments), 9),
                                   b"\t255\t150M\t*\t0\t0\t", np.broadcast_to(seq, (n_alignments, RL)), b"\t", np.broadcast_to(qual, (n_alignments, RL)), b"\n"])
    return sam, fastq


def median_of(rows, key):
    return statistics.median(r[key] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=1_000_000)
    ap.add_argument("--alignments", type=int, default=1_300_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text", "result.json"))
    ap.add_argument("--host", default=os.path.join(HERE, "text_host"), help="the built text_host.cpp, '' to skip")
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    a = ap.parse_args()
    from defuse_amd import dsa, text
    sam, fastq = make_chunk(a.fragments, a.alignments)
    names = ["chr%02d" % k for k in range(1, 25)]
    sam_bytes, fastq_bytes = sam.size, sum(f.size for f in fastq)
    res = dict(fragments=a.fragments, alignments=a.alignments, sam_bytes=int(sam_bytes), fastq_bytes=int(fastq_bytes), sam_record_bytes=int(sam.shape[1]),
               fastq_record_bytes=int(fastq[0].shape[1]), library=dsa.load_library().dsa_version().decode(), sam_runs=[], fastq_runs=[], host={})
    with text.Names(names) as nm, text.Context(nm) as T:
        for rep in range(a.repeats + 1):                       # the first is the warm-up: buffers grow, code objects load
            t0 = time.perf_counter()
            r = T.parse_sam(sam.reshape(-1))
            wall = (time.perf_counter() - t0) * 1e3
            assert (r.n_alignments, r.stop_kind, r.n_bad_fragment) == (a.alignments, 0, 0)
            T.sam_alignments()
            t = T.timing()
            run = dict(wall_ms=wall, upload_ms=t["upload_ms"], device_ms=t["device_ms"], download_ms=t["download_ms"])
            T.fastq_begin()
            fq_run = dict(wall_ms=0.0, upload_ms=0.0, device_ms=0.0)
            for f in fastq:
                t0 = time.perf_counter()
                r = T.fastq_add(f.reshape(-1))
                fq_run["wall_ms"] += (time.perf_counter() - t0) * 1e3
                assert (r.n_records, r.stop_kind) == (a.fragments, 0)
                t = T.timing()
                fq_run["upload_ms"] += t["upload_ms"]
                fq_run["device_ms"] += t["device_ms"]
            v = T.fastq_view()
            assert (v.n_reads, v.bytes_len) == (2 * a.fragments, 2 * a.fragments * RL)
            if rep:
                res["sam_runs"].append(run)
                res["fastq_runs"].append(fq_run)
            print(json.dumps(dict(sam=run, fastq=fq_run)), flush=True)
    for kind, rows, nbytes in (("sam", res["sam_runs"], sam_bytes), ("fastq", res["fastq_runs"], fastq_bytes)):
        med = {k: median_of(rows, k) for k in rows[0]}
        med["device_gb_per_s"] = nbytes / med["device_ms"] / 1e6
        med["upload_gb_per_s"] = nbytes / med["upload_ms"] / 1e6
        res[kind + "_median"] = med
    if a.host and os.path.exists(a.host):
        d = tempfile.mkdtemp(dir=a.tmp)
        try:
            for kind, arrays in (("sam", [sam]), ("fastq", fastq)):
                pieces = []
                for j, arr in enumerate(arrays):                  # cut at record starts: rows of one width
                    per = -(-len(arr) // (THREADS // len(arrays)))
                    for k in range(THREADS // len(arrays)):
                        path = os.path.join(d, "%s.%d.%d.%s" % (kind, j, k, "fastq" if kind == "fastq" else "sam"))
                        arr[k * per:(k + 1) * per].tofile(path)
                        pieces.append(path)
                out = subprocess.run([a.host, kind, str(a.repeats + 1)] + pieces, capture_output=True, text=True, check=True).stdout.splitlines()
                ms = [float(l.split()[4]) for l in out[1:]]
                records = {int(l.split()[6]) for l in out}
                assert records == {a.alignments if kind == "sam" else 2 * a.fragments}, out
                res["host"][kind] = dict(threads=len(pieces), lines=out, median_ms=statistics.median(ms))
                print("\n".join(out), flush=True)
                for p in pieces:
                    os.remove(p)
        finally:
            os.rmdir(d)
    print(json.dumps({k: res[k] for k in ("sam_median", "fastq_median")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
