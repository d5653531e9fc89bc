"""Table build and candidate enumeration of include/defuse_cand.h on a chunk-sized problem, and the same work through the
dosplitalign tool's host classes (profiles/microbench/cand_host.cpp) on 1 and 16 threads.

    python profiles/microbench/cand_throughput.py [--fusions 100000] [--alignments 1300000] [--out profiles/cand/chunk.json]

The problem has the shape of a dosplitalign chunk of the end-to-end case (tests/e2e_case.py: 2x150 bp, fragment mean 450, sd 30):
per fusion and cluster end one genomic mate region of mate_max - mate_min + 1 bases (SplitAlignmentTask's arithmetic, 869 for
these parameters) on one of 25 chromosomes and one to three transcript regions of the same length on transcript references;
improper mate alignments of 150 bases, two thirds of them placed inside a mate region (so that they are candidates), the rest
anywhere on a chromosome.  The mates inside a fusion's regions come from six fragments per fusion, so that a read is met through
several regions and the de-duplication has work.  (tests/e2e_case.py itself writes text files at test size; this generator
makes the arrays directly.)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_problem(n_fusions, n_alignments, seed=1):
    from defuse_amd import cand
    rng = np.random.default_rng(seed)
    n_chrom, chrom_len, n_transcripts, region_len, read_len = 25, 120_000_000, 40_000, 869, 150
    rows = []
    for end in (0, 1):
        ids = (np.arange(n_fusions, dtype=np.int64) | (end << 31)).astype(np.uint32).view(np.int32)
        start = rng.integers(1, chrom_len, size=n_fusions)
        rows.append((rng.integers(0, n_chrom, size=n_fusions), rng.integers(0, 2, size=n_fusions), start, start + region_len - 1, ids))
        for k in range(3):                                     # transcript regions: 1 + two with probability one half
            take = np.ones(n_fusions, bool) if k == 0 else rng.random(n_fusions) < 0.5
            start = rng.integers(1, 3000, size=n_fusions)
            rows.append(((n_chrom + rng.integers(0, n_transcripts, size=n_fusions))[take], rng.integers(0, 2, size=n_fusions)[take], start[take],
                         (start + region_len - 1)[take], ids[take]))
    regs = np.zeros(sum(len(r[0]) for r in rows), dtype=cand.REGION_DTYPE)
    at = 0
    for ref, strand, start, end_, ids in rows:
        s = slice(at, at + len(ref))
        regs["ref"][s], regs["strand"][s], regs["start"][s], regs["end"][s], regs["id"][s] = ref, strand, start, end_, ids
        at += len(ref)
    regs = regs[rng.permutation(len(regs))]
    als = np.zeros(n_alignments, dtype=cand.ALIGNMENT_DTYPE)
    inside = rng.random(n_alignments) < 2 / 3
    pick = regs[rng.integers(0, len(regs), size=n_alignments)]
    als["ref"] = np.where(inside, pick["ref"], rng.integers(0, n_chrom, size=n_alignments))
    als["strand"] = np.where(inside, pick["strand"], rng.integers(0, 2, size=n_alignments))
    als["start"] = np.where(inside, pick["start"] + rng.integers(-100, region_len - 50, size=n_alignments), rng.integers(1, chrom_len, size=n_alignments))
    als["end"] = als["start"] + read_len - 1
    # a fusion's candidates come from a handful of fragments, met through several of its regions: the de-duplication has work
    als["fragment"] = np.where(inside, (pick["id"] & 0x7FFFFFFF).astype(np.int64) * 6 + rng.integers(0, 6, size=n_alignments),
                               rng.integers(0, n_alignments // 2, size=n_alignments))
    als["read_end"] = rng.integers(0, 2, size=n_alignments)
    return regs, als


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusions", type=int, default=100_000)
    ap.add_argument("--alignments", type=int, default=1_300_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cand", "chunk.json"))
    ap.add_argument("--host", default=os.path.join(ROOT, "profiles", "microbench", "cand_host"), help="the built cand_host.cpp, '' to skip")
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    from defuse_amd import cand, dsa
    regs, als = make_problem(a.fusions, a.alignments)
    res = dict(fusions=a.fusions, regions=len(regs), alignments=len(als), library=dsa.load_library().dsa_version().decode(), runs=[], host={})
    for rep in range(a.repeats):
        t0 = time.perf_counter()
        table = cand.Table(regs)
        t1 = time.perf_counter()
        run = dict(table_create_ms=(t1 - t0) * 1e3)
        for order, name in ((cand.ORDER_VISIT, "visit"), (cand.ORDER_FUSION, "fusion")):
            with table.session() as s:
                rc, n = s.count(als, order)
                out = np.zeros(n, dtype=cand.RECORD_DTYPE)
                t2 = time.perf_counter()
                s.enumerate_into(als, out, order)
                t3 = time.perf_counter()
                t = s.timing
                run[name] = dict(wall_ms=(t3 - t2) * 1e3, upload_ms=t.upload_ms, device_ms=t.device_ms, download_ms=t.download_ms, n_hits=t.n_hits,
                                 n_visited=t.n_visited, n_kept=t.n_kept)
                # a session that already holds every key: the search in the seen keys at full size, nothing kept
                t4 = time.perf_counter()
                again = s.enumerate(als, order)
                run[name]["second_pass_wall_ms"] = (time.perf_counter() - t4) * 1e3
                run[name]["second_pass_device_ms"] = s.timing.device_ms
                assert len(again) == 0
        table.close()
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    if a.host and os.path.exists(a.host):
        rp, ap_ = os.path.join(a.tmp, "cand_regions.bin"), os.path.join(a.tmp, "cand_alignments.bin")
        regs.tofile(rp)
        als.tofile(ap_)
        for threads in (1, 16):
            txt = subprocess.run([a.host, rp, ap_, str(threads), str(a.repeats)], capture_output=True, text=True, check=True).stdout
            res["host"][str(threads)] = txt.splitlines()
            print(txt, end="", flush=True)
        os.remove(rp)
        os.remove(ap_)
        kept = {int(l.split()[-1]) for v in res["host"].values() for l in v}
        assert kept == {res["runs"][0]["visit"]["n_kept"]}, "the host driver keeps another number of candidates"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
