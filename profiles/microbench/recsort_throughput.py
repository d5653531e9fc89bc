"""`defuse_glue sort_alignments` against GNU sort on alignment chunk files (profiles/recsort/README.md).

    python profiles/microbench/recsort_throughput.py --json result.json

Writes --chunks files of alignment lines (--bytes in all; records drawn like a 20 M fragment run's: 100 k fusions, nine "%d\\t"
fields of about 40 bytes a line, printed by the record store itself), warms the page cache, and times, --runs times each and
alternating:
  (a) `LC_ALL=C sort -n -k 1` per chunk, then `sort -m -n -k 1` over the sorted chunks: the chain's sort stage;
  (b) one `defuse_glue sort_alignments -o OUT chunks...` with DEFUSE_TIMING=1.
The two files must be equal.  Then single files of --small lines, to find the size below which the HIP runtime's start makes
the tool the slower of the two.  If the directory's file system has no room for four copies of --bytes, the size is reduced
and the result says so."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GLUE = os.path.join(ROOT, "bin", "defuse_glue")
C_ENV = dict(os.environ, LC_ALL="C")


def draw(rng, n, n_fusions=100_000, n_fragments=20_000_000):
    from defuse_amd.dsa import RECORD_DTYPE
    r = np.zeros(n, RECORD_DTYPE)
    r["fusion_id"] = rng.integers(0, n_fusions, n)
    r["frag"] = rng.integers(0, n_fragments, n)
    r["read_end"] = rng.integers(0, 2, n)
    r["revcomp"] = rng.integers(0, 2, n)
    r["ref_first"] = rng.integers(1, 2000, n)
    r["ref_second"] = rng.integers(-1, 2000, n)
    r["read_first"] = rng.integers(0, 101, n)
    r["read_second"] = 100 - r["read_first"]
    r["score"] = rng.integers(8, 101, n)
    return r


def write_lines(store, path, rng, n):
    """n unsorted alignment lines, printed by the store (rec_text of the records in the order they were appended)."""
    store.clear()
    store.append(draw(rng, n))
    text = store.text()
    open(path, "wb").write(text)
    return len(text)


def gnu_chain(chunks, out):
    t0 = time.time()
    for c in chunks:
        subprocess.check_call("LC_ALL=C sort -n -k 1 %s > %s.sorted" % (c, c), shell=True)
    t1 = time.time()
    subprocess.check_call("LC_ALL=C sort -m -n -k 1 %s > %s" % (" ".join(c + ".sorted" for c in chunks), out), shell=True)
    return {"wall_s": round(time.time() - t0, 3), "per_chunk_sorts_s": round(t1 - t0, 3), "merge_s": round(time.time() - t1, 3)}


def tool(chunks, out):
    t0 = time.time()
    r = subprocess.run([GLUE, "sort_alignments", "-o", out] + chunks, capture_output=True, text=True, env=dict(os.environ, DEFUSE_TIMING="1"))
    wall = time.time() - t0
    if r.returncode != 0:
        raise SystemExit("sort_alignments: status %d: %s" % (r.returncode, r.stderr[-500:]))
    return {"wall_s": round(wall, 3), "timing": [l for l in r.stderr.splitlines() if l.startswith("[sort_alignments]")]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="/tmp/recsort")
    ap.add_argument("--bytes", type=float, default=2.1e9)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", type=int, nargs="*", default=[1_000, 10_000, 100_000, 300_000, 1_000_000, 3_000_000])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from defuse_amd import rec
    os.makedirs(args.out, exist_ok=True)
    P = lambda n: os.path.join(args.out, n)
    free = shutil.disk_usage(args.out).free
    want = args.bytes
    if 4.5 * want > free:
        want = free / 4.5
    res = {"what": "GNU sort per chunk + sort -m against one defuse_glue sort_alignments, wall seconds, warm page cache", "bytes_asked": int(args.bytes),
           "reduced_to_fit_the_disk": want < args.bytes, "host_cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "sort_version": subprocess.run(["sort", "--version"], capture_output=True, text=True).stdout.splitlines()[0]}
    rng = np.random.default_rng(7)
    per_chunk = int(want / args.chunks / 40.1)
    chunks, total = [], 0
    with rec.Store(0) as store:
        for c in range(args.chunks):
            chunks.append(P("split.%d" % c))
            total += write_lines(store, chunks[-1], rng, per_chunk)
        small = []
        for n in args.small:
            small.append((n, P("small.%d" % n), write_lines(store, P("small.%d" % n), rng, n)))
    res.update(chunks=args.chunks, lines=per_chunk * args.chunks, bytes=total)
    print("generated %d bytes in %d chunks" % (total, args.chunks), flush=True)
    for c in chunks:                                                    # the page cache holds the inputs before anything is timed
        open(c, "rb").read()
    res["gnu"], res["tool"] = [], []
    for k in range(args.runs):
        res["gnu"].append(gnu_chain(chunks, P("gnu.alignments")))
        print("gnu", res["gnu"][-1], flush=True)
        res["tool"].append(tool(chunks, P("gpu.alignments")))
        print("tool", res["tool"][-1], flush=True)
        if subprocess.call(["cmp", "-s", P("gnu.alignments"), P("gpu.alignments")]) != 0:
            raise SystemExit("the two sorted files differ")
    res["same_file"] = True
    res["gnu_median_s"] = float(np.median([r["wall_s"] for r in res["gnu"]]))
    res["tool_median_s"] = float(np.median([r["wall_s"] for r in res["tool"]]))
    res["small_files"] = []
    for n, path, size in small:
        open(path, "rb").read()
        g, t = [], []
        for k in range(args.runs):
            t0 = time.time()
            subprocess.check_call(["sort", "-n", "-k", "1", "-o", path + ".gnu", path], env=C_ENV)
            g.append(time.time() - t0)
            t.append(tool([path], path + ".gpu")["wall_s"])
            if subprocess.call(["cmp", "-s", path + ".gnu", path + ".gpu"]) != 0:
                raise SystemExit("the two sorted files differ at %d lines" % n)
        res["small_files"].append({"lines": n, "bytes": size, "gnu_sort_s": round(float(np.median(g)), 4), "sort_alignments_s": round(float(np.median(t)), 4)})
        print(res["small_files"][-1], flush=True)
    shutil.rmtree(args.out)
    text = json.dumps(res, indent=1)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
