"""The "cluster text" section of include/defuse_sc.h on one synthetic cluster file, and the setcover tool on the same file with
and without DEFUSE_SC_DEVICE_TEXT=1.

    python profiles/microbench/sctext_throughput.py [--clusters 800000] [--seed 1] [--parent-tool PATH] [--out profiles/sctext/result.json]

The file: random_clusters(seed, n_clusters, n_frag = 3 * n_clusters, big = 4) of tests/test_setcover.py in the line format of
its write_cluster_file (the strand column drawn as one array), minimum cluster size 3.  800 000 clusters are about 10 M lines.

What is timed.  Library: the HIP-event stages of sct_get_timing (upload and tables are sums over the pieces; download is
sct_fetch of the whole output) and the wall time of begin + add + cover (time.perf_counter, the calls end in a synchronise),
one warm-up call, then the median of --repeats; the file goes up in one piece and, as a second row, in pieces of 64 MiB.  Tool:
the wall time of bin/setcover from start to exit and the "read", "set cover" and "write" stages it prints under DEFUSE_TIMING=1,
the file in the page cache, the output into a temporary directory, 16 host threads; the default path, the device-text path and
(if --parent-tool names a binary built from the parent commit's tools_src/setcover.cpp) the parent's tool take turns in a
rotating order, one warm-up round, then the median of --repeats.  Every output is compared with the library's."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
THREADS = 16


def make_file(path, n_clusters, seed):
    from tests.test_setcover import random_clusters
    clusters = random_clusters(seed, n_clusters=n_clusters, n_frag=3 * n_clusters, big=4)
    n_members = sum(len(c) for c in clusters)
    strand = np.random.default_rng(seed).integers(0, 2, size=2 * n_members).tolist()
    k = 0
    with open(path, "w") as f:
        for cid, frs in enumerate(clusters):
            rows = []
            for e in (0, 1):
                for fr in frs:
                    rows.append("%d\t%d\t%d\t%d\tchr%d\t%s\t%d\t%d\n" % (cid, e, fr, strand[k], 1 + cid % 3, "+-"[e], 1000 + fr, 1050 + fr))
                    k += 1
            f.write("".join(rows))
    return 2 * n_members


def median_rows(rows):
    return {k: statistics.median(r[k] for r in rows) for k in rows[0]}


def library(data, m, repeats, piece):
    from defuse_amd import sctext
    rows, res, out = [], None, None
    data = memoryview(data)                                 # (a slice of it is no copy)
    with sctext.SctContext() as ctx:
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            ctx.begin()
            if piece:
                pos = 0
                while len(data) - pos > piece:
                    pos += ctx.add(data[pos:pos + piece], final=False)
                ctx.add(data[pos:], final=True)
            else:
                ctx.add(data, final=True)
            res = ctx.cover(m)
            wall = time.perf_counter() - t0
            out = ctx.fetch()
            t = ctx.timing()
            t["wall_ms"] = 1e3 * wall
            if it:
                rows.append(t)
    return median_rows(rows), res, out


def run_tool(tool, path, outp, m, device_text, timing=False):
    if os.path.exists(outp):
        os.unlink(outp)
    env = dict(os.environ, DEFUSE_THREADS=str(THREADS))
    env.pop("DEFUSE_SC_DEVICE_TEXT", None)
    env.pop("DEFUSE_TIMING", None)
    if device_text:
        env["DEFUSE_SC_DEVICE_TEXT"] = "1"
    if timing:
        env["DEFUSE_TIMING"] = "1"
    t0 = time.perf_counter()
    r = subprocess.run([tool, "-c", path, "-m", str(m), "-o", outp], capture_output=True, text=True, env=env, timeout=600)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s failed: %s" % (tool, r.stderr[-400:]))
    return wall, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=800_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--min-size", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tool", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sctext", "result.json"))
    args = ap.parse_args()
    from defuse_amd import dsa
    tool = os.path.join(ROOT, "bin", "setcover")
    result = {"library": dsa.lib().dsa_version().decode(), "seed": args.seed, "clusters": args.clusters,
              "min_cluster_size": args.min_size, "host_threads": THREADS, "repeats": args.repeats}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clusters.txt")
        t0 = time.perf_counter()
        result["n_lines"] = make_file(path, args.clusters, args.seed)
        data = open(path, "rb").read()
        result["in_bytes"] = len(data)
        print("file: %d lines, %d bytes, made in %.1f s" % (result["n_lines"], len(data), time.perf_counter() - t0), flush=True)

        one, res, out = library(data, args.min_size, args.repeats, None)
        cut, res2, out2 = library(data, args.min_size, args.repeats, 64 << 20)
        assert res2 == res and out2 == out
        result["result"] = res
        result["one_piece"], result["pieces_64MiB"] = one, cut
        result["gather_GBps"] = one["gather_bytes"] / one["gather_ms"] / 1e6 if one["gather_ms"] else None
        result["upload_GBps"] = len(data) / one["upload_ms"] / 1e6
        print(json.dumps({"one_piece": one, "result": res}), flush=True)

        # the tool: (name, binary, DEFUSE_SC_DEVICE_TEXT) in an order that rotates, so that none always follows the same other
        configs = [("tool_default", tool, False), ("tool_device_text", tool, True)]
        if args.parent_tool:
            configs.append(("parent_tool", args.parent_tool, False))
        rows = {name: [] for name, _, _ in configs}
        last_err = {}
        for it in range(args.repeats + 1):
            for name, binary, device_text in configs[it % len(configs):] + configs[:it % len(configs)]:
                outp = os.path.join(tmp, name + ".sc")
                wall, err = run_tool(binary, path, outp, args.min_size, device_text, timing=True)
                assert open(outp, "rb").read() == out, name
                row = {"wall": wall}
                for stage in ("read", "set cover", "write"):
                    row[stage] = float(re.search(r"^\[setcover\] %s ([0-9.e+-]+) s$" % stage, err, re.M).group(1))
                if it:
                    rows[name].append(row)
                last_err[name] = err.splitlines()
        for name in rows:
            result[name + "_s"] = {k: {"median": statistics.median(r[k] for r in rows[name]), "min": min(r[k] for r in rows[name]),
                                       "max": max(r[k] for r in rows[name])} for k in rows[name][0]}
            result[name + "_stderr"] = last_err[name]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
