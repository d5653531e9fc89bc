"""The "alignment and cluster text" section of include/defuse_cmp.h on one synthetic alignment file, and the clustermatepairs
tool on the same file on its three paths.

    python profiles/microbench/cmptext_throughput.py [--fragments 1000000] [--seed 3] [--parent-tool PATH] [--out profiles/cmptext/result.json]

The file: tests/cmp_cases.py config3_write(fragments, seed), the generator of BASELINE configs[2] at any fraction; the tool runs
with -u 300 -s 30 -p 0.95 -m 5.

What is timed.  Library: the HIP-event stages of cmpt_get_timing (the parse stages are sums over the pieces) and the wall time
of begin + add (time.perf_counter; the calls end in a synchronise), one warm-up call, then the median of --repeats; the file
goes up in one piece and, as a second row, in pieces of 64 MiB.  The printer is timed on the rows of one real run through the
library: hand-over, cmp_bin_run, cmp_problems_build, mpe_cluster_batch_device and one cmp_problems_select over all problems;
cmpt_print_rows_device and cmpt_text_fetch of those rows, one warm-up, the median of --repeats.  Tool: the wall time of
bin/clustermatepairs from start to exit and every stage it prints under DEFUSE_TIMING=1, the file in the page cache, the output
into a temporary directory, 16 host threads; the default path, DEFUSE_CMP_DEVICE_PROBLEMS=1 alone, DEFUSE_CMP_DEVICE_TEXT=1 and
(if --parent-tool names a binary built from the parent commit's tools_src/clustermatepairs.cpp and linked with this library) the
parent's default path take turns in a rotating order, one warm-up round, then the median of --repeats.  Every output is compared
with the library's text, byte for byte."""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
THREADS = 16
MFR = int(300 + 10 * 30)


def median_rows(rows):
    return {k: statistics.median(r[k] for r in rows) for k in rows[0]}


def parse(ctx, data, repeats, piece):
    rows, res = [], None
    data = memoryview(data)                                 # (a slice of it is no copy)
    for it in range(repeats + 1):
        t0 = time.perf_counter()
        ctx.begin()
        pos = 0
        while piece and len(data) - pos > piece:
            pos += ctx.add(data[pos:pos + piece], final=False)["consumed"]
        res = ctx.add(data[pos:], final=True)
        wall = time.perf_counter() - t0
        t = {k: v for k, v in ctx.timing().items() if k in ("upload_ms", "tables_ms", "lines_ms", "names_ms", "layout_ms", "n_pieces")}
        t["wall_ms"] = 1e3 * wall
        if it:
            rows.append(t)
    return median_rows(rows), res


def print_rows(ctx, repeats):
    """The stream of ctx through the library down to the rows of all problems; the printer's stages on them."""
    from defuse_amd import cmp
    from oracle import clustermatepairs_oracle as ora
    with cmp.Binner(0) as binner, cmp.Problems(0) as problems:
        ctx.hand_over(binner)
        st = cmp.Stats()
        assert binner._lib.cmp_bin_run(binner.handle, MFR, ctypes.byref(st)) == 0 and st.err_record == -1
        c = problems.build(binner, MFR, 5, 300.0)
        off = problems.fetch(["prob_off"])["prob_off"]
        v = problems.view()
        prm = cmp.MpeParams(300.0, 30.0, ora.MatePairEM(300.0, 30.0, 0.95, 5).min_prob, 5, 0)
        ncl, _, status = cmp.cluster_batch(prm, off, None, None, None, None, None, on_device=(v.x, v.y, v.u, v.to_xo, v.to_yo, v.member))
        assert not status.any()
        n_rows = problems.select(0, c.n_problems, ncl, v.member)
        rows, text = [], None
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            text = ctx.print_problems(problems)
            wall = time.perf_counter() - t0
            t = {k: v for k, v in ctx.timing().items() if k in ("lengths_ms", "write_ms", "download_ms")}
            t["wall_ms"] = 1e3 * wall
            if it:
                rows.append(t)
        counts = {"n_fragments": st.n_fragments, "n_concordant": st.n_concordant, "n_bin_pairs": st.n_keys, "n_problems": c.n_problems,
                  "n_mate_pairs": c.n_mate_pairs, "n_clusters": int(ncl.sum()), "n_rows": n_rows, "out_bytes": len(text)}
        return median_rows(rows), counts, text


PATHS = {"default": {}, "device_problems": {"DEFUSE_CMP_DEVICE_PROBLEMS": "1"}, "device_text": {"DEFUSE_CMP_DEVICE_TEXT": "1"}}


def run_tool(tool, path, outp, switches):
    if os.path.exists(outp):
        os.unlink(outp)
    env = dict(os.environ, DEFUSE_THREADS=str(THREADS), DEFUSE_TIMING="1")
    for k in ("DEFUSE_CMP_DEVICE_PROBLEMS", "DEFUSE_CMP_DEVICE_TEXT"):
        env.pop(k, None)
    env.update(switches)
    t0 = time.perf_counter()
    r = subprocess.run([tool, "-a", path, "-c", outp, "-u", "300", "-s", "30", "-p", "0.95", "-m", "5"], capture_output=True, text=True, env=env, timeout=900)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s failed: %s" % (tool, r.stderr[-400:]))
    return wall, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tool", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmptext", "result.json"))
    args = ap.parse_args()
    from defuse_amd import cmptext, dsa
    from tests import cmp_cases
    tool = os.path.join(ROOT, "bin", "clustermatepairs")
    result = {"library": dsa.lib().dsa_version().decode(), "seed": args.seed, "fragments": args.fragments, "host_threads": THREADS, "repeats": args.repeats}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "spanning.txt")
        t0 = time.perf_counter()
        n_frag, n_loci, n_lines = cmp_cases.config3_write(args.fragments, path, args.seed)
        data = open(path, "rb").read()
        result.update(n_lines=n_lines, in_bytes=len(data), n_loci=n_loci)
        print("file: %d fragments, %d lines, %d bytes, made in %.1f s" % (n_frag, n_lines, len(data), time.perf_counter() - t0), flush=True)

        with cmptext.CmptContext(max_names=1 << 20) as ctx:
            cut, res2 = parse(ctx, data, args.repeats, 64 << 20)
            one, res = parse(ctx, data, args.repeats, None)
            assert {k: v for k, v in res.items() if k != "consumed"} == {k: v for k, v in res2.items() if k != "consumed"} and res["stop_line"] == 0
            result["parse_result"] = res
            result["parse_one_piece"], result["parse_pieces_64MiB"] = one, cut
            result["upload_GBps"] = len(data) / one["upload_ms"] / 1e6
            text_ms = one["tables_ms"] + one["lines_ms"] + one["names_ms"] + one["layout_ms"]
            result["parse_without_upload_GBps"] = len(data) / text_ms / 1e6
            print(json.dumps({"parse_one_piece": one, "parse_result": res}), flush=True)
            pr, counts, text = print_rows(ctx, args.repeats)
            result["print"], result["counts"] = pr, counts
            result["write_GBps"] = len(text) / pr["write_ms"] / 1e6 if pr["write_ms"] else None
            print(json.dumps({"print": pr, "counts": counts}), flush=True)

        # the tool: (name, binary, switches) in an order that rotates, so that none always follows the same other
        configs = [(name, tool, sw) for name, sw in PATHS.items()]
        if args.parent_tool:
            configs.append(("parent_default", args.parent_tool, {}))
        rows = {name: [] for name, _, _ in configs}
        last_err = {}
        for it in range(args.repeats + 1):
            for name, binary, switches in configs[it % len(configs):] + configs[:it % len(configs)]:
                outp = os.path.join(tmp, name + ".clusters")
                wall, err = run_tool(binary, path, outp, switches)
                assert open(outp, "rb").read() == text, name
                row = {"wall": wall}
                for stage, secs in re.findall(r"^\[clustermatepairs\] +([a-z+ ]+?) ([0-9.e+-]+) s$", err, re.M):
                    row[stage] = float(secs)
                if it:
                    rows[name].append(row)
                last_err[name] = err.splitlines()
        for name in rows:
            keys = [k for k in rows[name][0] if all(k in r for r in rows[name])]
            result["tool_" + name + "_s"] = {k: {"median": statistics.median(r[k] for r in rows[name]), "min": min(r[k] for r in rows[name]),
                                                 "max": max(r[k] for r in rows[name])} for k in keys}
            result["tool_" + name + "_stderr"] = last_err[name]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
