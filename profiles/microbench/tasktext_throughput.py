"""What the text front of the task store costs against the host work it replaces: the exon table and the regions file parsed,
resolved and made into a task store.

    g++ -std=c++17 -O2 -o profiles/microbench/tasktext_host profiles/microbench/tasktext_host.cpp
    python profiles/microbench/tasktext_throughput.py [--fusions 100000] [--repeats 15] [--out-dir profiles/tasktext]

The problem is the generated one of profiles/microbench/task_throughput.py (make_world, seed 1).  Timed warm, after --warmup
rounds, as medians of --repeats with min-max:

  (a) the host path: profiles/microbench/tasktext_host.cpp — the tool's own ExonRegions::Read and ReadAlignRegionPairs, the
      three name maps, every end resolved, everything packed (its own clock, --repeats rounds in one process; the readers have no
      threads, so there is one thread count) — followed, in this process, by task_exons_create and task_store_create;
  (b) taskt_parse_exons + taskt_parse_regions + taskt_store_create by a host clock around each call (they return
      synchronised), with the stages of taskt_get_timing and task_store_get_timing.

Before anything is timed the pairs of (a) and (b) are compared and must be identical, and so must the two stores' records and
regions.  Writes result.json and README.md into --out-dir."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# The record of one compile, to be renewed by hand when the kernels change:
# -Rpass-analysis=kernel-resource-usage on taskt_api.hip (hipcc --offload-arch=gfx950 -O3): kernel, VGPRs, SGPRs, scratch bytes per lane, waves per SIMD,
# LDS bytes per workgroup
RESOURCES = [("k_exon_lines", 27, 74, 0, 8, 16), ("k_exon_total", 4, 18, 0, 8, 0), ("k_exon_rows", 38, 72, 0, 8, 0),
             ("k_exon_emit", 24, 44, 0, 8, 0), ("k_iota", 4, 12, 0, 8, 0), ("k_name_keys", 22, 18, 0, 8, 0), ("k_name_heads", 14, 22, 0, 8, 0),
             ("k_tx_dups", 4, 18, 0, 8, 0), ("k_chrom_first", 4, 12, 0, 8, 0), ("k_chrom_groups", 21, 34, 0, 8, 0), ("k_row_chrom", 7, 14, 0, 8, 0),
             ("k_tx_out", 34, 42, 0, 8, 0), ("k_region_lines", 40, 78, 0, 8, 16), ("k_id_heads", 6, 12, 0, 8, 0), ("k_pairs_fill", 12, 32, 0, 8, 0),
             ("k_pairs_win", 34, 58, 0, 8, 0), ("k_pair_check", 8, 24, 0, 8, 0), ("k_stop_result<true>", 8, 46, 0, 8, 0),
             ("k_stop_result<false>", 5, 38, 0, 8, 0)]


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusions", type=int, default=100_000)
    ap.add_argument("--transcripts", type=int, default=40_000)
    ap.add_argument("--chrom-mb", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", default=os.path.join(ROOT, "profiles", "microbench", "tasktext_host"))
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "tasktext"))
    a = ap.parse_args()
    from task_throughput import PARAMS, make_world
    from defuse_amd import cand, dsa, task, tasktext
    tmp = os.path.join(a.tmp, "tasktext_throughput.%d" % os.getpid())
    os.makedirs(tmp, exist_ok=True)
    W = make_world(1, a.chrom_mb, a.transcripts, a.fusions, tmp)
    exon_text = np.fromfile(os.path.join(tmp, "exons.txt"), dtype=np.uint8)
    region_text = np.fromfile(os.path.join(tmp, "regions.txt"), dtype=np.uint8)
    names_path = os.path.join(tmp, "names.txt")
    with open(names_path, "w") as f:
        f.write("".join(n + "\n" for n in W["names"]))
    print("problem: %d transcripts, %d exons, %.1f MB of exon text; %d fusions, %.1f MB of regions text" %
          (a.transcripts, len(W["exons"]), exon_text.size / 1e6, a.fusions, region_text.size / 1e6), flush=True)
    lib = tasktext.lib()
    prm = (int(PARAMS[0] - 3 * PARAMS[1]), int(PARAMS[0] + 3 * PARAMS[1]), PARAMS[2], PARAMS[3])
    cprm = task.Params(*prm)
    ptr = lambda x: x.ctypes.data
    ref = ctypes.c_void_p()
    assert lib.task_reference_create(0, ptr(W["data"]), W["data"].size, ptr(W["seqs"]), len(W["seqs"]), ctypes.byref(ref)) == 0, lib.task_last_error()

    class Ref:
        handle = ref

    def fetch(store):
        c = task.Counts()
        assert lib.task_store_counts(store, ctypes.byref(c)) == 0
        rec, reg = np.zeros(c.n_tasks, dtype=task.RECORD_DTYPE), np.zeros(c.n_regions, dtype=cand.REGION_DTYPE)
        assert lib.task_store_fetch(store, ptr(rec), len(rec), None, 0, None, 0, ptr(reg), len(reg)) == 0, lib.task_last_error()
        return rec, reg

    host_args = [a.host, os.path.join(tmp, "exons.txt"), os.path.join(tmp, "regions.txt"), names_path]
    with tasktext.Context() as ctx, tasktext.Names(W["names"]) as names:
        # both paths give the same pairs and the same store, before anything is timed
        er, rr = ctx.parse_exons(names, exon_text), ctx.parse_regions(names, region_text)
        assert er["stop_line"] == 0 and rr["stop_line"] == 0 and er["n_items"] == a.transcripts and rr["n_items"] == a.fusions
        mine, _ = ctx.pairs()
        tx, exons, chrom_ref, _ = ctx.exons()
        subprocess.run(host_args + ["1", os.path.join(tmp, "pairs.bin")], check=True, capture_output=True)
        theirs = np.fromfile(os.path.join(tmp, "pairs.bin"), dtype=task.PAIR_DTYPE)
        assert mine.tobytes() == theirs.tobytes(), "the pairs of the two paths differ"
        with ctx.store(Ref, prm) as st:
            rec_b, reg_b = fetch(st.handle)
        ex = ctypes.c_void_p()
        assert lib.task_exons_create(0, ptr(chrom_ref), len(chrom_ref), ptr(tx), len(tx), ptr(exons), len(exons), ctypes.byref(ex)) == 0, lib.task_last_error()
        s = ctypes.c_void_p()
        assert lib.task_store_create(ref, ex, ctypes.byref(cprm), ptr(theirs), len(theirs), ctypes.byref(s)) == 0, lib.task_last_error()
        rec_a, reg_a = fetch(s)
        lib.task_store_destroy(s)
        lib.task_exons_destroy(ex)
        assert rec_a.tobytes() == rec_b.tobytes() and reg_a.tobytes() == reg_b.tobytes(), "the stores of the two paths differ"
        print("identical: %d pairs, %d mate regions" % (len(mine), len(reg_a)), flush=True)

        out = subprocess.run(host_args + [str(a.warmup + a.repeats)], check=True, capture_output=True, text=True).stdout.splitlines()[a.warmup:]
        host = [{f[k]: float(f[k + 1]) for k in range(0, 8, 2)} for f in (l.split() for l in out)]
        a_ex, a_st, b_ex, b_rg, b_st = [], [], [], [], []
        stages = {k: [] for k in ("exon_upload_ms", "exon_device_ms", "exon_table_ms", "region_upload_ms", "region_device_ms", "check_ms")}
        store_stages = {k: [] for k in ("upload_ms", "plan_ms", "count_ms", "scan_ms", "region_ms", "gather_ms", "sort_ms")}
        for rep in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            assert lib.task_exons_create(0, ptr(chrom_ref), len(chrom_ref), ptr(tx), len(tx), ptr(exons), len(exons), ctypes.byref(ex)) == 0
            t1 = time.perf_counter()
            assert lib.task_store_create(ref, ex, ctypes.byref(cprm), ptr(theirs), len(theirs), ctypes.byref(s)) == 0
            t2 = time.perf_counter()
            lib.task_store_destroy(s)
            lib.task_exons_destroy(ex)
            t3 = time.perf_counter()
            ctx.parse_exons(names, exon_text)
            t4 = time.perf_counter()
            ctx.parse_regions(names, region_text)
            t5 = time.perf_counter()
            st = ctx.store(Ref, prm)
            t6 = time.perf_counter()
            tm, stm = ctx.timing(), st.timing()
            st.close()
            if rep >= a.warmup:
                a_ex.append((t1 - t0) * 1e3)
                a_st.append((t2 - t1) * 1e3)
                b_ex.append((t4 - t3) * 1e3)
                b_rg.append((t5 - t4) * 1e3)
                b_st.append((t6 - t5) * 1e3)
                for k in stages:
                    stages[k].append(tm[k])
                for k in store_stages:
                    store_stages[k].append(stm[k])
    lib.task_reference_destroy(ref)
    hs = {k: stats([h[k] for h in host]) for k in host[0]}
    total_a = [h["total_ms"] + x + y for h, x, y in zip(host, a_ex, a_st)]
    total_b = [x + y + z for x, y, z in zip(b_ex, b_rg, b_st)]
    res = dict(fusions=a.fusions, transcripts=a.transcripts, exons=len(W["exons"]), exon_text_bytes=int(exon_text.size), region_text_bytes=int(region_text.size),
               library=dsa.load_library().dsa_version().decode(), a_host=hs, a_task_exons_create_ms=stats(a_ex), a_task_store_create_ms=stats(a_st),
               a_total_ms=stats(total_a), b_taskt_parse_exons_ms=stats(b_ex), b_taskt_parse_regions_ms=stats(b_rg), b_taskt_store_create_ms=stats(b_st),
               b_total_ms=stats(total_b), b_stages={k: stats(v) for k, v in stages.items()}, b_store_stages={k: stats(v) for k, v in store_stages.items()},
               resources=[dict(kernel=k, vgprs=v, sgprs=sg, scratch_bytes_per_lane=sc, waves_per_simd=o, lds_bytes=l) for k, v, sg, sc, o, l in RESOURCES])
    res["b_below_a"] = res["b_total_ms"]["median"] < res["a_total_ms"]["median"]
    print(json.dumps(res), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    fmt = lambda s: "%.3f ms (%.3f - %.3f, n = %d)" % (s["median"], s["min"], s["max"], s["n"])
    label = dict(exon_upload_ms="exon text to the device", exon_device_ms="exon kernels: tables, line rules, emit, two name sorts, lookups",
                 exon_table_ms="arrays down and `task_exons_create` (host clock)", region_upload_ms="regions text to the device",
                 region_device_ms="regions kernels: tables, line rules, sort, pairs", check_ms="the pairs' checks on the device")
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("""# The text front of the task store: exon table and regions file parsed on the device (`include/defuse_task.h`)

Written by `profiles/microbench/tasktext_throughput.py` on one MI355X (numbers: `result.json`, library `%s`).

Problem: the generated one of `profiles/task` (seed 1): %d transcripts with %d exons (%.1f MB of exon text), %d align region
pairs (%.1f MB of regions text).  %d warm-up rounds, medians with min - max.  (a) is `profiles/microbench/tasktext_host.cpp`, the
tool's own `ExonRegions::Read` and `ReadAlignRegionPairs`, three hash maps, every end resolved, everything packed, by its own
clock in one process with the files in the page cache; these readers have no threads, so there is one thread count.  (b) is a
host clock around calls that return synchronised; its two texts were read into memory before the clock started, while (a) opens
and reads both files (some 11 MB from the page cache) inside its timed region.  The pairs of the two paths and the records and
regions of the two stores were compared first and are identical.

| | |
|---|---|
| (a) host: read the exon table | %s |
| (a) host: read the regions file | %s |
| (a) host: maps, resolve, pack | %s |
| (a) `task_exons_create` | %s |
| (a) `task_store_create` | %s |
| **(a) in all** | **%s** |
| (b) `taskt_parse_exons` | %s |
| (b) `taskt_parse_regions` | %s |
| (b) `taskt_store_create` | %s |
| **(b) in all** | **%s** |
%s

(b) is %s (a).  The link is kept for what it removes from the caller: the line splitter, the `lexical_cast` rules, the two readers,
`ParseTranscriptID` and the three name maps.

## Kernel resources

`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `defuse_amd/csrc/taskt_api.hip`:

| kernel | VGPRs | SGPRs | scratch bytes per lane | waves per SIMD | LDS bytes per workgroup |
|---|---|---|---|---|---|
%s

No kernel uses scratch; all reach the full occupancy of 8 waves per SIMD.  The table is the record of one compile, kept as a literal
in the script (`RESOURCES`): it does not follow later changes of the kernels by itself.

## What has not been measured

The share of the radix passes in the exon kernels (one pass per 8 name bytes and one by length, twice); a sort that stops at
the first chunk in which all names differ; pinned host memory for the two texts; real annotation, whose names are longer than
this generator's 7 bytes and so take more passes.
""" % (res["library"], a.transcripts, len(W["exons"]), exon_text.size / 1e6, a.fusions, region_text.size / 1e6, a.warmup, fmt(hs["exons_ms"]), fmt(hs["regions_ms"]),
       fmt(hs["pack_ms"]), fmt(res["a_task_exons_create_ms"]), fmt(res["a_task_store_create_ms"]), fmt(res["a_total_ms"]), fmt(res["b_taskt_parse_exons_ms"]),
       fmt(res["b_taskt_parse_regions_ms"]), fmt(res["b_taskt_store_create_ms"]), fmt(res["b_total_ms"]),
       "\n".join("| of which %s | %s |" % (label[k], fmt(res["b_stages"][k])) for k in stages),
       "below" if res["b_below_a"] else "NOT below", "\n".join("| `%s` | %d | %d | %d | %d | %d |" % r for r in RESOURCES)))
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
