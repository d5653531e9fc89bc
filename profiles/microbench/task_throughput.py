"""What the first link of the resident chain costs against the host work it replaces: the tasks of a run (windows, remainders,
mate regions) from the regions, the reference and the exon table.

    g++ -std=c++17 -O2 -pthread -o profiles/microbench/task_host profiles/microbench/task_host.cpp defuse_amd/libdefuse_dsa.so \
        '-Wl,-rpath,$ORIGIN/../../defuse_amd'
    python profiles/microbench/task_throughput.py [--fusions 100000] [--repeats 15] [--out-dir profiles/task]

The problem is generated from a seed: 24 chromosomes of --chrom-mb MB and --transcripts transcripts of 1-12 exons with their
"gene|transcript" sequences, as one FASTA with its .fai; --fusions align region pairs of 50-400 bases, 60 % of the ends on a
transcript reference; fragment and read lengths (300, 30, 50, 50).  Timed after --warmup rounds as medians of --repeats with
min-max, the paths alternating round by round:

  (a) the host path: profiles/microbench/task_host.cpp, the tool's own CreateTasks on 1 and on 16 threads, the packing of its
      result, bat_windows_create and pred_tasks_create.  One process per round and thread count (its device is up before its
      clock starts); host clock;
  (b) the device path in this process: task_store_create by a host clock around the call, which returns synchronised, its
      stages by HIP events (task_timing), and task_store_fetch of the records and regions (no pool bytes).  The one-time
      task_reference_create / task_exons_create are timed on their own.

Before anything is timed the tasks of (a) and (b) are compared and must be identical: every field, both byte pools, every
region.  Writes result.json and README.md into --out-dir."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PARAMS = (300.0, 30.0, 50, 50)
LINE = 60

# -Rpass-analysis=kernel-resource-usage on task_api.hip (hipcc --offload-arch=gfx950 -O3): kernel, VGPRs, SGPRs, scratch bytes per lane, waves per SIMD
RESOURCES = [("k_task_plan", 31, 34, 0, 8), ("k_task_regions<false> (count)", 25, 56, 0, 8), ("k_task_regions<true> (emit)", 30, 67, 0, 8),
             ("k_task_records", 56, 26, 0, 8), ("k_task_stores", 34, 19, 0, 8), ("k_bat_gather<64, true, Seg> (windows)", 30, 36, 0, 8),
             ("k_bat_gather<16, true, Seg64> (remainders)", 30, 34, 0, 8)]


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def make_world(seed, chrom_mb, n_tx, n_fusions, tmp):
    """Writes ref.fa(.fai), exons.txt, regions.txt under tmp; returns what the device path takes."""
    from defuse_amd import task
    rng = np.random.default_rng(seed)
    n_chrom, chrom_len = 24, int(chrom_mb * 1e6)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    # the exon table: transcript k is "T%06d" (ascending names are ascending indices), gene k // 2
    n_ex = rng.integers(1, 13, size=n_tx)
    first = np.concatenate(([0], np.cumsum(n_ex)))[:-1]
    total = int(n_ex.sum())
    ex_len = rng.integers(50, 401, size=total)
    gap = rng.integers(100, 5001, size=total)
    step = ex_len + gap
    run = np.cumsum(step) - step
    rel = run - np.repeat(run[first], n_ex)                                # offset of each exon's start from its transcript's first
    span = np.add.reduceat(step, first)
    t_chrom = rng.integers(0, n_chrom, size=n_tx)
    t_start = rng.integers(1, chrom_len - span.max() - 1, size=n_tx)
    ex_start = (np.repeat(t_start, n_ex) + rel).astype(np.int32)
    ex_end = (ex_start + ex_len - 1).astype(np.int32)
    t_len = np.add.reduceat(ex_len, first)
    t_strand = rng.integers(0, 2, size=n_tx)
    # the sequences
    seq_len = np.concatenate((np.full(n_chrom, chrom_len, dtype=np.int64), t_len.astype(np.int64)))
    seq_off = np.concatenate(([0], np.cumsum(seq_len)))[:-1]
    data = acgt[rng.integers(0, 4, size=int(seq_len.sum()), dtype=np.uint8)]
    names = ["chr%d" % (c + 1) for c in range(n_chrom)] + ["G%05d|T%06d" % (k // 2, k) for k in range(n_tx)]
    fa = os.path.join(tmp, "ref.fa")
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fai:
        pos = 0
        for k, name in enumerate(names):
            head = b">" + name.encode() + b"\n"
            f.write(head)
            pos += len(head)
            n = int(seq_len[k])
            s = data[seq_off[k]:seq_off[k] + n]
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, n, pos, LINE, LINE + 1))
            full = n // LINE
            body = np.full((full, LINE + 1), 10, dtype=np.uint8)
            body[:, :LINE] = s[:full * LINE].reshape(full, LINE)
            out = body.tobytes() + (s[full * LINE:].tobytes() + b"\n" if n % LINE else b"")
            f.write(out)
            pos += len(out)
    with open(os.path.join(tmp, "exons.txt"), "w") as f:
        es, ee = ex_start.tolist(), ex_end.tolist()
        for k in range(n_tx):
            a, b = int(first[k]), int(first[k] + n_ex[k])
            f.write("G%05d\tT%06d\tchr%d\t%s\t%s\n" % (k // 2, k, t_chrom[k] + 1, "+-"[t_strand[k]], "\t".join("%d\t%d" % p for p in zip(es[a:b], ee[a:b]))))
    # the align region pairs, ascending fusion ids with gaps
    pairs = np.zeros(n_fusions, dtype=task.PAIR_DTYPE)
    pairs["fusion_id"] = np.cumsum(rng.integers(1, 4, size=n_fusions))
    on_tx = rng.random((n_fusions, 2)) < 0.6
    tx = rng.integers(0, n_tx, size=(n_fusions, 2))
    ch = rng.integers(0, n_chrom, size=(n_fusions, 2))
    seq = np.where(on_tx, n_chrom + tx, ch)
    length = rng.integers(50, 401, size=(n_fusions, 2))
    start = (rng.random((n_fusions, 2)) * np.maximum(seq_len[seq] - length, 1)).astype(np.int64) + 1
    pairs["end"]["seq"] = seq
    pairs["end"]["transcript"] = np.where(on_tx, tx, -1)
    pairs["end"]["chrom"] = np.where(on_tx, -1, ch)
    pairs["end"]["strand"] = rng.integers(0, 2, size=(n_fusions, 2))
    pairs["end"]["start"] = start
    pairs["end"]["end"] = start + length - 1
    with open(os.path.join(tmp, "regions.txt"), "w") as f:
        fid, e = pairs["fusion_id"].tolist(), pairs["end"]
        sq, st, s0, s1 = e["seq"].tolist(), e["strand"].tolist(), e["start"].tolist(), e["end"].tolist()
        for k in range(n_fusions):
            for ce in (0, 1):
                f.write("%d\t%d\t%s\t%s\t%d\t%d\n" % (fid[k], ce, names[sq[k][ce]], "+-"[st[k][ce]], s0[k][ce], s1[k][ce]))
    seqs = np.zeros(len(names), dtype=task.SEQ_DTYPE)
    seqs["off"], seqs["len"] = seq_off, seq_len
    txs = np.zeros(n_tx, dtype=task.TRANSCRIPT_DTYPE)
    txs["chrom"], txs["strand"], txs["first_exon"], txs["n_exons"], txs["name_ref"] = t_chrom, t_strand, first, n_ex, n_chrom + np.arange(n_tx)
    exons = np.zeros(total, dtype=task.EXON_DTYPE)
    exons["start"], exons["end"] = ex_start, ex_end
    return dict(data=data, seqs=seqs, chrom_ref=np.arange(n_chrom, dtype=np.int32), tx=txs, exons=exons, pairs=pairs, names=names, fasta=fa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusions", type=int, default=100_000)
    ap.add_argument("--transcripts", type=int, default=40_000)
    ap.add_argument("--chrom-mb", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", default=os.path.join(ROOT, "profiles", "microbench", "task_host"))
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "task"))
    a = ap.parse_args()
    import ctypes
    from defuse_amd import cand, dsa, task
    tmp = os.path.join(a.tmp, "task_throughput.%d" % os.getpid())
    os.makedirs(tmp, exist_ok=True)
    t0 = time.perf_counter()
    W = make_world(1, a.chrom_mb, a.transcripts, a.fusions, tmp)
    print("problem: %.0f MB of reference, %d sequences, %d exons, %d fusions (%.1f s)" % (W["data"].size / 1e6, len(W["seqs"]), len(W["exons"]), a.fusions,
                                                                                          time.perf_counter() - t0), flush=True)
    lib = task.lib()
    err = lambda: lib.task_last_error().decode()
    prm = task.Params(int(PARAMS[0] - 3 * PARAMS[1]), int(PARAMS[0] + 3 * PARAMS[1]), PARAMS[2], PARAMS[3])
    ptr = lambda x: x.ctypes.data
    host_args = [a.host, W["fasta"], os.path.join(tmp, "exons.txt"), os.path.join(tmp, "regions.txt")] + [str(v) for v in PARAMS]

    # the one-time objects
    t_ref, t_ex = [], []
    ref, ex = ctypes.c_void_p(), ctypes.c_void_p()
    for rep in range(3):
        for h, fn in ((ref, lib.task_reference_destroy), (ex, lib.task_exons_destroy)):
            if h:
                fn(h)
        t0 = time.perf_counter()
        assert lib.task_reference_create(0, ptr(W["data"]), W["data"].size, ptr(W["seqs"]), len(W["seqs"]), ctypes.byref(ref)) == 0, err()
        t1 = time.perf_counter()
        assert lib.task_exons_create(0, ptr(W["chrom_ref"]), len(W["chrom_ref"]), ptr(W["tx"]), len(W["tx"]), ptr(W["exons"]), len(W["exons"]), ctypes.byref(ex)) == 0, err()
        t2 = time.perf_counter()
        t_ref.append((t1 - t0) * 1e3)
        t_ex.append((t2 - t1) * 1e3)

    pairs = W["pairs"]

    def create():
        s = ctypes.c_void_p()
        assert lib.task_store_create(ref, ex, ctypes.byref(prm), ptr(pairs), len(pairs), ctypes.byref(s)) == 0, err()
        return s

    # both paths give the same tasks, before anything is timed
    prefix = os.path.join(tmp, "host")
    subprocess.run(host_args + ["16", "1", prefix], check=True, capture_output=True)
    s = create()
    c = task.Counts()
    assert lib.task_store_counts(s, ctypes.byref(c)) == 0
    rec = np.zeros(c.n_tasks, dtype=task.RECORD_DTYPE)
    win, rem = np.zeros(c.window_bytes, dtype=np.uint8), np.zeros(c.rem_bytes, dtype=np.uint8)
    reg = np.zeros(c.n_regions, dtype=cand.REGION_DTYPE)
    assert lib.task_store_fetch(s, ptr(rec), len(rec), ptr(win), len(win), ptr(rem), len(rem), ptr(reg), len(reg)) == 0, err()
    lib.task_store_destroy(s)
    assert (rec["status"] == 0).all()
    hrec = np.fromfile(prefix + ".rec", dtype=np.int32).reshape(-1, 11)
    mine = np.column_stack([rec["fusion_id"], rec["seq_start"], rec["seq_len"], rec["seq_strand"], rec["rem_len"], rec["n_regions"]])
    assert mine.shape == hrec.shape and (mine == hrec).all(), "the task records of the two paths differ"
    assert win.tobytes() == open(prefix + ".win", "rb").read(), "the windows of the two paths differ"
    assert rem.tobytes() == open(prefix + ".rem", "rb").read(), "the remainders of the two paths differ"
    index = {n: k for k, n in enumerate(W["names"])}
    hreg = [l.split("\t") for l in open(prefix + ".reg").read().splitlines()]
    assert len(hreg) == len(reg), "the numbers of mate regions differ"
    theirs = np.array([(index[r[0]], int(r[1]), int(r[2]), int(r[3])) for r in hreg], dtype=np.int64)
    assert (np.column_stack([reg["ref"], reg["strand"], reg["start"], reg["end"]]) == theirs).all(), "the mate regions of the two paths differ"
    ids = np.repeat(np.repeat(rec["fusion_id"].astype(np.int64), 2) | (np.tile(np.array([0, 1], dtype=np.int64), len(rec)) << 31), rec["n_regions"].reshape(-1))
    assert (reg["id"].astype(np.int64) & 0xFFFFFFFF == ids).all(), "the ids of the mate regions differ"
    print("identical: %d tasks, %d window bytes, %d remainder bytes, %d mate regions" % (c.n_tasks, c.window_bytes, c.rem_bytes, c.n_regions), flush=True)

    host = {"1": [], "16": []}
    tb, tf = [], []
    stages = {k: [] for k in ("upload_ms", "plan_ms", "count_ms", "scan_ms", "region_ms", "gather_ms", "sort_ms", "download_ms")}
    tm = task.TaskTiming()
    for rep in range(a.warmup + a.repeats):
        lines = {}
        for threads in ("1", "16"):
            if threads == "1" and rep >= a.warmup + 5:
                continue                                                   # (seconds each: five timed rounds of the single thread)
            out = subprocess.run(host_args + [threads, "1"], check=True, capture_output=True, text=True).stdout.split()
            lines[threads] = {out[k]: float(out[k + 1]) for k in range(3, len(out) - 1, 2)}
        t0 = time.perf_counter()
        s = create()
        t1 = time.perf_counter()
        assert lib.task_store_fetch(s, ptr(rec), len(rec), None, 0, None, 0, ptr(reg), len(reg)) == 0, err()
        t2 = time.perf_counter()
        assert lib.task_store_get_timing(s, ctypes.byref(tm)) == 0
        lib.task_store_destroy(s)
        if rep >= a.warmup:
            for threads, l in lines.items():
                host[threads].append(l)
            tb.append((t1 - t0) * 1e3)
            tf.append((t2 - t1) * 1e3)
            for k in stages:
                stages[k].append(getattr(tm, k))
    lib.task_exons_destroy(ex)
    lib.task_reference_destroy(ref)

    hs = {t: {k: stats([l[k] for l in host[t]]) for k in host[t][0] if k.endswith("_ms")} for t in host}
    moved = 2 * (c.window_bytes + c.rem_bytes)
    res = dict(fusions=a.fusions, reference_bytes=int(W["data"].size), sequences=len(W["seqs"]), transcripts=a.transcripts, exons=len(W["exons"]),
               params=list(PARAMS), window_bytes=c.window_bytes, rem_bytes=c.rem_bytes, mate_regions=c.n_regions, library=dsa.load_library().dsa_version().decode(),
               a_host=hs, b_task_store_create_ms=stats(tb), b_fetch_records_regions_ms=stats(tf), b_stages={k: stats(v) for k, v in stages.items()},
               one_time_task_reference_create_ms=stats(t_ref), one_time_task_exons_create_ms=stats(t_ex), gather_bytes_moved=int(moved),
               gather_GB_per_s=moved / (stats(stages["gather_ms"])["median"] * 1e-3) / 1e9, bat_pred_gather_GB_per_s=[1760, 1970],
               resources=[dict(kernel=k, vgprs=v, sgprs=sg, scratch_bytes_per_lane=sc, waves_per_simd=o) for k, v, sg, sc, o in RESOURCES])
    res["b_below_a_16_threads"] = res["b_task_store_create_ms"]["median"] + res["b_fetch_records_regions_ms"]["median"] < hs["16"]["total_ms"]["median"]
    print(json.dumps(res), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    fmt = lambda s: "%.3f ms (%.3f - %.3f, n = %d)" % (s["median"], s["min"], s["max"], s["n"])
    rows = ["| (a) host path, %s thread%s: `CreateTasks` + packing + `bat_windows_create` + `pred_tasks_create` | %s |\n| of which `CreateTasks` | %s |\n"
            "| of which the packing | %s |\n| of which `bat_windows_create` | %s |\n| of which `pred_tasks_create` | %s |\n" %
            (t, "" if t == "1" else "s", fmt(hs[t]["total_ms"]), fmt(hs[t]["create_tasks_ms"]), fmt(hs[t]["pack_ms"]), fmt(hs[t]["windows_create_ms"]),
             fmt(hs[t]["pred_tasks_create_ms"])) for t in ("1", "16")]
    names = dict(upload_ms="the pairs to the device", plan_ms="plan kernel", count_ms="region kernel, counting", scan_ms="three sums, totals to the host (one round trip)",
                 region_ms="region kernel, emitting; records and gather descriptors", gather_ms="the two gather launches", sort_ms="radix sort and the two stores' key order",
                 download_ms="`task_store_fetch` of records and regions (HIP events)")
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("""# The first link of the resident chain: the tasks made on the device (`include/defuse_task.h`)

Written by `profiles/microbench/task_throughput.py` on one MI355X (numbers: `result.json`, library `%s`).

Problem, generated from a seed: %.0f MB of reference (24 chromosomes and %d transcript sequences, %d exons), %d align region
pairs of 50-400 bases, 60 %% of the ends on a transcript reference, parameters (300, 30, 50, 50): %.1f MB of windows, %.1f MB of
remainders, %d mate regions.  %d warm-up rounds, medians with min - max, the paths alternating round by round; the host path is
one process per round (`profiles/microbench/task_host.cpp`, the tool's own `CreateTasks`; its device is up before its clock
starts, the FASTA is in the page cache), the device path a host clock around calls that return synchronised.  The tasks of the
two paths were compared first and are identical: every field, both byte pools, every mate region.

| | |
|---|---|
%s| (b) `task_store_create` | %s |
| (b) `task_store_fetch` of the records and the regions, no pool bytes (host clock) | %s |
%s
| one-time `task_reference_create` (the reference bytes to the device, pageable host memory) | %s |
| one-time `task_exons_create` (derived columns and bins on the host, then the copies) | %s |

(b) is %s (a) at 16 threads.  %s

The stages of (b) add up to about a sixth of the call: the rest is host work around them, above all the allocation and release of
the store's and the call's device buffers (some twenty `hipMalloc` / `hipFree`), which a caller pays once per regions file.

The two gather launches (`gather_ms` holds nothing else) read and write %.1f MB together: an achieved %.0f GB/s, beside the
1760-1970 GB/s of the gathers of `profiles/bat` and `profiles/pred`.  Why it is lower has not been looked into; the launches
are short (0.11 ms for both) and the sources lie scattered over a reference of some hundred megabytes.

## Kernel resources

`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `defuse_amd/csrc/task_api.hip`:

| kernel | VGPRs | SGPRs | scratch bytes per lane | waves per SIMD |
|---|---|---|---|---|
%s

No kernel uses scratch or LDS; all reach the full occupancy of 8 waves per SIMD.

## What has not been measured

The region kernel lays 16 lanes over a (task, end)'s bin and compacts with a ballot; the alternative (a per-segment
sort) and other group widths have not been timed against it.  The reference here is random bases, which costs the gather the same
as a real one; the density of transcripts per 100 kb bin follows from --transcripts and --chrom-mb and is above a real genome's.
""" % (res["library"], W["data"].size / 1e6, a.transcripts, len(W["exons"]), a.fusions, c.window_bytes / 1e6, c.rem_bytes / 1e6, c.n_regions, a.warmup, "".join(rows),
       fmt(res["b_task_store_create_ms"]), fmt(res["b_fetch_records_regions_ms"]),
       "\n".join("| of which %s | %s |" % (names[k], fmt(res["b_stages"][k])) for k in stages if k != "download_ms") + "\n| %s | %s |" % (names["download_ms"], fmt(res["b_stages"]["download_ms"])),
       fmt(res["one_time_task_reference_create_ms"]), fmt(res["one_time_task_exons_create_ms"]),
       "below" if res["b_below_a_16_threads"] else "NOT below",
       "The windows never exist on the host either way." if res["b_below_a_16_threads"] else "The windows staying off the host is then the remaining argument.",
       moved / 1e6, res["gather_GB_per_s"],
       "\n".join("| `%s` | %d | %d | %d | %d |" % r for r in RESOURCES)))
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
