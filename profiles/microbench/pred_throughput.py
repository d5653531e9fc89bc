"""What the last link of the resident chain costs against the host work it replaces: each fusion's predicted sequence,
break positions and averages from the groups of eval_groups_device.

    python profiles/microbench/pred_throughput.py [--fusions 100000] [--alignments 1300000] [--repeats 25] [--out-dir profiles/pred]

The problem is the chunk of cand_throughput.py (make_problem) with the reads and windows of bat_throughput.py (2x150, two
windows of 540 bases per fusion), taken through the resident chain up to the DP records in device memory.  Every fusion has
a task: random window starts and strands, and for half of the cluster ends a remainder sequence of 1-100 bases.  Timed in
one process, alternating, after a warm-up, as medians of --repeats with min-max, by a host clock around calls that return
synchronised:

  (a) what a chain caller does without pred: eval_groups_device with its download of groups and kept indices, then the
      assembly of every group's sequence, break positions and averages on the host from host copies of the windows.  The
      host assembly here is a Python loop over the groups that slices and joins bytes objects and fills numpy arrays: it
      stands for the caller's own loop and is slower than a C++ one would be;
  (b) eval_groups_device + pred_predict_resident + pred_fetch;
  (c) the two gather launches alone by HIP events (pred_timing.gather_ms), with the bytes they read and wrote per second.

Before anything is timed the results and the sequence bytes of (a) and (b) are compared for equality.  Writes result.json
and README.md into --out-dir."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def host_predict(groups, tasks, win_mat, rem_bytes, out):
    """(a)'s host assembly: tools/SplitAlignment.cpp:545-569, 589-591 per group into `out` (pred.RESULT_DTYPE); returns the
    sequence bytes.  Every group of this problem has a task."""
    parts, off = [], 0
    rem = rem_bytes.tobytes()
    fid, first, second = groups["fusion_id"].tolist(), groups["best_first"].tolist(), groups["best_second"].tolist()
    start, length, strand = tasks["seq_start"].tolist(), tasks["seq_len"].tolist(), tasks["seq_strand"].tolist()
    rem_off, rem_len = tasks["rem_off"].tolist(), tasks["rem_len"].tolist()
    seq_off, seq_len, bp, status = [], [], [], groups["status"].tolist()
    for g in range(len(groups)):
        t, f, s = fid[g], first[g], second[g]                                      # (task t has fusion_id t)
        if status[g] & 1 or f < 0 or f > length[t][0] or s + 1 < 0 or s + 1 >= length[t][1]:
            if not status[g] & 1:
                status[g] |= 8
            seq_off.append(off)
            seq_len.append(0)
            bp.append((0, 0))
            continue
        w0, w1 = win_mat[t, 0], win_mat[t, 1]
        seq = b"".join((rem[rem_off[t][0]:rem_off[t][0] + rem_len[t][0]], w0[:f].tobytes(), b"|", w1[s + 1:].tobytes(),
                        rem[rem_off[t][1]:rem_off[t][1] + rem_len[t][1]]))
        parts.append(seq)
        seq_off.append(off)
        seq_len.append(len(seq))
        off += len(seq)
        bp.append((start[t][0] + f - 1 if strand[t][0] == 0 else start[t][0] + length[t][0] - f,
                   start[t][1] + s + 1 if strand[t][1] == 0 else start[t][1] + length[t][1] - s - 2))
    out["fusion_id"], out["status"], out["count"] = groups["fusion_id"], status, groups["count"]
    out["seq_off"], out["seq_len"], out["break_pos"] = seq_off, seq_len, bp
    has = (out["seq_len"] > 0) & (out["status"] & 2 == 0)
    out["pos_avg"] = np.where(has, groups["pos_sum"] / np.maximum(groups["count"], 1).astype(np.float64), 0.0)
    out["min_avg"] = np.where(has, groups["min_sum"] / np.maximum(groups["count"], 1).astype(np.float64), 0.0)
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusions", type=int, default=100_000)
    ap.add_argument("--alignments", type=int, default=1_300_000)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "pred"))
    a = ap.parse_args()
    assert a.repeats >= 20
    from cand_throughput import make_problem
    from defuse_amd import bat, cand, dsa, pred, synth
    from defuse_amd import eval as ev
    rng = np.random.default_rng(7)
    regs, als = make_problem(a.fusions, a.alignments)
    lq, lr = 150, synth.window_length(450, 30, 150, 150, 300)
    win_mat = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(a.fusions, 2, lr), dtype=np.uint8)]
    wfus = np.zeros(a.fusions, dtype=dsa.FUSION_DTYPE)
    wfus["fusion_id"] = np.arange(a.fusions, dtype=np.int32)
    wfus["ref0_off"] = np.arange(a.fusions, dtype=np.int64) * 2 * lr
    wfus["ref0_len"] = wfus["ref1_len"] = lr
    wfus["ref1_off"] = wfus["ref0_off"] + lr

    table = cand.Table(regs)
    session = table.session()
    ptr, n = session.enumerate_device(als, cand.ORDER_FUSION)
    cands = np.zeros(n, dtype=cand.RECORD_DTYPE)
    hip = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = ctypes.CDLL(line.split()[-1])
            break
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    assert hip.hipMemcpy(cands.ctypes.data, ptr, cands.nbytes, 2) == 0
    # the reads of bat_throughput.py: each crosses the junction of the fusion its fragment was made for
    keys = np.unique((cands["fragment"].astype(np.uint32) & 0x7FFFFFFF) | (cands["read_end"].astype(np.uint32) << 31))
    owner = ((keys & 0x7FFFFFFF) // 6 % a.fusions).astype(np.int64)
    cut = rng.integers(8, lq - 8, size=len(keys))
    col = np.arange(lq, dtype=np.int64)[None, :]
    read_mat = np.where(col < cut[:, None], win_mat[owner, 0][np.arange(len(keys))[:, None], np.minimum(lr - 100 - cut[:, None] + col, lr - 1)],
                        win_mat[owner, 1][np.arange(len(keys))[:, None], np.clip(100 - cut[:, None] + col, 0, lr - 1)])
    rrec = np.zeros(len(keys), dtype=bat.READ_DTYPE)
    rrec["off"] = np.arange(len(keys), dtype=np.int64) * lq
    rrec["len"] = lq
    rrec["fragment"] = (keys & 0x7FFFFFFF).astype(np.int32)
    rrec["read_end"] = (keys >> 31).astype(np.int32)
    reads = bat.Reads(read_mat.reshape(-1), rrec)
    windows = bat.Windows(win_mat.reshape(-1), wfus)
    batch = bat.Batch()
    ctx = dsa.Context(0)
    ctx.upload_device(batch.assemble_device(reads, windows, ptr, n))
    n_rec = ctx.run()
    assert n_rec > 0, "the batch aligns nowhere"
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), n_rec * 40) == 0
    assert ctx.records_to_device(dev.value, n_rec) == n_rec

    # the tasks: task t has fusion_id t
    tasks = np.zeros(a.fusions, dtype=pred.TASK_DTYPE)
    tasks["fusion_id"] = np.arange(a.fusions)
    tasks["seq_start"] = rng.integers(1, 10 ** 8, size=(a.fusions, 2))
    tasks["seq_len"] = lr
    tasks["seq_strand"] = rng.integers(0, 2, size=(a.fusions, 2))
    tasks["rem_len"] = np.where(rng.random((a.fusions, 2)) < 0.5, rng.integers(1, 101, size=(a.fusions, 2)), 0)
    ends = np.cumsum(tasks["rem_len"].reshape(-1).astype(np.int64))
    tasks["rem_off"] = (ends - tasks["rem_len"].reshape(-1)).reshape(-1, 2)
    rem_bytes = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(ends[-1]), dtype=np.uint8)]
    ptasks = pred.Tasks(windows, rem_bytes, tasks)
    ectx = ev.Context(0)
    pctx = pred.Context(ptasks)

    groups = np.zeros(n_rec, dtype=ev.GROUP_DTYPE)
    kept = np.zeros(n_rec, dtype=np.int64)
    ng, nk = ctypes.c_int64(), ctypes.c_int64()

    def evaluate():
        rc = ectx.lib.eval_groups_device(ectx.h, dev, n_rec, groups.ctypes.data, len(groups), ctypes.byref(ng), kept.ctypes.data, len(kept), ctypes.byref(nk))
        assert rc == 0, ectx.lib.eval_last_error()
        return groups[:ng.value]

    # both paths give the same results and the same bytes, before anything is timed
    g = evaluate()
    assert len(g) > 0
    res_a = np.zeros(len(g), dtype=pred.RESULT_DTYPE)
    seq_a = host_predict(g, tasks, win_mat, rem_bytes, res_a)
    pctx.predict_resident(ectx)
    res_b, seq_b = pctx.fetch()
    assert res_b.tobytes() == res_a.tobytes(), "the results of the two paths differ"
    assert seq_b.tobytes() == seq_a, "the sequences of the two paths differ"
    lib, h = pctx._lib, pctx.handle

    ta, tb, te, th = [], [], [], []
    tim = {k: [] for k in ("plan_ms", "scan_ms", "gather_ms", "download_ms")}
    for rep in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        g = evaluate()
        t1 = time.perf_counter()
        host_predict(g, tasks, win_mat, rem_bytes, res_a)
        t2 = time.perf_counter()
        evaluate()
        assert lib.pred_predict_resident(h, ptasks.handle, ectx.h) == 0
        assert lib.pred_fetch(h, res_b.ctypes.data, len(res_b), seq_b.ctypes.data, len(seq_b)) == 0
        t3 = time.perf_counter()
        if rep >= a.warmup:
            ta.append((t2 - t0) * 1e3)
            te.append((t1 - t0) * 1e3)
            th.append((t2 - t1) * 1e3)
            tb.append((t3 - t2) * 1e3)
            t = pctx.timing()
            for k in tim:
                tim[k].append(t[k])
    assert res_b.tobytes() == res_a.tobytes() and seq_b.tobytes() == seq_a
    moved = 2 * (len(seq_a) - int((res_a["seq_len"] > 0).sum()))                                              # the gathers write every byte but the separators
    res = dict(fusions=a.fusions, alignments=len(als), candidates=int(n), records=int(n_rec), groups=len(g), window_len=lr,
               remainder_bytes=int(len(rem_bytes)), seq_bytes=len(seq_a), library=dsa.load_library().dsa_version().decode(),
               a_eval_download_host_assembly_ms=stats(ta), a_eval_groups_device_ms=stats(te), a_host_assembly_python_ms=stats(th),
               b_eval_predict_resident_fetch_ms=stats(tb), b_minus_eval_ms=stats(tb)["median"] - stats(te)["median"],
               c_gather_ms=stats(tim["gather_ms"]), plan_ms=stats(tim["plan_ms"]), scan_ms=stats(tim["scan_ms"]), fetch_ms=stats(tim["download_ms"]),
               gather_bytes_moved=int(moved), gather_GB_per_s=moved / (stats(tim["gather_ms"])["median"] * 1e-3) / 1e9,
               bat_gather_GB_per_s=1760, b_not_above_a=stats(tb)["median"] <= stats(ta)["median"])
    print(json.dumps(res), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    fmt = lambda s: "%.3f ms (%.3f - %.3f, n = %d)" % (s["median"], s["min"], s["max"], s["n"])
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("""# The last link of the resident chain: sequences and break positions on the device

Written by `profiles/microbench/pred_throughput.py` on one MI355X (numbers: `result.json`, library `%s`).

Problem: the chunk of `cand_throughput.py` (%d fusions, %d improper mate alignments) through the resident chain: %d
candidates, %d DP records in device memory, %d groups.  Two windows of %d bases per fusion, %.1f MB of remainder
sequences (half of the cluster ends have one, of 1-100 bases); the predicted sequences are %.1f MB.  One process, the two
paths alternating, %d warm-up rounds, medians with min - max, host clock around calls that return synchronised.  The results
and the sequence bytes of the two paths were compared first and are identical.

| | |
|---|---|
| (a) `eval_groups_device` with its download + host assembly from host copies of the windows | %s |
| of which `eval_groups_device` | %s |
| of which the host assembly (a Python loop over the groups: bytes slices and joins, numpy columns) | %s |
| (b) `eval_groups_device` + `pred_predict_resident` + `pred_fetch` | %s |
| (c) the two gather launches alone (HIP events) | %s |
| plan kernel | %s |
| 64-bit sum, total to the host, descriptors (one host round trip inside) | %s |
| `pred_fetch` (HIP events, pageable host memory) | %s |

(b) costs %.3f ms more than the `eval_groups_device` call it contains.  The gathers read and write %.1f MB together: an
achieved rate of %.0f GB/s, beside the 1760 GB/s of the batch assembly's gathers (`profiles/bat/README.md`), whose segments
are whole reads and windows; here a group's four segments are a window cut at the break and remainders of at most 100 bases.

(b) is %s (a).  The host assembly of (a) is a Python loop and stands for the caller's own; a C++ loop would be faster, so the
ratio between (a) and (b) says less than what (b) costs on top of the evaluation, and that the windows need no host copy.
""" % (res["library"], a.fusions, len(als), n, n_rec, len(g), lr, len(rem_bytes) / 1e6, len(seq_a) / 1e6, a.warmup,
       fmt(res["a_eval_download_host_assembly_ms"]), fmt(res["a_eval_groups_device_ms"]), fmt(res["a_host_assembly_python_ms"]),
       fmt(res["b_eval_predict_resident_fetch_ms"]), fmt(res["c_gather_ms"]), fmt(res["plan_ms"]), fmt(res["scan_ms"]), fmt(res["fetch_ms"]),
       res["b_minus_eval_ms"], moved / 1e6, res["gather_GB_per_s"], "not above" if res["b_not_above_a"] else "ABOVE"))
    assert hip.hipFree(dev) == 0
    for o in (pctx, ptasks, batch, windows, reads, session, table):
        o.close()
    ectx.close()
    ctx.close()


if __name__ == "__main__":
    main()
