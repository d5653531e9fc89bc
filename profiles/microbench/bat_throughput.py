"""What the resident link between cand_enumerate and dsa_run costs against the upload it replaces.

    python profiles/microbench/bat_throughput.py [--fusions 100000] [--alignments 1300000] [--repeats 25] [--out-dir profiles/bat]

The problem is the chunk of cand_throughput.py (make_problem), plus one generated read of 150 bases for every (fragment,
read end) a candidate names (2x150) and two windows per fusion of synth.window_length(450, 30, 150, 150, 300) = 540 bases, the
length SplitAlignmentTask's arithmetic gives for these library parameters.  Timed in one process, alternating, after a
warm-up, as medians of --repeats with min-max:

  (a) dsa_upload of the finished batch from pinned host buffers: what the new path replaces, less the host gather that
      built those buffers;
  (b) bat_assemble_device + dsa_upload_device from candidates that are on the device already;
  (c) the two gather launches alone by HIP events (bat_timing.gather_ms), with the bytes they read and wrote per second.

Before anything is timed the batch of (b) is compared byte for byte with a numpy gather of the downloaded candidates, and
the records of dsa_run after (a) with those after (b).  Writes result.json and README.md into --out-dir."""
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


def host_batch(cands, keys, read_mat, fusion_ids, win_mat):
    """The batch of cand.dsa_batch for reads of one length and windows of one length, without its Python loop."""
    from defuse_amd import cand, dsa
    key = (cands["fragment"].astype(np.uint32) & 0x7FFFFFFF) | (cands["read_end"].astype(np.uint32) << 31)
    at = np.searchsorted(keys, key)
    assert (keys[at] == key).all()
    seqs = read_mat[at]
    rc = cands["revcomp"] != 0
    seqs[rc] = cand._COMPLEMENT[seqs[rc][:, ::-1]]
    lq, lr = read_mat.shape[1], win_mat.shape[2]
    uniq, first = np.unique(cands["fusion_id"], return_index=True)
    order = uniq[np.argsort(first, kind="stable")]
    slot = np.searchsorted(fusion_ids, order)
    fus = np.zeros(len(order), dtype=dsa.FUSION_DTYPE)
    fus["fusion_id"] = order
    fus["ref0_off"] = np.arange(len(order), dtype=np.int64) * 2 * lr
    fus["ref0_len"] = fus["ref1_len"] = lr
    fus["ref1_off"] = fus["ref0_off"] + lr
    fidx = np.zeros(int(fusion_ids.max()) + 1, dtype=np.int32)
    fidx[order] = np.arange(len(order), dtype=np.int32)
    pairs = np.zeros(len(cands), dtype=dsa.PAIR_DTYPE)
    pairs["fusion_idx"] = fidx[cands["fusion_id"]]
    pairs["read_off"] = np.arange(len(cands), dtype=np.int64) * lq
    pairs["read_len"] = lq
    pairs["frag"], pairs["read_end"], pairs["revcomp"] = cands["fragment"], cands["read_end"], cands["revcomp"]
    return win_mat[slot].reshape(-1), fus, seqs.reshape(-1), pairs


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusions", type=int, default=100_000)
    ap.add_argument("--alignments", type=int, default=1_300_000)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bat"))
    a = ap.parse_args()
    assert a.repeats >= 20
    from cand_throughput import make_problem
    from defuse_amd import bat, cand, dsa, synth
    rng = np.random.default_rng(7)
    regs, als = make_problem(a.fusions, a.alignments)
    lq, lr = 150, synth.window_length(450, 30, 150, 150, 300)
    fusion_ids = np.arange(a.fusions, dtype=np.int32)
    win_mat = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(a.fusions, 2, lr), dtype=np.uint8)]
    wfus = np.zeros(a.fusions, dtype=dsa.FUSION_DTYPE)
    wfus["fusion_id"] = fusion_ids
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
    assert hip.hipMemcpy(cands.ctypes.data, ptr, cands.nbytes, 2) == 0
    # 2x150: one read for every key a candidate names
    keys = np.unique((cands["fragment"].astype(np.uint32) & 0x7FFFFFFF) | (cands["read_end"].astype(np.uint32) << 31))
    # each read crosses the junction of the fusion its fragment was made for (cand_throughput: fragment = fusion * 6 + k), as
    # synth.make_batch builds its reads, so that the candidates met without reverse complement align and the DP has records
    owner = ((keys & 0x7FFFFFFF) // 6 % a.fusions).astype(np.int64)
    cut = rng.integers(8, lq - 8, size=len(keys))
    col = np.arange(lq, dtype=np.int64)[None, :]
    left = col < cut[:, None]
    read_mat = np.where(left, win_mat[owner, 0][np.arange(len(keys))[:, None], np.minimum(lr - 100 - cut[:, None] + col, lr - 1)],
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

    # both paths give the same batch and the same records, before anything is timed
    host = host_batch(cands, keys, read_mat, fusion_ids, win_mat)
    view = batch.assemble_device(reads, windows, ptr, n)
    for got, want in zip(batch.fetch(), host):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    pinned = [dsa.pinned_copy(x) for x in host]
    ctx.upload(*(p.array for p in pinned))
    ctx.run()
    rec_a, tile_a = ctx.download(), ctx.tile_cols_in_use()
    ctx.upload_device(view)
    ctx.run()
    rec_b = ctx.download()
    assert len(rec_a) > 0, "the batch aligns nowhere"
    assert tile_a == ctx.tile_cols_in_use() and len(rec_a) == len(rec_b) and rec_a.tobytes() == rec_b.tobytes(), "the records of the two paths differ"

    ta, tb, tg, tl, ts = [], [], [], [], []
    for rep in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        ctx.upload(*(p.array for p in pinned))
        t1 = time.perf_counter()
        view = batch.assemble_device(reads, windows, ptr, n)
        ctx.upload_device(view)
        t2 = time.perf_counter()
        if rep >= a.warmup:
            t = batch.timing()
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
            tg.append(t.gather_ms)
            tl.append(t.lookup_ms)
            ts.append(t.scan_ms)
    t = batch.timing()
    moved = 2 * (t.read_bytes + t.ref_bytes)
    res = dict(fusions=a.fusions, alignments=len(als), candidates=int(n), reads=len(keys), read_len=lq, window_len=lr, fusions_used=int(t.n_fusions),
               read_bytes=int(t.read_bytes), ref_bytes=int(t.ref_bytes), records=len(rec_a), library=dsa.load_library().dsa_version().decode(),
               a_upload_pinned_ms=stats(ta), b_assemble_upload_device_ms=stats(tb), c_gather_ms=stats(tg), lookup_ms=stats(tl), scan_ms=stats(ts),
               gather_bytes_moved=int(moved), gather_GB_per_s=moved / (stats(tg)["median"] * 1e-3) / 1e9,
               b_not_above_a=stats(tb)["median"] <= stats(ta)["median"])
    print(json.dumps(res), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    fmt = lambda s: "%.3f ms (%.3f - %.3f, n = %d)" % (s["median"], s["min"], s["max"], s["n"])
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("""# The resident link between the candidate loop and the split-read DP

Written by `profiles/microbench/bat_throughput.py` on one MI355X (numbers: `result.json`, library `%s`).

Problem: the chunk of `cand_throughput.py` (%d fusions, %d improper mate alignments), %d kept candidates in fusion order,
%d reads of %d bases, two windows of %d bases per fusion; the batch has %d fusions, %.1f MB of read bytes and %.1f MB of window
bytes.  One process, the two paths alternating, %d warm-up rounds, medians with min - max.  The records of `dsa_run` after
both paths were compared first and are identical (%d records), and the assembled batch equals a numpy gather byte for byte.

| | |
|---|---|
| (a) `dsa_upload` of the finished batch from pinned host buffers | %s |
| (b) `bat_assemble_device` + `dsa_upload_device`, candidates on the device | %s |
| (c) the two gather launches alone (HIP events) | %s |
| lookup kernel | %s |
| sums, compaction, sort, descriptors (one host round trip inside) | %s |

The gathers read and write %.1f MB together: an achieved rate of %.0f GB/s.

(b) is %s (a).  (a) leaves out what the host spends on building the buffers it uploads (the loop of `cand.dsa_batch`, or its
C++ twin in a tool), and the download of the candidate records that loop needs (`profiles/cand/README.md`: 2.1 ms per 38 MB);
(b) contains everything between the candidates and a planned upload.  Both contain the same planning (`enqueue_plan`).
""" % (res["library"], a.fusions, len(als), n, len(keys), lq, lr, t.n_fusions, t.read_bytes / 1e6, t.ref_bytes / 1e6, a.warmup, len(rec_a),
       fmt(res["a_upload_pinned_ms"]), fmt(res["b_assemble_upload_device_ms"]), fmt(res["c_gather_ms"]), fmt(res["lookup_ms"]), fmt(res["scan_ms"]),
       moved / 1e6, res["gather_GB_per_s"], "not above" if res["b_not_above_a"] else "ABOVE"))
    for p in pinned:
        p.free()
    for o in (batch, windows, reads, session, table):
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
