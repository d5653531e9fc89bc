"""What printing splitreads.seq and splitreads.break on the device costs beside the download any host formatter pays first.

    python profiles/microbench/ptext_throughput.py [--fusions 100000] [--alignments 1300000] [--repeats 25] [--out-dir profiles/ptext]

The problem is the chunk of pred_throughput.py: make_problem of cand_throughput.py with the reads and windows of
bat_throughput.py, through the resident chain up to pred_predict_resident (97 881 groups, 91 MB of sequences with the
defaults).  Every fusion's two ends have one of 25 reference names and a random align strand.  Timed in one process,
alternating, after a warm-up, as medians of --repeats with min-max, by a host clock around calls that return synchronised:

  (a) pred_fetch alone: the binary rows and the byte pool that a host formatter needs before it can print a line;
  (b) ptext_format + ptext_fetch: the finished bytes of both files and the line table, with the device parts by HIP events
      (ptext_get_timing) and the bytes the gather reads and writes per second.

Before anything is timed both texts are compared with pred.Context.format_seq / format_break over the rows of (a).  Writes
result.json and README.md into --out-dir."""
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

# -Rpass-analysis=kernel-resource-usage of defuse_amd/csrc/ptext_api.hip for gfx950 (hipcc of ROCm 7.2, -O3)
RESOURCES = """| kernel | VGPRs | SGPRs | scratch | LDS | occupancy (waves/SIMD) |
|---|---|---|---|---|---|
| `k_ptext_lengths` (status rules, `%g` twice, line lengths) | 38 | 48 | 0 | 32 B (the block sum of the bytes to copy) | 8 |
| `k_ptext_totals` | 5 | 22 | 0 | 0 | 8 |
| `k_ptext_write` (`%g` twice, heads, tails, `.break` lines, rows, segments) | 48 | 46 | 0 | 0 | 8 |
| `k_bat_gather<64, false, Seg64>` | 21 | 16 | 0 | 0 | 8 |
| `k_ptext_g_lengths` / `k_ptext_g_write` (`ptext_format_doubles`) | 24 / 22 | 34 / 34 | 0 | 0 | 8 |

No kernel of the module uses scratch: the formatter keeps its six digits in one register and its 128 fraction bits in four, and
writes digits from the last to the first with divisions by the constant 10, so nothing is indexed at run time."""


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusions", type=int, default=100_000)
    ap.add_argument("--alignments", type=int, default=1_300_000)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ptext"))
    a = ap.parse_args()
    assert a.repeats >= 20
    from cand_throughput import make_problem
    from defuse_amd import bat, cand, dsa, pred, ptext, synth
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

    # the resident chain of pred_throughput.py up to the DP records in device memory
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

    tasks = np.zeros(a.fusions, dtype=pred.TASK_DTYPE)
    tasks["fusion_id"] = np.arange(a.fusions)
    tasks["seq_start"] = rng.integers(1, 10 ** 8, size=(a.fusions, 2))
    tasks["seq_len"] = lr
    tasks["seq_strand"] = rng.integers(0, 2, size=(a.fusions, 2))
    tasks["rem_len"] = np.where(rng.random((a.fusions, 2)) < 0.5, rng.integers(1, 101, size=(a.fusions, 2)), 0)
    rem_ends = np.cumsum(tasks["rem_len"].reshape(-1).astype(np.int64))
    tasks["rem_off"] = (rem_ends - tasks["rem_len"].reshape(-1)).reshape(-1, 2)
    rem_bytes = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(rem_ends[-1]), dtype=np.uint8)]
    ptasks = pred.Tasks(windows, rem_bytes, tasks)
    ectx = ev.Context(0)
    pctx = pred.Context(ptasks)

    # the names: 25 of them, per cluster end a name and an align strand
    names = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrY", b"GL000192.1"]
    name_off = np.zeros(len(names) + 1, dtype=np.int64)
    name_off[1:] = np.cumsum([len(x) for x in names])
    ends = np.zeros(2 * a.fusions, dtype=ptext.END_DTYPE)
    ends["fusion_id"] = np.repeat(np.arange(a.fusions, dtype=np.int32), 2)
    ends["cluster_end"] = np.tile(np.array([0, 1], dtype=np.int32), a.fusions)
    ends["name"] = rng.integers(0, len(names), size=2 * a.fusions)
    ends["strand"] = rng.integers(0, 2, size=2 * a.fusions)
    pnames = ptext.Names(np.frombuffer(b"".join(names), dtype=np.uint8), name_off, ends)
    tctx = ptext.Context(pnames)

    groups = np.zeros(n_rec, dtype=ev.GROUP_DTYPE)
    kept = np.zeros(n_rec, dtype=np.int64)
    ng, nk = ctypes.c_int64(), ctypes.c_int64()
    rc = ectx.lib.eval_groups_device(ectx.h, dev, n_rec, groups.ctypes.data, len(groups), ctypes.byref(ng), kept.ctypes.data, len(kept), ctypes.byref(nk))
    assert rc == 0, ectx.lib.eval_last_error()
    pctx.predict_resident(ectx)

    # equal outputs, before anything is timed
    res, seq = pctx.fetch()
    tctx.format(pctx)
    seq_text, brk_text, lines = tctx.fetch()
    want_seq, want_brk, n_host_seq = [], [], 0
    dec = [x.decode() for x in names]
    ename, estrand = ends["name"].reshape(-1, 2).tolist(), ends["strand"].reshape(-1, 2).tolist()
    for row in res:
        fid, st = int(row["fusion_id"]), int(row["status"])
        if st & 12:
            continue
        nm = [dec[ename[fid][0]], dec[ename[fid][1]]]
        if st & 1:
            want_seq.append("%d\tN\t0\t0\t-1\t-1\n" % fid)
            want_brk.append("".join("%d\t%d\t%s\t%s\t0\n" % (fid, ce, nm[ce], "+-"[estrand[fid][ce]]) for ce in (0, 1)))
            continue
        want_brk.append(pred.Context.format_break(row, nm, estrand[fid]))
        if st & 2:
            n_host_seq += 1
        else:
            want_seq.append(pred.Context.format_seq(row, seq))
    assert seq_text == "".join(want_seq).encode("latin-1"), "the .seq text differs from the host formatting"
    assert brk_text == "".join(want_brk).encode("latin-1"), "the .break text differs from the host formatting"
    assert int((lines["status"] & ptext.HOST_SEQ != 0).sum()) == n_host_seq
    assert int(lines["seq_len"].sum()) == len(seq_text) and int(lines["brk_len"].sum()) == len(brk_text)

    plib, ph = pctx._lib, pctx.handle
    tlib, th = tctx._lib, tctx.handle
    seq_buf, brk_buf = np.zeros(len(seq_text), np.uint8), np.zeros(len(brk_text), np.uint8)
    ta, tb, tf, tfe = [], [], [], []
    tim = {k: [] for k in ("lengths_ms", "write_ms", "gather_ms", "download_ms")}
    pdl = []
    for rep in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        assert plib.pred_fetch(ph, res.ctypes.data, len(res), seq.ctypes.data, len(seq)) == 0
        t1 = time.perf_counter()
        assert tlib.ptext_format(th, ph, pnames.handle) == 0
        t2 = time.perf_counter()
        assert tlib.ptext_fetch(th, seq_buf.ctypes.data, len(seq_buf), brk_buf.ctypes.data, len(brk_buf), lines.ctypes.data, len(lines)) == 0
        t3 = time.perf_counter()
        if rep >= a.warmup:
            ta.append((t1 - t0) * 1e3)
            tb.append((t3 - t1) * 1e3)
            tf.append((t2 - t1) * 1e3)
            tfe.append((t3 - t2) * 1e3)
            pdl.append(pctx.timing()["download_ms"])
            t = tctx.timing()
            for k in tim:
                tim[k].append(t[k])
    assert seq_buf.tobytes() == seq_text and brk_buf.tobytes() == brk_text
    t = tctx.timing()
    moved = 2 * t["gather_bytes"]
    device_ms = stats(tim["lengths_ms"])["median"] + stats(tim["write_ms"])["median"] + stats(tim["gather_ms"])["median"]
    out = dict(fusions=a.fusions, alignments=len(als), records=int(n_rec), groups=len(res), seq_bytes=len(seq), seq_text_bytes=len(seq_text),
               brk_text_bytes=len(brk_text), host_seq_groups=n_host_seq, library=dsa.load_library().dsa_version().decode(),
               a_pred_fetch_ms=stats(ta), a_pred_fetch_events_ms=stats(pdl), b_format_fetch_ms=stats(tb), b_format_ms=stats(tf), b_fetch_ms=stats(tfe),
               lengths_ms=stats(tim["lengths_ms"]), write_ms=stats(tim["write_ms"]), gather_ms=stats(tim["gather_ms"]), fetch_events_ms=stats(tim["download_ms"]),
               device_ms=device_ms, gather_bytes_moved=int(moved), gather_GB_per_s=moved / (stats(tim["gather_ms"])["median"] * 1e-3) / 1e9)
    print(json.dumps(out), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "result.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    fmt = lambda s: "%.3f ms (%.3f - %.3f, n = %d)" % (s["median"], s["min"], s["max"], s["n"])
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("""# splitreads.seq and splitreads.break printed on the device

Written by `profiles/microbench/ptext_throughput.py` on one MI355X (numbers: `result.json`, library `%s`).

Problem: the chunk of `pred_throughput.py` (%d fusions, %d improper mate alignments) through the resident chain up to
`pred_predict_resident`: %d DP records, %d groups, %.1f MB of predicted sequences.  Each cluster end has one of %d reference
names and a random align strand.  The `.seq` text is %.1f MB, the `.break` text %.1f MB, the line table %.1f MB; %d groups carry
`PTEXT_HOST_SEQ`.  One process, the paths alternating, %d warm-up rounds, medians with min - max, host clock around calls that return
synchronised.  Both texts were compared first with `pred.Context.format_seq` / `format_break` over the rows of (a) and are identical.
There is no parent number: the module is new.

| | |
|---|---|
| (a) `pred_fetch` alone: what a host formatter downloads before it prints its first line | %s |
| of which the copies by HIP events | %s |
| (b) `ptext_format` + `ptext_fetch` | %s |
| of which `ptext_format` (host clock, one round trip inside) | %s |
| of which `ptext_fetch` (host clock; pageable host memory) | %s |
| lengths kernel, two 64-bit sums, totals to the host (HIP events) | %s |
| write kernel: heads, tails, `.break` lines, rows, segments | %s |
| gather: the sequences into the `.seq` text | %s |
| `ptext_fetch` by HIP events | %s |

The device part of (b) is %.3f ms beside a download of %.3f ms.  The gather reads and writes %.1f MB together: an achieved
%.0f GB/s (the two gathers of `pred` on the same chunk: 1970 GB/s, `profiles/pred/README.md`; one segment per group here, of about
930 bytes; source and output together fit in the 256 MiB Infinity Cache, so this is no HBM rate).  Of the device part the lengths, sums and the round trip are %.0f %%, the write kernel %.0f %% and the gather %.0f %%.  (b) brings
down %.1f MB where (a) brings down %.1f MB; the caller of (a) still has every line to print.

## Resource usage

%s
""" % (out["library"], a.fusions, len(als), n_rec, len(res), len(seq) / 1e6, len(names), len(seq_text) / 1e6, len(brk_text) / 1e6, lines.nbytes / 1e6, n_host_seq,
       a.warmup, fmt(out["a_pred_fetch_ms"]), fmt(out["a_pred_fetch_events_ms"]), fmt(out["b_format_fetch_ms"]), fmt(out["b_format_ms"]), fmt(out["b_fetch_ms"]),
       fmt(out["lengths_ms"]), fmt(out["write_ms"]), fmt(out["gather_ms"]), fmt(out["fetch_events_ms"]), device_ms, out["fetch_events_ms"]["median"],
       moved / 1e6, out["gather_GB_per_s"], 100 * out["lengths_ms"]["median"] / device_ms, 100 * out["write_ms"]["median"] / device_ms,
       100 * out["gather_ms"]["median"] / device_ms, (len(seq_text) + len(brk_text) + lines.nbytes) / 1e6, (len(seq) + res.nbytes) / 1e6, RESOURCES))
    assert hip.hipFree(dev) == 0
    for o in (tctx, pnames, pctx, ptasks, batch, windows, reads, session, table):
        o.close()
    ectx.close()
    ctx.close()


if __name__ == "__main__":
    main()
