"""What the record store costs on the bench workload, against what it replaces.

    python profiles/microbench/rec_throughput.py [--fusions 10000] [--reads 100] [--repeats 20] [--out-dir profiles/rec]

The records are those of BASELINE configs[1] (10k fusions x 100 reads, 2x76: about 1.76 M records) from dsa_run.  They are
dealt into ten shares by read (frag mod 10), as the chunks of a run would hold them: every fusion is in every share.  One
process, after a warm-up, the arms alternating, medians of --repeats with min - max:

  (a) the store: ten rec_append from the host, rec_sort, rec_text of all lines into a host buffer.  The parts by HIP events
      (rec_get_timing), the whole by a host clock around the calls, which return synchronised;
  (b) dsa_download alone, host clock;
  (c) dsa_download, then `LC_ALL=C sort -n -k 1` of the printed lines as the pipeline calls it (a file in, a file out).  The
      lines are printed once, outside the clock, so (c) is short of the time its printing takes.  Every fourth round only.

Before anything is timed the store's text is compared with sort's output for equality.  Prints one JSON line and writes
result.json into --out-dir."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusions", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "rec"))
    a = ap.parse_args()
    from defuse_amd import dsa, rec, synth
    ctx = dsa.Context(0)
    ctx.upload(*synth.make_batch(a.fusions, a.reads, lq=76, lr=389, seed=2))
    ctx.plan()
    n = ctx.run()
    records = ctx.download()
    shares = [np.ascontiguousarray(records[records["frag"] % 10 == k]) for k in range(10)]
    fmt = b"%d\t" * 9 + b"\n"
    text_in = b"".join(fmt % t for t in zip(*(np.concatenate(shares)[f].tolist() for f in rec.FIELDS)))
    tmp = tempfile.mkdtemp(prefix="rec_throughput.")
    src, dst = os.path.join(tmp, "in.align"), os.path.join(tmp, "sorted.align")
    open(src, "wb").write(text_in)
    env = dict(os.environ, LC_ALL="C")

    def gnu_sort():
        subprocess.check_call(["sort", "-n", "-k", "1", "-o", dst, src], env=env)

    store = rec.Store(0)
    buf = np.empty(n * rec.MAX_LINE, np.uint8)
    got = ctypes.c_int64()
    host = np.zeros(n, dsa.RECORD_DTYPE)
    cnt = ctypes.c_int64()

    def device_arm():
        store.clear()
        for s in shares:
            store.append(s)
        t0 = time.perf_counter()
        store.sort()
        t1 = time.perf_counter()
        assert store.lib.rec_text(store.h, None, 0, buf.ctypes.data, len(buf), ctypes.byref(got)) == 0
        return t1 - t0, time.perf_counter() - t1

    def download():
        assert ctx.lib.dsa_download(ctx.h, host.ctypes.data, n, ctypes.byref(cnt)) == 0 and cnt.value == n

    device_arm()
    gnu_sort()
    assert buf[:got.value].tobytes() == open(dst, "rb").read(), "the store's text differs from sort's"
    keys = ("append_ms", "keys_ms", "sort_ms", "gather_ms", "format_ms", "write_ms", "download_ms")
    ev = {k: [] for k in keys}
    t_sort, t_text, t_down, t_gnu = [], [], [], []
    for rep in range(a.warmup + a.repeats):
        ts, tt = device_arm()
        tm = store.timing()
        t0 = time.perf_counter()
        download()
        t1 = time.perf_counter()
        timed = rep >= a.warmup
        if timed:
            t_sort.append(ts * 1e3)
            t_text.append(tt * 1e3)
            t_down.append((t1 - t0) * 1e3)
            for k in keys:
                ev[k].append(tm[k])
        if timed and (rep - a.warmup) % 4 == 0:
            t0 = time.perf_counter()
            download()
            gnu_sort()
            t_gnu.append((time.perf_counter() - t0) * 1e3)
    res = dict(records=int(n), shares=[len(s) for s in shares], text_bytes=int(got.value), n_sorts=int(tm["n_sorts"]),
               library=dsa.load_library().dsa_version().decode(), events_ms={k: stats(v) for k, v in ev.items()},
               rec_sort_host_clock_ms=stats(t_sort), rec_text_host_clock_ms=stats(t_text),
               sort_plus_text_ms=stats([x + y for x, y in zip(t_sort, t_text)]),
               dsa_download_ms=stats(t_down), dsa_download_gnu_sort_ms=stats(t_gnu),
               write_GB_per_s=got.value / (stats(ev["write_ms"])["median"] * 1e-3) / 1e9)
    print(json.dumps(res), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for p in (src, dst):
        os.unlink(p)
    os.rmdir(tmp)
    store.close()
    ctx.close()


if __name__ == "__main__":
    main()
