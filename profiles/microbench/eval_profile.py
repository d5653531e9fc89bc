"""profiles/eval: the evaluation of BASELINE configs[1]'s records on the device against the split-read step that made them and
against the host evaluator.

    python profiles/microbench/eval_profile.py --out profiles/eval/device_1M.json       # device time, dsa step, host side
    python profiles/microbench/eval_profile.py --tool --out profiles/eval/tool_540k.json  # evalsplitalign with / without DEFUSE_EVAL_GPU
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/microbench/eval_profile.py --calls 5    # kernel shares, its own run

The host side is profiles/microbench/eval_host (built from eval_host.cpp with g++, see its head comment)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def device_side(args):
    import numpy as np
    from defuse_amd import dsa, synth
    from defuse_amd import eval as ev
    ref, fus, reads, pairs = synth.make_batch(10000, 100, lq=76, lr=389, seed=2)
    ctx = dsa.Context(0)
    ctx.upload(ref, fus, reads, pairs)
    steps = []
    for _ in range(5):                                   # bench.py's step: plan + run
        ctx.plan()
        n = ctx.run()
        t = ctx.timing()
        steps.append(t.plan_ms + t.total_ms)
    hip = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = ctypes.CDLL(line.split()[-1])
            break
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), n * 40) == 0
    assert ctx.records_to_device(dev.value, n) == n
    ectx = ev.Context(0)
    groups, kept = ectx.evaluate_device(dev.value, n)    # sizes, and warm-up
    for _ in range(3):
        ectx.evaluate_device(dev.value, n, group_cap=len(groups), kept_cap=len(kept))
    device_ms, download_ms, wall_ms = [], [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        ectx.evaluate_device(dev.value, n, group_cap=len(groups), kept_cap=len(kept))
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        t = ectx.timing()
        device_ms.append(t["device_ms"])
        download_ms.append(t["download_ms"])
    counts = {k: v for k, v in ectx.timing().items() if k.startswith("n_")}
    downloads = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = ctx.download()
        downloads.append((time.perf_counter() - t0) * 1e3)
    hip.hipFree(dev)
    out = dict(records=int(n), counts=counts, calls=args.calls,
               eval_device_ms_median=statistics.median(device_ms), eval_device_ms_all=device_ms,
               eval_download_ms_median=statistics.median(download_ms),
               eval_call_wall_ms_median=statistics.median(wall_ms),
               dsa_step_ms_median=statistics.median(steps), dsa_step_ms_all=steps,
               dsa_download_ms_median=statistics.median(downloads), dsa_download_ms_all=downloads)
    host = os.path.join(ROOT, "profiles", "microbench", "eval_host")
    if os.path.exists(host) and not args.no_host:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "records.bin")
            got.tofile(path)
            for threads in (16, 1):
                txt = subprocess.run([host, path, str(threads), "7"], capture_output=True, text=True, check=True).stdout
                ms = [float(l.split()[1]) for l in txt.splitlines()]
                out["host_eval_ms_%d_threads" % threads] = dict(median=statistics.median(ms), all=ms)
                out["host_eval_kept"] = int(txt.splitlines()[0].split()[7])
    ectx.close()
    ctx.close()
    return out


def tool_side(args):
    import pathlib
    from tests.eval_case import generated_case
    tool = os.path.join(ROOT, "bin", "evalsplitalign")
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        case, lines = generated_case(tmp, 2700)
        align = str(tmp / "big.align")
        open(align, "w").write("".join(lines))
        out = dict(lines=len(lines), bytes=os.path.getsize(align), runs=[])
        files = {}
        for rep in range(3):
            for mode in ("host", "gpu"):
                env = {k: v for k, v in os.environ.items() if k != "DEFUSE_EVAL_GPU"}
                env.update(DEFUSE_TIMING="1", DEFUSE_THREADS="16")
                if mode == "gpu":
                    env["DEFUSE_EVAL_GPU"] = "1"
                t0 = time.perf_counter()
                out_prefix = str(tmp / mode)
                cmd = [tool, "-f", case["fasta"], "-e", case["exons"], "-u", str(case["ufrag"]), "-s", str(case["sfrag"]), "-n", str(case["minread"]),
                       "-x", str(case["maxread"]), "-r", case["regions"], "-a", align, "-q", out_prefix + ".seq", "-b", out_prefix + ".break",
                       "-p", out_prefix + ".predalign"]
                r = subprocess.run(cmd, capture_output=True, text=True, env=env)
                wall = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr
                files[mode] = tuple(open(str(tmp / mode) + "." + x).read() for x in ("seq", "break", "predalign"))
                out["runs"].append(dict(mode=mode, wall_s=wall, stderr=[l for l in r.stderr.splitlines() if l.startswith("[evalsplitalign]")]))
        out["identical_files"] = files["host"] == files["gpu"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--tool", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    out = tool_side(args) if args.tool else device_side(args)
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
