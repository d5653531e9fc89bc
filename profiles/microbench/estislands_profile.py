"""estislands end to end on a synthetic intronEst-shaped table: writes the inputs (tests/estislands_oracle.py's generators),
runs bin/estislands with DEFUSE_TIMING=1 and records wall time, the stage split, sizes and, with --check, whether the output
equals the oracle's byte for byte.  The inputs stay in --dir for a profiler run of the same command.

    python profiles/microbench/estislands_profile.py --est 5000000 --breaks 100000 --dir /tmp/est --out est.json --check"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import estislands_oracle as eo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--est", type=int, default=5_000_000)
    ap.add_argument("--breaks", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default="/tmp/estislands_profile")
    ap.add_argument("--out", required=True)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    rng = np.random.default_rng(a.seed)
    t = time.time()
    c, ts, te = eo.segment_columns(rng, a.est, span=250_000_000, degenerate=0.0005)
    est_data = eo.est_table(rng, c, ts, te)
    cat = eo.catalog(eo.read_ests(est_data)) if a.check else None
    if cat is None:                                  # queries need islands: those of a sample are close enough for a profile
        cat = eo.catalog(eo.read_ests(eo.est_table(rng, c[:200_000], ts[:200_000], te[:200_000])))
    qc, qs, qe = eo.queries_near(rng, cat, eo.CHROMS, a.breaks, span=250_000_000)
    brk_data = eo.break_psl(rng, qc, qs, qe)
    est, brk, out = (os.path.join(a.dir, x) for x in ("est.txt", "breaks.psl", "out.psl"))
    for p, data in ((est, est_data), (brk, brk_data)):
        with open(p, "wb") as f:
            f.write(data)
    gen_s = time.time() - t
    runs = []
    for _ in range(a.runs):
        t = time.time()
        r = subprocess.run([os.path.join(ROOT, "bin", "estislands"), "-e", est, "-b", brk, "-o", out], capture_output=True, text=True,
                           env=dict(os.environ, DEFUSE_TIMING="1"), timeout=600)
        wall = time.time() - t
        assert r.returncode == 0, r.stderr
        stages = {m.group(1): float(m.group(2)) for m in re.finditer(r"\[estislands\] (read\+parse|catalogue|lookup|write) ([0-9.e-]+) s", r.stderr)}
        runs.append({"wall_s": round(wall, 4), "stages_s": stages, "stderr": r.stderr})
    got = open(out, "rb").read()
    res = {"est_rows": a.est, "break_rows": a.breaks, "seed": a.seed, "est_bytes": len(est_data), "break_bytes": len(brk_data),
           "degenerate_rows": int((te < ts + 1).sum()), "threads": os.environ.get("DEFUSE_THREADS", "default (8)"),
           "generate_s": round(gen_s, 2), "output_lines": got.count(b"\n"), "output_md5": hashlib.md5(got).hexdigest(), "runs": runs}
    if a.check:
        want = eo.run(est_data, brk_data)
        res["equals_oracle"] = want == (got, "", 0)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    for r in runs:
        print(r["wall_s"], r["stages_s"])
    if a.check and not res["equals_oracle"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
