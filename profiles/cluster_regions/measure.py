"""remove_duplicates + get_align_regions: the two host steps of bin/defuse_glue against `defuse_glue cluster_regions` and the
library route (include/defuse_task.h, "cluster text") on one synthetic cluster file.

    python profiles/cluster_regions/measure.py --clusters 10500 --json profiles/cluster_regions/result.json

The file has the shape of setcover's output in profiles/microbench/e2e_scale.py (runs of 100-300 fragments per cluster, two lines
per fragment, a third of the fragments PCR duplicates); --clusters sets its size.  Every comparison first checks that both sides
give the same bytes.  Each part is timed --runs times on warm files; median and range are written."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GLUE = os.path.join(ROOT, "bin", "defuse_glue")
MIN = 5


def generate(path, n_clusters, seed=7):
    rng = np.random.default_rng(seed)
    frag, parts = 0, []
    for cid in range(n_clusters):
        n = int(rng.integers(100, 301))
        chrom = rng.integers(1, 25, size=2)
        base = rng.integers(10000, 50_000_000, size=2)
        strand = [b"+-"[int(s):][:1] for s in rng.integers(0, 2, size=2)]
        off = rng.integers(0, 150, size=(n, 2))
        dup = rng.random(n) < 0.33
        off[1:][dup[1:]] = off[:-1][dup[1:]]                  # the pair of the fragment in front
        for k in range(n):
            for e in (0, 1):
                a = int(base[e] + off[k, e])
                parts.append(b"%d\t%d\t%d\t%d\tchr%d\t%s\t%d\t%d\n" % (cid, e, frag + k, e, chrom[e], strand[e], a, a + 149))
        frag += n
    data = b"".join(parts)
    with open(path, "wb") as f:
        f.write(data)
    return data


def stats(ts):
    return {"median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="cluster_regions_")
    P = lambda n: os.path.join(tmp, n)
    data = generate(P("clusters.sc"), args.clusters)
    res = {"input": {"clusters": args.clusters, "lines": data.count(b"\n"), "bytes": len(data)}, "min_cluster_size": MIN, "runs": args.runs}

    def save():
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)

    env16 = dict(os.environ, DEFUSE_THREADS="16")
    host = "%s remove_duplicates %d < %s > %s && %s get_align_regions < %s > %s" % (GLUE, MIN, P("clusters.sc"), P("h.nodup"), GLUE, P("h.nodup"), P("h.regions"))
    ts = []
    for _ in range(args.runs + 1):
        t0 = time.perf_counter()
        subprocess.check_call(host, shell=True, env=env16)
        ts.append(time.perf_counter() - t0)
    res["host_two_steps_16_threads"] = stats(ts[1:])
    res["output"] = {"nodup_bytes": os.path.getsize(P("h.nodup")), "regions_bytes": os.path.getsize(P("h.regions"))}
    save()

    ts, stages = [], []
    for _ in range(args.runs + 1):
        t0 = time.perf_counter()
        p = subprocess.run([GLUE, "cluster_regions", str(MIN), "-c", P("g.nodup"), "-r", P("g.regions"), P("clusters.sc")], capture_output=True, text=True,
                           env=dict(os.environ, DEFUSE_TIMING="1"))
        ts.append(time.perf_counter() - t0)
        assert p.returncode == 0, p.stderr
        stages.append(p.stderr.strip().splitlines())
    assert open(P("g.nodup"), "rb").read() == open(P("h.nodup"), "rb").read() and open(P("g.regions"), "rb").read() == open(P("h.regions"), "rb").read()
    res["tool_cluster_regions"] = dict(stats(ts[1:]), same_bytes_as_the_host_steps=True, timing_lines_of_the_last_run=stages[-1])
    save()

    from defuse_amd import clusterregions as cr, sctext, tasktext as tt
    arr = np.frombuffer(data, dtype=np.uint8)
    seq_names = [b"chr%d" % k for k in range(1, 25)]
    exon_text = b"G\tT\tchr1\t+\t1\t100\n"
    nodup, regions = open(P("h.nodup"), "rb").read(), open(P("h.regions"), "rb").read()
    with cr.Context() as ctx:
        per_stage, walls = [], []
        for _ in range(args.runs + 1):
            t0 = time.perf_counter()
            ctx.begin()
            ctx.add(arr)
            d = ctx.dedup(MIN)
            r = ctx.regions(cr.DEDUP)
            walls.append(time.perf_counter() - t0)
            per_stage.append(ctx.timing())
        assert ctx.fetch(cr.DEDUP) == nodup and ctx.fetch(cr.REGIONS) == regions
        keys = [k for k in per_stage[0] if k.endswith("_ms")]
        res["library_from_host_text"] = dict(stats(walls[1:]), result=dict(d, n_clusters=r["n_clusters"]),
                                             stage_ms_median={k: round(statistics.median(t[k] for t in per_stage[1:]), 3) for k in keys})
        save()

        # the resident route against the host route, from a cover's output in device memory to the pairs of a taskt_ctx
        with sctext.SctContext() as cover, tt.Context() as into, tt.Names([b"chr1"]) as rn, tt.Names(seq_names) as sn:
            cover.begin()
            cover.add(arr)
            cres = cover.cover(1)
            assert cres["status"] == sctext.OK and cres["out_bytes"] == len(data)          # disjoint clusters: everything is kept
            into.parse_exons(rn, exon_text)
            resident, hostroute = [], []
            for _ in range(args.runs + 1):
                t0 = time.perf_counter()
                ctx.begin()
                ctx.add_cover(cover)
                ctx.dedup(MIN)
                ctx.regions(cr.DEDUP)
                a = ctx.parse_regions(into, sn)
                resident.append(time.perf_counter() - t0)
                pa = into.pairs()[0].tobytes()
                t0 = time.perf_counter()
                with open(P("clusters.sc.fetched"), "wb") as f:
                    f.write(cover.fetch())
                subprocess.check_call(host.replace(P("clusters.sc") + " ", P("clusters.sc.fetched") + " "), shell=True, env=env16)
                b = into.parse_regions(sn, open(P("h.regions"), "rb").read())
                hostroute.append(time.perf_counter() - t0)
                assert a == b and pa == into.pairs()[0].tobytes()
            res["resident_route_add_cover_to_parse_regions"] = stats(resident[1:])
            res["host_route_fetch_two_steps_parse_regions"] = stats(hostroute[1:])
            res["pairs"] = a["n_items"]
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
