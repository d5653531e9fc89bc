"""calc_span_stats: the reference's Perl script, the host step of bin/defuse_glue, `defuse_glue span_stats` and the library route
(include/defuse_ptext.h, "span statistics") on one synthetic run.

    python profiles/span_stats/measure.py --clusters 10500 --json profiles/span_stats/result.json --keep DIR      # needs a GPU
    python profiles/span_stats/measure.py --clusters 10500 --json profiles/span_stats/result.json --perl DIR      # needs perl and the reference

The cluster file is what `remove_duplicates 5` leaves of the file of profiles/cluster_regions/measure.py (runs of 100-300 fragments
per cluster, a third of them PCR duplicates): it is clusters.sc.  The .break and .seq files are what ptext_format prints of a
prediction with one group per cluster, so the resident route (span_breaks_pred on that pred_ctx) and the text routes see the same
break positions; --keep writes the two small files to DIR, and --perl reads them from there on a machine that has the reference and
no GPU, regenerates the same cluster file and times the script and the host step.  Every comparison first checks that both sides
give the same bytes (the script: the same lines, its order is Perl's hash order).  Each part is timed --runs times on warm files;
median and range are written."""
import argparse
import importlib.util
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
SCRIPT = "/root/reference/scripts/calc_span_stats.pl"
MIN = 5


def stats(ts):
    return {"median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "n": len(ts)}


def timed(runs, fn):
    ts = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return stats(ts[1:])                                    # (the first run warms the files and the contexts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=10500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--keep", default=None, help="write splitreads.break and splitreads.seq here")
    ap.add_argument("--perl", default=None, help="time the script and the host step on the two files kept here; no GPU is used")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("cluster_regions_measure", os.path.join(ROOT, "profiles", "cluster_regions", "measure.py"))
    shape = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shape)
    generate = shape.generate                               # the input shape of profiles/cluster_regions/README.md
    tmp = tempfile.mkdtemp(prefix="span_stats_")
    P = lambda n: os.path.join(tmp, n)
    res = {}
    if args.json and os.path.exists(args.json):
        res = json.load(open(args.json))

    def save():
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)

    raw = generate(P("clusters.raw"), args.clusters)
    with open(P("clusters.raw"), "rb") as fin, open(P("clusters.sc"), "wb") as fout:
        subprocess.check_call([GLUE, "remove_duplicates", str(MIN)], stdin=fin, stdout=fout, env=dict(os.environ, DEFUSE_THREADS="16"))
    clusters = open(P("clusters.sc"), "rb").read()
    files = lambda b, s: ["-c", P("clusters.sc"), "-b", b, "-s", s]
    host_step = lambda b, s, out: subprocess.check_call([GLUE, "calc_span_stats"] + files(b, s), stdout=open(out, "wb"))

    if args.perl:
        brk, seq = os.path.join(args.perl, "splitreads.break"), os.path.join(args.perl, "splitreads.seq")
        assert res.get("input", {}).get("clusters_sc_bytes") == len(clusters), "the kept files are of another run"
        host_step(brk, seq, P("host.stats"))
        env = dict(os.environ, PERL_HASH_SEED="0")
        run_perl = lambda: subprocess.check_call(["perl", SCRIPT] + files(brk, seq), stdout=open(P("perl.stats"), "wb"), env=env)
        res["a_perl_script_build_container"] = timed(args.runs, run_perl)
        assert sorted(open(P("perl.stats"), "rb").read().splitlines()) == sorted(open(P("host.stats"), "rb").read().splitlines())
        res["a_perl_script_build_container"]["same_lines_as_the_host_step"] = True
        res["b_host_step_build_container"] = timed(args.runs, lambda: host_step(brk, seq, P("host.stats")))
        save()
        print(json.dumps(res, indent=1))
        return

    from defuse_amd import bat, clusterregions as cr, eval as ev, pred, ptext, spanstats as sp
    from tests.test_pred import Store, make_task
    from tests.test_ptext import groups_of
    ids = list(range(args.clusters))
    tasks = [make_task(i, b"ACGTNACGTACGTTGCA" * 20, b"acgtnacgttgcaacgt" * 20, start=(10000 + 37 * i, 50000 + 11 * i), strand=(i % 2, (i // 2) % 2),
                       name=("chr%d" % (1 + i % 24), "chr%d" % (1 + i % 7))) for i in ids]
    groups = groups_of(ev, [(i, 100 + i % 200, 30 + i % 250, 3, 1.0, 2.0, 0) for i in ids])
    res.update({"input": {"clusters": args.clusters, "raw_lines": raw.count(b"\n"), "clusters_sc_lines": clusters.count(b"\n"), "clusters_sc_bytes": len(clusters)},
                "min_cluster_size": MIN, "runs": args.runs, "a_perl_script": "not run on the GPU machine, which has no reference: see a_perl_script_build_container"})
    with Store(bat, pred, tasks) as S, ptext.Names.from_oracle(tasks) as N, ptext.Context(N) as T, cr.Context() as tc, sp.Context() as ctx:
        S.predict(groups)
        T.format(S.ctx)
        seq_text, brk_text, lines = T.fetch()
        assert not (lines["status"] != 0).any() and brk_text.count(b"\n") == 2 * args.clusters
        for name, data in (("splitreads.break", brk_text), ("splitreads.seq", seq_text)):
            for d in [tmp] + ([args.keep] if args.keep else []):
                os.makedirs(d, exist_ok=True)
                with open(os.path.join(d, name), "wb") as f:
                    f.write(data)
        res["input"].update(break_bytes=len(brk_text), seq_bytes=len(seq_text))
        brk, seq = P("splitreads.break"), P("splitreads.seq")
        # (b) the host step
        res["b_host_step"] = timed(args.runs, lambda: host_step(brk, seq, P("host.stats")))
        want = open(P("host.stats"), "rb").read()
        res["output"] = {"rows": want.count(b"\n"), "bytes": len(want)}
        save()
        # (c) the tool
        last = []

        def tool():
            p = subprocess.run([GLUE, "span_stats"] + files(brk, seq) + ["-o", P("tool.stats")], capture_output=True, text=True, env=dict(os.environ, DEFUSE_TIMING="1"))
            assert p.returncode == 0, p.stderr
            last[:] = p.stderr.strip().splitlines()
        res["c_tool_span_stats"] = timed(args.runs, tool)
        assert open(P("tool.stats"), "rb").read() == want
        res["c_tool_span_stats"].update(same_bytes_as_the_host_step=True, timing_lines_of_the_last_run=list(last))
        save()
        # (d) the resident route on warm contexts: the dedup text and the prediction are where their steps left them
        tc.begin()
        tc.add(np.frombuffer(raw, dtype=np.uint8))
        assert tc.dedup(MIN)["stop_kind"] == 0 and tc.fetch(cr.DEDUP) == clusters
        per_stage, out = [], []

        def resident():
            b = ctx.breaks_pred(S.ctx)
            r = ctx.stats(tc, sp.DEDUP)
            assert b["stop_kind"] == 0 and r["stop_kind"] == 0 and r["n_noncanonical"] == 0
            out[:] = [ctx.fetch()[1]]
            per_stage.append(ctx.timing())
        res["d_resident_breaks_pred_stats_fetch"] = timed(args.runs, resident)
        assert out[0] == want
        keys = [k for k in per_stage[0] if k.endswith("_ms")]
        res["d_resident_breaks_pred_stats_fetch"].update(same_bytes_as_the_host_step=True,
                                                         stage_ms_median={k: round(statistics.median(t[k] for t in per_stage[1:]), 3) for k in keys})
        # the same with the tables from the two files' text
        ctx.breaks_text(brk_text, seq_text)
        ctx.stats(tc, sp.DEDUP)
        assert ctx.fetch()[1] == want
        res["d_resident_breaks_pred_stats_fetch"]["breaks_text_stage_ms"] = {k: round(v, 3) for k, v in ctx.timing().items() if k in ("upload_ms", "lines_ms", "tables_ms")}
        save()
        # (e) the host route that (d) replaces: the dedup text down to a file, then the host step

        def host_route():
            with open(P("clusters.sc"), "wb") as f:
                f.write(tc.fetch(cr.DEDUP))
            host_step(brk, seq, P("route.stats"))
        res["e_host_route_fetch_dedup_text_then_host_step"] = timed(args.runs, host_route)
        assert open(P("route.stats"), "rb").read() == want
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
