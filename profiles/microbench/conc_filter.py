"""The concordant-cluster filter (include/defuse_task.h, section "concordant clusters") on a seeded synthetic of about 20 000 clusters at R = 2000: the library's
stage times, and the host route it replaces on the same input, each step timed.

    python profiles/microbench/conc_filter.py --out result.json                 # library stages and bin/localalign (needs the GPU)
    python profiles/microbench/conc_filter.py --perl SCRIPTS_DIR --out perl.json  # the two Perl steps (needs the reference's scripts, no GPU)

The input is tests/concfilter_cases.random_case(20, ...): 5 contigs of about 1 Mb, 2000 genes, half of the clusters inside a gene.
The lines bin/localalign reads are rebuilt on the host from the library's descriptors (the clusters.sc.local.seq text in canonical
order); the Perl leg writes the script's own file.  profiles/conc_filter/README.md holds what was measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import concfilter_cases as cases      # noqa: E402

SCORES = dict(match=10, mismatch=-5, gap=-5, threshold=0.8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def build_case(n_clusters, zero_ok=False):
    return cases.random_case(20, n_clusters=n_clusters, n_contigs=5, n_genes=max(20, n_clusters // 10), contig_len=(900000, 1100000), zero_ok=zero_ok)


def perl_leg(case, scripts, seq_range):
    """prep_local_alignment_seqs.pl and filter_column.pl, wall seconds each (filter_column.pl over an empty values file: its
    time is reading and printing the cluster file)."""
    with tempfile.TemporaryDirectory() as tmp:
        for ext in ("fa", "gtf", "clusters"):
            with open(os.path.join(tmp, "in." + ext), "wb") as f:
                f.write(case[ext])
        t0 = time.perf_counter()
        with open(os.path.join(tmp, "local.seq"), "wb") as out:
            subprocess.run(["perl", os.path.join(scripts, "prep_local_alignment_seqs.pl"), "-r", os.path.join(tmp, "in.fa"), "-g", os.path.join(tmp, "in.gtf"),
                            "-c", os.path.join(tmp, "in.clusters"), "-s", str(seq_range)], stdout=out, check=True)
        t1 = time.perf_counter()
        open(os.path.join(tmp, "values"), "wb").close()
        with open(os.path.join(tmp, "in.clusters"), "rb") as f, open(os.devnull, "wb") as out:
            subprocess.run(["perl", os.path.join(scripts, "filter_column.pl"), os.path.join(tmp, "values"), "0", "1"], stdin=f, stdout=out, check=True)
        t2 = time.perf_counter()
        return dict(prep_local_alignment_seqs_s=t1 - t0, filter_column_s=t2 - t1, local_seq_bytes=os.path.getsize(os.path.join(tmp, "local.seq")),
                    local_seq_lines=sum(1 for _ in open(os.path.join(tmp, "local.seq"), "rb")), includes="BioPerl's index of the FASTA, built in the same run")


def device_leg(case, seq_range, reps, with_tool):
    from defuse_amd import clusterregions, concfilter as cf, task
    models, fasta = cf.read_gene_models(case["gtf"]), cf.read_fasta(case["fa"])
    out = dict(n_cluster_lines=case["clusters"].count(b"\n"), cluster_bytes=len(case["clusters"]), fasta_bytes=sum(len(s) for s in fasta.values()))
    t0 = time.perf_counter()
    ref = task.Reference(fasta)
    mod = cf.Models(models, list(fasta))
    out["one_time_reference_and_models_s"] = time.perf_counter() - t0
    runs = []
    with clusterregions.Context() as cl, cf.Context() as ctx:
        cl.begin()
        cl.add_pieces(case["clusters"])
        for _ in range(reps):
            w0 = time.perf_counter()
            r1 = ctx.targets(cl, mod, ref, seq_range)
            w1 = time.perf_counter()
            assert r1["stop_kind"] == 0, r1
            ctx.align(ref, **SCORES)
            w2 = time.perf_counter()
            r3 = ctx.filter()
            w3 = time.perf_counter()
            runs.append(dict(ctx.timing(), wall_targets_ms=1e3 * (w1 - w0), wall_align_ms=1e3 * (w2 - w1), wall_filter_ms=1e3 * (w3 - w2), wall_ms=1e3 * (w3 - w0)))
        out.update(n_clusters=r1["n_clusters"], n_targets=r1["n_targets"], n_kept_targets=r3["n_kept_targets"], n_hit_clusters=r3["n_hit_clusters"],
                   n_kept_lines=r3["n_kept_lines"], out_bytes=r3["out_bytes"])
        out["stages_median"] = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        out["runs"] = runs
        out["dp_gcups"] = out["stages_median"]["cells"] / (out["stages_median"]["dp_ms"] * 1e6)
        out["pack_share"] = out["stages_median"]["pack_ms"] / (out["stages_median"]["pack_ms"] + out["stages_median"]["dp_ms"])
        if with_tool:
            tg, names = ctx.fetch_targets(), list(fasta)
            align = ctx.fetch(cf.ALIGN_TEXT)
            t0 = time.perf_counter()
            lines = []
            for t in tg:
                a = fasta[names[t["seq"]]][t["start"]:t["start"] + t["len"]]
                b = fasta[names[t["other_seq"]]][t["other_start"]:t["other_start"] + t["other_len"]]
                lines.append(b"%d\t%s\t%s\n" % (t["cluster_id"], a[::-1].translate(COMP) if t["revcomp"] else a, b[::-1].translate(COMP) if t["other_rev"] else b))
            text = b"".join(lines)
            out["local_seq_bytes"] = len(text)
            out["rebuild_local_seq_s"] = time.perf_counter() - t0
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "local.seq")
                with open(path, "wb") as f:
                    f.write(text)
                walls = []
                for _ in range(2):
                    with open(path, "rb") as f:
                        t0 = time.perf_counter()
                        done = subprocess.run([os.path.join(ROOT, "bin", "localalign"), "-m", "10", "-x", "-5", "-g", "-5", "-t", "0.8"], stdin=f,
                                              capture_output=True, check=True, timeout=600)
                        walls.append(time.perf_counter() - t0)
                out["bin_localalign_s"] = walls
                out["tool_text_equals_library_text"] = done.stdout == align
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=20000)
    ap.add_argument("--range", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--perl", help="the reference's scripts directory: time the two Perl steps instead")
    ap.add_argument("--no-tool", action="store_true")
    ap.add_argument("--zero-ok", action="store_true", help="keep extents that end at 0: subseq makes them whole contigs (stop ||= length)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    t0 = time.perf_counter()
    case = build_case(a.clusters, a.zero_ok)
    res = dict(clusters_asked=a.clusters, zero_ok=a.zero_ok, seq_range=a.range, build_case_s=time.perf_counter() - t0)
    res.update(perl_leg(case, a.perl, a.range) if a.perl else device_leg(case, a.range, a.reps, not a.no_tool))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}, indent=1))


if __name__ == "__main__":
    main()
