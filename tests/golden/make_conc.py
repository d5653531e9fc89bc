"""Generates tests/golden/conc/: a FASTA, a GTF and cluster files, and what the reference's scripts printed for them.  Run in
the build container only (needs /root/reference and perl); the fixtures it writes are what travels.

    python tests/golden/make_conc.py

  <case>.fa / .gtf / .clusters      the inputs (`edges` and `random1` share nothing; `one_end` and `missing_other` are cluster
                                    files over the FASTA and GTF of `edges`)
  <case>.R<range>.seq.perl.txt      prep_local_alignment_seqs.pl -s <range>, its lines sorted (their order is Perl's hash order)
  <case>.R<range>.align.txt         tests/concfilter_oracle.py's local.align text over Perl's lines in canonical order: the
                                    reference's localalign needs Boost and cannot be built here, so the scores come from
                                    oracle/localalign_oracle.py (-m 10 -x -5 -g -5 -t 0.8)
  <case>.R<range>.filtered.perl.txt filter_column.pl <align> 0 1 over the cluster file
  <case>.status.perl.txt            the script's exit status (the two cases it dies on), .stderr.perl.txt what it said (the scripts' directory
                                    written as SCRIPTS, the temporary one as TMP)

BioPerl writes an index beside the FASTA, so the scripts run on copies in a temporary directory."""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import concfilter_oracle as oracle           # noqa: E402
from tests.concfilter_cases import edges_case, one_end_case, missing_other_case, random_case      # noqa: E402
from defuse_amd import concfilter                       # noqa: E402

REF = "/root/reference/scripts"
OUT = os.path.join(HERE, "conc")
ENV = dict(os.environ, PERL_HASH_SEED="0", PERL_PERTURB_KEYS="0")


def perl_seq(tmp, name, seq_range):
    return subprocess.run(["perl", os.path.join(REF, "prep_local_alignment_seqs.pl"), "-r", os.path.join(tmp, name + ".fa"), "-g",
                           os.path.join(tmp, name + ".gtf"), "-c", os.path.join(tmp, name + ".clusters"), "-s", str(seq_range)],
                          capture_output=True, env=ENV, cwd=tmp)


README = """Fixtures of tests/test_conc_filter.py, written by tests/golden/make_conc.py: data only.

The inputs (`*.fa`, `*.gtf`, `*.clusters`) are synthetic (tests/concfilter_cases.py).  `*.seq.perl.txt` is what the reference's
`prep_local_alignment_seqs.pl` printed for them, its lines sorted (their order is Perl's hash order); `*.filtered.perl.txt` is
what its `filter_column.pl ALIGN 0 1` printed; `*.status.perl.txt` / `*.stderr.perl.txt` record the two inputs the script dies
on.  `*.align.txt` is NOT the reference's: its `localalign` needs Boost and cannot be built where the fixtures were made, so
the local.align text comes from oracle/localalign_oracle.py (-m 10 -x -5 -g -5 -t 0.8) over Perl's lines in canonical order.
"""


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    with open(os.path.join(OUT, "README.md"), "w") as f:
        f.write(README)
    cases = [("edges", edges_case(), (40, 130)), ("random1", random_case(1), (40,)), ("one_end", one_end_case(), (40,)),
             ("missing_other", missing_other_case(), (40,))]
    with tempfile.TemporaryDirectory() as tmp:
        for name, case, ranges in cases:
            for ext in ("fa", "gtf", "clusters"):
                for d in (tmp, OUT):
                    if d == OUT and ext != "clusters" and name in ("one_end", "missing_other"):
                        assert case[ext] == cases[0][1][ext]    # (the inputs of `edges`, committed once)
                        continue
                    with open(os.path.join(d, "%s.%s" % (name, ext)), "wb") as f:
                        f.write(case[ext])
            models, fasta = concfilter.read_gene_models(case["gtf"]), concfilter.read_fasta(case["fa"])
            for r in ranges:
                got = perl_seq(tmp, name, r)
                stem = os.path.join(OUT, "%s.R%d" % (name, r))
                if got.returncode != 0:
                    with open(os.path.join(OUT, name + ".status.perl.txt"), "w") as f:
                        f.write("%d\n" % got.returncode)
                    with open(os.path.join(OUT, name + ".stderr.perl.txt"), "wb") as f:
                        f.write(got.stderr.replace(tmp.encode(), b"TMP").replace(REF.encode(), b"SCRIPTS"))
                    continue
                lines = sorted(got.stdout.split(b"\n")[:-1])
                with open(stem + ".seq.perl.txt", "wb") as f:
                    f.write(b"".join(l + b"\n" for l in lines))
                tg = oracle.targets(models, fasta, case["clusters"], r)
                assert sorted(oracle.target_lines(tg)) == [l + b"\n" for l in lines], (name, r)
                align = oracle.local_align(tg, 10, -5, -5, 0.8)[0]
                with open(stem + ".align.txt", "wb") as f:
                    f.write(align)
                with open(os.path.join(tmp, "align"), "wb") as f:
                    f.write(align)
                with open(os.path.join(tmp, name + ".clusters"), "rb") as f:
                    done = subprocess.run(["perl", os.path.join(REF, "filter_column.pl"), os.path.join(tmp, "align"), "0", "1"], stdin=f,
                                          capture_output=True, env=ENV, check=True)
                with open(stem + ".filtered.perl.txt", "wb") as f:
                    f.write(done.stdout)
                print(name, r, len(lines), "target lines,", align.count(b"\n"), "printed,", done.stdout.count(b"\n"), "of", case["clusters"].count(b"\n"),
                      "cluster lines kept")


if __name__ == "__main__":
    main()
