"""Generates tests/golden/cluster_regions/: cluster files with what tests/golden/glue/ lacks, and the outputs of the
reference's own scripts/remove_duplicates.pl and scripts/get_align_regions.pl on them.  Run in the build container only (needs
/root/reference and perl); the fixtures it writes are what travels.

    python tests/golden/make_cluster_regions.py

Every file has
  - a (fragment, cluster end) that occurs twice in a cluster (the later line is the one both scripts keep),
  - a cluster id that comes back in a non-adjacent run (remove_duplicates.pl treats it as a new cluster, get_align_regions.pl
    as the same one),
  - reference name and strand that differ between the lines of one (cluster, end).
Both scripts print in Perl's hash order (PERL_HASH_SEED=0 here); tests/test_cluster_regions.py compares order-free, as
tests/test_glue.py does."""
import os
import random
import shutil
import subprocess

REF = "/root/reference/scripts"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cluster_regions")
ENV = dict(os.environ, PERL_HASH_SEED="0", PERL_PERTURB_KEYS="0")
MIN_SIZE = 2


def perl(script, args=(), stdin=None):
    r = subprocess.run(["perl", os.path.join(REF, script)] + list(args), input=stdin, capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (script, r.stderr)
    return r.stdout


def run_lines(rng, cid, frag0):
    """One run of lines of cluster `cid`: 2-8 fragments from frag0 on, PCR duplicates, and the three things of the docstring."""
    names = [rng.choice(["chr1", "chr2", "ENSG01|ENST07"]), rng.choice(["chr3", "chrX"])]
    strands = [rng.choice("+-"), rng.choice("+-")]
    base = [rng.randrange(1000, 90000), rng.randrange(1000, 90000)]
    lines, pos, frags = [], [], []
    for k in range(rng.randrange(2, 9)):
        pair = rng.choice(pos) if pos and rng.random() < 0.4 else (base[0] + rng.randrange(200), base[1] + rng.randrange(200))
        pos.append(pair)
        frags.append(frag0 + k)
        for e in (0, 1):
            name = names[e] if rng.random() < 0.8 else names[e] + "_alt"          # differs between lines of one (cluster, end)
            strand = strands[e] if rng.random() < 0.8 else "+-"[strands[e] == "+"]
            lines.append("%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (cid, e, frag0 + k, rng.randrange(2), name, strand, pair[e], pair[e] + 49))
    for _ in range(rng.randrange(1, 3)):                                          # a (fragment, end) again, elsewhere: the later line wins
        e = rng.randrange(2)
        at = base[e] + rng.randrange(200)
        lines.append("%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (cid, e, rng.choice(frags), rng.randrange(2), names[e], strands[e], at, at + 49))
    return lines


def cluster_file(seed):
    rng = random.Random(seed)
    ids = [4, 0, 9, 4, 2, 11, 0, 7, 9, 30, 5]                                     # 4, 0 and 9 come back
    lines, frag = [], rng.randrange(1000)
    for cid in ids:
        run = run_lines(rng, cid, frag)
        frag += 10
        lines += run
    return "".join(lines)


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for seed in (1, 2):
        text = cluster_file(seed)
        for name, data in (("clusters%d_in.txt" % seed, text), ("clusters%d_dedup.perl.txt" % seed, perl("remove_duplicates.pl", [str(MIN_SIZE)], stdin=text)),
                           ("clusters%d_regions.perl.txt" % seed, perl("get_align_regions.pl", stdin=text))):
            with open(os.path.join(OUT, name), "w") as f:
                f.write(data)
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
