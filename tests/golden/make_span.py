"""Generates tests/golden/span/: cluster, .break and .seq inputs and what the reference's scripts/calc_span_stats.pl printed for
them.  Run in the build container only (needs /root/reference and perl); the fixtures it writes are what travels.

    python tests/golden/make_span.py

The script's row order is Perl's hash order (PERL_HASH_SEED=0 here), so tests/test_span_stats.py compares rows as a set.  Every
key field of the inputs is plain decimal: there Perl's string keys and the library's int keys are the same keys."""
import os
import random
import shutil
import subprocess

REF = "/root/reference/scripts"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "span")
ENV = dict(os.environ, PERL_HASH_SEED="0", PERL_PERTURB_KEYS="0")


def cl(cid, ce, frag, strand, start, end, name="chr1", read_end=0):
    return "%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (cid, ce, frag, read_end, name, strand, start, end)


def example():
    """The issue's example: the last end-0 line makes end 0 a minus end for all three fragments, fragment 11 has one end."""
    clusters = cl(5, 0, 10, "+", 100, 149) + cl(5, 1, 10, "-", 300, 349) + cl(5, 0, 11, "+", 90, 139) + cl(5, 0, 12, "-", 95, 144) + cl(5, 1, 12, "-", 310, 359)
    return clusters, "5\t0\tchr1\t+\t160\n5\t1\tchr2\t-\t290\n", "5\tACGTACGT\t0\t3\t0.5\t0.25\n"


def random_files(seed, n_clusters=40):
    """Clusters of 1-12 fragments, now and then a fragment with one end, a (fragment, end) given again, a strand that changes
    inside an end, an id that comes back later, a negative id, ends {0, 2}, ids without a break entry (one of them with a
    single end), duplicates in the two small files, an inter length other than 0."""
    rng = random.Random(seed)
    ids = rng.sample(range(-3, 400), n_clusters)
    blocks, brk, seq = [], [], []
    for k, cid in enumerate(ids):
        ends = (0, 2) if k % 11 == 5 else (0, 1)
        base = [rng.randrange(1000, 90000), rng.randrange(1000, 90000)]
        strands = [rng.choice("+-"), rng.choice("+-")]
        lines = []
        for frag in rng.sample(range(1000), rng.randrange(1, 13)):
            for e in (0, 1):
                if rng.random() < 0.12 and len(lines) > 1:
                    continue                                # a fragment with one end (or, rarely, none)
                s = strands[e] if rng.random() < 0.9 else rng.choice("+-")
                a = base[e] + rng.randrange(300)
                lines.append(cl(cid, ends[e], frag, s, a, a + rng.randrange(30, 76), rng.choice(["chr1", "chrX", "G1|T2"]), e))
                if rng.random() < 0.1:
                    a = base[e] + rng.randrange(300)
                    lines.append(cl(cid, ends[e], frag, rng.choice("+-"), a, a + 49, "chr7", e))
        if {l.split("\t")[1] for l in lines} != {str(e) for e in ends}:
            lines.append(cl(cid, ends[1], 1000, strands[1], base[1], base[1] + 49))
            lines.append(cl(cid, ends[0], 1000, strands[0], base[0], base[0] + 49))
        no_break = k % 7 == 3
        if no_break and k % 14 == 3:
            lines = [l for l in lines if l.split("\t")[1] == str(ends[0])]          # one end only: skipped all the same
        half = len(lines) // 2 if k % 5 == 0 else len(lines)
        blocks.append("".join(lines[:half]))
        if half < len(lines):
            blocks.append(("late", "".join(lines[half:])))  # the rest of the id comes back later
        if not no_break:
            for e in (0, 1):
                if rng.random() < 0.2:
                    brk.append("%d\t%d\tchr9\t+\t%d\n" % (cid, ends[e], rng.randrange(1000, 90000)))    # an earlier entry, overwritten
                brk.append("%d\t%d\t%s\t%s\t%d\n" % (cid, ends[e], "chr1", strands[e], base[e] + rng.randrange(-100, 400)))
        if rng.random() < 0.2:
            seq.append("%d\tNNNN\t7\t1\t1\t1\n" % cid)
        seq.append("%d\t%s\t%d\t%d\t%g\t%g\n" % (cid, "".join(rng.choice("ACGT") for _ in range(rng.randrange(20, 200))), 0 if k % 4 else rng.randrange(-5, 40),
                                                rng.randrange(1, 30), rng.random() * 20, rng.random() * 20))
    early = [b for b in blocks if isinstance(b, str)]
    late = [b[1] for b in blocks if not isinstance(b, str)]
    rng.shuffle(late)
    rng.shuffle(brk)                                        # (an overwritten entry may now be the later one: either is a fixture)
    return "".join(early + late), "".join(brk), "".join(seq)


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)

    def put(name, text):
        with open(os.path.join(OUT, name), "w") as f:
            f.write(text)

    def perl(name, files):
        for kind, text in zip(("clusters", "break", "seq"), files):
            put("%s_%s.txt" % (name, kind), text)
        return subprocess.run(["perl", os.path.join(REF, "calc_span_stats.pl"), "-c", "%s_clusters.txt" % name, "-b", "%s_break.txt" % name, "-s", "%s_seq.txt" % name],
                              capture_output=True, text=True, env=ENV, cwd=OUT)

    for name, files in (("example", example()), ("random1", random_files(1)), ("random2", random_files(2, 90))):
        r = perl(name, files)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr)
        put("%s_stats.perl.txt" % name, r.stdout)
    # a cluster with a break entry and one cluster end: the script dies (what it printed before it did is hash order, and not kept)
    clusters, brk, seq = example()
    r = perl("one_end", (clusters + cl(9, 0, 1, "+", 10, 59) + cl(9, 0, 2, "+", 20, 69), brk + "9\t0\tchr1\t+\t100\n", seq + "9\tAC\t0\t1\t1\t1\n"))
    assert r.returncode != 0 and r.stderr, r
    put("one_end_stderr.perl.txt", r.stderr)
    put("one_end_status.perl.txt", "%d\n" % r.returncode)
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
