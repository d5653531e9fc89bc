"""calccov: the drop-in binary against oracle/calccov_oracle.py; the oracle's restatement of glibc's
rand() against the platform's libc."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "calccov")


@pytest.fixture(scope="module")
def tools(built):
    from defuse_amd import build
    build.build_tools()
    return True


def make_case(d, seed=3, n_genes=40, n_frag=3000, rl=50):
    """Exon table with single- and multi-transcript genes, and a concordant SAM of paired alignments on `gene|transcript`
    references (two records per fragment), some on transcripts that are not sampled, some with flag-named read ends."""
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    tx = []
    with open(os.path.join(d, "cdna.regions"), "w") as f:
        for g in range(n_genes):
            gene = "ENSG%05d" % int(rng.integers(0, 99999))
            for t in range(1 if g % 3 else 2):
                name = "ENST%05d" % (g * 10 + t)
                exons, pos = [], int(rng.integers(1000, 50000))
                for _ in range(int(rng.integers(1, 5))):
                    ln = int(rng.integers(200, 1500))
                    exons.append((pos, pos + ln - 1))
                    pos += ln + int(rng.integers(100, 3000))
                f.write("\t".join([gene, name, "chr%d" % (1 + g % 5), "+-"[g % 2]] + [str(x) for e in exons for x in e]) + "\t\n")
                tx.append((gene + "|" + name, sum(e - b + 1 for b, e in exons)))
        f.write("short\tline\n\n")
    lines = ["@HD\tVN:1.0", "@SQ\tSN:x\tLN:1"]
    for fr in range(n_frag):
        ref, ln = tx[int(rng.integers(0, len(tx)))]
        flen = int(rng.normal(200, 30))
        if ln < flen + 10:
            continue
        s = int(rng.integers(1, ln - flen))
        a = (s, 0), (s + flen - rl, 16)
        if fr % 2:
            a = a[::-1]
        for k, (pos, flag) in enumerate(a):
            qname = "%d/%d" % (fr, k + 1) if fr % 7 else "frag%d" % fr
            fl = flag if fr % 7 else flag | (0x40 if k == 0 else 0x80)
            lines.append("%s\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t%s" % (qname, fl, ref, pos, rl, "A" * rl, "I" * rl))
    with open(os.path.join(d, "cdna.pair.sam"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return os.path.join(d, "cdna.pair.sam"), os.path.join(d, "cdna.regions")


def run_tool(sam, regions, out, density="0.01", anchor="4", trim="50", extra=(), env=None):
    return subprocess.run([TOOL, "-c", sam, "-g", regions, "-l", out + ".len", "-p", out + ".pos", "-m", out + ".min", "-d", density,
                           "-a", anchor, "-t", trim] + list(extra), capture_output=True, text=True,
                          env=dict(os.environ, **env) if env else None)


def test_glibc_rand_restatement_equals_libc():
    from oracle import calccov_oracle as c
    libc = ctypes.CDLL("libc.so.6")
    for seed in (11, 1, 0, 12345, 2 ** 31 + 5):
        libc.srand(seed)
        g = c.GlibcRand(seed)
        assert [libc.rand() for _ in range(2000)] == [g.rand() for _ in range(2000)]


def test_oracle_shapes(tmp_path):
    from oracle import calccov_oracle as c
    sam, regions = make_case(str(tmp_path))
    ln, pos, mn = c.calccov(sam, regions, 0.01, 4, 50)
    assert len(ln.splitlines()) > 100 and len(pos.splitlines()) == len(mn.splitlines()) > 100
    ln2, pos2, _ = c.calccov(sam, regions, 0.01, 4, 50, multiexon=True)
    assert len(ln2.splitlines()) > len(ln.splitlines())                 # multi-transcript genes are sampled too
    vals = [float(l.split("\t")[1]) for l in pos.splitlines()]
    assert 0.0 <= min(vals) and max(vals) <= 1.0


def test_cli_and_errors(tools, tmp_path):
    r = subprocess.run([TOOL, "-c", "x"], capture_output=True, text=True)
    assert r.returncode == 1 and "One or more required arguments missing!" in r.stderr
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True)
    assert "Calculate covariance stats from concordant alignments" in r.stdout and "--multiexon" in r.stdout
    sam, regions = make_case(str(tmp_path))
    bad = tmp_path / "bad.sam"
    lines = open(sam).read().splitlines()
    bad.write_text("\n".join(lines[:40] + [lines[40]] + lines[40:]) + "\n")      # three alignments for one fragment
    r = run_tool(str(bad), regions, str(tmp_path / "o"))
    assert r.returncode == 1 and "Error: expected 2 alignments per fragment" in r.stderr and "retrieved 3 alignments for" in r.stderr
    r = run_tool(sam, str(tmp_path / "nope"), str(tmp_path / "o"))
    assert r.returncode == 1 and "Error: Unable to gene transcripts file" in r.stderr
    # no fragment on a sampled transcript: three empty files, no GPU needed
    empty = tmp_path / "none.sam"
    empty.write_text("@HD\tVN:1.0\nq/1\t0\tother|tx\t5\t255\t50M\t*\t0\t0\t%s\t*\nq/2\t16\tother|tx\t200\t255\t50M\t*\t0\t0\t%s\t*\n" % ("A" * 50, "A" * 50))
    r = run_tool(str(empty), regions, str(tmp_path / "e"))
    assert r.returncode == 0, r.stderr
    assert all(os.path.getsize(str(tmp_path / "e") + x) == 0 for x in (".len", ".pos", ".min"))


@pytest.mark.gpu
@pytest.mark.parametrize("multiexon,threads", [(False, None), (True, "5"), (False, "64")])
def test_tool_matches_oracle(tools, tmp_path, multiexon, threads):
    from oracle import calccov_oracle as c
    sam, regions = make_case(str(tmp_path), seed=4, n_frag=6000)
    exp = c.calccov(sam, regions, 0.01, 4, 50, multiexon=multiexon)
    out = str(tmp_path / "cov")
    r = run_tool(sam, regions, out, extra=["--multiexon"] if multiexon else [], env={"DEFUSE_THREADS": threads} if threads else None)
    assert r.returncode == 0, r.stderr
    assert (open(out + ".len").read(), open(out + ".pos").read(), open(out + ".min").read()) == exp
    assert len(exp[0].splitlines()) > 200


# ---- the NaN lines: an anchored range of 0 or 1 bases ---------------------------------------------------------------------

def test_oracle_prints_every_nan_as_the_reference_does():
    from oracle import calccov_oracle as c
    nan = float("nan")
    assert c._fmt(nan) == "-nan" and c._fmt(-nan) == "-nan" and c._fmt(c._div(0.0, 0.0)) == "-nan"
    assert c._fmt(0.5) == "0.5" and c._fmt(0.0) == "0" and c._fmt(1.0) == "1"


@pytest.mark.parametrize("rl", [50, 51])
def test_oracle_nan_lines(tmp_path, rl):
    """Reads of 2 x anchor bases have an anchored range of 0 (one position, 0/0 in both files), reads of 2 x anchor + 1 a
    range of 1 (two positions, 0/1 and 1/1 in the split positions, 0/floor(0.5) in the split minimums)."""
    from oracle import calccov_oracle as c
    sam, regions = make_case(str(tmp_path), seed=5, n_genes=12, n_frag=1500, rl=rl)
    ln, pos, mn = c.calccov(sam, regions, 0.05, 25, 50)
    assert len(mn.splitlines()) == len(pos.splitlines()) > 20 and "nan" not in ln
    assert all(l.endswith("\t-nan") for l in mn.splitlines())
    if rl == 50:
        assert all(l.endswith("\t-nan") for l in pos.splitlines())
    else:
        assert {l.split("\t")[1] for l in pos.splitlines()} == {"0", "1"}


@pytest.mark.gpu
@pytest.mark.parametrize("rl", [50, 51])
def test_tool_nan_lines(tools, tmp_path, rl):
    """The same two inputs through the tool: the NaN lines are "-nan" whatever sign the device's division left, the length
    samples are untouched by it."""
    from oracle import calccov_oracle as c
    sam, regions = make_case(str(tmp_path), seed=5, n_genes=12, n_frag=1500, rl=rl)
    exp = c.calccov(sam, regions, 0.05, 25, 50)
    out = str(tmp_path / "cov")
    r = run_tool(sam, regions, out, density="0.05", anchor="25")
    assert r.returncode == 0, r.stderr
    got = (open(out + ".len").read(), open(out + ".pos").read(), open(out + ".min").read())
    assert got == exp
    assert "\t-nan\n" in got[2] and ("\t-nan\n" in got[1]) == (rl == 50) and len(got[0].splitlines()) > 20 and "nan" not in got[0]


# ---- the kernel itself (include/defuse_cov.h through defuse_amd/cov.py) against the oracle's sample_batch -----------------

RANGES = (-1, 0, 1, 2, 3, 46)                  # end - start + 1 - 2 x anchor: empty below 0, 0/0 at 0, x/floor(0.5) at 1
ANCHORS = (0, 4, 25)
TRIMS = (0, 50, 1000)                          # 1000: unseqStart > unseqEnd, no length sample at all
COUNTS = (1, 255, 256, 257, 513)               # around one block of 256 lanes, and more than two


def cov_samples():
    """Three transcripts: 0 without a sample, 1 with one (position 30), 2 of 120 bases with every position sampled, in no
    order, and four positions twice."""
    rng = np.random.default_rng(8)
    pos2 = list(range(1, 121)) + [10, 10 + 47, 57, 120]
    rng.shuffle(pos2)
    pos = [30] + pos2
    return [0, 0, 1, len(pos)], pos


def cov_fragments(n, anchor):
    """n fragments whose two reads run through RANGES independently of each other; on transcript 2 mostly, every 7th on
    transcript 1 and every 11th on transcript 0; the second read equal to the first, in front of it, behind it, or apart.
    Fragment 0 spans transcript 2."""
    frs = []
    for i in range(n):
        l0, l1 = RANGES[i % 6] + 2 * anchor, RANGES[(i // 6) % 6] + 2 * anchor
        ref = 0 if i % 11 == 10 else 1 if i % 7 == 6 else 2
        s0 = 1 + (7 * i) % 113
        how = (i // 3) % 4
        if how == 0:
            s1, l1 = s0, l0                                             # both ends identical
        elif how == 1:
            s1 = max(1, s0 - 3 - i % 40)                                 # end 1 in front of end 0
        elif how == 2:
            s1 = s0 + 5 + i % 60
        else:
            s1 = 1 + (13 * i) % 119
        frs.append((ref, (s0, s0 + l0 - 1), (s1, s1 + l1 - 1)))
    frs[0] = (2, (3, 3 + RANGES[0] + 2 * anchor - 1), (100, 118))
    return frs


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def cov_expected():
    """The oracle's arrays for every (anchor, trim, count), computed once; with what the inputs are meant to reach."""
    from oracle import calccov_oracle as c
    off, pos = cov_samples()
    exp = {}
    for anchor in ANCHORS:
        for trim in TRIMS:
            for n in COUNTS:
                exp[(anchor, trim, n)] = c.sample_batch(off, pos, cov_fragments(n, anchor), trim, anchor)
    for anchor in ANCHORS:
        li, lv, si, sp, sm = exp[(anchor, 0, 513)]
        sp, sm = np.array(sp), np.array(sm)
        assert np.isnan(sp).any()                                                    # range 0
        assert (np.isnan(sm) & np.isfinite(sp)).any()                                # range 1
        assert np.isfinite(sm).any() and (sp[np.isfinite(sp)] <= 1.0).all()
        per = [c.sample_batch(off, pos, [f], 0, anchor) for f in cov_fragments(513, anchor)]
        assert sum(1 for p in per if not p[0] and not p[2]) > 10                     # fragments with no output
        assert len(per[0][0]) > 100                                                  # one fragment with more than 100 samples
        assert sum(len(p[0]) for p in per) == len(li) and sum(len(p[2]) for p in per) == len(si)
        assert not exp[(anchor, 1000, 513)][0] and exp[(anchor, 1000, 513)][2] == si  # the trim only moves the length samples
    return exp


def test_cov_inputs_reach_the_edges(cov_expected):
    assert len(cov_expected) == 45


@pytest.mark.gpu
@pytest.mark.parametrize("anchor", ANCHORS)
def test_gpu_sample_batch_equals_the_oracle(built, cov_expected, anchor):
    """Indices and lengths exactly; doubles bit for bit where finite (IEEE division and floor are the same values on both
    sides); a NaN only as a NaN, its sign is the tool's to print."""
    from defuse_amd import cov
    off, pos = cov_samples()
    signs = set()
    for trim in TRIMS:
        for n in COUNTS:
            li, lv, si, sp, sm = cov_expected[(anchor, trim, n)]
            g_li, g_lv, g_si, g_sp, g_sm, t = cov.sample_batch(off, pos, cov.fragments_array(cov_fragments(n, anchor)), trim, anchor)
            assert g_li.tolist() == li and g_lv.tolist() == lv and g_si.tolist() == si, (anchor, trim, n)
            assert (t.n_length_samples, t.n_split_samples) == (len(li), len(si))
            for got, want in ((g_sp, np.array(sp, dtype=np.float64)), (g_sm, np.array(sm, dtype=np.float64))):
                assert (np.isnan(got) == np.isnan(want)).all(), (anchor, trim, n)
                fin = ~np.isnan(want)
                assert (bits(got)[fin] == bits(want)[fin]).all(), (anchor, trim, n)
                signs |= set(np.signbit(got[np.isnan(got)]).tolist())
    print("sign bit of the device's 0.0/0.0:", sorted(signs))


def test_sample_batch_refuses_bad_arguments_before_it_needs_a_device(built):
    from defuse_amd import cov, dsa
    off, pos = cov_samples()

    def call(off, frs):
        room = (np.full(4, -7, np.int32), np.full(4, -7, np.int32), np.full(4, -7, np.int32), np.full(4, 7.5), np.full(4, 7.5))
        rc, nl, ns, _ = cov.sample_batch_raw(off, pos, cov.fragments_array(frs), 0, 4, *room)
        assert all((a == a[0]).all() for a in room)
        return rc, nl, ns
    assert call(off, []) == (0, 0, 0)                                                # no fragment: DSA_OK, nothing needed
    good = cov_fragments(5, 4)
    for bad_ref in (-1, 3):
        assert call(off, good + [(bad_ref, (1, 50), (60, 110))])[0] == dsa.DSA_E_ARG
    assert call([0, 1, 0, len(pos)], good)[0] == dsa.DSA_E_ARG                       # ref_sample_off descends


@pytest.mark.gpu
def test_gpu_sample_batch_capacity_protocol(built, cov_expected):
    """A capacity one short on either side: DSA_E_CAPACITY, both needed counts, nothing written."""
    from defuse_amd import cov, dsa
    off, pos = cov_samples()
    li, lv, si, sp, sm = cov_expected[(4, 0, 257)]
    frs = cov.fragments_array(cov_fragments(257, 4))
    for short_len, short_split in ((1, 0), (0, 1), (1, 1)):
        nl, ns = len(li) - short_len, len(si) - short_split
        room = (np.full(nl, -7, np.int32), np.full(nl, -7, np.int32), np.full(ns, -7, np.int32), np.full(ns, 7.5), np.full(ns, 7.5))
        rc, need_l, need_s, _ = cov.sample_batch_raw(off, pos, frs, 0, 4, *room)
        assert (rc, need_l, need_s) == (dsa.DSA_E_CAPACITY, len(li), len(si))
        assert all((a == (7.5 if a.dtype == np.float64 else -7)).all() for a in room)
    room = (np.zeros(len(li), np.int32), np.zeros(len(li), np.int32), np.zeros(len(si), np.int32), np.zeros(len(si)), np.zeros(len(si)))
    rc, need_l, need_s, _ = cov.sample_batch_raw(off, pos, frs, 0, 4, *room)            # exactly enough
    assert (rc, need_l, need_s) == (0, len(li), len(si)) and room[0].tolist() == li and room[2].tolist() == si
    rc, need_l, need_s, _ = cov.sample_batch_raw(off, pos, frs[:0], 0, 4, *room)        # no fragment
    assert (rc, need_l, need_s) == (0, 0, 0)
