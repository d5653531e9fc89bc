"""DEFUSE_DSA_TASK_CACHE=1: dosplitalign and evalsplitalign keep the split-read task set in "<regions>.dsatasks" and load it
instead of building it again (tools_src/task_cache.hpp).  Host tests run through the test double of the streaming ABI
(tests/shim/dsa_abi_double.c); every output is compared with the oracle and with a run without the variable — stdout, stderr
and exit status included.  The GPU test runs the same cold and warm pair on the real library."""
import glob
import os
import shutil
import subprocess

import pytest

from tests import pipeline_case
from tests.test_tool_host import double  # noqa: F401  (the fixture: the test double, built as test_tool_host builds it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "dosplitalign")
EVAL = os.path.join(ROOT, "bin", "evalsplitalign")
ON = {"DEFUSE_DSA_TASK_CACHE": "1"}
TIMED = {"DEFUSE_DSA_TASK_CACHE": "1", "DEFUSE_TIMING": "1"}
HEADER = 200                                  # bytes of the file's header (task_cache.hpp, struct Header)
FILES = ("ref.fa", "ref.fa.fai", "exons.txt", "regions.txt", "improper.sam", "reads.1.fastq", "reads.2.fastq")


def oracle(c):
    from oracle import dosplitalign_oracle as ora
    return ora.dosplitalign(c["fasta"], c["exons"], c["ufrag"], c["sfrag"], c["minread"], c["maxread"], c["regions"], c["improper"],
                            c["seq1"], c["seq2"])


@pytest.fixture(scope="module")
def base(tmp_path_factory, double):  # noqa: F811
    """A pipeline case of more than 64 fusions (tasks set up on threads) with its FASTA index, and the oracle's output."""
    d = tmp_path_factory.mktemp("taskcache")
    c = pipeline_case.build(str(d / "case"), seed=31, n_fusions=70, reads_per_fusion=8, lq=50)
    exp = oracle(c)
    assert exp.count("\n") > 500
    r = run(c, str(d / "first.align"), double)          # writes ref.fa.fai, as the tool does without the variable
    assert r.returncode == 0 and open(str(d / "first.align")).read() == exp, r.stderr[-2000:]
    assert os.path.exists(c["fasta"] + ".fai") and not os.path.exists(cache_of(c))
    return c, exp


@pytest.fixture
def case(base, tmp_path):
    """The case copied into a directory of the test's own (its own cache file)."""
    c, exp = base
    src = os.path.dirname(c["fasta"])
    dst = tmp_path / "case"
    dst.mkdir()
    for n in FILES:
        shutil.copy2(os.path.join(src, n), str(dst / n))
    c2 = dict(c, fasta=str(dst / "ref.fa"), exons=str(dst / "exons.txt"), regions=str(dst / "regions.txt"), improper=str(dst / "improper.sam"),
              seq1=str(dst / "reads.1.fastq"), seq2=str(dst / "reads.2.fastq"))
    return c2, exp, tmp_path


def cache_of(c):
    return c["regions"] + ".dsatasks"


def run(c, out, lib, env=None, tool=TOOL, extra_env=None):
    e = dict(os.environ, DEFUSE_DSA_LIB=lib, **(env or {}), **(extra_env or {}))
    for k in ("DEFUSE_DSA_TASK_CACHE", "DEFUSE_TIMING"):
        if k not in (env or {}) and k not in (extra_env or {}):
            e.pop(k, None)
    return subprocess.run([tool] + pipeline_case.tool_args(c, out), capture_output=True, text=True, env=e, timeout=600)


def outcome(r, out):
    return r.returncode, r.stdout, r.stderr, (open(out).read() if os.path.exists(out) else None)


def leftovers(c):
    return [p for p in glob.glob(cache_of(c) + ".*")]


def assert_hit(c, lib, exp, tmp):
    out = str(tmp / "hit.align")
    r = run(c, out, lib, TIMED)
    assert r.returncode == 0 and "task cache hit" in r.stderr, r.stderr[-2000:]
    assert open(out).read() == exp


def test_cold_run_writes_the_cache_and_the_next_run_loads_it(case, double):  # noqa: F811
    c, exp, tmp = case
    plain = outcome(run(c, str(tmp / "plain.align"), double), str(tmp / "plain.align"))
    assert plain[0] == 0 and plain[3] == exp
    assert not os.path.exists(cache_of(c))
    cold = outcome(run(c, str(tmp / "cold.align"), double, ON), str(tmp / "cold.align"))
    assert os.path.isfile(cache_of(c)) and os.path.getsize(cache_of(c)) > HEADER
    assert cold == plain
    r = run(c, str(tmp / "timed.align"), double, TIMED)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stderr.splitlines() if "task cache" in l]
    assert len(lines) == 1 and lines[0].startswith("[dosplitalign] task cache hit: 70 tasks") and "with bins" in lines[0], lines
    assert "[tasks]" not in r.stderr                     # nothing was set up cold
    warm = outcome(run(c, str(tmp / "warm.align"), double, ON), str(tmp / "warm.align"))
    assert warm == cold
    assert leftovers(c) == []


def test_without_the_variable_no_cache_is_read_or_written(case, double):  # noqa: F811
    c, exp, tmp = case
    r = run(c, str(tmp / "o.align"), double, {"DEFUSE_TIMING": "1"})
    assert r.returncode == 0 and open(str(tmp / "o.align")).read() == exp
    assert "task cache" not in r.stderr
    assert not os.path.exists(cache_of(c)) and leftovers(c) == []
    for v in ("0", ""):
        r = run(c, str(tmp / "o.align"), double, {"DEFUSE_DSA_TASK_CACHE": v})
        assert r.returncode == 0 and not os.path.exists(cache_of(c))


def _rewrite_region_line(c):
    """One regions line rewritten at the same size (a start moved by one digit), mtime put back."""
    st = os.stat(c["regions"])
    lines = open(c["regions"]).read().split("\n")
    f = lines[6].split("\t")
    s = f[4]
    f[4] = s[:-1] + str((int(s[-1]) + 5) % 10)
    lines[6] = "\t".join(f)
    text = "\n".join(lines)
    assert len(text) == st.st_size
    open(c["regions"], "w").write(text)
    os.utime(c["regions"], ns=(st.st_atime_ns, st.st_mtime_ns))
    assert os.stat(c["regions"]).st_mtime_ns == st.st_mtime_ns and os.stat(c["regions"]).st_size == st.st_size


def _change_fasta(c):
    """Bases changed in place (every A of every other sequence line a C: same size, the index still right), a later mtime."""
    st = os.stat(c["fasta"])
    lines = open(c["fasta"], "rb").read().split(b"\n")
    lines = [l.replace(b"A", b"C") if k % 2 and not l.startswith(b">") else l for k, l in enumerate(lines)]
    open(c["fasta"], "wb").write(b"\n".join(lines))
    assert os.path.getsize(c["fasta"]) == st.st_size
    os.utime(c["fasta"], ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))


@pytest.mark.parametrize("change", ["regions", "exons", "fasta", "u", "s", "n", "x", "fai"])
def test_a_changed_input_is_a_miss(case, double, change):  # noqa: F811
    c, exp, tmp = case
    r = run(c, str(tmp / "w.align"), double, ON)
    assert r.returncode == 0 and os.path.isfile(cache_of(c))
    if change == "regions":
        _rewrite_region_line(c)
    elif change == "exons":
        st = os.stat(c["exons"])
        os.utime(c["exons"], ns=(st.st_atime_ns, st.st_mtime_ns + 2_000_000_000))
    elif change == "fasta":
        _change_fasta(c)
    elif change == "u":
        c["ufrag"] = 310.0
    elif change == "s":
        c["sfrag"] = 30.5
    elif change == "n":
        c["minread"] = 48
    elif change == "x":
        c["maxread"] = 52
    elif change == "fai":
        fai = open(c["fasta"] + ".fai").read()
        os.remove(c["fasta"] + ".fai")
    want = oracle(c) if change not in ("exons", "fai") else exp
    if change in ("regions", "fasta", "u", "s", "n", "x"):
        assert want != exp                                     # the change matters to the output
    out = str(tmp / "m.align")
    r = run(c, out, double, TIMED)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[dosplitalign] task cache miss" in r.stderr and "task cache hit" not in r.stderr, r.stderr
    assert open(out).read() == want
    if change == "fai":                                        # rebuilt as without the variable; nothing kept after a message
        assert "[fai_load] build FASTA index." in r.stderr and open(c["fasta"] + ".fai").read() == fai
        assert "task cache not written" in r.stderr
        r = run(c, out, double, TIMED)
        assert "task cache miss" in r.stderr and "task cache written" in r.stderr and open(out).read() == want
    else:
        assert "task cache written" in r.stderr
    assert_hit(c, double, want, tmp)
    assert leftovers(c) == []


def _damage(path, how):
    data = open(path, "rb").read()
    if how == "truncated":
        open(path, "wb").write(data[:len(data) * 2 // 3])
    elif how == "empty":
        open(path, "wb").close()
    elif how.startswith("payload"):
        at = HEADER + (len(data) - HEADER) * int(how[-1]) // 4
        open(path, "wb").write(data[:at] + bytes([data[at] ^ 0x01]) + data[at + 1:])
    elif how.startswith("header"):
        at = int(how.split("_")[1])
        open(path, "wb").write(data[:at] + bytes([data[at] ^ 0x20]) + data[at + 1:])
    elif how == "directory":
        os.remove(path)
        os.mkdir(path)
        open(os.path.join(path, "inside"), "w").write("x")


@pytest.mark.parametrize("how", ["truncated", "empty", "payload_1", "payload_3", "header_2", "header_40", "header_180", "header_199", "directory"])
def test_a_damaged_cache_is_ignored_and_replaced(case, double, how):  # noqa: F811
    c, exp, tmp = case
    plain = outcome(run(c, str(tmp / "plain.align"), double), str(tmp / "plain.align"))
    r = run(c, str(tmp / "w.align"), double, ON)
    assert r.returncode == 0 and os.path.isfile(cache_of(c))
    _damage(cache_of(c), how)
    got = outcome(run(c, str(tmp / "d.align"), double, ON), str(tmp / "d.align"))
    assert got == plain and got[3] == exp
    if how == "directory":
        assert os.path.isdir(cache_of(c)) and os.listdir(cache_of(c)) == ["inside"]
        r = run(c, str(tmp / "d2.align"), double, TIMED)
        assert r.returncode == 0 and open(str(tmp / "d2.align")).read() == exp
        assert "task cache miss (not a regular file)" in r.stderr and "task cache not written (rename" in r.stderr, r.stderr
    else:
        assert_hit(c, double, exp, tmp)                         # the cold run wrote a valid cache again
    assert leftovers(c) == []


def test_a_miss_line_names_its_reason(case, double):  # noqa: F811
    c, exp, tmp = case
    r = run(c, str(tmp / "a.align"), double, TIMED)
    assert "task cache miss (no cache file)" in r.stderr and "task cache written:" in r.stderr
    _damage(cache_of(c), "payload_2")
    r = run(c, str(tmp / "a.align"), double, TIMED)
    assert "task cache miss (payload checksum)" in r.stderr
    _damage(cache_of(c), "header_0")
    r = run(c, str(tmp / "a.align"), double, TIMED)
    assert "task cache miss (bad magic)" in r.stderr
    c["ufrag"] = 301.0
    r = run(c, str(tmp / "a.align"), double, TIMED)
    assert "task cache miss (key differs" in r.stderr and r.returncode == 0


def test_eight_processes_start_together_on_a_cold_cache(case, double):  # noqa: F811
    c, exp, tmp = case
    env = dict(os.environ, DEFUSE_DSA_LIB=double, DEFUSE_DSA_TASK_CACHE="1", DEFUSE_THREADS="2")
    env.pop("DEFUSE_TIMING", None)
    procs = [subprocess.Popen([TOOL] + pipeline_case.tool_args(c, str(tmp / ("p%d.align" % k))), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              env=env) for k in range(8)]
    res = [p.communicate(timeout=600) + (p.returncode,) for p in procs]
    for k, (so, se, rc) in enumerate(res):
        assert rc == 0 and so == b"" and se == b"", se[-2000:]
        assert open(str(tmp / ("p%d.align" % k))).read() == exp
    assert leftovers(c) == []
    assert_hit(c, double, exp, tmp)


def _error_inputs(c, kind):
    if kind == "one_ended_fusion":            # Initialize refuses it with a message and goes on
        open(c["regions"], "a").write("99999\t0\tchr1\t+\t1000\t1100\n")
    elif kind == "unknown_reference":        # the window cannot be cut: the set-up dies
        open(c["regions"], "a").write("99999\t0\tchrNone\t+\t1000\t1100\n99999\t1\tchr1\t-\t2000\t2100\n")
    elif kind == "negative_fusion_id":       # dies right after the set-up
        open(c["regions"], "a").write("-4\t0\tchr1\t+\t1000\t1100\n-4\t1\tchr2\t-\t2000\t2100\n")
    elif kind == "missing_exons":
        os.remove(c["exons"])
    elif kind == "bad_exon_line":
        open(c["exons"], "a").write("G\tT\tchr1\t+\t10\tx20\t\n")
    elif kind == "missing_fasta":
        os.remove(c["fasta"])


@pytest.mark.parametrize("kind", ["one_ended_fusion", "unknown_reference", "negative_fusion_id", "missing_exons", "bad_exon_line", "missing_fasta"])
def test_a_set_up_that_speaks_or_dies_is_not_kept(case, double, kind):  # noqa: F811
    c, exp, tmp = case
    _error_inputs(c, kind)
    plain = outcome(run(c, str(tmp / "plain.align"), double), str(tmp / "plain.align"))
    assert plain[0] != 0 or plain[2] != "", plain                # the input does make the tool speak
    for k in range(2):                                             # (the second time: still nothing to load)
        got = outcome(run(c, str(tmp / ("c%d.align" % k)), double, ON), str(tmp / ("c%d.align" % k)))
        assert got == plain
        assert not os.path.exists(cache_of(c)) and leftovers(c) == []


def _eval(c, align, out, env=None, tool=EVAL):
    e = dict(os.environ, **(env or {}))
    for k in ("DEFUSE_DSA_TASK_CACHE", "DEFUSE_TIMING"):
        if k not in (env or {}):
            e.pop(k, None)
    args = ["-f", c["fasta"], "-e", c["exons"], "-u", str(c["ufrag"]), "-s", str(c["sfrag"]), "-n", str(c["minread"]), "-x", str(c["maxread"]),
            "-r", c["regions"], "-a", align, "-q", out + ".seq", "-b", out + ".break", "-p", out + ".predalign"]
    r = subprocess.run([tool] + args, capture_output=True, text=True, env=e, timeout=600)
    files = tuple(open(out + x).read() for x in (".seq", ".break", ".predalign"))
    return r, (r.returncode, r.stdout, r.stderr) + files


def test_evalsplitalign_loads_the_cache_dosplitalign_wrote(case, double):  # noqa: F811
    c, exp, tmp = case
    align = str(tmp / "sorted.align")
    open(align, "w").write("".join(sorted(exp.splitlines(True), key=lambda l: int(l.split("\t")[0]))))
    _, plain = _eval(c, align, str(tmp / "plain"))
    assert plain[0] == 0 and len(plain[4]) > 0
    r = run(c, str(tmp / "w.align"), double, ON)
    assert r.returncode == 0 and os.path.isfile(cache_of(c))
    r, _ = _eval(c, align, str(tmp / "timed"), TIMED)
    assert "[evalsplitalign] task cache hit: 70 tasks" in r.stderr and "[tasks]" not in r.stderr, r.stderr
    _, warm = _eval(c, align, str(tmp / "warm"), ON)
    assert warm == plain
    # evalsplitalign as the first writer (a file without the bins): dosplitalign loads the tasks and bins them itself
    os.remove(cache_of(c))
    r, cold = _eval(c, align, str(tmp / "cold"), TIMED)
    assert "task cache written" in r.stderr and cold[3:] == plain[3:]
    out = str(tmp / "d.align")
    r = run(c, out, double, TIMED)
    assert "task cache hit: 70 tasks" in r.stderr and "with bins" not in r.stderr, r.stderr
    assert open(out).read() == exp
    assert leftovers(c) == []


def test_tasks_from_the_cache_equal_tasks_built_cold(base, tmp_path):
    """Field by field, for every task, and the bins' answers to a sweep of queries: a table loaded from the file against the one
    that was built and written (tasks set up by CreateTasks, bins as dosplitalign fills them)."""
    c, exp = base
    src = tmp_path / "eq.cpp"
    src.write_text(r'''
#include "%s/tools_src/task_cache.hpp"
using namespace defuse;
static BinnedLocations bins_of(const std::map<int, SplitAlignmentTask>& tasks) {
    BinnedLocations b(2000);
    int k = 0;
    for (const auto& kv : tasks) { for (int ce = 0; ce < 2; ++ce) for (const Location& l : kv.second.mMateRegions[ce]) b.Add(pack_id(k, ce), l); ++k; }
    b.Finish();
    return b;
}
int main(int argc, char** argv) {
    const std::string fasta = argv[1], exons = argv[2], regions_file = argv[3], path = argv[4];
    task_cache::SetUp cold;
    cold.on = true; cold.path = path;
    const auto regions = cold.read_regions(regions_file, 3);
    auto tasks = cold.tasks(fasta, exons, 300.0, 30.0, 50, 50, regions, 3, nullptr);
    if (cold.hit || !cold.clean || !cold.key_ok) { std::cerr << "expected a clean cold set-up\n"; return 1; }
    BinnedLocations b0 = bins_of(tasks);
    cold.keep(tasks, &b0, 3);
    task_cache::SetUp warm;
    warm.on = true; warm.path = path;
    BinnedLocations b1(2000);
    const auto regions2 = warm.read_regions(regions_file, 2);
    auto loaded = warm.tasks(fasta, exons, 300.0, 30.0, 50, 50, regions2, 2, &b1);
    if (!warm.hit || !warm.have_binned || loaded.size() != tasks.size() || loaded.size() < 64) { std::cerr << "no hit\n"; return 1; }
    int bad = 0;
    auto a = tasks.begin();
    for (auto b = loaded.begin(); b != loaded.end(); ++a, ++b) {
        const SplitAlignmentTask &x = a->second, &y = b->second;
        bool same = a->first == b->first && x.mFusionID == y.mFusionID;
        for (int ce = 0; ce < 2; ++ce) {
            same = same && x.mAlignRefName[ce] == y.mAlignRefName[ce] && x.mAlignStrand[ce] == y.mAlignStrand[ce] &&
                   x.mSplitAlignSeqStart[ce] == y.mSplitAlignSeqStart[ce] && x.mSplitAlignSeqLength[ce] == y.mSplitAlignSeqLength[ce] &&
                   x.mSplitSeqStrand[ce] == y.mSplitSeqStrand[ce] && x.mSplitAlignSeq[ce] == y.mSplitAlignSeq[ce] &&
                   x.mSplitRemainderSeq[ce] == y.mSplitRemainderSeq[ce] && x.mMateRegions[ce].size() == y.mMateRegions[ce].size();
            for (size_t m = 0; same && m < x.mMateRegions[ce].size(); ++m) {
                const Location &l = x.mMateRegions[ce][m], &r = y.mMateRegions[ce][m];
                same = l.refName == r.refName && l.strand == r.strand && l.start == r.start && l.end == r.end;
            }
        }
        if (!same) { std::cerr << "task " << a->first << " differs\n"; ++bad; }
    }
    const char* refs[] = {"chr1", "chr2", "chr3", "ENSG01|ENST01", "ENSG02|ENST02", "nowhere"};
    std::vector<int> i0, i1;
    size_t found = 0;
    for (const char* ref : refs)
        for (int strand = 0; strand < 2; ++strand)
            for (int s = -3000; s < 9000; s += 97) {
                const Region q{s, s + 150};
                b0.Overlapping(ref, strand, q, i0);
                b1.Overlapping(ref, strand, q, i1);
                found += i0.size();
                if (i0 != i1) { std::cerr << "bins differ at " << ref << ":" << s << "\n"; ++bad; }
            }
    if (found == 0) { std::cerr << "the sweep found nothing\n"; return 1; }
    std::cout << (bad ? "differ" : "same") << std::endl;
    return bad ? 1 : 0;
}
''' % ROOT)
    exe = tmp_path / "eq"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), str(src)])
    cache = str(tmp_path / "eq.dsatasks")
    r = subprocess.run([str(exe), c["fasta"], c["exons"], c["regions"], cache], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip() == "same", r.stderr[-3000:]


def test_cold_hit_and_damaged_cache_under_asan(case, double):  # noqa: F811
    """The sanitizer build of the tools (defuse_amd/build.py:build_sanitized, as tests/test_sanitizers.py uses it): cold run,
    hit, and a damaged file, for dosplitalign and evalsplitalign."""
    from defuse_amd import build
    from tests.test_sanitizers import ENV, BAD
    tools = build.build_sanitized("asan")
    c, exp, tmp = case
    for step in ("cold", "hit", "damaged"):
        if step == "damaged":
            _damage(cache_of(c), "payload_2")
        out = str(tmp / ("asan_%s.align" % step))
        r = run(c, out, double, TIMED, tool=tools["dosplitalign"], extra_env=ENV["asan"])
        assert not any(b in r.stderr for b in BAD), r.stderr[-3000:]
        assert r.returncode == 0 and open(out).read() == exp, r.stderr[-2000:]
        assert ("task cache hit" in r.stderr) == (step == "hit"), r.stderr
    align = str(tmp / "sorted.align")
    open(align, "w").write("".join(sorted(exp.splitlines(True), key=lambda l: int(l.split("\t")[0]))))
    _, plain = _eval(c, align, str(tmp / "plain"))
    for step in ("hit", "damaged"):
        if step == "damaged":
            _damage(cache_of(c), "truncated")
        r, got = _eval(c, align, str(tmp / ("asan_" + step)), dict(TIMED, **ENV["asan"]), tool=tools["evalsplitalign"])
        assert not any(b in r.stderr for b in BAD), r.stderr[-3000:]
        assert got[3:] == plain[3:] and got[0] == 0
        assert ("task cache hit" in r.stderr) == (step == "hit"), r.stderr


@pytest.mark.gpu
def test_cold_and_warm_runs_on_the_gpu(built, tmp_path):
    """The real library: a cold run that writes the cache and a warm run that loads it, both equal to the oracle."""
    from defuse_amd import build
    build.build_tools()
    c = pipeline_case.build(str(tmp_path / "case"), seed=5, n_fusions=70, reads_per_fusion=10)
    exp = oracle(c)
    env = dict(os.environ, DEFUSE_TIMING="1")
    env.pop("DEFUSE_DSA_TASK_CACHE", None)
    r = subprocess.run([TOOL] + pipeline_case.tool_args(c, str(tmp_path / "plain.align")), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and open(str(tmp_path / "plain.align")).read() == exp, r.stderr[-2000:]
    env["DEFUSE_DSA_TASK_CACHE"] = "1"
    for step, line in (("cold", "task cache written"), ("warm", "task cache hit: 70 tasks")):
        out = str(tmp_path / (step + ".align"))
        r = subprocess.run([TOOL] + pipeline_case.tool_args(c, out), capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert line in r.stderr, r.stderr[-2000:]
        assert open(out).read() == exp
