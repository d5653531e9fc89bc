"""The EM problems of clustermatepairs built on the GPU (include/defuse_cmp.h cmp_problems_*, defuse_amd/csrc/cmpp_api.hip),
the EM entry that takes them where they are (mpe_cluster_batch_device), the cluster rows chosen on the device
(cmp_problems_select) and the tool's DEFUSE_CMP_DEVICE_PROBLEMS=1 path.

Without a GPU: the checker (tests/cmp_problem_cases.py:problems_of) against the tool's host path, dump for dump; the exports;
the struct layouts.  With a GPU: hand-made lists with one property each, the binner's lists of 3 000 random fragments, the EM
from device arrays against the EM from host arrays, the rows against the rule in Python, and the tool both ways."""
import ctypes
import os

import numpy as np
import pytest

from tests import abi
from tests import cmp_cases
from tests import cmp_problem_cases as pc

ROOT = pc.ROOT
MFR = int(300 + 10 * 30)                # the tool's minFusionRange with -u 300 -s 30


@pytest.fixture(scope="module")
def cmp(built):
    from defuse_amd import cmp as module
    return module


@pytest.fixture(scope="module")
def tools(built):
    from defuse_amd import build
    build.build_tools()
    return True


# ---------------------------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("seed", [3, 6])
def test_checker_equals_the_host_path(tools, tmp_path, seed):
    """problems_of() over the oracle's bin pairs gives the arrays the tool's host stages hand to the EM (DEFUSE_CMP_DUMP_EM with
    the host transcription of the binning, -m 2), byte for byte: the yardstick of every device test below."""
    lines = cmp_cases.many_loci(seed)
    path = tmp_path / "spanning.txt"
    path.write_text("".join(lines))
    dump = tmp_path / "em.bin"
    r = pc.run_tool(path, tmp_path / "clusters.txt", m=2, env={"DEFUSE_CMP_HOST_BINNING": "1", "DEFUSE_CMP_DUMP_EM": str(dump)})
    assert r.returncode == 0, r.stderr
    got = pc.parse_em_dump(dump.read_bytes())
    bp, _ = pc.bin_pairs_of_lines(lines, MFR)
    want = pc.problems_of(bp, MFR, 2, 300.0)
    assert len(want["prob_off"]) > 10 and want["prob_off"][-1] > 200
    for name in ("prob_off", "x", "y", "u", "to_xo", "to_yo"):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name


def test_library_exports_cmp_problems(cmp):
    from defuse_amd import mpe
    assert abi.check_functions("defuse_cmp.h", cmp, r"cmp_[a-z_]+") == 17
    assert cmp.MPE_EXPORTS is mpe.EXPORTS
    assert abi.check_functions("defuse_mpe.h", mpe, r"mpe_[a-z_]+") == len(cmp.MPE_EXPORTS)


def test_cmp_struct_layouts_match_header(cmp):
    """sizeof and offsetof of every struct of the two headers, as a C++ and a C compiler see them, against the ctypes structs,
    and the numpy dtypes against the ctypes structs."""
    from defuse_amd import mpe
    assert cmp.MPE_STRUCTS is mpe.STRUCTS and (cmp.MpeParams, cmp.MpeTiming) == tuple(mpe.STRUCTS.values())
    abi.check("defuse_mpe.h", mpe, r"mpe_[a-z_]+")
    abi.check("defuse_cmp.h", cmp, r"cmp_[a-z_]+", dtypes=[(cmp.STRUCTS[cname], dt) for cname, dt in cmp.DTYPES.items()])
    assert (ctypes.sizeof(cmp.Row), ctypes.sizeof(cmp.ProblemCounts), ctypes.sizeof(cmp.ProblemsDevice)) == (52, 32, 96)


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def problems(cmp):
    with cmp.Problems(0) as p:
        yield p


EDGES = pc.edge_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_edges_through_build_lists(cmp, problems, case):
    """cmp_problems_build_lists of hand-made lists, one property each, against the restatement: every fetched array."""
    name, bp, mfr, mcs, mean, sizes = case
    want = pc.problems_of(bp, mfr, mcs, mean)
    if sizes is not None:                                  # the case shows what its name says
        assert np.diff(want["prob_off"]).tolist() == sizes
    else:
        n = int(name.split("_")[-1])
        kept = len({int(v) for v in want["pairs"]["first"][:-1]})
        assert 1 <= kept <= n and (n < 64 or kept < n)     # a group of n alignments, some dropped once there are many
    c = problems.build_lists(*pc.lists_of(bp), mfr, mcs, mean)
    assert (c.n_problems, c.n_mate_pairs, c.n_candidates) == (len(want["prob_off"]) - 1, int(want["prob_off"][-1]), want["n_candidates"])
    pc.assert_same_problems(problems.fetch(), want)
    # a subset only
    some = problems.fetch(("u", "bin_pair"))
    assert set(some) == {"u", "bin_pair"} and some["u"].tobytes() == want["u"].tobytes()


@pytest.fixture(scope="module")
def binner(cmp):
    with cmp.Binner(0) as b:
        yield b


@pytest.mark.gpu
@pytest.mark.parametrize("seed,mfr", [(1, 600), (5, 1500), (7, 250)])
def test_problems_from_the_binner(cmp, binner, problems, seed, mfr):
    """cmp_problems_build on what cmp_bin_run left on the device, for -m 1, 2, 3: every array equals the restatement over the
    oracle's bin pairs; the inputs populate every path (asserted on the restatement first)."""
    from tests import test_cmp_bins as tb
    frs = tb.random_fragments(seed, 3000)
    bp, _ = tb.oracle_bin_pairs(frs, mfr)
    recs, starts = tb.to_records(frs)
    st = binner.run(recs, starts, mfr)
    assert st.err_record == -1 and st.n_keys == len(bp)
    for mcs in (1, 2, 3):
        want = pc.problems_of(bp, mfr, mcs, 300.0)
        n_prob, n_mp = len(want["prob_off"]) - 1, int(want["prob_off"][-1])
        assert n_prob >= 900 and n_mp >= 20000
        if mcs == 3:
            short = sum(1 for v in bp.values() if len(v[0]) < mcs or len(v[1]) < mcs)
            entries = sum(len(a1) + len(a2) for a1, a2 in want["als"])
            both_ends = sum(1 for a1, _ in want["als"] if len({(a["frag"], a["readEnd"]) for a in a1}) > len({a["frag"] for a in a1}))
            two_bins = sum(1 for a1, _ in want["als"] for a in a1 if a["region"][0] // mfr != a["region"][1] // mfr)
            kept = sum(len(set(want["pairs"]["first"][lo:hi].tolist())) + len(set(want["pairs"]["second"][lo:hi].tolist()))
                       for lo, hi in zip(want["prob_off"], want["prob_off"][1:]))
            assert short > 0 and want["n_candidates"] > n_prob                  # lists too short; too few fragments
            products = sum(1 for fr in want["frags"] if len(fr) > len(set(fr)))                      # a fragment with several mate pairs
            assert kept < entries and products > 0 and both_ends > 0 and two_bins > 0
        c = problems.build(binner, mfr, mcs, 300.0)
        assert (c.n_problems, c.n_mate_pairs, c.n_candidates) == (n_prob, n_mp, want["n_candidates"])
        pc.assert_same_problems(problems.fetch(), want)
        v = problems.view()
        assert (v.n_problems, v.n_mate_pairs, v.device) == (n_prob, n_mp, 0) and v.x and v.to_yo and v.pairs and v.prob_off


@pytest.fixture(scope="module")
def case4(cmp):
    """the bin pairs of random_fragments(1, 3000) at minFusionRange 600 with -m 2 and their restatement"""
    from tests import test_cmp_bins as tb
    bp, _ = tb.oracle_bin_pairs(tb.random_fragments(1, 3000), 600)
    return bp, pc.problems_of(bp, 600, 2, 300.0)


def mpe_params(cmp, mcs):
    from oracle import clustermatepairs_oracle as ora
    em = ora.MatePairEM(300.0, 30.0, 0.95, mcs)
    return cmp.MpeParams(300.0, 30.0, em.min_prob, mcs, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["adversarial", "tie_heavy", "case4"])
def test_em_from_device_arrays(cmp, case4, which):
    """mpe_cluster_batch_device on arrays in device memory against mpe_cluster_batch on the same arrays in host memory:
    n_clusters, status and every member mask."""
    from tests.test_batch_assembly import DeviceArray, from_device
    if which == "case4":
        w = case4[1]
        off, x, y, u, txo, tyo = (w[n] for n in ("prob_off", "x", "y", "u", "to_xo", "to_yo"))
        prm = mpe_params(cmp, 2)
    else:
        off, x, y, u, txo, tyo = cmp_cases.adversarial_em_batch(1) if which == "adversarial" else cmp_cases.tie_heavy_em_batch(1)
        prm = mpe_params(cmp, 5)
    n_prob = min(300, len(off) - 1)
    off = np.ascontiguousarray(off[:n_prob + 1])
    n = int(off[-1])
    x, y, u = (np.ascontiguousarray(a[:n], dtype=np.float64) for a in (x, y, u))
    txo, tyo = (np.ascontiguousarray(a[:n], dtype=np.int32) for a in (txo, tyo))
    ncl, member, status = cmp.cluster_batch(prm, off, x, y, u, txo, tyo)
    with DeviceArray(x) as dx, DeviceArray(y) as dy, DeviceArray(u) as du, DeviceArray(txo) as dtx, DeviceArray(tyo) as dty, \
            DeviceArray(np.full(n, 0xAAAA, dtype=np.uint16)) as dm:
        ncl_d, none, status_d = cmp.cluster_batch(prm, off, None, None, None, None, None, on_device=(dx.ptr, dy.ptr, du.ptr, dtx.ptr, dty.ptr, dm.ptr))
        member_d = from_device(dm.ptr, n, np.uint16)
    # (random fragments seldom cluster: the case-4 input is there for its many small problems, the two batches for their clusters)
    assert none is None and n > 1000 and int(ncl.sum()) > (0 if which == "case4" else 20)
    assert ncl_d.tobytes() == ncl.tobytes() and status_d.tobytes() == status.tobytes() and member_d.tobytes() == member.tobytes()


@pytest.mark.gpu
def test_rows_chosen_on_the_device(cmp, problems, case4):
    """cmp_problems_select with synthetic n_clusters (0..10) and random masks against the rule in Python: whole, over a range
    of problems with a cluster base, and through the capacity protocol."""
    from tests.test_batch_assembly import DeviceArray
    bp, want = case4
    c = problems.build_lists(*pc.lists_of(bp), 600, 2, 300.0)
    n_prob, n = c.n_problems, c.n_mate_pairs
    assert n_prob == len(want["prob_off"]) - 1 and n == int(want["prob_off"][-1])
    rng = np.random.default_rng(8)
    ncl = rng.integers(0, 11, size=n_prob).astype(np.int32)
    member = (rng.integers(0, 1 << 16, size=n) & rng.integers(0, 1 << 16, size=n)).astype(np.uint16)      # a quarter of the bits, above n_clusters too
    ncl[:4] = (0, 10, 1, 3)
    member[want["prob_off"][5]:want["prob_off"][6]] &= 0xFFFE                                                # a cluster without members
    ncl[5] = max(ncl[5], 1)
    exp = pc.select_rows(want, 0, n_prob, ncl, member)
    # the cases the rule is about occur: a fragment whose first mate pair is no member but a later one is; a fragment with two
    # members; bits at and above n_clusters
    first_not, two, above = 0, 0, 0
    for p in range(n_prob):
        lo, hi = int(want["prob_off"][p]), int(want["prob_off"][p + 1])
        fr = want["frags"][p]
        for j in range(int(ncl[p])):
            seen = {}
            for i in range(lo, hi):
                seen.setdefault(fr[i - lo], []).append((int(member[i]) >> j) & 1)
            first_not += sum(1 for v in seen.values() if not v[0] and any(v))
            two += sum(1 for v in seen.values() if sum(v) > 1)
        above += int(np.count_nonzero(member[lo:hi] >> ncl[p]))
    assert first_not > 50 and two > 50 and above > 1000 and len(exp) > 2000
    with DeviceArray(member) as dm:
        assert problems.select(0, n_prob, ncl, dm.ptr) == len(exp)
        assert pc.rows_as_tuples(problems.rows()) == exp
        # the capacity protocol: a short buffer gets the count and nothing else, the same call with room succeeds
        with pytest.raises(cmp.CmpError) as e:
            problems.rows(cap=len(exp) - 1)
        assert e.value.code == cmp.DSA_E_CAPACITY and e.value.needed == len(exp)
        assert len(problems.rows(cap=len(exp) + 7)) == len(exp)
        # a range of problems: its own counts, the masks from its first mate pair, cluster ids from the caller's base
        p0, p1 = n_prob // 3, n_prob // 3 + 70
        lo, hi = int(want["prob_off"][p0]), int(want["prob_off"][p1])
        part = pc.select_rows(want, p0, p1, ncl[p0:p1], member[lo:hi], cluster_base=1000)
        assert len(part) > 50
        assert problems.select(p0, p1, ncl[p0:p1], dm.ptr + 2 * lo, cluster_base=1000) == len(part)
        assert pc.rows_as_tuples(problems.rows()) == part
        assert problems.select(7, 7, ncl[7:7], dm.ptr) == 0 and len(problems.rows()) == 0


def lines_of_rows(text):
    return text.splitlines(True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loci3", "loci6", "config3"])
def test_tool_with_device_problems(tools, tmp_path, name):
    """The tool with DEFUSE_CMP_DEVICE_PROBLEMS=1 against the tool without: clusters file, stdout, exit status and the
    DEFUSE_CMP_DUMP_EM file, for 1 and 7 host threads times 1 and 3 chunks; the loci inputs also against the oracle."""
    path = tmp_path / "spanning.txt"
    if name == "config3":
        cmp_cases.config3_write(20000, str(path))
        lines = None
    else:
        lines = cmp_cases.many_loci(int(name[4:]))
        path.write_text("".join(lines))
    outs = {}
    for threads, chunks in (("1", "1"), ("1", "3"), ("7", "1"), ("7", "3")):
        for dev in ("0", "1"):
            env = {"DEFUSE_THREADS": threads, "DEFUSE_CMP_CHUNKS": chunks, "DEFUSE_TIMING": "1"}
            if dev == "1":
                env["DEFUSE_CMP_DEVICE_PROBLEMS"] = "1"
            out = tmp_path / ("clusters.%s.%s.%s" % (threads, chunks, dev))
            r = pc.run_tool(path, out, env=env)
            assert r.returncode == 0, r.stderr
            assert ("problems on the device" in r.stderr) == (dev == "1"), r.stderr      # the path that ran, from its timing line
            outs[(threads, chunks, dev)] = (out.read_text(), r.stdout)
    ref = outs[("1", "1", "0")]
    assert len(ref[0]) > 500 and all(v == ref for v in outs.values())
    if lines is not None:
        from oracle import clustermatepairs_oracle as o
        exp, n = o.clustermatepairs(lines, 300, 30, 0.95, 5)
        assert n >= 8 and ref[0] == exp
    dumps = []
    for dev in ("0", "1"):
        dump = tmp_path / ("em." + dev)
        env = {"DEFUSE_CMP_DUMP_EM": str(dump)}
        if dev == "1":
            env["DEFUSE_CMP_DEVICE_PROBLEMS"] = "1"
        r = pc.run_tool(path, tmp_path / "unused.txt", env=env)
        assert r.returncode == 0, r.stderr
        dumps.append(dump.read_bytes())
    assert len(dumps[0]) > 1000 and dumps[0] == dumps[1]


@pytest.mark.gpu
def test_tool_stays_on_the_host_path_where_it_must(tools, tmp_path):
    """DEFUSE_CMP_HOST_BINNING=1 keeps the host path and says so; so does DEFUSE_GPUS when it names more than one distinct
    device, which takes a machine with two GPUs to run: on a machine with one, the same variable naming one device several
    times must leave the device path in place (the other side of that decision).  The output is the default's either way."""
    import ctypes
    from defuse_amd import dsa
    lib = ctypes.CDLL(dsa.LIB_PATH)
    lines = cmp_cases.many_loci(3)
    path = tmp_path / "spanning.txt"
    path.write_text("".join(lines))
    r0 = pc.run_tool(path, tmp_path / "a.txt")
    assert r0.returncode == 0, r0.stderr
    want = (tmp_path / "a.txt").read_text()
    several = lib.dsa_device_count() >= 2
    for k, (env, stays) in enumerate((({"DEFUSE_CMP_HOST_BINNING": "1"}, True), ({"DEFUSE_GPUS": "0,1" if several else "0,0,0"}, several))):
        out = tmp_path / ("b%d.txt" % k)
        r = pc.run_tool(path, out, env=dict(env, DEFUSE_CMP_DEVICE_PROBLEMS="1", DEFUSE_TIMING="1"))
        assert r.returncode == 0, r.stderr
        assert ("stays on the host path" in r.stderr) == stays and ("problems on the device" in r.stderr) == (not stays), r.stderr
        assert out.read_text() == want and r.stdout == r0.stdout
