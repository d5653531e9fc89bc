"""setcover: oracle behaviour (CPU) and GPU parity, including the drop-in binary."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "setcover")


def random_clusters(seed, n_clusters=300, n_frag=900, big=0):
    rng = np.random.default_rng(seed)
    clusters = []
    for c in range(n_clusters):
        kind = rng.integers(0, 10)
        if kind == 0:
            clusters.append([])                                          # id gap
            continue
        base = int(rng.integers(0, n_frag - 40))
        n = int(rng.integers(1, 14))
        frs = [base + int(x) for x in rng.integers(0, 30, size=n)]       # overlapping neighbourhoods, duplicates
        if kind == 1 and clusters:
            frs = list(clusters[int(rng.integers(0, len(clusters)))])    # exact copy: size ties
        clusters.append(frs)
    for b in range(big):                                                 # one large component: a chain of overlapping clusters
        start = n_frag + 10 + 400 * b
        for k in range(70):
            clusters.append([start + 3 * k + d for d in range(5)])
    return clusters


def write_cluster_file(path, clusters, seed=0):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for cid, frs in enumerate(clusters):
            for e in (0, 1):
                for fr in frs:
                    f.write("%d\t%d\t%d\t%d\tchr%d\t%s\t%d\t%d\n" % (cid, e, fr, int(rng.integers(0, 2)), 1 + cid % 3, "+-"[e],
                                                                   1000 + fr, 1050 + fr))


def test_oracle_tie_rule():
    from oracle import setcover_oracle as o
    # equal sizes: the highest index wins first; after a decrement the most recently changed wins
    assert o.set_cover([[1, 2, 3], [3, 4], [4, 5, 6], [1, 2, 3]]) == [[], [], [4, 5, 6], [1, 2, 3]]


def test_oracle_chain_exact():
    from oracle import setcover_oracle as o
    # sizes 2,2,2: cluster 2 wins (last arrival) and takes 3,4; cluster 1 drops to 1 (fragment 3 gone);
    # cluster 0 (size 2) then takes 1,2; cluster 1 ends empty
    assert o.set_cover([[1, 2], [2, 3], [3, 4]]) == [[1, 2], [], [3, 4]]


def test_oracle_file_roundtrip(tmp_path):
    from oracle import setcover_oracle as o
    clusters = random_clusters(1, n_clusters=40, n_frag=120)
    p = tmp_path / "clusters.txt"
    write_cluster_file(p, clusters)
    assert o.read_clusters(str(p)) == [c for c in clusters][:len(o.read_clusters(str(p)))]
    out = o.setcover(str(p), 3)
    kept = {}
    for line in out.splitlines():
        f = line.split("\t")
        kept.setdefault(int(f[0]), set()).add(int(f[2]))
    assert kept and all(len(v) >= 3 for v in kept.values())
    allf = [fr for v in kept.values() for fr in v]
    assert len(allf) == len(set(allf))                                   # every fragment in at most one cluster


def test_cli(built):
    from defuse_amd import build
    build.build_tools()
    r = subprocess.run([TOOL, "-c", "x"], capture_output=True, text=True)
    assert r.returncode == 1 and "One or more required arguments missing!" in r.stderr
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True)
    assert "Set cover for maximum parsimony" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("seed,big", [(1, 0), (2, 1), (3, 2)])
def test_gpu_cover_matches_oracle(built, seed, big):
    from defuse_amd import sc
    from oracle import setcover_oracle as o
    clusters = random_clusters(seed, big=big)
    sol, t = sc.cover(clusters)
    exp = o.set_cover(clusters)
    assert [sorted(set(s)) for s in sol] == [sorted(set(s)) for s in exp]
    assert t.n_components > 10 and t.n_large >= (1 if big else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [None, "1", "7", "64"])
def test_setcover_tool_matches_oracle(built, tmp_path, threads):
    import os
    from defuse_amd import build
    from oracle import setcover_oracle as o
    build.build_tools()
    clusters = random_clusters(7, n_clusters=500, n_frag=1500, big=1)
    p = tmp_path / "clusters.txt"
    write_cluster_file(p, clusters)
    outp = tmp_path / "clusters.sc"
    env = dict(os.environ, DEFUSE_THREADS=threads) if threads else None        # host pieces: one, several, more than lines
    r = subprocess.run([TOOL, "-c", str(p), "-m", "3", "-o", str(outp)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Reading clusters\nCalculating set cover solution\nWriting out clusters\n"
    exp = o.setcover(str(p), 3)
    assert outp.read_text() == exp and len(exp.splitlines()) > 100


GOOD_LINES = ["%d\t%d\t%d\t1\tchr1\t+\t%d\t%d" % (c, e, 10 * c + k, 1000 + k, 1050 + k) for c in range(40) for e in (0, 1) for k in range(6)]


@pytest.mark.parametrize("threads", [None, "3", "16"])
@pytest.mark.parametrize("bad,message", [
    ("", "Error: Empty clusters line {n} of {path}\n"),
    ("7\t0", "Error: Format error for clusters line {n} of {path}\n"),
    ("7\tx\t12\t1\tchr1\t+\t5\t9", "Failed to interpret line:\n7\tx\t12\t1\tchr1\t+\t5\t9\n"),
    ("7\t0\t12 \t1\tchr1\t+\t5\t9", "Failed to interpret line:\n7\t0\t12 \t1\tchr1\t+\t5\t9\n"),
    ("7\t0\t99999999999\t1", "Failed to interpret line:\n7\t0\t99999999999\t1\n"),
    ("-3\t0\t12\t1\tchr1\t+\t5\t9", "Error: Invalid cluster ID for line {n} of {path}\n"),
])
def test_setcover_tool_reports_the_first_bad_line_as_a_serial_reader_would(built, tmp_path, threads, bad, message):
    """ReadClusters' error exits (tools/Parsers.cpp:23-84) from the threaded, one-pass reader: the first bad line of the file
    decides, whichever piece it is in and whatever comes later; these runs end before the tool needs a GPU."""
    import os
    lines = list(GOOD_LINES)
    n = 301
    lines.insert(n - 1, bad)
    lines.insert(n + 60, "9\ty\t1")                      # a later bad line of another kind: never reported
    p = tmp_path / "clusters.txt"
    p.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, DEFUSE_THREADS=threads) if threads else dict(os.environ)
    r = subprocess.run([TOOL, "-c", str(p), "-m", "3", "-o", str(tmp_path / "out.sc")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 1
    assert r.stdout == "Reading clusters\n"
    assert r.stderr == message.format(n=n, path=str(p))


def test_setcover_tool_negative_cluster_id_on_end_one_is_not_an_error_in_the_reader(built, tmp_path):
    """The reader skips end-1 lines before it looks at the cluster id (tools/Parsers.cpp:60-70): such a file gets as far as the
    set cover (and, without a GPU, to the tool's own message about that)."""
    lines = list(GOOD_LINES)
    lines.insert(100, "-3\t1\t12\t1\tchr1\t+\t5\t9")
    p = tmp_path / "clusters.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([TOOL, "-c", str(p), "-m", "3", "-o", str(tmp_path / "out.sc")], capture_output=True, text=True, timeout=120)
    assert r.stdout.startswith("Reading clusters\nCalculating set cover solution\n")
    assert "Invalid cluster ID" not in r.stderr or r.stderr.startswith("Error: Invalid cluster ID for line 101")      # the writer (:86-170) does look at it


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [None, "5"])
def test_setcover_tool_writer_reports_a_negative_cluster_id_on_an_end_one_line(built, tmp_path, threads):
    """WriteClusters (tools/Parsers.cpp:86-170) checks the id of every line, whatever its end, and names the OUTPUT file."""
    import os
    lines = list(GOOD_LINES)
    lines.insert(100, "-3\t1\t12\t1\tchr1\t+\t5\t9")
    p, outp = tmp_path / "clusters.txt", tmp_path / "out.sc"
    p.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, DEFUSE_THREADS=threads) if threads else dict(os.environ)
    r = subprocess.run([TOOL, "-c", str(p), "-m", "3", "-o", str(outp)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 1
    assert r.stdout == "Reading clusters\nCalculating set cover solution\nWriting out clusters\n"
    assert r.stderr == "Error: Invalid cluster ID for line 101 of %s\n" % outp


@pytest.mark.gpu
@pytest.mark.parametrize("threads", ["1", "6"])
def test_setcover_tool_cluster_lines_in_any_order(built, tmp_path, threads):
    """clusters[id] is built in file order whatever the order of the lines (tools/Parsers.cpp:72-73): a file whose lines are
    shuffled — every host piece then sees every cluster id — against the oracle reading the same file."""
    import os
    from oracle import setcover_oracle as o
    clusters = random_clusters(11, n_clusters=300, n_frag=900, big=1)
    p, outp = tmp_path / "clusters.txt", tmp_path / "clusters.sc"
    write_cluster_file(p, clusters)
    lines = p.read_text().splitlines()
    np.random.default_rng(5).shuffle(lines)
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([TOOL, "-c", str(p), "-m", "3", "-o", str(outp)], capture_output=True, text=True,
                       env=dict(os.environ, DEFUSE_THREADS=threads), timeout=300)
    assert r.returncode == 0, r.stderr
    exp = o.setcover(str(p), 3)
    assert outp.read_text() == exp and len(exp.splitlines()) > 100


# ---- connected components: a label that has to travel the length of a chain ------------------------------------------------

def label_chain(n, ids, first_element=0):
    """One component of n clusters, the path 0 - (n-1) - (n-2) - ... - 1 (cluster indices), consecutive clusters of the path
    sharing one element; the shared elements' ids descend ("down") or ascend ("up") along the path from cluster 0.  Every
    cluster also holds one element of its own, so the greedy has sizes that tie.  Elements are first_element .. first_element
    + 2n - 2."""
    assert n >= 2 and ids in ("down", "up")
    path = [0] + list(range(n - 1, 0, -1))
    clusters = [[] for _ in range(n)]
    for j in range(n - 1):
        e = first_element + (j if ids == "up" else n - 2 - j)
        clusters[path[j]].append(e)
        clusters[path[j + 1]].append(e)
    for c in range(n):
        clusters[c].append(first_element + n - 1 + c)
    return clusters


def element_lists(clusters):
    e2c = {}
    for c, lst in enumerate(clusters):
        for e in lst:
            e2c.setdefault(e, []).append(c)
    return [e2c[e] for e in sorted(e2c)]                                 # ascending element id = ascending lane


def rounds_cluster_hooking(clusters, schedule, cap):
    """The component rounds as they were before hooking went to the roots, in plain Python.  Hook: every element lowers the
    label of each of ITS CLUSTERS to the minimum label among them.  Compress: label[c] = root of label[c].  One round = one
    launch of each and one look at the `changed` flag.  schedule "lockstep": a launch reads all labels before it writes any
    (64 consecutive elements are one wave; nothing cascades inside a launch); "serial": elements one after the other in
    ascending id, each seeing what the earlier ones wrote."""
    label = list(range(len(clusters)))
    lists = [l for l in element_lists(clusters) if len(l) >= 2]
    for rounds in range(1, cap + 1):
        changed = False
        src = list(label) if schedule == "lockstep" else label
        for l in lists:
            m = min(src[c] for c in l)
            for c in l:
                if src[c] > m:
                    label[c] = min(label[c], m)
                    changed = True
        for c in range(len(label)):
            r = label[c]
            while label[r] != r:
                r = label[r]
            if r != label[c]:
                label[c] = r
                changed = True
        if not changed:
            return rounds, label
    return None, label


def rounds_root_hooking(clusters, cap):
    """The rounds of defuse_amd/csrc/sc_api.hip (k_hook, k_compress) under the lockstep schedule: every element hangs the roots
    of its clusters' trees under the smallest of them; then every label becomes its root."""
    label = list(range(len(clusters)))
    lists = [l for l in element_lists(clusters) if len(l) >= 2]

    def root(lab, c):
        while lab[c] != c:
            c = lab[c]
        return c
    for rounds in range(1, cap + 1):
        changed = False
        src = list(label)
        for l in lists:
            roots = [root(src, c) for c in l]
            m = min(roots)
            for r in roots:
                if r > m:
                    label[r] = min(label[r], m)
                    changed = True
        label = [root(label, c) for c in range(len(label))]
        if not changed:
            return rounds, label
    return None, label


# root hooking with full compression: the trees of a component halve at least every two rounds (a tree that does not hang
# itself under a neighbour sees every neighbour hang itself somewhere, and in the round after either follows one of them or
# has them all), plus the round that finds nothing to do; ceil(log2 n) + 2 is the figure for halving every round.  The tests
# allow four times that.
def cc_round_bound(n):
    return 4 * ((n - 1).bit_length() + 2)


def test_label_chain_needs_a_round_per_cluster_when_clusters_are_hooked():
    """Why label_chain is a case: with hooking by cluster the smallest label advances one cluster per round along the path,
    under either schedule, so the rounds grow with the length of the chain (and past the 10 000-round cap a valid input was
    refused); hooking by root does not care about the length."""
    n = 400
    for ids in ("down", "up"):
        clusters = label_chain(n, ids)
        assert sorted(len(c) for c in clusters) == [2, 2] + [3] * (n - 2)
        slow, label = rounds_cluster_hooking(clusters, "lockstep", 2 * n)
        assert slow is not None and slow >= n // 2 and set(label) == {0}, (ids, slow)
        fast, label = rounds_root_hooking(clusters, 2 * n)
        assert fast is not None and fast <= cc_round_bound(n) and set(label) == {0}, (ids, fast)
    slow, _ = rounds_cluster_hooking(label_chain(n, "down"), "serial", 2 * n)      # ascending ids run against the label's way
    assert slow >= n // 2


@pytest.mark.gpu
def test_gpu_components_of_long_chains(built):
    """Two chains of 12 000 clusters, one numbered each way, as two components of one call: converges in a number of rounds
    that does not grow with the chain (cc_round_bound: 64 here), and every owner is the oracle's."""
    from defuse_amd import sc
    from oracle import setcover_oracle as o
    n = 12000
    clusters = label_chain(n, "down") + label_chain(n, "up", first_element=2 * n - 1)
    sol, t = sc.cover(clusters)
    print("cc_iterations", t.cc_iterations, "components_ms", t.components_ms, "greedy_ms", t.greedy_ms)
    assert t.n_components == 2 and t.n_large == 2
    assert cc_round_bound(n) == 64 and t.cc_iterations <= 64
    assert sol == o.set_cover(clusters)


# ---- routing (lane kernel / wave kernel) and ties -----------------------------------------------------------------------------

EDGE_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 129)       # 32 | 33: SMALL_MAX; 64, 65, 129: lane strides of the wave kernel
FAR_ELEMENT = (1 << 20) - 3


def tie_component(k, base, far=None):
    """One component of exactly k clusters on elements base, base + 1, ...: a three-cluster core on which the tie rules
    part ([a, b, e], [a, b], [e, f, g]: the last of the two largest goes first and takes e; that decrement makes cluster 0 the
    most recent of the two that are left with two elements), then exact copies of earlier clusters and near copies (one
    element more, or one element listed twice), so that most choices are ties and elements sit in three and more clusters.
    Which clusters are copied is drawn at random, and copies can level the core's difference out again: the first seed is
    taken whose component still tells both wrong rules of greedy_with_rule from the reference's (components do not touch,
    so this can be asked of one alone).  Returns (clusters, number of elements used)."""
    if k == 1:
        return [[base, base + 1, base]], 2                               # nothing to choose; an element listed twice
    if k == 2:
        return [[base, base + 1], [base + 1, base]], 2                   # one choice: which of two equal clusters
    a, b, e, f, g = range(base, base + 5)
    for seed in range(200):
        clusters = [[a, b, e], [a, b], [e, f, g]]
        nxt = base + 5
        rng = np.random.default_rng(1000 * k + seed)
        while len(clusters) < k:
            src = list(clusters[int(rng.integers(0, len(clusters)))])
            kind = len(clusters) % 4
            if kind == 1 and len(src) < 6:
                src.append(nxt)                                          # near copy: one new element
                nxt += 1
            elif kind == 2:
                src.append(src[int(rng.integers(0, len(src)))])          # near copy: an element twice
            elif kind == 3:
                rng.shuffle(src)                                         # exact copy, other order of taking
            clusters.append(src)
        if far is not None:
            clusters[-1].append(far)
        ref = greedy_with_rule(clusters, "reference")
        if greedy_with_rule(clusters, "lowest") != ref and greedy_with_rule(clusters, "stale") != ref:
            return clusters, nxt - base
    raise AssertionError("no component of %d clusters tells the tie rules apart" % k)


def tie_case():
    """Components of every size in EDGE_SIZES, empty clusters between them, small element ids but one.
    Returns (clusters, [cluster index range of each component])."""
    clusters, spans, base = [], [], 0
    for k in EDGE_SIZES:
        comp, used = tie_component(k, base, far=FAR_ELEMENT if k == 129 else None)
        spans.append(range(len(clusters), len(clusters) + k))
        clusters += comp
        clusters += [[]] * (1 + k % 3)
        base += used + 2                                                 # and element ids nobody lists
    return clusters, spans


def greedy_with_rule(clusters, rule):
    """The greedy of tools/setcover.cpp:30-110 written the slow way, with the tie rule as a parameter: "reference" = among the
    largest the one that arrived at its size last (arrival refreshed by every decrement); "lowest" = the lowest index
    among the largest; "stale" = arrival order never refreshed (the highest index among the largest)."""
    e2c = {}
    for c, lst in enumerate(clusters):
        for e in lst:
            e2c.setdefault(e, []).append(c)
    size = [len(c) for c in clusters]
    seq = list(range(1, len(clusters) + 1))
    counter = len(clusters)
    sol, owned = [[] for _ in clusters], set()
    while True:
        if rule == "lowest":
            best = max(range(len(clusters)), key=lambda c: (size[c], -c), default=None)
        else:
            best = max(range(len(clusters)), key=lambda c: (size[c], seq[c]), default=None)
        if best is None or size[best] <= 0:
            return sol
        for e in clusters[best]:
            if e in owned:
                continue
            owned.add(e)
            sol[best].append(e)
            for c2 in e2c[e]:
                size[c2] -= 1
                counter += 1
                if rule != "stale":
                    seq[c2] = counter


def component_count(clusters):
    """(components, components of more than 32 clusters) by union-find; every cluster is a node, the empty ones too."""
    parent = list(range(len(clusters)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    seen = {}
    for c, lst in enumerate(clusters):
        for e in lst:
            if e in seen:
                parent[find(c)] = find(seen[e])
            else:
                seen[e] = c
    sizes = {}
    for c in range(len(clusters)):
        sizes[find(c)] = sizes.get(find(c), 0) + 1
    return len(sizes), sum(1 for s in sizes.values() if s > 32)


def test_tie_case_tells_the_tie_rules_apart():
    """Precondition of test_gpu_routing_and_ties, on the oracle alone: in every component of the case the oracle's answer
    is not the answer of either wrong tie rule, so a kernel that breaks ties one of those ways fails there.  (A component of
    one cluster has no choice to make, and one of two clusters only the first: there a rule cannot show, and the test says so
    by asserting equality.)"""
    from oracle import setcover_oracle as o
    clusters, spans = tie_case()
    assert [len(s) for s in spans] == list(EDGE_SIZES)
    exp = o.set_cover(clusters)
    assert greedy_with_rule(clusters, "reference") == exp
    lowest, stale = greedy_with_rule(clusters, "lowest"), greedy_with_rule(clusters, "stale")
    for span in spans:
        k = len(span)
        part = lambda sol: [sorted(sol[c]) for c in span]
        assert (part(lowest) != part(exp)) == (k >= 2), k
        assert (part(stale) != part(exp)) == (k >= 3), k
    # what is mixed in
    assert any(len(set(c)) < len(c) for c in clusters)                               # an element listed twice
    lists = element_lists(clusters)
    assert sum(1 for l in lists if len(set(l)) >= 3) > 50                            # elements of three and more clusters
    assert all(clusters[s[-1] + 1] == [] for s in spans)                             # empty clusters between components
    els = sorted({e for c in clusters for e in c})
    assert els[-1] == FAR_ELEMENT and els[-2] < 2000                                 # one far id: a sparse element table
    n_comp, n_large = component_count(clusters)
    assert n_large == 5 and n_comp == len(EDGE_SIZES) + sum(1 for c in clusters if not c)


@pytest.mark.gpu
def test_gpu_routing_and_ties(built):
    from defuse_amd import sc
    from oracle import setcover_oracle as o
    clusters, _ = tie_case()
    sol, t = sc.cover(clusters)
    assert sol == o.set_cover(clusters)
    assert (t.n_components, t.n_large) == component_count(clusters)
