"""Which fill kernel sweeps a workgroup, pinned at every routing edge, and every record against the CPU oracle.

k_fill_fast<0> picks the owner of each workgroup of 256 pairs on the device: the 25-row-table tier 0 (at most GMAX = 4 runs of
pairs of one fusion), the split-table tiers 1 (at most GSPLIT = 20 runs) and 2 (at most GSPLIT2 = 40), or k_fill_generic (more
runs, or a read byte outside A/C/G/T/N).  The host picks the WIDE instantiation for the whole upload (its widest window has
9-16 tiles of 64 columns).  Each case asserts the workgroup counts the device reported (dsa_get_kernel_counts) and byte
equality with the oracle.  Under DSA_PLAN_NO_REORDER the caller's order is the sweep order, so pairs 256 k .. 256 k + 255 are
workgroup k and the runs are those the caller wrote; with the default planner each workgroup is counted exactly once.
"""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

LQ = 76


@pytest.fixture(scope="module")
def ctx(built):
    from defuse_amd import dsa
    c = dsa.Context(0)
    yield c
    c.close()


def oracle(batch):
    import bench
    return bench.oracle_records(batch, len(batch[3]))


class Fusions:
    """Fusions with windows of given lengths; reads that cross the junction (some at the windows' ends) or lie in one window."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.bb = cases.BatchBuilder()
        self.win = []

    def fusion(self, l0, l1):
        r0, r1 = cases.rnd(self.rng, l0), cases.rnd(self.rng, l1, b"ACGTN" if len(self.win) % 3 == 2 else b"ACGT")
        self.win.append((r0, r1))
        return self.bb.add_fusion(r0, r1, fusion_id=10 * len(self.win) + 3)

    def read(self, f, exotic=None):
        r0, r1 = self.win[f]
        rng = self.rng
        k = int(rng.integers(0, 8))
        lq = min(LQ, len(r0) + len(r1)) if k else int(rng.integers(9, LQ))
        if k == 1:                                        # junction at the last column of window 0 / first base of window 1
            read = cases.split_read(rng, r0, r1, lq, first=len(r0), s1=0)
        elif k == 2:                                      # junction at the end of window 1
            read = cases.split_read(rng, r0, r1, lq, s1=max(0, len(r1) - lq // 2))
        elif k == 3:
            w = r0 if rng.integers(0, 2) else r1
            p = int(rng.integers(0, max(1, len(w) - lq + 1)))
            read = w[p:p + lq]
        else:
            read = cases.split_read(rng, r0, r1, lq)
        read = cases.mutate(rng, read, 0.01)
        if exotic is not None and len(read) > 0:
            read = read.lower() if exotic == "lower" else read[:len(read) // 2] + exotic + read[len(read) // 2 + 1:]
        self.bb.add_read(f, read, read_end=int(rng.integers(0, 2)), revcomp=int(rng.integers(0, 2)))

    def workgroup(self, fus, n=256, exotic=None):
        """n pairs in len(fus) runs of about equal length: run k is fusion fus[k] (a fusion may come back in a later run)."""
        cut = np.linspace(0, n, len(fus) + 1).astype(int)
        for k, f in enumerate(fus):
            for j in range(cut[k], cut[k + 1]):
                self.read(f, exotic if (exotic and j == n // 2) else None)

    def arrays(self):
        return self.bb.arrays()


def run_counts(ctx, batch, flags, exp=None):
    ctx.set_plan_options(flags)
    try:
        got = ctx.align_batch(*batch)
    finally:
        ctx.set_plan_options(0)
    exp = oracle(batch) if exp is None else exp
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    kc = ctx.kernel_counts()
    assert sum(kc["fast"]) + sum(kc["fast_wide"]) + kc["generic"] == kc["workgroups"]      # every workgroup swept exactly once
    if kc["slices"] == 1:
        assert kc["workgroups"] == (len(batch[3]) + 255) // 256
    return kc, exp


def assert_counts(kc, fast=(0, 0, 0), wide=(0, 0, 0), generic=0):
    assert (kc["fast"], kc["fast_wide"], kc["generic"]) == (list(fast), list(wide), generic), kc


def runs_batch(seed=1):
    """Eight workgroups of 1, 4, 5, 20, 21, 40, 41 and 128 runs; in those of 4 and 5 runs a fusion comes back (read-major order:
    tiers count runs, not fusions)."""
    fz = Fusions(seed)
    pool = [fz.fusion(int(fz.rng.integers(150, 390)), int(fz.rng.integers(150, 390))) for _ in range(130)]
    fz.workgroup([pool[0]])
    fz.workgroup([pool[1], pool[2], pool[1], pool[3]])                 # 4 runs of 3 fusions: tier 0
    fz.workgroup([pool[4], pool[5], pool[4], pool[5], pool[4]])        # 5 runs of 2 fusions: tier 1
    fz.workgroup(pool[6:26])
    fz.workgroup(pool[26:47])
    fz.workgroup(pool[47:87])
    fz.workgroup(pool[87:128])
    fz.workgroup([pool[k % 3] for k in range(128)])                    # 128 runs of 3 fusions: generic
    return fz.arrays()


def test_runs_per_workgroup_pick_the_tier(ctx):
    kc, _ = run_counts(ctx, runs_batch(), 1)
    assert_counts(kc, fast=(2, 2, 2), generic=2)
    assert kc["slices"] == 1 and kc["workgroups"] == 8


def window_batch(seed, lens, wide_one=None):
    """A workgroup each of 2, 10 and 30 runs and one of 50 (tiers 0, 1, 2, generic) over fusions whose two windows have the
    lengths in `lens` (a different tile count on either side); wide_one: one more fusion with windows of that length, in the
    middle of the 10-run workgroup."""
    fz = Fusions(seed)
    fus = [fz.fusion(*lens[k % len(lens)]) for k in range(50)]
    extra = fz.fusion(wide_one, wide_one - 64) if wide_one else None
    fz.workgroup(fus[:2])
    fz.workgroup(fus[2:11] + ([extra] if extra is not None else fus[11:12]))
    fz.workgroup(fus[:30])
    fz.workgroup(fus[:50])
    return fz.arrays()


@pytest.mark.parametrize("lens,wide_one,wide", [
    ([(64, 65), (65, 64), (389, 300)], None, False),
    ([(512, 448), (449, 512), (64, 65)], None, False),          # 8 tiles: the widest narrow upload
    ([(389, 300), (64, 65)], 513, True),                        # one window of 9 tiles makes the whole upload WIDE
    ([(1024, 960), (960, 1024), (389, 65)], None, True),        # 16 tiles: the last WIDE upload, the 16-tile masks' edge
    ([(389, 300), (64, 65)], 1025, False),                      # one window of 17 tiles: narrow again, beyond the masks
], ids=["64-65", "512", "one-513", "1024", "one-1025"])
def test_window_lengths_pick_the_instantiation(ctx, lens, wide_one, wide):
    kc, _ = run_counts(ctx, window_batch(len(lens) * 7 + (wide_one or 0), lens, wide_one), 1)
    if wide:
        assert_counts(kc, wide=(1, 1, 1), generic=1)
    else:
        assert_counts(kc, fast=(1, 1, 1), generic=1)


@pytest.mark.parametrize("n,tail_runs,tier", [(511, 4, 0), (511, 5, 1), (513, 1, 0), (321, 20, 1), (321, 21, 2), (257, 1, 0)])
def test_last_workgroup_with_shadow_lanes(ctx, n, tail_runs, tier):
    """Batches of 256 k - 1, 256 k + 1 and 64 k + 1 pairs: the lanes past the end shadow the last pair and must not open a run
    of their own (the last workgroup has exactly tail_runs runs, the last of them ends at the last pair)."""
    fz = Fusions(n + tail_runs)
    fus = [fz.fusion(int(fz.rng.integers(100, 389)), int(fz.rng.integers(100, 389))) for _ in range(tail_runs + 1)]
    full = n // 256
    for _ in range(full):
        fz.workgroup([fus[-1]])
    fz.workgroup(fus[:tail_runs], n=n - 256 * full)
    kc, _ = run_counts(ctx, fz.arrays(), 1)
    fast = [0, 0, 0]
    fast[0] += full
    fast[tier] += 1
    assert_counts(kc, fast=fast)
    assert kc["workgroups"] == full + 1


def test_exotic_read_moves_exactly_its_workgroup(ctx):
    """One lowercase read in a tier-0 workgroup, one IUPAC code in a tier-1 and in a tier-2 workgroup: exactly those three go to
    the generic kernel, the others stay where their runs put them."""
    fz = Fusions(5)
    fus = [fz.fusion(int(fz.rng.integers(100, 389)), int(fz.rng.integers(100, 389))) for _ in range(30)]
    fz.workgroup(fus[:2])
    fz.workgroup(fus[2:4], exotic="lower")
    fz.workgroup(fus[:8])
    fz.workgroup(fus[:8], exotic=b"R")
    fz.workgroup(fus[:25])
    fz.workgroup(fus[:25], exotic=b"Y")
    kc, _ = run_counts(ctx, fz.arrays(), 1)
    assert_counts(kc, fast=(1, 1, 1), generic=3)


def test_missing_tier_reruns_the_slice(built):
    """A context whose lane last ran a tier-0 batch launches k_fill_fast<0> alone for the next one; a batch that needs tier 2
    and the generic kernel is run again with every kernel, and the next run of it is not."""
    from defuse_amd import dsa
    fz = Fusions(6)
    f = fz.fusion(389, 389)
    for _ in range(3):
        fz.workgroup([f])
    first = fz.arrays()
    second = window_batch(9, [(389, 300), (200, 389)])
    c = dsa.Context(0)
    try:
        c.set_plan_options(dsa.PLAN_NO_REORDER)
        for batch, reruns, counts in ((first, 0, dict(fast=(3, 0, 0))), (second, 1, dict(fast=(1, 1, 1), generic=1)),
                                      (second, 0, dict(fast=(1, 1, 1), generic=1))):
            got = c.align_batch(*batch)
            assert got.tobytes() == oracle(batch).tobytes()
            kc = c.kernel_counts()
            assert kc["slices_rerun"] == reruns and kc["slices"] == 1, kc
            assert_counts(kc, **counts)
    finally:
        c.close()


def classes_batch(seed=8):
    """Fusions of 256, 16, 8 and 2 pairs, grouped by fusion: the planner's size classes, one per fill kernel."""
    fz = Fusions(seed)
    for n_pairs, n_fusions in ((256, 3), (16, 30), (8, 60), (2, 200)):
        for _ in range(n_fusions):
            f = fz.fusion(int(fz.rng.integers(100, 389)), int(fz.rng.integers(100, 389)))
            for _ in range(n_pairs):
                fz.read(f)
    return fz.arrays()


@pytest.mark.parametrize("which", ["runs", "classes", "one-513"])
def test_default_planner_counts_each_workgroup_once(ctx, which):
    batch = {"runs": runs_batch, "classes": classes_batch,
             "one-513": lambda: window_batch(3 * 7 + 513, [(389, 300), (64, 65)], 513)}[which]()
    kc, _ = run_counts(ctx, batch, 0)
    if which == "classes":
        assert all(k > 0 for k in kc["fast"]) and kc["generic"] > 0, kc
    elif which == "one-513":
        assert kc["fast_wide"][0] > 0 and kc["fast"] == [0, 0, 0], kc
    else:
        assert kc["generic"] > 0 and kc["fast"][0] > 0, kc


# ------------------------------------------------------------------------------------------------------ chunk-shaped batches
@pytest.mark.parametrize("lq,ufrag,long_read", [(76, 300, False), (100, 300, False), (150, 500, True)], ids=["2x76", "2x100", "2x150-long"])
def test_chunk_shaped_batches_equal_the_oracle(built, lq, ufrag, long_read):
    """About 100 000 candidates in the shape of a chunk of the pipeline (tests/cases.chunk_batch): in read-major order under
    NO_REORDER (every workgroup holds more runs than the table tiers take), grouped by fusion as dosplitalign hands them over
    with the default planner and without per-pair bounds, and read-major through a stream in four batches."""
    from defuse_amd import dsa
    batch = cases.chunk_batch(lq, lq=lq, ufrag=ufrag, long_read=long_read)
    exp = oracle(batch)
    grouped, exp_grouped = cases.group_by_fusion(batch, exp)
    wide = ufrag + 90 > 512
    ctx = dsa.Context(0)
    try:
        kc, _ = run_counts(ctx, batch, dsa.PLAN_NO_REORDER, exp)
        assert kc["generic"] == kc["workgroups"]
        assert kc["long_pairs"] == (1 if long_read else 0)
        for flags in (0, dsa.PLAN_NO_TIGHTEN):
            kc, _ = run_counts(ctx, grouped, flags, exp_grouped)
            tiers = kc["fast_wide"] if wide else kc["fast"]
            assert tiers[2] > 0 and kc["generic"] > 0, (flags, kc)
            assert sum(kc["fast"] if wide else kc["fast_wide"]) == 0, kc
            assert kc["long_pairs"] == (1 if long_read else 0)
            assert kc["generic_tasks"] > 0
    finally:
        ctx.close()
    ref, fus, reads, pairs = batch
    n = len(pairs)
    cuts = [0, n // 5, n // 2, n // 2 + 7, n]
    st = dsa.Stream(0, depth=3)
    try:
        outs = []
        for k in range(len(cuts) - 1):
            part = pairs[cuts[k]:cuts[k + 1]].copy()
            out = np.zeros(3 * len(part) + 64, dtype=dsa.RECORD_DTYPE)
            outs.append((part, out))
        got = []
        sub = 0
        for k in range(len(outs)):
            while sub < len(outs) and sub - k < 3:
                st.submit(ref, fus, reads, outs[sub][0], outs[sub][1])
                sub += 1
            got.append(st.collect().copy())
        for k, g in enumerate(got):
            e = exp[(exp["pair_idx"] >= cuts[k]) & (exp["pair_idx"] < cuts[k + 1])].copy()
            e["pair_idx"] -= cuts[k]
            assert g.tobytes() == e.tobytes(), k
    finally:
        st.close()
