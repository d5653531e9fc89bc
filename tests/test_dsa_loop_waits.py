"""The row-group loops of the fill kernels - the sweeps of a tile, the table-driven tail replay and its kept-row cursor -
against the CPU oracle.

These loops fetch the next row group's operands (row codes, the boundary column of the tile to the left) while the current
one is swept; the change this file came with moved where those loads are waited for: nothing is pending when a loop is
entered, the first boundary group is one 16-byte load under the uniform branch, the replay keeps the two sides' boundary
words as loaded and merges them at use, and kept_row() reads LDS or, past KCACHE kept rows, global memory on a path of its
own.  What can go wrong there is decided by how many row groups a wave has (one; the last group prefetching itself), how
many tiles (first and last at once), where the tile to the left stops, whether a tile is entered again after a dead
stretch (the gap-skip resume, the second way into the loop), which kernel owns the workgroup, and in the replay by which
sides a task has, where the lanes' left tiles stop and how many kept rows a pair has.  The cases plant exactly that; every
one must be byte-equal to the oracle and must hand the replay the same number of tasks as the commit before the change.

Where a tile stops is decided by the pruning and is not visible from outside; the cases are built so that the stops differ,
the assertions are on records and task counts.
"""
import numpy as np
import pytest

from tests import cases

WT = 56          # every case runs at this tile width (DEFUSE_DSA_TILE_COLS)
KCACHE = 3       # dsa_kernels.hpp: kept rows per pair that travel through LDS
NO_REORDER = 1   # dsa.PLAN_NO_REORDER: pair p is thread p % 256 of workgroup p // 256


def other(base):
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


class Junctions:
    """Fusions whose windows hold the two anchors of a junction read at chosen columns.  Window 0 holds anchor A, followed by
    the first `homology` bases of anchor B, at every column of at0; M2 runs over window 1 reversed, and window 1 holds B so
    that it begins at every column of at1 of the reversed window.  A read that leaves window 0 after `a` bases is
    A[-a:] + B[:lq - a]; with homology h it scores the same for h + 1 splits.  alt0 / alt1 plant a second, unrelated pair of
    anchors (A', B') the same way: read(..., alt=(1, 0)) is A'[-a:] + B[:lq - a], and so on."""

    def __init__(self, seed, anchor=40, alphabet=b"ACGT"):
        self.rng = np.random.default_rng(seed)
        self.bb = cases.BatchBuilder()
        self.anchor = anchor
        self.alphabet = alphabet
        self.fus = []

    def fusion(self, l0, l1, at0, at1, homology=0, alt0=(), alt1=(), fill0=(), fill1=()):
        n = self.anchor
        A, B, A2, B2 = (cases.rnd(self.rng, n, self.alphabet) for _ in range(4))
        ref0 = bytearray(cases.rnd(self.rng, l0))
        ref1 = bytearray(cases.rnd(self.rng, l1))
        for lo, hi, base in fill0:
            ref0[lo:hi] = base * (hi - lo)
        for lo, hi, base in fill1:
            ref1[lo:hi] = base * (hi - lo)
        for cols, a, b in ((at0, A, B), (alt0, A2, B)):
            for p in cols:
                ref0[p:p + n + homology] = a + b[:homology]
                if p + n + homology < l0:        # the homology ends here, in every copy: no split scores the same by chance
                    ref0[p + n + homology] = other(b[homology])
        for cols, a, b in ((at1, A, B), (alt1, A, B2)):
            for r in cols:
                p = l1 - r - n
                ref1[p:p + n] = b
                if p > 0:
                    ref1[p - 1] = other(a[-1])
        assert len(ref0) == l0 and len(ref1) == l1
        self.fus.append(((A, A2), (B, B2)))
        return self.bb.add_fusion(bytes(ref0), bytes(ref1), fusion_id=5 * len(self.fus) + 2)

    def read(self, f, lq, a, alt=(0, 0), exotic=None):
        A, B = self.fus[f][0][alt[0]], self.fus[f][1][alt[1]]
        assert 0 <= a <= self.anchor and 0 <= lq - a <= self.anchor
        read = A[self.anchor - a:] + B[:lq - a]
        if exotic is not None:
            read = read[:2] + exotic + read[3:]
        assert len(read) == lq
        self.bb.add_read(f, read, read_end=len(self.bb.pairs) & 1, revcomp=(len(self.bb.pairs) >> 1) & 1)

    def arrays(self):
        return self.bb.arrays()


# ---- the sweeps ----

def lq_case(lq, n=200):
    """Reads of one length over windows of two tiles whose anchors straddle the tile boundary: lq 1 and 3 are one row group
    (rows 0-3), lq 4 and 5 two (the second prefetches itself), 76 the usual twenty."""
    def make():
        js = Junctions(20 + lq)
        f = js.fusion(100, 100, [WT - 20], [WT - 20])
        for k in range(n):
            js.read(f, lq, (lq // 2 + k % 3) % (lq + 1) if lq < 76 else 36 + k % 5)
        return js.arrays(), 0
    return make


def window_case(l, n=200):
    """Windows of l bases on both sides: 56 is one tile (the first and the last at once), 57 a second tile of one column, 112
    two whole tiles, 389 seven.  The anchors lie at the end of the window, in its last tile(s)."""
    def make():
        js = Junctions(500 + l)
        f = js.fusion(l, l, [l - 42], [l - 41])
        g = js.fusion(l, l - 1 if l > 56 else l, [3], [5], homology=1)
        for k in range(n):
            js.read(f if (k >> 6) & 1 else g, 50, 12 + k % 25)      # four runs: the workgroup is tier 0's
        return js.arrays(), 0
    return make


def left_stops_early_case():
    """Two waves, reads of 76 bases (20 row groups), windows of four tiles.  Tile 0 of both matrices is a homopolymer no read
    has a base of: nothing in it is alive, it stops after its first row group, and the tile behind it lives on - its
    boundary past the stop reads as V = 0.  Tile 3 is random and stops in between."""
    l = 3 * WT + 40
    js = Junctions(11, anchor=60, alphabet=b"ACG")
    f = js.fusion(l, l, [WT + 10], [WT + 12], fill0=[(0, WT, b"T")], fill1=[(l - WT, l, b"T")])
    for k in range(128):
        js.read(f, 76, 20 + (k * 7) % 37)
    return js.arrays(), 0


def late_resume_case():
    """As above, but the anchors straddle the boundary of tiles 1 and 2: a read that takes `a` bases of A crosses into tile 2
    at row a - 30 (M1; M2 alike), so tile 2 has nothing alive in its first row groups and is entered again only over its
    boundary column, at rows from 1 to 26 depending on the lane - the gap-skip resume, the loop's second way in."""
    l = 3 * WT + 40
    js = Junctions(12, anchor=60, alphabet=b"ACG")
    f = js.fusion(l, l, [2 * WT - 30], [2 * WT - 30], fill0=[(0, WT, b"T")], fill1=[(l - WT, l, b"T")])
    for k in range(128):
        js.read(f, 76, 56 - (k % 4) if k < 64 else 20 + (k * 7) % 37)     # first wave: every lane crosses at rows 23-26
    return js.arrays(), 0


OWNER_RUNS = {"owner-tier0": 4, "owner-tier1": 10, "owner-tier2": 30, "owner-generic": 50}


def owner_case(n_runs):
    """One workgroup of 256 pairs in the caller's order, in n_runs runs of pairs of one fusion: 4, 10, 30 and 50 runs are
    owned by the table tiers 0, 1, 2 and by the generic kernel.  Windows of three tiles; every third fusion ties over two."""
    def make():
        js = Junctions(700 + n_runs, anchor=50)
        cut = np.linspace(0, 256, n_runs + 1).astype(int)
        for k in range(n_runs):
            l0, l1 = 3 * WT - 8 - k % 5, 2 * WT + 30 + k % 7
            f = js.fusion(l0, l1, [WT + 10] + ([5] if k % 3 == 0 else []), [WT - 12], homology=k % 3)
            for t in range(cut[k], cut[k + 1]):
                js.read(f, 40 + t % 23, 14 + t % 20)
        return js.arrays(), NO_REORDER
    return make


def wide_case():
    """Windows of nine tiles (the WIDE instantiation), the junction in the first and in the last tile of both."""
    l = 8 * WT + 50
    js = Junctions(900)
    f = js.fusion(l, l, [3, 8 * WT + 2], [3, 8 * WT + 2], homology=2)
    g = js.fusion(l - 1, l - 3, [4 * WT + 30], [2 * WT + 30])
    for k in range(200):
        js.read(f if (k >> 6) & 1 else g, 50, 12 + k % 24)          # four runs: the workgroup is tier 0's
    return js.arrays(), 0


# ---- the tail replay ----

def one_side_case(side):
    """Most reads of the fusion have their junction in tiles (1, 1): that is the tile pair the workgroup agrees on and
    replays from its tables.  Every fifth read takes the second anchor on `side`, which lies two tiles further on: its
    task 0 has the agreed tile on the other side only (NO_CHUNK on this one)."""
    def make():
        l = 4 * WT
        js = Junctions(1000 + side)
        f = js.fusion(l, l, [WT + 5], [WT + 7], alt0=[3 * WT + 5] if side == 0 else (), alt1=[3 * WT + 7] if side == 1 else (), homology=1)
        for k in range(200):
            js.read(f, 50, 14 + k % 22, alt=((1, 0) if side == 0 else (0, 1)) if k % 5 == 4 else (0, 0))
        return js.arrays(), 0
    return make


def zero_stop_case():
    """The agreed tiles are (0, 2) for one fusion and (2, 0) for the other: the side in tile 0 has no tile to its left (stop 0,
    the bias), the other side reads the boundary of tile 1."""
    l = 3 * WT + 20
    js = Junctions(1100)
    f = js.fusion(l, l, [8], [2 * WT + 9], homology=2)
    g = js.fusion(l, l - 2, [2 * WT + 6], [10], homology=1)
    for k in range(200):
        js.read(f if (k >> 4) & 1 else g, 50, 13 + k % 23)
    return js.arrays(), 0


def mixed_stops_case():
    """A workgroup of four fusions in sixteen runs of 16 pairs (tier 1), so that every wave holds lanes of all four; their agreed tile
    pairs are (1, 3), (3, 1), (0, 2) and (2, 0): the lanes of one wave read the boundaries of different tiles, which stop
    at different row groups, on the two sides.  Reads of 30 to 76 bases."""
    l = 4 * WT
    js = Junctions(1200, anchor=50)
    fs = [js.fusion(l, l - k, [c0 * WT + 2], [c1 * WT + 1], homology=k % 2)
          for k, (c0, c1) in enumerate([(1, 3), (3, 1), (0, 2), (2, 0)])]
    for k in range(256):
        lq = 30 + (k * 5) % 47
        js.read(fs[(k >> 4) & 3], lq, lq // 2 - 4 + k % 9)
    return js.arrays(), NO_REORDER


KEPT_ROWS = {"kept-1": 1, "kept-3": KCACHE, "kept-4": KCACHE + 1, "kept-7": 7}


def kept_case(n_kept, n=200):
    """Microhomology of n_kept - 1 bases: n_kept read splits score the same, every pair has that many kept rows.  The first
    KCACHE are read from LDS, those past them from global memory."""
    def make():
        l = 2 * WT + 30
        js = Junctions(1300 + n_kept)
        f = js.fusion(l, l, [WT - 45], [WT + 4], homology=n_kept - 1)
        g = js.fusion(l - 3, l, [WT + 20], [6], homology=n_kept - 1)
        for k in range(n):
            js.read(f if (k >> 3) & 1 else g, 50, 12 + k % 24)
        return js.arrays(), 0
    return make


def partial_case(n_pairs):
    """The batch ends inside the second workgroup's first wave."""
    def make():
        l = 3 * WT + 30
        js = Junctions(1400 + n_pairs)
        f = js.fusion(l, l, [WT + 5], [2 * WT + 5], homology=KCACHE)
        for k in range(n_pairs):
            js.read(f, 40 + k % 11, 12 + k % 17)
        return js.arrays(), 0
    return make


CASES = {
    "lq-1": lq_case(1),
    "lq-3": lq_case(3),
    "lq-4": lq_case(4),
    "lq-5": lq_case(5),
    "lq-76": lq_case(76),
    "window-56": window_case(56),
    "window-57": window_case(57),
    "window-112": window_case(112),
    "window-389": window_case(389),
    "left-stops-early": left_stops_early_case,
    "late-resume": late_resume_case,
    "owner-tier0": owner_case(4),
    "owner-tier1": owner_case(10),
    "owner-tier2": owner_case(30),
    "owner-generic": owner_case(50),
    "wide-9": wide_case,
    "only-m2-tile": one_side_case(0),
    "only-m1-tile": one_side_case(1),
    "zero-stop": zero_stop_case,
    "mixed-stops": mixed_stops_case,
    "kept-1": kept_case(1),
    "kept-3": kept_case(KCACHE),
    "kept-4": kept_case(KCACHE + 1),
    "kept-7": kept_case(7),
    "pairs-289": partial_case(289),
}

# (dsa_timing.n_replay_tasks, n_generic_tasks) of every case, taken once with the library of the commit before this change
# (DEFUSE_DSA_LIB pointing at a build of it, profiles/loop_waits/task_counts.txt): the tile sets have not changed.
PARENT_TASKS = {
    "lq-1": (0, 0),
    "lq-3": (0, 0),
    "lq-4": (0, 0),
    "lq-5": (0, 0),
    "lq-76": (200, 0),
    "window-56": (200, 0),
    "window-57": (200, 0),
    "window-112": (200, 0),
    "window-389": (200, 0),
    "left-stops-early": (128, 0),
    "late-resume": (128, 0),
    "owner-tier0": (384, 128),
    "owner-tier1": (359, 103),
    "owner-tier2": (340, 84),
    "owner-generic": (343, 343),
    "wide-9": (272, 72),
    "only-m2-tile": (240, 40),
    "only-m1-tile": (240, 40),
    "zero-stop": (200, 0),
    "mixed-stops": (256, 0),
    "kept-1": (200, 0),
    "kept-3": (200, 0),
    "kept-4": (200, 0),
    "kept-7": (296, 96),
    "pairs-289": (289, 0),
}

_made = {}


def made(name):
    """The case's batch, its plan flags and the oracle's records: computed once, shared, never modified."""
    if name not in _made:
        from oracle import dosplitalign_oracle as ora
        batch, flags = CASES[name]()
        _made[name] = (batch, flags, ora.align_batch(*batch))
    return _made[name]


def splits_of(exp, p):
    return np.unique(exp["read_first"][exp["pair_idx"] == p])


def test_every_case_has_its_parent_counts():
    assert sorted(PARENT_TASKS) == sorted(CASES)


def test_cases_are_small():
    for name in CASES:
        assert 100 <= len(made(name)[0][3]) <= 300, name


@pytest.mark.parametrize("name", sorted(KEPT_ROWS))
def test_oracle_kept_rows(built, name):
    """The oracle alone: every pair of a microhomology case has the number of read splits (kept rows) it is named for, one,
    KCACHE, and more than KCACHE."""
    batch, _, exp = made(name)
    for p in range(len(batch[3])):
        assert len(splits_of(exp, p)) == KEPT_ROWS[name], (p, splits_of(exp, p))
    assert KEPT_ROWS["kept-3"] == KCACHE < KEPT_ROWS["kept-4"] < KEPT_ROWS["kept-7"]


def test_oracle_cases_reach_their_paths(built):
    """Read lengths, tile counts, runs and batch sizes are what the case names say; the planted junctions are found where
    they were planted."""
    tiles = lambda batch: -(-int(max(batch[1]["ref0_len"].max(), batch[1]["ref1_len"].max())) // WT)
    for lq in (1, 3, 4, 5, 76):
        batch, _, exp = made("lq-%d" % lq)
        assert set(batch[3]["read_len"].tolist()) == {lq} and (lq >> 2) + 1 == {1: 1, 3: 1, 4: 2, 5: 2, 76: 20}[lq]
        assert (len(exp) > 0) == (lq == 76)          # the short reads are below every minimum score: swept, no records
    for l, n in ((56, 1), (57, 2), (112, 2), (389, 7)):
        batch, _, exp = made("window-%d" % l)
        assert tiles(batch) == n and int(batch[1]["ref0_len"][0]) == l
        assert len(np.unique(exp["pair_idx"])) == len(batch[3])
    assert tiles(made("wide-9")[0]) == 9
    for name in ("left-stops-early", "late-resume"):
        batch, _, exp = made(name)
        assert len(batch[3]) == 128 and len(np.unique(exp["pair_idx"])) == 128 and set(batch[3]["read_len"].tolist()) == {76}
        assert bytes(batch[0][:WT]) == b"T" * WT and b"T" not in bytes(batch[2])          # tile 0 of M1: nothing a read could match
    # late-resume, first wave: the M1 part ends in tile 2 (column 2 * WT + 29), 23 to 26 of its rows lie there
    batch, _, exp = made("late-resume")
    assert set((exp["ref_first"][exp["pair_idx"] < 64] // WT).tolist()) == {2}
    for name, runs in OWNER_RUNS.items():
        batch = made(name)[0]
        f = batch[3]["fusion_idx"]
        assert len(f) == 256 and 1 + int(np.count_nonzero(np.diff(f))) == runs
    # the one-sided cases: every fifth read has its junction two tiles further on, on that side only
    for name, field in (("only-m2-tile", "ref_first"), ("only-m1-tile", "ref_second")):
        batch, _, exp = made(name)
        far = {int(p) for p in np.unique(exp["pair_idx"]) if np.ptp(exp[field][exp["pair_idx"] == p] // WT) == 0
               and abs(int(exp[field][exp["pair_idx"] == p][0]) // WT - int(exp[field][exp["pair_idx"] == 0][0]) // WT) == 2}
        assert far == set(range(4, 200, 5)), (name, sorted(far)[:8])
    batch, _, exp = made("mixed-stops")
    where = {(int(f), int(a) // WT) for f, a in zip(batch[3]["fusion_idx"][exp["pair_idx"]], exp["ref_first"])}
    assert where == {(0, 1), (1, 3), (2, 0), (3, 2)}, where
    assert len(made("pairs-289")[0][3]) == 289 and 289 % 256 < 64
    assert all(len(splits_of(made("pairs-289")[2], p)) == KCACHE + 1 for p in range(289))


@pytest.fixture(scope="module")
def ctx(built):
    from defuse_amd import dsa
    c = dsa.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_records_and_task_counts(ctx, name, monkeypatch):
    batch, flags, exp = made(name)
    monkeypatch.setenv("DEFUSE_DSA_TILE_COLS", str(WT))
    ctx.set_plan_options(flags)
    try:
        got = ctx.align_batch(*batch)
    finally:
        ctx.set_plan_options(0)
    t = ctx.timing()
    print("tasks", repr(name), (int(t.n_replay_tasks), int(t.n_generic_tasks)))
    assert ctx.tile_cols_in_use() == WT
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert (int(t.n_replay_tasks), int(t.n_generic_tasks)) == PARENT_TASKS[name]
    kc = ctx.kernel_counts()
    if name in OWNER_RUNS:
        tier = list(OWNER_RUNS).index(name)
        assert (kc["generic"] if tier == 3 else kc["fast"][tier]) == 1 and kc["generic"] + sum(kc["fast"]) + sum(kc["fast_wide"]) == 1, kc
    if name.startswith("window-") or name.startswith("lq-"):
        assert kc["fast"][0] == 1 and kc["generic"] == 0, kc
    if name == "wide-9":
        assert sum(kc["fast_wide"]) == 1 and sum(kc["fast"]) == 0 and kc["generic"] == 0, kc
