"""The winning tiles of a pair, looked up in the per-tile row maxima at its kept rows, against the CPU oracle byte for byte.

The fill kernels' combine step keeps the read splits of the best score (the kept rows) and asks, per kept row and side, which
tiles of the window attain the row maximum: those tiles are replayed to enumerate the tied columns.  The cases here plant what
decides that set: the same anchor in the first and in the last tile of a window (a tie across tiles at a kept row), a junction
with microhomology (more kept rows than the KCACHE = 3 that stay in registers), late splits whose other tiles were pruned long
before the kept row, pairs without any kept row, windows of 8, 9, 16, 17 and more than 64 tiles, batches that end inside a wave,
and every kernel that can own a workgroup.  A tile set that is too large still gives the right records, so every case also
pins the number of replay tasks.
"""
import numpy as np
import pytest

from tests import cases

ANCHOR = 40
LQ = 50


def tiles_of(length, wt):
    return (length + wt - 1) // wt


def window_of_tiles(n, last_cols=1):
    """The shortest window that has n tiles, the last of them last_cols wide if a width allows it, at the tile width an upload
    of such windows runs with (dsa_tile_cols_for)."""
    from defuse_amd import dsa
    fallback = None
    for length in range(2 * ANCHOR + 20, 64 * n + 1):
        wt = dsa.tile_cols_for(length)
        if tiles_of(length, wt) == n:
            if length == (n - 1) * wt + last_cols:
                return length, wt
            fallback = fallback or (length, wt)
    assert fallback is not None, n
    return fallback


class Planted:
    """Fusions whose windows hold the read's anchor once or twice.  Window 0 has anchor A in its first tile (columns 5..44)
    and, for tie0, again in its last columns: the M1 row maximum of a read that leaves window 0 at A's end is attained in the
    first and in the last tile.  Window 1 begins with anchor B and, for tie1, has it again 50 bases before its end: M2 runs
    over the reversed window, so those are its last and its first tile.  homology: window 0 goes on behind the first A with
    the bases B begins with, so the read can leave window 0 at homology + 1 places with the same score."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.bb = cases.BatchBuilder()
        self.fus = []

    def fusion(self, l0, l1, tie0=False, tie1=False, homology=0):
        rng = self.rng
        A, B = cases.rnd(rng, ANCHOR), cases.rnd(rng, ANCHOR)
        ref0 = bytearray(cases.rnd(rng, l0))
        ref1 = bytearray(cases.rnd(rng, l1))
        ref0[5:5 + ANCHOR] = A
        ref0[5 + ANCHOR:5 + ANCHOR + homology] = B[:homology]
        if tie0:
            ref0[l0 - ANCHOR:] = A
        ref1[:ANCHOR] = B
        if tie1:
            ref1[l1 - 50:l1 - 50 + ANCHOR] = B
        assert len(ref0) == l0 and len(ref1) == l1
        self.fus.append((A, B))
        return self.bb.add_fusion(bytes(ref0), bytes(ref1), fusion_id=7 * len(self.fus) + 1)

    def read(self, f, a=None, exotic=None):
        A, B = self.fus[f]
        a = int(self.rng.integers(12, 39)) if a is None else a
        read = A[ANCHOR - a:] + B[:LQ - a]
        if exotic is not None:
            read = read[:3] + exotic + read[4:]
        self.bb.add_read(f, read, read_end=len(self.bb.pairs) & 1, revcomp=(len(self.bb.pairs) >> 1) & 1)

    def arrays(self):
        return self.bb.arrays()


TIES = ((True, False), (False, True), (True, True))


TIE_WT = 56      # the tie cases run at this tile width (DEFUSE_DSA_TILE_COLS), whatever the picker takes for their windows


def tie_case(tie0, tie1, homology=0, n=6):
    """One fusion with windows of two tiles and one column."""
    def make():
        length = 2 * TIE_WT + 1
        pl = Planted(11 + 2 * tie0 + tie1 + 5 * homology)
        f = pl.fusion(length, length, tie0, tie1, homology)
        for _ in range(n):
            pl.read(f)
        return pl.arrays(), 0
    return make


def tiles_case(n_tiles):
    """Windows of n_tiles tiles with the anchors in the first and the last tile of both, and two fusions without a tie."""
    def make():
        length, _ = window_of_tiles(n_tiles)
        pl = Planted(100 + n_tiles)
        for k in range(3 if n_tiles <= 64 else 1):
            f = pl.fusion(length, length - (k % 2), k == 0, k == 0, homology=4 if k == 2 else 0)
            for a in ((14, 25, 37) if n_tiles > 64 else range(12, 39, 3)):
                pl.read(f, a)
        return pl.arrays(), 0
    return make


def batch_case(n_pairs):
    def make():
        length, _ = window_of_tiles(3)
        pl = Planted(200 + n_pairs)
        f = pl.fusion(length, length, True, True, homology=5)
        for _ in range(n_pairs):
            pl.read(f)
        return pl.arrays(), 0
    return make


def headline_case():
    """Windows of 389 bases, reads of 76, one fusion: splits at every depth, the deep ones long after the tiles that do not
    hold the junction have stopped."""
    rng = np.random.default_rng(5)
    bb = cases.BatchBuilder()
    r0, r1 = cases.rnd(rng, 389), cases.rnd(rng, 389)
    f = bb.add_fusion(r0, r1)
    for k in range(300):
        a = (9 + k) % 68 if k % 3 else 60 + k % 8
        bb.add_read(f, cases.mutate(rng, cases.split_read(rng, r0, r1, 76, a=a), 0.01))
    return bb.arrays(), 0


def no_kept_row_case(empty_window):
    """Reads wholly inside window 0 of a fusion whose window 1 has none of their bases (no column of M2 reaches the least
    split score) and random decoys; or reads of a fusion that has a window of no bases: no pair has a kept row."""
    def make():
        rng = np.random.default_rng(6)
        bb = cases.BatchBuilder()
        r0, e0 = cases.rnd(rng, 200, b"CGT"), cases.rnd(rng, 150)
        if empty_window:
            e = bb.add_fusion(e0, b"")
        else:
            f = bb.add_fusion(r0, b"A" * 180)
            d = bb.add_fusion(cases.rnd(rng, 200), cases.rnd(rng, 180))
        for k in range(40):
            if empty_window:
                bb.add_read(e, e0[k:k + LQ])
            else:
                bb.add_read(f, r0[3 * k:3 * k + LQ])
                bb.add_read(d, cases.rnd(rng, LQ))
        return bb.arrays(), 0
    return make


def owners_case():
    """Workgroups (in the caller's order) of 3, 10, 30 and 50 fusions and one of 2 fusions with a read byte outside
    A/C/G/T/N: table tiers 0, 1, 2 and twice the generic kernel; every third fusion ties in window 0, in window 1, in both."""
    from defuse_amd import dsa
    length, _ = window_of_tiles(3)
    pl = Planted(300)
    pool = [pl.fusion(length, length - (k % 3), *TIES[k % 3], homology=(k % 5) if k % 2 else 0) for k in range(50)]
    for n_fus, exotic in ((3, None), (10, None), (30, None), (50, None), (2, b"R")):
        cut = np.linspace(0, 256, n_fus + 1).astype(int)
        for k in range(n_fus):
            for j in range(cut[k], cut[k + 1]):
                pl.read(pool[k], exotic=exotic if j == 128 else None)
    return pl.arrays(), dsa.PLAN_NO_REORDER


CASES = {
    "tie-window0": tie_case(True, False),
    "tie-window1": tie_case(False, True),
    "tie-both": tie_case(True, True),
    "homology-5": tie_case(False, False, homology=5),
    "homology-5-tie-both": tie_case(True, True, homology=5),
    "headline-late-splits": headline_case,
    "no-kept-row": no_kept_row_case(False),
    "no-kept-row-empty-window": no_kept_row_case(True),
    "tiles-8": tiles_case(8),
    "tiles-9": tiles_case(9),
    "tiles-16": tiles_case(16),
    "tiles-17": tiles_case(17),
    "tiles-65": tiles_case(65),
    "pairs-1": batch_case(1),
    "pairs-63": batch_case(63),
    "pairs-65": batch_case(65),
    "pairs-257": batch_case(257),
    "owners": owners_case,
}
TIE_CASES = {"tie-window0": (True, False), "tie-window1": (False, True), "tie-both": (True, True),
             "homology-5-tie-both": (True, True), "pairs-63": (True, True)}
FORCED_WT = {name: TIE_WT for name in CASES if name.startswith(("tie-", "homology-"))}

# (dsa_timing.n_replay_tasks, n_generic_tasks) of every case, taken once with the library of the commit before the winning
# tiles were looked up at the kept rows (DEFUSE_DSA_LIB pointing at a build of it): the tile sets have not changed.
PARENT_TASKS = {
    "tie-window0": (12, 6),
    "tie-window1": (12, 6),
    "tie-both": (12, 6),
    "homology-5": (12, 6),
    "homology-5-tie-both": (18, 12),
    "headline-late-splits": (430, 297),
    "no-kept-row": (0, 0),
    "no-kept-row-empty-window": (0, 0),
    "tiles-8": (36, 9),
    "tiles-9": (36, 9),
    "tiles-16": (45, 18),
    "tiles-17": (36, 9),
    "tiles-65": (195, 195),
    "pairs-1": (2, 1),
    "pairs-63": (126, 63),
    "pairs-65": (130, 65),
    "pairs-257": (514, 257),
    "owners": (2560, 1792),
}

_made = {}


def made(name):
    """The case's batch, its plan flags and the oracle's records: computed once, shared, never modified."""
    if name not in _made:
        from oracle import dosplitalign_oracle as ora
        batch, flags = CASES[name]()
        _made[name] = (batch, flags, ora.align_batch(*batch))
    return _made[name]


@pytest.mark.parametrize("name", sorted(TIE_CASES))
def test_oracle_ties_across_tiles_at_one_split(built, name):
    """The oracle alone: every pair of a tie case has, for one read split, two records further apart than a tile is wide on
    the tied side - without that the GPU cases would not reach the lookup's several-winners path."""
    from defuse_amd import dsa
    batch, _, exp = made(name)
    wt = FORCED_WT.get(name) or dsa.tile_cols_for(int(max(batch[1]["ref0_len"].max(), batch[1]["ref1_len"].max())))
    assert tiles_of(int(batch[1]["ref0_len"][0]), wt) == 3
    for p in range(len(batch[3])):
        mine = exp[exp["pair_idx"] == p]
        for side, field in enumerate(("ref_first", "ref_second")):
            if not TIE_CASES[name][side]:
                continue
            spread = max(int(np.ptp(mine[field][mine["read_first"] == s])) for s in np.unique(mine["read_first"]))
            assert spread > wt, (p, field, spread)


def test_oracle_cases_reach_their_paths(built):
    """More kept rows than KCACHE, and no record where no row is kept."""
    _, _, exp = made("homology-5")
    assert all(len(np.unique(exp["read_first"][exp["pair_idx"] == p])) >= 6 for p in range(6))
    assert len(made("no-kept-row")[2]) == 0 and len(made("no-kept-row-empty-window")[2]) == 0
    assert len(made("headline-late-splits")[2]) >= 250


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
    if name in FORCED_WT:
        monkeypatch.setenv("DEFUSE_DSA_TILE_COLS", str(FORCED_WT[name]))
    ctx.set_plan_options(flags)
    try:
        got = ctx.align_batch(*batch)
    finally:
        ctx.set_plan_options(0)
    t = ctx.timing()
    print("tasks", name, (int(t.n_replay_tasks), int(t.n_generic_tasks)))
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert (int(t.n_replay_tasks), int(t.n_generic_tasks)) == PARENT_TASKS[name]
    kc = ctx.kernel_counts()
    if name in FORCED_WT:
        assert ctx.tile_cols_in_use() == FORCED_WT[name]
    if name == "owners":
        assert (kc["fast"], kc["fast_wide"], kc["generic"]) == ([1, 1, 1], [0, 0, 0], 2), kc
    if name.startswith("tiles-"):
        n = int(name.split("-")[1])
        assert sum(kc["fast_wide"]) == (1 if 9 <= n <= 16 else 0) and sum(kc["fast"]) == (0 if 9 <= n <= 16 else 1), kc
