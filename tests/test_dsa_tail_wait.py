"""The fill kernels' tail - row maxima over the tiles, then the winning tiles of the kept rows - against the CPU oracle.

reduce_row_max loads a row group of every tile at once, a dead tile's slot reading the wave's longest-lived tile instead, and
keeps the next row groups' loads in flight; combine_wg looks the winning tiles of the kept rows up in the per-tile maxima, the
first three kept rows from registers.  What can go wrong there is decided by where tiles stop, how many row groups and tiles
a wave has, which lanes are shorter than the wave's longest read, and how many kept rows tie over how many tiles (the cases
were also run against a combine_wg that issues all those lookups at once, profiles/tail_wait).  The cases plant exactly that; every one
must be byte-equal to the oracle and must hand the replay the same number of tasks as the commit before the change (a tile
set that is too large still gives the right records).

Where a tile stops is decided by the pruning and is not visible from outside; the cases are built so that the stops differ
(see uneven_stops_case), the assertions are on records and task counts.
"""
import numpy as np
import pytest

from tests import cases

WT = 56          # every case runs at this tile width (DEFUSE_DSA_TILE_COLS)


class Junctions:
    """Fusions whose windows hold the two anchors of a junction read at chosen places.  Window 0 holds anchor A followed by
    the first `homology` bases of anchor B at every position of at0; window 1 holds B at every position of at1.  A read
    that leaves window 0 after `a` bases is A[-a:] + B[:lq - a]; with homology h it scores the same for h + 1 splits."""

    def __init__(self, seed, anchor=40, alphabet=b"ACGT"):
        self.rng = np.random.default_rng(seed)
        self.bb = cases.BatchBuilder()
        self.anchor = anchor
        self.alphabet = alphabet
        self.fus = []

    def fusion(self, l0, l1, at0, at1, homology=0, fill0=None, fill1=None):
        n = self.anchor
        A, B = cases.rnd(self.rng, n, self.alphabet), cases.rnd(self.rng, n, self.alphabet)
        ref0 = bytearray(cases.rnd(self.rng, l0))
        ref1 = bytearray(cases.rnd(self.rng, l1))
        for lo, hi, base in fill0 or ():
            ref0[lo:hi] = base * (hi - lo)
        for lo, hi, base in fill1 or ():
            ref1[lo:hi] = base * (hi - lo)
        other = lambda base: b"ACGT"[(b"ACGT".index(base) + 1) % 4]
        for p in at0:
            ref0[p:p + n + homology] = A + B[:homology]
            if p + n + homology < l0:        # the homology ends here, in every copy: no split scores the same by chance
                ref0[p + n + homology] = other(B[homology])
        for p in at1:
            ref1[p:p + n] = B
            if p > 0:
                ref1[p - 1] = other(A[-1])
        assert len(ref0) == l0 and len(ref1) == l1
        self.fus.append((A, B))
        return self.bb.add_fusion(bytes(ref0), bytes(ref1), fusion_id=5 * len(self.fus) + 2)

    def read(self, f, lq, a, exotic=None):
        A, B = self.fus[f]
        assert 0 <= a <= self.anchor and 0 <= lq - a <= self.anchor
        read = A[self.anchor - a:] + B[:lq - a]
        if exotic is not None:
            read = read[:2] + exotic + read[3:]
        assert len(read) == lq
        self.bb.add_read(f, read, read_end=len(self.bb.pairs) & 1, revcomp=(len(self.bb.pairs) >> 1) & 1)

    def arrays(self):
        return self.bb.arrays()


def rev_start(l1, r, n=40):
    """Where to put an anchor of n bases in window 1 so that it begins at column r of the reversed window M2 runs over."""
    return l1 - r - n


def uneven_stops_case():
    """One wave, reads of 76 bases (20 row groups), windows of four tiles.  Tile 0 of both matrices is a homopolymer no read
    has a base of: nothing in it is alive, it stops after its first row group, and the tile behind it lives.  The anchors
    straddle the boundary of tiles 1 and 2: tile 2 has nothing alive until the alignment comes in over its boundary column
    (a gap-skipped stretch inside a tile) and lives to the last row; tile 3 is random and stops in between."""
    l = 3 * WT + 40
    js = Junctions(1, anchor=60, alphabet=b"ACG")
    f = js.fusion(l, l, [2 * WT - 30], [rev_start(l, 2 * WT - 30, 60)], fill0=[(0, WT, b"T")], fill1=[(l - WT, l, b"T")])
    for k in range(64):
        js.read(f, 76, 20 + (k * 7) % 37)
    return js.arrays(), 0


def lq_case(lqs, n=70):
    """Reads of the given lengths (cycled) over windows of two tiles whose anchors straddle the tile boundary."""
    def make():
        js = Junctions(20 + sum(lqs))
        f = js.fusion(100, 100, [WT - 20], [rev_start(100, WT - 20)])
        for k in range(n):
            lq = lqs[k % len(lqs)]
            js.read(f, lq, lq // 2)
        return js.arrays(), 0
    return make


def tiles_case(n_tiles):
    """Windows of n_tiles tiles, the anchors in the first and in the last tile of both (a tie over two tiles), three kept rows;
    a second fusion one base shorter without a tie."""
    def make():
        l = (n_tiles - 1) * WT + 50 if n_tiles > 1 else 50
        js = Junctions(100 + n_tiles)
        for k in range(2):
            far = [(n_tiles - 1) * WT + 2] if (k == 0 and n_tiles > 1) else []
            lk = l - k
            at1 = [rev_start(lk, r) for r in [3] + far]
            f = js.fusion(lk, lk, [3] + far, at1, homology=2 if n_tiles > 1 else 0)
            for a in range(12, 36, 3):
                js.read(f, 50, a)
        return js.arrays(), 0
    return make


def narrow_wave_case():
    """A workgroup whose first wave has windows of two tiles and whose second has windows of seven: for the first wave the
    tiles from the third on have stop 0."""
    from defuse_amd import dsa
    js = Junctions(7)
    narrow = js.fusion(2 * WT - 6, 2 * WT - 9, [WT - 20], [rev_start(2 * WT - 9, 4)], homology=1)
    wide = js.fusion(389, 389, [3 * WT - 10], [rev_start(389, 5 * WT + 3)], homology=2)
    for k in range(64):
        js.read(narrow, 50, 12 + k % 25)
    for k in range(50):
        js.read(wide, 60, 22 + k % 17)
    return js.arrays(), dsa.PLAN_NO_REORDER


TIES = {"tie-2x2": (2, 2), "tie-3x3": (3, 3), "tie-2x3": (2, 3), "tie-3x2": (3, 2)}
TIE_HOMOLOGY = 2     # three kept rows


def tie_case(n0, n1, n=20):
    """Windows of four tiles; the junction lies in n0 tiles of window 0 and in n1 tiles of window 1, with two bases of
    homology: three kept rows, each attained in n0 tiles of M1 and n1 tiles of M2.  The tiles without a copy are random and
    stop long before the kept rows, which lie in row groups 3 to 9."""
    def make():
        l = 3 * WT + 30
        js = Junctions(40 + 4 * n0 + n1)
        f = js.fusion(l, l, [c * WT + 5 for c in range(n0)], [rev_start(l, c * WT + 5) for c in range(n1)], homology=TIE_HOMOLOGY)
        for k in range(n):
            js.read(f, 50, 12 + k % 24)
        return js.arrays(), 0
    return make


def generic_owner_case():
    """Two workgroups in the caller's order; one read of the second has a byte outside A/C/G/T/N, which hands that workgroup
    to the generic kernel and its copy of the reduction.  The batch ends inside the second workgroup's third wave."""
    from defuse_amd import dsa
    l = 3 * WT + 30
    js = Junctions(9)
    fs = [js.fusion(l, l - k, [c * WT + 5 for c in range(1 + k % 2)], [rev_start(l - k, 5)], homology=k) for k in range(3)]
    for k in range(256 + 150):
        js.read(fs[k * 3 // 256 if k < 256 else (2 if k < 330 else 1)], 50, 12 + k % 24, exotic=b"R" if k == 300 else None)
    return js.arrays(), dsa.PLAN_NO_REORDER


def partial_case(n_pairs):
    def make():
        l = 3 * WT + 30
        js = Junctions(300 + n_pairs)
        f = js.fusion(l, l, [5, 2 * WT + 5], [rev_start(l, 5)], homology=1)
        for k in range(n_pairs):
            js.read(f, 40 + k % 11, 12 + k % 17)
        return js.arrays(), 0
    return make


CASES = {
    "uneven-stops": uneven_stops_case,
    "lq-1": lq_case([1]),
    "lq-3": lq_case([3]),
    "lq-4": lq_case([4]),
    "lq-7": lq_case([7]),
    "lq-8": lq_case([8]),
    "lq-mixed": lq_case([76, 9, 33, 12, 50, 20, 61, 16, 45]),
    "tiles-1": tiles_case(1),
    "tiles-7": tiles_case(7),
    "tiles-8": tiles_case(8),
    "tiles-9": tiles_case(9),
    "tiles-16": tiles_case(16),
    "tiles-17": tiles_case(17),
    "narrow-wave": narrow_wave_case,
    "tie-2x2": tie_case(2, 2),
    "tie-3x3": tie_case(3, 3),
    "tie-2x3": tie_case(2, 3),
    "tie-3x2": tie_case(3, 2),
    "generic-owner": generic_owner_case,
    "pairs-257": partial_case(257),
    "pairs-300": partial_case(300),
    "pairs-37": partial_case(37),
}

# (dsa_timing.n_replay_tasks, n_generic_tasks) of every case, taken once with the library of the commit before this change
# (DEFUSE_DSA_LIB pointing at a build of it): the tile sets have not changed.
PARENT_TASKS = {
    "uneven-stops": (64, 0),
    "lq-1": (0, 0),
    "lq-3": (0, 0),
    "lq-4": (0, 0),
    "lq-7": (0, 0),
    "lq-8": (70, 0),
    "lq-mixed": (70, 0),
    "tiles-1": (16, 0),
    "tiles-7": (24, 8),
    "tiles-8": (24, 8),
    "tiles-9": (24, 8),
    "tiles-16": (24, 8),
    "tiles-17": (24, 8),
    "narrow-wave": (114, 0),
    "tie-2x2": (40, 20),
    "tie-3x3": (60, 40),
    "tie-2x3": (60, 40),
    "tie-3x2": (60, 40),
    "generic-owner": (567, 311),
    "pairs-257": (514, 257),
    "pairs-300": (600, 300),
    "pairs-37": (74, 37),
}

_made = {}


def made(name):
    """The case's batch, its plan flags and the oracle's records: computed once, shared, never modified."""
    if name not in _made:
        from oracle import dosplitalign_oracle as ora
        batch, flags = CASES[name]()
        _made[name] = (batch, flags, ora.align_batch(*batch))
    return _made[name]


def test_every_case_has_its_parent_counts():
    assert sorted(PARENT_TASKS) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(TIES))
def test_oracle_ties_over_the_intended_tiles(built, name):
    """The oracle alone: every pair of a tie case has three read splits (kept rows), and at each of them its records lie in
    as many places of window 0 / window 1 as planted, every two of them at least a tile apart - in different tiles."""
    batch, _, exp = made(name)
    n0, n1 = TIES[name]
    for p in range(len(batch[3])):
        mine = exp[exp["pair_idx"] == p]
        splits = np.unique(mine["read_first"])
        assert len(splits) == TIE_HOMOLOGY + 1, (p, splits)
        for s in splits:
            for field, want in (("ref_first", n0), ("ref_second", n1)):
                places = np.unique(mine[field][mine["read_first"] == s])
                assert len(places) == want and (want == 1 or int(np.diff(places).min()) >= WT), (p, s, field, places)


def test_oracle_cases_reach_their_paths(built):
    """Tile counts, read lengths and batch sizes are what the case names say; the planted junctions are found."""
    for n in (1, 7, 8, 9, 16, 17):
        batch, _, exp = made("tiles-%d" % n)
        assert -(-int(max(batch[1]["ref0_len"].max(), batch[1]["ref1_len"].max())) // WT) == n
        assert len(np.unique(exp["pair_idx"])) == len(batch[3])
        if n > 1:      # the first fusion's reads: three kept rows, each in the first and the last tile of both windows
            mine = exp[exp["pair_idx"] == 0]
            assert len(np.unique(mine["read_first"])) == 3
            for field in ("ref_first", "ref_second"):
                assert int(np.ptp(mine[field])) > (n - 2) * WT
    for lq in (1, 3, 4, 7, 8):
        assert set(made("lq-%d" % lq)[0][3]["read_len"].tolist()) == {lq}
    assert len(set(made("lq-mixed")[0][3]["read_len"][:64].tolist())) == 9
    batch, _, exp = made("narrow-wave")
    assert [-(-int(x) // WT) for x in batch[1]["ref0_len"]] == [2, 7] and len(np.unique(exp["pair_idx"])) == len(batch[3])
    batch, _, exp = made("uneven-stops")
    assert len(batch[3]) == 64 and len(np.unique(exp["pair_idx"])) == 64
    assert sum(bytes(made("generic-owner")[0][2]).count(b) for b in b"R") == 1
    for n in (257, 300, 37):
        assert len(made("pairs-%d" % n)[0][3]) == n and n % 64 != 0


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
    if name == "generic-owner":
        assert kc["generic"] == 1 and sum(kc["fast"]) + sum(kc["fast_wide"]) == 1, kc
    if name.startswith("tiles-"):
        n = int(name.split("-")[1])
        assert sum(kc["fast_wide"]) == (1 if 9 <= n <= 16 else 0) and sum(kc["fast"]) == (0 if 9 <= n <= 16 else 1), kc
