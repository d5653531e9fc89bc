"""The table-driven sweeps and the table-driven tail replay with a drift of period four (dsa_kernels.hpp, drift_of).

A tile's column i lives in a register in the frame V + 1024 + d(i).  The generic kernels let d(i) = 2i run over the whole
tile; the table kernels use d(i) = 2 (i mod 4): the move from the left neighbour is free inside a quad of columns, the frame
wraps once per quad (X[4q-1] - 8 enters column 4q, the table term of column 4q carries -6), and the tile's row maximum is
taken per residue and rebased once.  Nothing that is stored may change by that, so every GPU case here must be byte-equal to
the CPU oracle and must hand the replay kernels as many tasks as the commit before the change did.

What can go wrong is decided by where a value sits relative to a quad wrap and a tile edge (winning columns at residue 0 and
3, at a tile's first and last column, ties across a wrap), by the padding of a last tile (1, 3, 4, 5 valid columns: padding
at every residue), by the three tile widths (56, 60 = fifteen quads, the odd one folded on its own, 64), by the two table
encodings (25-row tables: tier 0; split tables joined by v_perm: tiers 1 and 2) beside a workgroup of the generic kernel, by
table rows with an N, by fields at the floor (decoys: candidates below 1024 at wrap columns) and far above it (reads of 300),
and by the gap-skip resume, which sets the registers up a second time.

The CPU test is a model of one tile row in both frames, both fields in one 32-bit word, with both table encodings.
"""
import numpy as np
import pytest

from tests import cases
from tests.test_dsa_loop_waits import Junctions

NO_REORDER = 1   # dsa.PLAN_NO_REORDER: pair p is thread p % 256 of workgroup p // 256
BIAS = 1024


# ---------------------------------------------------------------------------------------------
# CPU: one tile row, period 56 (the drift runs over the tile) against period 4
# ---------------------------------------------------------------------------------------------

def pack(lo, hi):
    return np.uint32((int(lo) & 0xFFFF) | ((int(hi) & 0xFFFF) << 16))


def fields(x):
    return int(x) & 0xFFFF, (int(x) >> 16) & 0xFFFF


def add32(a, b):
    return np.uint32((int(a) + int(b)) & 0xFFFFFFFF)      # v_add_u32: the carry out of the word is dropped


def fmax(flush, *xs):
    """Per-field maximum as v_pk_maximum3_f16 orders positive patterns; flush: patterns below the smallest normal read as 0."""
    los, his = zip(*(fields(x) for x in xs))
    f = (lambda v: 0 if v < BIAS else v) if flush else (lambda v: v)
    return pack(max(map(f, los)), max(map(f, his)))


def drift(period, i):
    return 2 * (i % period)


def tables(terms_lo, terms_hi, period):
    """The row's table words: ('sum') the exact 32-bit two's complement sum lo + (hi << 16), as the 25-row tables hold it, and
    ('perm') the split tables' 16-bit halves joined as v_perm does, the upper half one short where the lower one is negative."""
    exact, joined = [], []
    for i, (lo, hi) in enumerate(zip(terms_lo, terms_hi)):
        dd = 0 if i == 0 else drift(period, i) - drift(period, i - 1)
        exact.append(np.uint32((lo + dd + ((hi + dd) << 16)) & 0xFFFFFFFF))
        half_lo = (lo + dd) & 0xFFFF
        half_hi = (hi + dd - (1 if lo + dd < 0 else 0)) & 0xFFFF
        joined.append(np.uint32(half_lo | (half_hi << 16)))
    return exact, joined


def row_step(X, T, bprev, bcur, period, flush):
    """One row of sweep_tile_fast over the registers X (in place): returns (tile row maximum, outgoing boundary), Z frame."""
    nw = len(X)
    const2 = lambda v: pack(v, v)
    a = add32(bprev, T[0])
    up = np.uint32(int(bcur) - int(const2(2)))
    for i in range(nw):
        an = add32(X[i], T[i + 1]) if i + 1 < nw else None
        X[i] = fmax(flush, a, X[i], up)
        a = an
        up = X[i]
        if (i + 1) % period == 0 and i + 1 < nw:
            up = np.uint32(int(X[i]) - int(const2(2 * period)))       # the frame wraps
    if period >= nw:                                                     # every column rebased, then compared
        m = const2(BIAS)
        for i in range(nw):
            m = fmax(flush, m, np.uint32(int(X[i]) - int(const2(drift(period, i)))))
    else:                                                                # one accumulator per residue, rebased at the end
        acc = [const2(BIAS)] * period
        for i in range(nw):
            acc[i % period] = fmax(flush, acc[i % period], X[i])
        m = const2(BIAS)
        for k in range(period):
            m = fmax(flush, m, np.uint32(int(acc[k]) - int(const2(2 * k))))
    return m, np.uint32(int(X[nw - 1]) - int(const2(drift(period, nw - 1))))


@pytest.mark.parametrize("nw", [56, 60, 64])
def test_one_tile_row_in_both_frames(nw):
    """Random rows over a tile with padding, from the floor upwards: the same Z-frame values, tile maxima and boundary in the
    frame of period nw (one frame per column), of period 4 with exact-sum tables and of period 4 with joined halves, whether
    or not patterns below 1024 are flushed."""
    rng = np.random.default_rng(nw)
    saw_negative = saw_carry = saw_low = 0
    for trial in range(6):
        nv0, nv1 = (int(v) for v in rng.integers(1, nw + 1, 2)) if trial else (nw, nw - 3)
        ref = rng.integers(0, 4, (2, nw))
        decoy = trial % 3 == 2                                        # nothing matches: every field stays near the floor
        frames = [(nw, "sum", False), (4, "sum", False), (4, "perm", False), (4, "sum", True), (4, "perm", True)]
        Xs = [[pack(BIAS + drift(p, i), BIAS + drift(p, i)) for i in range(nw)] for p, _, _ in frames]
        bprev = pack(BIAS, BIAS)
        for j in range(1, 41):
            base = rng.integers(0, 4, 2) if not decoy else (9, 9)
            lo = [0 if i >= nv0 else 4 if ref[0, i] == base[0] else 1 for i in range(nw)]
            hi = [0 if i >= nv1 else 4 if ref[1, i] == base[1] else 1 for i in range(nw)]
            bcur = pack(BIAS + int(rng.integers(0, 3 * j + 1)), BIAS + int(rng.integers(0, 3 * j + 1))) if trial % 2 else pack(BIAS, BIAS)
            out = []
            for (period, enc, flush), X in zip(frames, Xs):
                exact, joined = tables(lo, hi, period)
                assert [int(v) for v in exact] == [int(v) for v in joined]    # the halves join to the exact sum
                if period == 4:
                    saw_negative += sum(1 for i in range(4, nw, 4) if lo[i] - 6 < 0)
                    saw_carry += sum(1 for i in range(4, nw, 4) if (int(joined[i]) >> 16) == ((hi[i] - 7) & 0xFFFF))
                    saw_low += sum(1 for i in range(3, nw - 1, 4) if min(fields(X[i])) - 8 < BIAS)
                m, b = row_step(X, exact if enc == "sum" else joined, bprev, bcur, period, flush)
                z = [tuple(v - BIAS - drift(period, i) for v in fields(x)) for i, x in enumerate(X)]
                out.append((z, fields(m), fields(b)))
            for o in out[1:]:
                assert o == out[0], (trial, j)
            z, m, b = out[0]
            assert all(v >= 0 for zz in z for v in zz)
            assert m == (BIAS + max(v[0] for v in z), BIAS + max(v[1] for v in z)) and b == (BIAS + z[-1][0], BIAS + z[-1][1])
            # padded columns never exceed the valid ones: the unmasked maximum is the valid columns' maximum
            assert m[0] == BIAS + max(v[0] for v in z[:nv0]) and m[1] == BIAS + max(v[1] for v in z[:nv1])
            bprev = bcur
    assert saw_negative and saw_carry and saw_low      # negative wrap terms, a carrying low half, candidates below 1024


def test_wrap_terms_of_the_split_tables():
    """Every (lo, hi) of {padding, mismatch, match}^2 at a wrap column: the joined halves are the exact sum, and adding it to
    fields at the floor of a residue-3 column gives both fields exactly."""
    for lo in (0, 1, 4):
        for hi in (0, 1, 4):
            exact, joined = tables([4] * 4 + [lo] + [1] * 3, [1] * 4 + [hi] + [4] * 3, 4)
            assert int(exact[4]) == int(joined[4]) == ((hi - 7) & 0xFFFF) << 16 | ((lo - 6) & 0xFFFF)
            for x_lo, x_hi in ((BIAS + 6, BIAS + 6), (BIAS + 6, 31000), (31000, BIAS + 6)):
                assert fields(add32(pack(x_lo, x_hi), joined[4])) == (x_lo + lo - 6, x_hi + hi - 6)


# ---------------------------------------------------------------------------------------------
# GPU cases
# ---------------------------------------------------------------------------------------------

def junction_reads(bb, rng, f, ref0, ref1, n, lq, firsts, n_rate=0.0, mutate=0.0, one_junction=False):
    """n reads of fusion f that leave window 0 after column first - 1 for the given values of `first`, in turn, and enter
    window 1 anywhere.  one_junction: all reads of the fusion cross at the same place, firsts[f % len(firsts)] and a start in
    window 1 that the fusion fixes, and differ in where the read is split.  Workgroups of more than four fusions and windows
    of more than eight tiles take the FIRST pair's offer of a tile pair for a fusion's table-driven replay, and which pair
    is first depends on the order the waves arrive in: only where all pairs of a fusion offer the same tiles is the number
    of tasks left to the generic replay the same in every run."""
    s1_fixed = int(rng.integers(0, max(1, len(ref1) - lq)))
    for k in range(n):
        first = firsts[(f if one_junction else k) % len(firsts)]
        a = min(first, lq // 2 - 6 + k % 13)
        s1 = s1_fixed if one_junction else int(rng.integers(0, max(1, len(ref1) - lq)))
        read = cases.split_read(rng, ref0, ref1, lq, first=first, s1=s1, a=a)
        if mutate:
            read = cases.mutate(rng, read, mutate)
        if n_rate and k % int(1 / n_rate) == 0:
            b = bytearray(read)
            b[(7 * k) % len(b)] = ord("N")
            read = bytes(b)
        bb.add_read(f, read, read_end=k & 1, revcomp=(k >> 1) & 1)


def width_case(windows, wt, lq, n_fusions, n_reads, seed, one_junction=False):
    """Windows that make the upload pick tile width wt; junctions at a tile's first and last column, at residues 0 and 3."""
    def make():
        rng = np.random.default_rng(seed)
        bb = cases.BatchBuilder()
        for k in range(n_fusions):
            l = windows[k % len(windows)]
            ref0, ref1 = cases.rnd(rng, l), cases.rnd(rng, l - k)
            f = bb.add_fusion(ref0, ref1)
            t = wt * (1 + (lq // 2 + 6) // wt)            # the first tile boundary the longest M1 part fits in front of
            firsts = [c for c in (t, t + 1, t + 3, t + 4, t + 5, t + wt, l - 1, l) if c <= l]
            junction_reads(bb, rng, f, ref0, ref1, n_reads, lq, firsts, mutate=0.02, one_junction=one_junction)
        return bb.arrays(), 0, wt
    return make


def tiers_case():
    """Four workgroups in the caller's order: 100 + 100 + 56 reads of three fusions (tier 0), sixteen fusions of 16 reads
    (tier 1), 36 fusions of 7 reads and one of 4 (tier 2), and 255 reads of two fusions with one read that has a byte
    outside ACGTN (the generic kernel)."""
    rng = np.random.default_rng(77)
    bb = cases.BatchBuilder()
    runs = [100, 100, 56] + [16] * 16 + [7] * 36 + [4] + [128, 128]
    for k, n in enumerate(runs):
        l0, l1 = 150 + k % 9, 140 + k % 11
        ref0, ref1 = cases.rnd(rng, l0), cases.rnd(rng, l1)
        f = bb.add_fusion(ref0, ref1)
        junction_reads(bb, rng, f, ref0, ref1, n, 50, [56, 57, 59, 60, 61, 112, 113, l0], one_junction=True)
    arrays = bb.arrays()
    arrays[2][int(arrays[3]["read_off"][-1]) + 5] = ord("R")
    return arrays, NO_REORDER, 56


def n_case():
    """Every fourth read has an N (table rows 16..24 and the split tables' fifth class), the windows a few as well."""
    rng = np.random.default_rng(78)
    bb = cases.BatchBuilder()
    for k in range(3):
        ref0, ref1 = bytearray(cases.rnd(rng, 130)), bytearray(cases.rnd(rng, 125))
        ref0[57 + k] = ref1[60] = ord("N")
        f = bb.add_fusion(bytes(ref0), bytes(ref1))
        junction_reads(bb, rng, f, bytes(ref0), bytes(ref1), 80, 50, [56, 57, 59, 60, 116], n_rate=0.25)
    return bb.arrays(), 0, 56


def n_split_case():
    """The same with ten fusions in the workgroup: the split tables."""
    rng = np.random.default_rng(79)
    bb = cases.BatchBuilder()
    for k in range(10):
        ref0, ref1 = cases.rnd(rng, 120), cases.rnd(rng, 118)
        f = bb.add_fusion(ref0, ref1)
        junction_reads(bb, rng, f, ref0, ref1, 25, 50, [56, 57, 59, 60, 116], n_rate=0.25, one_junction=True)
    return bb.arrays(), NO_REORDER, 56


def last_tile_case(l):
    """Windows of l bases at tile width 56: 40 and 56 are one tile, 57, 59, 60 and 61 leave 1, 3, 4 and 5 valid columns in
    the last tile (padding from every residue on); junctions in the last columns that exist."""
    def make():
        rng = np.random.default_rng(100 + l)
        bb = cases.BatchBuilder()
        for k in range(2):
            ref0, ref1 = cases.rnd(rng, l), cases.rnd(rng, l)
            f = bb.add_fusion(ref0, ref1)
            junction_reads(bb, rng, f, ref0, ref1, 70, 44, [l, l - 1, max(l - 4, 22), max(l - 5, 22), min(l, 56)])
        return bb.arrays(), 0, 56
    return make


def junction_column_case(residue_first):
    """Every read leaves window 0 after `first` bases with first = 56 + residue_first (mod 56: 0 the tile's last column and
    residue 3, 1 its first column and residue 0, 3, 4, 5) or one tile further, and enters window 1 the same way.  Five runs of pairs: the split tables."""
    def make():
        js = Junctions(300 + residue_first, anchor=40)
        at = 56 + residue_first - 40                   # anchor A ends at column at + 39 (0-based): first = at + 40
        f = js.fusion(180, 180, [at], [at], homology=0)
        g = js.fusion(180, 179, [at + 56], [at + 56], homology=1)
        for k in range(160):
            js.read(f if (k >> 5) & 1 else g, 50, 12 + k % 27)
        return js.arrays(), 0, 56
    return make


def repeat_case():
    """A dinucleotide repeat over the junction that runs across a tile boundary (columns 44..68) on both sides: the kept rows'
    maxima tie in columns on both sides of quad wraps and of the tile boundary (the tail replay's masks)."""
    rng = np.random.default_rng(81)
    bb = cases.BatchBuilder()
    for k in range(3):
        unit = (b"AC", b"GT", b"AG")[k]
        ref0 = cases.rnd(rng, 44) + unit * 12 + cases.rnd(rng, 60)
        ref1 = cases.rnd(rng, 50 + k) + unit * 13 + cases.rnd(rng, 44 - k)
        f = bb.add_fusion(ref0, ref1)
        for t in range(70):
            a = 10 + t % 30
            first = 50 + (t * 3) % 19                   # inside the repeat
            s1 = 50 + k + (t * 5) % 20
            bb.add_read(f, (ref0[first - a:first] + ref1[s1:s1 + 50 - a])[:50], read_end=t & 1, revcomp=(t >> 1) & 1)
    return bb.arrays(), 0, 56


def gap_skip_case():
    """test_dsa_loop_waits.late_resume_case: tile 2 has nothing alive in its first row groups and is entered again over its
    boundary column: the registers are set up a second time, in the new frames."""
    l = 3 * 56 + 40
    js = Junctions(12, anchor=60, alphabet=b"ACG")
    f = js.fusion(l, l, [2 * 56 - 30], [2 * 56 - 30], fill0=[(0, 56, b"T")], fill1=[(l - 56, l, b"T")])
    for k in range(128):
        js.read(f, 76, 56 - (k % 4) if k < 64 else 20 + (k * 7) % 37)
    return js.arrays(), 0, 56


def high_score_case():
    """Reads of 300 bases against windows of 1000 (sixteen tiles of 64, six fusions: the split tables of the WIDE
    instantiation): fields up to 1024 + 1200, far from the bias."""
    rng = np.random.default_rng(82)
    bb = cases.BatchBuilder()
    for first in (320, 321, 323, 324, 576, 1000):          # one junction per fusion (sixteen tiles: first offer, junction_reads)
        ref0, ref1 = cases.rnd(rng, 1000), cases.rnd(rng, 1000)
        f = bb.add_fusion(ref0, ref1)
        s1 = int(rng.integers(0, 700))
        for k in range(16):
            bb.add_read(f, cases.split_read(rng, ref0, ref1, 300, first=first, s1=s1, a=140 + k), read_end=k & 1)
    return bb.arrays(), 0, None


def decoy_case():
    """Half the reads are random: nothing of theirs matches, every field stays at the floor, where the candidates below 1024
    occur at the wrap columns; the others are junction reads in the same waves."""
    rng = np.random.default_rng(83)
    bb = cases.BatchBuilder()
    for k in range(2):
        ref0, ref1 = cases.rnd(rng, 389), cases.rnd(rng, 389)
        f = bb.add_fusion(ref0, ref1)
        for t in range(100):
            if t & 1:
                bb.add_read(f, cases.rnd(rng, 76), read_end=t & 1)
            else:
                bb.add_read(f, cases.split_read(rng, ref0, ref1, 76, first=(56, 60, 113, 389)[(t >> 1) % 4], s1=int(rng.integers(0, 300)), a=30 + t % 17))
    # a fusion whose windows share no base with its reads
    f = bb.add_fusion(b"T" * 120, b"T" * 120)
    for t in range(56):
        bb.add_read(f, cases.rnd(rng, 60, b"ACG"))
    return bb.arrays(), 0, 56


CASES = {
    "width-56": width_case([389], 56, 76, 3, 80, 1),
    "width-60": width_case([590], 60, 150, 5, 64, 2, one_junction=True),      # ten tiles: first offer, see junction_reads
    "width-64-128": width_case([128], 64, 50, 3, 64, 3),
    "width-64-192": width_case([192, 190], 64, 76, 3, 100, 4),
    "tiers": tiers_case,
    "reads-with-n": n_case,
    "reads-with-n-split": n_split_case,
    "window-40": last_tile_case(40),
    "window-56": last_tile_case(56),
    "window-57": last_tile_case(57),
    "window-59": last_tile_case(59),
    "window-60": last_tile_case(60),
    "window-61": last_tile_case(61),
    "first-0": junction_column_case(0),
    "first-1": junction_column_case(1),
    "first-3": junction_column_case(3),
    "first-4": junction_column_case(4),
    "first-5": junction_column_case(5),
    "repeat": repeat_case,
    "gap-skip-resume": gap_skip_case,
    "high-scores": high_score_case,
    "decoys": decoy_case,
}

# (dsa_timing.n_replay_tasks, n_generic_tasks) of every case, taken once with the library of the commit before this change
# (DEFUSE_DSA_LIB pointing at a build of it, profiles/quad_drift/task_counts.txt): the tile sets have not changed.
PARENT_TASKS = {
    "width-56": (385, 209),
    "width-60": (385, 68),
    "width-64-128": (252, 61),
    "width-64-192": (465, 204),
    "tiers": (1061, 293),
    "reads-with-n": (373, 155),
    "reads-with-n-split": (300, 50),
    "window-40": (140, 0),
    "window-56": (140, 0),
    "window-57": (185, 46),
    "window-59": (218, 90),
    "window-60": (205, 81),
    "window-61": (217, 82),
    "first-0": (256, 96),
    "first-1": (256, 96),
    "first-3": (160, 0),
    "first-4": (160, 0),
    "first-5": (160, 0),
    "repeat": (361, 157),
    "gap-skip-resume": (128, 0),
    "high-scores": (96, 0),
    "decoys": (149, 94),
}

_made = {}


def made(name):
    """The case's batch, its plan flags, the tile width it is to run at (None: the upload's own choice) and the oracle's
    records: computed once, shared, never modified."""
    if name not in _made:
        from oracle import dosplitalign_oracle as ora
        batch, flags, wt = CASES[name]()
        _made[name] = (batch, flags, wt, ora.align_batch(*batch))
    return _made[name]


def test_every_case_has_its_parent_counts():
    assert sorted(PARENT_TASKS) == sorted(CASES)


def test_oracle_cases_reach_their_edges(built):
    """Window lengths, read lengths and the planted junction columns are what the case names say."""
    from defuse_amd import dsa
    for name in CASES:
        batch, _, wt, exp = made(name)
        assert len(batch[3]) <= 1100 and len(exp) > 0, name
    for name, wt in (("width-56", 56), ("width-60", 60), ("width-64-128", 64), ("width-64-192", 64)):
        batch = made(name)[0]
        assert dsa.tile_cols_for(int(max(batch[1]["ref0_len"].max(), batch[1]["ref1_len"].max()))) == wt
    assert -(-590 // 60) == 10 > 8                                   # the WIDE instantiation
    for l in (40, 56, 57, 59, 60, 61):
        batch = made("window-%d" % l)[0]
        assert set(batch[1]["ref0_len"].tolist()) == {l} and (l <= 56 or l - 56 in (1, 3, 4, 5))
    for r in (0, 1, 3, 4, 5):
        batch, _, _, exp = made("first-%d" % r)
        # ref_first is `first`, the bases of window 0 up to the junction: the M1 part ends in column first - 1
        cols = set((exp["ref_first"] % 56).tolist())
        assert r in cols, (r, sorted(cols))
    batch, _, _, exp = made("reads-with-n")
    assert np.count_nonzero(batch[2] == ord("N")) >= 60
    batch, _, _, exp = made("tiers")
    f = batch[3]["fusion_idx"]
    runs = [1 + int(np.count_nonzero(np.diff(f[k:k + 256]))) for k in range(0, len(f), 256)]
    assert runs[0] <= 4 < runs[1] <= 20 < runs[2] <= 40 and len(runs) == 4, runs
    assert np.count_nonzero(batch[2] == ord("R")) == 1
    batch, _, _, exp = made("high-scores")
    # a score of 300 is a field of 1024 + 4 * 300 in the kernels (+4 per matching row)
    assert set(batch[3]["read_len"].tolist()) == {300} and int(exp["score"].max()) == 300
    # the repeat case ties: some pair has records in columns on both sides of the tile boundary
    batch, _, _, exp = made("repeat")
    both = [p for p in np.unique(exp["pair_idx"]) if len({int(c) // 56 for c in exp["ref_first"][exp["pair_idx"] == p]}) > 1]
    assert both


@pytest.fixture(scope="module")
def ctx(built):
    from defuse_amd import dsa
    c = dsa.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_records_and_task_counts(ctx, name, monkeypatch):
    batch, flags, wt, exp = made(name)
    if wt is not None:
        monkeypatch.setenv("DEFUSE_DSA_TILE_COLS", str(wt))
    else:
        monkeypatch.delenv("DEFUSE_DSA_TILE_COLS", raising=False)
    ctx.set_plan_options(flags)
    try:
        got = ctx.align_batch(*batch)
    finally:
        ctx.set_plan_options(0)
    t = ctx.timing()
    kc = ctx.kernel_counts()
    print("tasks", repr(name), (int(t.n_replay_tasks), int(t.n_generic_tasks)), kc)
    if wt is not None:
        assert ctx.tile_cols_in_use() == wt
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert (int(t.n_replay_tasks), int(t.n_generic_tasks)) == PARENT_TASKS[name]
    if name == "tiers":
        assert kc["fast"] == [1, 1, 1] and kc["generic"] == 1 and sum(kc["fast_wide"]) == 0, kc
    elif name == "width-60":
        assert sum(kc["fast_wide"]) >= 1 and sum(kc["fast"]) == 0 and kc["generic"] == 0, kc
    elif name == "reads-with-n-split" or name.startswith("first-"):      # five and more runs of pairs: the split tables
        assert kc["fast"][1] == 1 and kc["generic"] == 0 and sum(kc["fast"]) == 1, kc
    elif name == "high-scores":                                           # six fusions, sixteen tiles
        assert kc["fast_wide"][1] == 1 and kc["generic"] == 0 and sum(kc["fast"]) == 0, kc
    else:
        assert kc["generic"] == 0 and kc["fast"][0] >= 1 and kc["fast"][1:] == [0, 0] and sum(kc["fast_wide"]) == 0, kc
