"""The tile width in use: how it is picked (CPU) and that every width sweeps to the oracle's records (GPU).

An upload is swept in register tiles of WT <= 64 reference columns, the built width for which its widest window pads out to
the fewest swept columns (dsa_tile.hpp: 389 bases are seven tiles of 56 instead of seven of 64).  Every place that turns a
(tile, column) into a reference position depends on WT, so the GPU cases take window lengths that pick each built width and
sit on its edges (a last tile of one column, of WT columns, one base more), with junctions on the tile boundaries of every
width, all four fill kernels (table tiers 0-2 and the generic one), ties that need the left-over replay, and the WIDE
instantiation (9-16 tiles).  Records are compared with oracle/dsa_oracle.c byte for byte.
"""
import numpy as np
import pytest

from tests import cases

BUILT_WIDTHS = (64, 60, 56)          # TILE_WIDTHS of defuse_amd/csrc/dsa_tile.hpp
LQ = 76


def tile_class(tiles):
    return 0 if tiles <= 8 else 1 if tiles <= 16 else 2 if tiles <= 64 else 3 if tiles <= 255 else 4


def expected_width(length, widths=BUILT_WIDTHS):
    """The rule as the issue states it, written independently of the library: fewest swept columns, ties to the wider tile;
    64 where the tile count would land in another class of the kernels' limits (8 / 16 / 64 / 255 tiles)."""
    if length <= 0:
        return 64
    best = min(widths, key=lambda w: (-(-length // w) * w, -w))
    if tile_class(-(-length // best)) != tile_class(-(-length // 64)):
        return 64
    return best


def test_pick_matches_the_rule(built):
    from defuse_amd import dsa
    for length in list(range(0, 4200)) + list(range(14000, 16400)) + [7600, 65536]:
        assert dsa.tile_cols_for(length) == expected_width(length), length
        assert length > 16320 or -(-length // dsa.tile_cols_for(length)) <= 255           # tile indices are bytes, 255 = none


def test_pick_known_windows(built):
    from defuse_amd import dsa
    # the benchmark's windows (389, multi-GPU shape 390): seven tiles of 56 = 392 columns instead of 448
    assert [dsa.tile_cols_for(n) for n in (389, 390, 392)] == [56, 56, 56]
    assert dsa.tile_cols_for(393) == 60 and dsa.tile_cols_for(420) == 60          # 7 x 60
    assert dsa.tile_cols_for(590) == 60                                           # 2x150 bp: ten tiles of 60 = 600 (640 with 64)
    for n in (64, 128, 384, 448, 512, 640):                                       # multiples of 64: nothing changes
        assert dsa.tile_cols_for(n) == 64
    assert dsa.tile_cols_for(449) == 60 and dsa.tile_cols_for(450) == 60          # eight tiles of 60; nine of 56 would cross the 8-tile limit
    assert dsa.tile_cols_for(0) == 64 and dsa.tile_cols_for(1) == 56
    for n in range(1, 3000):
        wt = dsa.tile_cols_for(n)
        assert wt in BUILT_WIDTHS
        assert -(-n // wt) * wt <= -(-n // 64) * 64                               # never more columns than 64-column tiles sweep
        assert tile_class(-(-n // wt)) == tile_class(-(-n // 64))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def ctx(built):
    from defuse_amd import dsa
    c = dsa.Context(0)
    yield c
    c.close()


def oracle(batch):
    import bench
    return bench.oracle_records(batch, len(batch[3]))


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.bb = cases.BatchBuilder()
        self.win = []

    def fusion(self, l0, l1):
        r0, r1 = cases.rnd(self.rng, l0), cases.rnd(self.rng, l1, b"ACGTN" if len(self.win) % 3 == 2 else b"ACGT")
        if len(self.win) % 4 == 1 and l0 > 200:           # a duplicated segment: tied columns in two tiles (left-over replay)
            seg = r0[l0 - 40:l0 - 10]
            r0 = r0[:70] + seg + r0[100:]
        self.win.append((r0, r1))
        return self.bb.add_fusion(r0, r1, fusion_id=10 * len(self.win) + 3)

    def read(self, f, exotic=None):
        r0, r1 = self.win[f]
        rng = self.rng
        k = int(rng.integers(0, 10))
        lq = min(LQ, len(r0) + len(r1)) if k else int(rng.integers(9, LQ))
        if k == 1:                                        # junction at the last column of window 0 / first base of window 1
            read = cases.split_read(rng, r0, r1, lq, first=len(r0), s1=0)
        elif k == 2:                                      # junction at the end of window 1
            read = cases.split_read(rng, r0, r1, lq, s1=max(0, len(r1) - lq // 2))
        elif k == 3:
            w = r0 if rng.integers(0, 2) else r1
            p = int(rng.integers(0, max(1, len(w) - lq + 1)))
            read = w[p:p + lq]
        elif k in (4, 5, 6):                              # junction on or next to a tile boundary of one of the widths, either side
            wt = int(rng.choice(BUILT_WIDTHS))
            d = int(rng.integers(-1, 2))
            first = min(len(r0), max(1, wt * int(rng.integers(1, len(r0) // wt + 2)) + d))
            e1 = min(len(r1), max(1, wt * int(rng.integers(1, len(r1) // wt + 2)) + d))       # M2 runs over the reversed window
            read = cases.split_read(rng, r0, r1, lq, first=first, s1=len(r1) - e1 if k != 4 else None)
        else:
            read = cases.split_read(rng, r0, r1, lq)
        read = cases.mutate(rng, read, 0.01)
        if exotic is not None and len(read) > 0:
            read = read[:len(read) // 2] + exotic + read[len(read) // 2 + 1:]
        self.bb.add_read(f, read, read_end=int(rng.integers(0, 2)), revcomp=int(rng.integers(0, 2)))

    def workgroup(self, fus, n=256, exotic=None):
        cut = np.linspace(0, n, len(fus) + 1).astype(int)
        for k, f in enumerate(fus):
            for j in range(cut[k], cut[k + 1]):
                self.read(f, exotic if (exotic and j == n // 2) else None)

    def arrays(self):
        return self.bb.arrays()


def length_batch(seed, lens):
    """Workgroups of 2, 10, 30 and 50 runs (tiers 0, 1, 2 and the generic kernel) and one with a read byte outside
    A/C/G/T/N, over fusions whose windows have the lengths `lens` (the widest sets the tile width; either side gets each)."""
    bz = Builder(seed)
    pool = []
    for k in range(92):
        l0, l1 = lens[k % len(lens)], lens[(k // len(lens) + 1) % len(lens)]
        pool.append(bz.fusion(l0, l1))
    bz.workgroup(pool[0:2])
    bz.workgroup(pool[2:12])
    bz.workgroup(pool[12:42])
    bz.workgroup(pool[42:92])
    bz.workgroup(pool[0:3], exotic=b"R")
    return bz.arrays()


def check(ctx, batch, width, flags=0):
    ctx.set_plan_options(flags)
    try:
        got = ctx.align_batch(*batch)
    finally:
        ctx.set_plan_options(0)
    assert ctx.tile_cols_in_use() == width
    exp = oracle(batch)
    assert len(exp) > 0
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    kc = ctx.kernel_counts()
    assert sum(kc["fast"]) + sum(kc["fast_wide"]) + kc["generic"] == kc["workgroups"]
    return kc


# window length -> the width it picks: the benchmark's windows, a last tile of WT columns / of one column for every built
# width, and the WIDE shapes (590: ten tiles of 60; 601: eleven of 56; 640: ten of 64)
LENGTHS = [(389, 56), (390, 56), (392, 56), (393, 60), (448, 64), (449, 60), (590, 60),
           (56, 56), (57, 60), (60, 60), (61, 64), (65, 56), (112, 56), (113, 60), (420, 60), (421, 64),
           (600, 60), (601, 56), (616, 56), (617, 64), (640, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("length,width", LENGTHS)
def test_windows_of_one_length(ctx, length, width):
    assert expected_width(length) == width
    kc = check(ctx, length_batch(length, [length, max(20, length - 37)]), width, flags=1)     # the caller's order: the workgroups as built
    wide = length > 8 * width and length <= 16 * width
    fast = kc["fast_wide"] if wide else kc["fast"]
    assert fast == [1, 1, 1] and kc["generic"] == 2 and sum(kc["fast" if wide else "fast_wide"]) == 0, kc


@pytest.mark.gpu
@pytest.mark.parametrize("longest,width", [(389, 56), (393, 60), (448, 64), (590, 60)])
def test_mixed_window_lengths_in_one_slice(ctx, longest, width):
    """Windows of many lengths in one upload: the widest picks the width, the others end anywhere in their last tile (and
    have fewer tiles)."""
    rng = np.random.default_rng(longest)
    lens = [longest] + [int(x) for x in rng.integers(30, longest, size=22)] + [width, width + 1, 2 * width - 1, 2 * width, 64, 128]
    batch = length_batch(1000 + longest, lens)
    check(ctx, batch, width)                  # planned sweep order
    check(ctx, batch, width, flags=1)         # the caller's order


@pytest.mark.gpu
def test_repeats_and_ties_in_narrow_tiles(ctx):
    """Repeat-rich windows (many kept splits in several tiles: every emit path) and low-complexity ties under a 56-column tiling."""
    ref, fusions, reads, pairs = cases.repeat_batch(11, n_fusions=12, reads_per_fusion=100)
    bb = cases.BatchBuilder()
    rng = np.random.default_rng(3)
    bb.add_fusion(cases.rnd(rng, 389), cases.rnd(rng, 389))          # sets the width for the whole upload
    bb.add_read(0, cases.split_read(rng, bytes(bb.ref[:389]), bytes(bb.ref[389:]), LQ))
    r2, f2, q2, p2 = bb.arrays()
    f = fusions.copy()
    f["ref0_off"] += len(r2)
    f["ref1_off"] += len(r2)
    p = pairs.copy()
    p["fusion_idx"] += len(f2)
    p["read_off"] += len(q2)
    batch = (np.concatenate([r2, ref]), np.concatenate([f2, f]), np.concatenate([q2, reads]), np.concatenate([p2, p]))
    longest = int(max(batch[1]["ref0_len"].max(), batch[1]["ref1_len"].max()))
    check(ctx, batch, expected_width(longest))
    tie = cases.tie_batch(5)
    longest = int(max(tie[1]["ref0_len"].max(), tie[1]["ref1_len"].max()))
    check(ctx, tie, expected_width(longest))
