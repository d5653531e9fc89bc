"""The fill kernels keep what is the same in every lane of a wave in scalar registers: the wave's longest read and tile count,
the row-group counter of a sweep, the stop of the tile to the left, the workgroup's tile count and its number of fusion runs.
A value taken for wave-uniform that is not one reads the FIRST lane's: these are the smallest batches at which that shows.

* Mixed read lengths in one wave: lane 0 holds the shortest read (1-5 bases) and another lane the longest (76); waves whose
  reads all have 1-3 bases (one row group) and 1-5 bases (two), so that the lane's read ends before the wave's does and its
  threshold is the 0xFFFF of rows past the read.
* Batches of 1, 63, 65, 255 and 257 pairs: a last wave with shadow lanes, and a workgroup with whole waves past the end that
  still join its barriers.
* Windows of 56, 57, 113 and 389 bases in one workgroup, one length per wave: the waves of a workgroup sweep different numbers
  of tiles, fewer than the workgroup builds tables for.
* One lane with many mismatches between exact neighbours: the pruning slack differs from lane to lane.
* Junction reads, reads wholly inside one window and decoys mixed (synth.make_batch): sweeps that stop early, skip dead gaps
  and resume; once without the planner's per-pair bounds.

Every case runs through the four fill kernels (workgroups of 4, 10, 30 and 50 runs of pairs of one fusion: table tiers 0, 1, 2
and the generic kernel, and a workgroup a read byte outside A/C/G/T/N hands over) and with each built tile width forced
(DEFUSE_DSA_TILE_COLS).  Records are compared byte for byte with oracle.dosplitalign_oracle.align_batch; the oracle's records of
a case are computed once and shared by its widths.  test_every_case_has_records (no GPU) keeps the cases from being vacuous.
"""
import functools

import numpy as np
import pytest

from tests import cases

WIDTHS = (64, 60, 56)                 # TILE_WIDTHS of defuse_amd/csrc/dsa_tile.hpp
LQ = 76
RUNS = (4, 10, 30, 50)                # runs per workgroup of 256 pairs: tiers 0, 1, 2, generic (GMAX 4, GSPLIT 20, GSPLIT2 40)
WG = 256
NO_REORDER, NO_TIGHTEN = 1, 4         # dsa.PLAN_NO_REORDER, dsa.PLAN_NO_TIGHTEN


def tier_of_runs(n):
    return 0 if n <= 4 else 1 if n <= 20 else 2 if n <= 40 else 3


def junction(rng, r0, r1, lq, a=None):
    return cases.split_read(rng, r0, r1, min(lq, len(r0) + len(r1)), a=a)


def with_mismatches(rng, read, n):
    b = bytearray(read)
    for i in rng.choice(len(b), size=min(n, len(b)), replace=False):
        b[i] = ord("ACGT"[("ACGT".index(chr(b[i])) + 1 + int(rng.integers(0, 3))) % 4]) if chr(b[i]) in "ACGT" else ord("A")
    return bytes(b)


def tiered_batch(seed, windows, make_read, exotic=True):
    """One workgroup of 256 pairs for each entry of RUNS (in the caller's order pair p is thread p % 256 of workgroup p // 256)
    and one more of three runs with a read that holds an 'R'.  windows(rng, wave) -> the lengths of the two windows of a run that
    begins in that wave; make_read(rng, ref0, ref1, thread) -> the read of that thread."""
    rng = np.random.default_rng(seed)
    bb = cases.BatchBuilder()
    for wg, n_runs in enumerate(list(RUNS) + ([3] if exotic else [])):
        cut = np.linspace(0, WG, n_runs + 1).astype(int)
        for k in range(n_runs):
            l0, l1 = windows(rng, int(cut[k]) >> 6)
            r0, r1 = cases.rnd(rng, l0), cases.rnd(rng, l1, b"ACGTN" if k % 3 == 2 else b"ACGT")
            f = bb.add_fusion(r0, r1, fusion_id=1000 * wg + 7 * k + 3)
            for t in range(cut[k], cut[k + 1]):
                read = make_read(rng, r0, r1, int(t))
                if wg == len(RUNS) and t == WG // 2:
                    read = read[:len(read) // 2] + b"R" + read[len(read) // 2 + 1:] if len(read) else b"R"
                bb.add_read(f, read, read_end=int(t & 1), revcomp=int((t >> 1) & 1))
    return bb.arrays()


def windows_389(rng, wave):
    return 389, 352


def mixed_read_lengths(seed):
    long_lane = {0: 41, 3: 63}

    def make_read(rng, r0, r1, t):
        wave, lane = t >> 6, t & 63
        if wave == 1:                                        # every read of the wave in the first row group (rows 0-3)
            lq = 1 if lane == 0 else int(rng.integers(1, 4))
        elif wave == 2:                                      # two row groups; lane 0 ends in the first
            lq = 1 if lane == 0 else 5 if lane == 9 else int(rng.integers(1, 6))
        elif lane == 0:                                      # lane 0 the shortest of its wave
            lq = int(rng.integers(1, 6))
        elif lane == long_lane[wave]:
            lq = LQ
        else:
            lq = int(rng.integers(6, LQ))
        return cases.mutate(rng, junction(rng, r0, r1, lq), 0.01)
    return tiered_batch(seed, windows_389, make_read)


def mixed_window_lengths(seed):
    lens = [(56, 40), (57, 57), (113, 100), (389, 352)]     # by wave: 1, 2, 3 and 7 tiles of 56 columns
    return tiered_batch(seed, lambda rng, wave: lens[wave],
                        lambda rng, r0, r1, t: cases.mutate(rng, junction(rng, r0, r1, LQ if t % 5 else int(rng.integers(20, LQ))), 0.01))


def lane_slack(seed):
    def make_read(rng, r0, r1, t):
        read = junction(rng, r0, r1, LQ, a=int(rng.integers(20, 57)))
        return with_mismatches(rng, read, 4 + t % 2) if (t & 63) in (0, 17, 40, 63) else read      # exact neighbours: slack 0
    return tiered_batch(seed, windows_389, make_read)


def sized_batch(n_pairs, n_fusions, seed):
    rng = np.random.default_rng(seed)
    bb = cases.BatchBuilder()
    cut = np.linspace(0, n_pairs, n_fusions + 1).astype(int)
    for k in range(n_fusions):
        r0, r1 = cases.rnd(rng, 389), cases.rnd(rng, 300)
        f = bb.add_fusion(r0, r1, fusion_id=11 * k + 5)
        for t in range(cut[k], cut[k + 1]):
            exact = t == 0 or t == n_pairs - 1               # the first and the last pair certainly have a record
            read = junction(rng, r0, r1, LQ, a=38 if exact else None)
            bb.add_read(f, read if exact else cases.mutate(rng, read, 0.01), read_end=int(t & 1), revcomp=int((t >> 1) & 1))
    return bb.arrays()


def pruning_mix(n_fusions, reads_per_fusion, seed):
    from defuse_amd import synth
    return synth.make_batch(n_fusions, reads_per_fusion, lq=LQ, lr=389, seed=seed, decoy_frac=0.3, inside_frac=0.3)


SIZES = (1, 63, 65, 255, 257)
# 3 fusions x 100 reads as the headline has them, and the same mix in workgroups of 12, 29 and 128 runs
MIXES = ((3, 100), (12, 22), (30, 9), (150, 2))
CASES = {"read_lengths": lambda: mixed_read_lengths(101),
         "window_lengths": lambda: mixed_window_lengths(102),
         "lane_slack": lambda: lane_slack(103)}
for _n in SIZES:
    for _f in RUNS:
        if _f <= _n:
            CASES["size_%d_runs_%d" % (_n, _f)] = functools.partial(sized_batch, _n, _f, 200 + _n + _f)
CASES["size_1_runs_1"] = functools.partial(sized_batch, 1, 1, 201)
for _f, _r in MIXES:
    CASES["mix_%dx%d" % (_f, _r)] = functools.partial(pruning_mix, _f, _r, 300 + _f)
TIERED = ("read_lengths", "window_lengths", "lane_slack")


@functools.lru_cache(maxsize=None)
def case(name):
    """(batch, the oracle's records), computed once per session and never modified"""
    from oracle import dosplitalign_oracle as ora
    batch = tuple(CASES[name]())
    exp = ora.align_batch(*batch)
    for a in batch + (exp,):
        a.setflags(write=False)
    return batch, exp


def runs_of_first_workgroup(batch):
    f = batch[3]["fusion_idx"][:WG]
    return 1 + int(np.count_nonzero(f[1:] != f[:-1]))


def test_every_case_has_records(built):
    for name in CASES:
        batch, exp = case(name)
        assert len(exp) > 0, name
    # the shapes the cases are there for
    pairs = case("read_lengths")[0][3]
    for wg in range(len(RUNS) + 1):
        lq = pairs["read_len"][wg * WG:(wg + 1) * WG].reshape(4, 64)
        assert (lq[:, 0] == lq.min(axis=1)).all() and (lq[:, 0] <= 5).all()
        assert lq[0].max() == LQ and lq[3].max() == LQ and lq[1].max() <= 3 and 4 <= lq[2].max() <= 5
    ref, fus, _, pairs = case("window_lengths")[0]
    longest = np.maximum(fus["ref0_len"], fus["ref1_len"])[pairs["fusion_idx"][:2 * WG]].reshape(2, 4, 64)
    assert longest.max(axis=2).tolist() == [[56, 57, 113, 389]] * 2       # the workgroups of tiers 0 and 1: one length per wave
    for n in SIZES:
        assert len(case("size_%d_runs_%d" % (n, 1 if n == 1 else RUNS[0]))[0][3]) == n


# ---------------------------------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def ctx(built):
    from defuse_amd import dsa
    c = dsa.Context(0)
    yield c
    c.close()


def check(ctx, monkeypatch, name, width, flags=0):
    batch, exp = case(name)
    monkeypatch.setenv("DEFUSE_DSA_TILE_COLS", str(width))
    ctx.set_plan_options(flags)
    try:
        got = ctx.align_batch(*batch)
    finally:
        ctx.set_plan_options(0)
    assert ctx.tile_cols_in_use() == width
    assert len(exp) > 0
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes(), name
    kc = ctx.kernel_counts()
    assert sum(kc["fast"]) + sum(kc["fast_wide"]) + kc["generic"] == kc["workgroups"]
    return kc


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", TIERED)
def test_lane_values_in_all_fill_kernels(ctx, monkeypatch, name, width):
    kc = check(ctx, monkeypatch, name, width, flags=NO_REORDER)          # the caller's order: waves and workgroups as built
    assert kc["fast"] == [1, 1, 1] and kc["generic"] == 2 and sum(kc["fast_wide"]) == 0, kc
    check(ctx, monkeypatch, name, width)                                 # the planned order: other lanes meet in a wave


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n_pairs", SIZES)
def test_batch_sizes_at_wave_and_workgroup_edges(ctx, monkeypatch, n_pairs, width):
    for runs in ((1,) if n_pairs == 1 else RUNS):
        if runs > n_pairs:
            continue
        name = "size_%d_runs_%d" % (n_pairs, runs)
        kc = check(ctx, monkeypatch, name, width, flags=NO_REORDER)
        assert kc["workgroups"] == -(-n_pairs // WG)
        tier = tier_of_runs(runs_of_first_workgroup(case(name)[0]))
        assert (kc["generic"] if tier == 3 else kc["fast"][tier]) >= 1, (name, kc)
        check(ctx, monkeypatch, name, width)


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mix", MIXES)
def test_stop_gap_skip_and_resume(ctx, monkeypatch, mix, width):
    name = "mix_%dx%d" % mix
    kc = check(ctx, monkeypatch, name, width, flags=NO_REORDER)
    tier = tier_of_runs(runs_of_first_workgroup(case(name)[0]))
    assert (kc["generic"] if tier == 3 else kc["fast"][tier]) >= 1, (name, kc)
    check(ctx, monkeypatch, name, width)
    check(ctx, monkeypatch, name, width, flags=NO_TIGHTEN)               # the slack of minScore alone: later stops, other gaps
