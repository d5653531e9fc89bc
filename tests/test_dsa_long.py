"""The 32-bit split-read path (defuse_amd/csrc/dsa_long.hpp: k_long_rows, k_long_cols, k_long_emit, k_long_blank) at the edges
of its column partition, its grid-stride loop, the slices, the emit and the context's state: every record against the CPU
oracle, byte for byte, and every test checks from the kernel counts and the oracle's answer that it is on the path it means."""
import numpy as np
import pytest

from tests import cases, long_cases as lc
from tests.test_dsa_gpu import check_batch, ora  # noqa: F401  (ora is a fixture)

gpu = pytest.mark.gpu


def pairs_with_records(exp, n_pairs):
    return np.bincount(exp["pair_idx"], minlength=n_pairs) > 0


def report(name, long_pairs, exp):
    print("%s: long_pairs %d, records %d" % (name, long_pairs, len(exp)))


def run_sliced(monkeypatch, batch):
    """The batch on a context of its own under DEFUSE_DSA_SLICE_PAIRS: records, fill launches, kernel counts."""
    from defuse_amd import dsa
    with monkeypatch.context() as m:
        m.setenv("DEFUSE_DSA_SLICE_PAIRS", str(lc.SLICE_PAIRS))
        ctx = dsa.Context(0)
        try:
            got = ctx.align_batch(*batch)
            return got, ctx.timing().fill_launches, ctx.kernel_counts()
        finally:
            ctx.close()


# ---- 1. the tables reach the edges they are meant to (no GPU) ----

def test_tables_reach_every_partition_class():
    """dsa_long.hpp: LONG_THREADS = 256, FAST_MAX_READ = 7600, FAST_MAX_REF = 255 * 64; long_row: nw = (len + 1 + 31) / 32 words,
    per = ceil(nw / 256) words per thread.  A changed length that no longer reaches a class fails here."""
    assert (lc.LONG_THREADS, lc.FAST_MAX_READ, lc.FAST_MAX_REF) == (256, 7600, 16320)
    wide = {length: lc.layout(length) for length in lc.WINDOW_TABLE}
    for length, (nw, per) in lc.WINDOW_TABLE.items():
        assert (wide[length]["nw"], wide[length]["per"]) == (nw, per), length
        assert length > lc.FAST_MAX_REF and lc.SHORT_WINDOW <= lc.FAST_MAX_REF      # exactly one over-long side
    assert min(lc.WINDOW_TABLE) == lc.FAST_MAX_REF + 1 and lc.CONTROL_WINDOW == lc.FAST_MAX_REF
    assert lc.LONG_READ == lc.FAST_MAX_READ + 1
    under_read = {}
    for (l0, l1), (nw0, nw1) in lc.LONG_READ_TABLE.items():
        assert max(l0, l1) <= lc.FAST_MAX_REF and l0 + l1 >= lc.LONG_READ            # long by the read alone, which spans ref1
        under_read[l0], under_read[l1] = lc.layout(l0), lc.layout(l1)
        assert (under_read[l0]["nw"], under_read[l1]["nw"]) == (nw0, nw1), (l0, l1)

    def some(table, **want):
        return any(all(lo[k] == v for k, v in want.items()) for lo in table.values())

    # section 2: one over-long window, per = 2 and per = 3
    assert some(wide, per=2, active=256, last_run=1)                    # thread 255 has one word
    assert some(wide, per=2, active=256, last_run=2, last_cols=32)      # every run full, last word full
    assert some(wide, per=2, last_run=1, last_cols=32)                  # ragged run, last word full
    assert some(wide, per=2, last_cols=1)
    assert some(wide, per=3, active=171, last_run=3, last_cols=1)       # wave 3 wholly idle, wave 2 partly (128 < 171 < 192)
    assert some(wide, per=3, active=171, last_run=3, last_cols=2)
    assert some(wide, per=3, active=256, last_run=2, last_cols=32)      # no idle thread, thread 255 has two words
    assert some(wide, per=3, active=256, last_run=3, last_cols=1)       # 256 x 3 words
    # section 3: a long read over short windows, per = 1 and the flip to per = 2
    assert some(under_read, nw=1, active=1, last_cols=32)               # thread 0 alone, one full word
    assert some(under_read, nw=2, active=2, last_cols=1)                # two threads, one column in word 1
    assert some(under_read, nw=255, per=1)
    assert some(under_read, nw=256, per=1, active=256, last_cols=32)    # all 256 threads, one word each
    assert some(under_read, nw=257, per=2, active=129, last_run=1, last_cols=1)      # the flip: thread 128 holds a one-column word
    assert any(lo["per"] == 1 and 192 < lo["active"] < 256 for lo in under_read.values())      # idle threads in the last wave only
    assert sorted(n for n, lo in under_read.items() if lo["per"] == 1 and lo["nw"] > 2) == [7570, 8159, 8191]


# ---- 2. partition edges under short reads, one over-long window ----

@pytest.fixture(scope="module")
def window_edges(ora):
    batch, n_long = lc.window_edge_batch()
    return batch, n_long, ora.align_batch(*batch)


@gpu
def test_one_over_long_window_at_every_partition_edge(gpu_ctx, window_edges):
    """Each window length of WINDOW_TABLE as ref0 and as ref1, junctions at the first and last columns of both matrices; the
    fusion of 16320 + 64 bases in the same batch stays with the 16-bit kernels."""
    batch, n_long, exp = window_edges
    assert n_long == 64 and len(batch[3]) == 68
    assert pairs_with_records(exp, 68).all()
    got = gpu_ctx.align_batch(*batch)
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert gpu_ctx.kernel_counts()["long_pairs"] == n_long
    report("window edges", n_long, exp)


# ---- 3. partition edges under a long read, short windows ----

@gpu
def test_long_read_over_short_windows_at_every_partition_edge(gpu_ctx, ora):
    """per = 1 (255, 256 and 237 words), the flip to per = 2 at 257 words, and second windows of one and two words."""
    batch = lc.long_read_batch()
    exp = ora.align_batch(*batch)
    assert pairs_with_records(exp, 4).all()                 # each clears int(0.9 * 2 * 7601)
    assert (batch[3]["read_len"] == lc.LONG_READ).all()
    got = gpu_ctx.align_batch(*batch)
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert gpu_ctx.kernel_counts()["long_pairs"] == 4
    report("long reads", 4, exp)


# ---- 4. more long pairs than workgroups ----

@gpu
@pytest.mark.parametrize("second_turn_aligns", [True, False], ids=["second-turn-aligns", "second-turn-empty"])
def test_a_workgroup_takes_a_second_long_pair(gpu_ctx, ora, monkeypatch, second_turn_aligns):
    """513 long pairs on 512 workgroups: block 0 sweeps pair 0 and then pair 512, of the other fusion (other nw0, nw1, the same
    row buffers).  Pairs without a kept split (k_long_cols' `continue`) fall on first turns and, in one of the two variants, on
    the second turn; in the other the second turn's records are checked.  Also as three slices, all long, the last of one pair."""
    batch, empty = lc.many_pairs_batch(second_turn_aligns)
    n = lc.MANY_PAIRS
    assert len(batch[3]) == n and batch[3]["fusion_idx"][0] != batch[3]["fusion_idx"][n - 1]
    exp = ora.align_batch(*batch)
    has = pairs_with_records(exp, n)
    assert not has[empty].any() and has.sum() == n - len(empty)       # every pair meant to align does, no random read does
    assert bool(has[n - 1]) == second_turn_aligns and bool(has[0]) != second_turn_aligns
    assert has[1:n - 1].any() and not has[1:n - 1].all()
    got = gpu_ctx.align_batch(*batch)
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert gpu_ctx.kernel_counts()["long_pairs"] == n
    got, fill_launches, kc = run_sliced(monkeypatch, batch)
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert fill_launches == 3 and kc["long_pairs"] == n
    report("513 long pairs", n, exp)


# ---- 5. long pairs at slice boundaries among ordinary pairs ----

@gpu
def test_long_pairs_at_the_first_and_last_index_of_every_slice(gpu_ctx, ora, monkeypatch):
    """Three slices of 256, 256 and 94 pairs with a long pair at either end of each; frag, read_end, revcomp and fusion_id, none
    at its default, come through LongDesc.  Sliced and unsliced give the same bytes, which are the oracle's."""
    batch, long_at = lc.slice_boundary_batch()
    n = len(batch[3])
    assert long_at == [0, 255, 256, 511, 512, n - 1]
    exp = ora.align_batch(*batch)
    assert pairs_with_records(exp, n)[long_at].all()
    mine = exp[np.isin(exp["pair_idx"], long_at)]
    assert (mine["read_end"] == 1).all() and (mine["revcomp"] == 1).all()
    assert set(mine["fusion_id"].tolist()) == {900001, 123456789} and (mine["frag"] == 70000 - 3 * mine["pair_idx"]).all()
    whole = gpu_ctx.align_batch(*batch)
    assert gpu_ctx.timing().fill_launches == 1 and gpu_ctx.kernel_counts()["long_pairs"] == len(long_at)
    assert len(whole) == len(exp) and whole.tobytes() == exp.tobytes()
    sliced, fill_launches, kc = run_sliced(monkeypatch, batch)
    assert fill_launches == 3 and kc["long_pairs"] == len(long_at)
    assert len(sliced) == len(exp) and sliced.tobytes() == exp.tobytes()
    assert sliced.tobytes() == whole.tobytes()
    report("slice boundaries", len(long_at), exp)


# ---- 6. the minimum score at equality ----

@gpu
def test_minimum_score_at_equality_and_one_below(gpu_ctx, ora):
    """s >= d.min_score in k_long_rows: a 41-base read (minimum 73) with 0..4 substitutions scores 82 - 3 k."""
    batch, (ref0, ref1), reads = lc.min_score_batch()
    exp = ora.align_batch(*batch)
    assert ora.lib().ora_min_score(lc.MIN_SCORE_READ) == 73
    sums = [int(ora.row_maxima(ref0, r)[21]) + int(ora.row_maxima(ref1[::-1], r[::-1])[20]) for r in reads]
    assert sums == [82, 79, 76, 73, 70]
    assert np.bincount(exp["pair_idx"], minlength=5).tolist() == [1, 1, 1, 1, 0]
    assert (exp["read_first"] == 21).all() and exp["score"].tolist() == [40, 39, 36, 36]
    got = gpu_ctx.align_batch(*batch)
    assert len(got) == len(exp) and got.tobytes() == exp.tobytes()
    assert gpu_ctx.kernel_counts()["long_pairs"] == 5
    report("minimum score", 5, exp)


# ---- 7. the emit runs again after the record buffer has grown ----

@gpu
def test_emit_again_after_the_record_buffer_grows(built, ora):
    """A fresh context has room for 2 * n_pairs + 1024 records; the first pair alone has more (at least 40 x 30 tied columns),
    so k_long_emit<true> gives up (rec_offset[o + 1] > out_cap) and is run again into the grown buffer.  The second pair ties
    at neighbouring splits: the refSplit de-duplication across kept splits."""
    from defuse_amd import dsa
    batch = lc.regrow_batch()
    exp = ora.align_batch(*batch)
    room = 2 * len(batch[3]) + 1024
    assert np.sum(exp["pair_idx"] == 0) > room
    assert len(np.unique(exp["read_first"][exp["pair_idx"] == 1])) >= 2
    ctx = dsa.Context(0)
    try:
        ctx.upload(*batch)
        assert ctx.run() == len(exp)
        got = ctx.download()
        assert got.tobytes() == exp.tobytes()
        assert ctx.kernel_counts()["long_pairs"] == 2
    finally:
        ctx.close()
    report("record buffer grows", 2, exp)


# ---- 8. state between runs and uploads of one context ----

@gpu
def test_nothing_of_a_long_upload_stays_in_the_context(built, ora, window_edges):
    """A second run of the resident upload gives the same records and counts its long pairs once (the kernel counts are those
    of the last run); an ordinary upload after it sees no long pair, no blanked pair or fusion; an upload whose over-long
    fusion sits where an ordinary one was, and the other way round, equals the oracle."""
    from defuse_amd import dsa
    batch, n_long, exp = window_edges
    ctx = dsa.Context(0)
    try:
        ctx.upload(*batch)
        for _ in range(2):
            assert ctx.run() == len(exp)
            assert ctx.download().tobytes() == exp.tobytes()
            assert ctx.kernel_counts()["long_pairs"] == n_long
        plain = cases.mixed_batch(1)
        check_batch(ctx, ora, plain)
        assert ctx.kernel_counts()["long_pairs"] == 0
        moved, n_moved = lc.moved_fusion_batch()
        assert (moved[1]["ref1_len"][:16] <= lc.FAST_MAX_REF).all() and moved[1]["ref1_len"][16] > lc.FAST_MAX_REF
        exp_moved = ora.align_batch(*moved)
        assert pairs_with_records(exp_moved, len(moved[3]))[-n_moved:].all()
        got = ctx.align_batch(*moved)
        assert len(got) == len(exp_moved) and got.tobytes() == exp_moved.tobytes()
        assert ctx.kernel_counts()["long_pairs"] == n_moved == 4
        check_batch(ctx, ora, plain)
        assert ctx.kernel_counts()["long_pairs"] == 0
    finally:
        ctx.close()
    report("state between uploads", n_long, exp)
