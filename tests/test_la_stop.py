"""localalign / matealign's packed kernel k_la16 at its early stop and its 16-bit limits, k_la32 at its wave edges.

The random batches of test_localalign.py keep some lane of every wave alive almost everywhere, so the wave-uniform stop, what
a tile remembers of its left neighbour's stop (stop_prev), the rule that keeps sweeping while the entering boundary is alive
(l_in) and the Y = 0 that stands in for boundary rows nobody wrote almost never decide a score there.  The cases of
la_stop_cases.py are built so that they do; la_sweep_model.py says, in plain integers, what the kernel is documented to
sweep, and la_timing.row_groups16 says what it swept.  The CPU tests prove on the model that each case reaches its path and
that a kernel with one of four errors in the stop rule could not pass; the GPU tests hold the kernel to the oracle's scores
and to the model's count, so one that stops too early fails the scores or the count and one that no longer stops fails the
count.

The operand range of the packed fields: the top is BIAS16 + rows * step (29048 for 27 rows at a step of 1000), the bottom is
BIAS16 - gd, which is 1048 only where gap = -1000; the scorings with gap = -500 and gap = 0 reach 1548 and 2048, and the test
asserts BIAS16 - gd for each.
"""
import numpy as np
import pytest

from tests import la_stop_cases as cs
from tests import la_sweep_model as model

NO_MODEL = ("h-copy-1863", "h-copy-1864")        # 30 tiles of 1863 rows: the closed form covers them


def _names():
    names = ["a-%d-%d" % (L, need) for L in cs.ZERO_SLACK_L for need in (1000, 1001)] + ["b"]
    names += ["c-%d" % L for L in cs.ONE_LIVE_L] + ["d", "e-0", "e-1"]
    names += ["f-%d-%s" % (n, mn) for n in (1, 127, 128, 129) for mn in ("0.8", "none")]
    names += ["g-max", "g-min", "g-zero", "h-copy-1863", "h-copy-1864"]
    names += ["h-%d_%d_%d" % prm for prm in cs.PACKED_SCORINGS + cs.INT32_SCORINGS] + ["h-28rows"]
    names += ["i-%d-%d_%d_%d" % ((n,) + prm) for n in (1, 63, 64, 65) for prm in cs.LA32_SCORINGS]
    return names


NAMES = _names()


def _want(case):
    from oracle import localalign_oracle as o
    return np.array([o.simple_align(*case.prm, r, s) for r, s in case.pairs], dtype=np.int64)


def _build(name):
    p = name.split("-")
    if p[0] == "a":
        return cs.zero_slack(int(p[1]), int(p[2]))
    if p[0] == "b":
        return cs.split_copy()
    if p[0] == "c":
        return cs.one_live(int(p[1]))
    if p[0] == "d":
        return cs.all_dead()
    if p[0] == "e":
        return cs.at_minimum(_want(cs.at_minimum(None, 0)), int(p[1]))
    if p[0] == "f":
        return cs.wave_edges(int(p[1]), None if p[2] == "none" else p[2])
    if p[0] == "g":
        return cs.wave_edges(128, p[1])
    if name.startswith("h-copy"):
        return cs.long_copy(int(p[2]))
    if name == "h-28rows":
        return cs.range_batch((500, -5, -500), 28)
    if p[0] == "h":
        return cs.range_batch(tuple(int(v) for v in name[2:].split("_")))
    return cs.la32_batch(int(p[1]), tuple(int(v) for v in name.split("-", 2)[2].split("_")))


class Known:
    """A case, the oracle's scores and what the model says the kernel does (None for NO_MODEL)."""

    def __init__(self, name):
        self.name = name
        self.case = _build(name)
        self.want = _want(self.case)
        c = self.case
        self.model = None if name in NO_MODEL else model.run(c.pairs, *c.prm, c.min_score)
        order, first16 = model.routing(c.pairs, *c.prm)
        self.n_int32, self.n_packed16 = first16, len(c.pairs) - first16
        self.closed_form = model.closed_form(c.pairs, *c.prm)


@pytest.fixture(scope="module")
def known():
    """Computed once, read by the CPU and the GPU tests, never changed."""
    from defuse_amd import build
    build.build_oracle()
    return {name: Known(name) for name in NAMES}


def contract_breach(case, want, got):
    """None if `got` is what la_align_batch_min may return: exact where the score reaches its minimum (everywhere without
    one), else anything in [0, minimum).  Otherwise a description of the first pair that is not."""
    got = np.asarray(got, dtype=np.int64)
    if case.min_score is None:
        bad = got != want
    else:
        hit = want >= case.min_score
        bad = np.where(hit, got != want, (got < 0) | (got >= case.min_score))
    if not bad.any():
        return None
    k = int(np.nonzero(bad)[0][0])
    return "pair %d: got %d, oracle %d, minimum %s" % (k, got[k], want[k], None if case.min_score is None else int(case.min_score[k]))


# ---------------------------------------------------------------------------------------------- CPU
def test_model_obeys_the_contract(known):
    for name, kn in known.items():
        if kn.model is not None:
            assert contract_breach(kn.case, kn.want, kn.model.scores) is None, name
            assert (kn.model.n_packed16, kn.model.n_int32) == (kn.n_packed16, kn.n_int32)


def test_expected_scores_of_the_built_cases(known):
    """The cases are what their descriptions say, by the oracle."""
    for L in cs.ZERO_SLACK_L:
        assert list(known["a-%d-1000" % L].want) == [1000] and list(known["a-%d-1001" % L].want) == [1000]
    assert list(known["b"].want) == [600, 1000]
    for L in cs.ONE_LIVE_L:
        w = known["c-%d" % L].want
        assert w[cs.ONE_LIVE_AT] == 1000 and np.all(np.delete(w, cs.ONE_LIVE_AT) < 800)
    assert np.all(known["d"].want < 800)                      # the precondition of (d): no pair reaches the minimum
    assert (known["e-0"].want > 0).sum() > 150
    for n in (127, 128, 129):
        kn = known["f-%d-0.8" % n]
        hit = kn.want >= kn.case.min_score
        assert hit.sum() > 20 and (~hit).sum() > 20
        ls = [len(s) for _, s in kn.case.pairs]
        assert all(ls.count(v) >= 2 for v in (0, 1, 3, 4, 5)) and max(ls) > 90
        assert {len(r) for r, _ in kn.case.pairs} == set(cs.REF_LENS)
    assert list(known["h-copy-1863"].want) == [18630] and list(known["h-copy-1864"].want) == [18640]


def test_cases_reach_their_paths(known):
    for L in cs.ZERO_SLACK_L:                                  # (a) dead tiles leave after one group, tile 3 lives on l_in
        (sw,) = known["a-%d-1000" % L].model.swept
        assert len(sw) == 8 and sw[0] == 1 and sw[3] == 26 and sw[4:] == [1, 1, 1, 1], (L, sw)
        assert sw[1] == 1 or L > 64                            # L = 99: the copy starts in tile 1
        assert known["a-%d-1001" % L].model.swept == [[1] * 8]
    assert known["a-43-1000"].model.swept == [[1, 1, 12, 26, 1, 1, 1, 1]]
    (sw,) = known["b"].model.swept                             # (b) tile 3 sweeps rows that tile 2 never wrote
    assert sw[2] < 11 and sw[3] >= 16 and sw == [20, 20, 5, 21, 26, 26]
    (dead,) = known["d"].model.swept                           # (d) every tile stops early
    assert len(dead) == 8 and all(g < 26 for g in dead)
    for L in cs.ONE_LIVE_L:                                    # (c) one lane carries the tiles of its path to the last row
        (sw,) = known["c-%d" % L].model.swept
        first, last = (192 - L) // 64, (291 - L) // 64
        assert sw[last] == 26 and max(sw[:first]) < 26 and sw[7] < 26, (L, sw)      # the others stop where they die
    for name in ("e-0", "e-1", "f-127-0.8", "f-128-0.8", "f-129-0.8", "g-max", "g-zero"):
        assert 0 < known[name].model.row_groups < known[name].closed_form, name
    assert known["g-max"].model.row_groups == 5               # one group per tile: nothing is ever alive


@pytest.mark.parametrize("mutate,fails,passes", [
    ("no_l_in", ["a-%d-1000" % L for L in cs.ZERO_SLACK_L], []),
    ("l_in_ge", ["a-%d-1000" % L for L in (39, 43, 63, 99)], ["a-%d-1000" % L for L in (40, 41, 42, 64)]),
    ("thr_high", ["a-%d-1000" % L for L in cs.ZERO_SLACK_L], []),
    ("read_plane", ["b"], []),
])
def test_an_error_in_the_stop_rule_fails_the_cases(known, mutate, fails, passes):
    """A kernel with this error could not pass: the model with the error breaks the contract on the named cases."""
    for name in fails + passes:
        kn = known[name]
        got = model.run(kn.case.pairs, *kn.case.prm, kn.case.min_score, mutate=mutate).scores
        assert (contract_breach(kn.case, kn.want, got) is not None) == (name in fails), (mutate, name, got)
        if name == "b":
            assert got[0] >= 800 and kn.want[0] == 600         # the stale plane makes a hit of the miss


def test_closed_form_without_a_minimum(known):
    seen = 0
    for name, kn in known.items():
        if kn.model is not None and kn.case.min_score is None:
            assert kn.model.row_groups == kn.closed_form == kn.model.closed_form, name
            seen += kn.n_packed16 > 0
    assert seen >= 10
    assert known["g-min"].model.row_groups == known["g-min"].closed_form       # a minimum nothing falls below
    assert known["h-copy-1863"].closed_form == 30 * 466 and known["h-copy-1864"].closed_form == 0


def test_routing_and_range_limits(known):
    for prm in cs.PACKED_SCORINGS:
        kn = known["h-%d_%d_%d" % prm]
        assert (kn.n_packed16, kn.n_int32) == (5, 0)
        top = model.BIAS + 27 * 1000 if prm != (-3, -4, 0) else model.BIAS
        assert (kn.model.hi, kn.model.lo) == (top, model.BIAS + prm[2]), prm
    assert known["h-0_-1000_-1000"].model.lo == known["h-0_0_-1000"].model.lo == 1048 and known["h-0_0_-1000"].model.hi == 29048
    for prm in cs.INT32_SCORINGS:
        kn = known["h-%d_%d_%d" % prm]
        assert (kn.n_packed16, kn.n_int32) == (0, 5)
    kn = known["h-28rows"]
    assert (kn.n_packed16, kn.n_int32) == (2, 3) and sorted(len(s) for _, s in kn.case.pairs)[-3:] == [28, 28, 28]
    assert (known["h-copy-1863"].n_packed16, known["h-copy-1864"].n_int32) == (1, 1)
    assert model.BIAS + 1863 * 15 == 29993 <= model.Y_LIMIT < model.BIAS + 1864 * 15
    for name, kn in known.items():
        if name[0] == "i":
            assert kn.n_packed16 == 0


# ---------------------------------------------------------------------------------------------- GPU
def _check_gpu(kn):
    from defuse_amd import la
    c = kn.case
    got, t = la.align_batch(c.pairs, *c.prm, min_score=c.min_score)
    assert contract_breach(c, kn.want, got) is None, kn.name
    assert (t.n_packed16, t.n_int32) == (kn.n_packed16, kn.n_int32), kn.name
    if kn.model is not None:
        assert t.row_groups16 == kn.model.row_groups, (kn.name, t.row_groups16, kn.model.swept)
    if c.min_score is None:
        assert t.row_groups16 == kn.closed_form, kn.name
    return got, t


@pytest.mark.gpu
@pytest.mark.parametrize("group", "abcdefghi")
def test_gpu_scores_and_row_groups(built, known, group):
    names = [n for n in NAMES if n[0] == group]
    assert names
    for name in names:
        _check_gpu(known[name])


@pytest.mark.gpu
def test_gpu_windows_entry_sweeps_the_same(built, known):
    from defuse_amd import la
    for name in ("f-129-0.8", "f-129-none"):
        kn = known[name]
        got, t = _check_gpu(kn)
        data, reads, windows = cs.windows_of(kn.case.pairs)
        with la.genome(data) as gen:
            got_w, t_w = la.align_windows(gen, reads, windows, *kn.case.prm, min_score=kn.case.min_score)
        assert np.array_equal(got_w, got)
        assert (t_w.row_groups16, t_w.n_packed16, t_w.n_int32) == (t.row_groups16, t.n_packed16, t.n_int32)
