"""The batches of tests/test_la_stop.py: inputs that make k_la16's early stop, its boundary rules and the 16-bit routing
limits decide a score.  Everything is built from fixed seeds.  A case is (pairs, scoring, minimum scores or None)."""
import numpy as np

PIPELINE = (10, -5, -5)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
ZERO_SLACK_L = (39, 40, 41, 42, 43, 63, 64, 99)
ONE_LIVE_L = (1, 4, 41, 100)
ONE_LIVE_AT = 77                     # lane 38, high field
SEQ_LENS = (0, 0, 0, 1, 1, 3, 3, 4, 4, 5, 5)         # wave_edges: these first, then 0..100 at random
REF_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 300)
PACKED_SCORINGS = ((0, -1000, -1000), (0, 0, -1000), (500, -5, -500), (1000, 0, 0), (500, -500, -500), (-3, -4, 0))
INT32_SCORINGS = ((0, -1001, -1001), (501, -5, -500), (0, 1, -1), (0, 0, 1))
LA32_SCORINGS = ((5, 2, -1), (3, -2, 1), (10, -5, -2000))


class Case:
    def __init__(self, pairs, min_score=None, prm=PIPELINE):
        self.pairs = pairs
        self.prm = prm
        self.min_score = None if min_score is None else np.asarray(min_score, dtype=np.int64)


def _s(rng, n, alphabet=ACGT):
    return rng.choice(alphabet, size=n).tobytes()


def _embed(n_ref, at, seq, fill=None):
    ref = bytearray(b"N" * n_ref if fill is None else fill)
    assert len(ref) == n_ref and 0 <= at and at + len(seq) <= n_ref
    ref[at:at + len(seq)] = seq
    return bytes(ref)


def zero_slack(L, need):
    """(a) a perfect copy whose row L sits in the last column of tile 2; need 1000 is its score, 1001 is out of reach."""
    seq = _s(np.random.default_rng(100 + L), 100)
    return Case([(_embed(512, 192 - L, seq), seq)], [need])


def split_copy():
    """(b) pair A's copy is cut in two (60 rows in tile 0, 40 in tile 3: 600), pair B's is whole in tiles 3 and 4 (1000)."""
    rng = np.random.default_rng(200)
    sa, sb = _s(rng, 100), _s(rng, 100)
    ref_a = _embed(384, 192, sa[60:], _embed(384, 4, sa[:60]))
    return Case([(ref_a, sa), (_embed(384, 192, sb), sb)], [800, 800])


def dead_pairs(rng, n):
    return [(_s(rng, 512), _s(rng, 100)) for _ in range(n)]


def one_live(L):
    """(c) 127 unrelated pairs and one that carries a perfect copy as in (a), in a random reference."""
    rng = np.random.default_rng(300 + L)
    pairs = dead_pairs(rng, 127)
    seq = _s(rng, 100)
    pairs.insert(ONE_LIVE_AT, (_embed(512, 192 - L, seq, _s(rng, 512)), seq))
    return Case(pairs, [800] * 128)


def all_dead():
    """(d) a wave in which nothing reaches the minimum."""
    return Case(dead_pairs(np.random.default_rng(400), 128), [800] * 128)


def at_minimum(want, delta):
    """(e) every pair's minimum is its own score (+ delta)."""
    from tests.test_localalign import random_pairs
    pairs = random_pairs(500, 256, related=0.7)
    return Case(pairs, None if want is None else np.asarray(want, dtype=np.int64) + delta)


def wave_edges(n, minimum="0.8"):
    """(f), (g) n pairs with sequences of 0..100 bases and references at the tile edges; every second pair is related."""
    rng = np.random.default_rng(600 + n)
    pairs = []
    for k in range(n):
        ls = SEQ_LENS[k] if k < len(SEQ_LENS) and n > 1 else int(rng.integers(0, 101))
        ref = _s(rng, REF_LENS[int(rng.integers(0, len(REF_LENS)))])
        seq = _s(rng, ls)
        if k % 2 == 0 and len(ref) > 0 and ls > 0:
            at = int(rng.integers(0, len(ref)))
            seq = (ref[at:at + ls] + seq)[:ls]
        pairs.append((ref, seq))
    need = {None: None, "0.8": [int(np.ceil(0.8 * 10 * len(s))) for _, s in pairs], "max": [INT32_MAX] * n,
            "min": [INT32_MIN] * n, "zero": [0] * n}[minimum]
    return Case(pairs, need)


def windows_of(pairs):
    """The batch as la.align_windows takes it: the references end to end as the genome."""
    genome = b"".join(r for r, _ in pairs)
    offs = np.cumsum([0] + [len(r) for r, _ in pairs])
    return genome, [s for _, s in pairs], [(k, int(offs[k]), len(pairs[k][0]), 0, 0, 0) for k in range(len(pairs))]


def long_copy(n):
    """(h) a perfect copy of n bases: 1863 rows are the most the packed kernel takes at the pipeline's scoring."""
    rng = np.random.default_rng(700 + n)
    q = _s(rng, n)
    return Case([(_s(rng, 20) + q + _s(rng, 10), q)])


def range_batch(prm, n=27):
    """(h) a perfect copy of n bases at scorings that put the 16-bit fields at the ends of their range."""
    rng = np.random.default_rng(800 + n)
    q = _s(rng, n)
    return Case([(_s(rng, 40) + q + _s(rng, 30), q), (q, q), (_s(rng, 130), _s(rng, 27)), (b"", q), (q, b"")], prm=prm)


def la32_batch(n, prm):
    """(i) n pairs for the int32 kernel."""
    rng = np.random.default_rng(900 + n)
    al = np.frombuffer(b"ACGTN", dtype=np.uint8)
    lens = SEQ_LENS + tuple(range(6, 101))
    pairs = [(_s(rng, REF_LENS[int(rng.integers(0, len(REF_LENS)))], al), _s(rng, lens[int(rng.integers(0, len(lens)))], al))
             for _ in range(n)]
    return Case(pairs, prm=prm)
