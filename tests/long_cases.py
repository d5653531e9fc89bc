"""Seeded batches for the 32-bit split-read path (defuse_amd/csrc/dsa_long.hpp): the window and read lengths at which the
per-thread column partition of long_row changes its layout, and batches that put long pairs where the grid-stride loop, the
slices, the emit and the context's state can go wrong.  No GPU is needed to build them (tests/test_dsa_long.py)."""
import numpy as np

from tests import cases

# restated from defuse_amd/csrc/dsa_long.hpp
LONG_THREADS = 256
FAST_MAX_READ = 7600
FAST_MAX_REF = 16320

# window length -> (nw, per) as dsa_long.hpp's long_row derives them: one over-long window beside a SHORT_WINDOW-base one
WINDOW_TABLE = {
    16321: (511, 2),     # thread 255 has one word
    16351: (511, 2),     # last word full
    16352: (512, 2),     # last word holds one column
    16383: (512, 2),     # last word full, every run full
    16384: (513, 3),     # 171 active threads, wave 3 wholly idle, wave 2 partly idle
    16385: (513, 3),     # same layout, last word holds two columns
    24543: (767, 3),     # last word full, thread 255 has two words
    24544: (768, 3),     # 256 x 3 words, last word holds one column
}
SHORT_WINDOW = 64
CONTROL_WINDOW = 16320   # the longest window of the 16-bit kernels: not a long pair

# (ref0_len, ref1_len) -> (nw of ref0, nw of ref1): windows the 16-bit kernels would take, under a read they do not
LONG_READ_TABLE = {
    (8159, 31): (255, 1),    # ref1: thread 0 alone, one full word
    (8191, 32): (256, 2),    # all 256 threads, per = 1; ref1: one column in word 1
    (8192, 33): (257, 2),    # per flips to 2: 129 active threads, thread 128 holds a one-column word
    (7570, 31): (237, 1),    # per = 1, idle threads inside the last wave only
}
LONG_READ = 7601


def layout(length):
    """The column partition of long_row for a window of `length` bases (columns 0..length)."""
    nw = (length + 1 + 31) // 32
    per = (nw + LONG_THREADS - 1) // LONG_THREADS
    active = (nw + per - 1) // per
    return dict(nw=nw, per=per, active=active, last_run=nw - (active - 1) * per, last_cols=length + 1 - 32 * (nw - 1))


def rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def corner_reads(bb, f, ref0, ref1):
    """Four 40-base reads whose junction sits at the last or among the first columns of either matrix."""
    for first in (len(ref0), 20):
        for s1 in (0, len(ref1) - 20):
            bb.add_read(f, cases.split_read(None, ref0, ref1, 40, first=first, s1=s1, a=20))


def window_edge_batch():
    """Every length of WINDOW_TABLE once as ref0 and once as ref1 beside a short window, four corner reads each, and the
    control fusion last.  Returns the batch and the number of pairs that are long."""
    rng = np.random.default_rng(1601)
    bb = cases.BatchBuilder()
    for length in WINDOW_TABLE:
        for flip in (0, 1):
            wide, short = rnd(rng, length), rnd(rng, SHORT_WINDOW)
            ref0, ref1 = (short, wide) if flip else (wide, short)
            corner_reads(bb, bb.add_fusion(ref0, ref1), ref0, ref1)
    n_long = len(bb.pairs)
    ref0, ref1 = rnd(rng, CONTROL_WINDOW), rnd(rng, SHORT_WINDOW)
    corner_reads(bb, bb.add_fusion(ref0, ref1), ref0, ref1)
    return bb.arrays(), n_long


def long_read_batch():
    """One read of LONG_READ bases across the junction of every fusion of LONG_READ_TABLE."""
    rng = np.random.default_rng(1602)
    bb = cases.BatchBuilder()
    for l0, l1 in LONG_READ_TABLE:
        ref0, ref1 = rnd(rng, l0), rnd(rng, l1)
        f = bb.add_fusion(ref0, ref1)
        bb.add_read(f, cases.mutate(rng, ref0[-(LONG_READ - l1):] + ref1, 0.01))
    return bb.arrays()


MANY_PAIRS = 513          # one more than run_long launches workgroups: block 0 takes pair 0 and then pair 512


def many_pairs_batch(second_turn_aligns, seed=1604):
    """MANY_PAIRS long pairs over two fusions of different shapes, alternating pair by pair; the alternation turns over at pair
    512, so that block 0 meets other window lengths in its second pair (512 is even).  Every sixteenth pair is a random read
    that aligns nowhere, and so is pair 512 (second_turn_aligns = False) or pair 0 (True); at this seed no other read takes the
    three substitutions that would put it below the minimum score.  Returns the batch and the pairs that are random reads."""
    rng = np.random.default_rng(seed)
    bb = cases.BatchBuilder()
    refs = [(rnd(rng, 16321), rnd(rng, 40)), (rnd(rng, 50), rnd(rng, 16352))]
    for r in refs:
        bb.add_fusion(*r)
    empty = set(range(7, MANY_PAIRS, 16)) | {0 if second_turn_aligns else MANY_PAIRS - 1}
    for p in range(MANY_PAIRS):
        f = (p & 1) ^ (p >> 9 & 1)
        ref0, ref1 = refs[f]
        read = cases.mutate(rng, cases.split_read(rng, ref0, ref1, 40, a=int(rng.integers(10, 31))), 0.01)
        noise = rnd(rng, 40)
        bb.add_read(f, noise if p in empty else read)
    return bb.arrays(), sorted(empty)


SLICE_PAIRS = 256


def slice_boundary_batch():
    """606 pairs, three slices of SLICE_PAIRS: an ordinary fusion's 76-base reads, and pairs of two fusions with one over-long
    window at the first and last index of every slice.  Nothing carries a default frag, read_end, revcomp or fusion_id.
    Returns the batch and the indices of the long pairs."""
    rng = np.random.default_rng(1605)
    bb = cases.BatchBuilder()
    s0, s1 = rnd(rng, 331), rnd(rng, 329)
    wide = [(rnd(rng, 16321), rnd(rng, 300)), (rnd(rng, 300), rnd(rng, 16352))]
    f_wide0 = bb.add_fusion(*wide[0], fusion_id=900001)
    f_short = bb.add_fusion(s0, s1, fusion_id=4242)
    f_wide = [f_wide0, bb.add_fusion(*wide[1], fusion_id=123456789)]
    n = 606
    long_at = [0, SLICE_PAIRS - 1, SLICE_PAIRS, 2 * SLICE_PAIRS - 1, 2 * SLICE_PAIRS, n - 1]
    for p in range(n):
        if p in long_at:
            k = long_at.index(p) & 1
            bb.add_read(f_wide[k], cases.split_read(rng, *wide[k], 76, a=int(rng.integers(20, 57))), frag=70000 - 3 * p, read_end=1, revcomp=1)
        else:
            bb.add_read(f_short, cases.mutate(rng, cases.split_read(rng, s0, s1, 76), 0.01), frag=5 * p + 2, read_end=p & 1, revcomp=(p >> 1) & 1)
    return bb.arrays(), long_at


MIN_SCORE_READ = 41       # min_score = int(82 * 0.9) = 73
MIN_SCORE_SUBS = (5, 14, 30, 36)


def min_score_batch():
    """ref0[-21:] + ref1[:20] with the first 0..4 of MIN_SCORE_SUBS substituted: 2 * 41 - 3 * k, which is the minimum score
    at k = 3.  Returns the batch, the windows and the reads."""
    rng = np.random.default_rng(1606)
    bb = cases.BatchBuilder()
    ref0, ref1 = rnd(rng, 16321), rnd(rng, 300)
    f = bb.add_fusion(ref0, ref1)
    reads = []
    for k in range(5):
        read = bytearray(ref0[-21:] + ref1[:20])
        for pos in MIN_SCORE_SUBS[:k]:
            read[pos] = ord("A") if read[pos] != ord("A") else ord("C")
        reads.append(bytes(read))
        bb.add_read(f, reads[-1])
    return bb.arrays(), (ref0, ref1), reads


def regrow_batch():
    """One fusion of 16321 + 16352 bases: J0 stands 40 times in ref0 (the last copy at its end), J1 30 times in ref1 (the first
    at its start); no copy of J0 is followed, none of J1 preceded by a T.  Reads J0 + J1 (40 x 30 tied columns at the split
    after J0, and more where a copy's neighbour happens to go on like the other segment) and J0 + T + J1 (the splits after J0
    and after the T tie)."""
    rng = np.random.default_rng(1607)
    j0, j1 = rnd(rng, 30), rnd(rng, 30)

    def filler(n):
        b = bytearray(rnd(rng, n))
        for k in (0, n - 1):
            if b[k] == ord("T"):
                b[k] = ord("G")
        return bytes(b)

    def repeated(j, copies, total):
        gaps = copies - 1
        room = total - copies * len(j)
        sizes = [room // gaps + (1 if k < room % gaps else 0) for k in range(gaps)]
        return b"".join(j + filler(s) for s in sizes) + j

    ref0 = filler(16321 - 16000) + repeated(j0, 40, 16000)
    ref1 = repeated(j1, 30, 16000) + filler(16352 - 16000)
    assert len(ref0) == 16321 and len(ref1) == 16352 and ref0.endswith(j0) and ref1.startswith(j1)
    bb = cases.BatchBuilder()
    f = bb.add_fusion(ref0, ref1)
    bb.add_read(f, j0 + j1)
    bb.add_read(f, j0 + b"T" + j1)
    return bb.arrays()


def moved_fusion_batch():
    """Sixteen ordinary fusions and then an over-long one: the fusion indices at which window_edge_batch has its over-long
    fusions hold ordinary ones here, and the index of its control fusion an over-long one."""
    rng = np.random.default_rng(1608)
    bb = cases.BatchBuilder()
    for _ in range(16):
        ref0, ref1 = rnd(rng, 150), rnd(rng, 170)
        f = bb.add_fusion(ref0, ref1)
        for _ in range(3):
            bb.add_read(f, cases.mutate(rng, cases.split_read(rng, ref0, ref1, 50), 0.01))
    n_short = len(bb.pairs)
    ref0, ref1 = rnd(rng, SHORT_WINDOW), rnd(rng, 16385)
    corner_reads(bb, bb.add_fusion(ref0, ref1), ref0, ref1)
    return bb.arrays(), len(bb.pairs) - n_short
