"""Seeded candidate batches for the parity tests (shared by CPU and GPU tests)."""
import numpy as np

from defuse_amd.dsa import FUSION_DTYPE, PAIR_DTYPE


class BatchBuilder:
    def __init__(self):
        self.ref = bytearray()
        self.reads = bytearray()
        self.fusions = []
        self.pairs = []

    def add_fusion(self, ref0: bytes, ref1: bytes, fusion_id=None):
        idx = len(self.fusions)
        o0 = len(self.ref)
        self.ref += ref0
        o1 = len(self.ref)
        self.ref += ref1
        self.fusions.append((idx if fusion_id is None else fusion_id, o0, len(ref0), o1, len(ref1)))
        return idx

    def add_read(self, fusion_idx, read: bytes, frag=None, read_end=0, revcomp=0):
        off = len(self.reads)
        self.reads += read
        self.pairs.append((fusion_idx, off, len(read), len(self.pairs) if frag is None else frag, read_end, revcomp, (0, 0)))

    def arrays(self):
        ref = np.frombuffer(bytes(self.ref), dtype=np.uint8).copy()
        reads = np.frombuffer(bytes(self.reads), dtype=np.uint8).copy()
        return ref, np.array(self.fusions, dtype=FUSION_DTYPE), reads, np.array(self.pairs, dtype=PAIR_DTYPE)


def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).tolist())


def mutate(rng, s: bytes, rate):
    b = bytearray(s)
    for i in range(len(b)):
        if rng.random() < rate:
            b[i] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8))
    return bytes(b)


def split_read(rng, ref0, ref1, lq, first=None, s1=None, a=None):
    first = int(rng.integers(min(lq, len(ref0)), len(ref0) + 1)) if first is None else first
    s1 = int(rng.integers(0, max(1, len(ref1) - lq + 1))) if s1 is None else s1
    a = int(rng.integers(0, min(lq, first) + 1)) if a is None else a
    return (ref0[first - a:first] + ref1[s1:s1 + lq - a])[:lq]


def mixed_batch(seed, n_fusions=12, reads_per_fusion=40, lq=50, lr=(100, 260)):
    """Split reads, unsplit reads, random reads, Ns, lowercase, variable lengths, odd window sizes."""
    rng = np.random.default_rng(seed)
    bb = BatchBuilder()
    for f in range(n_fusions):
        l0 = int(rng.integers(lr[0], lr[1]))
        l1 = int(rng.integers(lr[0], lr[1]))
        alpha = b"ACGT" if f % 4 else b"ACGTN"
        ref0, ref1 = rnd(rng, l0, alpha), rnd(rng, l1, alpha)
        if f % 5 == 3:
            ref0 = ref0[: l0 // 2] + ref0[: l0 // 2].lower()[::-1] + ref0[l0 // 2:]
        fi = bb.add_fusion(ref0, ref1, fusion_id=1000 + 7 * f)
        n = reads_per_fusion + (int(rng.integers(0, 120)) if f % 3 == 0 else 0)
        for r in range(n):
            kind = rng.integers(0, 10)
            q = lq if kind < 7 else int(rng.integers(0, lq + 20))
            if kind <= 5:
                read = split_read(rng, ref0, ref1, q)
            elif kind == 6:
                p = int(rng.integers(0, max(1, l0 - q)))
                read = ref0[p:p + q]                      # aligns unsplit to window 0
            elif kind == 7:
                p = int(rng.integers(0, max(1, l1 - q)))
                read = ref1[p:p + q]                      # aligns unsplit to window 1
            else:
                read = rnd(rng, q)
            read = mutate(rng, read, 0.02)
            if rng.random() < 0.05 and len(read) > 0:
                b = bytearray(read)
                b[int(rng.integers(0, len(b)))] = ord("N")
                read = bytes(b)
            if rng.random() < 0.03:
                read = read.lower()
            bb.add_read(fi, read, read_end=int(r & 1), revcomp=int((r >> 1) & 1))
    return bb.arrays()


def tie_batch(seed):
    """Low-complexity sequence: homopolymers and tandem repeats around the junction, so that many
    columns and many read splits tie (tools/SplitReadAligner.cpp:233-269 emits all of them)."""
    rng = np.random.default_rng(seed)
    bb = BatchBuilder()
    unit = b"ACG"
    cases = [
        (b"A" * 90, b"A" * 70, [b"A" * 30, b"A" * 12, b"A" * 7]),
        (rnd(rng, 40) + b"T" * 40 + rnd(rng, 50), rnd(rng, 30) + b"T" * 25 + rnd(rng, 60), None),
        (rnd(rng, 30) + unit * 20 + rnd(rng, 40), rnd(rng, 50) + unit * 15 + rnd(rng, 20), None),
        (rnd(rng, 140), rnd(rng, 150), None),
    ]
    for ref0, ref1, reads in cases:
        fi = bb.add_fusion(ref0, ref1)
        if reads is None:
            reads = []
            for _ in range(24):
                q = int(rng.integers(20, 45))
                reads.append(split_read(rng, ref0, ref1, q))
            # a read made of the repeat itself
            reads.append((unit * 12)[:30])
            reads.append(b"T" * 28)
        for r in reads:
            bb.add_read(fi, r)
    # one fusion whose window 1 contains window 0's tail twice (two tied columns on one side)
    core = rnd(rng, 25)
    ref0 = rnd(rng, 60) + core
    ref1 = rnd(rng, 10) + rnd(rng, 30) + rnd(rng, 70)
    fi = bb.add_fusion(ref0 + rnd(rng, 20), ref1)
    dup0 = rnd(rng, 50) + core + rnd(rng, 37) + core + rnd(rng, 11)
    fj = bb.add_fusion(dup0, ref1)
    for s1 in (0, 5, 17):
        bb.add_read(fi, core + ref1[s1:s1 + 20])
        bb.add_read(fj, core + ref1[s1:s1 + 20])
        bb.add_read(fj, core[5:] + ref1[s1:s1 + 25])
    return bb.arrays()


def repeat_batch(seed, n_fusions=40, reads_per_fusion=100, lq=60):
    """Full workgroups of repeat-rich fusions: windows of several tiles that hold a tandem repeat, a duplicated segment or a
    junction on a tile boundary, with a hundred reads each, so that pairs have many kept splits in several tiles (the emit
    paths for many masks, runs of such pairs in one wave, many generic replay tasks, device buffers that overflow and make the
    host re-run the slice) next to ordinary fusions."""
    rng = np.random.default_rng(seed)
    bb = BatchBuilder()
    for f in range(n_fusions):
        kind = f % 5
        if kind == 0:                      # tandem repeat across two tiles of window 0, plain window 1
            unit = rnd(rng, int(rng.integers(2, 7)))
            ref0 = rnd(rng, 40) + (unit * 60)[:150] + rnd(rng, 30)
            ref1 = rnd(rng, 200)
        elif kind == 1:                    # window 1 holds a segment three times, tiles apart
            seg = rnd(rng, 30)
            ref0 = rnd(rng, 230)
            ref1 = seg + rnd(rng, 50) + seg + rnd(rng, 70) + seg + rnd(rng, 20)
        elif kind == 2:                    # junction on a tile boundary, both sides continue alike (several kept splits)
            shared = rnd(rng, 6)
            ref0 = rnd(rng, 128 - 3) + shared + rnd(rng, 80)
            ref1 = shared + rnd(rng, 180)
        elif kind == 3:                    # homopolymer stretches on both sides
            ref0 = rnd(rng, 70) + b"A" * 80 + rnd(rng, 60)
            ref1 = b"A" * 40 + rnd(rng, 160)
        else:
            ref0, ref1 = rnd(rng, 389), rnd(rng, 389)
        fi = bb.add_fusion(ref0, ref1)
        for r in range(reads_per_fusion):
            if kind == 2:
                a = int(rng.integers(8, lq - 8))
                read = ref0[125 + 3 - a:125 + 3] + ref1[3:3 + lq - a] if r % 3 else split_read(rng, ref0, ref1, lq)
            elif kind == 1 and r % 2:
                a = int(rng.integers(6, lq - 20))
                s0 = int(rng.integers(a, len(ref0)))
                read = ref0[s0 - a:s0] + ref1[:lq - a]       # the suffix starts with the repeated segment
            elif kind == 0 and r % 2:
                a = int(rng.integers(10, lq - 10))
                read = ref0[40 + 150 - a:40 + 150] + ref1[:lq - a]      # the prefix lies in the repeat
            elif kind == 3 and r % 2:
                a = int(rng.integers(10, lq - 10))
                read = (b"A" * a) + ref1[40 - (lq - a) // 3:][:lq - a]
            else:
                read = split_read(rng, ref0, ref1, lq)
            if r % 7 == 0:
                read = mutate(rng, read, 0.03)
            bb.add_read(fi, read, read_end=int(r & 1), revcomp=int((r >> 1) & 1))
    return bb.arrays()


def edge_batch():
    """Degenerate shapes: empty read, read shorter than the 4-base anchor, empty window, window
    shorter than one tile, window of exactly one/two tiles, ungrouped pairs."""
    rng = np.random.default_rng(99)
    bb = BatchBuilder()
    r0, r1 = rnd(rng, 64), rnd(rng, 128)
    f0 = bb.add_fusion(r0, r1)
    f1 = bb.add_fusion(rnd(rng, 10), rnd(rng, 200))
    f2 = bb.add_fusion(b"", rnd(rng, 80))
    f3 = bb.add_fusion(rnd(rng, 65), b"")
    f4 = bb.add_fusion(rnd(rng, 63), rnd(rng, 129))
    refs = {f0: (r0, r1)}
    for f in (f0, f1, f2, f3, f4, f0, f4, f1):     # deliberately not grouped by fusion
        bb.add_read(f, b"")
        bb.add_read(f, rnd(rng, 3))
        bb.add_read(f, rnd(rng, 8))
        bb.add_read(f, rnd(rng, 33))
        bb.add_read(f, r0[30:64] + r1[0:30])
        bb.add_read(f, r0[40:64] + r1[100:128])
    return bb.arrays()


_COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def chunk_genome(rng, length=300_000):
    """A synthetic genome with what makes windows and reads of the real one awkward: tandem repeats and duplicated segments (tied
    columns and read splits), soft-masked lowercase stretches and runs of N."""
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=length)].copy()
    for _ in range(length // 2000):                           # tandem repeats, units of 1-6 bases over 20-200 bases
        unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(rng.integers(1, 7)))]
        n = int(rng.integers(20, 201))
        p = int(rng.integers(0, length - n))
        g[p:p + n] = np.resize(unit, n)
    for _ in range(length // 5000):                           # duplicated segments of 100-600 bases, 1 % diverged
        n = int(rng.integers(100, 601))
        a, b = int(rng.integers(0, length - n)), int(rng.integers(0, length - n))
        seg = g[a:a + n].copy()
        mut = rng.random(n) < 0.01
        seg[mut] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(mut.sum()))]
        g[b:b + n] = seg
    for _ in range(length // 4000):                           # soft-masked stretches
        n = int(rng.integers(30, 400))
        p = int(rng.integers(0, length - n))
        g[p:p + n] |= 0x20
    for _ in range(length // 20000):                          # runs of N
        n = int(rng.integers(5, 120))
        p = int(rng.integers(0, length - n))
        g[p:p + n] = ord("N")
    return g.tobytes()


def chunk_batch(seed, n_pairs=100_000, lq=76, ufrag=300, sfrag=30, long_read=False):
    """Candidates in the shape dosplitalign enumerates them for one chunk of reads (SplitReadRealigner::DoAlignment,
    tools/SplitAlignment.cpp:266-303): many fusions with 1-7 candidates of their own (and now and then one a neighbouring fusion shares), windows cut from one genome (repeats, duplicated
    segments, soft-masked lowercase, runs of N) whose lengths follow synth.window_length over region lengths that differ per
    fusion and per side (windows shorter than the read included), pairs in read-major order (one fusion's candidates are not
    contiguous, a read is a candidate of several fusions), reads that cross the junction, lie inside one window, align nowhere,
    and their reverse complements.  long_read: one read of 7700 bases, for the 32-bit kernels.  Deterministic in the arguments."""
    from defuse_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = chunk_genome(rng)
    G = len(genome)
    bb = BatchBuilder()
    max_region = synth.window_length(ufrag, sfrag, lq, lq, 0) + 2 * lq - 8      # longer regions leave windows of fewer than 8 bases
    wins = []
    n_fusions = 0
    cand = []                                  # (read order key, fusion, read bytes, revcomp)
    while len(cand) < n_pairs:
        f = n_fusions
        n_fusions += 1
        sides = []
        for _ in range(2):
            region = int(rng.integers(1, max_region))
            lr = synth.window_length(ufrag, sfrag, lq, lq, region)
            p = int(rng.integers(0, G - lr))
            sides.append(genome[p:p + lr])
        ref0, ref1 = sides
        bb.add_fusion(ref0, ref1, fusion_id=3 * f + 1)
        wins.append((ref0, ref1))
        for _ in range(int(rng.integers(1, 8))):
            kind = int(rng.integers(0, 10))
            if kind < 5:                                       # crosses the junction
                a = int(rng.integers(4, lq - 3))
                first = int(rng.integers(0, len(ref0) + 1))
                s1 = int(rng.integers(0, len(ref1) + 1))
                read = (ref0[max(0, first - a):first] + ref1[s1:s1 + lq - a])
            elif kind < 7:                                     # inside one window
                w = ref0 if kind == 5 else ref1
                p = int(rng.integers(0, max(1, len(w) - lq + 1)))
                read = w[p:p + lq]
            else:                                              # a decoy from elsewhere in the genome
                p = int(rng.integers(0, G - lq))
                read = genome[p:p + lq]
            if len(read) < lq:                                 # a short window: the read goes on in the genome
                p = int(rng.integers(0, G - lq))
                read = read + genome[p:p + lq - len(read)]
            read = read.upper()
            rc = int(rng.integers(0, 2))
            if rc:
                read = revcomp(read)
            cand.append((int(rng.integers(0, 1 << 30)), f, read, rc))
            if rng.random() < 0.15 and f > 0:                  # the same read is a candidate of a neighbouring fusion too
                cand.append((cand[-1][0], f - 1, read, rc))
    cand = cand[:n_pairs]
    order = sorted(range(len(cand)), key=lambda k: (cand[k][0], cand[k][1]))    # read-major
    reads = bytearray()
    offs = np.zeros(len(cand), dtype=np.int64)
    for j, k in enumerate(order):
        offs[j] = len(reads)
        reads += cand[k][2]
    buf = np.frombuffer(bytes(reads), dtype=np.uint8).copy()
    sub = rng.random(buf.size) < 0.01                          # sequencing errors, an N now and then
    buf[sub] = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=int(sub.sum()), p=[0.24, 0.24, 0.24, 0.24, 0.04])]
    if long_read:
        ref0, ref1 = wins[0]
        lr = 7700
        long = np.frombuffer((ref0 * (lr // max(1, len(ref0)) + 1))[:lr // 2] + (ref1 * (lr // max(1, len(ref1)) + 1))[:lr - lr // 2],
                             dtype=np.uint8)
        offs = np.append(offs, buf.size)
        buf = np.concatenate([buf, long])
    fusions = np.array(bb.fusions, dtype=FUSION_DTYPE)
    n = len(offs)
    pairs = np.zeros(n, dtype=PAIR_DTYPE)
    pairs["fusion_idx"][:len(order)] = [cand[k][1] for k in order]
    pairs["revcomp"][:len(order)] = [cand[k][3] for k in order]
    pairs["read_off"] = offs
    pairs["read_len"][:len(order)] = [len(cand[k][2]) for k in order]
    pairs["frag"][:len(order)] = [cand[k][0] >> 1 for k in order]
    pairs["read_end"][:len(order)] = [cand[k][0] & 1 for k in order]
    if long_read:                                             # among the first pairs, so that the first slice holds it
        pairs[-1] = (0, offs[-1], buf.size - offs[-1], 5, 0, 0, (0, 0))
        pairs = np.concatenate([pairs[:100], pairs[-1:], pairs[100:-1]])
    ref = np.frombuffer(bytes(bb.ref), dtype=np.uint8).copy()
    return ref, fusions, buf, pairs


def group_by_fusion(batch, exp):
    """The batch with its pairs stably sorted by fusion (the order dosplitalign hands them to the aligner in), and the oracle
    records `exp` of the original order rewritten for it (records follow their pairs; pair_idx renumbered)."""
    ref, fus, reads, pairs = batch
    perm = np.argsort(pairs["fusion_idx"], kind="stable")
    n = len(pairs)
    counts = np.bincount(exp["pair_idx"], minlength=n)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    c2 = counts[perm]
    first2 = np.concatenate([[0], np.cumsum(c2)[:-1]])
    idx = np.repeat(starts[perm] - first2, c2) + np.arange(int(c2.sum()))
    exp2 = exp[idx].copy()
    exp2["pair_idx"] = np.repeat(np.arange(n, dtype=np.int32), c2)
    return (ref, fus, reads, pairs[perm].copy()), exp2
