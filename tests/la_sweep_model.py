"""What the host of la_api.hip and its packed kernel k_la16 are documented to do (the header comment of
defuse_amd/csrc/la_api.hip), in plain integers — TEST INFRASTRUCTURE ONLY.  No fp16, no GPU.

Host part: the order (sequence length descending, reference length descending, index), the 16-bit / int32 split, waves of
128 (packed) or 64 (int32) consecutive pairs, nch / ls_max / rows4 per wave and the clamp of a minimum score.

Kernel part, per packed wave: the recurrence on the biased Y = H - gap*j with the clamped dm, dx, gd, the per-row thresholds,
rows_alive_at_zero, l_in, last_bnd, stop_prev, and the two boundary planes, which are written only for swept row groups and
only when another tile follows, and which start filled with POISON (device memory is not BIAS either).

The dependency along a row, X[i] = max(V[i], X[i-1] - gd), is a running maximum of V[i] + gd*i.

`mutate` puts one deliberate error into the stop rule; the CPU tests use it to prove that their cases would catch it:
    "no_l_in"     leave a tile at a dead row group without asking whether the entering boundary is still alive
    "l_in_ge"     4*gq+3 >= l_in instead of >
    "thr_high"    thresholds one too high
    "read_plane"  read the plane past the left tile's stop instead of taking Y = 0
"""
import numpy as np

W = 64
REF_PAD = 0x0100
ROW_PAD = 0x0200
BIAS = 0x0800
Y_LIMIT = 30000
NO_NEED = -0x40000000
POISON = Y_LIMIT                # a large live value: a read of a row nobody wrote shows
MUTATIONS = (None, "no_l_in", "l_in_ge", "thr_high", "read_plane")


class Result:
    """scores; swept[w][c] = row groups packed wave w swept in tile c; row_groups = their sum; hi / lo = the largest and
    smallest field value an operand of the packed recurrence took (None without a packed row); the routing counts."""

    def __init__(self, n):
        self.scores = np.zeros(n, dtype=np.int64)
        self.swept = []
        self.closed_form = 0
        self.hi = None
        self.lo = None
        self.n_packed16 = 0
        self.n_int32 = 0

    @property
    def row_groups(self):
        return sum(sum(t) for t in self.swept)

    def _seen(self, hi, lo):
        self.hi = hi if self.hi is None else max(self.hi, hi)
        self.lo = lo if self.lo is None else min(self.lo, lo)


def params(match, mismatch, gap):
    gd = -gap
    dm = max(match, 2 * gap) - gap
    dx = max(mismatch, 2 * gap) - gap
    return dm, dx, gd, max(match, 0)


def routing(pairs, match, mismatch, gap):
    """(order, first16): order[:first16] go to the int32 kernel, the rest to the packed one."""
    dm, dx, gd, _ = params(match, mismatch, gap)
    order = sorted(range(len(pairs)), key=lambda k: (-len(pairs[k][1]), -len(pairs[k][0]), k))
    scores16 = gap <= 0 and mismatch <= 0 and gd <= 1000 and 0 <= dm <= 1000 and 0 <= dx <= 1000
    first16 = len(pairs)
    if scores16:
        step = max(dm, dx, 1)
        first16 = 0
        while first16 < len(pairs) and BIAS + len(pairs[order[first16]][1]) * step > Y_LIMIT:
            first16 += 1
    return order, first16


def closed_form(pairs, match, mismatch, gap):
    """row_groups16 without a minimum score: sum over the packed waves of nch * ((ls_max >> 2) + 1)."""
    order, first16 = routing(pairs, match, mismatch, gap)
    total = 0
    for k in range(first16, len(pairs), 128):
        wave = [pairs[i] for i in order[k:k + 128]]
        nch = (max(len(r) for r, _ in wave) + W - 1) // W
        total += nch * ((max(len(s) for _, s in wave) >> 2) + 1)
    return total


def _align_int32(match, mismatch, gap, ref, seq):
    """One pair of the int32 kernel: the plain recurrence on H, row by row."""
    r = np.frombuffer(bytes(ref), dtype=np.uint8).astype(np.int64)
    idx = np.arange(1, len(r) + 1, dtype=np.int64)
    prev = np.zeros(len(r) + 1, dtype=np.int64)
    best = 0
    for j, q in enumerate(bytes(seq), 1):
        v = np.maximum(prev[:-1] + np.where(r == q, match, mismatch), prev[1:] + gap)
        # H[i] = max(v[i], H[i-1] + gap): a running maximum of v[i] - gap*i, started at H(0,j) = j*gap
        z = np.maximum.accumulate(np.concatenate([[j * gap], v - gap * idx]))
        cur = z + gap * np.arange(0, len(r) + 1, dtype=np.int64)
        if len(r):
            best = max(best, int(cur[1:].max()))
        prev = cur
    return best


def _rows_alive_at_zero(base, ls, slope):
    if ls <= 0:
        return 0
    if base - BIAS <= 0 and slope <= 0:
        return ls
    if base - BIAS > 0:
        return 0
    return min(ls, (BIAS - base) // slope)


def _wave16(res, wave, need, prm, mutate):
    """One packed wave: `wave` is a list of up to 128 (index, ref, seq), need the clamped minimum of each."""
    dm, dx, gd, mp = prm
    P = 128
    lr = np.zeros(P, dtype=np.int64)
    ls = np.zeros(P, dtype=np.int64)
    nd = np.full(P, NO_NEED, dtype=np.int64)
    for k, (_, r, s) in enumerate(wave):
        lr[k], ls[k], nd[k] = len(r), len(s), need[k]
    nch = (int(lr.max()) + W - 1) // W
    ls_max = int(ls.max())
    rows4 = (ls_max + 1 + 3) & ~3
    ngq = (ls_max >> 2) + 1
    res.closed_form += nch * ngq
    refc = np.full((P, nch * W), REF_PAD, dtype=np.int64)
    rowc = np.full((P, rows4), ROW_PAD, dtype=np.int64)
    for k, (_, r, s) in enumerate(wave):
        refc[k, :len(r)] = np.frombuffer(bytes(r), dtype=np.uint8)
        rowc[k, 1:len(s) + 1] = np.frombuffer(bytes(s), dtype=np.uint8)

    slope = mp + gd
    base = nd - mp * ls + BIAS
    thr_add = 1 if mutate == "thr_high" else 0
    planes = np.full((2, P, rows4), POISON, dtype=np.int64)
    gdi = gd * np.arange(W, dtype=np.int64)
    best = np.zeros(P, dtype=np.int64)
    l_in = max(_rows_alive_at_zero(int(base[k]), int(ls[k]), slope) for k in range(P))
    stop_prev = 0
    swept = []
    for c in range(nch):
        r = refc[:, c * W:(c + 1) * W]
        X = np.full((P, W), BIAS, dtype=np.int64)             # row 0: Y = 0
        pin, pout = planes[(c - 1) & 1], planes[c & 1]
        bprev = np.full(P, BIAS, dtype=np.int64)
        last_bnd = 0
        gq = 0
        while gq < ngq:
            from_plane = c > 0 and (gq < stop_prev or mutate == "read_plane")
            bo = np.full((P, 4), BIAS, dtype=np.int64)
            alive_any = False
            for s in range(4):
                j = 4 * gq + s
                bcur = pin[:, j].copy() if from_plane else np.full(P, BIAS, dtype=np.int64)     # past the left tile's stop: Y = 0
                if 1 <= j <= ls_max:
                    term = np.where(r == rowc[:, j:j + 1], dm, dx)
                    a = np.concatenate([bprev[:, None], X[:, :-1]], axis=1) + term          # diagonal
                    v = np.maximum(a, X)                                                    # ... or from the row above
                    z = np.maximum.accumulate(np.concatenate([(bcur - gd)[:, None], v + gdi], axis=1), axis=1)[:, 1:]
                    X = z - gdi                                                             # ... or from the left
                    res._seen(int(max(a.max(), X.max())), int(min((bcur - gd).min(), (X - gd).min())))
                    m = np.maximum(X.max(axis=1), BIAS)
                    counts = j <= ls
                    best = np.where(counts, np.maximum(best, m - (BIAS + gd * j)), best)
                    t = np.where(counts, np.clip(base + slope * j + thr_add - 1, 0, 0xFFFE), 0xFFFF)
                    alive_any = alive_any or bool((m > t).any())
                    if (X[:, W - 1] > t).any():
                        last_bnd = j
                    bo[:, s] = X[:, W - 1]
                bprev = bcur
            if c + 1 < nch:
                pout[:, 4 * gq:4 * gq + 4] = bo
            # a live boundary value at row l_in also enters row l_in + 1 (diagonal move): sweep past it
            past = True if mutate == "no_l_in" else 4 * gq + 3 >= l_in if mutate == "l_in_ge" else 4 * gq + 3 > l_in
            gq += 1
            if past and not alive_any:
                break
        stop_prev = gq
        swept.append(gq)
        l_in = last_bnd
    res.swept.append(swept)
    for k, (i, _, _) in enumerate(wave):
        res.scores[i] = best[k]


def run(pairs, match, mismatch, gap, min_score=None, mutate=None):
    """The scores la_align_batch_min returns for `pairs` ((reference, sequence) byte strings), and how it got there."""
    assert mutate in MUTATIONS
    res = Result(len(pairs))
    prm = params(match, mismatch, gap)
    order, first16 = routing(pairs, match, mismatch, gap)
    res.n_int32, res.n_packed16 = first16, len(pairs) - first16
    for i in order[:first16]:                                  # waves of 64; the lanes do not interact
        res.scores[i] = _align_int32(match, mismatch, gap, *pairs[i])
    for k in range(first16, len(pairs), 128):
        wave = [(i, pairs[i][0], pairs[i][1]) for i in order[k:k + 128]]
        need = [NO_NEED if min_score is None else max(min(int(min_score[i]), prm[3] * len(s) + 1), NO_NEED) for i, _, s in wave]
        _wave16(res, wave, need, prm, mutate)
    return res
