"""matealign throughput on one MI355X (profiles/matealign/): a seeded synthetic genome (24 contigs, 200 Mb), 1 M fragments 2x100,
1-4 mate alignments per read, `-s 500 -m 2 -x -1 -g -2`.

    python profiles/microbench/matealign_throughput.py [--frags N] [--mb M] [--ab-pairs K] [--skip-tool] [--out DIR]

1. bin/matealign end to end with DEFUSE_TIMING=1: wall time, its stage lines, and a fixed sample of 300 reads whose output lines
   are checked against tests/matealign_oracle.py's windows and oracle.localalign_oracle.simple_align;
2. an A/B on the same K pairs (windows of the run above): la_align_windows_min (genome in HBM, k_pack_win) against
   la_align_batch_min on windows gathered on the host (numpy; that gather time is reported beside it).  Device time =
   pack_ms + kernel_ms of la_timing, GCUPS over kernel time; the genome upload (la_genome_create) is timed on its own.
Prints one JSON line and writes DIR/result.json when --out is given.  Run it under `rocprofv3 --kernel-trace --stats` with
--skip-tool for the kernel table."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from defuse_amd import la  # noqa: E402

RC = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
    RC[a] = b
SEARCH, PRM = 500, (2, -1, -2)


def make_inputs(d, n_frags, mb, seed=1):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(50, 150, size=24).astype(np.float64)
    sizes = (sizes / sizes.sum() * mb * 1_000_000).astype(np.int64)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    contigs = []
    with open(os.path.join(d, "genome.fa"), "wb") as f:
        for k, n in enumerate(sizes):
            g = acgt[rng.integers(0, 4, size=int(n))]
            g[rng.random(int(n)) < 0.001] = ord("N")
            contigs.append(g)
            f.write(b">chr%d\n" % (k + 1))
            full = (len(g) // 60) * 60
            body = np.concatenate([g[:full].reshape(-1, 60), np.full((full // 60, 1), 10, dtype=np.uint8)], axis=1).tobytes()
            f.write(body + (g[full:].tobytes() + b"\n" if full < len(g) else b""))
    L = 100
    reads = [[], []]
    mates = [[], []]            # per end: (contig, strand, anchor) lists
    for end in (0, 1):
        ci = rng.integers(0, 24, size=n_frags)
        starts = np.array([rng.integers(0, len(contigs[c]) - L) for c in ci])
        seqs = np.empty((n_frags, L), dtype=np.uint8)
        for c in range(24):
            m = ci == c
            seqs[m] = contigs[c][starts[m][:, None] + np.arange(L)]
        flips = rng.random(seqs.shape) < 0.02
        seqs[flips] = acgt[rng.integers(0, 4, size=int(flips.sum()))]
        rev = rng.random(n_frags) < 0.5
        seqs[rev] = RC[seqs[rev][:, ::-1]]
        reads[end] = seqs
        nm = rng.integers(1, 5, size=n_frags)
        for k in range(n_frags):
            al = [(int(ci[k]), int(rev[k]), int(starts[k]) + 1 + (L - 1 if rev[k] else 0))]
            for _ in range(int(nm[k]) - 1):
                c = int(rng.integers(0, 24))
                al.append((c, int(rng.integers(0, 2)), int(rng.integers(1, len(contigs[c]) + 1))))
            mates[end].append(al)
    sam = ["@HD\tVN:1.0\n"]
    seq_txt = "A" * L
    for end in (0, 1):
        for k, al in enumerate(mates[end]):
            for c, strand, anchor in al:
                pos = anchor - (L - 1) if strand else anchor
                sam.append("%d/%d\t%d\tchr%d\t%d\t60\t100M\t*\t0\t0\t%s\t*\n" % (k, end + 1, 16 if strand else 0, c + 1, pos, seq_txt))
    with open(os.path.join(d, "aln.sam"), "w") as f:
        f.write("".join(sam))
    for end in (0, 1):
        with open(os.path.join(d, "reads%d.fastq" % (end + 1)), "wb") as f:
            qual = b"I" * L
            f.write(b"".join(b"@%d/%d\n%s\n+\n%s\n" % (k, end + 1, reads[end][k].tobytes(), qual) for k in range(n_frags)))
    return contigs, reads, mates


def windows_of(contigs, reads, mates):
    """Every (read, mate alignment) in the tool's output order: LA_WINDOW descriptors against the concatenated genome and the
    read pool (reads of file 1 then file 2, 100 bytes each)."""
    from tests import matealign_oracle as mo
    offs = np.cumsum([0] + [len(c) for c in contigs])
    n_frags = len(reads[0])
    out = []
    for read_end in (0, 1):
        other = mates[1 - read_end]
        for k in range(n_frags):
            for c, strand, anchor in other[k]:
                start, end = (anchor, anchor + SEARCH) if strand == 0 else (anchor - SEARCH, anchor)
                off, sl, pl, pr = mo.get_parts(len(contigs[c]), start, end)
                out.append((offs[c] + off, (read_end * n_frags + k) * 100, sl, pl, pr, 100, 1 - strand, 0))
    return np.array(out, dtype=la.LA_WINDOW)


def gather(genome, wins):
    """Host-built references of windows (what la_align_batch_min needs): numpy, chunked."""
    refs = []
    for w in wins:
        r = np.concatenate([np.full(w["pad_left"], 78, np.uint8), genome[w["slice_off"]:w["slice_off"] + w["slice_len"]],
                            np.full(w["pad_right"], 78, np.uint8)])
        refs.append(RC[r[::-1]] if w["revcomp"] else r)
    return refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1_000_000)
    ap.add_argument("--mb", type=int, default=200)
    ap.add_argument("--ab-pairs", type=int, default=400_000)
    ap.add_argument("--skip-tool", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"frags": a.frags, "genome_mb": a.mb, "search": SEARCH, "scoring": PRM}
    with tempfile.TemporaryDirectory() as d:
        t = time.time()
        contigs, reads, mates = make_inputs(d, a.frags, a.mb)
        res["make_inputs_s"] = round(time.time() - t, 1)
        wins = windows_of(contigs, reads, mates)
        res["pairs"] = len(wins)
        genome = np.concatenate(contigs)
        pool = np.concatenate([reads[0].reshape(-1), reads[1].reshape(-1)])
        if not a.skip_tool:
            cmd = [os.path.join(ROOT, "bin", "matealign"), "-m", "2", "-x", "-1", "-g", "-2", "-s", str(SEARCH), "-r",
                   os.path.join(d, "genome.fa"), "-1", os.path.join(d, "reads1.fastq"), "-2", os.path.join(d, "reads2.fastq")]
            t = time.time()
            with open(os.path.join(d, "aln.sam"), "rb") as sam:
                p = subprocess.run(cmd, stdin=sam, capture_output=True, env=dict(os.environ, DEFUSE_TIMING="1"), timeout=1200)
            res["tool_wall_s"] = round(time.time() - t, 2)
            res["tool_rc"] = p.returncode
            res["tool_stderr"] = p.stderr.decode()[-2000:]
            lines = p.stdout.decode().splitlines()
            res["tool_lines"] = len(lines)
            # the sample: 300 fixed pairs, checked against the oracle's window and score
            from oracle.localalign_oracle import simple_align, format_double
            rng = np.random.default_rng(99)
            sample = rng.choice(len(wins), size=min(300, len(wins)), replace=False)
            bad = 0
            for k in sample:
                w = wins[k]
                ref = gather(genome, [w])[0].tobytes()
                seq = pool[w["seq_off"]:w["seq_off"] + 100].tobytes()
                s = simple_align(*PRM, ref, seq)
                frag = (w["seq_off"] // 100) % a.frags
                want = "%d\t%d\t%s" % (frag, s, format_double(s / 200.0))
                bad += k >= len(lines) or lines[k] != want
            res["sample_checked"] = int(len(sample))
            res["sample_mismatches"] = int(bad)
            del lines
        # A/B on the same pairs
        lib = la.lib()
        ab = wins[:a.ab_pairs]
        t = time.time()
        gen = la.genome(genome.tobytes())
        res["genome_upload_s"] = round(time.time() - t, 3)          # includes the Python copy of 200 MB
        tw = la.LaTiming()
        scores_w = np.zeros(len(ab), np.int32)
        lib.la_align_windows_min(gen.handle, *PRM, pool.ctypes.data, len(pool), ab.ctypes.data, len(ab), None, scores_w.ctypes.data, ctypes.byref(tw))
        runs_w = []
        for _ in range(3):
            lib.la_align_windows_min(gen.handle, *PRM, pool.ctypes.data, len(pool), ab.ctypes.data, len(ab), None, scores_w.ctypes.data, ctypes.byref(tw))
            runs_w.append((tw.pack_ms, tw.kernel_ms, tw.total_ms))
        t = time.time()
        refs = gather(genome, ab)
        items = np.zeros(len(ab), dtype=la.LA_ITEM)
        lens = np.array([len(r) for r in refs], dtype=np.int64)
        items["ref_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
        items["ref_len"] = lens
        items["seq_off"] = lens.sum() + ab["seq_off"]
        items["seq_len"] = ab["seq_len"]
        bpool = np.concatenate(refs + [pool])
        res["host_gather_s"] = round(time.time() - t, 3)
        res["host_pool_bytes"] = int(len(bpool))
        res["window_pool_bytes"] = int(len(pool) + len(ab) * la.LA_WINDOW.itemsize)
        tb = la.LaTiming()
        scores_b = np.zeros(len(ab), np.int32)
        runs_b = []
        for _ in range(4):
            lib.la_align_batch_min(0, *PRM, bpool.ctypes.data, len(bpool), items.ctypes.data, len(ab), None, scores_b.ctypes.data, ctypes.byref(tb))
            runs_b.append((tb.pack_ms, tb.kernel_ms, tb.total_ms))
        runs_b = runs_b[1:]
        gen.close()
        res["ab_pairs"] = len(ab)
        res["ab_scores_equal"] = bool(np.array_equal(scores_w, scores_b))
        res["cells"] = int(tw.cells)
        for tag, runs in (("windows", runs_w), ("batch", runs_b)):
            pk = float(np.median([r[0] for r in runs]))
            kn = float(np.median([r[1] for r in runs]))
            res[tag] = {"pack_ms": round(pk, 3), "kernel_ms": round(kn, 3), "device_ms": round(pk + kn, 3),
                        "total_ms": round(float(np.median([r[2] for r in runs])), 1), "pack_share": round(pk / (pk + kn), 4),
                        "gcups_kernel": round(tw.cells / kn / 1e6, 1), "runs": [[round(x, 3) for x in r] for r in runs]}
        res["device_ratio_windows_over_batch"] = round(res["windows"]["device_ms"] / res["batch"]["device_ms"], 4)
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "result.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
