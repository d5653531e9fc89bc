"""A generated alignment file for evalsplitalign (test infrastructure; profiles/microbench/eval_profile.py times the tool on it)."""
import numpy as np

from tests import pipeline_case


def generated_case(tmp_path, lines_per_fusion, n_fusions=200, seed=21):
    """Regions and tasks from pipeline_case, and an alignment file written from the tasks' own window lengths: per fusion
    lines_per_fusion lines on a handful of splits inside the windows (so the DebugChecks hold), reads of 50 bases."""
    from oracle import dosplitalign_oracle as ora
    case = pipeline_case.build(str(tmp_path / "case"), seed=seed, n_fusions=n_fusions, reads_per_fusion=1, chrom_len=20000)
    tasks = ora.create_tasks(case["fasta"], case["exons"], case["ufrag"], case["sfrag"], case["minread"], case["maxread"],
                             ora.read_align_region_pairs(case["regions"]))
    rng = np.random.default_rng(seed)
    out = []
    for fid in sorted(tasks):
        t = tasks[fid]
        l0, l1 = len(t.seq[0]), len(t.seq[1])
        if l0 < 8 or l1 < 8:
            continue
        firsts = rng.integers(1, l0 + 1, 6)
        seconds = rng.integers(-1, l1 - 2, 3)
        m = lines_per_fusion
        a = rng.integers(0, 51, m)
        cols = np.stack([np.full(m, fid), rng.integers(0, 10 ** 6, m), rng.integers(0, 2, m), rng.integers(0, 2, m), rng.choice(firsts, m),
                         rng.choice(seconds, m), a, 50 - a, rng.integers(8, 101, m)], axis=1)
        out.extend("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t\n" % tuple(row) for row in cols.tolist())
    return case, out
