"""bench.py --dump-outputs and --steps: the records of the last timed step written as DIR/<field>.npy (float64, at most 64 MB,
a fixed sample of a larger output), and exactly the requested number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("fusion_id", "frag", "read_end", "revcomp", "ref_first", "ref_second", "read_first", "read_second", "score", "pair_idx")


def load_outputs(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in FIELDS + ("sample_index", "n_records")}


def test_dump_outputs_samples_a_large_output_within_the_cap(tmp_path):
    import torch
    import bench
    sizes = (400_000, 0, 350_000, 250_000)                 # more records than fit: a sample is written
    parts, base = [], 0
    for n in sizes:
        rows = (np.arange(base, base + n, dtype=np.int64)[:, None] * 16 + np.arange(10)).astype(np.int32)
        parts.append((n, (lambda r=rows: r) if len(parts) % 2 == 0 else (lambda r=rows: torch.from_numpy(r))))
        base += n
    info = bench.dump_outputs(str(tmp_path / "a"), parts)
    assert info["records"] == sum(sizes) and info["sampled"] and info["written"] < sum(sizes)
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 10 ** 6
    out = load_outputs(str(tmp_path / "a"))
    idx = out["sample_index"].astype(np.int64)
    assert out["n_records"].tolist() == [sum(sizes)] and len(idx) == info["written"] and np.all(np.diff(idx) > 0)
    for k, n in enumerate(FIELDS):
        assert out[n].dtype == np.float64 and np.array_equal(out[n], (idx * 16 + k).astype(np.float64)), n
    bench.dump_outputs(str(tmp_path / "b"), parts)          # the same sample every time
    again = load_outputs(str(tmp_path / "b"))
    assert all(np.array_equal(out[n], again[n]) for n in out)


def test_dump_outputs_writes_a_small_output_whole(tmp_path):
    import bench
    rows = np.arange(70, dtype=np.int32).reshape(7, 10)
    info = bench.dump_outputs(str(tmp_path), [(7, lambda: rows)])
    assert info == {"dir": str(tmp_path), "records": 7, "written": 7, "sampled": False, "seed": bench.DUMP_SEED}
    out = load_outputs(str(tmp_path))
    assert np.array_equal(np.stack([out[n] for n in FIELDS], axis=1), rows.astype(np.float64))


@pytest.mark.gpu
def test_bench_runs_the_requested_steps_and_dumps_the_oracle_records(built, tmp_path):
    """N = 1: --steps 2 times two steps; the dumped records of the last one are the CPU oracle's on the same synthetic batch,
    and a second run with the same arguments dumps the same arrays."""
    from oracle import dosplitalign_oracle as ora
    from defuse_amd import synth
    F, P = 300, 100
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--fusions", str(F), "--reads", str(P),
                            "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-sensitivity",
                            "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == line["steps_requested"] == 2 and line["ms_per_step"] > 0
    a, b = load_outputs(str(tmp_path / "a")), load_outputs(str(tmp_path / "b"))
    assert all(a[n].tobytes() == b[n].tobytes() for n in a)
    ref, fus, reads, pairs = synth.make_batch(F, P, lq=76, lr=389, seed=2)      # bench.py's batch at these sizes
    exp = ora.align_batch(ref, fus, reads, pairs)
    assert lines[0]["dump_outputs"]["records"] == len(exp) and not lines[0]["dump_outputs"]["sampled"]
    for n in FIELDS:
        assert np.array_equal(a[n], exp[n].astype(np.float64)), n
