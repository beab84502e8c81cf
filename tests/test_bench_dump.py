"""CPU: `bench.py --dump-outputs DIR` — the arrays land as DIR/<name>.npy in float32 / float64, a run over the byte budget
keeps a fixed, seeded sample of rows (same rows every run), and the dry run of the plumbing writes the metric sums its
timed steps computed (the same numbers as its JSON line)."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_dtypes_and_budget(tmp_path):
    import bench
    y = torch.arange(64 * 2 * 100, dtype=torch.float32).reshape(64, 2, 100)
    s = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "all"), {"separated": y, "metric_sums": s, "half": y[:2].half()})
    got = {f: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["half.npy", "metric_sums.npy", "separated.npy"]
    assert got["separated.npy"].dtype == np.float32 and np.array_equal(got["separated.npy"], y.numpy())
    assert got["metric_sums.npy"].dtype == np.float64 and np.array_equal(got["metric_sums.npy"], s.numpy())
    assert got["half.npy"].dtype == np.float32
    # 20 KB limit: `separated` (51 KB) is cut to a seeded sample of its rows, the small array stays whole
    limit = 20000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"separated": y, "metric_sums": s}, limit=limit)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["metric_sums.npy", "separated.npy", "separated_rows.npy"]
    assert sum(v.nbytes for v in a.values()) <= limit
    rows = a["separated_rows.npy"].astype(np.int64)
    assert len(rows) > 1 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["separated.npy"], y.numpy()[rows])
    for k in a:
        assert np.array_equal(a[k], b[k])


def test_dry_run_dumps_its_metric_sums(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dry-run-cpu", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    sums = np.load(tmp_path / "metric_sums.npy")
    assert sums.dtype == np.float64 and sums.tolist() == line["metric_sums"]
