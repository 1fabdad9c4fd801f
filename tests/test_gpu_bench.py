"""GPU: a plain `bench.py` run times the steps it is asked for and nothing else, and `--dump-outputs` writes the last timed
step's labels and tables, identical from run to run (same seeded phantom, same seeded weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_and_output_dump(tmp_path):
    def run(out):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "128", "--steps", "2", "--warmup", "1",
               "--dump-outputs", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    a, b = run(tmp_path / "a"), run(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "volumes/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f16" and line["value"] > 0
        assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-6
        assert line["kernel_variants"]["conv_ws"] > 0 and line["roofline"]["achieved"] > 0
        # the extras that take runs of their own wait for --full
        for k in ("cpu_baseline", "no_event_profiling", "two_lanes", "phantom_stages", "host_to_host", "total_only", "parity"):
            assert line.get(k) is None, k
        assert line["roofline"]["attainable"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for v in ("total", "body_parts", "body_regions", "tissues"):
        assert f"{v}.npy" in names and f"{v}_counts.npy" in names
    for t in ("total_measurements", "bca_measurements"):
        assert f"{t}.npy" in names and f"{t}_nonfinite.npy" in names
    size = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
        size += x.nbytes
    assert size <= 64 << 20
    # 128^3 voxels = the sample size: the whole `total` volume is in the dump, and its counts cover every voxel
    total = np.load(tmp_path / "a" / "total.npy")
    counts = np.load(tmp_path / "a" / "total_counts.npy")
    assert total.size == 128 ** 3 and counts.sum() == 128 ** 3
    np.testing.assert_array_equal(np.bincount(total.astype(np.int64), minlength=counts.size), counts)
