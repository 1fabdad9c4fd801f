"""CPU: bench.py's launch contract.  `--gpus N` must never report N GPUs unless N ranks are running: outside a launcher it
starts the ranks itself (torch.distributed.run on 127.0.0.1), inside one it refuses when WORLD_SIZE != N."""
import os
import subprocess
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2, r.stderr
    assert "WORLD_SIZE=1" in r.stderr and r.stdout.strip() == ""       # no JSON line for GPUs that are not running


def test_self_launch_starts_one_rank_per_gpu():
    sys.path.insert(0, ROOT)
    import bench
    with mock.patch.object(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "2", "--warmup", "1"]):
        args = bench.parse_args()
        with mock.patch.object(bench.subprocess, "call", return_value=0) as call:
            assert bench.self_launch(args) == 0
    cmd = call.call_args[0][0]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "8", "--steps", "2", "--warmup", "1"]
    assert call.call_args[1]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_plain_run_is_lean_and_full_is_opt_in():
    sys.path.insert(0, ROOT)
    import bench
    with mock.patch.object(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"]):
        args = bench.parse_args()
    assert args.full is False and args.dump_outputs is None and args.steps == 3 and args.warmup == 2
    with mock.patch.object(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"]):
        args = bench.parse_args()
    assert args.full is True and args.dump_outputs == "out"
    with mock.patch.object(sys, "argv", ["bench.py", "--steps", "0"]), mock.patch.object(sys, "stderr"):
        try:
            bench.parse_args()
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError("--steps 0 accepted")


def test_dump_outputs_is_a_fixed_bounded_sample(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(3)
    big = rng.integers(0, 118, size=(160, 160, 128), dtype=np.uint8)          # 3.3 M voxels: sampled
    small = rng.integers(0, 7, size=(20, 30, 40), dtype=np.uint8)              # whole volume
    tables = {"total_measurements": {"b": {"present": True, "mean": 1.5, "name": "x"}, "a": [1, None, 2.0],
                                     "c": [float("nan"), float("inf"), -float("inf")]},
              "vertebrae": {}}
    a = bench.dump_outputs(str(tmp_path / "a"), {"total": big, "body_parts": small}, tables)
    b = bench.dump_outputs(str(tmp_path / "b"), {"total": big.copy(), "body_parts": small.copy()}, dict(tables))
    assert a == b and sum(a.values()) <= bench.DUMP_MAX_BYTES
    assert sorted(a) == ["body_parts.npy", "body_parts_counts.npy", "total.npy", "total_counts.npy", "total_measurements.npy",
                         "total_measurements_nonfinite.npy", "vertebrae.npy", "vertebrae_nonfinite.npy"]
    for name in a:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), name
        np.testing.assert_array_equal(x, y)
    t = np.load(tmp_path / "a" / "total.npy")
    assert t.dtype == np.float32 and t.size == bench.DUMP_VOXELS
    assert set(np.unique(t)) <= set(np.unique(big).astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "body_parts.npy"), small.reshape(-1).astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "total_counts.npy")[:118], np.bincount(big.reshape(-1), minlength=118))
    # numeric leaves, keys sorted: a = [1, None, 2.0], b = {mean, name (dropped), present}, c = [nan, inf, -inf]; the values are
    # finite (0 in place of None / NaN / inf), the kinds say which was which
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "total_measurements.npy"), [1.0, 0.0, 2.0, 1.5, 1.0, 0.0, 0.0, 0.0])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "total_measurements_nonfinite.npy"), [0, 4, 0, 0, 0, 1, 2, 3])
    assert np.load(tmp_path / "a" / "vertebrae.npy").size == 0
