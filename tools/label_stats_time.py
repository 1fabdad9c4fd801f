#!/usr/bin/env python3
"""Time of the per-label statistics pass (boa_label_basic_stats, csrc/label_stats.hip) on size^3 volumes (default 512, the bench's
size): (a) the 117-label structured phantom of boa_hip/synthetic.py, (b) per-voxel uniform random labels 0..255 (the worst case: 64
distinct labels in every wave), for an int16 and an int32 CT.  Device time: device events around `reps` back-to-back calls (table init
+ kernel each), after a warm-up call; GB/s = the algorithm's 3 B (int16) or 5 B (int32) per voxel over that time.  Next to it the
numpy statements of get_basic_statistics (TS/statistics.py:119-130: `seg == k`, touches_border, `data.sum()`, np.average) on the same
arrays on the host, timed on the first `--host-labels` structures of the class map (default 4; the reference runs all 117, one after
the other: its cost is that per-structure time x 117) and the check that both give the same counts, sums and flags.
A development aid: nothing here is asserted about speed.

    python tools/label_stats_time.py [size] [reps] [--host-labels K]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd")]
import numpy as np  # noqa: E402
from boa_hip import synthetic  # noqa: E402
from boa_hip._lib import check, int3  # noqa: E402
from boa_hip.device import Context  # noqa: E402

argv = sys.argv[1:]
host_labels = 4
if "--host-labels" in argv:
    i = argv.index("--host-labels")
    host_labels = int(argv[i + 1])
    del argv[i:i + 2]
size = int(argv[0]) if len(argv) > 0 else 512
reps = int(argv[1]) if len(argv) > 1 else 200
shape = (size, size, size)
HBM_PEAK = 8.0e12            # bytes / s
ctx = Context(0)
rng = np.random.default_rng(0)


def host_structure(seg, ct, k):
    """(count, sum, touches, mean) of structure k with the reference's numpy statements"""
    data = seg == k
    touches = bool(np.any(data[:3]) or np.any(data[-3:]) or np.any(data[:, :3]) or np.any(data[:, -3:])
                   or np.any(data[:, :, :3]) or np.any(data[:, :, -3:]))
    n = int(data.sum())
    roi = (data > 0).astype(np.uint8)
    mean = float(np.average(ct, weights=roi)) if n else 0.0
    return n, touches, mean


ct16 = synthetic.ct_phantom(shape)
cases = {"phantom total (117 labels)": synthetic.label_phantom_total(shape),
         "random labels 0..255": rng.integers(0, 256, size=shape, dtype=np.uint8)}
out = ctx.alloc(770 * 8)
for name, seg in cases.items():
    seg = np.ascontiguousarray(seg)
    d_seg = ctx.from_numpy(seg)
    for code, ct in ((1, ct16), (2, ct16.astype(np.int32))):
        d_ct = ctx.from_numpy(ct)
        call = lambda: check(ctx.lib.boa_label_basic_stats(ctx.h, d_ct.vp, code, d_seg.vp, int3(shape), 3, out.vp), "boa_label_basic_stats")
        call()
        ctx.sync()
        ctx.timer_start(0)
        for _ in range(reps):
            call()
        ms = ctx.timer_stop(0) / reps
        nbytes = seg.size * (3 if code == 1 else 5)
        t = out.download((770,), np.uint64)
        print(f"{name:28s} {size}^3  CT int{16 * code}:  {ms * 1e3:8.1f} us per call ({reps} calls)  {nbytes / ms / 1e6:7.1f} GB/s"
              f" = {nbytes / (ms * 1e-3) / HBM_PEAK:5.3f} of 8 TB/s", flush=True)
        d_ct.free()
    if host_labels > 0:
        ks = list(range(1, host_labels + 1))
        t0 = time.perf_counter()
        ref = [host_structure(seg, ct16, k) for k in ks]
        per = (time.perf_counter() - t0) / len(ks)
        same = all(int(t[k]) == n and bool(t[512 + k]) == tch and (n == 0 or float(np.int64(t[256 + k].view(np.int64))) / n == m)
                   for k, (n, tch, m) in zip(ks, ref))
        print(f"{'':28s} host numpy, same arrays: {per:6.2f} s per structure (measured on {len(ks)}; the reference runs 117 = "
              f"{per * 117:6.1f} s at this rate, not run)  same count / flag / mean: {same}", flush=True)
    d_seg.free()
out.free()
ctx.close()
