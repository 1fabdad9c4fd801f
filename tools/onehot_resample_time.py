#!/usr/bin/env python3
"""Device time of boa_resample_onehot_u8 (`higher_order_resampling`) next to boa_resample_nearest_u8 -- the pass it replaces -- on a
`--size`^3 output (default 512) from a 1.5 mm model grid holding a synthetic 117-label volume.  Cases: the 3-D form at factor 2
(0.75 mm input grid) and at a non-dyadic factor, the separate-z form without and with a change of extent along the coarse axis, and
white-noise labels (8 distinct labels in almost every cell: nothing takes the one-label shortcut).  Device events around `--reps`
back-to-back calls, median of `--rounds` brackets after a warm-up; the one-hot call builds its per-axis table in a small kernel of
its own, which is inside its figure.  Algorithmic bytes: the output written once + the source read once.
Development aid."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd")]
import numpy as np  # noqa: E402
from boa_hip._lib import check, int3  # noqa: E402
from boa_hip.device import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
N = args.size
out = (N, N, N)
ctx = Context(0)
print("device:", ctx.info()["name"], flush=True)


def organs(shape, seed=0, block=16, specks=0.02):
    """117 labels + background in blocks of `block` voxels with 2 % single-voxel specks: mostly one label per cell, boundaries everywhere"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 118, size=tuple(-(-s // block) for s in shape)).astype(np.uint8)
    a = np.kron(coarse, np.ones((block,) * 3, dtype=np.uint8))[:shape[0], :shape[1], :shape[2]]
    if specks:
        speck = rng.random(shape) < specks
        a[speck] = rng.integers(0, 118, size=int(speck.sum()))
    return np.ascontiguousarray(a)


def timed(name, fn, nbytes):
    for _ in range(2):
        fn()
    ctx.sync()
    ms = []
    for _ in range(args.rounds):
        ctx.timer_start(0)
        for _ in range(args.reps):
            fn()
        ms.append(ctx.timer_stop(0) / args.reps)
    m = float(np.median(ms))
    print(f"  {name:26s} {m:8.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})  {nbytes / m / 1e9:6.3f} TB/s algorithmic", flush=True)
    return m


h, t = N // 2, max(1, N // 3)
cases = [("3-D x2", (h, h, h), -1, organs), ("3-D x2, blocks without specks", (h, h, h), -1, lambda s: organs(s, specks=0)),
("3-D non-dyadic", (int(N / 2.1), int(N / 2.1), int(N / 2.55)), -1, organs),
         ("separate z, same extent", (h, h, N), 2, organs), ("separate z, extent x3", (h, h, t), 2, organs),
         ("3-D x2, white noise", (h, h, h), -1, lambda s: np.random.default_rng(1).integers(0, 118, size=s).astype(np.uint8))]
d_out = ctx.alloc(N ** 3)
for name, shp, sep, make in cases:
    d_in = ctx.from_numpy(make(shp))
    nbytes = float(N) ** 3 + float(np.prod(shp))
    print(f"{name}: {shp} -> {out}, sep_axis {sep}", flush=True)
    near = timed("boa_resample_nearest_u8", lambda: check(ctx.lib.boa_resample_nearest_u8(ctx.h, d_in.vp, int3(shp), d_out.vp, int3(out)),
                                                          "boa_resample_nearest_u8"), nbytes)
    one = timed("boa_resample_onehot_u8", lambda: check(ctx.lib.boa_resample_onehot_u8(ctx.h, d_in.vp, int3(shp), d_out.vp, int3(out), sep),
                                                        "boa_resample_onehot_u8"), nbytes)
    print(f"  one-hot / nearest = {one / near:.2f}", flush=True)
    d_in.free()
ctx.close()
