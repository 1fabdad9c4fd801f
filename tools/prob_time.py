#!/usr/bin/env python3
"""Device time of boa_logits_to_probabilities at C = 25 on a 256^3 grid (identity perm, no resampling, the box is the grid, labels
written), and of boa_finalize_labels on the same grid -- the pass with the same read traffic -- for comparison.  Device events around
`--reps` back-to-back calls, median of `--rounds` such brackets after a warm-up.  Algorithmic bytes: probabilities 2 C V read +
4 C V + V written; finalize 2 C V + 2 V read + V written.  Development aid; `--only prob` / `--only finalize` time one
of the two."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd")]
import numpy as np  # noqa: E402
from boa_hip._lib import check, int3  # noqa: E402
from boa_hip.device import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--classes", type=int, default=25)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--only", choices=("prob", "finalize"), default=None)
args = ap.parse_args()
Cn, V = args.classes, [args.size] * 3
n = args.size ** 3
ctx = Context(0)
print("device:", ctx.info()["name"], flush=True)
# one plane of noise, rolled per class (logits of a few units, like a trained net's; every class plane is distinct)
plane = (np.random.default_rng(0).standard_normal(n, dtype=np.float32) * 4).astype(np.float16).view(np.uint16)
d_lg = ctx.alloc(Cn * n * 2)
for c in range(Cn):
    check(ctx.lib.boa_h2d(ctx.h, C.c_void_p(d_lg.ptr + c * n * 2), np.roll(plane, 977 * c).ctypes.data_as(C.c_void_p), n * 2), "boa_h2d")
d_lab = ctx.alloc(n)


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
    print(f"{name:28s} C {Cn} grid {args.size}^3: {m:7.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})  "
          f"{nbytes / m / 1e9:6.3f} TB/s algorithmic = {nbytes / m / 1e9 / 8:.3f} of 8 TB/s", flush=True)


if args.only != "finalize":
    d_prob = ctx.alloc(Cn * n * 4)
    timed("boa_logits_to_probabilities",
          lambda: check(ctx.lib.boa_logits_to_probabilities(ctx.h, d_lg.vp, Cn, int3(V), None, None, None, -1, int3((0, 0, 0)), int3(V),
                                                            int3((0, 1, 2)), d_prob.vp, None, d_lab.vp), "boa_logits_to_probabilities"),
          2.0 * Cn * n + 4.0 * Cn * n + n)
    d_prob.free()
if args.only != "prob":
    d_n = ctx.from_numpy(np.full(n, 0x3C00, np.uint16))      # fp16 1.0: the logits stay what they are
    flag = ctx.zeros(4)
    fin = ctx.lib.boa_finalize_labels
    timed("boa_finalize_labels",
          lambda: check(fin(ctx.h, d_lg.vp, d_n.vp, Cn, int3(V), None, 0, 0, 0, None, 0, d_lab.vp, None, None, flag.vp), "boa_finalize_labels"),
          2.0 * Cn * n + 2.0 * n + n)
ctx.close()
