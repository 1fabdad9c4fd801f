#!/usr/bin/env python3
"""Time of the blob post-processing (remove_small_blobs of every label: boa_label_blobs6 + boa_label_blobs_filter,
csrc/ccl_labels.hip) on label volumes of size^3 (default 512, the bench's size): (a) the 117-label structured phantom of
boa_hip/synthetic.py, (b) noise-like labels (argmax of smooth random fields: what the argmax of a random-weight net looks like, the
worst case -- millions of blobs).  Next to it the reference's host loop on the same arrays on the same machine: scipy.ndimage.label
label by label as TS/postprocessing.py:77-98 does (`--no-host` skips it: minutes at 512^3).  Prints ms per call (median of `reps`
synchronised calls; the device labels are re-uploaded outside the timed region) and checks that both give the same volume.
A development aid: nothing here is asserted about speed.

    python tools/blobs_time.py [size] [reps] [--no-host]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd")]
import numpy as np  # noqa: E402
from boa_hip import blobs, label_maps, synthetic  # noqa: E402
from boa_hip.devarray import DevArray  # noqa: E402
from boa_hip.device import Context  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
size = int(args[0]) if len(args) > 0 else 512
reps = int(args[1]) if len(args) > 1 else 5
host = "--no-host" not in sys.argv
shape = (size, size, size)
ctx = Context(0)
rng = np.random.default_rng(0)
CM = label_maps.CLASS_MAP_TOTAL
LO, HI = blobs.interval_bounds([blobs.size_threshold_voxels(200, (1.5, 1.5, 1.5)), 1e10])     # 59 voxels at 1.5 mm


def smooth_noise_labels(n_classes):
    from scipy import ndimage
    best = np.full(shape, -1e9, np.float32)
    lab = np.zeros(shape, np.uint8)
    for c in range(n_classes):
        f = ndimage.uniform_filter(rng.standard_normal(shape).astype(np.float32), 3)
        m = f > best
        lab[m] = c
        best = np.maximum(best, f)
    return lab


def host_loop(data):
    """remove_small_blobs_multilabel as the reference runs it: one scipy labelling per label of the class map"""
    from scipy import ndimage
    data = data.copy()
    for idx in CM:
        roi = data == idx
        mask, n = ndimage.label(roi)
        counts = np.bincount(mask.ravel())
        if len(counts) <= 1:
            continue
        remove = (counts <= LO) | (counts > 1e10)
        keep = roi & ~remove[mask]
        data[roi] = 0
        data[keep] = idx
    return data


cases = {"phantom total (117 labels)": synthetic.label_phantom_total(shape), "noise (12 labels)": smooth_noise_labels(13)}
modes = blobs.modes_for(CM, list(CM.values()), blobs.MODE_INTERVAL)
for name, seg in cases.items():
    seg = np.ascontiguousarray(seg)
    t_label, t_filter, got, ncomp = [], [], None, 0
    for _ in range(reps + 1):
        d = DevArray.from_numpy(ctx, seg)
        ctx.sync()
        t0 = time.perf_counter()
        lab = blobs.BlobLabelling(ctx, d)
        ctx.sync()
        t1 = time.perf_counter()
        lab.filter(modes, LO, HI)
        ctx.sync()
        t2 = time.perf_counter()
        t_label.append((t1 - t0) * 1e3)
        t_filter.append((t2 - t1) * 1e3)
        lab.free()
        if _ == reps:
            got = d.download()
            chk = DevArray.from_numpy(ctx, seg)
            lc = blobs.BlobLabelling(ctx, chk, count=True)
            ncomp = lc.n_components
            lc.free()
            chk.free()
        d.free()
    line = (f"{name:28s} {size}^3  {ncomp:9d} blobs  label {np.median(t_label[1:]):7.2f} ms  filter {np.median(t_filter[1:]):6.2f} ms"
            f"  removed {int((got != seg).sum())} voxels")
    if host:
        t0 = time.perf_counter()
        want = host_loop(seg)
        line += f"  | host scipy loop {(time.perf_counter() - t0):7.1f} s  same volume: {bool(np.array_equal(got, want))}"
    print(line, flush=True)
ctx.close()
