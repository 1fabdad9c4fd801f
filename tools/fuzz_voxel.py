#!/usr/bin/env python3
"""Randomised differential test of the voxel kernels against scipy / numpy / the oracle on random shapes (1 ... 70 per axis,
odd, prime, non-multiples of every vector width): cubic + nearest resampling (bit-exact vs scipy.ndimage.zoom), erosion,
slice-wise hole filling, in-plane median, region / part post-processing (CCL), tissue aggregation, per-label HU histogram,
tissue projections.  Exit code 1 on any mismatch."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "body-and-organ-analysis_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import voxel_stats_reference as VR  # noqa: E402  (plain numpy statements of the voxel statistics)
from scipy import ndimage  # noqa: E402
from boa_hip import bca, resample  # noqa: E402
from boa_hip import measurements as M  # noqa: E402
from boa_hip._lib import check  # noqa: E402
from boa_hip.device import Context  # noqa: E402
from oracle import bca as obca  # noqa: E402
from oracle import measurements as OM  # noqa: E402

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
ctx = Context(0)
fails = []


def rshape(lo=1, hi=70):
    return tuple(int(v) for v in rng.integers(lo, hi + 1, size=3))


def expect(name, shape, ok, extra=""):
    if not ok:
        fails.append((name, shape, extra))
        print(f"MISMATCH {name} shape={shape} {extra}", flush=True)


for i in range(n_cases):
    # ---- resampling -------------------------------------------------------------------------------------
    sh = rshape(2, 48)
    zoom = tuple(float(v) for v in rng.uniform(0.3, 2.2, size=3))
    x = (rng.normal(size=sh) * 500).astype(rng.choice([np.int16, np.float32, np.float64]))
    if all(int(round(s * z)) >= 1 for s, z in zip(sh, zoom)):
        ref = ndimage.zoom(x.astype(np.float64), zoom, order=3, mode="nearest")
        out = resample.resample_img(ctx, x, zoom, 3)
        expect("cubic", sh, out.shape == ref.shape and np.array_equal(out.view(np.uint64), ref.view(np.uint64)), f"zoom={zoom}")
        lab = rng.integers(0, 120, size=sh, dtype=np.uint8)
        ref0 = ndimage.zoom(lab, zoom, order=0, mode="nearest")
        out0 = resample.resample_img(ctx, lab, zoom, 0)
        expect("nearest", sh, np.array_equal(out0, ref0), f"zoom={zoom}")
    # ---- erosion ----------------------------------------------------------------------------------------
    sh = rshape(1, 40)
    m = rng.random(sh) < rng.choice([0.9, 0.98, 1.0])
    expect("erode6", sh, np.array_equal(M.erode_region(ctx, m), OM.erode_region(m)))
    # ---- fill holes / median ----------------------------------------------------------------------------
    sh = rshape(1, 60)
    m = ndimage.binary_dilation(rng.random(sh) < 0.03, iterations=2) & (rng.random(sh) < 0.9)
    n = m.size
    d_m = ctx.from_numpy(m.astype(np.uint8))
    d_i, d_t, d_o = ctx.alloc(n * 4), ctx.alloc(n), ctx.alloc(n)
    check(ctx.lib.boa_fill_holes_2d(ctx.h, d_m.vp, sh[0], sh[1], sh[2], d_i.vp, d_t.vp, d_o.vp))
    out = d_o.download(sh, np.uint8).astype(bool)
    ref = np.stack([ndimage.binary_fill_holes(m[k]) for k in range(sh[0])])
    expect("fill_holes", sh, np.array_equal(out, ref))
    for b in (d_m, d_i, d_t, d_o):
        b.free()
    ct = rng.integers(-1024, 3071, size=sh).astype(np.int16)
    d = ctx.from_numpy(ct)
    ax = int(rng.integers(0, 3))
    o = bca.median_filter_inplane(ctx, d, sh, ax)
    size = [3, 3, 3]
    size[ax] = 1
    expect("median3", sh, np.array_equal(o.download(sh, np.int16), ndimage.median_filter(ct, size=size)), f"axis={ax}")
    d.free()
    o.free()
    # ---- CCL-based post-processing ----------------------------------------------------------------------
    sh = rshape(2, 36)
    seg = np.zeros(sh, np.uint8)
    for _ in range(int(rng.integers(2, 9))):
        c = [int(rng.integers(0, s)) for s in sh]
        r = int(rng.integers(1, 7))
        sl = tuple(slice(max(0, cc - r), cc + r + 1) for cc in c)
        seg[sl] = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 9, 10, 11]))
    seg[(rng.random(sh) < 0.003) & (seg == 0)] = int(rng.choice([3, 6, 7]))
    expect("region_post", sh, np.array_equal(bca.postprocess_region_segmentation(ctx, seg), obca.postprocess_region_segmentation(seg)))
    parts = (seg % 7).astype(np.uint8)
    thr = int(rng.choice([5, 30, 200]))
    expect("part_post", sh, np.array_equal(bca.postprocess_part_segmentation(ctx, parts, thr),
                                           obca.remove_small_labeled_objects(parts, threshold=thr)), f"thr={thr}")
    # ---- aggregation ------------------------------------------------------------------------------------
    sh = rshape(1, 50)
    ct = rng.integers(-1100, 3200, size=sh).astype(np.int16)
    lab = rng.integers(0, 118, size=sh, dtype=np.uint8)
    d_ct, d_lab = ctx.from_numpy(ct), ctx.from_numpy(lab)
    hist = M.label_hu_histogram(ctx, d_ct, d_lab, ct.size)
    cnt = np.bincount(lab.ravel(), minlength=256)
    cnt[0] = 0
    sums = np.bincount(lab.ravel(), weights=ct.ravel().astype(np.float64), minlength=256)
    hu = np.arange(hist.shape[1], dtype=np.int64) + M.HU_MIN
    expect("hist", sh, np.array_equal(hist.sum(axis=1), cnt) and
           np.array_equal((hist.astype(np.int64) * hu[None]).sum(axis=1)[1:], sums[1:].astype(np.int64)))
    expect("hist_bins", sh, np.array_equal(hist, VR.label_hu_histogram(ct, lab, None, M.HU_MIN, M.NBINS)))     # every bin
    regions = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 255], dtype=np.uint8), size=sh)
    d_reg = ctx.from_numpy(regions)
    tis, c2, h2 = bca.tissue_aggregate(ctx, d_ct, d_reg, None, sh)
    t = tis.download(sh, np.uint8)
    want_t = obca.subclassify_tissues(ct, regions) if hasattr(obca, "subclassify_tissues") else None
    if want_t is not None:
        expect("tissues", sh, np.array_equal(t, want_t))
    expect("tissue_counts", sh, np.array_equal(c2[:, 0, 1:].sum(axis=0).astype(np.int64), np.bincount(t.ravel(), minlength=8)[1:8]))
    vals = [v for _, v in bca.TISSUES]
    cor, sag, mc, ms = bca.tissue_projections(ctx, tis, d_reg, sh, vals)
    body = (regions > 0) & (regions < 255)
    okp = np.array_equal(mc, body.any(axis=1)) and np.array_equal(ms, body.any(axis=2))
    for k, v in enumerate(vals):
        okp = okp and np.array_equal(cor[k], (t == v).sum(axis=1)) and np.array_equal(sag[k], (t == v).sum(axis=2))
    expect("projections", sh, okp)
    for b in (d_ct, d_lab, d_reg, tis):
        b.free()
print(f"{n_cases} rounds, {len(fails)} mismatches", [f[0] for f in fails][:10])
ctx.close()
sys.exit(1 if fails else 0)
