"""numpy restatement of get_basic_statistics (TS/statistics.py:76-141) and of the table of boa_label_basic_stats, from their definitions.
Pinned against the reference's own function by tests/test_basic_statistics_reference_cpu.py (golden G17)."""
import numpy as np

BORDER = 3


def touches_border(mask, border=BORDER):
    """any voxel of `mask` in the first or last `border` indices of an axis (numpy slices: dims shorter than the slabs are all border)"""
    for ax in range(3):
        m = np.moveaxis(mask, ax, 0)
        if m[:border].any() or m[-border:].any():
            return True
    return False


def basic_statistics(seg, ct, zooms, class_map, exclude_masks_at_border=True, roi_subset=None, metric="mean", normalized_intensities=False):
    """{name: {"volume", "intensity"}} in the class map's order; `ct` is what get_fdata() returns (any real dtype), `zooms` the header's
    float32 zooms"""
    hu = np.asarray(ct).astype(np.int16)
    z = [np.float32(v) for v in zooms]
    vox_vol = z[0] * z[1] * z[2]
    if normalized_intensities:
        hu = (hu - hu.min()) / (hu.max() - hu.min())
    out = {}
    for idx, name in class_map.items():
        if roi_subset is not None and name not in roi_subset:
            continue
        sel = seg == idx
        n = sel.sum()
        if exclude_masks_at_border and touches_border(sel):
            out[name] = {"volume": 0.0, "intensity": 0.0}
            continue
        if n == 0:
            val = 0.0
        elif metric == "mean":
            val = np.average(hu, weights=sel.astype(np.uint8)).round(5)
        else:
            val = np.median(hu[sel]).round(5)
        out[name] = {"volume": n * vox_vol, "intensity": val}
    return out


def stats_table(seg, ct, border=BORDER):
    """the BOA_LABEL_STATS_WORDS words of boa_label_basic_stats as a uint64 array: count, sum (int64 bits), touches (0 / 1) per label
    value, then min and max of `ct` (int64 bits)"""
    seg = np.asarray(seg)
    hu = np.asarray(ct).astype(np.int64)
    cnt = np.bincount(seg.ravel(), minlength=256).astype(np.uint64)
    # hu = 65536 hi + lo: both weighted bincounts are sums of integers below 2^53 in float64, hence exact (np.add.at is slow at 10^7 voxels)
    assert hu.size < 2 ** 31 and (hu.size == 0 or (hu.min() >= -2 ** 31 and hu.max() < 2 ** 31))
    hi, lo = hu.ravel() >> 16, hu.ravel() & 0xFFFF
    sums = (np.bincount(seg.ravel(), weights=hi, minlength=256).astype(np.int64) * 65536
            + np.bincount(seg.ravel(), weights=lo, minlength=256).astype(np.int64))
    edge = np.zeros(seg.shape, bool)
    for ax, d in enumerate(seg.shape):
        i = np.arange(d)
        sh = [1, 1, 1]
        sh[ax] = d
        edge |= ((i < border) | (i >= d - border)).reshape(sh)
    touch = np.zeros(256, np.uint64)
    touch[np.unique(seg[edge])] = 1
    if hu.size:
        mm = np.array([hu.min(), hu.max()], np.int64)
    else:
        mm = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min], np.int64)
    return np.concatenate([cnt, sums.view(np.uint64), touch, mm.view(np.uint64)])
