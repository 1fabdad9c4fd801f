"""`statistics.json` of TotalSegmentator (get_basic_statistics, TS/statistics.py:76-141; TS/python_api.py:636-641,778-796) on resident data.

The reference makes, per structure of the class map, three full-volume numpy passes (`seg == k`, touches_border, np.average or
np.median): 117 x 3 for `total`.  Here ONE device pass (`boa_label_basic_stats`, csrc/label_stats.hip) gives the voxel count, the
integer HU sum and the touches-border flag of every label value plus the CT's min and max; the table is downloaded once and the dict
follows on the host in the reference's float arithmetic:

    vox_vol    float32 product (z0 * z1) * z2 of the header's float32 zooms
    volume     count * vox_vol in float64 (int64 scalar times float32 scalar); 0.0 for a touching label when they are excluded
    mean       float64(sum) / float64(count), .round(5): np.average of int16 values with 0 / 1 weights is exact (|sum| < 2^53)
    median     from the label's HU histogram (`boa_label_hu_histogram`): the middle value, or the mean of the two middle values
    normalized `(ct - min) / (max - min)` per voxel in the reference; mean = (sum - n min) / (n (max - min)) in float64 -- the one
               non-integer path: the reference sums n doubles pairwise, so the unrounded means agree to ~1e-14 relative, not bitwise

The CT is `get_fdata().astype(np.int16)` in the reference: float values are truncated on the device (`boa_copy3`), and a CT whose
values leave int16 raises ValueError (numpy's cast is undefined there); so does a normalised request whose HU range exceeds 32767, where
the reference's int16 `ct - ct.min()` wraps around."""
from __future__ import annotations

import json
from typing import Optional, Sequence

import numpy as np

from . import label_maps
from ._lib import check, int3
from .devarray import DevArray
from .device import Context, Scope

BORDER = 3                    # touches_border, TS/statistics.py:76-88
TABLE_WORDS = 770             # BOA_LABEL_STATS_WORDS


def label_stats_table(ctx: Context, seg: DevArray, ct: DevArray, border: int = BORDER):
    """(count uint64[256], sum int64[256], touches bool[256], ct min, ct max) of contiguous device arrays on one grid: uint8 labels,
    int16 or int32 CT.  min / max are None for an empty volume."""
    if seg.shape != ct.shape:
        raise ValueError(f"label_stats_table: labels {seg.shape} and CT {ct.shape} are on different grids")
    if seg.dtype != np.uint8 or not seg.is_contiguous or not ct.is_contiguous:
        raise ValueError("label_stats_table: contiguous arrays, uint8 labels")
    code = {np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(ct.dtype)
    if code is None:
        raise TypeError(f"label_stats_table: CT dtype {ct.dtype} (int16 or int32)")
    out = ctx.alloc(TABLE_WORDS * 8)
    try:
        check(ctx.lib.boa_label_basic_stats(ctx.h, ct.buf.vp, code, seg.buf.vp, int3(seg.shape), int(border), out.vp), "boa_label_basic_stats")
        t = out.download((TABLE_WORDS,), np.uint64)
    finally:
        out.free()
    mm = t[768:770].view(np.int64)
    empty = seg.size == 0
    return t[:256].copy(), t[256:512].view(np.int64).copy(), t[512:768] != 0, None if empty else int(mm[0]), None if empty else int(mm[1])


def _int_ct(sc: Scope, ctx: Context, ct) -> DevArray:
    """The CT as a contiguous int16 or int32 device array whose values are those of `get_fdata().astype(np.int16)` wherever that cast
    is defined (floats truncate towards zero; anything outside int16 stays outside and is refused by the caller)."""
    if not isinstance(ct, DevArray):
        ct = np.asarray(ct)
        if ct.dtype.kind not in "iuf":
            raise TypeError(f"basic_statistics: CT dtype {ct.dtype}")
        if ct.dtype.kind == "f":
            if not np.isfinite(ct).all():
                raise ValueError("basic_statistics: the CT holds non-finite values")
            if ct.size and (ct.min() <= -2147483649.0 or ct.max() >= 2147483648.0):
                raise ValueError("basic_statistics: the CT's values do not fit int16")
            ct = ct.astype(np.float64 if ct.dtype.itemsize > 4 else np.float32)
        elif ct.dtype not in (np.uint8, np.int16, np.int32):
            if ct.size and (ct.min() < -32768 or ct.max() > 32767):
                raise ValueError("basic_statistics: the CT's values do not fit int16")
            ct = ct.astype(np.int16)
        ct = sc.own(DevArray.from_numpy(ctx, ct))
    if ct.dtype in (np.dtype(np.int16), np.dtype(np.int32)):
        if ct.is_contiguous:
            return ct
        return sc.own(ct.contiguous(force_copy=True))
    return sc.own(ct.contiguous(np.int16 if ct.dtype == np.uint8 else np.int32, force_copy=True))


def _median_values(ctx: Context, sc: Scope, seg: DevArray, ct: DevArray, labels: Sequence[int], counts, lo: int, hi: int) -> dict:
    """{label: (lower middle HU, upper middle HU)} of the non-empty `labels`: order statistics (n - 1) // 2 and n // 2 of the label's
    voxels from its HU histogram over [lo, hi] (the CT's range: no value is clamped)."""
    labels = [int(v) for v in labels if counts[int(v)] > 0 and int(v) != 0]
    if not labels:
        return {}
    if ct.dtype != np.int16:
        ct = sc.own(ct.contiguous(np.int16, force_copy=True))
    nbins = hi - lo + 1
    hist = sc.own(ctx.alloc(256 * nbins * 4))
    check(ctx.lib.boa_label_hu_histogram(ctx.h, ct.buf.vp, seg.buf.vp, None, seg.size, lo, nbins, hist.vp), "boa_label_hu_histogram")
    from .device import BufferView
    out = {}
    for v in labels:                      # (only the rows that are reported come back)
        row = BufferView(hist, v * nbins * 4, nbins * 4).download((nbins,), np.uint32)
        cum = np.cumsum(row.astype(np.int64))
        n = int(counts[v])
        assert int(cum[-1]) == n, (v, int(cum[-1]), n)
        a = int(np.searchsorted(cum, (n - 1) // 2 + 1)) + lo
        b = int(np.searchsorted(cum, n // 2 + 1)) + lo
        out[v] = (a, b)
    return out


def stats_from_table(counts, sums, touches, ct_min, ct_max, zooms, class_map: dict, exclude_masks_at_border: bool = True,
                     roi_subset: Optional[Sequence[str]] = None, metric: str = "mean", normalized_intensities: bool = False,
                     medians: Optional[dict] = None, return_unrounded: bool = False) -> dict:
    """The dict of get_basic_statistics from the device table (host arithmetic only; `medians` = `_median_values` for metric median)."""
    z = [np.float32(v) for v in zooms]
    vox_vol = z[0] * z[1] * z[2]
    if normalized_intensities:
        lo, rng = np.float64(ct_min), np.float64(ct_max - ct_min)
    stats, raw = {}, {}
    for idx, name in class_map.items():
        if roi_subset is not None and name not in roi_subset:
            continue
        n = np.int64(counts[idx])
        if exclude_masks_at_border and touches[idx]:
            stats[name] = {"volume": 0.0, "intensity": 0.0}
            continue
        if n == 0:
            val = 0.0
        elif metric == "mean":
            with np.errstate(invalid="ignore", divide="ignore"):
                if normalized_intensities:
                    val = (np.float64(int(sums[idx]) - int(n) * int(ct_min))) / (np.float64(n) * rng)
                else:
                    val = np.float64(sums[idx]) / np.float64(n)
            raw[name] = float(val)
            val = val.round(5)
        else:
            a, b = medians[idx]
            with np.errstate(invalid="ignore", divide="ignore"):
                if normalized_intensities:
                    a, b = (np.float64(a) - lo) / rng, (np.float64(b) - lo) / rng
                val = np.mean(np.array([a, b] if n % 2 == 0 else [a], dtype=np.float64 if normalized_intensities else np.int16))
            raw[name] = float(val)
            val = val.round(5)
        stats[name] = {"volume": n * vox_vol, "intensity": val}
    return (stats, raw) if return_unrounded else stats


def basic_statistics(ctx: Context, seg, ct, zooms, task: str = "total", exclude_masks_at_border: bool = True,
                     roi_subset: Optional[Sequence[str]] = None, metric: str = "mean", normalized_intensities: bool = False,
                     file_out=None, return_unrounded: bool = False):
    """get_basic_statistics (TS/statistics.py:91-141) of a label volume `seg` (uint8) and the CT `ct` on the same grid -- numpy arrays
    or DevArrays -- with the float32 header zooms `zooms`: {structure name: {"volume": mm^3, "intensity": mean or median}} in the
    class map's order, also written to `file_out` (json, indent 4) when given.  `return_unrounded`: (dict, {name: intensity before
    `.round(5)`}) instead (what the normalised mean is compared on)."""
    if metric not in ("mean", "median"):
        raise ValueError(f"basic_statistics: metric {metric!r} (mean or median)")
    # (TS/map_to_binary.py declares every class map in ascending id order, the order of the reference's dict; the data file's is not)
    cm = dict(sorted(label_maps.class_map(task).items()))
    with Scope() as sc:
        d_seg = seg if isinstance(seg, DevArray) else sc.own(DevArray.from_numpy(ctx, np.ascontiguousarray(seg, dtype=np.uint8)))
        if not d_seg.is_contiguous:
            d_seg = sc.own(d_seg.contiguous(force_copy=True))
        d_ct = _int_ct(sc, ctx, ct)
        counts, sums, touches, lo, hi = label_stats_table(ctx, d_seg, d_ct)
        if lo is not None and (lo < -32768 or hi > 32767):
            raise ValueError(f"basic_statistics: the CT's values [{lo}, {hi}] do not fit int16 (the reference casts with astype(np.int16))")
        if normalized_intensities and lo is not None and hi - lo > 32767:
            raise ValueError(f"basic_statistics: normalized_intensities with an HU range of {hi - lo} > 32767 (the reference's int16 "
                             "`ct - ct.min()` wraps around)")
        medians = None
        if metric == "median" and lo is not None:
            wanted = [i for i, nme in cm.items() if (roi_subset is None or nme in roi_subset)
                      and not (exclude_masks_at_border and touches[i])]
            medians = _median_values(ctx, sc, d_seg, d_ct, wanted, counts, lo, hi)
    res = stats_from_table(counts, sums, touches, lo, hi, zooms, cm, exclude_masks_at_border, roi_subset, metric, normalized_intensities,
                           medians, return_unrounded=True)
    if file_out is not None:
        with open(file_out, "w") as f:
            json.dump(res[0], f, indent=4)
    return res if return_unrounded else res[0]
