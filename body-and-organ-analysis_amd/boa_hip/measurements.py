"""Per-label HU measurements from ONE device histogram pass (host side).

Mirrors BOA/compute/measurements.py for arrays in SimpleITK order (z, y, x):
  metrics_for_region (:74-123), metrics_for_each_region (:203-241), autochthon_reference (:42-58),
  erode_region (:61-71), compute_lung_measurement / ct_pfav (:126-200), compute_measurements (:244-343, the
  `total` branch incl. the CNR-adjusted regions of CNR_ADJUSTED_REGIONS).
The reference makes ~125 full-volume passes (one boolean mask, one fancy-index gather and seven reductions per
label).  Here the device builds hist[label][HU] over the whole int16 range in a single 3 B/voxel pass
(boa_label_hu_histogram); count / mean / std / min / max / median / percentiles of every label, of label unions
(autochthon left+right, lung lobes) and of HU-window sub-masks (pulmonary fat) follow exactly from the integer
counts on the host.  Only the eroded masks of the CNR adjustment need extra passes (mask -> separable erosion ->
histogram).
Exactness: counts, min, max, median, percentiles (numpy 'linear' interpolation restated operation for operation),
mean (exact integer sum / n) are bit-identical to numpy on the same integer data; std differs by summation order
only (<= 1e-12 relative).

CTs that are not int16-exact (float-valued, scaled, out of range: `require_int16_exact` refuses them) take the float64 path: the
values `get_fdata()` returns stay float64 on the device, boa_group_stats_f64 returns count / sum / centred sum of squares / min /
max and the six order statistics behind median and quartiles per label group (radix select: exact), and `stats_from_order`
forms the reference's statistics from them.  BOA_STATS_FLOAT=1 sends int16-exact CTs down that path as well (cross-check).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, Iterable, Optional, Tuple

import numpy as np

from ._lib import check
from .device import Context, DeviceBuffer

ADIPOSE_TISSUE = (-200, -40)  # BOA/compute/measurements.py:22
HU_MIN, NBINS = -32768, 65536
CNR_ADJUSTED_REGIONS = {"total": {"aorta", "autochthon_left", "autochthon_right"},
                        "heartchambers_highres": {"pulmonary_artery"}}
LUNG_MASKS = ["lung_upper_lobe_left", "lung_lower_lobe_left", "lung_upper_lobe_right", "lung_middle_lobe_right",
              "lung_lower_lobe_right"]


# ---- statistics from an integer histogram ---------------------------------------------------------------
def _lerp(a: float, b: float, t: float) -> float:
    """numpy.lib._function_base_impl._lerp for scalars."""
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1 - t)
    return r


def occupied_window(hist: np.ndarray):
    """[b0, b1): the bin range outside which every row of `hist` [rows, nbins] is empty (one OR-reduction over the rows
    instead of a 65 536-bin scan per label: CT values occupy a few thousand of the int16 bins)."""
    h = np.ascontiguousarray(hist)
    cols = np.bitwise_or.reduce(h.view(np.uint64) if (h.dtype.itemsize == 4 and h.shape[1] % 2 == 0) else h, axis=0)
    nz = np.flatnonzero(cols)
    if nz.size == 0:
        return 0, 0
    k = 2 if cols.shape[0] != h.shape[1] else 1
    return int(nz[0]) * k, (int(nz[-1]) + 1) * k


def stats_from_hist(h: np.ndarray, hu_min: int = HU_MIN) -> Optional[Dict[str, float]]:
    """h: uint32/int64 [nbins] counts of value hu_min + bin.  Returns None for an empty region."""
    nz = np.nonzero(h)[0]
    if nz.size == 0:
        return None
    cnt = h[nz].astype(np.int64)
    vals = nz.astype(np.int64) + hu_min
    n = int(cnt.sum())
    total = int((vals * cnt).sum())
    mean = float(np.float64(total) / np.float64(n))
    dev = vals.astype(np.float64) - mean
    var = float((dev * dev * cnt).sum() / n)
    cum = np.cumsum(cnt)

    def kth(k: int) -> float:
        return float(vals[np.searchsorted(cum, k, side="right")])

    def percentile(p: float) -> float:
        virt = (n - 1) * (p / 100.0)
        prev = int(np.floor(virt))
        nxt = min(prev + 1, n - 1)
        return float(_lerp(kth(prev), kth(nxt), virt - prev))

    if n % 2:
        median = kth(n // 2)
    else:
        median = (kth(n // 2 - 1) + kth(n // 2)) / 2.0
    return {"n": n, "mean": mean, "std": float(np.sqrt(var)), "min": float(vals[0]), "max": float(vals[-1]),
            "median": median, "p25": percentile(25), "p75": percentile(75)}


def _metrics(st: Optional[dict], ml_per_voxel: float, auto_mean, auto_std, cnr_none: bool = False) -> Dict[str, Any]:
    """Dict layout of metrics_for_region (:74-123)."""
    if st is None:
        return {"present": False}
    out: Dict[str, Any] = {"present": True, "volume_ml": st["n"] * ml_per_voxel, "mean_hu": st["mean"], "std_hu": st["std"],
                           "min_hu": st["min"], "median_hu": st["median"], "max_hu": st["max"],
                           "25th_percentile_hu": st["p25"], "75th_percentile_hu": st["p75"]}
    if auto_mean is not None and auto_std is not None and not cnr_none:
        # numpy scalar arithmetic like the reference (`np.mean(hu_region) - autochthon_mean) / autochthon_std`, :117-119): a
        # constant-HU autochthon (std 0) gives inf / nan with a RuntimeWarning there, not a ZeroDivisionError
        with np.errstate(divide="ignore", invalid="ignore"):
            out["cnr"] = (np.float64(st["mean"]) - auto_mean) / np.float64(auto_std)
    else:
        out["cnr"] = None
    return out


# ---- statistics of float64 voxels (CTs that are not int16-exact) -----------------------------------------
STATS_F64_COLS = 10   # boa_group_stats_f64: min, max, sum, m2, order statistics of q = 1/4, 1/2, 3/4 (floor rank, ceil rank)


def force_float_stats() -> bool:
    """BOA_STATS_FLOAT=1: int16-exact CTs take the float64 statistics path too (to compare the two paths on the same data)."""
    return os.environ.get("BOA_STATS_FLOAT", "") not in ("", "0")


def ct_for_stats(values: np.ndarray, what: str = "CT") -> Tuple[np.ndarray, bool]:
    """-> (array to upload, is_float): the int16 array when `require_int16_exact` accepts the values (today's histogram path),
    otherwise the values as float64 for the float path.  NaN / +-inf are refused: `what` names the file."""
    from .compute.util import require_int16_exact
    values = np.asarray(values)
    if not force_float_stats():
        try:
            with np.errstate(invalid="ignore"):       # (NaN / inf -> int16 in the check; they are refused below)
                return require_int16_exact(values, what), False
        except ValueError:
            pass
    f = np.ascontiguousarray(values, dtype=np.float64)
    if not np.isfinite(f).all():
        raise ValueError(f"{what}: the CT holds {int((~np.isfinite(f)).sum())} non-finite voxel values (NaN or inf); HU statistics "
                         "are undefined on them")
    return f, True


def stats_from_order(count: int, total: float, m2: float, vmin: float, vmax: float, order) -> Optional[Dict[str, float]]:
    """The reference's eight statistics of one voxel group from what the device returns: `count` voxels, their sum `total`, the
    centred sum of squares `m2` about total / count, min, max and `order` = the sorted group's elements at the 0-based ranks
    floor / ceil of (count-1)*q for q = 0.25, 0.5, 0.75.  np.percentile's linear rule (`_lerp`, as in `stats_from_hist`); the
    median is np.median's mean of the two middle elements, which can differ from the lerp form in the last bit.  None for an
    empty group."""
    n = int(count)
    if n == 0:
        return None
    o = [float(v) for v in order]

    def percentile(p: float, lo: float, hi: float) -> float:
        virt = (n - 1) * (p / 100.0)
        return float(_lerp(lo, hi, virt - int(np.floor(virt))))

    mean = float(np.float64(total) / np.float64(n))
    return {"n": n, "mean": mean, "std": float(np.sqrt(np.float64(m2) / np.float64(n))), "min": float(vmin), "max": float(vmax),
            "median": o[2] if n % 2 else (o[2] + o[3]) / 2.0, "p25": percentile(25, o[0], o[1]), "p75": percentile(75, o[4], o[5])}


def group_stats_f64(ctx: Context, d_ct: DeviceBuffer, d_labels: DeviceBuffer, n: int, lut: np.ndarray, n_groups: int):
    """boa_group_stats_f64 -> [stats dict | None per group].  lut: uint8[256], label value -> group, 0xFF = not measured."""
    lut = np.ascontiguousarray(lut, dtype=np.uint8)
    counts = np.zeros(n_groups, dtype=np.uint64)
    st = np.zeros((n_groups, STATS_F64_COLS), dtype=np.float64)
    check(ctx.lib.boa_group_stats_f64(ctx.h, d_ct.vp, d_labels.vp, int(n), lut.ctypes.data_as(C.c_void_p), int(n_groups),
                                      counts.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)), "boa_group_stats_f64")
    return [stats_from_order(int(counts[g]), st[g, 2], st[g, 3], st[g, 0], st[g, 1], st[g, 4:10]) for g in range(n_groups)]


def _group_lut(groups) -> np.ndarray:
    """groups: [iterable of label values per group] (disjoint) -> lut."""
    lut = np.full(256, 0xFF, dtype=np.uint8)
    for g, labels in enumerate(groups):
        for l in labels:
            lut[int(l)] = g
    return lut


def _masked_stats_f64(ctx, d_ct, d_mask, n):
    """stats of ct[mask != 0] for a 0/1 mask: the mask is the label volume, lut[1] = group 0."""
    return group_stats_f64(ctx, d_ct, d_mask, n, _group_lut([[1]]), 1)[0]


def label_hu_mask_f64(ctx: Context, d_ct, d_labels, labels, mode: int, n: int, out: DeviceBuffer, window=ADIPOSE_TISSUE):
    """`label_hu_mask` on float64 HU: the window is compared on the float value (numpy's `ct >= lo`, `ct < lo`)."""
    lut = _lut(labels)
    check(ctx.lib.boa_label_hu_mask_f64(ctx.h, d_ct.vp, d_labels.vp, lut.ctypes.data_as(C.c_void_p), mode, float(window[0]),
                                        float(window[1]), n, out.vp), "boa_label_hu_mask_f64")


def _label_stats_f64(ctx, d_ct, d_lab, n, label_map) -> Dict[int, Optional[dict]]:
    """{label value: stats} of every label of `label_map` from one boa_group_stats_f64 call."""
    labels = sorted({int(l) for l in label_map.values() if 0 < int(l) < 256})
    if not labels:
        return {}
    return dict(zip(labels, group_stats_f64(ctx, d_ct, d_lab, n, _group_lut([[l] for l in labels]), len(labels))))


def _metrics_from_groups(ctx, d_ct, d_lab, n, label_map, am, asd, spacing, by_label=None):
    """`_metrics_from_hist` for the float path -> (metrics, {label: stats})."""
    ml = np.prod(spacing) / 1000.0
    by_label = _label_stats_f64(ctx, d_ct, d_lab, n, label_map) if by_label is None else by_label
    res = {region: _metrics(by_label.get(int(label)), ml, am, asd) for region, label in label_map.items()}
    if "autochthon_left" in label_map and "autochthon_right" in label_map:
        both = group_stats_f64(ctx, d_ct, d_lab, n, _group_lut([[label_map["autochthon_left"], label_map["autochthon_right"]]]), 1)[0]
        res["autochthon"] = _metrics(both, ml, am, asd)
    return res, by_label


def _total_measurements_f64(ctx, d_ct, d_lab, shape, label_map, spacing, cnr_adjustment, model_name, mask_on_device, defer_host):
    """`total_measurements` on a resident float64 CT: the same masks and erosions, group statistics instead of histograms."""
    n = int(np.prod(shape))
    ml = np.prod(spacing) / 1000.0
    info: Dict[str, Any] = {}
    adj: Optional[Dict[str, Any]] = None
    d_m, d_e, d_t = ctx.alloc(max(n, 1)), ctx.alloc(max(n, 1)), ctx.alloc(max(n, 1))
    keep_mask = None
    try:
        by_label = _label_stats_f64(ctx, d_ct, d_lab, n, label_map)
        # autochthon reference: (left | right) minus fat, eroded (:42-58)
        auto_labels = [label_map["autochthon_left"], label_map["autochthon_right"]]
        label_hu_mask_f64(ctx, d_ct, d_lab, auto_labels, 2, n, d_m)
        binary_erode(ctx, d_m, d_e, d_t, shape)
        st_auto = _masked_stats_f64(ctx, d_ct, d_e, n)
        am, asd = (st_auto["mean"], st_auto["std"]) if st_auto else (None, None)
        seg, _ = _metrics_from_groups(ctx, d_ct, d_lab, n, label_map, am, asd, spacing, by_label)
        # pulmonary fat (ct_pfav, :151-200): the lung labels inside the fat window, as a label volume (d_e: lobe label or 0)
        lungs = [label_map[nm] for nm in LUNG_MASKS]
        label_hu_mask_f64(ctx, d_ct, d_lab, lungs, 1, n, d_m)
        check(ctx.lib.boa_copy3(ctx.h, d_lab.vp, 0, 0, (C.c_longlong * 3)(0, 0, 1), (C.c_int * 3)(1, 1, n), d_e.vp, 0, 0,
                                (C.c_longlong * 3)(0, 0, 1)), "boa_copy3")
        check(ctx.lib.boa_mask_assign(ctx.h, d_m.vp, n, 1, 0, d_e.vp), "boa_mask_assign")      # d_e[mask == 0] = 0
        sides = [[label_map[nm] for nm in LUNG_MASKS if nm.endswith(side)] for side in ("left", "right")]
        lobe = group_stats_f64(ctx, d_ct, d_e, n, _group_lut([[l] for l in lungs]), len(lungs))
        side = group_stats_f64(ctx, d_ct, d_e, n, _group_lut(sides), 2)
        whole = group_stats_f64(ctx, d_ct, d_e, n, _group_lut([lungs]), 1)
        pf = {"ct_pfav_" + nm: _metrics(st, ml, am, asd) for nm, st in zip(LUNG_MASKS, lobe)}
        pf["ct_pfav_lobe_left"], pf["ct_pfav_lobe_right"] = (_metrics(st, ml, am, asd) for st in side)
        pf["ct_pfav_lungs"] = _metrics(whole[0], ml, am, asd)
        if mask_on_device:
            keep_mask = ctx.alloc(n)
            check(ctx.lib.boa_copy3(ctx.h, d_m.vp, 0, 0, (C.c_longlong * 3)(0, 0, 1), (C.c_int * 3)(1, 1, n), keep_mask.vp, 0, 0,
                                    (C.c_longlong * 3)(0, 0, 1)), "boa_copy3")
            fat_mask = keep_mask
        else:
            fat_mask = d_m.download(shape, np.uint8)
        if cnr_adjustment and model_name in CNR_ADJUSTED_REGIONS and am is not None and asd is not None:
            adj = {}
            regions = [r for r in label_map if r in CNR_ADJUSTED_REGIONS[model_name]]
            for region in regions:
                is_auto = "autochthon" in region
                label_hu_mask_f64(ctx, d_ct, d_lab, [label_map[region]], 2 if is_auto else 0, n, d_m)
                binary_erode(ctx, d_m, d_e, d_t, shape)
                st = _masked_stats_f64(ctx, d_ct, d_e, n) if by_label.get(int(label_map[region])) else None
                adj[region] = _metrics(st, ml, am, asd, cnr_none=region.partition("_")[0] == "autochthon")
            if {"autochthon_left", "autochthon_right"} <= set(regions):
                present = any(by_label.get(int(l)) for l in auto_labels)      # union, minus fat, eroded == the reference mask above
                adj["autochthon"] = _metrics(st_auto if present else None, ml, am, asd, cnr_none=True)
        info["autochthon_mean"], info["autochthon_std"] = am, asd
        keep_mask = None
        out = {"segmentations": {model_name: {**seg, **pf}}, "info": info}      # key order of the reference's dict
        if adj is not None:
            out["cnr_adjusted"] = adj
        return ((lambda: out) if defer_host else out), fat_mask
    finally:
        for b in (d_m, d_e, d_t) + ((keep_mask,) if keep_mask is not None else ()):
            b.free()


# ---- device passes --------------------------------------------------------------------------------------
def _label_hu_histogram_local(ctx: Context, d_ct: DeviceBuffer, d_labels: DeviceBuffer, n: int,
                              d_mask: Optional[DeviceBuffer] = None) -> np.ndarray:
    d_hist = ctx.alloc(256 * NBINS * 4)
    check(ctx.lib.boa_label_hu_histogram(ctx.h, d_ct.vp, d_labels.vp, d_mask.vp if d_mask else None, n, HU_MIN, NBINS,
                                         d_hist.vp), "boa_label_hu_histogram")
    h = d_hist.download((256, NBINS), np.uint32)
    d_hist.free()
    return h


label_hu_histogram = _label_hu_histogram_local


def _lut(labels: Iterable[int]) -> np.ndarray:
    lut = np.zeros(256, dtype=np.uint8)
    for l in labels:
        lut[int(l)] = 1
    return lut


def label_hu_mask(ctx: Context, d_ct, d_labels, labels, mode: int, n: int, out: DeviceBuffer, window=ADIPOSE_TISSUE):
    """mode 0: label in set; 1: and lo <= HU <= hi; 2: and (HU < lo or HU > hi)."""
    lut = _lut(labels)
    check(ctx.lib.boa_label_hu_mask(ctx.h, d_ct.vp, d_labels.vp, lut.ctypes.data_as(C.c_void_p), mode, window[0], window[1],
                                    n, out.vp), "boa_label_hu_mask")


def binary_erode(ctx: Context, d_mask: DeviceBuffer, d_out: DeviceBuffer, d_tmp: DeviceBuffer, shape, kernel_value: int = 6):
    check(ctx.lib.boa_binary_erode(ctx.h, d_mask.vp, d_out.vp, d_tmp.vp, int(shape[0]), int(shape[1]), int(shape[2]),
                                   kernel_value), "boa_binary_erode")


def erode_region(ctx: Context, mask: np.ndarray, kernel_value: int = 6) -> np.ndarray:
    """erode_region (:61-71) for a host boolean array."""
    n = mask.size
    d_m = ctx.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8))
    d_o, d_t = ctx.alloc(n), ctx.alloc(n)
    try:
        binary_erode(ctx, d_m, d_o, d_t, mask.shape, kernel_value)
        return d_o.download(mask.shape, np.uint8).astype(bool)
    finally:
        for b in (d_m, d_o, d_t):
            b.free()


def _masked_stats_local(ctx, d_ct, d_mask, n):
    """stats of ct[mask != 0]: histogram with the mask itself as the (0/1) label volume; only row 1 comes back."""
    from .device import BufferView
    d_hist = ctx.alloc(256 * NBINS * 4)
    try:
        check(ctx.lib.boa_label_hu_histogram(ctx.h, d_ct.vp, d_mask.vp, None, n, HU_MIN, NBINS, d_hist.vp), "boa_label_hu_histogram")
        row = BufferView(d_hist, NBINS * 4, NBINS * 4).download((NBINS,), np.uint32)
    finally:
        d_hist.free()
    return stats_from_hist(row)


_masked_stats = _masked_stats_local


def metrics_for_each_region(ctx: Context, ct: np.ndarray, region_data: np.ndarray, label_map: Dict[str, int],
                            autochthon_mean, autochthon_std, img_spacing) -> Dict[str, Any]:
    """metrics_for_each_region (:203-241), cnr_adjustment=False, from one histogram pass (int16-exact CT) or one group
    statistics call (any other CT, as float64)."""
    n = ct.size
    ct, is_float = ct_for_stats(ct)
    d_ct = ctx.from_numpy(np.ascontiguousarray(ct))
    d_lab = ctx.from_numpy(np.ascontiguousarray(region_data, dtype=np.uint8))
    try:
        if is_float:
            return _metrics_from_groups(ctx, d_ct, d_lab, n, label_map, autochthon_mean, autochthon_std, img_spacing)[0]
        hist = label_hu_histogram(ctx, d_ct, d_lab, n)
    finally:
        d_ct.free()
        d_lab.free()
    return _metrics_from_hist(hist, label_map, autochthon_mean, autochthon_std, img_spacing)


def _metrics_from_hist(hist, label_map, am, asd, spacing):
    ml = np.prod(spacing) / 1000.0
    res = {}
    b0, b1 = occupied_window(hist)
    hw, hu0 = hist[:, b0:b1], HU_MIN + b0          # same statistics: bin b of the window is HU hu0 + b
    for region, label in label_map.items():
        res[region] = _metrics(stats_from_hist(hw[label], hu0) if 0 < label < 256 else None, ml, am, asd)
    if "autochthon_left" in label_map and "autochthon_right" in label_map:
        h = hw[label_map["autochthon_left"]].astype(np.int64) + hw[label_map["autochthon_right"]]
        res["autochthon"] = _metrics(stats_from_hist(h, hu0), ml, am, asd)
    return res


def cnr_adjusted_region_metrics(ctx: Context, d_ct: DeviceBuffer, d_lab: DeviceBuffer, shape, label_map: Dict[str, int],
                                regions: Iterable[str], hist, am, asd, spacing, ct_f64: bool = False) -> Dict[str, Any]:
    """`metrics_for_each_region(..., cnr_adjustment=True)` for the `regions` of a model other than `total`
    (BOA/compute/measurements.py:318-341; e.g. heartchambers_highres / pulmonary_artery): the region's mask (autochthon names:
    minus fat) is eroded with the 6^3 kernel before the statistics (metrics_for_region, :85-93).  `hist`: the model's
    per-label histogram (tells which labels are present).  `ct_f64`: `d_ct` holds float64 and `hist` is the {label: stats}
    table of `_metrics_from_groups`."""
    mask_of, stats_of = (label_hu_mask_f64, _masked_stats_f64) if ct_f64 else (label_hu_mask, _masked_stats_local)
    shape = tuple(int(v) for v in shape)
    n = int(np.prod(shape))
    ml = np.prod(spacing) / 1000.0
    d_m, d_e, d_t = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    out: Dict[str, Any] = {}
    try:
        for region in [r for r in label_map if r in set(regions)]:
            is_auto = "autochthon" in region
            mask_of(ctx, d_ct, d_lab, [label_map[region]], 2 if is_auto else 0, n, d_m)
            binary_erode(ctx, d_m, d_e, d_t, shape)
            present = bool(hist.get(int(label_map[region]))) if ct_f64 else hist[label_map[region]].any()
            st = stats_of(ctx, d_ct, d_e, n) if present else None
            out[region] = _metrics(st, ml, am, asd, cnr_none=region.partition("_")[0] == "autochthon")
    finally:
        for b in (d_m, d_e, d_t):
            b.free()
    return out


def total_measurements(ctx: Context, ct: Optional[np.ndarray], total_seg: Optional[np.ndarray], label_map: Dict[str, int],
                       spacing, cnr_adjustment: bool = True, model_name: str = "total", d_ct: Optional[DeviceBuffer] = None,
                       d_lab: Optional[DeviceBuffer] = None, shape=None, mask_on_device: bool = False, shard=None,
                       defer_host: bool = False, ct_f64: bool = False):
    """compute_measurements (:244-343) for models == ["total"] on (z,y,x) arrays.  Returns (measurements dict, ct_pfav
    mask).  `defer_host=True`: the device passes run now, the ~120 per-label order statistics (pure numpy on the downloaded
    histogram) are returned as a function `finish() -> measurements dict` in place of the dict, so that a caller can run them
    on a worker thread while the device works on the next stage (bench.py: under the BCA nets).  Resident inputs: pass `d_ct` (int16) / `d_lab` (uint8) + `shape` instead of the host arrays (not freed here);
    `mask_on_device=True` returns the mask as a DeviceBuffer (caller frees).

    `shard` = (agg_shard.AggComm, (a, b)): the arrays are this rank's z-slab of the volume INCLUDING a halo of
    agg_shard.ERODE_REACH planes towards its neighbours, and planes [a, b) of them are the ones the rank owns.  Masks and
    erosions run on the whole slab (the halo supplies the neighbours' voxels; its own planes are discarded), histograms only
    over the owned planes and are summed over the ranks -- every rank returns the volume's measurements; the returned
    ct_pfav mask covers the slab.

    A host `ct` that is not int16-exact (or any, with BOA_STATS_FLOAT=1) is uploaded as float64 and measured by the float path;
    `ct_f64=True` says that a resident `d_ct` holds float64."""
    own = d_ct is None
    if own:
        if ct.shape != total_seg.shape:
            raise ValueError("The spacing of the image and of the segmentation should be the same")  # shape contract
        shape = ct.shape
        ct, ct_f64 = ct_for_stats(ct)
        d_ct = ctx.from_numpy(np.ascontiguousarray(ct))
        d_lab = ctx.from_numpy(np.ascontiguousarray(total_seg, dtype=np.uint8))
    shape = tuple(int(v) for v in shape)
    if ct_f64:
        try:
            if shard is not None:
                raise NotImplementedError("total_measurements: z-slab sharding (agg_shard) of a float64 CT is not implemented")
            return _total_measurements_f64(ctx, d_ct, d_lab, shape, label_map, spacing, cnr_adjustment, model_name, mask_on_device,
                                           defer_host)
        finally:
            if own:
                d_ct.free()
                d_lab.free()
    n = int(np.prod(shape))
    ml = np.prod(spacing) / 1000.0
    meas: Dict[str, Any] = {"segmentations": {}, "info": {}}
    d_m, d_e, d_t = ctx.alloc(max(n, 1)), ctx.alloc(max(n, 1)), ctx.alloc(max(n, 1))
    keep_mask = None
    if shard is not None:
        from .device import BufferView
        comm, (own_a, own_b) = shard
        plane = shape[1] * shape[2]
        n_own = (own_b - own_a) * plane

        def owned(buf, itemsize):
            return BufferView(buf, own_a * plane * itemsize, n_own * itemsize)

        def label_hu_histogram(ctx_, dc, dl, n_, d_mask=None):          # noqa: F811  (slab version: owned planes, all-reduced)
            h = _label_hu_histogram_local(ctx_, owned(dc, 2), owned(dl, 1), n_own, owned(d_mask, 1) if d_mask is not None else None) \
                if n_own else np.zeros((256, NBINS), np.uint32)
            return comm.all_reduce_sum(h)

        def _masked_stats(ctx_, dc, d_mask, n_):                       # noqa: F811
            return stats_from_hist(label_hu_histogram(ctx_, dc, d_mask, n_)[1])
    else:
        label_hu_histogram = _label_hu_histogram_local
        _masked_stats = _masked_stats_local
    try:
        hist = label_hu_histogram(ctx, d_ct, d_lab, n)
        # autochthon reference: (left | right) minus fat, eroded (:42-58)
        auto_labels = [label_map["autochthon_left"], label_map["autochthon_right"]]
        label_hu_mask(ctx, d_ct, d_lab, auto_labels, 2, n, d_m)
        binary_erode(ctx, d_m, d_e, d_t, shape)
        st_auto = _masked_stats(ctx, d_ct, d_e, n)
        am, asd = (st_auto["mean"], st_auto["std"]) if st_auto else (None, None)
        # pulmonary fat (ct_pfav, :151-200): the fat window of a label (union) is a bin range of its histogram rows
        lo, hi = ADIPOSE_TISSUE[0] - HU_MIN, ADIPOSE_TISSUE[1] - HU_MIN

        def fat_metrics(names):
            h = np.zeros(hi + 1 - lo, dtype=np.int64)
            for nm in names:
                h += hist[label_map[nm]][lo:hi + 1]
            return _metrics(stats_from_hist(h, ADIPOSE_TISSUE[0]), ml, am, asd)

        def host_tables():
            seg = _metrics_from_hist(hist, label_map, am, asd, spacing)
            pf = {}
            for nm in LUNG_MASKS:
                pf["ct_pfav_" + nm] = fat_metrics([nm])
            for side in ("left", "right"):
                pf[f"ct_pfav_lobe_{side}"] = fat_metrics([nm for nm in LUNG_MASKS if nm.endswith(side)])
            pf["ct_pfav_lungs"] = fat_metrics(LUNG_MASKS)
            return {**seg, **pf}

        label_hu_mask(ctx, d_ct, d_lab, [label_map[nm] for nm in LUNG_MASKS], 1, n, d_m)
        if mask_on_device:
            keep_mask = ctx.alloc(n)
            check(ctx.lib.boa_copy3(ctx.h, d_m.vp, 0, 0, (C.c_longlong * 3)(0, 0, 1), (C.c_int * 3)(1, 1, n), keep_mask.vp, 0, 0,
                                    (C.c_longlong * 3)(0, 0, 1)), "boa_copy3")
            fat_mask = keep_mask
        else:
            fat_mask = d_m.download(shape, np.uint8)
        if cnr_adjustment and model_name in CNR_ADJUSTED_REGIONS:
            if am is not None and asd is not None:
                adj = {}
                regions = [r for r in label_map if r in CNR_ADJUSTED_REGIONS[model_name]]
                for region in regions:
                    is_auto = "autochthon" in region
                    label_hu_mask(ctx, d_ct, d_lab, [label_map[region]], 2 if is_auto else 0, n, d_m)
                    binary_erode(ctx, d_m, d_e, d_t, shape)
                    st = _masked_stats(ctx, d_ct, d_e, n) if hist[label_map[region]].any() else None
                    adj[region] = _metrics(st, ml, am, asd, cnr_none=region.partition("_")[0] == "autochthon")
                if "autochthon_left" in label_map and "autochthon_right" in label_map and \
                        {"autochthon_left", "autochthon_right"} <= set(regions):
                    # union, minus fat, eroded == the reference mask computed above
                    present = hist[auto_labels[0]].any() or hist[auto_labels[1]].any()
                    adj["autochthon"] = _metrics(st_auto if present else None, ml, am, asd, cnr_none=True)
                meas.setdefault("cnr_adjusted", {}).update(adj)
        meas["info"]["autochthon_mean"] = am
        meas["info"]["autochthon_std"] = asd
        keep_mask = None

        def finish():
            out = {"segmentations": {model_name: host_tables()}, "info": meas["info"]}      # key order of the reference's dict
            if "cnr_adjusted" in meas:
                out["cnr_adjusted"] = meas["cnr_adjusted"]
            return out

        return (finish if defer_host else finish()), fat_mask
    finally:
        for b in ((d_ct, d_lab) if own else ()) + (d_m, d_e, d_t) + ((keep_mask,) if keep_mask is not None else ()):
            b.free()
