"""Blob post-processing of label volumes on the device (TS/postprocessing.py:13-98): keep_largest_blob,
keep_largest_blob_multilabel, remove_small_blobs, remove_small_blobs_multilabel with the reference's names and argument order
plus a leading `ctx`.

The reference loops over the labels and calls `scipy.ndimage.label(data == idx)` (6-connected) for each; the per-label passes
never interact, so "maximal face-connected sets of equal non-zero label" is ONE labelling of the uint8 volume
(`boa_label_blobs6`, csrc/ccl_labels.hip) and each function is one `boa_label_blobs_filter` call on its roots and sizes.

Array order: the kernel numbers components in raster order of the array it is given, last axis fastest, which is the order
scipy sees for a C-ordered array; a non-contiguous host array or device view is made contiguous (C order of its own axes) first.
That order decides the tie of `keep_largest_blob` (np.argmax takes the first = the lowest scipy number = the smallest root).
Every function takes a host array or a `DevArray` and returns the same kind: host arrays are not modified (a new array of the
same dtype comes back), a `DevArray` is filtered in place and returned."""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence, Tuple

import numpy as np

from ._lib import check
from .devarray import DevArray
from .device import Context

MODE_KEEP, MODE_INTERVAL, MODE_LARGEST = 0, 1, 2
U32_MAX = 2 ** 32 - 1


def interval_bounds(interval) -> Tuple[int, int]:
    """(lo, hi) in whole voxels of the reference's test `count <= interval[0] or count > interval[1]` on integer counts with float
    bounds: lo = floor(interval[0]) (0 if negative), hi = min(floor(interval[1]), 2**32 - 1) -- 1e10 means no upper bound."""
    a, b = float(interval[0]), float(interval[1])
    if b < 0:                      # every count exceeds the upper bound: everything goes
        return U32_MAX, U32_MAX
    return min(max(math.floor(a), 0), U32_MAX), min(math.floor(b), U32_MAX)


def size_threshold_voxels(size_thr_mm3: float, zooms) -> np.float32:
    """`size_thr_mm3 / vox_vol` of TS/nnunet.py:595-617 with `vox_vol = np.prod(img.header.get_zooms())`: the product of the three
    float32 header zooms in float32 (x, then y, then z), the quotient float32 too.  Goes into `interval[0]`: blobs of at most
    floor(result) voxels are removed."""
    z = np.asarray(zooms, dtype=np.float32)[:3]
    vox_vol = np.float32(np.float32(z[0] * z[1]) * z[2])     # np.prod of a float32 tuple: left to right, in float32
    return np.float32(size_thr_mm3) / vox_vol                 # (python int / np.float32 -> np.float32; 200 and 50000 are exact)


def modes_for(class_map: dict, rois: Sequence[str], mode: int) -> np.ndarray:
    """host_mode table of boa_label_blobs_filter: `mode` for the label ids of `rois`, 0 elsewhere."""
    inv = {v: k for k, v in class_map.items()}
    m = np.zeros(256, dtype=np.uint8)
    for roi in rois:
        idx = int(inv[roi])
        if not 0 < idx < 256:
            raise ValueError(f"label id {idx} of {roi!r} is not in 1..255")
        m[idx] = mode
    return m


class BlobLabelling:
    """One labelling of a contiguous uint8 DevArray (up to three axes of extent; last axis fastest) and the filters on it.  The
    filters work in place on that array; several may follow one labelling (the sizes of what remains do not change)."""

    def __init__(self, ctx: Context, labels: DevArray, count: bool = False):
        if labels.dtype != np.uint8 or not labels.is_contiguous:
            raise ValueError("BlobLabelling: contiguous uint8 DevArray required")
        self.ctx, self.labels, self.n = ctx, labels, labels.size
        self.n_components = None
        self.roots = self.sizes = None
        if self.n == 0:
            return
        self.roots, self.sizes = ctx.alloc(self.n * 4), ctx.alloc(self.n * 4)
        nc = C.c_int(0)
        try:
            check(ctx.lib.boa_label_blobs6(ctx.h, labels.buf.vp, *[int(s) for s in labels.shape], self.roots.vp, self.sizes.vp,
                                           C.byref(nc) if count else None), "boa_label_blobs6")
        except BaseException:
            self.free()
            raise
        if count:
            self.n_components = int(nc.value)

    def filter(self, modes: np.ndarray, lo: int = 0, hi: int = U32_MAX):
        if self.n == 0:
            return
        m = np.ascontiguousarray(modes, dtype=np.uint8)
        if m.shape != (256,):
            raise ValueError("modes: 256 entries")
        check(self.ctx.lib.boa_label_blobs_filter(self.ctx.h, self.roots.vp, self.sizes.vp, self.n, m.ctypes.data_as(C.c_void_p),
                                                  int(lo), int(hi), self.labels.buf.vp), "boa_label_blobs_filter")

    def free(self):
        for b in (self.roots, self.sizes):
            if b is not None:
                b.free()
        self.roots = self.sizes = None


def _filter_device(ctx: Context, d: DevArray, modes: np.ndarray, lo: int, hi: int):
    lab = BlobLabelling(ctx, d)
    try:
        lab.filter(modes, lo, hi)
    finally:
        lab.free()


def _as3d(a: np.ndarray) -> np.ndarray:
    if a.ndim > 3 or a.ndim == 0:
        raise ValueError("blobs: arrays of one to three dimensions")
    return np.ascontiguousarray(a).reshape((1,) * (3 - a.ndim) + a.shape)   # (unit axes add no neighbours)


def _run(ctx: Context, data, modes: np.ndarray, lo: int, hi: int, binary: bool):
    """The common body: `binary` = the reference labels `data` itself (non-zero = foreground) and returns a 0 / 1 mask."""
    if isinstance(data, DevArray):
        if data.dtype != np.uint8:
            raise TypeError("blobs: uint8 DevArray required")
        work = data.contiguous()
        try:
            if binary:
                check(ctx.lib.boa_label_select(ctx.h, work.buf.vp, work.size, 1, None, work.buf.vp), "boa_label_select")
            _filter_device(ctx, work, modes, lo, hi)
            if work is not data:
                work.copy_to(data)
        finally:
            if work is not data:
                work.free()
        return data
    data = np.asarray(data)
    if binary:
        host = (data != 0).astype(np.uint8)
    else:
        if data.dtype.kind not in "uib":
            raise TypeError(f"blobs: integer label array required, not {data.dtype}")
        if data.size and (data.min() < 0 or data.max() > 255):
            raise ValueError("blobs: label values must lie in 0..255")
        host = data.astype(np.uint8)
    if host.size == 0:
        return data
    d = DevArray.from_numpy(ctx, _as3d(host))
    try:
        _filter_device(ctx, d, modes, lo, hi)
        out = d.download().reshape(data.shape)
    finally:
        d.free()
    return out if binary else out.astype(data.dtype)


def _binary_modes(mode: int) -> np.ndarray:
    m = np.zeros(256, dtype=np.uint8)
    m[1] = mode
    return m


def keep_largest_blob(ctx: Context, data, debug: bool = False):
    """TS/postprocessing.py:13-21: the largest 6-connected blob of `data != 0` as a uint8 0 / 1 mask (tie: the first in array
    order).  Without foreground a host array is returned as it is; a DevArray becomes the mask in place."""
    if not isinstance(data, DevArray) and not np.asarray(data).any():
        return data
    return _run(ctx, data, _binary_modes(MODE_LARGEST), 0, U32_MAX, True)


def keep_largest_blob_multilabel(ctx: Context, data, class_map: dict, rois: Sequence[str], debug: bool = False, quiet: bool = False):
    """TS/postprocessing.py:24-43: for every label of `rois` only its largest blob stays; other labels are untouched."""
    return _run(ctx, data, modes_for(class_map, rois, MODE_LARGEST), 0, U32_MAX, False)


def remove_small_blobs(ctx: Context, img, interval=(10, 30), debug: bool = False):
    """TS/postprocessing.py:46-74: the blobs of `img != 0` whose voxel count is <= interval[0] or > interval[1] are removed; the
    result is a uint8 0 / 1 mask (the reference returns scipy's int32 label array with the same 0 / 1 values).  Without foreground a
    host array is returned as it is."""
    if not isinstance(img, DevArray) and not np.asarray(img).any():
        return img
    lo, hi = interval_bounds(interval)
    return _run(ctx, img, _binary_modes(MODE_INTERVAL), lo, hi, True)


def remove_small_blobs_multilabel(ctx: Context, data, class_map: dict, rois: Sequence[str], interval=(10, 30), debug: bool = False,
                                  quiet: bool = False):
    """TS/postprocessing.py:77-98: remove_small_blobs on every label of `rois`; other labels are untouched."""
    lo, hi = interval_bounds(interval)
    return _run(ctx, data, modes_for(class_map, rois, MODE_INTERVAL), lo, hi, False)
