"""numpy references of nnU-Net's one-hot label resampling (TotalSegmentator's `higher_order_resampling`; TS/resample_nnunet.py
`resize_segmentation` :11-33 and the is_seg branch of `resample_data_or_seg` :119-205, order 1, order_z 0).

  resample_seg_loop   the literal algorithm: every label's 0/1 mask through `oracle.nnunet_resample.skimage_resize` (the project's
                      stand-in for skimage.transform.resize, which is not installed: scipy.ndimage.zoom(grid_mode=True,
                      mode="nearest") + clip), `>= 0.5`, labels ascending; per slice + map_coordinates(order=0) in the separate-z
                      form.  THE reference of the GPU tests.
  resample_seg_taps   the kernel's blueprint: per output voxel the 8 taps (4 in a slice), per tap label the fp64 sum of the
                      matching tap weights in tap order, the largest label with a sum >= 0.5.

Both work on the reference's axis order [z, x, y] (TS/resampling.py:105-125).  `to_ref` / `from_ref` move an (x, y, z) array --
the memory layout of the device pass -- there and back; `resample_xyz` wraps either function for (x, y, z) arrays."""
import itertools

import numpy as np
from scipy import ndimage

from oracle.nnunet_resample import skimage_resize


def to_ref(a_xyz):
    return np.ascontiguousarray(np.asarray(a_xyz).transpose(2, 0, 1))


def from_ref(a_zxy):
    return np.ascontiguousarray(np.asarray(a_zxy).transpose(1, 2, 0))


def resize_segmentation(seg, new_shape):
    """TS/resample_nnunet.py:11-33 with order 1."""
    out = np.zeros(tuple(int(v) for v in new_shape), dtype=seg.dtype)
    for c in np.unique(seg):
        out[skimage_resize((seg == c).astype(float), new_shape, 1) >= 0.5] = c
    return out


def resample_seg_loop(seg, new_shape, sep_axis=None):
    """seg [z, x, y] uint8 -> new_shape; sep_axis None / -1: one 3-D resize_segmentation, else the separate-z form along it."""
    seg = np.asarray(seg)
    new_shape = np.array([int(v) for v in new_shape])
    shape = np.array(seg.shape)
    if not np.any(shape != new_shape):
        return seg.copy()                                   # "no resampling necessary"
    data = seg.astype(float)
    if sep_axis is None or sep_axis < 0:
        return resize_segmentation(data, new_shape).astype(seg.dtype)
    axis = int(sep_axis)
    shape2d = np.delete(new_shape, axis)
    slices = [resize_segmentation(np.take(data, s, axis=axis), shape2d) for s in range(shape[axis])]
    here = np.stack(slices, axis)
    if shape[axis] != new_shape[axis]:
        rows, cols, dim = (int(v) for v in new_shape)
        orows, ocols, odim = here.shape
        mr, mc, md = np.mgrid[:rows, :cols, :dim]
        coords = np.array([float(orows) / rows * (mr + 0.5) - 0.5, float(ocols) / cols * (mc + 0.5) - 0.5,
                           float(odim) / dim * (md + 0.5) - 0.5])
        here = ndimage.map_coordinates(here, coords, order=0, cval=-1, mode="nearest")
    return here.astype(seg.dtype)


def axis_taps(n_in, n_out, active):
    """Per output index: (i0, i1, w0, w1), the table of csrc/resample_onehot.h `onehot_axis_tap`."""
    cc = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
    if active:
        fl = np.floor(cc)
        x = cc - fl
        i0 = np.clip(fl.astype(np.int64), 0, n_in - 1)
        i1 = np.clip(fl.astype(np.int64) + 1, 0, n_in - 1)
        return i0, i1, 1.0 - x, x
    i = np.arange(n_out) if n_in == n_out else np.clip(np.floor(cc + 0.5).astype(np.int64), 0, n_in - 1)
    return i, i, np.ones(n_out), np.zeros(n_out)


def resample_seg_taps(seg, new_shape, sep_axis=None, select=None):
    """The 8-tap formulation on [z, x, y]: taps in itertools.product order, weight 1.0 * w_0 * w_1 * w_2 left to right.
    `select` (three index arrays or None per axis): only these output indices are computed (a slab of a huge output)."""
    seg = np.asarray(seg)
    new_shape = tuple(int(v) for v in new_shape)
    if seg.shape == new_shape and select is None:
        return seg.copy()
    sep = -1 if sep_axis is None else int(sep_axis)
    tabs = [axis_taps(seg.shape[a], new_shape[a], a != sep) for a in range(3)]
    if select is not None:
        tabs = [t if s is None else tuple(v[np.asarray(s)] for v in t) for t, s in zip(tabs, select)]
        new_shape = tuple(len(t[0]) for t in tabs)
    labels, weights = [], []
    for taps in itertools.product(range(2), repeat=3):
        ii = [tabs[a][taps[a]] for a in range(3)]
        labels.append(seg[np.ix_(*ii)])
        w = np.ones(new_shape)
        for a in range(3):
            sh = [1, 1, 1]
            sh[a] = -1
            w = w * tabs[a][2 + taps[a]].reshape(sh)
        weights.append(w)
    best = np.zeros(new_shape, dtype=np.int64)
    for t in range(8):
        s = np.zeros(new_shape)
        for u in range(8):
            s = s + np.where(labels[u] == labels[t], weights[u], 0.0)
        best = np.maximum(best, np.where(s >= 0.5, labels[t].astype(np.int64), 0))
    return best.astype(seg.dtype)


def resample_xyz(seg_xyz, out_shape_xyz, sep_axis=None, fn=resample_seg_loop):
    """`fn` for an (x, y, z) array and an (x, y, z) target shape; sep_axis in the reference's [z, x, y] numbering."""
    o = [int(v) for v in out_shape_xyz]
    return from_ref(fn(to_ref(seg_xyz), (o[2], o[0], o[1]), sep_axis))
