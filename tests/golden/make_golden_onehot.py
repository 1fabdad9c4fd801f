#!/usr/bin/env python3
"""Generate tests/golden/g_onehot_*.npz by EXECUTING THE REFERENCE's own label resampling of `higher_order_resampling`:
TS/resampling.py `resample_img_nnunet(None, seg, img_spacing, new_spacing, order_data=1, order_seg=1)` (what
`change_spacing(..., target_shape, order=1, nnunet_resample=True)` calls, :171-175,203-205) -> TS/resample_nnunet.py
`resample_patient(None, seg, ...)` -> `resample_data_or_seg(is_seg=True)` -> `resize_segmentation`.

`skimage.transform.resize` is absent from the dev container: it is replaced, as for G13 of make_golden.py, by the oracle's
restatement of its published algorithm (oracle/nnunet_resample.py `skimage_resize`).  The fixtures pin everything around it: the
spacing arithmetic and its dtypes, the axis choice, the two-equal-axes fallback, the per-slice loop, the nearest sampling along
the coarse axis, the label order and the `>= 0.5` rule -- NOT skimage.

Runs only in the dev container (needs the reference checkout); the outputs are committed and are all the tests read.

    python tests/golden/make_golden_onehot.py
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_harness as H  # noqa: E402

H.install()
warnings.simplefilter("ignore", DeprecationWarning)

# (name, shape (x, y, z), target shape (x, y, z), header zooms, label palette, blocky)
CASES = [
    ("iso_x2", (9, 7, 5), (18, 14, 10), (3.0, 3.0, 3.0), (0, 1, 2, 3), True),                  # exact ties at 0.5
    ("nondyadic", (11, 13, 6), (23, 20, 17), (1.5, 1.5, 1.5), (0, 1, 127, 255), True),
    ("down", (20, 18, 16), (7, 9, 5), (1.0, 1.0, 1.0), (0, 5, 6, 7, 90), True),
    ("noise", (7, 6, 8), (15, 11, 19), (1.5, 1.5, 1.5), tuple(range(0, 256, 5)), False),       # 8 labels in most cells
    ("sepz_target_ax0", (12, 10, 8), (24, 20, 4), (1.5, 1.5, 1.5), (0, 1, 2, 117), True),      # target (0.75, 0.75, 3): z coarse
    ("sepz_target_ax1", (8, 10, 12), (3, 20, 24), (1.5, 1.5, 1.5), (0, 1, 2, 117), True),      # x coarse, extent 8 -> 3
    ("sepz_target_ax2", (6, 8, 5), (20, 8, 17), (1.5, 1.5, 1.5), (0, 3, 4, 200), True),        # y coarse, extent unchanged
    ("sepz_original", (10, 9, 4), (13, 11, 6), (1.0, 1.0, 4.0), (0, 9, 10, 11), True),          # decided on the original spacing
    ("two_equal_axes", (8, 8, 6), (4, 4, 24), (1.5, 1.5, 1.5), (0, 1, 2, 3), True),            # target (3, 3, 0.375): fallback
]


def labels(rng, shape, palette, blocky):
    pal = np.array(palette, dtype=np.uint8)
    if not blocky:
        return pal[rng.integers(0, len(pal), size=shape)]
    coarse = rng.integers(0, len(pal), size=tuple((s + 2) // 3 for s in shape))
    a = np.kron(coarse, np.ones((3, 3, 3), dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
    flip = rng.random(shape) < 0.1                                   # single-voxel specks on the blocks
    a[flip] = rng.integers(0, len(pal), size=int(flip.sum()))
    return pal[a]


def main():
    from oracle.nnunet_resample import skimage_resize
    import totalsegmentator.resample_nnunet as rn
    from totalsegmentator.resampling import resample_img_nnunet

    def resize(image, output_shape, order=None, mode="reflect", cval=0, clip=True, anti_aliasing=None, **kw):
        assert mode == "edge" and anti_aliasing is False and clip is True and not kw, (mode, anti_aliasing, clip, kw)
        return skimage_resize(image, output_shape, order)
    rn.resize = resize

    seen = {}
    inner = rn.resample_data_or_seg

    def spy(data, new_shape, is_seg, axis=None, order=3, do_separate_z=False, cval=0, order_z=0):
        seen.update(new_shape=[int(v) for v in new_shape], do_separate_z=bool(do_separate_z), order=order, order_z=order_z,
                    axis=-1 if (axis is None or not do_separate_z) else int(axis[0]), is_seg=is_seg)
        return inner(data, new_shape, is_seg, axis, order, do_separate_z, cval=cval, order_z=order_z)
    rn.resample_data_or_seg = spy

    rng = np.random.default_rng(2024)
    for name, shape, target, zooms, palette, blocky in CASES:
        seg = labels(rng, shape, palette, blocky)
        # change_spacing (TS/resampling.py:157-175,203-217) around the call, with its dtypes
        data = seg.astype(np.float64)                               # img_in.get_fdata()
        img_spacing = np.array(tuple(np.float32(z) for z in zooms))  # header.get_zooms(): float32
        zoom = np.array(target) / np.array(data.shape)
        new_spacing = img_spacing / zoom
        assert not np.array_equal(img_spacing, new_spacing)
        seen.clear()
        _, new = resample_img_nnunet(None, data, img_spacing, new_spacing, order_data=1, order_seg=1)
        out = new.astype(np.uint8)
        assert seen["is_seg"] and seen["order"] == 1 and seen["order_z"] == 0 and out.shape == tuple(target), (name, seen, out.shape)
        path = os.path.join(HERE, f"g_onehot_{name}.npz")
        np.savez_compressed(path, seg=seg, out=out, zooms=img_spacing, target=np.array(target),
                            do_separate_z=np.array(seen["do_separate_z"]), axis=np.array(seen["axis"]),
                            new_shape=np.array(seen["new_shape"]))
        print("wrote", os.path.basename(path), shape, "->", target, "sep", seen["do_separate_z"], "axis", seen["axis"],
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
