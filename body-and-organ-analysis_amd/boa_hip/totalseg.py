"""`total` task (TS/python_api.py:totalsegmentator task table :168-189) on the generic task driver (task.py).

Per CT: canonicalise -> resample to 1.5 mm (identity at 1.5 mm, TS/resampling.py:179-181) -> for each part model
291..295: crop_to_nonzero, CTNormalization, sliding window (step 0.8, TS/nnunet.py:507-514), fp16 Gaussian accumulation,
normalise + argmax + `seg_combined[seg == jdx] = class_map_inv[name]` merge on device (TS/nnunet.py:553-556) -> restore.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

from .device import Context
from .plans import ModelConfig
from .task import SegmentationTask, nonzero_bbox, rough_crop_mask  # noqa: F401  (nonzero_bbox re-exported)

TOTAL_TASK = {"task_id": [291, 292, 293, 294, 295], "resample": 1.5, "trainer": "nnUNetTrainerNoMirroring",
              "model": "3d_fullres", "folds": [0], "step_size": 0.8}          # TS/python_api.py:183-189
TOTAL_FAST_TASK = {"task_id": [297], "resample": 3.0, "trainer": "nnUNetTrainer_4000epochs_NoMirroring",
                   "model": "3d_fullres", "folds": [0], "step_size": 0.5}     # TS/python_api.py:169-176


class TotalSegmentatorHip(SegmentationTask):
    """Holds one HipPredictor per part model; `predict(ct_xyz, spacing)` returns the merged `total` label volume."""

    def __init__(self, ctx: Context, models: Sequence[Tuple[int, ModelConfig, Sequence[np.ndarray]]],
                 step_size: float = 0.8, max_batch: int = 16, resample: float = 1.5, precision=None):
        super().__init__(ctx, "total", models, resample=resample, multimodel=True, max_batch=max_batch, precision=precision)
        if abs(step_size - self.step_size) > 1e-12:   # explicit override (the reference derives it, TS/nnunet.py:507-514)
            self.step_size = float(step_size)
            for _, _, p, _ in self.parts:
                p.tile_step_size = float(step_size)

    def predict(self, ct_xyz: np.ndarray, spacing_xyz=(1.5, 1.5, 1.5), affine=None, force_split: bool = False,
                roi_subset=None, roi_subset_robust=None, rough_models=None, remove_small_blobs: bool = False,
                statistics: bool = False, statistics_exclude_masks_at_border: bool = True, stats_aggregation: str = "mean",
                statistics_normalized_intensities: bool = False, higher_order_resampling: bool = False):
        """(x,y,z) CT in RAS+ order with `spacing_xyz` (or any axis order with an explicit `affine`) -> the `total` label volume.

        The TotalSegmentator keywords of `compute_all_models` (TS/python_api.py:636-664,778-796):
        `roi_subset` / `roi_subset_robust` (a list of structure names): `rough_models` -- the single rough `total` model, Dataset298
        at 6 mm, for `roi_subset_robust` Dataset297 at 3 mm, as `model_store.load_task_models` gives it -- makes the crop mask, only
        the parts that hold the names run on the crop (+ 20 mm), only their labels are kept; `statistics`: returns
        (labels, get_basic_statistics dict of the labels and the CT on the input grid) instead of the labels;
        `higher_order_resampling`: the labels go back to the input grid by nnU-Net's one-hot order-1 resampling instead of nearest
        neighbour (`SegmentationTask.predict_image`; the rough model of `roi_subset` keeps nearest)."""
        from . import label_maps, orientation
        if affine is None:
            affine = np.diag([float(spacing_xyz[0]), float(spacing_xyz[1]), float(spacing_xyz[2]), 1.0])
        robust = roi_subset_robust is not None
        if robust:
            roi_subset = roi_subset_robust
        if roi_subset is None:
            seg = self.predict_image(ct_xyz, affine, force_split=force_split, remove_small_blobs=remove_small_blobs,
                                     higher_order_resampling=higher_order_resampling)
        else:
            if type(roi_subset) is not list:
                raise ValueError("roi_subset must be a list of strings")
            if rough_models is None:
                raise ValueError("roi_subset needs the rough `total` model: rough_models=model_store.load_task_models('total_6mm')")
            label_maps.parts_for_roi_subset(roi_subset)      # (validates the names before the rough model runs)
            crop_mask = rough_crop_mask(self.ctx, ct_xyz, affine, rough_models, roi_subset, 3.0 if robust else 6.0)
            # (the parts that do not hold the names stay loaded, they just do not run)
            seg = self.predict_roi_subset(ct_xyz, affine, crop_mask, roi_subset, force_split=force_split, remove_small_blobs=remove_small_blobs,
                                          higher_order_resampling=higher_order_resampling)
        if not statistics:
            return seg
        from . import statistics as st
        zooms = np.asarray(orientation.zooms_from_affine(np.asarray(affine, dtype=np.float64)), dtype=np.float32)
        return seg, st.basic_statistics(self.ctx, seg, ct_xyz, zooms, task="total",
                                        exclude_masks_at_border=statistics_exclude_masks_at_border, roi_subset=roi_subset,
                                        metric=stats_aggregation, normalized_intensities=statistics_normalized_intensities)
