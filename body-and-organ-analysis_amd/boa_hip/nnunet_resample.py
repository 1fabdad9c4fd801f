"""nnU-Net's own resampling between the image grid and the plans' spacing, host side (the decisions; the arithmetic is
`boa_resize_skimage_f32` / `boa_resize_logits_argmax` in libboa_hip.so):

  compute_new_shape / get_do_separate_z / get_lowres_axis / determine_do_sep_z_and_axis
        NN/preprocessing/resampling/default_resampling.py:13-62 (ANISO_THRESHOLD = 3, NN/configuration.py:7)
  data_plan(...)     NN/preprocessing/preprocessors/default_preprocessor.py:71-93: the image (already cropped to its
                     nonzero box and normalised) goes to the plans' spacing with `resampling_fn_data` (order 3, order_z 0)
  logits_plan(...)   NN/inference/export_prediction.py:25-33: the logits go back to the pre-resampling shape with
                     `resampling_fn_probabilities` (order 1, order_z 0) before the argmax

Only the kwargs every nnU-Net v2 planner writes (and the BOA / TotalSegmentator models ship) are implemented:
resample_data_or_seg_to_shape with is_seg False, order 3 (data) / 1 (probabilities), order_z 0; `force_separate_z` may be
None, True or False.  Anything else raises instead of silently resampling differently.

  onehot_plan(...)   TotalSegmentator's `higher_order_resampling`: change_spacing(..., target_shape, order=1, nnunet_resample=True)
                     -> resample_img_nnunet -> resample_patient (TS/resampling.py:79-126,157-205, TS/resample_nnunet.py:46-116) of
                     the model-grid labels; the arithmetic is `boa_resample_onehot_u8`"""
from __future__ import annotations

import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np

ANISO_THRESHOLD = 3
_FN = "resample_data_or_seg_to_shape"
DEFAULT_KW = {"data": {"is_seg": False, "order": 3, "order_z": 0, "force_separate_z": None},
              "probabilities": {"is_seg": False, "order": 1, "order_z": 0, "force_separate_z": None}}


def compute_new_shape(old_shape: Sequence[int], old_spacing: Sequence[float], new_spacing: Sequence[float]) -> List[int]:
    assert len(old_spacing) == len(old_shape) == len(new_spacing)
    return [int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)]


def get_do_separate_z(spacing, anisotropy_threshold=ANISO_THRESHOLD) -> bool:
    return bool((np.max(spacing) / np.min(spacing)) > anisotropy_threshold)


def get_lowres_axis(new_spacing) -> np.ndarray:
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


def determine_do_sep_z_and_axis(force_separate_z, current_spacing, new_spacing,
                                separate_z_anisotropy_threshold=ANISO_THRESHOLD) -> Tuple[bool, Optional[int]]:
    if force_separate_z is not None:
        do_separate_z = bool(force_separate_z)
        axis = get_lowres_axis(current_spacing) if force_separate_z else None
    elif get_do_separate_z(current_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(current_spacing)
    elif get_do_separate_z(new_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(new_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None:
        if len(axis) in (2, 3):     # e.g. (0.24, 1.25, 1.25): no separate treatment of the out-of-plane axis
            do_separate_z, axis = False, None
        else:
            axis = int(axis[0])
    return do_separate_z, axis


def checked_kwargs(cfg_extra: dict, which: str) -> dict:
    """The plans' `resampling_fn_<which>` + kwargs (`which`: data | probabilities), validated against what the device does."""
    fn = cfg_extra.get(f"resampling_fn_{which}", _FN)
    kw = dict(DEFAULT_KW[which])
    kw.update(cfg_extra.get(f"resampling_fn_{which}_kwargs") or {})
    want = DEFAULT_KW[which]
    if fn != _FN or kw["is_seg"] or kw["order"] != want["order"] or kw["order_z"] != 0:
        raise NotImplementedError(f"resampling_fn_{which} = {fn}({kw}) is not implemented on the device "
                                  f"(supported: {_FN} with is_seg False, order {want['order']}, order_z 0)")
    return kw


def slice_axis_for(kw: dict, current_spacing, new_spacing) -> int:
    """-1: one 3-D resize; else the axis that is resampled separately (per-slice 2-D resize + nearest along it)."""
    sep, axis = determine_do_sep_z_and_axis(kw["force_separate_z"], current_spacing, new_spacing)
    return axis if sep else -1


def onehot_plan(old_shape: Sequence[int], target_shape: Sequence[int], img_spacing) -> Tuple[bool, Optional[int], Tuple[int, ...]]:
    """The decisions of change_spacing(img, target_shape=..., nnunet_resample=True) for a label image of `old_shape` (x, y, z) whose
    header zooms are `img_spacing` (float32, as header.get_zooms() gives them): -> (do_separate_z, axis, new_shape), axis and
    new_shape in the reference's [z, x, y] order (TS/resampling.py:105-116), axis None unless do_separate_z.

    zoom = target_shape / old_shape, new_spacing = img_spacing / zoom (TS/resampling.py:171-175, dtypes as there: float32 zooms,
    float64 target spacing); resample_patient(force_separate_z=None): separate z when max / min > 3 on the original spacing, else
    on the target spacing; the coarse axis from get_lowres_axis, three equal axes -> axis 0, two equal axes -> separate z off with
    the reference's warning; new_shape = round(original / target * shape) must be the target shape (the reference would fail its
    shape check after the resampling), else ValueError."""
    old = np.array([int(v) for v in old_shape])
    img_spacing = np.array(img_spacing, dtype=np.float32)
    zoom = np.array([int(v) for v in target_shape]) / old
    new_spacing = img_spacing / zoom
    front = lambda l: np.array([l[2], l[0], l[1]])                   # noqa: E731  (move_last_elem_to_front)
    original_spacing, target_spacing, shape = front(img_spacing), front(new_spacing), front(old)
    new_shape = np.round((np.array(original_spacing) / np.array(target_spacing)).astype(float) * shape).astype(int)
    if get_do_separate_z(original_spacing):
        do_separate_z, axis = True, get_lowres_axis(original_spacing)
    elif get_do_separate_z(target_spacing):
        do_separate_z, axis = True, get_lowres_axis(target_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None:
        if len(axis) == 3:
            axis = (0,)
        elif len(axis) == 2:
            warnings.warn(f"axis has len 2, axis: {axis}, spacing: {original_spacing}, target_spacing: {target_spacing}: "
                          "no separate resampling of the coarse axis")
            do_separate_z = False
    want = tuple(int(v) for v in front([int(v) for v in target_shape]))
    got = tuple(int(v) for v in new_shape)
    if got != want:
        raise ValueError(f"higher_order_resampling: the reference's new_shape {got} is not the target shape {want} "
                         f"(spacing {img_spacing}, shape {tuple(old)})")
    return bool(do_separate_z), (int(axis[0]) if do_separate_z else None), got
