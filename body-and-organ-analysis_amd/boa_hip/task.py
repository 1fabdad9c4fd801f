"""One segmentation task end to end (host side of SURVEY 8 a10-a13): the array-level equivalent of
TS/nnunet.py:nnUNet_predict_image (:326-829) + nnUNetPredictor.predict_from_files for one CT.

    crop to mask (opt., TS/cropping.py:75-110) -> as_closest_canonical (TS/alignment.py:8-12)
    -> [resample_only_thickness: (sx, sy, resample)] change_spacing order 3 -> int32 (TS/nnunet.py:457-474, device)
    -> triple z-split if > 512*512*900 voxels and z > 200 and multi-model, or force_split (:489-505)
    -> per sub-volume and per model: (x,y,z) -> (z,y,x) float32 (nibabel reader), crop_to_nonzero
       (NN/preprocessing/cropping/cropping.py:19-39), CTNormalization, sliding window (step 0.8 for `total` below 3 mm,
       else 0.5, :507-514), fold mean, argmax, part -> global remap (:553-556)       -- all on the device
    -> recombine the thirds (:580-587) -> change_spacing order 0 back to the input grid (:685-687, device)
    -> undo_canonical (:691) -> undo_crop (:695) -> uint8 labels on the input grid.

Axis permutes / flips / crops are index remaps done with device views; every per-voxel computation runs in
libboa_hip.so.  nnU-Net's own resampling to the plans' spacing (default_preprocessor.py:82-93) and of the logits back
(export_prediction.py:25-33) happens per model inside `predict_zyx_device` whenever the array's spacing differs from the
model's plans (`boa_hip/nnunet_resample.py`); it is the identity at every BASELINE.json config (`total` is resampled to
1.5 mm = plans spacing) and active for real-world BCA / cascade inputs whose in-plane spacing differs from the plans'.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import label_maps, orientation
from . import nnunet_resample as nr
from . import resample as rs
from ._lib import check, int3
from .devarray import DevArray
from .device import Context, Scope, Workspace
from .plans import ModelConfig
from .predictor import HipPredictor

NR_VOXELS_THR = 512 * 512 * 900  # TS/nnunet.py:484
SPLIT_MARGIN = 20                # TS/nnunet.py:497


def get_bbox_from_mask(mask: np.ndarray, outside_value=0, addon=0) -> List[List[int]]:
    """TS/cropping.py:11-38."""
    addon = [addon] * 3 if isinstance(addon, (int, np.integer)) else [int(a) for a in addon]
    sel = mask > outside_value
    if sel.sum() == 0:
        return [[0, mask.shape[0]], [0, mask.shape[1]], [0, mask.shape[2]]]
    bbox = []
    for ax in range(3):
        idx = np.flatnonzero(sel.any(axis=tuple(a for a in range(3) if a != ax)))
        bbox.append([max(0, int(idx[0]) - addon[ax]), min(mask.shape[ax], int(idx[-1]) + 1 + addon[ax])])
    return bbox


def nonzero_bbox(data_zyx: np.ndarray) -> List[List[int]]:
    """Bounding box of data != 0 (binary_fill_holes cannot change it), cropping.py:6-29."""
    bbox = []
    for ax in range(3):
        other = tuple(a for a in range(3) if a != ax)
        nz = np.flatnonzero((data_zyx != 0).any(axis=other))
        bbox.append([0, data_zyx.shape[ax]] if nz.size == 0 else [int(nz[0]), int(nz[-1]) + 1])
    return bbox


def split_bounds(nz: int) -> Tuple[List[Tuple[int, int]], List[Tuple[slice, slice]]]:
    """Triple split along z (TS/nnunet.py:495-505) and its recombination (:583-586):
    returns [(lo, hi) of each part], [(destination slice, source slice within the part)]."""
    third, m = nz // 3, SPLIT_MARGIN
    parts = [(0, third + m), (third + 1 - m, third * 2 + m), (third * 2 + 1 - m, nz)]
    comb = [(slice(0, third), slice(None, -m)), (slice(third, third * 2), slice(m - 1, -m)),
            (slice(third * 2, nz), slice(m - 1, None))]
    return parts, comb


class _WayBack(NamedTuple):
    """What `SegmentationTask._to_model_grid` did to the input, for `_to_input_grid` to undo."""
    bbox: Optional[list]              # crop to the mask, on the input array (None: no crop)
    cropped_affine: np.ndarray        # of the cropped input: its orientation is what undo_canonical restores
    thick_ornt: Optional[np.ndarray]  # the `resample_only_thickness` reorientation RAS -> axcodes (None: none)
    in_shape: tuple                   # before change_spacing
    zoom: Optional[np.ndarray]        # of change_spacing (None: the spacing did not change)
    ss: tuple                         # after it: the model grid
    orig_shape: tuple                 # of the input array
    cast: Optional[type]              # dtype of crop_to_mask (None: no crop)


class SegmentationTask(contextlib.AbstractContextManager):
    """`models`: [(task_id, ModelConfig, [weight blob per fold])]; several entries = multi-model task (`total`)
    whose part label maps are merged into the global map (later parts overwrite).  `with SegmentationTask(...) as t:` closes it."""

    def __init__(self, ctx: Context, task_name: str, models: Sequence[Tuple[int, ModelConfig, Sequence[np.ndarray]]],
                 resample: Optional[float] = None, resample_only_thickness: bool = False, multimodel: Optional[bool] = None,
                 max_batch: int = 16, part_luts: Optional[Dict[int, np.ndarray]] = None, precision: Optional[str] = None):
        self.ctx = ctx
        self.task_name = task_name
        self.resample = None if resample is None else float(resample)
        self.resample_only_thickness = bool(resample_only_thickness)
        # {key: DeviceBuffer} shared between tasks that resample the SAME resident volume to the same grid (the two BCA
        # nets both take the CT to (sx, sy, 5 mm)): the owner of the dict frees the buffers.  None = resample every time.
        self.resample_cache: Optional[dict] = None
        self.multimodel = (len(models) > 1) if multimodel is None else bool(multimodel)
        # TS/nnunet.py:507-514
        self.step_size = 0.8 if (task_name == "total" and self.resample is not None and self.resample < 3.0) else 0.5
        self.parts = []
        for task_id, cfg, blobs in models:
            if cfg.normalization_schemes[0] != "CTNormalization":
                raise ValueError(f"Dataset{task_id}: only CTNormalization is supported on device")
            tf, tb = [int(v) for v in cfg.transpose_forward], [int(v) for v in cfg.transpose_backward]
            if sorted(tf) != [0, 1, 2] or [tf[i] for i in tb] != [0, 1, 2]:
                raise ValueError(f"Dataset{task_id}: transpose_forward {tf} / transpose_backward {tb} are not inverse permutations")
            if self.parts and tf != [int(v) for v in self.parts[0][1].transpose_forward]:
                raise NotImplementedError("models of one task with different transpose_forward")
            p = HipPredictor(ctx, cfg.geometry, tile_step_size=self.step_size, max_batch=max_batch, precision=precision)
            p.set_parameters(list(blobs))
            if self.multimodel:
                lut = part_luts[task_id] if part_luts is not None else label_maps.part_lut(task_id)
            else:
                lut = None
            self.parts.append((task_id, cfg, p, lut))
        # the task's persistent device scratch and its FlagRing: reused across volumes and models, handed to the predictors as `work=`
        self._work = Workspace(ctx, ring=True)
        # tile_shard.TileShard: several ranks share every volume (tile rows split, overlap slabs exchanged); each rank
        # must be given the same input and ends with the same labels.  None = this process handles whole volumes.
        self.shard = None
        # tile_shard.ShardComm: the part models of a multi-model task are dealt out to the ranks (model k -> rank k mod
        # world, SURVEY 8e granularity 2); every rank must be given the same input and ends with the same labels.  Each
        # model runs exactly as on one GPU (same tiles, same batches), so the result is bit-identical to the one-GPU run.
        self.model_shard = None

    def close(self):
        for _, _, p, _ in self.parts:
            p.close()
        self._work.free()

    def __exit__(self, *exc):
        self.close()

    # ---- device core: resident CT [z,y,x] -> resident uint8 labels -----------------------------------------
    def predict_zyx_device(self, d_ct, shape, d_labels, in_dtype: int = 0, spacing_zyx=None, only=None):
        """in_dtype 0 int16 / 1 float32 / 2 int32.  Labels are zeroed here, then every model -- with `only` (task ids; `roi_subset`, not
        for the sharded modes) every model it lists -- writes (merges) into them.
        `spacing_zyx`: voxel spacing of the array (nnU-Net axis order); when it differs from a model's plans spacing the
        normalised volume is resampled to the plans' grid and the logits back (nnU-Net's own resampling,
        default_preprocessor.py:82-93 / export_prediction.py:25-33) -- None = the array is at the plans' spacing."""
        n = int(np.prod(shape))
        self._work.buf("vol", n * 4)      # (every model normalises into it; allocated before the ring, once per task)
        d_labels.zero()
        # The predictors of this task take their inf-flag slots from the ring of `self._work` (Workspace.flag), so EVERY
        # path below owns it: reset before the first model, one read after the last (a path that skipped the check would drop the
        # reference's "Encountered inf in predicted array" error and let unchecked slots pile up -- ADVICE r5).
        ring = self._work.ring
        ring.reset()
        if self.model_shard is not None and self.model_shard.world > 1 and self.multimodel:
            self._predict_zyx_model_sharded(d_ct, shape, d_labels, in_dtype, n, spacing_zyx)
        elif self.shard is not None and self.shard.comm.world > 1 and self.multimodel and len(self.parts) > 1 and self._units_applicable(shape, spacing_zyx):
            self._predict_zyx_unit_sharded(d_ct, shape, d_labels, in_dtype, n)
        else:
            for k in range(len(self.parts)):
                if only is None or self.parts[k][0] in only:
                    self._run_model(k, d_ct, shape, d_labels, in_dtype, n, spacing_zyx, merge=self.multimodel, shard=self.shard)
        ring.check()   # the models' inf flags of this rank, one read per volume

    # ---- (row x model) units: all ranks busy on one multi-model volume ---------------------------------------------------------
    def _units_applicable(self, shape, spacing_zyx) -> bool:
        """Every model runs on the array as it is (no plan-spacing resampling: that path all-reduces whole logit volumes)."""
        if spacing_zyx is None:
            return True
        return all(nr.compute_new_shape(shape, spacing_zyx, cfg.spacing) == list(shape) for _, cfg, _, _ in self.parts)

    def _predict_zyx_unit_sharded(self, d_ct, shape, d_labels, in_dtype, n):
        """The part models of a multi-model task are independent until the label merge (TS/nnunet.py:542-556), so the work units of a
        shared volume are (model, tile row) pairs: tile_shard.plan_units cuts the model-major unit list into one contiguous run
        per rank (512^3 `total`: 5 x 5 units -> 3-4 per rank on 8 GPUs, where tile rows alone keep 5 busy).  A model's rows then
        live on a subset of the ranks, which exchange that model's overlap slabs; every rank takes part in the label all-reduce.
        The models are software-pipelined: model k + 1's tiles are queued before model k's exchange is waited for, every model
        with its own normalised copy of the CT (the models have different intensity properties).  Labels are bit-identical to
        the one-GPU run in `exact` mode: per model the accumulation order is the reference's, the merge order is the part order."""
        import dataclasses
        from . import sliding_window as sw
        world = self.shard.comm.world
        rows, weights = [], []
        for _, cfg, p, _ in self.parts:
            PV, _b = sw.pad_amounts(list(shape), p.geom.patch_size)
            o = sw.get_sliding_window_origins(PV, p.geom.patch_size, p.tile_step_size)
            r = len(set(int(v) for v in o[:, 0]))
            rows.append(r)
            weights.append(len(o) / r)
        from .tile_shard import plan_units
        units = plan_units(rows, world, weights)
        prev = None
        for k in range(len(self.parts)):
            task_id, cfg, p, lut = self.parts[k]
            vol = self._normalized(cfg, d_ct, in_dtype, n, name=f"vol{k & 1}")
            shard_k = dataclasses.replace(self.shard, assignment=units[k])
            job = p.begin_segmentation_sharded(vol, list(shape), d_labels, lut, True, self._work, shard_k,
                                               after_first_start=(prev.finish if prev is not None else None))
            prev = job
        if prev is not None:
            prev.finish()

    def _normalized(self, cfg, d_ct, in_dtype: int, n: int, name: str = "vol"):
        """CTNormalization with the model's own intensity properties (default_preprocessor.py:336-348) of the `n` voxels at `d_ct`
        into the workspace buffer `name` (fp32), which is returned."""
        ctx = self.ctx
        vol = self._work.buf(name, n * 4)
        ip = cfg.intensity_properties["0"]
        check(ctx.lib.boa_ct_normalize(ctx.h, d_ct.vp, in_dtype, vol.vp, n, ip["mean"], ip["std"],
                                       ip["percentile_00_5"], ip["percentile_99_5"]), "boa_ct_normalize")
        return vol

    @contextlib.contextmanager
    def _at_plan_spacing(self, cfg, vol, shape, spacing):
        """nnU-Net's resampling to the plans' spacing (default_preprocessor.py:82-93) of the normalised `vol` (`spacing`: the array's,
        None = the plans'): yields (volume, shape, resample_to) for the predictor -- `vol` itself and None when the shape does not
        change, else a temporary at the plans' grid, freed on exit, and `resample_to` = (shape, slice axis) for the way back."""
        ctx, shape = self.ctx, [int(v) for v in shape]
        new_shape = shape if spacing is None else nr.compute_new_shape(shape, spacing, cfg.spacing)
        if new_shape == shape:      # resample_data_or_seg returns its input unchanged (default_resampling.py:194-196)
            yield vol, shape, None
            return
        # normalise BEFORE resampling (default_preprocessor.py:82-84), order 3 in; order 1 back, then argmax
        ax_in = nr.slice_axis_for(nr.checked_kwargs(cfg.extra, "data"), spacing, cfg.spacing)
        ax_out = nr.slice_axis_for(nr.checked_kwargs(cfg.extra, "probabilities"), cfg.spacing, spacing)
        vol_r = ctx.alloc(int(np.prod(new_shape)) * 4)
        try:
            check(ctx.lib.boa_resize_skimage_f32(ctx.h, vol.vp, int3(shape), vol_r.vp, int3(new_shape), 3, ax_in),
                  "boa_resize_skimage_f32")
            yield vol_r, new_shape, (shape, ax_out)
        finally:
            vol_r.free()

    def _run_model(self, k, d_ct, shape, d_out, in_dtype, n, spacing_zyx, merge, shard):
        """One model of the task on the resident array: CTNormalization, nnU-Net's resampling to the plans' spacing when it differs
        from the array's, sliding window, labels written (merge=False) or merged (merge=True) into `d_out`."""
        task_id, cfg, p, lut = self.parts[k]
        vol = self._normalized(cfg, d_ct, in_dtype, n)
        with self._at_plan_spacing(cfg, vol, shape, spacing_zyx) as (v, v_shape, resample_to):
            p.predict_segmentation_device(v, v_shape, d_out, lut=lut, merge=merge, work=self._work, shard=shard, resample_to=resample_to)

    def _predict_zyx_model_sharded(self, d_ct, shape, d_labels, in_dtype, n, spacing_zyx=None):
        from . import tile_shard as ts
        ctx, comm = self.ctx, self.model_shard
        part = self._work.buf("model_part", n)
        for k in range(len(self.parts)):
            check(ctx.lib.boa_memset(ctx.h, part.vp, 0, n), "boa_memset")
            if k % comm.world == comm.rank:   # exactly the one-GPU computation of this model (incl. its plan-spacing resampling)
                self._run_model(k, d_ct, shape, part, in_dtype, n, spacing_zyx, merge=False, shard=None)
            # the owner's label volume reaches every rank (sum over disjoint supports), then the reference's merge in part
            # order: `seg_combined[seg == jdx] = class_map_inv[name]` (TS/nnunet.py:553-556)
            ts.all_reduce_labels(ctx, comm, part, n)
            check(ctx.lib.boa_label_overlay(ctx.h, part.vp, n, d_labels.vp), "boa_label_overlay")

    # ---- one (sub-)volume, device resident ----------------------------------------------------------------------
    def _predict_part_device(self, part_xyz: DevArray, dst_xyz: DevArray, src_lo: int, src_hi: int, spacing_zyx=None,
                             save_probabilities=None, only=None):
        """`part_xyz`: (x,y,z) view of the (resampled) CT that TS would write to s0k_0000.nii.gz.  Its labels for the
        part-local z range [src_lo, src_hi) are written into `dst_xyz` (a zero-initialised (x,y,z) view of the same
        x/y extent and src_hi - src_lo slices).  nibabel reader view change, crop_to_nonzero and insert_crop_into_image
        (export_prediction.py:44-47) are views + one device copy each way.  `save_probabilities` (a path): every model's class
        probabilities on this part's (z, y, x) grid are written there and the labels are taken from them
        (`_predict_part_probabilities`).  `only`: as in `predict_zyx_device`."""
        dt = part_xyz.dtype
        want = dt if dt in (np.dtype(np.int16), np.dtype(np.int32)) else np.dtype(np.float32)
        code = {np.dtype(np.int16): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2}[want]
        # plans' transpose_forward (default_preprocessor.py:57-60: data.transpose([0, *[i + 1 for i in transpose_forward]]) before
        # cropping / resampling; export_prediction.py:56-58 transposes the segmentation back): a device view + one copy
        tf = [int(v) for v in self.parts[0][1].transpose_forward]
        ident = tf == [0, 1, 2]
        sp_t = None if spacing_zyx is None else [spacing_zyx[i] for i in tf]
        with Scope() as sc:
            def copy_of(a, src):      # a copy is released here; a view of `src` is its owner's
                return a if a.buf is src.buf else sc.own(a)
            zyx = copy_of(part_xyz.transpose((2, 1, 0)).contiguous(want, force_copy=False), part_xyz)
            work = zyx if ident else sc.own(zyx.transpose(tuple(tf)).contiguous(want, force_copy=True))
            bbox_t = work.nonzero_bbox()
            full = all(b == [0, n] for b, n in zip(bbox_t, work.shape))
            crop = work if full else copy_of(work.box(bbox_t).contiguous(), work)
            if save_probabilities is not None:
                # (the labels come back on the part's whole (z, y, x) grid: the crop box is already put back)
                lab_zyx = sc.own(self._predict_part_probabilities(crop, work.shape, bbox_t, code, spacing_zyx, sp_t, save_probabilities, only))
                bbox = [[0, int(v)] for v in lab_zyx.shape]
            else:
                d_lab = sc.own(DevArray.empty(self.ctx, crop.shape, np.uint8))
                self.predict_zyx_device(crop.buf, crop.shape, d_lab.buf, in_dtype=code, spacing_zyx=sp_t, only=only)
                # back to (z, y, x): axis i of the transposed array is axis tf[i] of the original
                bbox = [None, None, None]
                for i in range(3):
                    bbox[tf[i]] = bbox_t[i]
                lab_zyx = d_lab if ident else d_lab.transpose(tuple(int(v) for v in self.parts[0][1].transpose_backward))
            k0, k1 = max(bbox[0][0], src_lo), min(bbox[0][1], src_hi)
            if k0 < k1:
                src = lab_zyx.slice(0, k0 - bbox[0][0], k1 - bbox[0][0]).transpose((2, 1, 0))
                dst = dst_xyz.slice(2, k0 - src_lo, k1 - src_lo).slice(1, bbox[1][0], bbox[1][1]).slice(0, bbox[2][0], bbox[2][1])
                src.copy_to(dst)

    def _predict_part_probabilities(self, crop: DevArray, full_shape, bbox_t, in_dtype: int, spacing_zyx, sp_t, path, only=None) -> DevArray:
        """export_prediction_from_logits with save_probabilities (export_prediction.py:14-71, :99-102) for every model of the task
        on one part: `crop` is the transposed, nonzero-cropped array, `full_shape` its shape before the crop, `bbox_t` the crop box.
        Per model: the fold-mean logits -> `boa_logits_to_probabilities` (plan-spacing resampling reverted, the box put back into
        `full_shape` with background (1, 0, ..) around it, transpose_backward applied), the float32 [C, z, y, x] array written to
        `path` (np.savez_compressed, key `probabilities`) and the properties to `Path(path).with_suffix(".pkl")`; each model
        overwrites the files of the one before (TS/nnunet.py:286-293).  Returns the task's labels on the part's (z, y, x) grid --
        the first maximum of each model's probabilities, merged in part order for a multi-model task -- as a DevArray (caller frees)."""
        ctx = self.ctx
        shape = [int(v) for v in crop.shape]
        full = [int(v) for v in full_shape]
        n, n_full = int(np.prod(shape)), int(np.prod(full))
        tb = [int(v) for v in self.parts[0][1].transpose_backward]
        out_shape = [full[tb[i]] for i in range(3)]
        lo = [int(b[0]) for b in bbox_t]
        self._work.buf("vol", n * 4)
        ring = self._work.ring      # (owned here as in predict_zyx_device: reset before the first model, checked before a file is written)
        ring.reset()
        # what this engine knows of nnU-Net's properties_dict (plain types only: no nibabel / SimpleITK objects)
        props = {"spacing": None if spacing_zyx is None else [float(v) for v in spacing_zyx],
                 "shape_before_cropping": tuple(full), "bbox_used_for_cropping": [[int(a), int(b)] for a, b in bbox_t],
                 "shape_after_cropping_and_before_resampling": tuple(shape)}
        with Scope() as sc:
            labels = sc.own(DevArray.zeros(ctx, out_shape, np.uint8))
            part = sc.own(DevArray.empty(ctx, out_shape, np.uint8)) if self.multimodel else labels
            for task_id, cfg, p, lut in self.parts:
                if only is not None and task_id not in only:
                    continue
                nc = p.geom.num_classes
                prob = ctx.alloc(nc * n_full * 4)
                try:
                    vol = self._normalized(cfg, crop.buf, in_dtype, n)
                    with self._at_plan_spacing(cfg, vol, shape, sp_t) as (v, v_shape, resample_to):
                        p.predict_probabilities_device(v, v_shape, prob, part.buf, lut=lut, work=self._work, resample_to=resample_to,
                                                       bbox_lo=lo, full_dims=full, perm=tb)
                    if part is not labels:
                        check(ctx.lib.boa_label_overlay(ctx.h, part.buf.vp, n_full, labels.buf.vp), "boa_label_overlay")
                    ring.check()
                    write_probabilities(path, prob.download((nc, *out_shape), np.float32), props)
                finally:
                    prob.free()
            return sc.release(labels)

    @staticmethod
    def _supported(data: np.ndarray) -> np.ndarray:
        data = np.ascontiguousarray(data)
        if data.dtype in (np.uint8, np.int16, np.int32, np.float32, np.float64):
            return data
        return data.astype(np.float64)   # what get_fdata() hands to the reference

    def _postprocess_model_grid(self, seg: DevArray, zooms, remove_small: bool):
        """TS/nnunet.py:595-617 in place on the model-grid labels `seg` (contiguous (x, y, z), z fastest: the array order the
        reference's scipy.ndimage.label sees): ONE 6-connected labelling of all labels (boa_label_blobs6), then one filter call per
        reference step.  The steps only ever remove whole blobs, so the sizes of the first labelling hold for the later steps.
        Thresholds: mm^3 / voxel volume in float32 (`blobs.size_threshold_voxels`)."""
        from . import blobs
        cm = label_maps.class_map(self.task_name)
        lab = blobs.BlobLabelling(self.ctx, seg)
        try:
            if self.task_name == "body":
                lab.filter(blobs.modes_for(cm, ["body_trunc"], blobs.MODE_LARGEST))
                lo, hi = blobs.interval_bounds([blobs.size_threshold_voxels(50000, zooms), 1e10])
                lab.filter(blobs.modes_for(cm, ["body_extremities"], blobs.MODE_INTERVAL), lo, hi)
            if remove_small:
                lo, hi = blobs.interval_bounds([blobs.size_threshold_voxels(200, zooms), 1e10])
                lab.filter(blobs.modes_for(cm, list(cm.values()), blobs.MODE_INTERVAL), lo, hi)
        finally:
            lab.free()

    # ---- nnUNet_predict_image ------------------------------------------------------------------------------
    def predict_image(self, data, affine: np.ndarray, force_split: bool = False,
                      crop_mask: Optional[np.ndarray] = None, crop_addon=(3, 3, 3), axcodes: str = "RAS",
                      return_device: bool = False, save_probabilities=None, remove_small_blobs: bool = False,
                      model_grid_out: Optional[dict] = None, roi_subset: Optional[Sequence[str]] = None,
                      statistics_out: Optional[dict] = None, higher_order_resampling: bool = False):
        """CT array in file axis order + its affine -> uint8 label array on the same grid.  The volume is uploaded
        once; reorientation, crops, splits and restores are device views / copies, resampling and inference run on the
        device, only the final label volume comes back.  `data` may be a resident DevArray (not freed here);
        `return_device=True` returns the labels as a contiguous DevArray (caller frees) instead of downloading.

        `save_probabilities` (a path; nnUNet_predict_image(save_probabilities=...), TS/nnunet.py:335,550,572): every model run
        writes its softmax probabilities, float32 [C, z, y, x], with `np.savez_compressed(path, probabilities=...)` -- on the grid
        of the image handed to nnU-Net (TS-resampled, canonical; crop-to-nonzero and plan-spacing resampling reverted,
        transpose_backward applied) -- and a pickle next to it (`Path(path).with_suffix(".pkl")`) with the plain-dict subset of
        nnU-Net's properties_dict this engine knows: `spacing`, `shape_before_cropping`, `bbox_used_for_cropping`,
        `shape_after_cropping_and_before_resampling` (lists / tuples of numbers; no nibabel or SimpleITK objects).  As in the
        reference (TS/nnunet.py:286-293) each model OVERWRITES the file, so a multi-model task ends with its last model's
        array, and of a split image only part s01 is saved.  In this mode the labels are the first maximum of the saved
        probabilities; the label merge of `total` is unchanged.  The sharded modes raise NotImplementedError.

        Blob post-processing on the model grid (TS/nnunet.py:595-617), between the recombination of the parts and the nearest
        resample back (`_postprocess_model_grid`): task `body` always keeps the largest blob of `body_trunc` and drops the blobs
        of `body_extremities` of at most 50 000 mm^3; `remove_small_blobs=True` then drops, for every label of the task's class
        map, the blobs of at most 200 mm^3.  Not implemented for the sharded modes.  `model_grid_out` (a dict; test seam): gets
        `labels`, the model-grid label array (x, y, z) BEFORE that post-processing, and `zooms`, its float32 header zooms; with
        `statistics_out` also `labels_post`, the labels AFTER it, and `ct`, the model-grid image (the two arrays the statistics see).

        `roi_subset` (names of the task's class map; nnUNet_predict_image(roi_subset=...), TS/nnunet.py:388-390,519-531,707-709): of
        a multi-model `total` task only the part models whose class map holds one of the names run
        (`label_maps.parts_for_roi_subset`; a single-model task runs its one model), and on the input grid, after the restore, every
        label that is not one of them is cleared -- one look-up table pass on the device (`boa_label_apply_lut`).

        `statistics_out` (a dict; `statistics_fast` of TS/python_api.py:636-641, TS/nnunet.py:642-659): get_basic_statistics on the
        MODEL grid -- the resampled (and cropped) canonical image and the labels after the blob post-processing, before the resample
        back, header zooms those of that grid -- through `statistics.basic_statistics`; `statistics_out["params"]` (optional) holds
        its keyword arguments (exclude_masks_at_border, roi_subset, metric, normalized_intensities, file_out), the result goes to
        `statistics_out["stats"]`.  Neither is implemented for the sharded modes.

        `higher_order_resampling` (nnUNet_predict_image(nnunet_resampling=True), TS/nnunet.py:670-683): the model-grid labels go
        back to the input grid by nnU-Net's one-hot resampling instead of nearest neighbour -- every label's 0/1 mask resized with
        order 1, the label written where the result is >= 0.5, per slice with nearest along the coarse axis on anisotropic grids
        (`nnunet_resample.onehot_plan` decides as `resample_patient` does) -- in one device pass for all labels
        (`boa_resample_onehot_u8`).  With `roi_subset` the labels outside the subset are cleared on the model grid BEFORE the
        resampling as well (:671-674): they interpolate as background.  A task without `resample` is not resampled either way.
        Not implemented for the sharded modes."""
        if self.shard is not None or self.model_shard is not None:
            option = ("higher_order_resampling" if higher_order_resampling else
                      "roi_subset" if roi_subset is not None else "statistics" if statistics_out is not None else
                      "save_probabilities" if save_probabilities is not None else
                      "blob post-processing (remove_small_blobs, task body)" if (remove_small_blobs or self.task_name == "body") else None)
            if option is not None:
                raise NotImplementedError(f"{option} with a tile- or model-sharded task")
        keep_lut = only = None
        if roi_subset is not None:
            keep_lut = label_maps.subset_lut(roi_subset)
            if self.multimodel and self.task_name == "total":
                only = label_maps.parts_for_roi_subset(roi_subset)
        resident = isinstance(data, DevArray)
        if not resident:
            if data.ndim == 2:
                raise ValueError("TotalSegmentator does not work for 2D images. Use a 3D image.")
            if data.ndim > 3:
                data = data[:, :, :, 0]
            if data.dtype.fields is not None:
                raise TypeError(f"Invalid dtype {data.dtype}. Expected a simple dtype, not a structured one.")
        if crop_mask is not None and crop_mask.sum() == 0:              # TS/nnunet.py:428-446
            shape = tuple(int(v) for v in data.shape)
            return DevArray.zeros(self.ctx, shape, np.uint8) if return_device else np.zeros(shape, dtype=np.uint8)
        with Scope() as sc:                                            # device arrays to release
            img, spacing, back = self._to_model_grid(sc, data, affine, crop_mask, crop_addon, axcodes)
            seg = self._model_grid_labels(sc, img, spacing, force_split, save_probabilities, remove_small_blobs, model_grid_out,
                                          statistics_out, only)
            out = self._to_input_grid(sc, seg, back, axcodes, keep_lut, spacing if higher_order_resampling else None)
            if return_device:
                return sc.release(out.contiguous(force_copy=(resident and out.buf is data.buf)))
            return out.download()

    def _to_model_grid(self, sc: Scope, data, affine, crop_mask, crop_addon, axcodes):
        """Input grid -> model grid: crop to the mask, as_closest_canonical, the `resample_only_thickness` reorientation to
        `axcodes`, change_spacing (order 3, through `resample_cache` for a resident volume).  -> (the model-grid image, its spacing
        (x, y, z), the `_WayBack`).  Views of `data` stay its owner's, copies go to `sc`, a cached resample buffer is the cache's."""
        ctx, own = self.ctx, sc.own
        resident = isinstance(data, DevArray)
        orig_shape = tuple(int(v) for v in data.shape)
        affine = np.asarray(affine, dtype=np.float64)
        aff = affine
        bbox = None
        view = data if resident else own(DevArray.from_numpy(ctx, self._supported(data)))
        cast = None
        if crop_mask is not None:
            addon = (np.array(crop_addon) / orientation.zooms_from_affine(aff)).astype(int)   # mm -> voxels
            bbox = get_bbox_from_mask(crop_mask, outside_value=0, addon=addon)
            view = view.box(bbox)
            aff = aff.copy()
            aff[:3, 3] = np.dot(affine, np.array([bbox[0][0], bbox[1][0], bbox[2][0], 1]))[:3]
            cast = np.int32                                          # crop_to_mask(dtype=np.int32)
        cropped_affine = aff
        ornt = orientation.io_orientation(aff)                       # as_closest_canonical
        if not np.array_equal(ornt, orientation.RAS_ORNT):
            aff = aff.dot(orientation.inv_ornt_aff(ornt, view.shape))
            view = view.apply_orientation(ornt)
        resample = None if self.resample is None else [self.resample] * 3
        thick_ornt = None
        if self.resample_only_thickness:
            cur = "".join(orientation.aff2axcodes(aff))
            if cur != "".join(axcodes):
                thick_ornt = orientation.ornt_transform(orientation.axcodes2ornt(cur), orientation.axcodes2ornt(axcodes))
                aff = aff.dot(orientation.inv_ornt_aff(thick_ornt, view.shape))
                view = view.apply_orientation(thick_ornt)
            zooms = orientation.zooms_from_affine(aff)
            resample = [zooms[0], zooms[1], resample[0]]
        in_shape = view.shape
        zooms = orientation.zooms_from_affine(aff)
        zoom = None
        if resample is not None:                                     # change_spacing (TS/resampling.py:165-181)
            new_spacing = np.array(resample)
            zoom = zooms / new_spacing
            if np.array_equal(zooms, new_spacing):
                zoom = None
        if zoom is not None:
            out_shape = rs.zoomed_shape(in_shape, zoom)
            key = None
            if self.resample_cache is not None and resident:
                key = (data.buf.ptr, view.offset, view.shape, view.strides, str(view.dtype), str(cast), tuple(out_shape),
                       tuple(float(z) for z in zoom))   # (the cache lives for ONE resident volume: pipeline.run_resident)
            if key is not None and key in self.resample_cache:
                img_rsp = DevArray(ctx, self.resample_cache[key], out_shape, np.int32)      # (not owned: the cache's)
            else:
                src = view.contiguous(cast)
                if src.buf is not view.buf:
                    own(src)
                if src.dtype == np.uint8:
                    src = own(src.contiguous(np.int16, force_copy=True))
                buf = rs.resample_cubic_device(ctx, src.buf, src.dtype, src.shape, out_shape, np.int32)
                img_rsp = DevArray(ctx, buf, out_shape, np.int32)
                if key is not None:
                    self.resample_cache[key] = buf
                else:
                    own(img_rsp)
            sp_rsp = np.array(resample, dtype=np.float64)
        else:
            img_rsp = view if cast is None else own(view.contiguous(cast))
            sp_rsp = zooms
        return img_rsp, sp_rsp, _WayBack(bbox, cropped_affine, thick_ornt, in_shape, zoom, img_rsp.shape, orig_shape, cast)

    def _model_grid_labels(self, sc: Scope, img_rsp: DevArray, sp_rsp, force_split, save_probabilities, remove_small_blobs,
                           model_grid_out, statistics_out, only) -> DevArray:
        """Model-grid image -> its uint8 labels (x, y, z), owned by `sc`: the triple z-split or one part, per part every model of the
        task (`only`: of these task ids), then on the whole grid the `model_grid_out` seam, the blob post-processing and the
        `statistics_out` seam, as `predict_image` documents them."""
        ss = img_rsp.shape
        # nnU-Net reads the spacing from the header of the file TS wrote (float32 pixdim), in array axis order (z, y, x)
        sp_zyx = [float(np.float32(v)) for v in sp_rsp[::-1]]
        seg = sc.own(DevArray.zeros(self.ctx, ss, np.uint8))
        if (np.prod(ss) > NR_VOXELS_THR and ss[2] > 200 and self.multimodel) or force_split:
            parts, comb = split_bounds(ss[2])
            for k, ((lo, hi), (dst, srcsl)) in enumerate(zip(parts, comb)):
                a, b, _ = srcsl.indices(hi - lo)
                self._predict_part_device(img_rsp.slice(2, lo, hi), seg.slice(2, dst.start, dst.stop), a, b, sp_zyx,
                                          save_probabilities=save_probabilities if k == 0 else None, only=only)
        else:
            self._predict_part_device(img_rsp, seg, 0, ss[2], sp_zyx, save_probabilities=save_probabilities, only=only)
        zooms_rsp = np.asarray(sp_rsp, dtype=np.float32)            # header zooms of the model-grid image (float32 pixdim)
        if model_grid_out is not None:
            model_grid_out["labels"], model_grid_out["zooms"] = seg.download(), zooms_rsp
        if remove_small_blobs or self.task_name == "body":
            self._postprocess_model_grid(seg, zooms_rsp, bool(remove_small_blobs))
        if statistics_out is not None:
            from . import statistics as st
            statistics_out["stats"] = st.basic_statistics(self.ctx, seg, img_rsp, zooms_rsp, task=self.task_name,
                                                          **dict(statistics_out.get("params") or {}))
            if model_grid_out is not None:
                model_grid_out["labels_post"], model_grid_out["ct"] = seg.download(), img_rsp.download()
        return seg

    def _to_input_grid(self, sc: Scope, seg: DevArray, back: "_WayBack", axcodes, keep_lut, onehot_spacing=None) -> DevArray:
        """Model-grid labels -> labels on the input grid (views of `seg`, or copies owned by `sc`): nearest resample back, the
        thickness reorientation and the canonical one undone, undo_crop, the shape check, the `roi_subset` table `keep_lut`.
        `onehot_spacing` (higher_order_resampling: the model grid's spacing (x, y, z)): nnU-Net's one-hot resampling instead of
        the nearest one, on the labels `keep_lut` has already filtered."""
        ctx, out = self.ctx, seg
        if back.zoom is not None and tuple(back.in_shape) != tuple(back.ss):      # back to the input grid (TS/nnunet.py:685-687)
            if onehot_spacing is None:
                buf = rs.resample_nearest_device(ctx, seg.buf, back.ss, back.in_shape)
            else:                                                    # nnunet_resampling, TS/nnunet.py:670-683
                if keep_lut is not None:                             # (:671-674; `seg` is this call's own array)
                    check(ctx.lib.boa_label_apply_lut(ctx.h, seg.buf.vp, seg.size, keep_lut.ctypes.data_as(C.c_void_p), seg.buf.vp),
                          "boa_label_apply_lut")
                # img_pred's header zooms: the float32 pixdim of the model-grid image
                _, axis, _ = nr.onehot_plan(back.ss, back.in_shape, np.asarray(onehot_spacing, dtype=np.float32))
                buf = rs.resample_onehot_device(ctx, seg.buf, back.ss, back.in_shape, axis)
            out = sc.own(DevArray(ctx, buf, back.in_shape, np.uint8))
        if back.thick_ornt is not None:
            # the labels are in `axcodes` order; back to RAS before undo_canonical
            out = out.apply_orientation(orientation.ornt_transform(orientation.axcodes2ornt(axcodes), orientation.RAS_ORNT))
        out = out.apply_orientation(orientation.ornt_transform(orientation.RAS_ORNT, orientation.io_orientation(back.cropped_affine)))
        if back.bbox is not None:                                    # undo_crop, TS/cropping.py:126-132
            full = sc.own(DevArray.zeros(ctx, back.orig_shape, np.uint8))
            out.copy_to(full.box(back.bbox))
            out = full
        if tuple(out.shape) != back.orig_shape[:3]:
            raise ValueError(f"shape mismatch after restore: {out.shape} vs {back.orig_shape}")   # check_if_shape_and_affine_identical
        if keep_lut is not None:                                     # img_data *= np.isin(img_data, subset), TS/nnunet.py:707-709
            out = sc.own(out.contiguous(force_copy=True))
            check(ctx.lib.boa_label_apply_lut(ctx.h, out.buf.vp, out.size, keep_lut.ctypes.data_as(C.c_void_p), out.buf.vp),
                  "boa_label_apply_lut")
        return out

    def predict_roi_subset(self, data, affine, crop_mask: np.ndarray, roi_subset: Sequence[str], **options):
        """`roi_subset` from the crop mask onward (TS/python_api.py:725-736): `predict_image` on the image cropped to the mask plus
        20 mm, the parts that hold the names, only their labels.  `options`: further keywords of `predict_image`."""
        return self.predict_image(data, affine, crop_mask=crop_mask, crop_addon=[20, 20, 20], roi_subset=roi_subset, **options)


def write_probabilities(path, probabilities: np.ndarray, properties: dict) -> None:
    """export_prediction_from_logits with save_probabilities (export_prediction.py:99-102): `<path>` gets
    np.savez_compressed(probabilities=float32 [C, z, y, x]), `Path(path).with_suffix(".pkl")` the pickled properties.  Existing
    files are overwritten (TS copies every model's pair over the last one's, TS/nnunet.py:286-293)."""
    import pickle
    from pathlib import Path
    path = Path(path)
    if probabilities.dtype != np.float32 or probabilities.ndim != 4:
        raise ValueError("probabilities must be float32 [C, z, y, x]")
    with open(path, "wb") as f:        # (a file object: numpy appends ".npz" to a path that lacks it)
        np.savez_compressed(f, probabilities=probabilities)
    with open(path.with_suffix(".pkl"), "wb") as f:
        pickle.dump(dict(properties), f)


def write_structure_masks(ctx: Context, seg, affine: np.ndarray, names: Dict[int, str], folder, like=None,
                          roi_subset: Optional[Sequence[str]] = None, dynamic: bool = False) -> List[str]:
    """The `ml=False` output of nnUNet_predict_image (TS/nnunet.py:782-802): `<folder>/<name>.nii.gz` = uint8 (seg == k) for every
    class (k, name) of the task's class map `names`, or with `roi_subset` only for the names it lists (:732-734); the header is a
    copy of `like` with the data type set to uint8.  `seg`: the task's uint8 label volume on the input grid, numpy or a DevArray.
    The masks are binarised and deflated on the device from the label volume (`nifti.save_label_masks`).  -> the names written."""
    import os
    from . import nifti
    selected = dict(names)
    if roi_subset is not None:
        selected = {k: v for k, v in selected.items() if v in roi_subset}
    os.makedirs(os.fspath(folder), exist_ok=True)
    nifti.save_label_masks(folder, seg, affine, selected, ctx, like=like, dynamic=dynamic)
    return list(selected.values())


def remove_outside_of_mask(ctx: Context, seg: np.ndarray, mask: np.ndarray, addon: int = 1) -> np.ndarray:
    """TS/postprocessing.py:101-131 on arrays of the same grid: dilate `mask != 0` `addon` times with the 6-neighbour cross
    (scipy.ndimage.binary_dilation(mask, iterations=addon)), clear `seg` outside.  Runs on the device."""
    if seg.shape != mask.shape:
        raise ValueError("segmentation and mask must have the same shape")
    if addon < 1:
        raise NotImplementedError("remove_outside_of_mask with addon < 1 (scipy dilates until convergence)")
    n = int(seg.size)
    Z, Y, X = (int(v) for v in seg.shape)
    with Scope() as sc:
        d_seg = sc.own(ctx.from_numpy(np.ascontiguousarray(seg, dtype=np.uint8)))
        d_m = sc.own(ctx.from_numpy(np.ascontiguousarray(mask != 0, dtype=np.uint8)))
        d_o, d_t = sc.own(ctx.alloc(n)), sc.own(ctx.alloc(n))
        check(ctx.lib.boa_binary_dilate_cross(ctx.h, d_m.vp, d_o.vp, d_t.vp, Z, Y, X, int(addon)), "boa_binary_dilate_cross")
        check(ctx.lib.boa_mask_assign(ctx.h, d_o.vp, n, 1, 0, d_seg.vp), "boa_mask_assign")          # seg[mask == 0] = 0
        return d_seg.download(seg.shape, np.uint8)


def run_cascade_task(ctx: Context, task: str, data: np.ndarray, affine: np.ndarray, rough_models, task_models,
                     crop_names: Sequence[str], crop_addon=(3, 3, 3), max_batch: int = 16, rough_resample: float = 6.0,
                     remove_outside: Optional[Sequence[str]] = None, remove_outside_dilation: Optional[float] = None,
                     precision: Optional[str] = None, save_probabilities=None, higher_order_resampling: bool = False) -> np.ndarray:
    """Crop-cascade task of `--models all` (TS/python_api.py:670-757): a rough `total` segmentation at 6 mm (single model
    Dataset298; 3 mm / Dataset297 with robust_crop: `rough_resample`), labels = the `total` map -> crop mask = union of the
    `crop_names` structures -> the task's own model at native resolution on the cropped image -> labels on the input grid
    -> optionally cleared outside the dilated union of the `remove_outside` structures (TS/nnunet.py:711-716).
    rough_models / task_models: [(task_id, ModelConfig, [weight blob per fold])] as `model_store.load_task_models` gives.
    `save_probabilities` (a path): passed to the TASK's model (`SegmentationTask.predict_image`: the probabilities of the cropped
    image's grid); the rough model's are not kept -- in the reference every later model run overwrites the file.
    `higher_order_resampling`: that of `predict_image`, for the task's model (which resamples only if the task has a `resample`
    spacing; the cascade tasks run at native resolution); the rough model keeps nearest, as in the reference."""
    organ_seg = rough_total(ctx, data, affine, rough_models, rough_resample, max_batch=max_batch, precision=precision)
    inv = label_maps.CLASS_MAP_TOTAL_INV
    crop_mask = np.isin(organ_seg, [inv[n] for n in crop_names]).astype(np.uint8)
    with SegmentationTask(ctx, task, task_models, resample=None, multimodel=False, max_batch=max_batch, precision=precision) as t:
        seg = t.predict_image(data, affine, crop_mask=crop_mask, crop_addon=crop_addon, save_probabilities=save_probabilities,
                              higher_order_resampling=higher_order_resampling)
    if remove_outside_dilation is not None:
        remove_mask = np.isin(organ_seg, [inv[n] for n in (remove_outside or [])]).astype(np.uint8)
        # header zooms are float32 (nibabel): int(mm / np.mean(img.header.get_zooms()))
        zooms = np.asarray(orientation.zooms_from_affine(np.asarray(affine, dtype=np.float64)), dtype=np.float32)
        vx = int(remove_outside_dilation / np.mean(zooms))
        seg = remove_outside_of_mask(ctx, seg, remove_mask, addon=vx)
    return seg


def rough_total(ctx: Context, data, affine: np.ndarray, rough_models, rough_resample: float = 6.0, max_batch: int = 16,
                precision: Optional[str] = None) -> np.ndarray:
    """The rough single-model `total` segmentation at `rough_resample` mm that the crop masks are cut from (TS/python_api.py:705-722):
    its `total` label volume on the input grid."""
    with SegmentationTask(ctx, "total", rough_models, resample=rough_resample, multimodel=False, max_batch=max_batch, precision=precision) as rough:
        return rough.predict_image(data, affine)


def rough_crop_mask(ctx: Context, data, affine: np.ndarray, rough_models, names: Sequence[str], rough_resample: float = 6.0,
                    max_batch: int = 16, precision: Optional[str] = None) -> np.ndarray:
    """The crop mask of `roi_subset` (TS/python_api.py:705-725): of `rough_total`, the union of the `names` structures as a uint8
    0 / 1 mask on the input grid."""
    organ_seg = rough_total(ctx, data, affine, rough_models, rough_resample, max_batch=max_batch, precision=precision)
    return np.isin(organ_seg, [label_maps.CLASS_MAP_TOTAL_INV[n] for n in names]).astype(np.uint8)


def run_roi_subset(ctx: Context, data, affine: np.ndarray, rough_models, task_models, roi_subset: Sequence[str],
                   resample: Optional[float] = 1.5, multimodel: bool = True, rough_resample: float = 6.0, max_batch: int = 16,
                   precision: Optional[str] = None, remove_small_blobs: bool = False, force_split: bool = False,
                   statistics_out: Optional[dict] = None, model_grid_out: Optional[dict] = None, info_out: Optional[dict] = None,
                   higher_order_resampling: bool = False) -> np.ndarray:
    """`roi_subset` of task `total` (TS/python_api.py:655-736, TS/nnunet.py:388-390,519-531,707-709): a rough `total` segmentation
    (single model Dataset298 at 6 mm; with `roi_subset_robust` Dataset297 at 3 mm: `rough_models`, `rough_resample`) -> crop mask =
    union of the named structures -> the image cropped to it plus 20 mm -> of the five part models only those whose class map holds
    one of the names (`label_maps.parts_for_roi_subset`; the others in `task_models` are never instantiated, and
    `model_store.load_task_models(task_ids=...)` need not even have read them), merged in part order -> on the input grid every label
    outside the subset cleared.  `multimodel=False` (`fast`: the single model Dataset297) has no part selection, only crop and filter.
    An empty crop mask gives the all-zero volume without running a part model.  `remove_small_blobs`, `force_split`,
    `statistics_out`, `model_grid_out` and `higher_order_resampling` are those of `SegmentationTask.predict_image` (the task's
    models only: the rough model keeps nearest, TS/python_api.py:705-722); `info_out` (a dict; test seam) gets
    `task_ids`, the models that were instantiated, and `crop_mask`.  Names outside the class map raise KeyError."""
    roi_subset = list(roi_subset)
    selected = label_maps.parts_for_roi_subset(roi_subset)        # (validates the names also when there is nothing to select)
    if multimodel:
        have = [m[0] for m in task_models]
        missing = [t for t in selected if t not in have]
        if missing:
            raise ValueError(f"roi_subset {roi_subset} needs the part models {missing}, which were not given")
        task_models = [m for m in task_models if m[0] in selected]
    crop_mask = rough_crop_mask(ctx, data, affine, rough_models, roi_subset, rough_resample, max_batch=max_batch, precision=precision)
    if info_out is not None:
        info_out["crop_mask"], info_out["task_ids"] = crop_mask, []
    if crop_mask.sum() == 0:                                      # TS/nnunet.py:428-446: nothing to segment
        return np.zeros(crop_mask.shape, dtype=np.uint8)
    with SegmentationTask(ctx, "total", task_models, resample=resample, multimodel=multimodel, max_batch=max_batch, precision=precision) as t:
        if info_out is not None:
            info_out["task_ids"] = [p[0] for p in t.parts]
        return t.predict_roi_subset(data, affine, crop_mask, roi_subset, force_split=force_split, remove_small_blobs=remove_small_blobs,
                                    statistics_out=statistics_out, model_grid_out=model_grid_out,
                                    higher_order_resampling=higher_order_resampling)


def body_crop_mask(ctx: Context, data, affine: np.ndarray, body_models, max_batch: int = 16, precision: Optional[str] = None) -> np.ndarray:
    """The rough body segmentation of `body_seg` (TS/python_api.py:739-749): Dataset300 at 6 mm as task `body` with its blob
    post-processing, binarised (`save_binary`, TS/nnunet.py:700-701) -> uint8 0 / 1 mask on the input grid."""
    with SegmentationTask(ctx, "body", body_models, resample=6.0, multimodel=False, max_batch=max_batch, precision=precision) as body:
        return (body.predict_image(data, affine) > 0).astype(np.uint8)


def run_with_body_crop(ctx: Context, task: str, data, affine: np.ndarray, body_models, task_models, resample: Optional[float] = None,
                       multimodel: Optional[bool] = None, crop_addon=(3, 3, 3), max_batch: int = 16, precision: Optional[str] = None,
                       remove_small_blobs: bool = False, force_split: bool = False, higher_order_resampling: bool = False) -> np.ndarray:
    """`body_seg=True` (TS/python_api.py:739-764), TotalSegmentator's speed-up for large images: the task runs on the image cropped
    to the bounding box of the rough body mask (`body_crop_mask`) plus `crop_addon` mm (the API's default [3, 3, 3]); outside the
    box the result is 0, and an empty body mask gives an all-zero result without running the task's models (the early return of
    `predict_image`).  body_models / task_models: [(task_id, ModelConfig, [weight blob per fold])].  `higher_order_resampling`:
    that of `predict_image`, for the task; the body model keeps nearest."""
    crop_mask = body_crop_mask(ctx, data, affine, body_models, max_batch=max_batch, precision=precision)
    with SegmentationTask(ctx, task, task_models, resample=resample, multimodel=multimodel, max_batch=max_batch, precision=precision) as t:
        return t.predict_image(data, affine, force_split=force_split, crop_mask=crop_mask, crop_addon=crop_addon,
                               remove_small_blobs=remove_small_blobs, higher_order_resampling=higher_order_resampling)
