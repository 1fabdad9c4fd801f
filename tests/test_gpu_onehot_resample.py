"""`higher_order_resampling` on the device: `boa_resample_onehot_u8` bit for bit against the per-label loop of
tests/onehot_reference.py (`resample_seg_loop`: every label's mask through `oracle.nnunet_resample.skimage_resize`, `>= 0.5`, labels
ascending), then the option at the task level (`SegmentationTask.predict_image`) and at the file level (`compute_all_models`).

The fixtures tests/golden/g_onehot_*.npz are the reference's own `resample_patient(None, seg, ...)` with `skimage.transform.resize`
replaced by `oracle.nnunet_resample.skimage_resize` -- skimage is not installed where they were generated, and that function is the
project's documented stand-in (tests/golden/make_golden_onehot.py).

The kernel gives every lane a run of 4 consecutive bytes of the LINEAR output and every block 256 lanes (1024 voxels): the shapes
below end a row, a plane and the volume inside a run and one voxel past a run and a block."""
import glob
import os
import warnings

import numpy as np
import pytest

import onehot_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g_onehot_*.npz")))
NAMES = [os.path.basename(p)[len("g_onehot_"):-len(".npz")] for p in GOLDEN]


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _device(ctx, seg_xyz, out_xyz, sep_ref=None):
    """seg (x, y, z) uint8 -> out_xyz on the device; sep_ref in the reference's [z, x, y] numbering."""
    from boa_hip import resample as rs
    from boa_hip.device import DeviceBuffer
    seg_xyz = np.ascontiguousarray(seg_xyz, dtype=np.uint8)
    d = DeviceBuffer(ctx, seg_xyz.size).upload(seg_xyz)
    o = rs.resample_onehot_device(ctx, d, seg_xyz.shape, out_xyz, sep_ref)
    got = o.download(tuple(out_xyz), np.uint8)
    d.free(), o.free()
    return got


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


def _few(shape, seed, palette=(0, 1, 127, 255)):
    return np.array(palette, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(palette), size=shape)]


def _checker(shape, a=3, b=203):
    return np.where(np.indices(shape).sum(0) % 2 == 0, a, b).astype(np.uint8)


def _cases():
    c = []
    for name, make in (("noise", _noise), ("few", _few)):
        c += [(f"{name}-x2", make((9, 7, 5), 1), (18, 14, 10), None),
              (f"{name}-x4", make((9, 7, 5), 2), (36, 28, 20), None),
              (f"{name}-nondyadic", make((11, 13, 6), 3), (23, 20, 17), None),
              (f"{name}-down", make((20, 18, 16), 4), (7, 9, 5), None),
              (f"{name}-half", make((20, 18, 16), 5), (10, 9, 8), None),       # x = 0.5 on every axis: exact ties at 0.5
              (f"{name}-len1", make((1, 9, 7), 6), (1, 20, 11), None),
              (f"{name}-len1-in", make((6, 1, 1), 7), (13, 4, 3), None)]
    c += [("checker-x2", _checker((9, 7, 5)), (18, 14, 10), None), ("checker-x4", _checker((9, 7, 5)), (36, 28, 20), None),
          ("checker-half", _checker((12, 10, 8)), (6, 5, 4), None), ("checker-half-odd", _checker((12, 10, 8), 200, 7), (6, 5, 4), None),
          ("checker-nondyadic", _checker((11, 13, 6)), (23, 20, 17), None)]
    # run and block boundaries of the linear output: row length run + 1, volume of one block + 1 voxel, + 1 run, rows of 1 and 3 bytes
    for k, out in enumerate([(8, 8, 5), (3, 3, 5), (1, 1, 1025), (1, 257, 4), (257, 1, 4), (5, 41, 5), (41, 5, 5), (1025, 1, 1),
                             (33, 31, 3), (2, 2, 257)]):
        c.append((f"bounds-{out}", _noise((4, 3, 5), 20 + k), out, None))
    for sep in (0, 1, 2):                                              # [z, x, y] numbering: memory axes 2, 0, 1
        m = (2, 0, 1)[sep]
        for name, make in (("noise", _noise), ("few", _few)):
            shp, out = [7, 6, 5], [15, 11, 13]
            out[m] = 3                                                 # the extent along the separate axis changes: nearest slice
            c.append((f"{name}-sep{sep}-change", make(tuple(shp), 30 + sep), tuple(out), sep))
            out[m] = 11
            c.append((f"{name}-sep{sep}-up", make(tuple(shp), 33 + sep), tuple(out), sep))
            out[m] = shp[m]                                            # the identity along it
            c.append((f"{name}-sep{sep}-same", make(tuple(shp), 36 + sep), tuple(out), sep))
    c += [("equal-dims", _noise((7, 6, 5), 40), (7, 6, 5), None), ("equal-dims-sep", _noise((7, 6, 5), 41), (7, 6, 5), 1)]
    return c


CASES = _cases()


@pytest.mark.parametrize("name,seg,out,sep", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_per_label_loop(ctx, name, seg, out, sep):
    want = R.resample_xyz(seg, out, sep, R.resample_seg_loop)
    got = _device(ctx, seg, out, sep)
    np.testing.assert_array_equal(got, want)


def test_eight_distinct_labels_in_a_cell(ctx):
    seg = (np.arange(1, 9, dtype=np.uint8) * 31).reshape(2, 2, 2)
    for out in ((4, 4, 4), (7, 5, 6), (8, 8, 8)):
        np.testing.assert_array_equal(_device(ctx, seg, out), R.resample_xyz(seg, out))


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES)
def test_kernel_reproduces_the_reference_fixtures(ctx, path):
    with np.load(path) as z:
        seg, want, target, axis = z["seg"], z["out"], z["target"].tolist(), int(z["axis"])
    np.testing.assert_array_equal(_device(ctx, seg, tuple(target), axis), want)


def test_output_past_two_to_the_31(ctx):
    """2^31 + 2^16 output voxels: slabs at both ends and in the middle against the 8-tap reference of those slabs."""
    from boa_hip import resample as rs
    from boa_hip.devarray import DevArray
    from boa_hip.device import DeviceBuffer
    seg = _noise((7, 5, 6), 50)
    out = (32769, 256, 256)
    assert np.prod(out, dtype=np.int64) > 2 ** 31
    d = DeviceBuffer(ctx, seg.size).upload(seg)
    o = rs.resample_onehot_device(ctx, d, seg.shape, out, None)
    arr = DevArray(ctx, o, out, np.uint8)
    xs = [0, 1, 16384, 32767, 32768]
    got = np.stack([arr.slice(0, x, x + 1).download()[0] for x in xs])
    d.free(), o.free()
    # reference axes [z, x, y]: x is axis 1
    want = R.from_ref(R.resample_seg_taps(R.to_ref(seg), (out[2], out[0], out[1]), None, select=[None, xs, None]))
    np.testing.assert_array_equal(got, want)


def test_bad_arguments_are_refused(ctx):
    from boa_hip._lib import int3
    from boa_hip.device import DeviceBuffer
    d, o = DeviceBuffer(ctx, 64), DeviceBuffer(ctx, 64)
    lib = ctx.lib
    assert lib.boa_resample_onehot_u8(ctx.h, d.vp, int3((2, 2, 2)), o.vp, int3((4, 4, 4)), 3) != 0
    assert lib.boa_resample_onehot_u8(ctx.h, d.vp, int3((2, 2, 2)), o.vp, int3((4, 4, 4)), -2) != 0
    assert lib.boa_resample_onehot_u8(ctx.h, d.vp, int3((0, 2, 2)), o.vp, int3((4, 4, 4)), -1) != 0
    assert lib.boa_resample_onehot_u8(ctx.h, d.vp, int3((2, 2, 2)), o.vp, int3((4, 0, 4)), -1) != 0
    assert lib.boa_resample_onehot_u8(ctx.h, d.vp, int3((2, 2, 2)), d.vp, int3((4, 4, 4)), -1) != 0       # in place
    d.free(), o.free()


# ---------------------------------------------------------------------------------------------- task level
SHAPE = (56, 48, 52)


def _affine(sp):
    aff = np.diag([-sp, -sp, sp, 1.0])                              # LPS file: undo_canonical flips x and y back
    aff[:3, 3] = [30.0, 40.0, -100.0]
    return aff


@pytest.fixture(scope="module")
def rough():
    """The synthetic 6 mm `total` model (118 classes) and the tiny phantom of tests/test_gpu_ml_false.py."""
    from boa_hip import plans
    from boa_hip.synthetic import ct_phantom
    pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=118, spacing=(6.0, 6.0, 6.0))
    cfg = plans.model_config_from_plans(pj, dj)
    sd = plans.synthetic_state_dict(cfg.geometry, seed=298)
    return dict(model=(298, cfg, [plans.weight_blob_from_state_dict(cfg.geometry, sd)]), ct=ct_phantom(SHAPE, seed=7), pj=pj, dj=dj,
                geom=cfg.geometry)


def _nearest(labels, out_shape):
    """scipy.ndimage.zoom(order=0) as boa_resample_nearest_u8 restates it: index floor(k (n_in - 1) / (n_out - 1) + 0.5)."""
    idx = []
    for n_in, n_out in zip(labels.shape, out_shape):
        z = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
        idx.append(np.clip(np.floor(np.arange(n_out) * z + 0.5).astype(int), 0, n_in - 1))
    return labels[np.ix_(*idx)]


def _plan_axis(labels_shape, out_shape, zooms):
    from boa_hip import nnunet_resample as nr
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nr.onehot_plan(labels_shape, out_shape, zooms)[1]


def test_predict_image_resamples_the_model_grid_labels_one_hot(ctx, rough):
    from boa_hip.task import SegmentationTask
    ct, aff = rough["ct"], _affine(1.5)
    with SegmentationTask(ctx, "total", [rough["model"]], resample=6.0, multimodel=False, max_batch=4) as t:
        default = t.predict_image(ct, aff)
        mg = {}
        got = t.predict_image(ct, aff, higher_order_resampling=True, model_grid_out=mg, statistics_out={})
        off = t.predict_image(ct, aff, higher_order_resampling=False)
        for attr in ("shard", "model_shard"):
            setattr(t, attr, object())
            with pytest.raises(NotImplementedError, match="higher_order_resampling"):
                t.predict_image(ct, aff, higher_order_resampling=True)
            setattr(t, attr, None)
    labels = mg["labels_post"]                                      # canonical (x, y, z) on the 6 mm grid
    assert labels.shape == (14, 12, 13) and len(np.unique(labels)) > 3
    assert mg["zooms"].dtype == np.float32
    want = R.resample_xyz(labels, SHAPE, _plan_axis(labels.shape, SHAPE, mg["zooms"]))[::-1, ::-1, :]
    assert got.dtype == np.uint8 and got.shape == SHAPE
    np.testing.assert_array_equal(got, want)
    # the default is what it was: the nearest resampling of the same labels, with and without the keyword spelled out
    np.testing.assert_array_equal(default, _nearest(labels, SHAPE)[::-1, ::-1, :])
    np.testing.assert_array_equal(off, default)
    assert (got != default).any()


def test_roi_subset_filters_before_the_interpolation(ctx, rough):
    """The input grid is COARSER than the model grid (12 mm against 6 mm), so every output voxel averages a 2 x 2 x 2 cell with
    equal weights and 4 : 4 cells tie at exactly 0.5.  A kept label that shares such a cell with a larger dropped one survives only
    if the dropped one is cleared before the resampling (TS/nnunet.py:671-674)."""
    from boa_hip import label_maps
    from boa_hip.task import SegmentationTask, get_bbox_from_mask
    ct, aff = rough["ct"], _affine(12.0)
    crop_mask = np.zeros(SHAPE, np.uint8)
    crop_mask[16:40, 12:36, 14:38] = 1
    bbox = get_bbox_from_mask(crop_mask, addon=(np.array([20, 20, 20]) / np.float32(12.0)).astype(int))   # mm -> voxels
    box_shape = tuple(b - a for a, b in bbox)
    assert box_shape == (26, 26, 26)
    names = label_maps.CLASS_MAP_TOTAL
    with SegmentationTask(ctx, "total", [rough["model"]], resample=6.0, multimodel=False, max_batch=4) as t:
        mg0 = {}
        t.predict_image(ct, aff, crop_mask=crop_mask, crop_addon=[20, 20, 20], higher_order_resampling=True, model_grid_out=mg0,
                        statistics_out={})
        labels = mg0["labels_post"]                                  # the same model, the same crop: the labels of the run below
        assert labels.shape == (52, 52, 52)
        axis = _plan_axis(labels.shape, box_shape, mg0["zooms"])
        # the first label for which the order of filter and interpolation matters (searched with the 8-tap formulation)
        unfiltered = R.resample_xyz(labels, box_shape, axis, R.resample_seg_taps)
        kept = next((int(l) for l in np.unique(labels) if l and not np.array_equal(
            R.resample_xyz(labels * (labels == l), box_shape, axis, R.resample_seg_taps), unfiltered * (unfiltered == l))), None)
        assert kept is not None, "no label of the phantom ties with a larger one: the case shows nothing"
        mg = {}
        got = t.predict_roi_subset(ct, aff, crop_mask, [names[kept]], higher_order_resampling=True, model_grid_out=mg, statistics_out={})
    np.testing.assert_array_equal(mg["labels_post"], labels)         # (the seam shows the labels before the filter)
    before = R.resample_xyz(labels * (labels == kept), box_shape, axis)          # the per-label loop
    after = R.resample_xyz(labels, box_shape, axis)
    after = after * (after == kept)
    assert (before != after).any()
    want = np.zeros(SHAPE, np.uint8)
    want[tuple(slice(a, b) for a, b in bbox)] = before[::-1, ::-1, :]
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got).tolist()) == {0, kept}


def test_run_roi_subset_hands_the_option_to_the_task_only(ctx, rough):
    """`run_roi_subset` with the 6 mm model as rough model and as the (single-model) task: the crop mask comes from the nearest
    resampling whatever the option says, the task's labels from the one-hot one."""
    from boa_hip import label_maps
    from boa_hip.task import SegmentationTask, run_roi_subset
    ct, aff = rough["ct"], _affine(1.5)
    names = label_maps.CLASS_MAP_TOTAL
    with SegmentationTask(ctx, "total", [rough["model"]], resample=6.0, multimodel=False, max_batch=4) as t:
        organ = t.predict_image(ct, aff)
        lab, cnt = np.unique(organ[organ > 0], return_counts=True)
        subset = [names[int(lab[np.argmax(cnt)])]]
        crop_mask = np.isin(organ, [label_maps.CLASS_MAP_TOTAL_INV[subset[0]]]).astype(np.uint8)
        want = t.predict_roi_subset(ct, aff, crop_mask, subset, higher_order_resampling=True)
        nearest = t.predict_roi_subset(ct, aff, crop_mask, subset)
    info = {}
    got = run_roi_subset(ctx, ct, aff, [rough["model"]], [rough["model"]], subset, resample=6.0, multimodel=False, max_batch=4,
                         info_out=info, higher_order_resampling=True)
    np.testing.assert_array_equal(info["crop_mask"], crop_mask)
    np.testing.assert_array_equal(got, want)
    assert (want != nearest).any()
    np.testing.assert_array_equal(run_roi_subset(ctx, ct, aff, [rough["model"]], [rough["model"]], subset, resample=6.0, multimodel=False,
                                                 max_batch=4), nearest)


# ---------------------------------------------------------------------------------------------- file level
PARAMS = {"preview": False, "fast": False, "fastest": True, "nr_thr_resamp": 1, "nr_thr_saving": 1, "quiet": True, "verbose": False,
          "device": "gpu", "license_number": None}


def test_compute_all_models_honours_the_key(tmp_path, monkeypatch, rough):
    from boa_hip import model_store, nifti, plans
    from boa_hip.compute.inference import compute_all_models, get_context
    from boa_hip.task import SegmentationTask
    root = tmp_path / "results"
    model_store.write_model_folder(str(root), 298, "TotalSegmentator_6mm", "nnUNetTrainer_4000epochs_NoMirroring", rough["pj"], rough["dj"],
                                   [plans.synthetic_state_dict(rough["geom"], seed=298)])
    monkeypatch.setenv("nnUNet_results", str(root))
    monkeypatch.delenv("BOA_SAVE_DEVICE", raising=False)
    ct, aff = rough["ct"], _affine(1.5)
    ct_path = tmp_path / "ct.nii.gz"
    nifti.save(ct_path, ct, aff)
    plain, off, on = tmp_path / "plain", tmp_path / "off", tmp_path / "on"
    compute_all_models(ct_path, plain, ["total"], dict(PARAMS))                                  # no key
    compute_all_models(ct_path, off, ["total"], dict(PARAMS, higher_order_resampling=False))
    compute_all_models(ct_path, on, ["total"], dict(PARAMS, higher_order_resampling=True))
    files = sorted(os.listdir(plain))
    assert {"total-measurements.json", "total.nii.gz"} <= set(files)
    assert sorted(os.listdir(off)) == files and sorted(os.listdir(on)) == files
    for f in files:                                               # without the key (or with it off) nothing changes
        assert (off / f).read_bytes() == (plain / f).read_bytes(), f
    c = get_context("gpu")
    with SegmentationTask(c, "total", model_store.load_task_models("total_6mm"), resample=6.0, multimodel=False) as t:
        want = t.predict_image(ct, aff, higher_order_resampling=True)
        nearest = t.predict_image(ct, aff)
    total, taff, _ = nifti.load(on / "total.nii.gz")
    assert np.allclose(taff, aff)
    np.testing.assert_array_equal(total, want)
    np.testing.assert_array_equal(nifti.load(plain / "total.nii.gz")[0], nearest)
    assert (want != nearest).any()
