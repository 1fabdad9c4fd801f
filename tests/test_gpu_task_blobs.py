"""The blob post-processing of the task path (TS/nnunet.py:595-617, TS/python_api.py:739-764): `remove_small_blobs` and the `body`
task in SegmentationTask.predict_image, `body_seg` (run_with_body_crop) and the two TotalSegmentator parameters in
compute_all_models.  Synthetic random-weight nets as in tests/test_gpu_cascade.py (patch 32^3, features (32, 64)): their argmax is
speckle, which is what these filters exist for.

How the expected volumes are made: `predict_image(model_grid_out={})` (a keyword seam) hands out the device's own model-grid
labels of the SAME call, before the filters; tests/blob_reference.py (scipy) filters them and oracle.resample takes them back
to the input grid with order 0.  Both sides start from the same device labels, so every comparison is exact and fp16 rounding
plays no part."""
import numpy as np
import pytest

import blob_reference as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _model(tid, nc, seed, spacing_zyx, patch=(32, 32, 32), features=(32, 64), background_bias=0.0):
    """`background_bias` is added to the background logit of the head: the foreground of a random-weight net becomes sparse"""
    from boa_hip import plans
    pj, dj = plans.synthetic_plans(patch=patch, features=features, num_classes=nc, spacing=spacing_zyx)
    cfg = plans.model_config_from_plans(pj, dj)
    sd = plans.synthetic_state_dict(cfg.geometry, seed=seed)
    sd["decoder.seg_layers.0.bias"] = sd["decoder.seg_layers.0.bias"].copy()
    sd["decoder.seg_layers.0.bias"][0] += np.float32(background_bias)
    blob = plans.weight_blob_from_state_dict(cfg.geometry, sd)
    return (tid, cfg, [blob])


def _back(seg, mm, shape):
    """TS/nnunet.py:685-687: the model-grid labels back on the input grid, order 0"""
    from oracle import resample as orsp
    if tuple(seg.shape) == tuple(shape):
        return seg.astype(np.uint8)
    return orsp.change_spacing_array(seg, [mm] * 3, [mm] * 3, target_shape=shape, order=0, dtype=np.uint8)[0]


def test_remove_small_blobs_runs_on_the_model_grid(ctx):
    """a 1.2 x 1.2 x 2.0 mm phantom, a 1.5 mm model: blobs of at most floor(200 / 3.375) = 59 model-grid voxels go, then the labels
    are resampled back -- filtering the resampled labels (69 voxels of 2.88 mm^3) gives another volume"""
    from boa_hip import label_maps
    from boa_hip.synthetic import ct_phantom
    from boa_hip.task import SegmentationTask
    ct = ct_phantom((84, 76, 60), seed=11)
    aff = np.diag([1.2, 1.2, 2.0, 1.0])
    cm = label_maps.class_map("total")
    t = SegmentationTask(ctx, "total", [_model(297, 6, 297, (1.5, 1.5, 1.5))], resample=1.5, multimodel=False, max_batch=4)
    try:
        grid = {}
        got = t.predict_image(ct, aff, remove_small_blobs=True, model_grid_out=grid)
        plain = t.predict_image(ct, aff)
    finally:
        t.close()
    labels = grid["labels"]
    assert labels.shape == (67, 61, 80) and grid["zooms"].dtype == np.float32 and list(grid["zooms"]) == [1.5, 1.5, 1.5]
    thr = br.size_threshold_voxels(200, grid["zooms"])
    assert int(np.floor(thr)) == 59
    filtered = br.remove_small_blobs_multilabel(labels, cm, list(cm.values()), [thr, 1e10])
    removed = int((filtered != labels).sum())
    print(f"model grid: {len(br.components6(labels)[1])} blobs, {removed} of {int((labels != 0).sum())} labelled voxels removed")
    assert removed > 0 and filtered.any()
    assert got.shape == ct.shape and got.dtype == np.uint8
    np.testing.assert_array_equal(got, _back(filtered, 1.5, ct.shape))
    np.testing.assert_array_equal(plain, _back(labels, 1.5, ct.shape))          # the option off: the labels as before
    after = br.remove_small_blobs_multilabel(plain, cm, list(cm.values()), [br.size_threshold_voxels(200, (1.2, 1.2, 2.0)), 1e10])
    assert (after != got).any(), "filtering after the resample back gives the same volume: the test does not show the order"


@pytest.mark.parametrize("small", [False, True])
def test_body_task_at_6mm(ctx, small):
    """task body: keep the largest body_trunc blob, drop body_extremities blobs of at most 231 voxels, then (remove_small_blobs) blobs
    of at most floor(200 / 216) = 0 voxels: the reference's order, on the device's own unfiltered labels"""
    from boa_hip.synthetic import ct_phantom
    from boa_hip.task import SegmentationTask
    ct = ct_phantom((120, 112, 96), seed=300)
    aff = np.diag([1.5, 1.5, 1.5, 1.0])
    t = SegmentationTask(ctx, "body", [_model(300, 3, 300, (6.0, 6.0, 6.0))], resample=6.0, multimodel=False, max_batch=4)
    try:
        grid = {}
        got = t.predict_image(ct, aff, remove_small_blobs=small, model_grid_out=grid)
    finally:
        t.close()
    labels = grid["labels"]
    assert labels.shape == (30, 28, 24) and set(np.unique(labels)) == {0, 1, 2}
    want = br.body_postprocessing(labels, grid["zooms"], remove_small=small)
    assert (want != labels).any() and want.any(), "the filters removed nothing: the test shows nothing"
    n1 = len(br.components6((labels == 1).astype(np.uint8))[1])
    assert n1 > 1 and len(br.components6((want == 1).astype(np.uint8))[1]) == 1
    np.testing.assert_array_equal(got, _back(want, 6.0, ct.shape))


def test_body_seg_crops_to_the_body_mask(ctx, monkeypatch):
    """the body net's background logit is raised by 3.5 so that its labels are sparse specks (the torch-CPU restatement of this net
    leaves a largest body_trunc blob of 334 voxels at 6 mm, the next has 156, and no body_extremities blob above 231): the body
    mask is ONE blob and its box a real crop -- whichever blob the device's fp16 arithmetic makes the largest"""
    from boa_hip import task as T
    from boa_hip.synthetic import ct_phantom
    ct = ct_phantom((96, 88, 72), seed=21)
    # air around the phantom in the array, so that the box of the body mask is a real crop
    ct = np.pad(ct, ((20, 12), (16, 24), (10, 14)), constant_values=-1024)
    aff = np.diag([1.5, 1.5, 1.5, 1.0])
    body_m, task_m = _model(300, 3, 300, (6.0, 6.0, 6.0), background_bias=3.5), _model(297, 6, 297, (1.5, 1.5, 1.5))
    # the body labels, as the device gives them, and what the reference makes of them
    b = T.SegmentationTask(ctx, "body", [body_m], resample=6.0, multimodel=False, max_batch=4)
    try:
        grid = {}
        b.predict_image(ct, aff, model_grid_out=grid)
    finally:
        b.close()
    mask_want = (_back(br.body_postprocessing(grid["labels"], grid["zooms"]), 6.0, ct.shape) > 0).astype(np.uint8)
    mask = T.body_crop_mask(ctx, ct, aff, [body_m], max_batch=4)
    np.testing.assert_array_equal(mask, mask_want)
    assert mask.dtype == np.uint8 and set(np.unique(mask)) == {0, 1}
    bbox = T.get_bbox_from_mask(mask_want, outside_value=0, addon=(np.array([3, 3, 3]) / np.array([1.5, 1.5, 1.5])).astype(int))
    vol = int(np.prod([hi - lo for lo, hi in bbox]))
    print(f"body box {bbox}: {vol / ct.size:.2f} of the volume")
    got = T.run_with_body_crop(ctx, "total", ct, aff, [body_m], [task_m], resample=1.5, multimodel=False, max_batch=4)
    assert got.shape == ct.shape and got.dtype == np.uint8
    assert mask_want.any() and vol < 0.6 * ct.size, "the body box is no real crop: the test shows nothing"
    outside = np.ones(ct.shape, bool)
    outside[tuple(slice(lo, hi) for lo, hi in bbox)] = False
    assert not got[outside].any()
    # inside the box: the plain run on the cropped volume (crop_to_mask hands it over as int32)
    sl = tuple(slice(lo, hi) for lo, hi in bbox)
    t = T.SegmentationTask(ctx, "total", [task_m], resample=1.5, multimodel=False, max_batch=4)
    try:
        inner = t.predict_image(np.ascontiguousarray(ct[sl]).astype(np.int32), aff)
    finally:
        t.close()
    assert inner.any()
    np.testing.assert_array_equal(got[sl], inner)
    # an empty body mask: all zero, and the task's model never runs
    monkeypatch.setattr(T, "body_crop_mask", lambda *a, **k: np.zeros(ct.shape, np.uint8))

    def never(*a, **k):
        raise AssertionError("the task model ran on an empty body mask")

    monkeypatch.setattr(T.SegmentationTask, "predict_zyx_device", never)
    empty = T.run_with_body_crop(ctx, "total", ct, aff, [body_m], [task_m], resample=1.5, multimodel=False, max_batch=4)
    assert empty.shape == ct.shape and empty.dtype == np.uint8 and not empty.any()


def test_sharded_tasks_refuse_the_blob_options(ctx):
    from boa_hip.task import SegmentationTask
    t = SegmentationTask(ctx, "total", [_model(297, 6, 297, (1.5, 1.5, 1.5))], resample=1.5, multimodel=False, max_batch=4)
    b = SegmentationTask(ctx, "body", [_model(300, 3, 300, (6.0, 6.0, 6.0))], resample=6.0, multimodel=False, max_batch=4)
    try:
        t.model_shard = b.model_shard = object()
        ct = np.zeros((8, 8, 8), np.int16)
        with pytest.raises(NotImplementedError):
            t.predict_image(ct, np.eye(4), remove_small_blobs=True)
        with pytest.raises(NotImplementedError):
            b.predict_image(ct, np.eye(4))
    finally:
        t.model_shard = b.model_shard = None
        t.close()
        b.close()


def test_compute_all_models_parameters(tmp_path, monkeypatch):
    """`remove_small_blobs` / `body_seg` off (or absent) leave total.nii.gz byte for byte as it was; on, the file carries what the
    array-level calls give; model `body` (fast: Dataset300 at 6 mm) writes body.nii.gz with its label table"""
    from boa_hip import label_maps, model_store, nifti, plans
    from boa_hip.compute.inference import compute_all_models, get_context
    from boa_hip.synthetic import ct_phantom
    from boa_hip.task import SegmentationTask, run_with_body_crop
    root = tmp_path / "results"
    for tid, nc, name, trainer, sp in ((297, 118, "TotalSegmentator_3mm", "nnUNetTrainer_4000epochs_NoMirroring", (3.0, 3.0, 3.0)),
                                       (300, 3, "TotalSegmentator_body_6mm", "nnUNetTrainer", (6.0, 6.0, 6.0))):
        pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=nc, spacing=sp)
        geom = plans.model_config_from_plans(pj, dj).geometry
        model_store.write_model_folder(str(root), tid, name, trainer, pj, dj, [plans.synthetic_state_dict(geom, seed=tid)])
    monkeypatch.setenv("nnUNet_results", str(root))
    ct = ct_phantom((96, 80, 88), seed=5)
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])                       # LPS file
    aff[:3, 3] = [30.0, 40.0, -100.0]
    ct_path = tmp_path / "ct.nii.gz"
    nifti.save(ct_path, ct, aff)
    params = {"preview": False, "fast": True, "ml": True, "nr_thr_resamp": 1, "nr_thr_saving": 1, "quiet": True, "verbose": False,
              "device": "gpu", "license_number": None}

    def run(folder, models=("total",), **extra):
        compute_all_models(ct_path, tmp_path / folder, list(models), dict(params, **extra))
        return tmp_path / folder

    plain = (run("plain") / "total.nii.gz").read_bytes()
    assert (run("off", remove_small_blobs=False, body_seg=False) / "total.nii.gz").read_bytes() == plain
    ctx = get_context("gpu")
    t = SegmentationTask(ctx, "total", model_store.load_task_models("total_fast"), resample=3.0, multimodel=False)
    try:
        base = t.predict_image(ct, aff)
        small = t.predict_image(ct, aff, remove_small_blobs=True)
    finally:
        t.close()
    np.testing.assert_array_equal(nifti.load(tmp_path / "plain" / "total.nii.gz")[0], base)
    assert (small != base).any()
    np.testing.assert_array_equal(nifti.load(run("small", remove_small_blobs=True) / "total.nii.gz")[0], small)
    want = run_with_body_crop(ctx, "total", ct, aff, model_store.load_task_models("body_fast"), model_store.load_task_models("total_fast"),
                              resample=3.0, multimodel=False, remove_small_blobs=True)
    np.testing.assert_array_equal(nifti.load(run("crop", remove_small_blobs=True, body_seg=True) / "total.nii.gz")[0], want)
    out = run("body", models=("body",))
    body, _, bh = nifti.load(out / "body.nii.gz")
    assert nifti.parse_label_xml(bh.extensions[0][1]) == {1: "body_trunc", 2: "body_extremities"} == label_maps.class_map("body")
    b = SegmentationTask(ctx, "body", model_store.load_task_models("body_fast"), resample=6.0, multimodel=False)
    try:
        np.testing.assert_array_equal(body, b.predict_image(ct, aff))
    finally:
        b.close()
    assert not (out / "total-measurements.json").exists() or "body" not in (out / "total-measurements.json").read_text()
