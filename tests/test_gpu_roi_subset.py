"""`roi_subset` and `statistics` of task `total` (TS/python_api.py:636-664,671-736,778-796; TS/nnunet.py:388-390,519-531,642-659,707-709)
against an ORACLE composed here from oracle.pipeline.predict_image (rough model; then the selected part models only, on the crop),
oracle.cascade.crop_to_mask / undo_crop and the `isin` filter.  Networks: torch-CPU fp32 oracle vs the device in exact mode (0 label
flips expected, <= 1e-5 asserted: the bar of tests/test_gpu_cascade.py) and in the fp16 production mode (<= 5e-3).  The statistics are
integer work: compared bit for bit with tests/basic_statistics_reference.py."""
import json

import numpy as np
import pytest

import basic_statistics_reference as R

pytestmark = pytest.mark.gpu

SHAPE, SP = (84, 76, 60), (1.2, 1.2, 2.0)
PART_CLASSES = (25, 27, 19, 24, 27)          # background + the structures of class_map_part_* (label_maps.CLASS_MAP_PARTS)


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _model(tid, nc, seed, spacing_zyx, patch=(32, 32, 32), features=(32, 64)):
    import torch
    from boa_hip import plans
    from oracle.network import build_from_arch, network_fn_from_module
    pj, dj = plans.synthetic_plans(patch=patch, features=features, num_classes=nc, spacing=spacing_zyx)
    cfg = plans.model_config_from_plans(pj, dj)
    sd = plans.synthetic_state_dict(cfg.geometry, seed=seed)
    blob = plans.weight_blob_from_state_dict(cfg.geometry, sd)
    net = build_from_arch(pj["configurations"]["3d_fullres"]["architecture"]["arch_kwargs"], 1, nc)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return (tid, cfg, [blob]), ([network_fn_from_module(net, 8)], patch, nc, cfg.intensity_properties["0"])


@pytest.fixture(scope="module")
def setup():
    """phantom, models (device entry, oracle entry), the rough oracle segmentation and the subset drawn from it -- built once"""
    from boa_hip import label_maps
    from boa_hip.synthetic import ct_phantom
    from oracle import pipeline as opipe
    assert [len(label_maps.CLASS_MAP_PARTS[t]) + 1 for t in label_maps.PART_TASK_IDS] == list(PART_CLASSES)
    ct = ct_phantom(SHAPE, seed=298)
    rough_m, rough_o = _model(298, 118, 298, (6.0,) * 3)
    parts_m, parts_o = {}, {}
    for tid, nc in zip(label_maps.PART_TASK_IDS, PART_CLASSES):
        m, o = _model(tid, nc, tid, (1.5, 1.5, 1.5))
        parts_m[tid], parts_o[tid] = m, o + (label_maps.CLASS_MAP_PARTS[tid],)
    organ = opipe.predict_image(ct, SP, [rough_o + (None,)], None, "total", 6.0, multimodel=False)
    lab, cnt = np.unique(organ[organ > 0], return_counts=True)

    def bbox_volume(l):
        idx = np.where(organ == l)
        return int(np.prod([idx[a].max() - idx[a].min() + 1 for a in range(3)]))

    # the two structures with the smallest bounding boxes (>= 8 voxels) that belong to two different parts
    names = label_maps.CLASS_MAP_TOTAL
    cand = sorted((int(l) for l, c in zip(lab, cnt) if c >= 8), key=bbox_volume)
    first = cand[0]
    part_of = lambda l: label_maps.parts_for_roi_subset([names[l]])[0]
    second = next(l for l in cand[1:] if part_of(l) != part_of(first))
    subset = [names[first], names[second]]
    return dict(ct=ct, rough_m=rough_m, rough_o=rough_o + (None,), parts_m=parts_m, parts_o=parts_o, organ=organ, subset=subset)


def _oracle(s, subset, models_o, multimodel, resample):
    from boa_hip import label_maps
    from oracle import cascade as ocas
    from oracle import pipeline as opipe
    inv = label_maps.CLASS_MAP_TOTAL_INV
    ids = [inv[n] for n in subset]
    crop_mask = np.isin(s["organ"], ids).astype(np.uint8)
    crop, bbox = ocas.crop_to_mask(s["ct"], crop_mask, np.asarray(SP, dtype=np.float32), (20, 20, 20))
    seg_c = opipe.predict_image(crop.astype(np.int32), SP, models_o, inv if multimodel else None, "total", resample, multimodel=multimodel)
    seg = ocas.undo_crop(seg_c, s["ct"].shape, bbox)
    seg *= np.isin(seg, ids)
    return seg, bbox


def test_roi_subset_vs_oracle(ctx, setup):
    from boa_hip import label_maps
    from boa_hip.task import run_roi_subset
    s = setup
    subset = s["subset"]
    selected = label_maps.parts_for_roi_subset(subset)
    assert len(selected) == 2
    want, bbox = _oracle(s, subset, [s["parts_o"][t] for t in selected], True, 1.5)
    vol_crop = int(np.prod([b[1] - b[0] for b in bbox]))
    print(f"subset {subset} -> parts {selected}, bbox {bbox} ({vol_crop / want.size:.2f} of the volume), labels {np.unique(want)}")
    assert vol_crop < want.size, "the crop is the whole volume"
    ids = {label_maps.CLASS_MAP_TOTAL_INV[n] for n in subset}
    assert want.any() and set(np.unique(want).tolist()) <= ids | {0}
    aff = np.diag([SP[0], SP[1], SP[2], 1.0])
    outside = np.ones(want.shape, bool)
    outside[tuple(slice(a, b) for a, b in bbox)] = False
    for prec, bar in (("fp32", 1e-5), ("fp16", 5e-3)):
        info = {}
        got = run_roi_subset(ctx, s["ct"], aff, [s["rough_m"]], list(s["parts_m"].values()), subset, resample=1.5, multimodel=True,
                             max_batch=4, precision=prec, info_out=info)
        assert got.shape == want.shape and got.dtype == np.uint8
        flips = float((got != want).mean())
        print(f"  {prec}: label flips vs the oracle {flips:.3g}")
        assert flips <= bar, (prec, flips)
        assert set(np.unique(got).tolist()) <= ids | {0}          # only subset labels
        assert not got[outside].any()                             # nothing outside the box
        assert info["task_ids"] == selected                       # only the parts that hold the names were instantiated
    # the part models that are not selected need not be given at all
    got2 = run_roi_subset(ctx, s["ct"], aff, [s["rough_m"]], [s["parts_m"][t] for t in selected], subset, max_batch=4, precision="fp16")
    np.testing.assert_array_equal(got, got2)
    with pytest.raises(ValueError, match="part models"):
        run_roi_subset(ctx, s["ct"], aff, [s["rough_m"]], [s["parts_m"][selected[0]]], subset, max_batch=4)
    with pytest.raises(KeyError, match="no_such_organ"):
        run_roi_subset(ctx, s["ct"], aff, [s["rough_m"]], list(s["parts_m"].values()), subset + ["no_such_organ"], max_batch=4)


def test_totalsegmentator_class_takes_the_same_keywords(ctx, setup):
    """TotalSegmentatorHip.predict(roi_subset=..., statistics=True): the labels of run_roi_subset, the dict of the restatement on the
    returned labels and the CT; all five parts stay loaded, only the selected ones run"""
    from boa_hip import label_maps, totalseg
    from boa_hip.task import run_roi_subset
    s = setup
    subset = s["subset"]
    aff = np.diag([SP[0], SP[1], SP[2], 1.0])
    want = run_roi_subset(ctx, s["ct"], aff, [s["rough_m"]], list(s["parts_m"].values()), subset, max_batch=4)
    ts = totalseg.TotalSegmentatorHip(ctx, list(s["parts_m"].values()), max_batch=4)
    try:
        got, stats = ts.predict(s["ct"], affine=aff, roi_subset=subset, rough_models=[s["rough_m"]], statistics=True,
                                statistics_exclude_masks_at_border=False, stats_aggregation="median")
        assert [p[0] for p in ts.parts] == list(label_maps.PART_TASK_IDS)
        with pytest.raises(ValueError, match="must be a list of strings"):
            ts.predict(s["ct"], affine=aff, roi_subset="liver", rough_models=[s["rough_m"]])
        with pytest.raises(ValueError, match="rough_models"):
            ts.predict(s["ct"], affine=aff, roi_subset=subset)
    finally:
        ts.close()
    np.testing.assert_array_equal(got, want)
    cm = dict(sorted(label_maps.class_map("total").items()))
    ref = R.basic_statistics(got, s["ct"], np.asarray(SP, dtype=np.float32), cm, exclude_masks_at_border=False, roi_subset=subset,
                             metric="median")
    assert list(stats) == list(ref)
    assert all(float(stats[n]["volume"]) == float(ref[n]["volume"]) and float(stats[n]["intensity"]) == float(ref[n]["intensity"]) for n in ref)
    assert any(v["volume"] > 0 for v in stats.values())


def test_roi_subset_empty_crop(ctx, setup):
    """names the rough model did not find: the all-zero volume, no part model instantiated (TS/nnunet.py:428-446)"""
    from boa_hip import label_maps
    from boa_hip.task import run_roi_subset
    s = setup
    present = set(np.unique(s["organ"]).tolist())
    absent = [n for n, l in label_maps.CLASS_MAP_TOTAL_INV.items() if l not in present][:2]
    assert len(absent) == 2
    info = {}
    got = run_roi_subset(ctx, s["ct"], np.diag([SP[0], SP[1], SP[2], 1.0]), [s["rough_m"]], list(s["parts_m"].values()), absent,
                         max_batch=4, precision="fp32", info_out=info)
    assert got.shape == SHAPE and got.dtype == np.uint8 and not got.any()
    assert info["task_ids"] == [] and not info["crop_mask"].any()


def test_fast_roi_subset_with_statistics_on_the_model_grid(ctx, setup, tmp_path):
    """`fast`: the single 3 mm model, no part selection, crop and filter only; `statistics` together with it is taken on the model grid
    (statistics_fast): the dict equals the restatement on the model-grid arrays, the label volume the oracle's"""
    from boa_hip import label_maps, statistics as S
    from boa_hip.task import run_roi_subset
    s = setup
    subset = s["subset"]
    fast_m, fast_o = _model(297, 118, 297, (3.0,) * 3)
    want, bbox = _oracle(s, subset, [fast_o + (None,)], False, 3.0)
    aff = np.diag([SP[0], SP[1], SP[2], 1.0])
    path = tmp_path / "statistics.json"
    st = {"params": dict(exclude_masks_at_border=False, roi_subset=subset, metric="mean", file_out=path)}
    mg, info = {}, {}
    got = run_roi_subset(ctx, s["ct"], aff, [s["rough_m"]], [fast_m], subset, resample=3.0, multimodel=False, max_batch=4,
                         precision="fp32", statistics_out=st, model_grid_out=mg, info_out=info)
    assert info["task_ids"] == [297]
    flips = float((got != want).mean())
    print(f"fast roi_subset: label flips vs the oracle {flips:.3g}, labels {np.unique(got)}")
    assert flips <= 1e-5
    cm = dict(sorted(label_maps.class_map("total").items()))
    lab, ct_mg, zooms = mg["labels_post"], mg["ct"], mg["zooms"]
    assert ct_mg.dtype == np.int32 and lab.shape == ct_mg.shape and lab.shape != SHAPE and zooms.tolist() == [3.0, 3.0, 3.0]
    ref = R.basic_statistics(lab, ct_mg, zooms, cm, exclude_masks_at_border=False, roi_subset=subset, metric="mean")
    stats = st["stats"]
    assert list(stats) == list(ref) and sorted(stats) == sorted(subset)
    for n in ref:
        assert float(stats[n]["volume"]) == float(ref[n]["volume"]) and float(stats[n]["intensity"]) == float(ref[n]["intensity"]), (n, stats[n], ref[n])
    assert any(v["volume"] > 0 for v in stats.values())           # (the unfiltered model-grid labels hold the subset)
    with open(path) as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    # the other aggregations on the same resident-style arrays
    for kw in (dict(metric="median", exclude_masks_at_border=False), dict(metric="mean", exclude_masks_at_border=True),
               dict(metric="median", exclude_masks_at_border=False, roi_subset=subset)):
        a, b = S.basic_statistics(ctx, lab, ct_mg, zooms, **kw), R.basic_statistics(lab, ct_mg, zooms, cm, **kw)
        assert list(a) == list(b)
        assert all(float(a[n]["volume"]) == float(b[n]["volume"]) and float(a[n]["intensity"]) == float(b[n]["intensity"]) for n in b)


def test_compute_all_models_roi_subset_statistics(tmp_path, monkeypatch):
    """file level: {"roi_subset": [...], "statistics": True} -> total.nii.gz with the subset only (voxels and header label table),
    statistics.json next to it = the restatement on the saved volume and the CT; only the selected parts' folders exist"""
    from boa_hip import label_maps, model_store, nifti, plans
    from boa_hip.compute.inference import compute_all_models, get_context
    from boa_hip.synthetic import ct_phantom
    from boa_hip.task import SegmentationTask
    root = tmp_path / "results"

    def write(tid, nc, name, trainer, sp):
        pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=nc, spacing=sp)
        geom = plans.model_config_from_plans(pj, dj).geometry
        model_store.write_model_folder(str(root), tid, name, trainer, pj, dj, [plans.synthetic_state_dict(geom, seed=tid)])

    write(298, 118, "TotalSegmentator_6mm", "nnUNetTrainer_4000epochs_NoMirroring", (6.0, 6.0, 6.0))
    monkeypatch.setenv("nnUNet_results", str(root))
    ct = ct_phantom((56, 48, 52), seed=7)
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])                       # LPS file
    aff[:3, 3] = [30.0, 40.0, -100.0]
    ct_path = tmp_path / "ct.nii.gz"
    nifti.save(ct_path, ct, aff)
    ctx = get_context("gpu")
    # the subset: the two most frequent structures of the rough segmentation that belong to two different parts
    rough = SegmentationTask(ctx, "total", model_store.load_task_models("total_6mm"), resample=6.0, multimodel=False)
    organ = rough.predict_image(ct, aff)
    rough.close()
    lab, cnt = np.unique(organ[organ > 0], return_counts=True)
    order = [int(l) for l in lab[np.argsort(-cnt)]]
    names = label_maps.CLASS_MAP_TOTAL
    part_of = lambda l: label_maps.parts_for_roi_subset([names[l]])[0]
    second = next(l for l in order[1:] if part_of(l) != part_of(order[0]))
    subset = [names[order[0]], names[second]]
    selected = label_maps.parts_for_roi_subset(subset)
    for tid in selected:                                         # (the other three parts have no folder: they must not be looked for)
        write(tid, len(label_maps.CLASS_MAP_PARTS[tid]) + 1, f"TotalSegmentator_part{tid - 290}", "nnUNetTrainerNoMirroring", (1.5, 1.5, 1.5))
    params = {"preview": False, "fast": False, "ml": True, "nr_thr_resamp": 1, "nr_thr_saving": 1, "quiet": True, "verbose": False,
              "device": "gpu", "license_number": None, "roi_subset": subset, "statistics": True}
    out = tmp_path / "seg"
    compute_all_models(ct_path, out, ["total"], params)
    total, taff, th = nifti.load(out / "total.nii.gz")
    ids = {label_maps.CLASS_MAP_TOTAL_INV[n] for n in subset}
    assert total.dtype == np.uint8 and total.shape == ct.shape and np.allclose(taff, aff)
    assert set(np.unique(total).tolist()) <= ids | {0}
    assert nifti.parse_label_xml(th.extensions[0][1]) == {i: names[i] for i in sorted(ids)}
    _, _, ch = nifti.load(ct_path)
    cm = dict(sorted(label_maps.class_map("total").items()))
    ref = R.basic_statistics(total, ct, np.asarray(ch.get_zooms()[:3], dtype=np.float32), cm, roi_subset=subset)
    with open(out / "statistics.json") as f:
        text = f.read()
    got = json.loads(text)
    assert list(got) == list(ref) and text == json.dumps(ref, indent=4)
    for n in ref:
        assert got[n]["volume"] == float(ref[n]["volume"]) and got[n]["intensity"] == float(ref[n]["intensity"])
    # the parameter refusals reach the file level
    with pytest.raises(ValueError, match="must be a list of strings"):
        compute_all_models(ct_path, tmp_path / "o2", ["total"], dict(params, roi_subset="liver"))
