"""`"ml": False` at the file level (`compute_all_models`): the directory `<segmentation_folder>/<name>/` with one binary mask file per
class next to an unchanged `<name>.nii.gz` (TS/nnunet.py:732-734,782-802; the directory's place is this engine's own), with the
synthetic 6 mm weights and the tiny volume of tests/test_gpu_roi_subset.py's file-level test."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = {"preview": False, "fast": False, "fastest": True, "nr_thr_resamp": 1, "nr_thr_saving": 1, "quiet": True, "verbose": False,
          "device": "gpu", "license_number": None}


def _write_ct(tmp_path):
    from boa_hip import nifti
    from boa_hip.synthetic import ct_phantom
    ct = ct_phantom((56, 48, 52), seed=7)
    aff = np.diag([-1.5, -1.5, 1.5, 1.0])                       # LPS file
    aff[:3, 3] = [30.0, 40.0, -100.0]
    nifti.save(tmp_path / "ct.nii.gz", ct, aff)
    return tmp_path / "ct.nii.gz", aff


def test_total_with_ml_false_writes_one_file_per_class(tmp_path, monkeypatch):
    from boa_hip import label_maps, model_store, nifti, plans
    from boa_hip.compute.inference import compute_all_models
    root = tmp_path / "results"
    pj, dj = plans.synthetic_plans(patch=(32, 32, 32), features=(32, 64), num_classes=118, spacing=(6.0, 6.0, 6.0))
    geom = plans.model_config_from_plans(pj, dj).geometry
    model_store.write_model_folder(str(root), 298, "TotalSegmentator_6mm", "nnUNetTrainer_4000epochs_NoMirroring", pj, dj,
                                   [plans.synthetic_state_dict(geom, seed=298)])
    monkeypatch.setenv("nnUNet_results", str(root))
    monkeypatch.delenv("BOA_SAVE_DEVICE", raising=False)
    ct_path, aff = _write_ct(tmp_path)
    plain, split = tmp_path / "plain", tmp_path / "split"
    compute_all_models(ct_path, plain, ["total"], dict(PARAMS))                     # no "ml" key
    compute_all_models(ct_path, split, ["total"], dict(PARAMS, ml=False))
    # the key changes nothing that was written before
    before = sorted(os.listdir(plain))
    assert {"total-measurements.json", "total.nii.gz"} <= set(before) and "total" not in before
    assert sorted(os.listdir(split)) == sorted(before + ["total"])
    for f in before:
        assert (split / f).read_bytes() == (plain / f).read_bytes(), f
    total, taff, _ = nifti.load(split / "total.nii.gz")
    names = label_maps.CLASS_MAP_TOTAL
    assert len(names) == 117 and len(np.unique(total)) > 3
    assert sorted(os.listdir(split / "total")) == sorted(f"{v}.nii.gz" for v in names.values())
    empty = 0
    for k, name in names.items():
        mask, maff, hdr = nifti.load(split / "total" / f"{name}.nii.gz")
        assert mask.dtype == np.uint8 and np.array_equal(maff, taff) and not hdr.extensions
        np.testing.assert_array_equal(mask, (total == k).astype(np.uint8), err_msg=name)
        empty += not mask.any()
    assert 0 < empty < 117                                       # structures without a voxel get their all-zero file
    # "ml": True is the default; roi_subset cuts the directory down to the named classes (here also the volume)
    order = [int(l) for l in np.unique(total) if l]
    subset = [names[order[0]], names[order[-1]]]
    sub = tmp_path / "sub"
    compute_all_models(ct_path, sub, ["total"], dict(PARAMS, ml=False, roi_subset=subset))
    assert sorted(os.listdir(sub / "total")) == sorted(f"{n}.nii.gz" for n in subset)
    stotal = nifti.load(sub / "total.nii.gz")[0]
    for n in subset:
        np.testing.assert_array_equal(nifti.load(sub / "total" / f"{n}.nii.gz")[0], (stotal == label_maps.CLASS_MAP_TOTAL_INV[n]).astype(np.uint8))
    true = tmp_path / "true"
    compute_all_models(ct_path, true, ["total"], dict(PARAMS, ml=True))
    assert sorted(os.listdir(true)) == before
    assert (true / "total.nii.gz").read_bytes() == (plain / "total.nii.gz").read_bytes()


def test_body_with_ml_false_names_what_is_missing(tmp_path):
    from boa_hip.compute.inference import compute_all_models
    ct_path, _ = _write_ct(tmp_path)
    with pytest.raises(NotImplementedError, match="body.nii.gz and skin.nii.gz"):
        compute_all_models(ct_path, tmp_path / "out", ["body"], dict(PARAMS, fastest=False, ml=False))
    assert not any((tmp_path / "out").glob("*.nii.gz"))
