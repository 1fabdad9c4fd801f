"""CPU: the host side of `roi_subset` (TS/python_api.py:655-664,168-189; TS/nnunet.py:388-390,519-531): part selection on the real
class-map tables, the label table of the filter, partial model loading, the parameter refusals and the fast / fastest resolution."""
import numpy as np
import pytest


def test_parts_for_roi_subset_on_the_real_tables():
    from boa_hip import label_maps as L
    assert L.parts_for_roi_subset(["liver"]) == [291]
    assert L.parts_for_roi_subset(["liver", "heart"]) == [291, 293]
    assert L.parts_for_roi_subset(["heart", "liver"]) == [291, 293]                      # part order, not the order of the names
    assert L.parts_for_roi_subset(["vertebrae_L3", "rib_left_4"]) == [292, 295]
    assert L.parts_for_roi_subset(["spleen", "kidney_left", "pancreas"]) == [291]
    assert L.parts_for_roi_subset([]) == []
    assert L.parts_for_roi_subset(L.TOTAL_NAMES) == list(L.PART_TASK_IDS)
    # every structure of `total` lives in exactly one part
    for name in L.TOTAL_NAMES:
        assert len(L.parts_for_roi_subset([name])) == 1, name


def test_unknown_names_raise_and_are_named():
    from boa_hip import label_maps as L
    with pytest.raises(KeyError, match="livr"):
        L.parts_for_roi_subset(["liver", "livr"])
    with pytest.raises(KeyError, match="body_trunc"):
        L.parts_for_roi_subset(["body_trunc"])                                           # a structure of another task


def test_subset_lut_is_the_isin_filter():
    from boa_hip import label_maps as L
    names = ["liver", "heart", "rib_right_12"]
    lut = L.subset_lut(names)
    ids = [L.CLASS_MAP_TOTAL_INV[n] for n in names]
    img = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(lut[img], img * np.isin(img, ids))
    assert lut.dtype == np.uint8 and lut.shape == (256,) and not L.subset_lut([]).any()


def test_parameter_refusals(tmp_path):
    """the reference's checks (TS/python_api.py:661-664) come before anything touches a device or a model folder"""
    from boa_hip.compute.inference import _segment_one
    for bad in ("liver", ("liver",), {"liver"}):
        with pytest.raises(ValueError, match="^roi_subset must be a list of strings$"):
            _segment_one(None, "total", None, None, None, tmp_path, False, True, {"roi_subset": bad})
    with pytest.raises(ValueError, match="^roi_subset must be a list of strings$"):
        _segment_one(None, "total", None, None, None, tmp_path, False, True, {"roi_subset_robust": "liver"})
    for task in ("body", "lung_vessels"):
        with pytest.raises(ValueError, match="^roi_subset only works with task 'total' or 'total_mr'$"):
            _segment_one(None, task, None, None, None, tmp_path, False, True, {"roi_subset": ["liver"]})
    assert not list(tmp_path.iterdir())


def test_fast_and_fastest_resolution():
    from boa_hip import model_store
    from boa_hip.compute.inference import total_model_key
    assert total_model_key(False, False) == "total" and model_store.TASKS["total"]["task_id"] == [291, 292, 293, 294, 295]
    assert total_model_key(True, False) == "total_fast" and total_model_key(True, True) == "total_fast"       # fast wins
    assert total_model_key(False, True) == "total_6mm"
    assert (model_store.TASKS["total_fast"]["task_id"], model_store.TASKS["total_fast"]["resample"]) == ([297], 3.0)
    assert (model_store.TASKS["total_6mm"]["task_id"], model_store.TASKS["total_6mm"]["resample"]) == ([298], 6.0)


def test_load_task_models_reads_only_the_selected_parts(tmp_path):
    from boa_hip import label_maps, model_store, plans
    selected = label_maps.parts_for_roi_subset(["liver", "heart"])
    for tid in selected:                                        # the other parts have no folder at all
        pj, dj = plans.synthetic_plans(patch=(16, 16, 16), features=(8, 16), num_classes=3)
        geom = plans.model_config_from_plans(pj, dj).geometry
        model_store.write_model_folder(str(tmp_path), tid, f"part{tid}", "nnUNetTrainerNoMirroring", pj, dj, [plans.synthetic_state_dict(geom, seed=tid)])
    got = model_store.load_task_models("total", root=str(tmp_path), task_ids=selected)
    assert [m[0] for m in got] == [291, 293]
    assert [m[0] for m in model_store.load_task_models("total", root=str(tmp_path), task_ids=[293, 291])] == [291, 293]   # the task's order
    with pytest.raises(RuntimeError):
        model_store.load_task_models("total", root=str(tmp_path))                 # all five: 292 is missing
    with pytest.raises(ValueError, match="297"):
        model_store.load_task_models("total", root=str(tmp_path), task_ids=[297])
    assert model_store.load_task_models("total", root=str(tmp_path), task_ids=[]) == []


def test_sharded_tasks_refuse_the_options():
    """predict_image checks before it touches the data"""
    from boa_hip.task import SegmentationTask
    t = SegmentationTask.__new__(SegmentationTask)
    t.shard, t.model_shard = object(), None
    with pytest.raises(NotImplementedError, match="roi_subset"):
        t.predict_image(None, None, roi_subset=["liver"])
    with pytest.raises(NotImplementedError, match="statistics"):
        t.predict_image(None, None, statistics_out={})
