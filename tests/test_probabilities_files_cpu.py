"""The files of `save_probabilities` (boa_hip.task.write_probabilities = export_prediction_from_logits' np.savez_compressed +
save_pickle, NN/inference/export_prediction.py:99-102): key, dtype and shape of the .npz, the four keys of the .pkl, and a second
model's write replacing the first (TS/nnunet.py:286-293).  The keyword exists on every layer that mirrors the reference's."""
import inspect
import pickle

import numpy as np
import pytest

PROPS = {"spacing": [3.0, 1.5, 1.5], "shape_before_cropping": (6, 9, 5), "bbox_used_for_cropping": [[2, 5], [3, 8], [0, 4]],
         "shape_after_cropping_and_before_resampling": (3, 5, 4)}
KEYS = {"spacing", "shape_before_cropping", "bbox_used_for_cropping", "shape_after_cropping_and_before_resampling"}


def _probs(C, shape, seed):
    p = np.random.default_rng(seed).random((C, *shape)).astype(np.float32)
    return p / p.sum(axis=0, keepdims=True)


def test_npz_key_dtype_shape_and_pkl_keys(tmp_path):
    from boa_hip.task import write_probabilities
    path = tmp_path / "s01.npz"
    p = _probs(3, (6, 9, 5), 0)
    write_probabilities(path, p, PROPS)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["s01.npz", "s01.pkl"]          # nothing like s01.npz.npz
    with np.load(path) as z:
        assert z.files == ["probabilities"]
        got = z["probabilities"]
    assert got.dtype == np.float32 and got.shape == (3, 6, 9, 5)
    np.testing.assert_array_equal(got, p)
    with open(tmp_path / "s01.pkl", "rb") as f:
        props = pickle.load(f)
    assert type(props) is dict and set(props) == KEYS
    assert props == PROPS
    # plain types only: the pickle loads without this package, nibabel or SimpleITK
    flat = [props["spacing"], props["shape_before_cropping"], props["shape_after_cropping_and_before_resampling"],
            *props["bbox_used_for_cropping"]]
    assert all(type(v) in (int, float) for seq in flat for v in seq)


def test_a_second_model_overwrites_the_first(tmp_path):
    from boa_hip.task import write_probabilities
    path = str(tmp_path / "prob.npz")                                   # a str path works like a Path
    write_probabilities(path, _probs(25, (4, 5, 6), 1), PROPS)
    second = _probs(3, (4, 5, 6), 2)
    props2 = dict(PROPS, spacing=[1.0, 1.0, 1.0])
    write_probabilities(path, second, props2)
    with np.load(path) as z:
        np.testing.assert_array_equal(z["probabilities"], second)
    with open(tmp_path / "prob.pkl", "rb") as f:
        assert pickle.load(f) == props2
    assert len(list(tmp_path.iterdir())) == 2


def test_only_float32_class_volumes_are_written(tmp_path):
    from boa_hip.task import write_probabilities
    with pytest.raises(ValueError):
        write_probabilities(tmp_path / "a.npz", _probs(3, (4, 5, 6), 0).astype(np.float64), PROPS)
    with pytest.raises(ValueError):
        write_probabilities(tmp_path / "a.npz", _probs(3, (4, 5, 6), 0)[0], PROPS)
    assert not list(tmp_path.iterdir())


def test_the_keyword_is_on_every_mirrored_seam():
    from boa_hip import task
    from boa_hip.predictor import HipPredictor
    assert inspect.signature(HipPredictor.predict_segmentation).parameters["return_probabilities"].default is False
    assert inspect.signature(task.SegmentationTask.predict_image).parameters["save_probabilities"].default is None
    assert inspect.signature(task.run_cascade_task).parameters["save_probabilities"].default is None
    for text in (task.SegmentationTask.predict_image.__doc__,):
        for word in ("overwrites", "s01", "shape_before_cropping", "bbox_used_for_cropping", "spacing",
                     "shape_after_cropping_and_before_resampling", "NotImplementedError"):
            assert word.lower() in text.lower(), word
