"""tests/blob_reference.py (the scipy restatement the GPU blob tests compare against) equals what the reference's own functions
returned (tests/golden/g16_blobs.npz, recorded by tests/golden/make_golden_blobs.py), the flood fill agrees with scipy's per-label
labelling, and the float32 threshold arithmetic of TS/nnunet.py:601-616 gives the documented voxel counts.  nibabel is not
available here: the threshold line is pinned against numpy float32 arithmetic only."""
import math
import os

import numpy as np
import pytest
from scipy import ndimage

import blob_cases
import blob_reference as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_blobs.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def reference_call(arr, fn, kw):
    if fn.endswith("_multilabel"):
        return np.asarray(getattr(br, fn)(arr.copy(), blob_cases.CLASS_MAP, **kw))
    return np.asarray(getattr(br, fn)(arr != 0, **kw))


CASES = blob_cases.golden_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_blob_reference_equals_golden(golden, name):
    arr, calls = CASES[name]
    assert np.array_equal(arr, golden[f"{name}.input"]), "the case generator changed: regenerate the golden"
    for k, (fn, kw) in enumerate(calls):
        want = golden[blob_cases.call_key(name, k, fn)]
        got = reference_call(arr, fn, kw)
        assert got.shape == want.shape
        assert np.array_equal(got.astype(np.uint8), want), (name, fn, kw)


def test_golden_cases_are_not_trivial(golden):
    """the recorded filters removed something where the case says so, and kept what they must"""
    k = golden[blob_cases.call_key("tie_equal", 0, "keep_largest_blob_multilabel")]
    assert k[0, 20, 0] == 3 and k[1, 0, 0] == 0                        # the first of two equal blobs stays
    k = golden[blob_cases.call_key("tie_second_larger", 0, "keep_largest_blob_multilabel")]
    assert k[0, 20, 0] == 0 and k[1, 0, 0] == 3
    s = [golden[blob_cases.call_key("sizes567", j, "remove_small_blobs_multilabel")] for j in range(3)]
    assert [int((a != 0).sum()) for a in s] == [13, 7, 18]             # lo 5.999: 5 goes; 6.0: 5 and 6 go; 4.999: nothing
    u_in = golden["untouched.input"]
    for j, fn in enumerate(("keep_largest_blob_multilabel", "remove_small_blobs_multilabel")):
        u = golden[blob_cases.call_key("untouched", j, fn)]
        for v in (9, 255):
            assert np.array_equal(u == v, u_in == v)
        assert (u != u_in).any()


@pytest.mark.parametrize("name", ["noise3", "percolation", "checkerboard", "parity12", "serpentine", "untouched", "row7"])
def test_flood_fill_equals_scipy_per_label(name):
    arr = CASES[name][0]
    roots, sizes = br.components6(arr)
    n = 0
    for v in np.unique(arr):
        if not v:
            continue
        lab, k = ndimage.label(arr == v)
        n += k
        first = ndimage.minimum(np.arange(arr.size).reshape(arr.shape), lab, index=np.arange(1, k + 1)).astype(np.int64)
        assert np.array_equal(roots[lab > 0], first[lab[lab > 0] - 1])          # scipy numbers components by their first voxel
        assert np.all(np.diff(first) > 0)
        cnt = np.bincount(lab.ravel())[1:]
        assert all(sizes[int(r)] == int(c) for r, c in zip(first, cnt))
    assert n == len(sizes)
    assert np.array_equal(roots < 0, arr == 0)


def test_component_counts_of_the_cases():
    assert len(br.components6(blob_cases.noise3())[1]) == 14396
    assert len(br.components6(blob_cases.checkerboard())[1]) == 6498
    assert len(br.components6(blob_cases.parity12((18, 19, 38)))[1]) == 12996
    r, s = br.components6(blob_cases.serpentine())
    assert list(s) == [40] and s[40] == int((blob_cases.serpentine() != 0).sum())


@pytest.mark.parametrize("zooms,thr,want", [((1.5, 1.5, 1.5), 200, 59), ((1.5, 1.5, 1.5), 50000, 14814), ((6.0, 6.0, 6.0), 50000, 231),
                                            ((1.2, 1.2, 2.0), 200, 69), ((1.0, 1.0, 1.0), 200, 200), ((2.0, 2.0, 2.0), 200, 25)])
def test_size_threshold_in_voxels(zooms, thr, want):
    """blobs of at most floor(thr / vox_vol) voxels are removed; at 1 mm and 2 mm the quotient is an integer, so a blob of exactly
    200 (25) voxels goes"""
    from boa_hip import blobs
    q = blobs.size_threshold_voxels(thr, zooms)
    assert isinstance(q, np.float32)
    ref = br.size_threshold_voxels(thr, zooms)
    assert type(ref) is np.float32 and q == ref
    lo, hi = blobs.interval_bounds([q, 1e10])
    assert lo == want == math.floor(float(ref)) and hi == 2 ** 32 - 1


def test_interval_bounds():
    from boa_hip import blobs
    assert blobs.interval_bounds([10, 30]) == (10, 30)
    assert blobs.interval_bounds([5.999, 6.0]) == (5, 6)
    assert blobs.interval_bounds([-3.5, 29.9]) == (0, 29)
    assert blobs.interval_bounds([0, 1e10]) == (0, 2 ** 32 - 1)
    assert blobs.interval_bounds([0, -1]) == (2 ** 32 - 1, 2 ** 32 - 1)     # count > -1 always: everything goes


def test_task_tables_know_body():
    from boa_hip import label_maps, model_store
    assert label_maps.class_map("body") == {1: "body_trunc", 2: "body_extremities"}
    assert model_store.TASKS["body"]["task_id"] == [299] and model_store.TASKS["body"]["resample"] == 1.5
    assert model_store.TASKS["body_fast"]["task_id"] == [300] and model_store.TASKS["body_fast"]["resample"] == 6.0
    for k in ("body", "body_fast"):
        assert model_store.TASKS[k]["trainer"] == "nnUNetTrainer" and model_store.TASKS[k]["folds"] == [0]
