"""Pins tests/resample_cases.py, the numpy side of tests/test_gpu_resample_edges.py: every generator against the property it
states, every reference one-liner against scipy or the oracle.  No device."""
import numpy as np
import pytest
from scipy import ndimage

import resample_cases as R

F64, F32, F16 = np.float64, np.float32, np.float16


@pytest.mark.parametrize("pair", R.HALF_PAIRS, ids=lambda p: f"{p[0]:g}")
def test_half_pairs_round_differently_once_and_twice(pair):
    """0.75 a + 0.25 b rounds to one half directly and to its neighbour through float32, and class 1 sits on the larger of the
    two: the oracle's labels (one rounding, numpy's float64 -> float16) differ from the twice-rounded ones at output plane 1,
    in all three arrangements, and `skimage_resize_explicit` (the kernels' blueprint) has the oracle's bits."""
    from oracle import labels as olab
    from oracle import nnunet_resample as nnr
    a, b, c1 = pair
    t = F64(0.75) * F64(a) + F64(0.25) * F64(b)
    once, twice = t.astype(F16), t.astype(F32).astype(F16)
    assert once != twice
    assert abs(float(once) - float(twice)) == float(np.spacing(min(abs(once), abs(twice))))     # neighbouring halves
    assert c1 == float(max(once, twice))
    arrs = R.half_rounding_case(pair)
    assert [x["axis"] for x in arrs] == [-1, 0, 2]
    for arr in arrs:
        assert arr["logits"].dtype == F16
        want16 = R.oracle_logits(arr)
        assert want16.dtype == F16 and want16.shape == (2, *arr["out"])
        exact = R.oracle_logits(arr, F64)
        line = [slice(None)] * 3
        line[arr["resized"]] = 1
        assert (exact[0][tuple(line)] == t).all()                                                # the planted value, unrounded
        assert (want16[0][tuple(line)] == once).all()
        lab_once = olab.argmax_labels(want16)
        lab_twice = olab.argmax_labels(exact.astype(F32).astype(F16))
        want_once, want_twice = (0, 1) if once > twice else (1, 0)
        assert (lab_once[tuple(line)] == want_once).all() and (lab_twice[tuple(line)] == want_twice).all()
        line[arr["resized"]] = 0
        assert (lab_once[tuple(line)] == lab_twice[tuple(line)]).all()                           # plane 0 is no tie: a against c1
        if arr["axis"] < 0:
            ex = np.stack([nnr.skimage_resize_explicit(arr["logits"][c].astype(F64), arr["out"], 1) for c in range(2)])
            np.testing.assert_array_equal(ex.astype(F16).view(np.uint16), want16.view(np.uint16))


def test_issue_case_values():
    """the first pair is the issue's: labels [0, 0, 1, 1] along axis 0, class 0 = [1366, 1025, 341.5, 2^-24]"""
    from oracle import labels as olab
    arr = R.half_rounding_case()[0]
    assert arr["logits"].shape == (2, 2, 3, 3) and arr["out"] == (4, 3, 3)
    want = R.oracle_logits(arr)
    np.testing.assert_array_equal(olab.argmax_labels(want)[:, 1, 1], [0, 0, 1, 1])
    np.testing.assert_array_equal(want[0, :, 1, 1], np.array([1366, 1025, 341.5, 2.0 ** -24], F16))
    assert (want[1] == 1025).all()


def test_nearest_index_is_scipy_order0():
    x = {n: (np.arange(n) % 251).astype(np.uint8) for n in R.NEAREST_IN}
    bad = 0
    for n_in in R.NEAREST_IN:
        for n_out in R.NEAREST_OUT:
            ref = ndimage.zoom(x[n_in], R.zoom_of(n_in, n_out), order=0, mode="nearest")
            idx = R.nearest_index(n_in, n_out)
            assert idx.shape == (n_out,) and idx.min() >= 0 and idx.max() <= n_in - 1
            bad += int(ref.shape != (n_out,) or (x[n_in][idx] != ref).any())
    assert bad == 0
    assert list(R.NEAREST_IN) == list(range(1, 40)) and list(R.NEAREST_OUT) == list(range(1, 60))
    # exact halves occur and go UP (floor(c + 0.5)), where round-half-even would go down: 3 -> 5 samples, c = 0.5 -> 1, 2.5 -> 3... clamped
    assert list(R.nearest_index(3, 5)) == [0, 1, 1, 2, 2]
    assert list(R.nearest_index(2, 3)) == [0, 1, 1]
    assert list(np.rint(np.arange(3) * 0.5).astype(int)) == [0, 0, 1]


def test_zoom_shapes_of_every_pair_used():
    pairs = R.all_zoom_shape_pairs()
    assert len(pairs) > 2000 and (1, 1) in pairs and (39, 59) in pairs and (47, 43) in pairs and (2, 1) in pairs
    assert [p for p in pairs if R.zoomed_len(*p) != p[1]] == []
    # scipy agrees with zoomed_len on whole shapes
    for i, o in [R.CUBIC_GEOMETRY["out1_all"], R.CUBIC_GEOMETRY["up8"], R.contig_cases(2)[0], R.contig_cases(33)[3]]:
        assert ndimage.zoom(np.zeros(i), R.zoom_tuple(i, o), order=3, mode="nearest").shape == o


def test_past_extent_pairs():
    pairs = R.past_extent_pairs()
    assert pairs and (47, 43) in pairs
    for n_in, n_out in pairs:
        assert 2 <= n_in <= 64 and 2 <= n_out <= 96
        last = F64(n_out - 1) * (F64(n_in - 1) / F64(n_out - 1))
        assert last == np.nextafter(F64(n_in - 1), np.inf)                                       # exactly one ulp
    assert (46, 43) not in pairs
    cases = R.past_extent_cases()
    assert len(cases) == 3 * len(pairs)
    for ax in range(3):
        assert {(i[ax], o[ax]) for i, o in cases[ax::3]} == set(pairs)


def test_contiguous_lengths_cover_every_residue():
    t = R.contig_residue_table()
    assert sorted(t) == list(range(8)) and min(len(v) for v in t.values()) >= 4
    for z in R.CONTIG_LENGTHS:
        cases = R.contig_cases(z)
        assert all(i == (*R.LEAD, z) for i, _ in cases)
        assert {o[2] < z for _, o in cases} == {True, False}                                     # down and up
        assert {o[:2] == R.LEAD for _, o in cases} == {True, False}                              # leading dims kept / resized
        assert all(min(o) >= 1 for _, o in cases)


def test_amplitude_regimes():
    n = R.amplitude_volume((3, 5, 17), "noise", 1)
    s = R.amplitude_volume((3, 5, 17), "step", 1)
    assert n.dtype == s.dtype == F64 and 300 < n.std() < 500
    assert set(np.unique(s)) == {-30000.0, 30000.0}
    over = ndimage.zoom(s, (1, 1, 35 / 17), order=3, mode="nearest")
    assert (np.abs(over) > 31000).sum() > 20                                                     # the clip of the skimage call is active


def test_slice_range_volume_ranges_differ_by_slice():
    for shape, _, axis in R.SLICE_CLIP_CASES:
        x = R.slice_range_volume(shape, axis, 3)
        assert x.dtype == F32 and x.shape == shape
        other = tuple(a for a in range(3) if a != axis)
        lo, hi = x.min(axis=other), x.max(axis=other)
        for s in range(1, shape[axis]):
            assert lo[s] != lo[s - 1] and hi[s] != hi[s - 1]
        if np.prod(shape) > 100:
            mean = x.mean(axis=other)
            assert ((mean > 0) == (np.arange(shape[axis]) % 2 == 0)).all()                       # the offsets alternate in sign
    axes = {(a, i[a] == o[a]) for i, o, a in R.SLICE_CLIP_CASES}
    assert axes == {(a, same) for a in range(3) for same in (True, False)}
    assert any(i[a] == 1 for i, _, a in R.SLICE_CLIP_CASES)
    sizes = [int(np.prod(i)) for i, _, _ in R.SLICE_CLIP_CASES]
    assert any(n < 8 for n in sizes) and any(n > 8 and n % 8 for n in sizes)
    for i, _, a in R.SLICE_CLIP_CASES:
        if a == 2 and i[2] > 1:
            assert i[2] % 8 != 0
        assert all(i[d] >= 2 for d in range(3) if d != a)                                        # a resized axis needs two samples


def test_slice_clip_bites():
    """the unclipped per-slice result, clipped with the PREVIOUS slice's range, differs from the right clip at most voxels"""
    shape, new_shape, axis = R.SLICE_CLIP_CASES[0]
    assert axis == 0 and shape[0] == new_shape[0]
    x = R.slice_range_volume(shape, axis, 3).astype(F64)
    differ = total = 0
    for s in range(1, shape[0]):
        u = ndimage.zoom(x[s], [o / i for o, i in zip(new_shape[1:], shape[1:])], order=3, mode="nearest", grid_mode=True)
        differ += int((np.clip(u, x[s].min(), x[s].max()) != np.clip(u, x[s - 1].min(), x[s - 1].max())).sum())
        total += u.size
    assert total > 1000 and differ > total // 2


def test_ct_normalize_ref_matches_oracle():
    from oracle import labels as olab
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(4000) * 600).astype(np.int16)
    want = olab.ct_normalize(x, 40.25, 310.5, -900.0, 1200.0)
    got = R.ct_normalize_ref(x, 40.25, 310.5, -900.0, 1200.0)
    assert got.dtype == F32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    for sd in (0.0, 1e-9):
        got = R.ct_normalize_ref(x, 40.25, sd, -900.0, 1200.0)
        np.testing.assert_array_equal(got.view(np.uint32), olab.ct_normalize(x, 40.25, sd, -900.0, 1200.0).view(np.uint32))
        assert np.isfinite(got).all() and np.abs(got).max() > 1e10
    big = np.array([2 ** 24 + 1, -(2 ** 24) - 3, 2 ** 30 - 1], np.int32)
    assert (big.astype(F32).astype(np.int64) != big).all()                                       # the conversion rounds
