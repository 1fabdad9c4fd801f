"""boa_label_blobs6 / boa_label_blobs_filter (csrc/ccl_labels.hip) and boa_hip/blobs.py on the label volumes of tests/blob_cases.py.
Roots, sizes and the component count are compared with the flood fill of tests/blob_reference.py, every filter result with its scipy
restatement of TS/postprocessing.py:13-98 (pinned against the reference's own functions in tests/test_blob_reference_cpu.py).
Integer work: every comparison is bit-exact.  Shapes are [D0][D1][D2], D2 fastest; the kernel's tiles are 16 x 16 x 32."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import blob_cases as BC
import blob_reference as br

pytestmark = pytest.mark.gpu

CM = BC.CLASS_MAP
U32 = 2 ** 32 - 1


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _check(rc, what=""):
    from boa_hip._lib import check
    check(rc, what)


def _label(ctx, arr):
    """(roots, sizes, n_components) of boa_label_blobs6 on a host uint8 array"""
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    d = ctx.from_numpy(a)
    d_r, d_s = ctx.alloc(a.size * 4), ctx.alloc(a.size * 4)
    n = C.c_int(-1)
    try:
        _check(ctx.lib.boa_label_blobs6(ctx.h, d.vp, *a.shape, d_r.vp, d_s.vp, C.byref(n)), "boa_label_blobs6")
        return d_r.download(a.shape, np.int32), d_s.download(a.shape, np.uint32), int(n.value)
    finally:
        for b in (d, d_r, d_s):
            b.free()


def _filter(ctx, arr, modes, lo=0, hi=U32):
    """boa_label_blobs6 + one boa_label_blobs_filter call, through the C ABI"""
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    d = ctx.from_numpy(a)
    d_r, d_s = ctx.alloc(a.size * 4), ctx.alloc(a.size * 4)
    m = np.zeros(256, dtype=np.uint8)
    for v, mode in modes.items():
        m[v] = mode
    try:
        _check(ctx.lib.boa_label_blobs6(ctx.h, d.vp, *a.shape, d_r.vp, d_s.vp, None), "boa_label_blobs6")
        _check(ctx.lib.boa_label_blobs_filter(ctx.h, d_r.vp, d_s.vp, a.size, m.ctypes.data_as(C.c_void_p), lo, hi, d.vp), "boa_label_blobs_filter")
        return d.download(a.shape, np.uint8)
    finally:
        for b in (d, d_r, d_s):
            b.free()


@functools.lru_cache(maxsize=None)
def _flood(name):
    return br.components6(LABEL_CASES[name]())


LABEL_CASES = {
    "noise3": BC.noise3,
    "percolation": BC.percolation,
    "checkerboard": BC.checkerboard,
    "parity12_small": lambda: BC.parity12((18, 19, 38)),
    "parity12_full_tiles": lambda: BC.parity12(BC.CHAIN_SHAPE),
    "serpentine": BC.serpentine,
    "tie_equal": lambda: BC.tie_pair(False),
    "tie_second_larger": lambda: BC.tie_pair(True),
    "sizes567": BC.sizes567,
    "row7": lambda: np.array([[[1, 1, 0, 2, 2, 2, 1]]], dtype=np.uint8),
    "small33": lambda: BC.noise3(seed=2, shape=(3, 2, 33)),
    "zeros": lambda: np.zeros((5, 5, 5), dtype=np.uint8),
    "untouched": BC.untouched,
    "one_solid_tile_and_more": lambda: np.pad(np.full((16, 16, 32), 7, np.uint8), ((0, 3), (0, 2), (0, 5)), constant_values=7),
}
for _ax in range(3):
    for _t in (1, 17):
        LABEL_CASES[f"slabs_axis{_ax}_t{_t}"] = functools.partial(BC.slabs, _ax, _t)


@pytest.mark.parametrize("name", sorted(LABEL_CASES))
def test_roots_sizes_count_equal_flood_fill(ctx, name):
    arr = LABEL_CASES[name]()
    want_roots, want_sizes = _flood(name)
    roots, sizes, n = _label(ctx, arr)
    assert n == len(want_sizes)
    np.testing.assert_array_equal(roots, want_roots.astype(np.int32))
    want = np.zeros(arr.size, dtype=np.uint32)
    for r, c in want_sizes.items():
        want[r] = c
    np.testing.assert_array_equal(sizes.ravel(), want)


def test_component_counts(ctx):
    """6-connected and per label: 14 396 components in the three-label noise (a 26-connected labelling per label finds 489), every
    voxel its own component in the checkerboard and the parity volumes (8 192 per full tile)"""
    assert _label(ctx, BC.noise3())[2] == 14396
    assert _label(ctx, BC.checkerboard())[2] == 6498
    assert _label(ctx, BC.parity12((18, 19, 38)))[2] == 12996
    assert _label(ctx, BC.parity12(BC.CHAIN_SHAPE))[2] == 34 * 35 * 70
    roots, sizes, n = _label(ctx, BC.serpentine())
    assert n == 1 and sizes.ravel()[40] == (BC.serpentine() != 0).sum() and set(np.unique(roots)) == {-1, 40}


def test_noise3_filters(ctx):
    arr = BC.noise3()
    rois = ["l1", "l2", "l3"]
    big = max(_flood("noise3")[1].values())
    for lo in (0, 1, 3, big, big - 1):
        got = _filter(ctx, arr, {1: 1, 2: 1, 3: 1}, lo, U32)
        np.testing.assert_array_equal(got, br.remove_small_blobs_multilabel(arr, CM, rois, [lo, 1e10]), err_msg=f"lo {lo}")
        if lo == 0:
            np.testing.assert_array_equal(got, arr)
        if lo == big:
            assert not got.any()
        if lo == big - 1:
            assert got.any()
    np.testing.assert_array_equal(_filter(ctx, arr, {1: 2, 2: 2, 3: 2}), br.keep_largest_blob_multilabel(arr, CM, rois))
    # modes mixed in one call: keep largest of 1, interval on 2, 3 alone
    want = br.remove_small_blobs_multilabel(br.keep_largest_blob_multilabel(arr, CM, ["l1"]), CM, ["l2"], [2, 5])
    np.testing.assert_array_equal(_filter(ctx, arr, {1: 2, 2: 1}, 2, 5), want)
    np.testing.assert_array_equal(want == 3, arr == 3)


def test_percolation_filters(ctx):
    """one blob of thousands of voxels across many tiles among ~5 000 small ones"""
    from boa_hip import blobs
    arr = BC.percolation()
    sizes = _flood("percolation")[1]
    assert max(sizes.values()) > 3000 and len(sizes) > 5000
    want = br.keep_largest_blob_multilabel(arr, CM, ["l4"])
    assert int((want != 0).sum()) == max(sizes.values())
    np.testing.assert_array_equal(blobs.keep_largest_blob_multilabel(ctx, arr, CM, ["l4"]), want)
    np.testing.assert_array_equal(blobs.keep_largest_blob(ctx, arr), br.keep_largest_blob(arr != 0))
    want = br.remove_small_blobs_multilabel(arr, CM, ["l4"], [10, 30])
    assert want.any() and (want != arr).any()
    np.testing.assert_array_equal(blobs.remove_small_blobs_multilabel(ctx, arr, CM, ["l4"]), want)           # the default [10, 30]
    np.testing.assert_array_equal(blobs.remove_small_blobs(ctx, arr), br.remove_small_blobs(arr != 0, [10, 30]))
    np.testing.assert_array_equal(blobs.remove_small_blobs(ctx, arr, [3, 1e10]), br.remove_small_blobs(arr != 0, [3, 1e10]))


@pytest.mark.parametrize("name", ["checkerboard", "parity12_small", "parity12_full_tiles"])
def test_one_voxel_components(ctx, name):
    """edge and corner contacts do not join; keep-largest keeps the very first voxel of each label; lo = 1 removes everything"""
    arr = LABEL_CASES[name]()
    labels = [int(v) for v in np.unique(arr) if v]
    rois = [CM[v] for v in labels]
    got = _filter(ctx, arr, {v: 2 for v in labels})
    np.testing.assert_array_equal(got, br.keep_largest_blob_multilabel(arr, CM, rois))
    assert int((got != 0).sum()) == len(labels) and got.ravel()[0] == arr.ravel()[0]
    assert not _filter(ctx, arr, {v: 1 for v in labels}, 1, U32).any()
    np.testing.assert_array_equal(_filter(ctx, arr, {v: 1 for v in labels}, 0, U32), arr)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("thickness", [1, 17])
def test_slabs(ctx, axis, thickness):
    """different labels in contact never merge; equal labels across a tile face do (thickness 17 crosses the 16 / 32 voxel faces)"""
    arr = BC.slabs(axis, thickness)
    roots, sizes, n = _label(ctx, arr)
    assert n == -(-arr.shape[axis] // thickness)
    slab = arr.size // arr.shape[axis] * thickness
    np.testing.assert_array_equal(_filter(ctx, arr, {1: 2, 2: 2}), br.keep_largest_blob_multilabel(arr, CM, ["l1", "l2"]))
    got = _filter(ctx, arr, {1: 1, 2: 1}, slab - 1, U32)
    np.testing.assert_array_equal(got, br.remove_small_blobs_multilabel(arr, CM, ["l1", "l2"], [slab - 1, 1e10]))
    assert got.any()


def test_serpentine(ctx):
    from boa_hip import blobs
    arr = BC.serpentine()
    np.testing.assert_array_equal(blobs.keep_largest_blob_multilabel(ctx, arr, CM, ["l5"]), arr)
    assert not blobs.remove_small_blobs_multilabel(ctx, arr, CM, ["l5"], [10, 30]).any()          # one blob, larger than hi
    cut = arr.copy()
    cut[16, 34, 35] = 0                      # the chain cut in a row of plane 16: two blobs of different sizes
    np.testing.assert_array_equal(blobs.keep_largest_blob_multilabel(ctx, cut, CM, ["l5"]), br.keep_largest_blob_multilabel(cut, CM, ["l5"]))


def test_tie_of_the_largest_blob(ctx):
    """raster order is not tile order: of two equal blobs the one met first in raster order stays; one voxel more wins"""
    from boa_hip import blobs
    eq, gt = BC.tie_pair(False), BC.tie_pair(True)
    got = blobs.keep_largest_blob_multilabel(ctx, eq, CM, ["l3"])
    np.testing.assert_array_equal(got, br.keep_largest_blob_multilabel(eq, CM, ["l3"]))
    assert got[0, 20, 0] == 3 and got[1, 0, 0] == 0
    got = blobs.keep_largest_blob_multilabel(ctx, gt, CM, ["l3"])
    np.testing.assert_array_equal(got, br.keep_largest_blob_multilabel(gt, CM, ["l3"]))
    assert got[0, 20, 0] == 0 and got[1, 0, 0] == 3
    np.testing.assert_array_equal(blobs.keep_largest_blob(ctx, eq), br.keep_largest_blob(eq != 0))
    # the array order decides: the same volume seen with its first two axes swapped (a non-contiguous view, made contiguous in ITS order)
    v = eq.transpose(1, 0, 2)
    assert not v.flags.c_contiguous
    got = blobs.keep_largest_blob_multilabel(ctx, v, CM, ["l3"])
    np.testing.assert_array_equal(got, br.keep_largest_blob_multilabel(v, CM, ["l3"]))
    assert got[0, 1, 0] == 3 and got[20, 0, 0] == 0


def test_thresholds_at_the_edge(ctx):
    from boa_hip import blobs
    arr = BC.sizes567()
    for lo, left in ((5.999, 13), (6.0, 7), (4.999, 18), (7, 0)):
        got = blobs.remove_small_blobs_multilabel(ctx, arr, CM, ["l2"], [lo, 1e10])
        np.testing.assert_array_equal(got, br.remove_small_blobs_multilabel(arr, CM, ["l2"], [lo, 1e10]))
        assert int((got != 0).sum()) == left
    got = blobs.remove_small_blobs_multilabel(ctx, arr, CM, ["l2"], [5, 6])         # 5 is too small, 7 too large
    np.testing.assert_array_equal(got, br.remove_small_blobs_multilabel(arr, CM, ["l2"], [5, 6]))
    assert int((got != 0).sum()) == 6
    got = blobs.remove_small_blobs_multilabel(ctx, arr, CM, ["l2"], [5.0, 6.999])
    assert int((got != 0).sum()) == 6


@pytest.mark.parametrize("name", ["row7", "small33", "zeros"])
def test_volumes_below_one_tile(ctx, name):
    from boa_hip import blobs
    arr = LABEL_CASES[name]()
    rois = ["l1", "l2", "l3"]
    np.testing.assert_array_equal(blobs.keep_largest_blob_multilabel(ctx, arr, CM, rois), br.keep_largest_blob_multilabel(arr, CM, rois))
    np.testing.assert_array_equal(blobs.remove_small_blobs_multilabel(ctx, arr, CM, rois, [1, 1e10]),
                                  br.remove_small_blobs_multilabel(arr, CM, rois, [1, 1e10]))
    if not arr.any():          # no foreground: the data comes back unchanged
        assert blobs.keep_largest_blob(ctx, arr) is arr and blobs.remove_small_blobs(ctx, arr) is arr
        assert _label(ctx, arr)[2] == 0


def test_labels_outside_rois_are_untouched(ctx):
    from boa_hip import blobs
    arr = BC.untouched()
    for got, want in ((blobs.keep_largest_blob_multilabel(ctx, arr, CM, ["l1", "l2"]), br.keep_largest_blob_multilabel(arr, CM, ["l1", "l2"])),
                      (blobs.remove_small_blobs_multilabel(ctx, arr, CM, ["l1", "l2"], [4, 1e10]),
                       br.remove_small_blobs_multilabel(arr, CM, ["l1", "l2"], [4, 1e10]))):
        np.testing.assert_array_equal(got, want)
        for v in (9, 255):
            np.testing.assert_array_equal(got == v, arr == v)
        assert (got != arr).any()
    np.testing.assert_array_equal(_filter(ctx, arr, {}, 1000, 0), arr)          # host_mode of all zeros changes nothing
    # label 255 filtered on its own
    np.testing.assert_array_equal(blobs.remove_small_blobs_multilabel(ctx, arr, CM, ["l255"], [2, 1e10]),
                                  br.remove_small_blobs_multilabel(arr, CM, ["l255"], [2, 1e10]))


def test_devarray_in_and_out(ctx):
    """a DevArray is filtered in place and returned; a non-contiguous device view is made contiguous in its own axis order"""
    from boa_hip import blobs
    from boa_hip.devarray import DevArray
    arr = BC.noise3()
    d = DevArray.from_numpy(ctx, arr)
    try:
        assert blobs.remove_small_blobs_multilabel(ctx, d, CM, ["l1", "l3"], [3, 1e10]) is d
        np.testing.assert_array_equal(d.download(), br.remove_small_blobs_multilabel(arr, CM, ["l1", "l3"], [3, 1e10]))
    finally:
        d.free()
    eq = BC.tie_pair(False)
    d = DevArray.from_numpy(ctx, eq)
    try:
        v = d.transpose((1, 0, 2))
        blobs.keep_largest_blob_multilabel(ctx, v, CM, ["l3"])
        np.testing.assert_array_equal(d.download().transpose(1, 0, 2), br.keep_largest_blob_multilabel(eq.transpose(1, 0, 2), CM, ["l3"]))
    finally:
        d.free()
    d = DevArray.from_numpy(ctx, BC.percolation())
    try:
        assert blobs.keep_largest_blob(ctx, d) is d
        np.testing.assert_array_equal(d.download(), br.keep_largest_blob(BC.percolation() != 0))
    finally:
        d.free()


def test_body_postprocessing_on_the_reference_output(ctx):
    """tests/golden/ref_example_ct_sm_T300_output.nii.gz is the reference's OWN output of task body at 6 mm (one blob of 239 392 voxels):
    the body post-processing is the identity on it.  With 40 seeded specks of body_extremities the ones of at most 231 voxels
    (50 000 mm^3 at 6 mm) go and the others stay."""
    from boa_hip import blobs, label_maps, nifti
    body = nifti.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_example_ct_sm_T300_output.nii.gz"))[0]
    body = np.ascontiguousarray(body, dtype=np.uint8)
    assert body.shape == (122, 101, 30) and int((body == 1).sum()) == 239392
    cm = label_maps.class_map("body")
    zooms = (6.0, 6.0, 6.0)
    lo, hi = blobs.interval_bounds([blobs.size_threshold_voxels(50000, zooms), 1e10])
    assert (lo, hi) == (231, U32)

    def device(a):
        out = blobs.keep_largest_blob_multilabel(ctx, a, cm, ["body_trunc"])
        return blobs.remove_small_blobs_multilabel(ctx, out, cm, ["body_extremities"], [blobs.size_threshold_voxels(50000, zooms), 1e10])

    np.testing.assert_array_equal(device(body), body)
    specks = BC.body_specks(body)
    want = br.body_postprocessing(specks, zooms)
    got = device(specks)
    np.testing.assert_array_equal(got, want)
    sz = np.array(list(br.components6((specks == 2) * np.uint8(2))[1].values()))
    assert (sz <= 231).any() and (sz > 231).any()
    assert int((got == 2).sum()) == int(sz[sz > 231].sum()) and np.array_equal(got == 1, body == 1)
    # one labelling, the reference's three steps as filter calls (what SegmentationTask.predict_image runs)
    from boa_hip.devarray import DevArray
    d = DevArray.from_numpy(ctx, specks)
    lab = blobs.BlobLabelling(ctx, d, count=True)
    try:
        assert lab.n_components == 1 + len(sz)
        lab.filter(blobs.modes_for(cm, ["body_trunc"], blobs.MODE_LARGEST))
        lab.filter(blobs.modes_for(cm, ["body_extremities"], blobs.MODE_INTERVAL), lo, hi)
        lo2, hi2 = blobs.interval_bounds([blobs.size_threshold_voxels(200, zooms), 1e10])
        lab.filter(blobs.modes_for(cm, list(cm.values()), blobs.MODE_INTERVAL), lo2, hi2)
        np.testing.assert_array_equal(d.download(), br.body_postprocessing(specks, zooms, remove_small=True))
    finally:
        lab.free()
        d.free()


def test_bad_arguments_are_named(ctx):
    """bad dimensions and null pointers: BOA_EINVAL, boa_last_error names the argument; nothing is launched"""
    from boa_hip._lib import BOA_EINVAL
    lib = ctx.lib
    d = ctx.from_numpy(np.zeros(64, np.uint8))
    d_r, d_s = ctx.alloc(256), ctx.alloc(256)
    modes = np.zeros(256, np.uint8)
    mp = modes.ctypes.data_as(C.c_void_p)

    def err():
        return lib.boa_last_error().decode()

    try:
        for args, word in (((None, 4, 4, 4, d_r.vp, d_s.vp, None), "dev_labels"), ((d.vp, 4, 4, 4, None, d_s.vp, None), "dev_roots"),
                           ((d.vp, 4, 4, 4, d_r.vp, None, None), "dev_sizes"), ((d.vp, 0, 4, 4, d_r.vp, d_s.vp, None), "D0"),
                           ((d.vp, 4, -1, 4, d_r.vp, d_s.vp, None), "D1"), ((d.vp, 4, 4, 0, d_r.vp, d_s.vp, None), "D2"),
                           ((d.vp, 70000, 1, 1, d_r.vp, d_s.vp, None), "D0"), ((d.vp, 2048, 2048, 512, d_r.vp, d_s.vp, None), "too large")):
            assert lib.boa_label_blobs6(ctx.h, *args) == BOA_EINVAL
            assert "boa_label_blobs6" in err() and word in err(), err()
        assert lib.boa_label_blobs6(None, d.vp, 4, 4, 4, d_r.vp, d_s.vp, None) == BOA_EINVAL and "ctx" in err()
        for args, word in (((None, d_s.vp, 64, mp, 0, 0, d.vp), "dev_roots"), ((d_r.vp, None, 64, mp, 0, 0, d.vp), "dev_sizes"),
                           ((d_r.vp, d_s.vp, 64, None, 0, 0, d.vp), "host_mode"), ((d_r.vp, d_s.vp, 64, mp, 0, 0, None), "dev_labels_inout"),
                           ((d_r.vp, d_s.vp, 2 ** 31, mp, 0, 0, d.vp), "n too large")):
            assert lib.boa_label_blobs_filter(ctx.h, *args) == BOA_EINVAL
            assert "boa_label_blobs_filter" in err() and word in err(), err()
        modes[7] = 3
        assert lib.boa_label_blobs_filter(ctx.h, d_r.vp, d_s.vp, 64, mp, 0, 0, d.vp) == BOA_EINVAL and "host_mode[7]" in err()
        assert lib.boa_label_blobs_filter(None, d_r.vp, d_s.vp, 64, mp, 0, 0, d.vp) == BOA_EINVAL and "ctx" in err()
        with pytest.raises(ValueError):
            from boa_hip import blobs
            blobs.remove_small_blobs_multilabel(ctx, np.full((2, 2, 2), 300, np.int32), CM, ["l1"])
    finally:
        for b in (d, d_r, d_s):
            b.free()
