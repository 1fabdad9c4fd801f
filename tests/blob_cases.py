"""The label volumes of the blob-filter tests (tests/test_gpu_label_blobs.py, tests/test_blob_reference_cpu.py) and the filter calls
recorded from the reference in tests/golden/g16_blobs.npz (tests/golden/make_golden_blobs.py).  Shapes are [D0][D1][D2], D2 fastest;
the labelling kernel works on tiles of 16 x 16 x 32 voxels in that order.  Everything is built from seeds: no files."""
import numpy as np

NOISE_SHAPE = (37, 21, 70)      # ragged tile remainders on all axes
CHAIN_SHAPE = (34, 35, 70)      # 3 x 3 x 3 tiles, the last of each axis partial


def noise3(seed=11, density=0.55, shape=NOISE_SHAPE):
    """three-label noise: 14 396 components (4 712 + 4 858 + 4 826), every one small"""
    r = np.random.default_rng(seed)
    fg = r.random(shape) < density
    lab = r.integers(1, 4, shape)
    return (fg * lab).astype(np.uint8)


def percolation(seed=7, p=0.32, shape=(40, 33, 70), label=4):
    """one label just above the site-percolation threshold of the cubic lattice: one blob of 3 371 voxels across many tiles plus
    about 5 000 small ones (188 of them with 11 to 30 voxels)"""
    r = np.random.default_rng(seed)
    return ((r.random(shape) < p) * label).astype(np.uint8)


def checkerboard(shape=(18, 19, 38), label=1):
    """6 498 one-voxel components: the voxels touch by edges and corners only"""
    g = np.indices(shape).sum(0)
    return ((g % 2 == 0) * label).astype(np.uint8)


def parity12(shape):
    """labels 1 / 2 alternating by parity, no background: every voxel is its own component (8 192 in a full tile)"""
    g = np.indices(shape).sum(0)
    return (1 + g % 2).astype(np.uint8)


def slabs(axis, thickness, shape=CHAIN_SHAPE):
    """slabs of labels 1, 2, 1, 2 ... along `axis`: each slab is one component; different labels in contact never merge, equal labels
    across a tile face do"""
    idx = np.indices(shape)[axis]
    return (1 + (idx // thickness) % 2).astype(np.uint8)


def serpentine(shape=CHAIN_SHAPE, label=5):
    """ONE one-voxel-wide face-connected chain through all 27 tiles: whole x rows at even y of the even z planes, joined at alternating
    row ends by one voxel at odd y, planes joined by one voxel at odd z.  Row (0, 0) starts at x = 40, so the chain's first voxel in
    raster order lies in the second x tile while the first tile (later rows) is occupied too: the root is handed over from a later
    tile."""
    D0, D1, D2 = shape
    a = np.zeros(shape, dtype=np.uint8)
    at_end = True                  # the next connector sits at the high-x end
    for z in range(0, D0, 2):
        ys = list(range(0, D1, 2))
        if (z // 2) % 2:
            ys.reverse()
        for k, y in enumerate(ys):
            a[z, y, :] = label
            if k + 1 < len(ys):
                a[z, (y + ys[k + 1]) // 2, D2 - 1 if at_end else 0] = label
                at_end = not at_end
        if z + 2 < D0:             # up to the next even plane, at the end of the last row walked
            a[z + 1, ys[-1], D2 - 1 if at_end else 0] = label
            at_end = not at_end
    a[0, 0, :40] = 0
    return a


def tie_pair(second_larger, shape=(4, 35, 40), label=3):
    """two blobs of one label: A starts at (0, 20, 0) -- raster index 800, tile 2 -- and B at (1, 0, 0) -- raster index 1 400, tile 0:
    raster order is not tile order.  Equal sizes: keep-largest keeps A (the first); B one voxel larger: it keeps B."""
    a = np.zeros(shape, dtype=np.uint8)
    a[0, 20:23, 0:3] = label
    a[1, 0:3, 0:3] = label
    if second_larger:
        a[1, 3, 0] = label
    return a


def sizes567(shape=(3, 5, 40), label=2):
    """three blobs of 5, 6 and 7 voxels (x runs in rows of their own)"""
    a = np.zeros(shape, dtype=np.uint8)
    a[0, 0, 3:8] = label
    a[1, 2, 30:36] = label
    a[2, 4, 10:17] = label
    return a


def untouched(seed=5, shape=NOISE_SHAPE):
    """noise of labels 1, 2, 9, 255: 9 and 255 are never in `rois`"""
    r = np.random.default_rng(seed)
    fg = r.random(shape) < 0.6
    lab = np.array([1, 2, 9, 255], dtype=np.uint8)[r.integers(0, 4, shape)]
    return (fg * lab).astype(np.uint8)


def body_specks(body, seed=3, n_specks=40, label=2):
    """`body` (labels 0 / 1) with `n_specks` boxes of label 2 put into its background, 1 x 1 x 1 to 9 x 9 x 9 voxels: some under,
    some over 231 voxels.  Boxes may touch or overlap (then they are one blob) and are clipped at the volume's rim."""
    r = np.random.default_rng(seed)
    a = np.array(body, dtype=np.uint8)
    bg = np.argwhere(a == 0)
    for _ in range(n_specks):
        c = bg[r.integers(0, len(bg))]
        e = r.integers(1, 10, 3)
        sl = tuple(slice(int(c[k]), int(min(c[k] + e[k], a.shape[k]))) for k in range(3))
        box = a[sl]
        box[box == 0] = label
    return a


CLASS_MAP = {1: "l1", 2: "l2", 3: "l3", 4: "l4", 5: "l5", 9: "l9", 255: "l255"}


def golden_cases():
    """{name: (array, [(function, kwargs), ...])}: the calls whose results the reference recorded.  function is one of
    `keep_largest_blob_multilabel`, `remove_small_blobs_multilabel` (kwargs: rois, interval) or, on `array != 0`, `keep_largest_blob` /
    `remove_small_blobs` (kwargs: interval)."""
    n3 = noise3()
    big = int(max(np.bincount(_scipy_label_all(n3)[0].ravel())[1:]))
    all3 = ["l1", "l2", "l3"]
    cases = {
        "noise3": (n3, [("keep_largest_blob_multilabel", dict(rois=all3)), ("keep_largest_blob_multilabel", dict(rois=["l2"]))]
                   + [("remove_small_blobs_multilabel", dict(rois=all3, interval=[lo, 1e10])) for lo in (0, 1, 3, big, big - 1)]
                   + [("remove_small_blobs", dict(interval=[3, 1e10])), ("keep_largest_blob", {})]),
        "percolation": (percolation(), [("keep_largest_blob_multilabel", dict(rois=["l4"])),
                                        ("remove_small_blobs_multilabel", dict(rois=["l4"], interval=[10, 30])),
                                        ("remove_small_blobs", dict(interval=[10, 30])), ("keep_largest_blob", {})]),
        "checkerboard": (checkerboard(), [("keep_largest_blob_multilabel", dict(rois=["l1"])),
                                          ("remove_small_blobs_multilabel", dict(rois=["l1"], interval=[1, 1e10])),
                                          ("remove_small_blobs_multilabel", dict(rois=["l1"], interval=[0.5, 1e10]))]),
        "parity12": (parity12((18, 19, 38)), [("keep_largest_blob_multilabel", dict(rois=["l1", "l2"])),
                                             ("remove_small_blobs_multilabel", dict(rois=["l2"], interval=[1, 1e10]))]),
        "slabs_z17": (slabs(0, 17), [("keep_largest_blob_multilabel", dict(rois=["l1", "l2"])),
                                     ("remove_small_blobs_multilabel", dict(rois=["l1", "l2"], interval=[17 * 35 * 70, 1e10]))]),
        "serpentine": (serpentine(), [("keep_largest_blob_multilabel", dict(rois=["l5"])),
                                      ("remove_small_blobs_multilabel", dict(rois=["l5"], interval=[10, 30]))]),
        "tie_equal": (tie_pair(False), [("keep_largest_blob_multilabel", dict(rois=["l3"])), ("keep_largest_blob", {})]),
        "tie_second_larger": (tie_pair(True), [("keep_largest_blob_multilabel", dict(rois=["l3"]))]),
        "sizes567": (sizes567(), [("remove_small_blobs_multilabel", dict(rois=["l2"], interval=[lo, 1e10])) for lo in (5.999, 6.0, 4.999)]
                     + [("remove_small_blobs_multilabel", dict(rois=["l2"], interval=[5, 6])), ("remove_small_blobs", dict(interval=[5.999, 1e10]))]),
        "row7": (np.array([[[1, 1, 0, 2, 2, 2, 1]]], dtype=np.uint8), [("keep_largest_blob_multilabel", dict(rois=["l1", "l2"])),
                                                                      ("remove_small_blobs_multilabel", dict(rois=["l1", "l2"], interval=[1, 1e10]))]),
        "small33": (noise3(seed=2, shape=(3, 2, 33)), [("keep_largest_blob_multilabel", dict(rois=all3)),
                                                       ("remove_small_blobs_multilabel", dict(rois=all3, interval=[2, 1e10]))]),
        "zeros": (np.zeros((5, 5, 5), dtype=np.uint8), [("keep_largest_blob_multilabel", dict(rois=all3)),
                                                        ("remove_small_blobs_multilabel", dict(rois=all3, interval=[2, 1e10])),
                                                        ("remove_small_blobs", dict(interval=[10, 30])), ("keep_largest_blob", {})]),
        "untouched": (untouched(), [("keep_largest_blob_multilabel", dict(rois=["l1", "l2"])),
                                    ("remove_small_blobs_multilabel", dict(rois=["l1", "l2"], interval=[4, 1e10]))]),
    }
    return cases


def _scipy_label_all(a):
    """component numbering over all labels (sizes only: tests/golden and the case table)"""
    from scipy import ndimage
    out = np.zeros(a.shape, dtype=np.int64)
    n = 0
    for v in np.unique(a):
        if v:
            l, k = ndimage.label(a == v)
            out[l > 0] = l[l > 0] + n
            n += k
    return out, n


def call_key(case, k, fn):
    return f"{case}.{k}.{fn}"
