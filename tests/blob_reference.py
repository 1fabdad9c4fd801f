"""Test-side restatement of the blob filters of TS/postprocessing.py:13-98 with scipy.ndimage.label (6-connected, as the reference
calls it), and a one-pass flood fill of "maximal face-connected sets of equal non-zero label" from the definition (no library
labelling) for the roots and sizes of boa_label_blobs6.  Pinned against the reference's own functions by
tests/golden/g16_blobs.npz (tests/test_blob_reference_cpu.py).  Test infrastructure only."""
import numpy as np
from scipy import ndimage


def keep_largest_blob(data):
    blob_map, n = ndimage.label(data)
    if n == 0:
        return data                                   # no foreground
    counts = np.bincount(blob_map.ravel(), minlength=n + 1)[1:]
    return (blob_map == int(np.argmax(counts)) + 1).astype(np.uint8)    # argmax: the first of equal counts


def keep_largest_blob_multilabel(data, class_map, rois):
    data = np.array(data)
    inv = {v: k for k, v in class_map.items()}
    for roi in rois:
        idx = inv[roi]
        sel = data == idx
        keep = keep_largest_blob(sel) > 0.5
        data[sel] = 0
        data[keep] = idx
    return data


def remove_small_blobs(img, interval=(10, 30)):
    mask, n = ndimage.label(img)
    counts = np.bincount(mask.ravel())
    if len(counts) <= 1:
        return img                                    # only background
    remove = (counts <= interval[0]) | (counts > interval[1])     # (index 0 = the background count: as in the reference)
    mask[np.isin(mask, np.nonzero(remove)[0])] = 0
    mask[mask > 0] = 1
    return mask


def remove_small_blobs_multilabel(data, class_map, rois, interval=(10, 30)):
    data = np.array(data)
    inv = {v: k for k, v in class_map.items()}
    for roi in rois:
        idx = inv[roi]
        sel = data == idx
        keep = remove_small_blobs(sel, interval) > 0.5
        data[sel] = 0
        data[keep] = idx
    return data


def size_threshold_voxels(size_thr_mm3, zooms):
    """TS/nnunet.py:601-605: np.prod of the float32 header zooms, python int / np.float32."""
    vox_vol = np.prod(tuple(np.float32(z) for z in zooms))
    return size_thr_mm3 / vox_vol


def body_postprocessing(data, zooms, remove_small=False, class_map=None):
    """TS/nnunet.py:595-617 for task `body` on the model grid: keep largest body_trunc, drop body_extremities blobs under
    50 000 mm^3, then (remove_small) every label's blobs under 200 mm^3."""
    cm = class_map or {1: "body_trunc", 2: "body_extremities"}
    out = keep_largest_blob_multilabel(data, cm, ["body_trunc"])
    out = remove_small_blobs_multilabel(out, cm, ["body_extremities"], [size_threshold_voxels(50000, zooms), 1e10])
    if remove_small:
        out = remove_small_blobs_multilabel(out, cm, list(cm.values()), [size_threshold_voxels(200, zooms), 1e10])
    return out


def components6(labels):
    """(roots, sizes): roots[v] = smallest linear index (C order) of v's component, -1 on background; sizes = {root: voxel count}.
    A component is a maximal set of voxels of equal non-zero value connected through faces.  Explicit flood fill."""
    a = np.ascontiguousarray(labels)
    a = a.reshape((1,) * (3 - a.ndim) + a.shape)
    D0, D1, D2 = a.shape
    flat = a.ravel().tolist()
    roots = [-1] * len(flat)
    sizes = {}
    s0, s1 = D1 * D2, D2
    for start, v in enumerate(flat):      # ascending linear index: the first voxel met of a component is its smallest index
        if not v or roots[start] >= 0:
            continue
        stack = [start]
        roots[start] = start
        count = 0
        while stack:
            p = stack.pop()
            count += 1
            z, r = divmod(p, s0)
            y, x = divmod(r, s1)
            for ok, q in ((z > 0, p - s0), (z + 1 < D0, p + s0), (y > 0, p - s1), (y + 1 < D1, p + s1), (x > 0, p - 1),
                          (x + 1 < D2, p + 1)):
                if ok and flat[q] == v and roots[q] < 0:
                    roots[q] = start
                    stack.append(q)
        sizes[start] = count
    return np.array(roots, dtype=np.int64).reshape(np.shape(labels)), sizes
