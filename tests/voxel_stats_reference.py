"""Plain numpy statements of the integer voxel statistics (csrc/agg.hip, k_median3_inplane of csrc/morph.hip) and the case
generators of tests/test_gpu_voxel_stats.py.  Written from the reference's semantics (oracle/bca.py, oracle/measurements.py,
the comments of include/boa_hip.h), not from the kernels: one vectorised expression per operation, int64 throughout, no
device, no tiling.  tests/test_voxel_stats_reference_cpu.py pins every helper here (against literal Python loops, against
oracle.bca.subclassify_tissues, and the generators against their own stated properties)."""
import numpy as np

# BCA/tissue/definition.py:6-30 in enum order (later rules overwrite): (tissue value, HU lo, HU hi, body region value)
TISSUE_RULES = (
    (1, -29, 150, 2),      # MUSCLE in MUSCLE
    (2, -1000, 3000, 5),   # BONE in BONE
    (3, -190, -30, 1),     # SAT: adipose HU in SUBCUTANEOUS_TISSUE
    (4, -190, -30, 3),     # VAT: ... in ABDOMINAL_CAVITY
    (5, -190, -30, 2),     # IMAT: ... in MUSCLE
    (6, -190, -30, 9),     # PAT: ... in MEDIASTINUM
    (7, -190, -30, 7),     # EAT: ... in PERICARDIUM
)
PART_TORSO = 1


# ---- the operations ---------------------------------------------------------------------------------------------------
def label_hu_histogram(ct, labels, mask, hu_min, nbins):
    """uint32 [256, nbins]: hist[l, clip(hu - hu_min, 0, nbins - 1)] over the voxels with label l != 0 and (no mask or
    mask != 0 -- any non-zero byte counts)."""
    ct = np.asarray(ct).ravel().astype(np.int64)
    lab = np.asarray(labels).ravel().astype(np.int64)
    keep = lab != 0
    if mask is not None:
        keep &= np.asarray(mask).ravel() != 0
    key = lab * nbins + np.clip(ct - hu_min, 0, nbins - 1)
    return np.bincount(key[keep], minlength=256 * nbins).reshape(256, nbins).astype(np.uint32)


def tissue_map(ct_rules, regions):
    t = np.zeros(np.shape(regions), np.uint8)
    hu = np.asarray(ct_rules).astype(np.int64)
    for value, lo, hi, region in TISSUE_RULES:
        t[(hu >= lo) & (hu <= hi) & (np.asarray(regions) == region)] = value
    return t


def tissue_aggregate(ct, ct_rules, regions, parts):
    """-> tissues uint8 [Z,Y,X] (rules look at ct_rules when given, else ct), counts int64 [Z,2,8], sums int64 [Z,2,8] of `ct`
    (always the unfiltered image); row 0 = all voxels, row 1 = parts == TORSO (zeros without parts); column 0 (no tissue) is
    not counted."""
    ct = np.asarray(ct)
    Z = ct.shape[0]
    t = tissue_map(ct if ct_rules is None else ct_rules, regions)
    key = (np.arange(Z, dtype=np.int64).reshape(Z, 1, 1) * 8 + t).ravel()
    hu = ct.ravel().astype(np.float64)                 # exact: a slice's |sum| stays far below 2^53
    counts = np.zeros((Z, 2, 8), np.int64)
    sums = np.zeros((Z, 2, 8), np.int64)
    rows = [np.ones(key.shape, bool)] + ([np.asarray(parts).ravel() == PART_TORSO] if parts is not None else [])
    for a, sel in enumerate(rows):
        counts[:, a] = np.bincount(key[sel], minlength=Z * 8).reshape(Z, 8)
        sums[:, a] = np.rint(np.bincount(key[sel], weights=hu[sel], minlength=Z * 8)).astype(np.int64).reshape(Z, 8)
    counts[:, :, 0] = 0
    sums[:, :, 0] = 0
    return t, counts, sums


def tissue_projections(tissues, regions, values):
    """-> coronal int64 [T,Z,X] (`(tissues == v).sum(axis=1)`), sagittal int64 [T,Z,Y] (`.sum(axis=2)`), and the body
    silhouettes `((regions > 0) & (regions < 255)).any(axis)`: bool [Z,X], bool [Z,Y]."""
    tissues, regions = np.asarray(tissues), np.asarray(regions)
    cor = np.stack([(tissues == v).sum(axis=1, dtype=np.int64) for v in values])
    sag = np.stack([(tissues == v).sum(axis=2, dtype=np.int64) for v in values])
    body = (regions > 0) & (regions < 255)
    return cor, sag, body.any(axis=1), body.any(axis=2)


def slice_label_presence(labels):
    """bool [Z,256]: present[z, l] = any voxel of slice z carries label l."""
    labels = np.asarray(labels)
    Z = labels.shape[0]
    key = np.arange(Z, dtype=np.int64).reshape(Z, 1, 1) * 256 + labels
    return np.bincount(key.ravel(), minlength=Z * 256).reshape(Z, 256) > 0


def label_hu_mask(ct, labels, lut, mode, lo, hi):
    """uint8 0/1: lut[label] != 0, and for mode 1 lo <= hu <= hi, for mode 2 hu < lo or hu > hi."""
    m = np.asarray(lut)[np.asarray(labels)] != 0
    if mode != 0:
        hu = np.asarray(ct).astype(np.int64)
        inside = (hu >= lo) & (hu <= hi)
        m &= inside if mode == 1 else ~inside
    return m.astype(np.uint8)


def label_select(labels, mode, vals):
    """uint8 0/1: mode 0 labels == vals[0]; mode 1 labels > 0; mode 2 labels in vals[:3]."""
    labels = np.asarray(labels)
    if mode == 0:
        m = labels == vals[0]
    elif mode == 1:
        m = labels > 0
    else:
        m = np.isin(labels, list(vals[:3]))
    return m.astype(np.uint8)


def median3_inplane(ct, flat_axis):
    from scipy import ndimage
    size = [3, 3, 3]
    size[flat_axis] = 1
    return ndimage.median_filter(np.asarray(ct), size=size, mode="reflect")


# ---- case generators ---------------------------------------------------------------------------------------------------
# A histogram key is the pair (label, bin); with hu_min = -32768 and nbins = 65536 it is the pair (label, HU).  The generators
# number the keys of labels 1..255 as  id = (label - 1) * nbins + bin  in [0, 255 * nbins).
def keys_of(ct, labels, hu_min, nbins):
    """key id per voxel, -1 where the voxel is not measured (label 0)."""
    lab = np.asarray(labels).astype(np.int64)
    b = np.clip(np.asarray(ct).astype(np.int64) - hu_min, 0, nbins - 1)
    return np.where(lab == 0, -1, (lab - 1) * nbins + b)


def keys_to_voxels(ids, hu_min, nbins):
    """(ct int16, labels uint8) carrying the key ids (-1 -> label 0, HU 0)."""
    ids = np.asarray(ids, dtype=np.int64)
    lab = np.where(ids < 0, 0, ids // nbins + 1)
    hu = np.where(ids < 0, 0, ids % nbins + hu_min)
    assert lab.max(initial=0) <= 255 and hu.min(initial=0) >= -32768 and hu.max(initial=0) <= 32767
    return hu.astype(np.int16), lab.astype(np.uint8)


def distinct_ids(rng, k, nbins, exclude=None):
    """k distinct key ids drawn uniformly from [0, 255 * nbins), none of them in `exclude`."""
    space = 255 * nbins
    have = np.empty(0, np.int64)
    while have.size < k:
        cand = np.unique(rng.integers(0, space, size=2 * (k - have.size) + 16))
        cand = np.setdiff1d(cand, have, assume_unique=True)
        if exclude is not None:
            cand = np.setdiff1d(cand, exclude, assume_unique=True)
        have = np.concatenate([have, rng.permutation(cand)[:k - have.size]])
    return rng.permutation(have)


def block_with_k_keys(rng, ids, size):
    """`size` key ids at shuffled positions in which every one of `ids` occurs at least once and nothing else occurs."""
    assert 1 <= ids.size <= size
    fill = ids[rng.integers(0, ids.size, size=size - ids.size)]
    return rng.permutation(np.concatenate([ids, fill]))


def threshold_volume(rng, n_wg, iters_per_wg, iter_vox, k_first, k_next, nbins):
    """Key ids of n_wg * iters_per_wg * iter_vox voxels.  Workgroup w owns voxels [w * iters_per_wg * iter_vox, (w + 1) * ...),
    iteration i of it the i-th iter_vox of those.  In every workgroup, iteration 0 holds exactly k_first distinct keys and every
    later iteration exactly k_next distinct keys, none of which occurred earlier in that workgroup's range.  (Different
    workgroups draw independently: their keys may coincide, and meet in the global table.)"""
    out = np.empty((n_wg, iters_per_wg, iter_vox), np.int64)
    for w in range(n_wg):
        ids = distinct_ids(rng, k_first + (iters_per_wg - 1) * k_next, nbins)
        out[w, 0] = block_with_k_keys(rng, ids[:k_first], iter_vox)
        for i in range(1, iters_per_wg):
            a = k_first + (i - 1) * k_next
            out[w, i] = block_with_k_keys(rng, ids[a:a + k_next], iter_vox)
    return out.ravel()


def repeated_keys_volume(rng, ids, lo, hi):
    """every id of `ids` between lo and hi times (inclusive, uniformly drawn), at shuffled positions"""
    reps = rng.integers(lo, hi + 1, size=ids.size)
    return rng.permutation(np.repeat(ids, reps)), reps


def run_cases(lane_vox=16):
    """[(offset, length)] of every run of equal keys that fits a lane's `lane_vox` voxels: all lengths 1..lane_vox at every
    start offset."""
    return [(o, L) for L in range(1, lane_vox + 1) for o in range(0, lane_vox - L + 1)]


def run_lanes(run_id, other_ids, lane_vox=16):
    """int64 [len(run_cases()), lane_vox]: row r holds `run_id` on the r-th case's voxels [offset, offset + length) and around
    the run the ids of `other_ids`, voxel j taking other_ids[j % len(other_ids)].  With two or more distinct ids no filler
    forms a run of its own; [-1] (not measured) surrounds the run with runs of key 0."""
    cases = run_cases(lane_vox)
    out = np.empty((len(cases), lane_vox), np.int64)
    for r, (o, L) in enumerate(cases):
        out[r] = [other_ids[j % len(other_ids)] for j in range(lane_vox)]
        out[r, o:o + L] = run_id
    return out


def run_lengths(row):
    """[(start, length, value)] of the maximal runs of equal values of a 1-D array"""
    row = np.asarray(row)
    cut = np.flatnonzero(np.concatenate([[True], row[1:] != row[:-1], [True]]))
    return [(int(a), int(b - a), int(row[a])) for a, b in zip(cut[:-1], cut[1:])]


def tissue_truth_table():
    """Every int16 HU x every region byte: (ct int16 [256, 256, 256], regions uint8 [256, 256, 256]) with
    regions[z] = z and ct[z] = all 65 536 HU values in ascending order -- slice z is region z's whole HU axis."""
    hu = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16).reshape(1, 256, 256)
    ct = np.ascontiguousarray(np.broadcast_to(hu, (256, 256, 256)))
    regions = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), (256, 256, 256)))
    return ct, regions


def binary_neighbourhoods(lo, hi, flat_axis):
    """All 512 binary 3x3 neighbourhoods as one int16 volume: pattern p (bit 3 * i + j <-> window position (i, j)) fills the
    in-plane 3x3 block whose centre is the centre voxel of cell p; cells are 3x3 blocks laid out on a 32 x 16 grid, so every
    pattern is the complete window of its own centre (the centre's window never leaves its cell).  flat_axis gets length 2
    (two copies).  -> (volume, centre index arrays (c0, c1) on the two in-plane axes, expected centre values = the median
    of the nine = hi where at least five bits are set)."""
    p = np.arange(512)
    bits = (p[:, None] >> np.arange(9)[None]) & 1                       # [512, 9]
    plane = np.empty((32 * 3, 16 * 3), np.int64)
    gi, gj = p // 16, p % 16
    for k in range(9):
        plane[gi * 3 + k // 3, gj * 3 + k % 3] = np.where(bits[:, k] == 1, hi, lo)
    vol = np.stack([plane, plane], axis=flat_axis).astype(np.int16)
    want = np.where(bits.sum(axis=1) >= 5, hi, lo).astype(np.int16)
    return vol, (gi * 3 + 1, gj * 3 + 1), want
