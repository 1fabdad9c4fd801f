"""Pins tests/voxel_stats_reference.py, the numpy side of tests/test_gpu_voxel_stats.py, so that it cannot drift: every
operation against a literal Python loop on a few hundred voxels (or against the oracle), every case generator against the
property it states."""
import numpy as np
import pytest

import voxel_stats_reference as R


def test_histogram_vs_python_loop():
    """clamps at both ends, mask bytes 0 / 1 / 2 / 255, labels 0 and 255 included"""
    rng = np.random.default_rng(0)
    n = 600
    ct = rng.choice(np.array([-32768, -200, -151, -150, -149, 0, 148, 149, 150, 151, 32767], np.int16), size=n)
    lab = rng.choice(np.array([0, 1, 2, 254, 255], np.uint8), size=n)
    mask = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    for hu_min, nbins in ((-150, 300), (-32768, 65536), (0, 1), (-200, 2)):
        for m in (None, mask):
            want = np.zeros((256, nbins), np.uint32)
            for i in range(n):
                if lab[i] == 0 or (m is not None and m[i] == 0):
                    continue
                want[lab[i], min(max(int(ct[i]) - hu_min, 0), nbins - 1)] += 1
            got = R.label_hu_histogram(ct, lab, m, hu_min, nbins)
            assert got.dtype == np.uint32 and got.shape == (256, nbins)
            np.testing.assert_array_equal(got, want)
            assert got[0].sum() == 0 and got.sum() > 0
    assert R.label_hu_histogram(ct[:0], lab[:0], None, -150, 300).sum() == 0


def test_tissue_aggregate_vs_oracle_on_the_truth_table():
    """every int16 HU x every region byte: the tissue map equals oracle.bca.subclassify_tissues, counts / sums equal plain
    per-slice reductions of it; ct_rules != ct: rules from ct_rules, sums from ct"""
    from oracle import bca as obca
    ct, regions = R.tissue_truth_table()
    assert ct.shape == regions.shape == (256, 256, 256)
    pairs = np.unique(ct.ravel().astype(np.int64) * 256 + regions.ravel())
    assert pairs.size == 1 << 24                                             # every (HU, region) pair exactly once
    ref_t = obca.subclassify_tissues(ct, regions)
    rng = np.random.default_rng(1)
    parts = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=ct.shape)
    t, counts, sums = R.tissue_aggregate(ct, None, regions, parts)
    np.testing.assert_array_equal(t, ref_t)
    assert set(np.unique(t)) == set(range(8))
    ct64 = ct.astype(np.int64)
    for a, sel in ((0, np.ones(ct.shape, bool)), (1, parts == 1)):
        assert (counts[:, a, 0] == 0).all() and (sums[:, a, 0] == 0).all()
        for k in range(1, 8):
            m = (ref_t == k) & sel
            np.testing.assert_array_equal(counts[:, a, k], m.sum(axis=(1, 2)))
            np.testing.assert_array_equal(sums[:, a, k], np.where(m, ct64, 0).sum(axis=(1, 2)))
    # without parts the torso row is empty
    _, c2, s2 = R.tissue_aggregate(ct, None, regions, None)
    assert (c2[:, 1] == 0).all() and (s2[:, 1] == 0).all()
    np.testing.assert_array_equal(c2[:, 0], counts[:, 0])
    # rules from a permuted copy, sums from ct
    rules = rng.permutation(ct.ravel()).reshape(ct.shape)
    t3, c3, s3 = R.tissue_aggregate(ct, rules, regions, parts)
    ref3 = obca.subclassify_tissues(rules, regions)
    np.testing.assert_array_equal(t3, ref3)
    for k in range(1, 8):
        m = (ref3 == k) & (parts == 1)
        np.testing.assert_array_equal(s3[:, 1, k], np.where(m, ct64, 0).sum(axis=(1, 2)))
        np.testing.assert_array_equal(c3[:, 1, k], m.sum(axis=(1, 2)))


def test_small_operations_vs_python_loops():
    rng = np.random.default_rng(2)
    Z, Y, X = 3, 5, 7
    tissues = rng.integers(0, 10, size=(Z, Y, X), dtype=np.uint8)
    regions = rng.choice(np.array([0, 1, 11, 254, 255], np.uint8), size=(Z, Y, X))
    regions[1] = 0
    vals = [2, 1, 9, 77]
    cor, sag, mc, ms = R.tissue_projections(tissues, regions, vals)
    for t, v in enumerate(vals):
        for z in range(Z):
            for x in range(X):
                assert cor[t, z, x] == sum(tissues[z, y, x] == v for y in range(Y))
            for y in range(Y):
                assert sag[t, z, y] == sum(tissues[z, y, x] == v for x in range(X))
    for z in range(Z):
        for x in range(X):
            assert mc[z, x] == any(0 < regions[z, y, x] < 255 for y in range(Y))
        for y in range(Y):
            assert ms[z, y] == any(0 < regions[z, y, x] < 255 for x in range(X))
    assert not mc[1].any() and cor[3].sum() == 0
    lab = rng.integers(0, 256, size=(Z, Y, X), dtype=np.uint8)
    pres = R.slice_label_presence(lab)
    for z in range(Z):
        for l in range(256):
            assert pres[z, l] == (l in lab[z])
    ct = rng.choice(np.array([-32768, -191, -190, -30, -29, 32767], np.int16), size=(Z, Y, X))
    lut = rng.integers(0, 3, size=256).astype(np.uint8)
    for mode in (0, 1, 2):
        got = R.label_hu_mask(ct, lab, lut, mode, -190, -30)
        for idx in np.ndindex(Z, Y, X):
            inside = -190 <= ct[idx] <= -30
            want = lut[lab[idx]] != 0 and (mode == 0 or (inside if mode == 1 else not inside))
            assert got[idx] == int(want)
    for mode, vals in ((0, (7, 0, 0)), (0, (0, 0, 0)), (1, (0, 0, 0)), (2, (3, 255, 0)), (2, (9, 9, 9))):
        got = R.label_select(lab, mode, vals)
        for idx in np.ndindex(Z, Y, X):
            l = lab[idx]
            want = l == vals[0] if mode == 0 else (l > 0 if mode == 1 else l in vals)
            assert got[idx] == int(want)


def test_median3_vs_sorted_windows():
    rng = np.random.default_rng(3)
    ct = rng.integers(-32768, 32768, size=(4, 5, 6)).astype(np.int16)
    for flat_axis in (0, 1, 2):
        got = R.median3_inplane(ct, flat_axis)
        axes = [a for a in range(3) if a != flat_axis]
        for idx in np.ndindex(*ct.shape):
            w = []
            for d0 in (-1, 0, 1):
                for d1 in (-1, 0, 1):
                    j = list(idx)
                    j[axes[0]] = min(max(idx[axes[0]] + d0, 0), ct.shape[axes[0]] - 1)   # reflect == clamp at radius 1
                    j[axes[1]] = min(max(idx[axes[1]] + d1, 0), ct.shape[axes[1]] - 1)
                    w.append(int(ct[tuple(j)]))
            assert got[idx] == sorted(w)[4]


def test_key_generators_keep_their_promises():
    rng = np.random.default_rng(4)
    nbins = 4096
    ids = R.distinct_ids(rng, 5000, nbins)
    assert ids.size == 5000 and np.unique(ids).size == 5000 and ids.min() >= 0 and ids.max() < 255 * nbins
    more = R.distinct_ids(rng, 3000, nbins, exclude=np.sort(ids))
    assert np.unique(more).size == 3000 and np.intersect1d(ids, more).size == 0
    ct, lab = R.keys_to_voxels(np.concatenate([ids, [-1, -1]]), -2048, nbins)
    assert ct.dtype == np.int16 and lab.dtype == np.uint8 and lab.min() == 0 and lab[:-2].min() >= 1
    np.testing.assert_array_equal(R.keys_of(ct, lab, -2048, nbins), np.concatenate([ids, [-1, -1]]))
    # the full key space: label 255 in the last bin is the last id
    ct, lab = R.keys_to_voxels([0, 255 * 65536 - 1], -32768, 65536)
    assert (ct[0], lab[0], ct[1], lab[1]) == (-32768, 1, 32767, 255)
    blk = R.block_with_k_keys(rng, ids[:100], 1000)
    assert blk.size == 1000 and set(blk) == set(ids[:100])
    vol, reps = R.repeated_keys_volume(rng, ids[:500], 2, 5)
    u, c = np.unique(vol, return_counts=True)
    assert reps.min() == 2 and reps.max() == 5 and vol.size == reps.sum()
    np.testing.assert_array_equal(c, reps[np.argsort(ids[:500])])


@pytest.mark.parametrize("k_first", [99, 100, 101, 102, 1])
def test_threshold_volume_has_exactly_k_distinct_keys_per_iteration(k_first):
    rng = np.random.default_rng(5)
    n_wg, iters, iv, k_next = 3, 3, 128, 60
    v = R.threshold_volume(rng, n_wg, iters, iv, k_first, k_next, 512)
    assert v.size == n_wg * iters * iv and v.min() >= 0
    for w in range(n_wg):
        seen = set()
        for i in range(iters):
            a = (w * iters + i) * iv
            ks = set(v[a:a + iv])
            assert len(ks) == (k_first if i == 0 else k_next), (w, i)
            assert not (ks & seen), (w, i)
            seen |= ks


def test_run_cases_cover_every_length_at_every_offset():
    cases = R.run_cases(16)
    assert len(cases) == len(set(cases)) == 136
    assert {L for _, L in cases} == set(range(1, 17))
    for L in range(1, 17):
        assert {o for o, l in cases if l == L} == set(range(0, 17 - L))
    lanes = R.run_lanes(7, [11, 12, 13])
    assert lanes.shape == (136, 16)
    for row, (o, L) in zip(lanes, cases):
        runs = R.run_lengths(row)
        assert (o, L, 7) in runs
        assert all(l == 1 for s, l, val in runs if val != 7)               # nothing else forms a run
    assert R.run_lengths([5, 5, 3, 5, 5, 5]) == [(0, 2, 5), (2, 1, 3), (3, 3, 5)]


@pytest.mark.parametrize("flat_axis", [0, 1, 2])
def test_binary_neighbourhoods_are_complete_windows(flat_axis):
    vol, (c0, c1), want = R.binary_neighbourhoods(-32768, 32767, flat_axis)
    axes = [a for a in range(3) if a != flat_axis]
    assert vol.shape[flat_axis] == 2 and vol.dtype == np.int16
    v = np.moveaxis(vol, flat_axis, 0)
    np.testing.assert_array_equal(v[0], v[1])
    assert vol.shape[axes[0]] == 96 and vol.shape[axes[1]] == 48
    seen = set()
    for p in range(512):
        w = v[0, c0[p] - 1:c0[p] + 2, c1[p] - 1:c1[p] + 2].ravel()
        bits = sum(1 << k for k in range(9) if w[k] == 32767)
        assert bits == p and set(w) <= {-32768, 32767}
        assert want[p] == sorted(int(x) for x in w)[4]
        seen.add(bits)
    assert len(seen) == 512
    # and the reference filter agrees with the stated medians
    med = np.moveaxis(R.median3_inplane(vol, flat_axis), flat_axis, 0)
    np.testing.assert_array_equal(med[0, c0, c1], want)
