"""Pins tests/morph_cases.py, the numpy side of tests/test_gpu_morph_worstcase.py: every case has the property it is built for,
shown once with the library-free flood fills of tests/floodfill.py and once with scipy.ndimage, and every reference one-liner agrees
with scipy / the oracle.  No device."""
from collections import Counter

import numpy as np
import pytest
from scipy import ndimage

import floodfill
import morph_cases as MC


# ---- connected components --------------------------------------------------------------------------------------------------------
def test_case_list_is_complete():
    assert tuple(MC.cc_cases()) == MC.CC_NAMES


@pytest.mark.parametrize("name", MC.CC_NAMES)
def test_cc_case_facts_flood_fill_and_scipy(name):
    """component count, size multiset and the component that wins the tie, by flood fill; scipy's 3 x 3 x 3 labelling is the same
    partition, numbered in the order of the first voxels (what `largest_ref` and `remove_small_ref` rely on)"""
    c = MC.cc_cases()[name]
    m = c["mask"]
    assert m.dtype == bool and m.size <= 1_300_000
    roots, sizes = MC.cc_flood(name)
    lab, k = MC.label26(m)
    assert len(sizes) == k
    if c["n"] is not None:
        assert k == c["n"]
    if c["sizes"] is not None:
        assert dict(Counter(sizes.values())) == {s: q for s, q in c["sizes"].items() if q}
    assert sum(sizes.values()) == int(m.sum())
    # the same partition: scipy's label i <-> the i-th root in ascending order
    order = np.array(sorted(sizes), np.int64)
    assert ((lab > 0) == m).all()
    np.testing.assert_array_equal(roots[m], order[lab[m] - 1])
    np.testing.assert_array_equal(np.bincount(lab[m] - 1, minlength=k), [sizes[r] for r in order])
    # the largest component; ties: the first in raster order
    if k:
        big = max(sizes.values())
        keep = min(r for r, s in sizes.items() if s == big)
        if c["keep"] is not None:
            assert keep == c["keep"]
        out = MC.largest_ref(m)
        np.testing.assert_array_equal(out, m & (roots != keep) if k > 1 else np.zeros_like(m))
    # the thresholds select different sets
    kept = [int(MC.remove_small_ref(m, t).sum()) for t in c["thresholds"]]
    assert kept == sorted(kept, reverse=True)
    if c["sizes"] is not None and len(c["thresholds"]) > 1:
        assert len(set(kept)) > 1
    if "complement_n" in c:
        _, kc = MC.label26(~m)
        assert kc == c["complement_n"]
        assert len(floodfill.components26(~m)[1]) == c["complement_n"]


def test_lattices_fill_the_tables():
    """every complete tile of a lattice holds CB_CAP = 1024 components, the largest number a tile can hold; the odd lattice puts one on
    each complete tile's last voxel; (32, 32, 64) is 8 complete tiles: 8192 components"""
    for name in ("lattice0_32x32x64", "lattice1_32x32x64", "lattice0_33x35x70", "lattice1_33x35x70"):
        c = MC.cc_cases()[name]
        m = c["mask"]
        full_tiles = 0
        for t, sl in MC.tile_slices(m.shape).items():
            sub = m[sl]
            if sub.shape == (MC.TZ, MC.TY, MC.TX):
                full_tiles += 1
                assert int(sub.sum()) == MC.CAP
                if name.startswith("lattice1"):
                    assert sub[-1, -1, -1]
        assert full_tiles == 8
    assert MC.cc_cases()["lattice0_32x32x64"]["n"] == MC.cc_cases()["lattice1_32x32x64"]["n"] == 8192
    for name in ("lattice0_32x32x64", "lattice1_33x35x70"):
        m = MC.cc_cases()[name]["mask"]
        assert not MC.remove_small_ref(m, 1).any() and MC.remove_small_ref(m, 0).sum() == m.sum()
        assert (~MC.remove_small_ref(~m, m.size)).all()                       # holes up to the volume: everything is filled
        assert int((m & ~MC.largest_ref(m)).sum()) == 1                        # one voxel stays


def test_bridged_lattice_sizes_by_tile():
    c = MC.cc_cases()["lattice_bridged"]
    roots, sizes = MC.cc_flood("lattice_bridged")
    by_tile = {}
    for r, s in sizes.items():
        z, rem = divmod(r, 32 * 64)
        y, x = divmod(rem, 64)
        by_tile.setdefault(MC.tile_of((32, 32, 64), z, y, x), Counter())[s] += 1
    threes = {t for t, cnt in by_tile.items() if cnt[3]}
    twos = {t for t, cnt in by_tile.items() if cnt[2]}
    assert threes == {0, 3, 5, 6} and twos == {1, 7}                           # alternate tiles; the pairs on the last bit elsewhere
    assert all(by_tile[t] == Counter({1: MC.CAP}) for t in (2, 4))            # untouched tiles stay at capacity
    kept = [int(MC.remove_small_ref(c["mask"], t).sum()) for t in (0, 1, 2, 3)]
    assert kept == [int(c["mask"].sum()), 2 * 64 + 3 * 1024, 3 * 1024, 0]


@pytest.mark.parametrize("name", ["tie_word_columns", "tie_y_tile_border", "tie_z_tile_border"])
def test_tie_winner_is_not_first_by_tile(name):
    """the raster-first component lies in a LATER tile than the other one (or than the other one's lowest tile): an implementation
    that breaks ties by tile / table order keeps the wrong one"""
    c = MC.cc_cases()[name]
    shape = c["mask"].shape
    roots, sizes = MC.cc_flood(name)
    assert len(set(sizes.values())) == 1
    low_tile = {}
    for r in sizes:
        vox = np.argwhere(roots == r)
        low_tile[r] = min(MC.tile_of(shape, *v) for v in vox)
    winner = min(sizes)
    assert winner == c["keep"]
    assert all(low_tile[winner] > low_tile[r] for r in sizes if r != winner)
    lab, _ = MC.label26(c["mask"])
    assert lab.flat[winner] == 1                                               # scipy numbers it first


def test_tie_mirrored_is_the_control():
    c = MC.cc_cases()["tie_mirrored"]
    assert MC.tile_of(c["mask"].shape, 0, 0, 0) == 0 and c["keep"] == 0


def test_chain_root_and_first_voxel_lie_in_different_tiles():
    for name in ("chain_first_in_later_tile", "chain_and_larger"):
        c = MC.cc_cases()[name]
        shape = c["mask"].shape
        roots, sizes = MC.cc_flood(name)
        first = c["chain_first"]
        assert sizes[first] == 10 and roots[c["chain_last"]] == first
        assert MC.tile_of(shape, 0, 0, 40) == 1 and MC.tile_of(shape, *c["chain_last"]) == 0     # the lowest tile holds the LAST voxel
        bar = MC.lin(shape, 0, 5, 0)
        assert sizes[bar] == 10 and first < bar
        lab, _ = MC.label26(c["mask"])
        assert lab.flat[first] == 1
    assert MC.cc_cases()["chain_first_in_later_tile"]["keep"] == first
    big = MC.cc_cases()["chain_and_larger"]
    assert MC.cc_flood("chain_and_larger")[1][big["keep"]] == 36 and big["keep"] > bar                # size beats order


def test_rods_hand_over_to_64_roots_per_tile():
    c = MC.cc_cases()["rods_64_roots"]
    m = c["mask"]
    roots, sizes = MC.cc_flood("rods_64_roots")
    for t, sl in MC.tile_slices(m.shape).items():
        sub = m[sl]
        lab, k = MC.label26(sub)
        if t % 2 == 1:                                                         # rod tile: 64 local components, 64 different roots
            assert k == c["rods_per_tile"] and (np.bincount(lab.ravel())[1:] == 32).all()
            r = np.unique(roots[sl][sub])
            assert len(r) == 64
            assert all(MC.tile_of(m.shape, *np.unravel_index(v, m.shape)) == t - 1 for v in r)   # every root in the lower tile
            assert all(sizes[v] == 33 for v in r)
        else:
            assert k == c["lower_tile_components"] == MC.CAP
    assert int(MC.remove_small_ref(m, 32).sum()) == 256 * 33 and not MC.remove_small_ref(m, 33).any()


def test_full_tile_contacts_by_flood_fill():
    c = MC.cc_cases()["full_tile_contacts"]
    m = c["mask"]
    roots, sizes = MC.cc_flood("full_tile_contacts")
    assert m[0:16, 0:16, 32:64].all()
    root = roots[0, 0, 32]
    assert root == c["keep"] and sizes[root] == c["big"]
    for v in c["touch"] + c["chain"]:
        assert roots[v] == root, v
    for v in c["far"]:
        assert roots[v] == MC.lin(m.shape, *v) and sizes[roots[v]] == 1, v
        d = [max(0 - v[0], v[0] - 15, 0), max(0 - v[1], v[1] - 15, 0), max(32 - v[2], v[2] - 63, 0)]
        if v != c["far"][-1]:
            assert max(d) == 2, v                                              # exactly two away from the block
    assert len(sizes) == 1 + len(c["far"])
    contact = set()
    for v in c["touch"]:
        contact.add(sum(int(not (lo <= q <= hi)) for q, (lo, hi) in zip(v, ((0, 15), (0, 15), (32, 63)))))
    assert contact == {1, 2, 3}                                                # face, edge, corner
    tiles = {MC.tile_of(m.shape, *v) for v in c["touch"]}
    assert min(tiles) < 1 < max(tiles)                                         # backward and forward neighbour tiles
    lab, k = MC.label26(m)
    assert k == len(sizes)
    assert MC.remove_small_ref(m, c["big"] - 1).sum() == c["big"] and not MC.remove_small_ref(m, c["big"]).any()


def test_full_tiles():
    m = MC.cc_cases()["full_tiles_corner"]["mask"]
    assert MC.label26(m)[1] == 1 and int(m.sum()) == 16384 and MC.cc_flood("full_tiles_corner")[1] == {0: 16384}
    m = MC.cc_cases()["full_empty_mixed"]["mask"]
    kinds = Counter("full" if m[sl].all() else ("empty" if not m[sl].any() else "mixed") for sl in MC.tile_slices(m.shape).values())
    assert kinds == Counter(full=1, empty=1, mixed=6)


def test_long_chains():
    c = MC.cc_cases()["boustrophedon"]
    m = c["mask"]
    assert c["n"] == 1
    for sl in MC.tile_slices(m.shape).values():
        assert m[sl].any() and not m[sl].all()                                 # through every tile
    # one voxel wide: a path -- every voxel has at most two 6-neighbours, exactly two voxels have one
    nb = ndimage.convolve(m.astype(np.int32), ndimage.generate_binary_structure(3, 1).astype(np.int32), mode="constant") - 1
    assert nb[m].max() == 2 and int((nb[m] == 1).sum()) == 2
    assert MC.label26(~m)[1] == len(MC.cc_flood("boustrophedon_complement")[1])
    c = MC.cc_cases()["checkerboard"]
    assert MC.label26(c["mask"])[1] == 1
    assert ndimage.label(c["mask"])[1] > 1000                                  # 6-connected: the blocks fall apart
    assert ndimage.label(c["mask"], structure=ndimage.generate_binary_structure(3, 2))[1] == 1   # joined along edges


# ---- contour fill ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("YX", [(300, 70), (300, 33), (300, 64), (7, 9)])
def test_corridor_closed_fills_open_does_not(YX):
    Y, X = YX
    for transpose in (False, True):
        closed, opened = MC.corridor(Y, X), MC.corridor(Y, X, True)
        if transpose:
            closed, opened = closed.T, opened.T
        assert int((~opened).sum()) == int((~closed).sum()) + 1
        for fill in (floodfill.fill_external_contours, ndimage.binary_fill_holes):
            f = fill(closed)
            assert f.all() and int(f[1:-1, 1:-1].sum()) == (Y - 2) * (X - 2)
            np.testing.assert_array_equal(fill(opened), opened)               # nothing is filled
    if YX == (300, 70):
        assert (Y - 2) * (X - 2) == 20264
    # the corridor turns at every baffle: its length in 4-connected steps is of the order of the inside area
    inside = ~MC.corridor(Y, X)
    lab, k = ndimage.label(inside)
    assert k == 1
    assert int(inside.sum()) > (Y - 2) * (X - 2) // 2


@pytest.mark.parametrize("YX", MC.CORRIDOR_SHAPES)
def test_corridor_batches(YX):
    masks = MC.corridor_batch(*YX)
    assert len(masks) == 2
    for v in masks:
        assert v.shape == (6, *YX)
        ref = MC.fill_ref(v)
        np.testing.assert_array_equal(ref, np.stack([floodfill.fill_external_contours(s) for s in v]))
        full = [bool(s.all()) for s in ref]
        assert sorted(full) == [False, False, False, True, True, True]         # closed, closed mirrored, full | open, open, blank
        assert not ref[~np.array(full)][..., 1:-1, 1:-1].all()
    assert MC.bits_fill_supported(*YX)


def test_big_slice_is_the_smallest_unsupported_row_count_rounded_up():
    Z, Y, X = MC.BIG_SLICE
    assert not MC.bits_fill_supported(Y, X) and not MC.bytes_fill_in_lds(Y, X)
    W = (X + 31) // 32
    ymin = MC.LDS_LIMIT // ((W | 1) * 8) + 1                                    # the first unsupported Y at this X
    assert MC.bits_fill_supported(ymin - 1, X) and not MC.bits_fill_supported(ymin, X) and ymin == 1746
    assert MC.bytes_fill_in_lds(ymin, X)                                       # ... would still flood in LDS on the byte path
    assert Z * Y * X <= 1_300_000


def test_big_slice_labels_do_something():
    from oracle import bca as obca
    seg = MC.big_slice_labels()
    ref = obca.remove_small_labeled_objects(seg, threshold=300)
    assert (ref[0, 11:2039, 6:294] > 0).all()                                  # the big frame of slice 0 is filled
    assert not (ref[1, 700:900, 6:294] > 0).any()                              # slice 1: it has a mouth
    assert (ref[:, 1003:1027, 53:87] == 2).all()                               # closed frames of label 2, over label 1's fill in slice 0
    assert (ref[0, 1103:1127, 53:87] == 1).all() and not ref[1, 1103:1127, 53:87].any()   # the frame with a mouth holds nothing of its own
    assert (ref != 3).all() and (seg == 3).sum() > 300                         # the specks are gone
    assert (ref[1, 310:350, 110:170] == 1).all()                               # the hole of the solid block
    bb = np.argwhere(seg == 1)
    box = np.prod(bb.max(0) - bb.min(0) + 1)
    assert box > 0.7 * seg.size                                                # label 1 is filled uncropped


def test_small_volume_oracle_floods_with_the_largest_present_label():
    from oracle import bca as obca
    seg = MC.small_volume_labels()
    assert seg.size < 3000 and set(np.unique(seg)) == {0, 2, 5}
    ref = obca.remove_small_labeled_objects(seg)
    assert (ref == 5).all()                                                    # the complement of a present label is "small"


# ---- erosion ---------------------------------------------------------------------------------------------------------------------
def test_erode_reach_is_the_oracles_footprint():
    assert [MC.erode_reach(k) for k in (1, 2, 3, 6, 63, 64, 65)] == [(0, 0), (-1, 0), (-1, 1), (-3, 2), (-31, 31), (-32, 31), (-32, 32)]
    assert [MC.erode_on_bits(*MC.erode_reach(k)) for k in MC.BYTE_K] == [True, False, False]
    assert all(MC.erode_on_bits(lo, hi) for lo, hi in MC.ASYM_REACHES)


@pytest.mark.parametrize("X", MC.PINHOLE_X)
def test_pinhole_erosion_band_and_box_reference(X):
    from oracle import measurements as OM
    Z, Y = MC.PINHOLE_ZY
    for k in MC.PINHOLE_K:
        m = MC.pinhole_mask(X, k)
        for v in ((0, 7, 0), (Z - 1, 12, X - 1), (9, 0, min(31, X - 1)), (14, Y - 1, min(32, X - 1))):
            assert not m[v]
        ref = OM.erode_region(m, k)
        frac = float(ref.mean())
        assert 0.2 <= frac <= 0.8, (X, k, frac)
        np.testing.assert_array_equal(MC.erode_box_ref(m, *MC.erode_reach(k)), ref)
        fp = np.ones((k,) * 3, bool)
        if k % 2 == 0:
            fp = np.pad(fp, [(0, 1)] * 3)
        np.testing.assert_array_equal(ndimage.binary_erosion(m, structure=fp, border_value=1), ref)


@pytest.mark.parametrize("X", MC.ASYM_X)
def test_asymmetric_reaches_reference(X):
    """erode_box_ref against scipy's erosion with the same box written as a structure centred on the larger reach"""
    m = MC.asym_mask(X)
    for lo, hi in MC.ASYM_REACHES:
        ref = MC.erode_box_ref(m, lo, hi)
        r = max(-lo, hi)
        line = np.zeros(2 * r + 1, bool)
        line[r + lo:r + hi + 1] = True
        want = m
        for ax in range(3):                                                    # a box is separable
            shp = [1, 1, 1]
            shp[ax] = 2 * r + 1
            want = ndimage.binary_erosion(want, structure=line.reshape(shp), border_value=1)
        np.testing.assert_array_equal(ref, want)
        if (lo, hi) == (0, 0):
            np.testing.assert_array_equal(ref, m)
        else:
            assert 0.02 <= float(ref.mean()) <= 0.98, (X, lo, hi)


@pytest.mark.parametrize("shape", MC.BYTE_THIN_SHAPES)
def test_byte_reach_reference_against_oracle(shape):
    from oracle import measurements as OM
    m = MC.byte_mask(shape)
    got = {}
    for k in MC.BYTE_K:
        ref = OM.erode_region(m, k)
        np.testing.assert_array_equal(MC.erode_box_ref(m, *MC.erode_reach(k)), ref)
        assert ref.any() and not ref.all()
        got[k] = int(ref.sum())
    assert got[63] > got[64] > got[65]                                         # each step of lo / hi costs a plane


@pytest.mark.parametrize("shape", MC.BYTE_SHAPES)
def test_byte_masks_leave_something(shape):
    m = MC.byte_mask(shape)
    got = [int(MC.erode_box_ref(m, *MC.erode_reach(k)).sum()) for k in MC.BYTE_K]
    assert got[0] > got[1] > got[2] > 0


# ---- dilation, assign ------------------------------------------------------------------------------------------------------------
def test_dilate_masks_touch_corners_edges_faces():
    for shape in MC.DILATE_SHAPES:
        ms = MC.dilate_masks(shape)
        assert set(ms) == {"empty", "full", "corners", "edges", "faces"}
        assert not ms["empty"].any() and ms["full"].all() and ms["corners"][0, 0, 0] and ms["corners"][-1, -1, -1]
        for m in ms.values():
            assert m.shape == shape
            a = ndimage.binary_dilation(m, iterations=2)
            b = ndimage.binary_dilation(ndimage.binary_dilation(m))
            np.testing.assert_array_equal(a, b)


def test_assign_inputs():
    for n in MC.ASSIGN_N:
        mask, prev, part = MC.assign_inputs(n)
        assert mask.shape == prev.shape == part.shape == (n,)
        assert mask[-1] and part[-1]
        if n > 256:
            assert {0, 1, 2, 255} == set(np.unique(mask)) and (part == 0).any()
