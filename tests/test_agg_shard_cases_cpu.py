"""Pins tests/agg_shard_cases.py, the numpy side of tests/test_gpu_agg_engine.py, and runs the sharded connected-component protocol
of boa_hip/agg_shard.py with its numpy engine over every (mask, cut plan) pair: each interface mask has the components it is built to
have (flood fill of tests/floodfill.py), the in-process communicator and the cut plans are what they claim to be, the protocol's
result equals the whole-volume reference for filter_largest_sharded and for remove_small_sharded at every threshold, and
merge_components keeps its invariants.  Integers only: every comparison is exact.  No device."""
from collections import Counter

import numpy as np
import pytest
from scipy import ndimage

import agg_shard_cases as AC
import floodfill
import morph_cases as MC
from boa_hip import agg_shard as ag


# ---- the cases, the plans and the communicator -----------------------------------------------------------------------------------
def test_case_lists_and_restated_constants():
    assert tuple(AC.interface_cases()) == AC.INTERFACE_NAMES
    assert tuple(AC.all_cases()) == AC.ALL_NAMES and len(set(AC.ALL_NAMES)) == len(AC.ALL_NAMES)
    assert AC.ERODE_REACH == ag.ERODE_REACH
    for Z in (0, 1, 2, 7, 20, 34):
        for world in (1, 2, 3, 7, Z + 2):
            assert AC.balanced(Z, world) == ag.slab_bounds(Z, world)
    for name in AC.INTERFACE_NAMES:
        assert AC.interface_cases()[name]["mask"].shape == (AC.SMALL if name.endswith("_small") else AC.BIG)


@pytest.mark.parametrize("Z", [7, 20, 32, 33, 34, 24])
def test_cut_plans(Z):
    plans = AC.cut_plans(Z)
    assert plans["balanced2"] == ag.slab_bounds(Z, 2) and plans["balanced3"] == ag.slab_bounds(Z, 3)
    if Z <= 8:
        assert plans["every_plane"] == [(z, z + 1) for z in range(Z)]
        assert len(plans["two_ranks_too_many"]) == Z + 2 and plans["two_ranks_too_many"][-2:] == [(Z, Z), (Z, Z)]
        assert plans["empty_in_the_middle"][1][0] == plans["empty_in_the_middle"][1][1] and 0 < plans["empty_in_the_middle"][1][0] < Z
        assert any(0 < b - a < AC.ERODE_REACH for a, b in plans["thin"])
    else:
        assert MC.TZ == 16
        assert [p[0] for p in plans["tile16"][1:]] == [16]
        assert [p[0] for p in plans["cut15"][1:]] == [15] and [p[0] for p in plans["cut17"][1:]] == [17]
        assert [p[0] for p in plans["cut15_16_17"][1:]] == [15, 16, 17]
        assert any(0 < b - a < AC.ERODE_REACH for a, b in plans["cut15_16_17"])


def test_two_pass_communicator():
    """every rank gets every rank's contribution, in rank order; a call without a collective, or with two, is an error"""
    got = {}

    def call(comm, r):
        assert comm.world == 3 and comm.rank == r
        got[r] = comm.all_gather(("part", r))

    AC.drive(3, call)
    assert got == {r: [("part", 0), ("part", 1), ("part", 2)] for r in range(3)}
    with pytest.raises(AssertionError):
        AC.drive(2, lambda comm, r: None)
    with pytest.raises(AssertionError):
        AC.drive(2, lambda comm, r: (comm.all_gather(r), comm.all_gather(r)))
    # the protocol's own AggComm with one rank is the same thing as a drive of one rank
    m = AC.interface_cases()["tie_three_small"]["mask"].astype(np.uint8)
    a, b = AC.seg_around(m != 0), AC.seg_around(m != 0)
    ag.filter_largest_sharded(ag.AggComm(None, 0, 1), ag.NumpyAggEngine(), m, a, 0, 255)
    AC.drive(1, lambda comm, r: ag.filter_largest_sharded(comm, ag.NumpyAggEngine(), m, b, 0, 255))
    np.testing.assert_array_equal(a, b)


def test_region_chain_is_read_from_the_product():
    from boa_hip.bca import REGION as R
    chain = AC.region_chain(ag, R)
    assert chain == [(1, (0, 0, 0), 255), (2, (R["THORACIC_CAVITY"], R["MEDIASTINUM"], R["PERICARDIUM"]), 255),
                     (0, (R["PERICARDIUM"], 0, 0), 255), (0, (R["ABDOMINAL_CAVITY"], 0, 0), 255)]
    assert ag.filter_largest_sharded.__name__ == "filter_largest_sharded"      # (put back)


@pytest.mark.parametrize("name", AC.INTERFACE_NAMES)
def test_interface_case_facts(name):
    """component count, size multiset and the winner by flood fill; scipy's labelling (behind largest_ref / remove_small_ref) is the
    same partition; then what each mask is built for"""
    c = AC.interface_cases()[name]
    m = c["mask"]
    Z, Y, X = m.shape
    roots, sizes = AC.flood(name)
    lab, k = MC.label26(m)
    assert k == len(sizes) == c["n"]
    assert dict(Counter(sizes.values())) == c["sizes"]
    assert sum(sizes.values()) == int(m.sum())
    order = np.array(sorted(sizes), np.int64)
    if k:
        np.testing.assert_array_equal(roots[m], order[lab[m] - 1])
        big = max(sizes.values())
        keep = min(r for r, s in sizes.items() if s == big)
        assert keep == c["keep"]
        np.testing.assert_array_equal(MC.largest_ref(m), m & (roots != keep) if k > 1 else np.zeros_like(m))
    kept = [int(MC.remove_small_ref(m, t).sum()) for t in c["thresholds"]]
    assert kept == sorted(kept, reverse=True) and c["thresholds"] == tuple(sorted(set(c["thresholds"])))
    if k:
        assert len(set(kept)) > 1
    plans = AC.cut_plans(Z)
    kind = name.rsplit("_", 1)[0]
    if kind in ("u_shape", "n_shape"):
        # away from the joining plane the arms are two components of their own, each smaller than the block
        part = m[:Z - 1] if kind == "u_shape" else m[1:]
        assert sorted(floodfill.components26(part)[1].values()) == [Z - 1, Z - 1, min(c["sizes"])] and c["arm"] < min(c["sizes"])
    if kind == "corner_chain":
        # no link of the chain survives without the diagonal offsets: 18-connectivity leaves one voxel per plane
        assert ndimage.label(m, structure=ndimage.generate_binary_structure(3, 2))[1] == Z + 1
        assert c["bar_first"] < c["keep"]
        ys, xs = [v[1] for v in c["chain"]], [v[2] for v in c["chain"]]
        if Z > 16:
            assert xs[15] == 0 and ys[16] == Y - 1
    if kind == "tie_three":
        assert len(set(sizes.values())) == 1 and c["keep"] == min(sizes)
        firsts = sorted(r // (Y * X) for r in sizes)
        for p in ("balanced3", "every_plane" if Z <= 8 else "cut15_16_17"):
            owners = {next(i for i, (a, b) in enumerate(plans[p]) if a <= z < b) for z in firsts}
            assert len(owners) == 3, p                                  # the three first voxels lie in three different slabs
    if kind == "late_winner":
        lose, win = sorted(sizes.values())
        assert min(r for r, s in sizes.items() if s == lose) < c["keep"]
        cut_through = 0
        for p, cuts in plans.items():
            part = [int((roots[a:b] == c["keep"]).sum()) for a, b in cuts if (roots[a:b] == c["keep"]).any()]
            if len(part) > 1:                                           # every plan that cuts the winner leaves pieces <= the loser
                cut_through += 1
                assert sum(part) == win and max(part) <= lose, p
        assert cut_through >= 4
    if kind == "through_middle":
        zc = 3 if Z < 16 else 15
        assert m[zc, 4, 4] and m[zc + 1, 4, 6] and not m[zc + 1, 4, 4] and not m[zc, 4, 6]
    if kind == "single_component":
        assert not m[0].any() and not m[-1].any()
    if kind == "background_gap":
        a, b = c["gap"]
        assert not m[a:b].any() and m[a - 1].any() and m[b].any()
        assert any(b2 > a2 and a <= a2 and b2 <= b and i not in (0, len(cuts) - 1) for cuts in plans.values() for i, (a2, b2) in enumerate(cuts))
    if kind == "threshold_merge":
        s = c["s"]
        cut_through = 0
        for p, cuts in plans.items():
            rod = [int(m[a:b, 0, 0].sum()) for a, b in cuts if b > a and m[a:b, 0, 0].any()]
            assert sum(rod) == s
            if len(rod) > 1:
                cut_through += 1
                assert max(rod) <= s - 2, p
        assert cut_through >= 2


# ---- the protocol with the numpy engine ------------------------------------------------------------------------------------------
def _run_largest(m8, seg, cuts):
    """filter_largest_sharded for every rank of a plan, on copies of the slabs; returns the reassembled label volume"""
    slabs = [seg[a:b].copy() for a, b in cuts]
    AC.drive(len(cuts), lambda comm, r: ag.filter_largest_sharded(comm, ag.NumpyAggEngine(), m8[cuts[r][0]:cuts[r][1]], slabs[r], cuts[r][0], 255))
    return np.concatenate(slabs, axis=0)


def _run_remove_small(m8, cuts, t):
    slabs = [m8[a:b].copy() for a, b in cuts]
    AC.drive(len(cuts), lambda comm, r: ag.remove_small_sharded(comm, ag.NumpyAggEngine(), slabs[r], cuts[r][0], t))
    return np.concatenate(slabs, axis=0)


@pytest.mark.parametrize("name,plan", AC.pairs(), ids=lambda v: v)
def test_protocol_numpy_engine(name, plan):
    """filter_largest_sharded and remove_small_sharded (every threshold of the case) equal the whole-volume references"""
    c = AC.all_cases()[name]
    m = c["mask"]
    cuts = AC.cut_plans(m.shape[0])[plan]
    m8 = m.astype(np.uint8)
    want_big, want_small = AC.references(name)
    seg = AC.seg_around(m)
    want = seg.copy()
    want[want_big] = 255
    np.testing.assert_array_equal(_run_largest(m8, seg, cuts), want, err_msg=f"{name} {plan}")
    for t in c["thresholds"]:
        got = _run_remove_small(m8, cuts, t)
        np.testing.assert_array_equal(got.astype(bool), want_small[t], err_msg=f"{name} {plan} max_size {t}")
        assert set(np.unique(got)) <= {0, 1}


def test_numpy_engine_slab_without_foreground():
    """regression: a non-empty slab without a foreground voxel (and a slab of no planes) has no components, and its planes are
    background -- NumpyAggEngine.ccl raised IndexError on the former"""
    eng = ag.NumpyAggEngine()
    for shape in ((2, 3, 4), (1, 3, 4)):
        cc = eng.ccl(np.zeros(shape, np.uint8))
        rf, rl, roots, sizes = eng.boundary_and_components(cc, 5)
        assert rf.shape == rl.shape == shape[1:] and (rf == -1).all() and (rl == -1).all()
        assert roots.shape == sizes.shape == (0,) and roots.dtype == sizes.dtype == np.int64
        seg = np.full(shape, 7, np.uint8)
        eng.fill_all_but(cc, [], 5, seg, 255)
        mask = np.zeros(shape, np.uint8)
        eng.remove_small(cc, [], 5, 3, mask)
        assert (seg == 7).all() and not mask.any()
    cc = eng.ccl(np.zeros((0, 3, 4), np.uint8))
    rf, rl, roots, sizes = eng.boundary_and_components(cc, 5)
    assert rf is None and rl is None and len(roots) == len(sizes) == 0
    # and through the protocol: one plane per slab, the outer planes empty
    c = AC.interface_cases()["single_component_small"]
    assert not c["mask"][0].any()
    got = _run_remove_small(c["mask"].astype(np.uint8), AC.cut_plans(7)["every_plane"], c["thresholds"][1])
    np.testing.assert_array_equal(got.astype(bool), c["mask"])


@pytest.mark.parametrize("name,plan", AC.pairs(), ids=lambda v: v)
def test_merge_components_invariants(name, plan):
    """every rep is the smallest global root of its set (= the whole component's first voxel), every merged size is the whole
    component's, the merged sizes sum to the foreground count and there are as many reps as components in the whole volume"""
    m = AC.all_cases()[name]["mask"]
    cuts = AC.cut_plans(m.shape[0])[plan]
    roots_ref, sizes_ref = AC.flood(name)
    plane = m.shape[1] * m.shape[2]
    out = {}

    def call(comm, r):
        a, b = cuts[r]
        eng = ag.NumpyAggEngine()
        rf, rl, roots, sizes = eng.boundary_and_components(eng.ccl(m[a:b]), a)
        assert len(roots) == len(sizes)
        assert (np.diff(roots) > 0).all() and (roots // plane >= a).all() and (roots // plane < b).all()
        out[r] = (roots, ag.merge_components(comm, rf, rl, roots, sizes))

    AC.drive(len(cuts), call)
    seen = {}
    for r, (roots, (rep_of, size_of, size_by_rep)) in out.items():
        assert size_by_rep == sizes_ref                                  # {first voxel of the component: size}, on every rank
        assert sum(size_by_rep.values()) == int(m.sum()) and len(size_by_rep) == len(sizes_ref)
        assert set(rep_of) == set(size_of) == {int(g) for g in roots}
        for g in roots:
            rep = int(roots_ref.flat[int(g)])
            assert rep_of[int(g)] == rep and rep <= g and size_of[int(g)] == sizes_ref[rep]
            seen.setdefault(rep, []).append(int(g))
    assert set(seen) == set(sizes_ref) and all(rep in pieces for rep, pieces in seen.items())


# ---- the region chain ------------------------------------------------------------------------------------------------------------
def test_region_chain_numpy_engine():
    """the four filters, filter by filter over all ranks, equal the oracle's post-processing of the whole phantom; the phantom's stray
    islands lie on both sides of every cut"""
    from boa_hip.bca import REGION as R
    from oracle import bca as obca
    seg = AC.region_phantom(R)
    assert seg.shape == AC.REGION_SHAPE
    want = obca.postprocess_region_segmentation(seg)
    gone = (want == 255) & (seg != 255)
    assert ((want == seg) | gone).all()
    islands = np.zeros(seg.shape, bool)
    for sl, _ in AC.region_islands(R):
        islands[sl] = True
    np.testing.assert_array_equal(gone, islands)                 # the islands go, all of them, and nothing else
    for z in (8, 12, 15, 16, 17):
        assert gone[:z].any() and gone[z:].any()
    assert gone[15].any() and gone[16].any() and gone[17].any() and len(np.unique(seg[gone])) >= 4
    plans = AC.cut_plans(AC.REGION_SHAPE[0], every_plane=True)
    assert {"balanced2", "balanced3", "every_plane", "two_ranks_too_many", "cut15_16_17"} <= set(plans)
    for plan, cuts in plans.items():
        slabs = [seg[a:b].copy() for a, b in cuts]
        for mode, vals, fill in AC.region_chain(ag, R):
            AC.drive(len(cuts), lambda comm, r: ag.filter_largest_sharded(comm, ag.NumpyAggEngine(), AC.select_ref(slabs[r], mode, vals), slabs[r],
                                                                          cuts[r][0], fill))
        np.testing.assert_array_equal(np.concatenate(slabs, axis=0), want, err_msg=plan)


# ---- the halo of the sharded erosion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", AC.ERODE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_erode_mask_needs_exactly_the_halo(shape):
    """on the host reference (erode_box_ref with the reach of the 6^3 footprint): slab + ERODE_REACH planes gives the whole volume's
    erosion on the owned planes for every plan; without a halo, or with one plane less on the low side, every cut decides something --
    so the GPU test of the claim can fail"""
    m = AC.erode_mask(shape)
    Z = shape[0]
    lo, hi = MC.erode_reach(6)
    assert (lo, hi) == (-AC.ERODE_REACH, AC.ERODE_REACH - 1)
    want = MC.erode_box_ref(m, lo, hi)
    assert want.any() and not want.all() and want[0].any() and not want[0].all() and want[-1].any() and not want[-1].all()

    def slab(a, b, below, above):
        h0, h1 = max(0, a - below), min(Z, b + above)
        return MC.erode_box_ref(m[h0:h1], lo, hi)[a - h0:b - h0]

    for plan, cuts in AC.cut_plans(Z).items():
        for a, b in cuts:
            if b == a:
                continue
            assert AC.halo(Z, a, b) == (max(0, a - 3), min(Z, b + 3))
            np.testing.assert_array_equal(slab(a, b, AC.ERODE_REACH, AC.ERODE_REACH), want[a:b], err_msg=plan)
            np.testing.assert_array_equal(slab(a, b, -lo, hi), want[a:b], err_msg=plan)      # (the footprint's own reach is enough)
            if a + lo >= 0:                  # the plane a - 3 exists: it decides something in plane a
                assert (slab(a, b, -lo - 1, hi) != want[a:b]).any(), (plan, a, b)
            if b - 1 + hi < Z:               # the plane b + 1 exists: it decides something in plane b - 1
                assert (slab(a, b, -lo, hi - 1) != want[a:b]).any(), (plan, a, b)
