"""GPU, C ABI: the float64 voxel statistics kernels against numpy.

boa_group_stats_f64: count, min, max and the six order statistics are exact (`==`); sum and m2 are fp64 sums in another
order than numpy's and are held to the project's bar for such sums, rtol 1e-9.  That bar means something only
where the sum does not cancel, so it is applied as |got - want| <= 1e-9 * max(|want|, sum|x| / 100): plain rtol 1e-9 wherever
|mean| >= mean|x| / 100, and for m2 only in groups with std >= 1 (in a group of neighbouring doubles the deviations are a few
ulp of the mean, which itself carries half an ulp of rounding: m2 has no stable digits there, in numpy either).  References
are `math.fsum`, i.e. exactly rounded.  boa_label_hu_mask_f64, the tissue map, the slice counts and the in-plane median
are exact."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE_ODD = (23, 29, 37)      # 24 679 voxels: not a multiple of the 8-voxel vectors, 7 voxels in the tail
SHAPE_VEC = (8, 16, 40)       # 5 120 voxels: vectors only


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _ranks(n):
    return [f((n - 1) * q) for q in (0.25, 0.5, 0.75) for f in (math.floor, math.ceil)]


def _group_stats(ctx, d_ct, d_lab, n, lut, n_groups):
    from boa_hip._lib import check
    lut = np.ascontiguousarray(lut, np.uint8)
    counts = np.full(n_groups, 12345, np.uint64)
    st = np.full((n_groups, 10), 777.0)
    check(ctx.lib.boa_group_stats_f64(ctx.h, d_ct.vp, d_lab.vp, n, lut.ctypes.data_as(C.c_void_p), n_groups,
                                      counts.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)), "boa_group_stats_f64")
    return counts, st


def _check_groups(ctx, ct, labels, lut, n_groups, views=None):
    """Run the entry on (ct, labels) and compare every group with numpy.  Returns the voxel count per group."""
    ct = np.ascontiguousarray(ct, np.float64).ravel()
    labels = np.ascontiguousarray(labels, np.uint8).ravel()
    d_ct, d_lab = views if views is not None else (ctx.from_numpy(ct), ctx.from_numpy(labels))
    try:
        counts, st = _group_stats(ctx, d_ct, d_lab, ct.size, lut, n_groups)
    finally:
        if views is None:
            d_ct.free()
            d_lab.free()
    grp = np.asarray(lut, np.uint8)[labels]
    for g in range(n_groups):
        x = ct[grp == g]
        assert counts[g] == x.size, (g, counts[g], x.size)
        if x.size == 0:
            assert not st[g].any(), g
            continue
        s = np.sort(x)
        assert st[g, 0] == s[0] and st[g, 1] == s[-1], (g, st[g, :2], s[0], s[-1])
        want = s[_ranks(x.size)]
        assert (st[g, 4:10] == want).all(), (g, x.size, st[g, 4:10], want)
        tot, mag = math.fsum(x), math.fsum(np.abs(x))
        print(f"group {g}: n {x.size} sum {st[g, 2]!r} (fsum {tot!r})")
        assert abs(st[g, 2] - tot) <= 1e-9 * max(abs(tot), mag / 100), (g, st[g, 2], tot)
        mean = tot / x.size
        m2 = math.fsum((x - mean) ** 2)
        if math.sqrt(m2 / x.size) >= 1.0 and math.isfinite(m2):
            print(f"group {g}: m2 {st[g, 3]!r} (fsum {m2!r})")
            assert abs(st[g, 3] - m2) <= 1e-9 * m2, (g, st[g, 3], m2)
    return counts


def _ct_with_air(rng, shape):
    """fractional HU, 30 % of all voxels at exactly -1024.0"""
    ct = np.round(rng.normal(40.0, 120.0, size=shape), 3) + 0.0625
    ct[rng.random(shape) < 0.3] = -1024.0
    return ct


def test_all_256_labels_with_air(ctx):
    rng = np.random.default_rng(0)
    n = int(np.prod(SHAPE_ODD))
    labels = rng.integers(0, 256, size=n).astype(np.uint8)
    labels[:256] = np.arange(256)                       # every label value occurs
    ct = _ct_with_air(rng, n)
    lut = np.full(256, 0xFF, np.uint8)
    lut[1:255] = np.arange(254)                         # 254 groups; labels 0 and 255 are holes
    counts = _check_groups(ctx, ct, labels, lut, 254)
    assert counts.min() > 0
    assert abs((ct == -1024.0).mean() - 0.3) < 0.02


def test_lut_merges_labels_and_has_holes(ctx):
    rng = np.random.default_rng(1)
    n = int(np.prod(SHAPE_ODD))
    labels = rng.integers(0, 256, size=n).astype(np.uint8)
    ct = _ct_with_air(rng, n)
    lut = (np.arange(256) % 7).astype(np.uint8)
    lut[np.arange(256) % 13 == 0] = 0xFF
    lut[0] = 0xFF
    _check_groups(ctx, ct, labels, lut, 7)
    # compact "organs": long runs of one label, as in a segmentation (waves and lanes on a single group)
    labels = np.repeat(rng.integers(0, 12, size=n // 97 + 1), 97)[:n].astype(np.uint8)
    _check_groups(ctx, ct, labels, lut, 7)


def test_several_iterations_per_workgroup_with_table_flushes(ctx):
    """150^3 voxels of noise labels: more 4 096-voxel iterations than three workgroups per CU, so workgroups loop, and with 254 groups
    every iteration brings more distinct (group, slot, digit) keys than the LDS table's flush threshold: the table is flushed inside
    the loop and filled again (the path the small volumes never reach).  Reference: one lexsort."""
    rng = np.random.default_rng(11)
    n = 150 ** 3
    labels = rng.integers(0, 256, size=n).astype(np.uint8)
    ct = np.round(rng.normal(40.0, 120.0, size=n), 3) + 0.0625
    ct[rng.random(n) < 0.3] = -1024.0
    lut = np.full(256, 0xFF, np.uint8)
    lut[1:255] = np.arange(254)
    d_ct, d_lab = ctx.from_numpy(ct), ctx.from_numpy(labels)
    try:
        counts, st = _group_stats(ctx, d_ct, d_lab, n, lut, 254)
    finally:
        d_ct.free()
        d_lab.free()
    grp = lut[labels]
    keep = grp != 0xFF
    g, x = grp[keep], ct[keep]
    order = np.lexsort((x, g))
    g, x = g[order], x[order]
    start = np.searchsorted(g, np.arange(255))
    for k in range(254):
        s = x[start[k]:start[k + 1]]
        assert counts[k] == s.size and s.size > 0
        assert st[k, 0] == s[0] and st[k, 1] == s[-1]
        assert (st[k, 4:10] == s[_ranks(s.size)]).all(), (k, st[k, 4:10], s[_ranks(s.size)])
        tot = math.fsum(s)
        assert abs(st[k, 2] - tot) <= 1e-9 * abs(tot), (k, st[k, 2], tot)      # (mean -280, mean|x| 390: no cancellation)
        m2 = math.fsum((s - tot / s.size) ** 2)
        assert abs(st[k, 3] - m2) <= 1e-9 * m2, (k, st[k, 3], m2)


def _special_volume(rng):
    n = int(np.prod(SHAPE_VEC))
    labels = np.zeros(n, np.uint8)
    ct = rng.normal(-300.0, 200.0, size=n)
    pos = rng.permutation(n)
    take = iter(pos)

    def put(label, values):
        idx = np.fromiter((next(take) for _ in range(len(values))), dtype=np.int64, count=len(values))
        labels[idx] = label
        ct[idx] = values
    put(2, [17.5])                                                       # one voxel
    put(3, [-3.25, 1e-3])                                                # two voxels
    put(4, np.full(500, 77.25))                                          # all equal
    chain = [100.0]
    for _ in range(299):
        chain.append(np.nextafter(chain[-1], np.inf))
    put(5, rng.permutation(chain))                                       # only the last radix digit separates them
    chain = [np.nextafter(np.nextafter(-200.0, -np.inf), -np.inf)]
    for _ in range(40):
        chain.append(np.nextafter(chain[-1], np.inf))
    put(6, np.repeat(chain, 3))                                          # neighbouring doubles, each three times
    mixed = np.concatenate([[0.0, -0.0, 0.0, -0.0, 5e-324, -5e-324, 1e-310, -2e-308, 1e30, -1e25, 3e-5, -7.5, 1e12],
                            rng.normal(0.0, 50.0, size=187)])
    put(7, mixed)                                                        # signs, zeros, subnormals, 1e30 in one group
    put(8, np.round(rng.normal(55.0, 20.0, size=700), 2) + 0.3)
    return ct, labels


def test_small_equal_neighbouring_and_extreme_groups(ctx):
    ct, labels = _special_volume(np.random.default_rng(2))
    lut = np.full(256, 0xFF, np.uint8)
    lut[1:9] = np.arange(8)                                              # label 1 does not occur: an empty group
    counts = _check_groups(ctx, ct, labels, lut, 8)
    assert list(counts[:4]) == [0, 1, 2, 500]


def test_mask_form_and_unaligned_views(ctx):
    """A 0/1 mask as the label volume with lut[1] = 0; and views that start at odd offsets (one voxel at a time)."""
    from boa_hip.device import BufferView
    rng = np.random.default_rng(3)
    n = int(np.prod(SHAPE_ODD))
    ct = _ct_with_air(rng, n)
    mask = (rng.random(n) < 0.4).astype(np.uint8)
    lut = np.full(256, 0xFF, np.uint8)
    lut[1] = 0
    _check_groups(ctx, ct, mask, lut, 1)
    _check_groups(ctx, ct, np.zeros(n, np.uint8), lut, 1)                # empty mask
    d_ct, d_m = ctx.from_numpy(ct), ctx.from_numpy(mask)
    try:
        for off in (1, 3):
            m = n - off - 2
            _check_groups(ctx, ct[off:off + m], mask[off:off + m], lut, 1,
                          views=(BufferView(d_ct, off * 8, m * 8), BufferView(d_m, off, m)))
    finally:
        d_ct.free()
        d_m.free()


def test_bad_arguments_are_refused(ctx):
    d = ctx.from_numpy(np.zeros(16))
    l = ctx.from_numpy(np.zeros(16, np.uint8))
    try:
        lut = np.zeros(256, np.uint8)
        lut[5] = 3
        with pytest.raises(ValueError, match="lut"):
            _group_stats(ctx, d, l, 16, lut, 2)
        with pytest.raises(ValueError, match="groups"):
            _group_stats(ctx, d, l, 16, np.full(256, 0xFF, np.uint8), 0)
    finally:
        d.free()
        l.free()


# ---- HU-window masks ------------------------------------------------------------------------------------------
def test_label_hu_mask_f64_window_edges(ctx):
    from boa_hip import measurements as M
    rng = np.random.default_rng(4)
    lo, hi = -200.0, -40.0
    edge = [lo, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), hi, np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
            -120.5, -199.999, -39.999, 0.0, -0.0, -1024.0, 1e30, -1e30]
    n = int(np.prod(SHAPE_ODD))
    ct = rng.choice(np.array(edge), size=n)
    labels = rng.integers(0, 6, size=n).astype(np.uint8)
    d_ct, d_lab, d_out = ctx.from_numpy(ct), ctx.from_numpy(labels), ctx.alloc(n)
    try:
        sel = np.isin(labels, [2, 3])
        want = {0: sel, 1: sel & (ct >= lo) & (ct <= hi), 2: sel & (np.less(ct, lo) | np.greater(ct, hi))}
        for mode in (0, 1, 2):
            M.label_hu_mask_f64(ctx, d_ct, d_lab, [2, 3], mode, n, d_out)
            np.testing.assert_array_equal(d_out.download((n,), np.uint8), want[mode].astype(np.uint8), err_msg=f"mode {mode}")
        assert want[1].sum() and want[2].sum() and (want[1] | want[2]).sum() == sel.sum()
    finally:
        for b in (d_ct, d_lab, d_out):
            b.free()


# ---- tissue pass ----------------------------------------------------------------------------------------------
RULES = [(1, (-29, 150), 2), (2, (-1000, 3000), 5), (3, (-190, -30), 1), (4, (-190, -30), 3), (5, (-190, -30), 2), (6, (-190, -30), 9),
         (7, (-190, -30), 7)]      # (tissue, HU range, region) in the order the reference applies them (later rules overwrite)


def _tissues_numpy(ct_rules, regions):
    out = np.zeros(regions.shape, np.uint8)
    for t, (lo, hi), region in RULES:
        out[(ct_rules >= lo) & (ct_rules <= hi) & (regions == region)] = t
    return out


def _boundary_values():
    vals = [-29.5, -190.0, -30.5, 0.25, 1e-300]
    for b in (-1000.0, -190.0, -30.0, -29.0, 150.0, 3000.0):
        vals += [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
    return np.array(vals)


@pytest.mark.parametrize("shape", [(7, 13, 11), SHAPE_VEC])
@pytest.mark.parametrize("with_parts", [False, True])
@pytest.mark.parametrize("with_rules", [False, True])
def test_tissue_aggregate_f64_vs_numpy(ctx, shape, with_parts, with_rules):
    from boa_hip import bca
    rng = np.random.default_rng(sum(shape))
    ct = rng.choice(_boundary_values(), size=shape)
    noise = rng.random(shape) < 0.3
    ct[noise] = np.round(rng.normal(-20.0, 150.0, size=int(noise.sum())), 2) + 0.125
    rules = np.ascontiguousarray(ct[:, ::-1, ::-1]) if with_rules else None     # another float volume for the rules
    regions = rng.integers(0, 12, size=shape).astype(np.uint8)
    parts = rng.integers(0, 4, size=shape).astype(np.uint8)
    bufs = [ctx.from_numpy(ct), ctx.from_numpy(regions), ctx.from_numpy(parts) if with_parts else None,
            ctx.from_numpy(rules) if with_rules else None]
    try:
        tis, counts, sums = bca.tissue_aggregate(ctx, bufs[0], bufs[1], bufs[2], shape, ct_rules=bufs[3], ct_f64=True)
        t = tis.download(shape, np.uint8)
        tis.free()
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    ref = _tissues_numpy(rules if with_rules else ct, regions)
    np.testing.assert_array_equal(t, ref)
    # -29.5 is neither muscle nor adipose tissue; -190.0 is adipose tissue
    probe = rules if with_rules else ct
    assert (ref[(probe == -29.5) & (regions == 2)] == 0).all() and (ref[(probe == -190.0) & (regions == 1)] == 3).all()
    assert sums.dtype == np.float64
    for a, m in ((0, np.ones(shape, bool)), (1, (parts == 1) if with_parts else np.zeros(shape, bool))):
        for k in range(1, 8):
            sel = (ref == k) & m
            np.testing.assert_array_equal(counts[:, a, k], sel.sum(axis=(1, 2)))
            for z in range(shape[0]):
                x = ct[z][sel[z]]
                want, mag = math.fsum(x), math.fsum(np.abs(x))
                assert abs(sums[z, a, k] - want) <= 1e-9 * max(abs(want), mag / 100), (z, a, k, sums[z, a, k], want)


# ---- in-plane median ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flat_axis", [0, 1, 2])
@pytest.mark.parametrize("shape", [(5, 7, 9), SHAPE_VEC, (1, 3, 2)])
def test_median3_inplane_f64_vs_numpy(ctx, flat_axis, shape):
    """np.median over the 3x3 window in the two other axes; at the border the window is clamped to the volume
    (scipy's mode="reflect" for a radius-1 window, which is what the int16 kernel does)."""
    from boa_hip import bca
    rng = np.random.default_rng(10 * flat_axis + shape[0])
    ct = rng.choice(np.concatenate([rng.normal(0.0, 100.0, size=40), [0.0, -0.0, 1e30, -1e30, 5e-324]]), size=shape)
    ax = [a for a in range(3) if a != flat_axis]
    pad = [(0, 0)] * 3
    for a in ax:
        pad[a] = (1, 1)
    p = np.pad(ct, pad, mode="edge")
    win = []
    for d0 in range(3):
        for d1 in range(3):
            sl = [slice(None)] * 3
            sl[ax[0]] = slice(d0, d0 + shape[ax[0]])
            sl[ax[1]] = slice(d1, d1 + shape[ax[1]])
            win.append(p[tuple(sl)])
    want = np.median(np.stack(win), axis=0)
    d = ctx.from_numpy(ct)
    o = bca.median_filter_inplane(ctx, d, shape, flat_axis, ct_f64=True)
    try:
        got = o.download(shape, np.float64)
    finally:
        d.free()
        o.free()
    assert (got == want).all()
