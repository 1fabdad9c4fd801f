"""Worst-case structure tests of the mask morphology kernels: the bit-packed component filters, contour fill and erosion of
csrc/ccl_bits.hip, their byte-mask twins (boa_ccl26, boa_ccl_remove_small, boa_ccl_filter_largest of csrc/ccl_bytes.hip) and k_erode_axis /
boa_fill_holes_2d / boa_binary_dilate_cross / boa_mask_assign / boa_label_overlay of csrc/morph.hip, on the masks of
tests/morph_cases.py: component tables at capacity, ties whose raster order is not the tile order, a first voxel handed over from a
later tile, 64 roots per wave, full tiles among mixed ones, long chains, baffled corridors of more than 256 rows, slices too large
for the LDS flood, volumes smaller than the size threshold, pinhole erosions that leave half the volume, reaches of +-31 on bits and of
32 on bytes.  Everything is integer work: every comparison is bit-exact.  References: scipy.ndimage and tests/floodfill.py (pinned
against each other, case by case, in tests/test_morph_cases_cpu.py), oracle.bca, oracle.measurements."""
import ctypes as C

import numpy as np
import pytest

import morph_cases as MC
from test_gpu_bits_morph import _pack, _unpack, ctx  # noqa: F401  (ctx: the module-scoped device context fixture)

pytestmark = pytest.mark.gpu


def _check(rc, what=""):
    from boa_hip._lib import check
    check(rc, what)


# ---- connected components: bit path ----------------------------------------------------------------------------------------------
def _bits_remove_small(ctx, masks, max_size, invert):
    shape = masks[0].shape
    d_bits, words = _pack(ctx, masks)
    _check(ctx.lib.boa_bits_remove_small(ctx.h, d_bits.vp, *shape, len(masks), max_size, invert), "boa_bits_remove_small")
    out = [_unpack(ctx, d_bits, words, shape, j) for j in range(len(masks))]
    d_bits.free()
    return out


def _seg_around(m):
    """label 3 on the mask, label 9 sprinkled around it (must stay untouched)"""
    rng = np.random.default_rng(int(m.sum()) % 1000)
    seg = m.astype(np.uint8) * 3
    seg[~m] = (rng.random(m.shape)[~m] < 0.1) * 9
    return seg


def _bits_filter_largest(ctx, m, seg):
    d_seg = ctx.from_numpy(seg)
    d_bits, _ = _pack(ctx, [m])
    _check(ctx.lib.boa_bits_filter_largest(ctx.h, d_bits.vp, *m.shape, d_seg.vp, 255), "boa_bits_filter_largest")
    got = d_seg.download(m.shape, np.uint8)
    d_seg.free()
    d_bits.free()
    return got


@pytest.mark.parametrize("name", MC.CC_NAMES)
def test_cc_bit_path(ctx, name):
    """boa_bits_remove_small (objects and, inverted, holes) at the case's thresholds and boa_bits_filter_largest"""
    c = MC.cc_cases()[name]
    m = c["mask"]
    for t in c["thresholds"]:
        got, = _bits_remove_small(ctx, [m], t, 0)
        np.testing.assert_array_equal(got, MC.remove_small_ref(m, t), err_msg=f"{name} max_size {t}")
    for t in c["inv_thresholds"]:
        got, = _bits_remove_small(ctx, [m], t, 1)
        np.testing.assert_array_equal(got, ~MC.remove_small_ref(~m, t), err_msg=f"{name} inverted max_size {t}")
    seg = _seg_around(m)
    want = seg.copy()
    want[MC.largest_ref(m)] = 255
    got = _bits_filter_largest(ctx, m, seg)
    np.testing.assert_array_equal(got, want, err_msg=name)
    if c["keep"] is not None and c["n"] != 1:
        assert got.flat[c["keep"]] == 3 and (got == 255).any()


@pytest.mark.parametrize("name", MC.CC_NAMES)
def test_cc_byte_path(ctx, name):
    """boa_ccl26 roots / sizes / count against the flood fill, then boa_ccl_remove_small and boa_ccl_filter_largest"""
    c = MC.cc_cases()[name]
    m = c["mask"]
    shape, n = m.shape, m.size
    roots_ref, sizes_ref = MC.cc_flood(name)
    d_m = ctx.from_numpy(m.astype(np.uint8))
    d_roots, d_sizes = ctx.alloc(n * 4), ctx.alloc(n * 4)
    ncomp = C.c_int()
    _check(ctx.lib.boa_ccl26(ctx.h, d_m.vp, *shape, d_roots.vp, d_sizes.vp, C.byref(ncomp)), "boa_ccl26")
    roots = d_roots.download(shape, np.int32)
    sizes = d_sizes.download((n,), np.uint32)
    assert ncomp.value == len(sizes_ref)
    np.testing.assert_array_equal(roots, roots_ref)
    want_sizes = np.zeros(n, np.uint32)
    want_sizes[list(sizes_ref)] = list(sizes_ref.values())
    np.testing.assert_array_equal(sizes, want_sizes)
    for t in c["thresholds"]:
        d_w = ctx.from_numpy(m.astype(np.uint8))
        _check(ctx.lib.boa_ccl_remove_small(ctx.h, d_roots.vp, d_sizes.vp, n, t, d_w.vp), "boa_ccl_remove_small")
        np.testing.assert_array_equal(d_w.download(shape, np.uint8).astype(bool), MC.remove_small_ref(m, t), err_msg=f"{name} max_size {t}")
        d_w.free()
    seg = _seg_around(m)
    want = seg.copy()
    want[MC.largest_ref(m)] = 255
    d_seg = ctx.from_numpy(seg)
    _check(ctx.lib.boa_ccl_filter_largest(ctx.h, d_roots.vp, d_sizes.vp, n, d_seg.vp, 255), "boa_ccl_filter_largest")
    np.testing.assert_array_equal(d_seg.download(shape, np.uint8), want, err_msg=name)
    for b in (d_m, d_roots, d_sizes, d_seg):
        b.free()


@pytest.mark.parametrize("name", ["lattice0_32x32x64", "lattice1_32x32x64", "lattice0_33x35x70", "lattice1_33x35x70"])
def test_capacity_lattice_statements(ctx, name):
    """the four statements of the capacity lattice, spelled out: max_size 0 changes nothing, max_size 1 empties the mask, inverted with
    max_size = volume everything is filled, and of the all-tying components only the raster-first voxel survives filter_largest"""
    c = MC.cc_cases()[name]
    m = c["mask"]
    got, = _bits_remove_small(ctx, [m], 0, 0)
    np.testing.assert_array_equal(got, m)
    got, = _bits_remove_small(ctx, [m], 1, 0)
    assert not got.any()
    got, = _bits_remove_small(ctx, [m], m.size, 1)
    assert got.all()
    got, = _bits_remove_small(ctx, [m], m.size - int(m.sum()) - 1, 1)          # one below the (single) hole's size: nothing is filled
    np.testing.assert_array_equal(got, m)
    seg = m.astype(np.uint8) * 3
    out = _bits_filter_largest(ctx, m, seg)
    assert int((out == 3).sum()) == 1 and out.flat[c["keep"]] == 3 and int((out == 255).sum()) == c["n"] - 1


@pytest.mark.parametrize("invert", [0, 1])
def test_cc_batch_of_worst_cases(ctx, invert):
    """the six (32, 32, 64) cases as ONE batch: every mask has its own tables, several of them full"""
    names = [k for k in MC.CC_NAMES if MC.cc_cases()[k]["mask"].shape == (32, 32, 64)]
    assert len(names) == 6
    masks = [MC.cc_cases()[k]["mask"] for k in names]
    for t in (1, 33, 8192):
        got = _bits_remove_small(ctx, masks, t, invert)
        for k, m, g in zip(names, masks, got):
            want = ~MC.remove_small_ref(~m, t) if invert else MC.remove_small_ref(m, t)
            np.testing.assert_array_equal(g, want, err_msg=f"{k} max_size {t} invert {invert}")


# ---- contour fill ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("YX", MC.CORRIDOR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_corridor_fill_bits_bytes_and_product(ctx, YX, monkeypatch):
    """closed / open / blank / full / upside-down / mirrored corridor slices, two masks per batched call: boa_bits_fill_holes_2d,
    boa_fill_holes_2d and the product path (threshold 1: the component filters remove nothing) on both of its paths"""
    from boa_hip import bca
    from oracle import bca as obca
    masks = MC.corridor_batch(*YX)
    shape = masks[0].shape
    refs = [MC.fill_ref(v) for v in masks]
    assert ctx.lib.boa_bits_fill_supported(*YX) == 1
    d_in, words = _pack(ctx, masks)
    d_out = ctx.alloc(words * 4 * len(masks))
    _check(ctx.lib.boa_bits_fill_holes_2d(ctx.h, d_in.vp, *shape, len(masks), d_out.vp), "boa_bits_fill_holes_2d")
    for j, ref in enumerate(refs):
        np.testing.assert_array_equal(_unpack(ctx, d_out, words, shape, j), ref, err_msg=f"bits, mask {j}")
    d_in.free()
    d_out.free()
    n = masks[0].size
    d_i, d_t, d_o = ctx.alloc(n * 4), ctx.alloc(n), ctx.alloc(n)
    for j, (v, ref) in enumerate(zip(masks, refs)):
        d_m = ctx.from_numpy(v.astype(np.uint8) * 255)
        _check(ctx.lib.boa_fill_holes_2d(ctx.h, d_m.vp, *shape, d_i.vp, d_t.vp, d_o.vp), "boa_fill_holes_2d")
        np.testing.assert_array_equal(d_o.download(shape, np.uint8), ref.astype(np.uint8), err_msg=f"bytes, mask {j}")
        d_m.free()
    for b in (d_i, d_t, d_o):
        b.free()
    seg = masks[0].astype(np.uint8) * 4
    want = obca.remove_small_labeled_objects(seg, threshold=1)
    np.testing.assert_array_equal(want, refs[0].astype(np.uint8) * 4)
    monkeypatch.delenv("BOA_MORPH_BYTES", raising=False)
    np.testing.assert_array_equal(bca.postprocess_part_segmentation(ctx, seg, threshold=1), want)
    monkeypatch.setenv("BOA_MORPH_BYTES", "1")
    np.testing.assert_array_equal(bca.postprocess_part_segmentation(ctx, seg, threshold=1), want)


def test_slice_too_large_for_the_lds_flood(ctx, monkeypatch):
    """2048 x 300 slices: boa_bits_fill_supported is 0, the product function takes its byte path, whose contour fill runs uncropped
    by union-find for label 1 (two [Y][W] arrays exceed the LDS too) and cropped in LDS for the others"""
    from boa_hip import bca
    from oracle import bca as obca
    Z, Y, X = MC.BIG_SLICE
    assert ctx.lib.boa_bits_fill_supported(Y, X) == 0 and not MC.bits_fill_supported(Y, X)
    assert ctx.lib.boa_bits_fill_supported(1745, X) == 1 and ctx.lib.boa_bits_fill_supported(1746, X) == 0
    monkeypatch.delenv("BOA_MORPH_BYTES", raising=False)
    seg = MC.big_slice_labels()
    want = obca.remove_small_labeled_objects(seg, threshold=300)
    got = bca.postprocess_part_segmentation(ctx, seg, threshold=300)
    np.testing.assert_array_equal(got, want)
    assert (want != seg).any()
    # the byte fill itself on the whole slice (union-find over the background) and the bit fill's refusal
    m = seg == 1
    n = m.size
    d_m, d_i, d_t, d_o = ctx.from_numpy(m.astype(np.uint8)), ctx.alloc(n * 4), ctx.alloc(n), ctx.alloc(n)
    _check(ctx.lib.boa_fill_holes_2d(ctx.h, d_m.vp, Z, Y, X, d_i.vp, d_t.vp, d_o.vp), "boa_fill_holes_2d")
    np.testing.assert_array_equal(d_o.download(seg.shape, np.uint8), MC.fill_ref(m).astype(np.uint8))
    for b in (d_m, d_i, d_t, d_o):
        b.free()


def test_volume_smaller_than_threshold(ctx, monkeypatch):
    """fewer voxels than `threshold`: the oracle floods the volume with the largest PRESENT label; the device does the same with
    labels=None and with a list that names absent labels (which must not be applied)"""
    from boa_hip import bca
    from oracle import bca as obca
    monkeypatch.delenv("BOA_MORPH_BYTES", raising=False)
    seg = MC.small_volume_labels()
    want = obca.remove_small_labeled_objects(seg)
    assert (want == 5).all()                                                   # not vacuous: the complement of label 5 is "small"
    assert ctx.lib.boa_bits_fill_supported(*seg.shape[1:]) == 1
    d_seg = ctx.from_numpy(seg)
    for labels in (None, [1, 2, 5, 7]):
        d_out = bca.postprocess_part_segmentation_device(ctx, d_seg, seg.shape, labels=labels)
        np.testing.assert_array_equal(d_out.download(seg.shape, np.uint8), want, err_msg=f"labels {labels}")
        d_out.free()
    d_seg.free()


# ---- erosion ---------------------------------------------------------------------------------------------------------------------
def _erode(ctx, m8, k):
    shape, n = m8.shape, m8.size
    d_m = ctx.from_numpy(m8)
    d_o, d_t = ctx.from_numpy(np.full(n, 0xAA, np.uint8)), ctx.from_numpy(np.full(n, 0xAA, np.uint8))
    _check(ctx.lib.boa_binary_erode(ctx.h, d_m.vp, d_o.vp, d_t.vp, *shape, k), "boa_binary_erode")
    out = d_o.download(shape, np.uint8)
    for b in (d_m, d_o, d_t):
        b.free()
    return out


def _erode_bits(ctx, m8, lo, hi):
    shape, n = m8.shape, m8.size
    d_m, d_o = ctx.from_numpy(m8), ctx.from_numpy(np.full(n, 0xAA, np.uint8))
    _check(ctx.lib.boa_bits_erode_u8(ctx.h, d_m.vp, d_o.vp, *shape, lo, hi), "boa_bits_erode_u8")
    out = d_o.download(shape, np.uint8)
    d_m.free()
    d_o.free()
    return out


def _bytes_of(m, seed):
    """uint8 mask whose set voxels carry 1, 2, 128 or 255 (every non-zero byte counts as set)"""
    return (m * np.random.default_rng(seed).choice(np.array([1, 2, 128, 255], np.uint8), size=m.shape)).astype(np.uint8)


@pytest.mark.parametrize("X", MC.PINHOLE_X)
def test_pinhole_erosion(ctx, X):
    """k^3 erosion, k = 1 .. 9, of solid volumes with pinholes (also at x = 0, 31, 32, X - 1 and on the first / last y and z) dense
    enough that 20 .. 80 % of the voxels survive, against oracle.measurements.erode_region; boa_bits_erode_u8 directly as well"""
    from oracle import measurements as OM
    for k in MC.PINHOLE_K:
        m = MC.pinhole_mask(X, k)
        want = OM.erode_region(m, k)
        assert 0.2 <= float(want.mean()) <= 0.8
        m8 = _bytes_of(m, k)
        np.testing.assert_array_equal(_erode(ctx, m8, k), want.astype(np.uint8), err_msg=f"X {X} k {k}")
        np.testing.assert_array_equal(_erode_bits(ctx, m8, *MC.erode_reach(k)), want.astype(np.uint8), err_msg=f"X {X} k {k} (bits)")


@pytest.mark.parametrize("X", MC.ASYM_X)
def test_asymmetric_reaches_on_bits(ctx, X):
    """boa_bits_erode_u8 with one-sided and full reaches of 31 on rows of 1, 2 and 4 words"""
    m = MC.asym_mask(X)
    m8 = _bytes_of(m, X)
    for lo, hi in MC.ASYM_REACHES:
        want = MC.erode_box_ref(m, lo, hi)
        np.testing.assert_array_equal(_erode_bits(ctx, m8, lo, hi), want.astype(np.uint8), err_msg=f"X {X} reach {lo, hi}")


def _erode_with_path(ctx, m8, k):
    """(result, "bits" | "bytes"): the aggregation class books 2 bytes per voxel for the bit form and 6 for the three byte passes"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = _erode(ctx, m8, k)
        booked = ctx.prof_get()["aggregation"]
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    assert booked["launches"] == 1
    per_voxel = booked["bytes"] / m8.size
    assert per_voxel in (2.0, 6.0), per_voxel
    return out, "bits" if per_voxel == 2.0 else "bytes"


@pytest.mark.parametrize("shape", MC.BYTE_SHAPES + MC.BYTE_THIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_erosion_reaches_of_32_run_on_bytes(ctx, shape):
    """k = 63 is the last footprint of the bit form, k = 64 and 65 (reaches -32 .. 31 / 32) are k_erode_axis.  Reference: the oracle on
    the thin volumes (scipy's erosion with a 65^3 structure costs half a minute on the others), erode_box_ref -- pinned against the
    oracle on the CPU -- everywhere."""
    from oracle import measurements as OM
    m = MC.byte_mask(shape)
    m8 = _bytes_of(m, sum(shape))
    for k in MC.BYTE_K:
        lo, hi = MC.erode_reach(k)
        got, path = _erode_with_path(ctx, m8, k)
        assert path == ("bits" if MC.erode_on_bits(lo, hi) else "bytes"), k
        assert path == ("bits" if k == 63 else "bytes")
        want = MC.erode_box_ref(m, lo, hi)
        assert want.any()
        np.testing.assert_array_equal(got, want.astype(np.uint8), err_msg=f"{shape} k {k}")
        if shape in MC.BYTE_THIN_SHAPES:
            np.testing.assert_array_equal(got, OM.erode_region(m, k).astype(np.uint8), err_msg=f"{shape} k {k} (oracle)")


# ---- dilation and the assign kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MC.DILATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dilate_cross_vs_scipy(ctx, shape):
    """scipy.ndimage.binary_dilation(mask, iterations=it) for odd and even it; dev_out and dev_tmp hold 0xAA beforehand, so a result
    left in the wrong buffer of the ping-pong shows"""
    from scipy import ndimage
    from boa_hip._lib import BOA_EINVAL
    n = int(np.prod(shape))
    for name, m in MC.dilate_masks(shape).items():
        d_m = ctx.from_numpy(m.astype(np.uint8) * 3)
        for it in MC.DILATE_ITERATIONS:
            d_o, d_t = ctx.from_numpy(np.full(n, 0xAA, np.uint8)), ctx.from_numpy(np.full(n, 0xAA, np.uint8))
            _check(ctx.lib.boa_binary_dilate_cross(ctx.h, d_m.vp, d_o.vp, d_t.vp, *shape, it), "boa_binary_dilate_cross")
            want = ndimage.binary_dilation(m, iterations=it).astype(np.uint8)
            np.testing.assert_array_equal(d_o.download(shape, np.uint8), want, err_msg=f"{name} iterations {it}")
            np.testing.assert_array_equal(d_m.download(shape, np.uint8), m.astype(np.uint8) * 3)      # the input is left alone
            d_o.free()
            d_t.free()
        d_m.free()
    m = MC.dilate_masks(shape)["corners"]
    d_m, d_o, d_t = ctx.from_numpy(m.astype(np.uint8)), ctx.alloc(n), ctx.alloc(n)
    assert ctx.lib.boa_binary_dilate_cross(ctx.h, d_m.vp, d_o.vp, d_t.vp, *shape, 0) == BOA_EINVAL
    for b in (d_m, d_o, d_t):
        b.free()


@pytest.mark.parametrize("n", MC.ASSIGN_N)
def test_mask_assign_and_label_overlay(ctx, n):
    """out[(mask != 0) != invert] = value and out[part != 0] = part: mask bytes 1 / 2 / 255 count as set, every other element keeps
    its previous content, n around the workgroup size and one large odd n"""
    mask, prev, part = MC.assign_inputs(n)
    d_mask, d_part = ctx.from_numpy(mask), ctx.from_numpy(part)
    for invert in (0, 1):
        d_out = ctx.from_numpy(prev)
        _check(ctx.lib.boa_mask_assign(ctx.h, d_mask.vp, n, invert, 77, d_out.vp), "boa_mask_assign")
        want = prev.copy()
        want[(mask != 0) != bool(invert)] = 77
        np.testing.assert_array_equal(d_out.download((n,), np.uint8), want, err_msg=f"invert {invert}")
        d_out.free()
    d_out = ctx.from_numpy(prev)
    _check(ctx.lib.boa_label_overlay(ctx.h, d_part.vp, n, d_out.vp), "boa_label_overlay")
    want = np.where(part != 0, part, prev)
    np.testing.assert_array_equal(d_out.download((n,), np.uint8), want)
    np.testing.assert_array_equal(d_mask.download((n,), np.uint8), mask)
    for b in (d_mask, d_part, d_out):
        b.free()
