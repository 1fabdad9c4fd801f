"""Pins tests/remap_cases.py, the numpy side of tests/test_gpu_index_remap.py: every case lands on the kernel it is named for by the
mirrored path rules, addresses nothing outside its buffers, and feeds numpy only conversions whose result is defined.  No device."""
import warnings

import numpy as np
import pytest

import remap_cases as RC

I16, I32, U8, F32, F64 = np.int16, np.int32, np.uint8, np.float32, np.float64


# ---- the mirrored rules ----------------------------------------------------------------------------------------------------------
def test_copy3_rule_on_hand_written_geometries():
    """the rule itself, on geometries written out by hand: contiguous output, input contiguous along axis 1 / axis 0, thresholds"""
    T = RC.copy3_axis
    assert T((3, 17, 33), (561, 1, 17), (561, 33, 1)) == 1
    assert T((17, 3, 33), (1, 17, 51), (99, 33, 1)) == 0
    assert T((3, 16, 16), (256, 1, 16), (256, 16, 1)) == 1 and T((3, 15, 16), (240, 1, 15), (240, 16, 1)) is None
    assert T((3, 16, 15), (240, 1, 16), (240, 15, 1)) is None
    assert T((3, 17, 33), (561, -1, 17), (561, 33, -1)) == 1                       # the sign of a unit stride does not matter
    assert T((3, 17, 33), (561, 1, 17), (1122, 66, 2)) is None                     # output not contiguous along axis 2
    assert T((3, 17, 33), (561, 33, 1), (561, 33, 1)) is None                      # plain copy
    assert T((17, 18, 33), (1, 1, 40), (594, 33, 1)) == 1                          # axis 1 before axis 0
    assert T((17, 15, 33), (1, 1, 40), (495, 33, 1)) == 0                          # ... unless it is too short
    assert T((16, 65535, 16), (1, 16, 16 * 65535), (16 * 65535, 16, 1)) == 0       # batch extent = blockIdx.z
    assert T((16, 65536, 16), (1, 16, 16 * 65536), (16 * 65536, 16, 1)) is None
    assert T((16, 1, 64 * 65535), (1, 16, 16), (64 * 65535, 64 * 65535, 1)) == 0   # tiles along axis 2 = blockIdx.y
    assert T((16, 1, 64 * 65535 + 1), (1, 16, 16), (64 * 65535 + 1, 64 * 65535 + 1, 1)) is None
    assert T((0, 17, 33), (561, 1, 17), (561, 33, 1)) is None                      # nothing is launched
    assert RC.copy3_transposed((3, 17, 33), (561, 1, 17), (561, 33, 1)) and not RC.copy3_transposed((3, 5, 7), (35, 1, 5), (35, 7, 1))


def test_bbox_rule_on_hand_written_geometries():
    V = RC.bbox_vectorised
    assert V((4, 5, 16), 1, 0) and V((4, 5, 8), 2, 0) and V((4, 5, 4), 4, 0) and V((4, 5, 12), 4, 32)
    assert not V((4, 5, 17), 1, 0) and not V((4, 5, 34), 2, 0) and not V((4, 5, 17), 4, 0)     # (20, 33, 17): the older tests' shape
    assert not V((4, 5, 16), 1, 5) and not V((4, 5, 4), 4, 4) and not V((0, 5, 16), 1, 0)


def test_counter_names_keep_their_indices():
    from boa_hip import _lib
    assert _lib.CNT_NAMES[:10] == ["head_mfma", "head_valu", "conv_ws", "conv_simple", "first_mfma", "first_valu", "f32", "conv_x3", "x3",
                                   "head_gather"]
    assert _lib.CNT_NAMES[10:] == ["copy_t", "bbox_vec", "finalize_vec8"]


# ---- boa_copy3: the view cases ---------------------------------------------------------------------------------------------------
def check_case(c):
    """what holds for every copy case: the named path by the mirrored rule; every address inside the buffers; the destination view
    addresses no element twice; the destination starts as 0xAA; the stored geometry is the numpy view the case was built from"""
    shape, n = c["shape"], int(np.prod(c["shape"]))
    assert n > 0 and c["src"].ndim == c["dst"].ndim == 1
    assert RC.copy3_axis(shape, c["in_strides"], c["out_strides"]) == c["axis"]
    lo, hi = RC.address_range(c["in_off"], shape, c["in_strides"])
    assert 0 <= lo <= hi < c["src"].size, (lo, hi, c["src"].size)
    lo, hi = RC.address_range(c["out_off"], shape, c["out_strides"])
    assert 0 <= lo <= hi < c["dst"].size, (lo, hi, c["dst"].size)
    assert (c["dst"].view(np.uint8) == 0xAA).all()
    if n <= 1 << 20:
        idx = c["out_off"] + sum(np.arange(d).reshape([-1 if k == a else 1 for k in range(3)]) * s
                                 for a, (d, s) in enumerate(zip(shape, c["out_strides"])))
        assert np.unique(idx).size == n                                        # no two outputs share an address
    if c["src_ops"] is not None:
        from boa_hip.devarray import DevArray
        for which, ops, base_shape, off, strides in (("src", c["src_ops"], c["src_base_shape"], c["in_off"], c["in_strides"]),
                                                     ("dst", c["dst_ops"], c["dst_base_shape"], c["out_off"], c["out_strides"])):
            base = c[which].reshape(base_shape)
            v = RC.apply_ops(base, ops)
            assert RC.geometry(base, v) == (off, strides) and v.shape == shape
            assert np.array_equal(RC.bits(RC.view_of(c[which], off, shape, strides)), RC.bits(v))
            # DevArray's view arithmetic (host-side metadata only) gives the same offset and strides as numpy's
            d = DevArray(None, None, base_shape, base.dtype)
            for op in ops:
                d = getattr(d, op[0])(*op[1:])
            assert (d.offset, d.strides, d.shape) == (off, strides, shape), (which, ops)


def test_case_list_is_complete():
    assert tuple(RC.copy_cases()) == RC.COPY_NAMES and len(set(RC.COPY_NAMES)) == len(RC.COPY_NAMES)


@pytest.mark.parametrize("name", RC.COPY_NAMES)
def test_copy_case_facts(name):
    c = RC.copy_cases()[name]
    check_case(c)
    if name.startswith("outside_"):
        assert c["axis"] is None
    elif name[-3:-1] == "_A":
        assert c["axis"] == int(name[-1])
    elif name.startswith("tiles_A"):
        assert c["axis"] == int(name[7])
    else:
        assert c["axis"] == 1                                                  # priority_*: both qualify, axis 1 is taken
    want = RC.expected_dst(c)
    changed = RC.bits(want) != RC.bits(c["dst"])
    inside = np.zeros(c["dst"].size, bool)
    RC.view_of(inside, c["out_off"], c["shape"], c["out_strides"])[...] = True
    assert not (changed & ~inside).any() and changed.sum() >= 0.99 * inside.sum()   # (a value may happen to equal the 0xAA pattern)
    assert inside.sum() == np.prod(c["shape"])


def test_tile_cases_cover_full_partial_and_single_tiles():
    for A in (1, 0):
        ext = [(dA, d2) for dA, d2, _ in RC.T_PAIRS]
        assert (16, 16) in ext                                                   # a single tile of 16 x 16
        assert (64, 64) in ext                                                   # exactly one full tile, no partial one
        assert any(dA > 64 and dA % 64 for dA, _ in ext) and any(d2 > 64 and d2 % 64 for _, d2 in ext)   # full + partial, each side
        assert any(dA < 64 for dA, _ in ext) and any(d2 < 64 for _, d2 in ext)
        assert {x for p in ext for x in p} == {16, 17, 63, 64, 65, 130} and {dC for _, _, dC in RC.T_PAIRS} == {1, 3}
        for dA, d2, dC in RC.T_PAIRS:
            c = RC.copy_cases()[f"tiles_A{A}_{dA}x{d2}x{dC}"]
            assert c["shape"] == RC.out_shape(A, dA, d2, dC) and c["shape"][A] == dA and c["shape"][2] == d2
            assert abs(c["in_strides"][A]) == 1 and c["out_strides"][2] == 1


def test_sign_cases_have_the_signs_they_name():
    cs = RC.copy_cases()
    for A in (1, 0):
        C = 1 - A
        c = cs[f"flipped_source_A{A}"]
        assert c["in_strides"][A] == -1 and c["out_strides"][2] == 1
        c = cs[f"flipped_destination_A{A}"]
        assert c["in_strides"][A] == 1 and c["out_strides"][2] == -1
        c = cs[f"negative_outer_strides_A{A}"]
        assert c["in_strides"][A] == 1 and c["in_strides"][2] < -1 and (c["in_strides"][C] < -1)
        assert c["out_strides"][2] == 1 and c["out_strides"][A] < -1 and c["out_strides"][C] < -1
        c = cs[f"all_flipped_A{A}"]
        assert c["in_strides"][A] == -1 and c["out_strides"][2] == -1 and all(s < 0 for s in c["in_strides"] + c["out_strides"])


def test_box_cases_touch_the_ends_they_name():
    cs = RC.copy_cases()
    for A in (1, 0):
        for name, first, last in ((f"box_inner_A{A}", False, False), (f"box_last_A{A}", False, True), (f"box_first_A{A}", True, False)):
            c = cs[name]
            for off, strides, buf in ((c["in_off"], c["in_strides"], c["src"]), (c["out_off"], c["out_strides"], c["dst"])):
                lo, hi = RC.address_range(off, c["shape"], strides)
                assert off != 0 and (lo == 0) == first and (hi == buf.size - 1) == last, (name, off, lo, hi)
            # row pitches larger than the extents: the stride of the axis above the contiguous one exceeds its extent
            assert abs(c["out_strides"][1]) > c["shape"][2]
            assert sorted(abs(s) for s in c["in_strides"])[1] > c["shape"][A]
        assert cs[f"box_inner_A{A}"]["dst"].dtype == I32 and cs[f"box_inner_A{A}"]["src"].dtype == I16


def test_priority_and_broadcast_cases():
    cs = RC.copy_cases()
    for name in ("priority_both_unit", "priority_unit_and_minus_unit"):
        c = cs[name]
        assert abs(c["in_strides"][0]) == abs(c["in_strides"][1]) == 1 and min(c["shape"]) >= 16          # both axes qualify
        lo, hi = RC.address_range(c["in_off"], c["shape"], c["in_strides"])
        assert (lo, hi) == (0, c["src"].size - 1)
    assert cs["broadcast_batch_A1"]["in_strides"][0] == 0 and cs["broadcast_batch_A0"]["in_strides"][1] == 0
    c = cs["broadcast_axis1_of_16_A0"]
    assert c["in_strides"][1] == 0 and c["shape"][1] >= 16 and c["axis"] == 0


def test_outside_cases_miss_the_rule_by_one_condition():
    """each fallback case differs from a transposed one in exactly the named condition"""
    cs = RC.copy_cases()
    for A in (1, 0):
        c = cs[f"outside_15_on_A_A{A}"]
        assert c["shape"][A] == 15 and c["shape"][2] >= 16 and abs(c["in_strides"][A]) == 1 and c["out_strides"][2] == 1
        grown = list(c["shape"])
        grown[A] = 16
        assert RC.copy3_axis(grown, c["in_strides"], c["out_strides"]) == A
        c = cs[f"outside_15_on_axis2_A{A}"]
        assert c["shape"][2] == 15 and c["shape"][A] >= 16 and abs(c["in_strides"][A]) == 1 and c["out_strides"][2] == 1
        assert RC.copy3_axis(c["shape"][:2] + (16,), c["in_strides"], c["out_strides"]) == A
        c = cs[f"outside_out_stride_2_A{A}"]
        assert c["out_strides"][2] == 2 and RC.copy3_axis(c["shape"], c["in_strides"], c["out_strides"][:2] + (1,)) == A
    c = cs["outside_plain_copy"]
    assert c["in_strides"][2] == 1 and c["out_strides"][2] == 1 and min(c["shape"][1:]) >= 16


@pytest.mark.parametrize("batch", RC.GRID_BATCHES + RC.GRID_TILE_ROWS)
def test_grid_limit_cases(batch):
    c = RC.grid_limit_case(batch)
    check_case(c)
    assert c["src"].dtype == U8 and c["dst"].dtype == U8
    if batch in RC.GRID_BATCHES:
        assert c["shape"] == (16, batch, 16) and c["src"].nbytes <= 16 << 20
        assert (c["axis"] is None) == (batch > 65535) and {65535, 65536} == set(RC.GRID_BATCHES)
    else:
        assert c["shape"] == (16, 1, batch) and (c["axis"] is None) == (-(-batch // 64) > 65535)
        assert {-(-b // 64) for b in RC.GRID_TILE_ROWS} == {65535, 65536}


# ---- boa_copy3: the dtype matrix -------------------------------------------------------------------------------------------------
PAIRS = [(i, o) for i in RC.DTYPES for o in RC.DTYPES]


def test_matrix_runs_every_pair_through_both_kernels():
    """25 pairs x {k_copy3_t, k_copy3} by the mirrored rule"""
    assert len(PAIRS) == 25
    ran = set()
    for kernel in ("t", "e"):
        for i, o in PAIRS:
            c = RC.matrix_case(kernel, i, o)
            check_case(c)
            assert c["shape"] == RC.MATRIX_SHAPES[kernel] and c["src"].dtype == i and c["dst"].dtype == o
            ran.add(("k_copy3_t" if RC.copy3_transposed(c["shape"], c["in_strides"], c["out_strides"]) else "k_copy3", i.name, o.name))
    assert len(ran) == 50 and sum(k == "k_copy3_t" for k, _, _ in ran) == 25


@pytest.mark.parametrize("kernel", ["t", "e"])
def test_matrix_conversions_are_defined_and_silent(kernel):
    """no float -> int conversion sees NaN, an infinity or a value outside the target range (undefined in C++, platform-dependent in
    numpy): by the generators' own rule and by numpy's, which warns about such casts"""
    n = int(np.prod(RC.MATRIX_SHAPES[kernel]))
    for i, o in PAIRS:
        v = RC.matrix_values(i, o, n)
        assert v.dtype == i and v.size == n
        assert RC.conversion_defined(v, o), (i, o)
        if i.kind == "f" and o.kind in "iu":
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                got = v.astype(o)
            np.testing.assert_array_equal(got, np.trunc(v.astype(F64)).astype(np.int64))          # truncation toward zero, in range
            frac = v.astype(F64) != np.trunc(v.astype(F64))
            assert frac.sum() > n // 4 and (v[frac] > 0).any() and ((v[frac] < 0).any() or o == U8)
            if o == U8:
                assert not np.signbit(v).any()


def test_conversion_defined_rejects_what_it_should():
    for bad in (np.nan, np.inf, -np.inf, 255.0, 256.0, -1.0, -0.0, 300.5):
        assert not RC.conversion_defined(np.array([1.5, bad], F32), U8), bad
    for bad in (np.nan, 32767.0, 32768.5, -32768.0, -40000.0):
        assert not RC.conversion_defined(np.array([1.5, bad], F64), I16), bad
    for bad in (np.nan, 2147483647.0, 2147483648.0, -2147483648.0, 1e10):
        assert not RC.conversion_defined(np.array([1.5, bad], F64), I32), bad
    assert RC.conversion_defined(np.array([0.0, 254.999], F32), U8) and RC.conversion_defined(np.array([-32767.5, 32766.5]), I16)
    assert RC.conversion_defined(np.array([np.nan, np.inf]), F32) and RC.conversion_defined(np.array([70000], I32), I16)


def test_matrix_special_values_pin_numpy():
    """the conversions the special values are there for, as numpy performs them (the GPU must give the same bits)"""
    def conv(i, o, values):
        v = RC.matrix_values(i, o, 105)
        for x in values:
            assert (v == np.array(x, i)).any(), (i, o, x)                      # the generator holds the value
        with np.errstate(all="ignore"):
            return np.array(values, i).astype(o)

    np.testing.assert_array_equal(conv(RC.DTYPES[2], RC.DTYPES[1], [70000, -70000, 32768, -32769, 65536]), [4464, -4464, -32768, 32767, 0])
    np.testing.assert_array_equal(conv(RC.DTYPES[1], RC.DTYPES[0], [-1, 256, 255, -129, -256]), [255, 0, 255, 127, 0])
    np.testing.assert_array_equal(conv(RC.DTYPES[2], RC.DTYPES[0], [-1, 256, 70000]), [255, 0, 70000 % 256])
    np.testing.assert_array_equal(conv(RC.DTYPES[0], RC.DTYPES[1], [255, 128]), [255, 128])                    # no sign extension
    # int32 -> float32 rounds to nearest even; -> float64 is exact
    got = conv(RC.DTYPES[2], RC.DTYPES[3], [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, 2 ** 31 - 64, 2 ** 31 - 65, -(2 ** 24 + 1)])
    np.testing.assert_array_equal(got.astype(F64), [2 ** 24, 2 ** 24 + 4, 2 ** 31, 2 ** 31, 2 ** 31 - 128, -(2 ** 24)])
    np.testing.assert_array_equal(conv(RC.DTYPES[2], RC.DTYPES[4], [2 ** 24 + 1, 2 ** 31 - 1, -2 ** 31]), [2 ** 24 + 1, 2 ** 31 - 1, -2 ** 31])
    # float64 -> float32: ties to even, subnormal results, overflow to inf, signed zeros, NaN
    u = 2.0 ** -24
    got = conv(RC.DTYPES[4], RC.DTYPES[3], [1 + u, 1 + 3 * u, 1 + u + 2.0 ** -50, 1e-40, 2.0 ** -150, 1.5 * 2.0 ** -150, 3.5e38, -1e300,
                                           (2 - 2.0 ** -24) * 2.0 ** 127, RC.F32_MAX])
    assert got[0] == 1.0 and got[1] == F32(1 + 4 * u) and got[2] == F32(1 + 2 * u)
    assert 0 < got[3] < np.finfo(F32).tiny and got[4] == 0 and got[5] == F32(2.0 ** -149)
    assert got[6] == np.inf and got[7] == -np.inf and got[8] == np.inf and got[9] == np.finfo(F32).max
    v = RC.matrix_values(F64, F32, 105)
    assert np.isnan(v).any() and np.isinf(v).sum() >= 2 and (RC.bits(v) == 1 << 63).any() and (RC.bits(v) == 0).any()
    # same dtype: NaN payloads, signalling NaNs, both zeros and subnormals are among the values, and numpy passes their bits on
    for dt, pats in ((RC.DTYPES[3], [0x7FC12345, 0x7F800001, 0x80000000, 0x00000001]),
                     (RC.DTYPES[4], [0x7FF8000012345678, 0x7FF0000000000001, 0x8000000000000000, 0x0000000000000001])):
        v = RC.matrix_values(dt, dt, 105)
        assert np.isin(np.array(pats, RC.bits(v).dtype), RC.bits(v)).all()
        assert np.array_equal(RC.bits(v.astype(dt)), RC.bits(v))
    # converting NaNs are the canonical quiet NaN only (payload propagation across widths is the hardware's business)
    for i, o in ((RC.DTYPES[3], RC.DTYPES[4]), (RC.DTYPES[4], RC.DTYPES[3])):
        v = RC.matrix_values(i, o, 1683)
        nan = v[np.isnan(v)]
        assert nan.size >= 1 and (RC.bits(nan) == RC.bits(np.array([np.nan], i))[0]).all()


# ---- boa_nonzero_bbox ------------------------------------------------------------------------------------------------------------
def ref_bbox(vol):
    from boa_hip.task import nonzero_bbox
    return nonzero_bbox(vol)


@pytest.mark.parametrize("dtype", RC.BBOX_DTYPES, ids=lambda d: d.name)
def test_bbox_row_lengths_take_both_loops(dtype):
    isz = dtype.itemsize
    rows = RC.bbox_row_lengths(dtype)
    assert [d2 * isz for d2, vec in rows if vec] == [16, 32, 48, 1040]
    assert [d2 * isz for d2, vec in rows if not vec] == [16 - isz, 16 + isz, 1040 - isz, 1040 + isz]
    assert 1040 // 16 > 64 and (1040 - isz) // isz > 64                         # a lane takes a second chunk / a second element
    lead = RC.BBOX_LEAD[isz]
    assert (lead * isz) % 16 != 0
    loops = set()
    for d2, vec in rows:
        shape = (RC.D0, RC.D1, d2)
        assert RC.bbox_vectorised(shape, isz, 0) == vec
        assert not RC.bbox_vectorised(shape, isz, lead * isz)                   # a vectorisable shape at a misaligned address
        loops |= {vec, False}
    assert loops == {True, False}


@pytest.mark.parametrize("dtype", RC.BBOX_DTYPES, ids=lambda d: d.name)
def test_bbox_patterns_have_the_boxes_they_are_built_for(dtype):
    E = 16 // dtype.itemsize
    shapes = [(RC.D0, RC.D1, d2) for d2, _ in RC.bbox_row_lengths(dtype)] + RC.bbox_degenerate_shapes(dtype)
    for shape in shapes:
        full = [[0, n] for n in shape]
        pats = RC.bbox_patterns(shape, dtype)
        assert all(v.shape == shape and v.dtype == dtype and v.flags.c_contiguous for v in pats.values())
        assert ref_bbox(pats["zeros"]) == full and not pats["zeros"].any()
        corners = set()
        for name, v in pats.items():
            if name.startswith("corner_") or name.startswith("chunk_") or name == "last_chunk_of_row":
                pos = np.argwhere(v != 0)
                assert len(pos) == 1
                assert ref_bbox(v) == [[int(p), int(p) + 1] for p in pos[0]]
                if name.startswith("corner_"):
                    corners.add(tuple(int(p) for p in pos[0]))
                    assert all(p in (0, n - 1) for p, n in zip(pos[0], shape))
        assert len(corners) == len({(z, y, x) for z in (0, shape[0] - 1) for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)})
        if shape[2] >= 2 * E:
            x0 = int(np.argwhere(pats["chunk_first_element"])[0][2])
            x1 = int(np.argwhere(pats["chunk_last_element"])[0][2])
            assert x0 % E == 0 and x1 % E == E - 1 and x0 // E == x1 // E
        if shape[2] % E == 0:
            assert int(np.argwhere(pats["last_chunk_of_row"])[0][2]) // E == shape[2] // E - 1
        for ax in range(3):
            v = pats[f"lo_hi_axis{ax}"]
            pos = np.argwhere(v != 0)
            assert len(pos) == (2 if shape[ax] > 1 else 1)
            bb = ref_bbox(v)
            assert bb[ax] == [int(pos[:, ax].min()), int(pos[:, ax].max()) + 1]
            for p in pos:                                                          # each voxel alone decides one end
                w = v.copy()
                w[tuple(p)] = 0
                assert ref_bbox(w) != bb
        v = pats["only_negative"]
        assert v.any() and ((v[v != 0].astype(np.int64) < 0).all() if dtype != U8 else (v[v != 0] >= 128).all()) and ref_bbox(v) != full
        if dtype == F32:
            v = pats["all_negative_zero"]
            assert (RC.bits(v) == 0x80000000).all() and ref_bbox(v) == full
            v = pats["negative_zero_around_a_value"]
            pos = np.argwhere(v != 0)
            assert len(pos) == 1 and (RC.bits(v) != 0).all() and ref_bbox(v) == [[int(p), int(p) + 1] for p in pos[0]]
            v = pats["nan_is_nonzero"]
            pos = np.argwhere(np.isnan(v))
            assert len(pos) == 1 and ref_bbox(v) == [[int(p), int(p) + 1] for p in pos[0]] and (RC.bits(v) == 0x80000000).any()
            v = pats["subnormal_is_nonzero"]
            assert RC.bits(v).max() == 1 and ref_bbox(v) == [[shape[0] - 1, shape[0]], [0, 1], [shape[2] - 1, shape[2]]]


@pytest.mark.parametrize("dtype", RC.BBOX_DTYPES, ids=lambda d: d.name)
def test_bbox_embedding_stays_inside_its_buffer(dtype):
    vol = RC.bbox_patterns((RC.D0, RC.D1, 16 // dtype.itemsize), dtype)["corner_111"]
    for lead in (0, RC.BBOX_LEAD[dtype.itemsize]):
        flat, off = RC.bbox_embed(vol, lead)
        assert off == lead and flat.dtype == dtype and flat.size == lead + vol.size + RC.BBOX_GUARD
        assert 0 <= off and off + vol.size <= flat.size                         # first and last voxel inside the buffer
        assert np.array_equal(flat[off:off + vol.size], vol.reshape(-1))
        assert (flat[:off] != 0).all() and (flat[off + vol.size:] != 0).all()   # a read outside the volume would widen the box
        assert (lead * dtype.itemsize) % dtype.itemsize == 0


@pytest.mark.parametrize("cu_count", [64, 256, 304])
def test_bbox_sweep_case_needs_the_second_sweep(cu_count):
    for dtype in RC.BBOX_DTYPES:
        vol, f = RC.bbox_sweep_case(dtype, cu_count)
        d0, d1, d2 = vol.shape
        assert d2 == 16 and f["rows"] == d0 * d1 > 2 * 32 * cu_count and f["sweep"] == 32 * cu_count
        assert RC.bbox_vectorised(vol.shape, dtype.itemsize, 0) and vol.nbytes <= 4 << 20
        rows = {k: p[0] * d1 + p[1] for k, p in f["voxels"].items()}
        assert rows["first_row"] == 0 and rows["last_row"] == f["rows"] - 1
        assert all(f["sweep"] <= rows[k] < 2 * f["sweep"] for k in ("second_sweep_lo2", "second_sweep_hi2"))
        assert int((vol != 0).sum()) == 4 and ref_bbox(vol) == f["bbox"] != [[0, d0], [0, d1], [0, d2]]
        for p in f["voxels"].values():                                            # every one of the four decides
            w = vol.copy()
            w[p] = 0
            assert ref_bbox(w) != f["bbox"]
        first_sweep_only = vol.copy().reshape(-1, d2)
        first_sweep_only[f["sweep"]:] = 0
        assert ref_bbox(first_sweep_only.reshape(vol.shape)) != f["bbox"]         # a kernel without the row stride loop


def test_bbox_degenerate_shapes():
    for dtype in RC.BBOX_DTYPES:
        shapes = RC.bbox_degenerate_shapes(dtype)
        assert any(s[1] == 1 and s[0] > 1 for s in shapes) and any(s[0] == 1 and s[1] > 1 for s in shapes)
        assert all(s[2] * dtype.itemsize == 48 for s in shapes)


def test_every_bbox_instantiation_is_reached():
    """four dtypes x {vector loop, per-element loop} by the mirrored rule, over the shapes and leads the GPU test runs"""
    ran = set()
    for dtype in RC.BBOX_DTYPES:
        isz = dtype.itemsize
        for d2, _ in RC.bbox_row_lengths(dtype):
            for lead in (0, RC.BBOX_LEAD[isz]):
                ran.add((dtype.name, RC.bbox_vectorised((RC.D0, RC.D1, d2), isz, lead * isz)))
    assert ran == {(d.name, v) for d in RC.BBOX_DTYPES for v in (True, False)}
